"""CPU: the T2-MI reference (tests/t2mi_ref.py) that the GPU deframer is compared with -- its CRC-32 against the
known check value, the kernel's table / combine formulation against the bitwise CRC, encapsulate -> parse round
trips, hand-derived counter values for every malformation of tests/t2mi_cases.py, and the resume property."""
import numpy as np
import pytest

import t2mi_cases as C
import t2mi_ref as R

ZERO = dict.fromkeys(R.TS_COUNTERS + R.PKT_COUNTERS, 0)


def test_crc32_check_value():
    assert R.crc32_bitwise(b"123456789") == 0x0376E6E7
    assert R.crc32_table(b"123456789") == 0x0376E6E7
    assert R.crc32_combine(b"123456789") == 0x0376E6E7


def test_table_and_combine_match_bitwise_on_every_length_to_300():
    rng = np.random.default_rng(3)
    for n in range(301):
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        want = R.crc32_bitwise(d)
        assert R.crc32_table(d) == want, n
        assert R.crc32_combine(d) == want, n
    d = rng.integers(0, 256, 8202, dtype=np.uint8).tobytes()     # the longest T2-MI packet
    assert R.crc32_combine(d) == R.crc32_bitwise(d)
    assert R.crc32_combine(d + R.crc32_bitwise(d).to_bytes(4, "big")) == 0


def test_xpow_is_multiplication_by_x8():
    for n in (0, 1, 2, 63, 64, 129, 8202):
        assert R.gf_mul(R.xpow8(n), 0x100) == R.xpow8(n + 1)
        assert R.crc32_table(bytes(n), 1) == R.xpow8(n)       # n zero bytes multiply the register by x^(8 n)


def _expect_clean(res, ts, bbf, npkt):
    assert res.resume == (len(ts), 0)
    want = dict(ZERO, accepted=npkt, ts_contributing=res.counters["ts_contributing"])
    assert res.counters == dict(want, ts_foreign=res.counters["ts_foreign"], ts_null=res.counters["ts_null"],
                                ts_no_payload=res.counters["ts_no_payload"])
    assert len(res.packets) == npkt and (res.packets["flags"] == 15).all()
    for got, w in zip(res.bbframes, bbf):
        np.testing.assert_array_equal(got, w)


def test_round_trip_single_plp():
    ts = C.clean_ts()
    res = R.parse(ts, C.PID, C.PLPS1)
    _expect_clean(res, ts, [C.bbframes(C.L1, C.NFRAMES * C.F1)], C.NPKT1)
    assert res.counters["ts_contributing"] == len(ts) // 188
    assert res.by_type == {0x20: 9, 0x10: 3, 0x00: 6} and res.blocks == [6]
    p = res.packets
    assert list(p["packet_count"]) == list(range(C.NPKT1))
    bb = p[p["packet_type"] == 0]
    assert list(bb["block"]) == list(range(6)) and list(bb["frame_idx"]) == [0, 0, 1, 1, 2, 2]
    assert list(bb["intl_frame_start"]) == [1, 0] * 3 and (bb["plp_id"] == 5).all() and (bb["out_index"] == 0).all()
    assert (p[p["packet_type"] != 0]["block"] == -1).all()
    assert list(p[p["packet_type"] == 0x10]["payload_len"]) == [203] * 3
    assert R.interleaving_frames(p, 0) == [C.F1] * C.NFRAMES
    # the record's position: the packet's first byte in the TS
    for r in p:
        assert ts[r["ts_byte"]] == r["packet_type"] and r["ts_byte"] // 188 == r["ts_index"]


def test_round_trip_three_plps_with_foreign_packets():
    plps = [(0, 879, 2), (1, 1194, 3), (9, 4836, 1)]
    bbf = [C.bbframes(L, 2 * F, seed=k) for k, (_, L, F) in enumerate(plps)]
    pk = R.encapsulate([(i, b, L, F) for (i, L, F), b in zip(plps, bbf)], 2, timestamps=1)
    ts = R.ts_mux(pk, C.PID, foreign_every=2, cc0=9, afc10_before=[3])
    res = R.parse(ts, C.PID, [(i, L) for i, L, _ in plps])
    _expect_clean(res, ts, bbf, len(pk))
    assert res.counters["ts_foreign"] == res.counters["ts_null"] == res.counters["ts_contributing"] // 2
    assert res.counters["ts_no_payload"] == 1 and res.blocks == [4, 6, 2]
    # the stream_id filter: nothing accepted, everything indexed
    res = R.parse(ts, C.PID, [(i, L) for i, L, _ in plps], stream_id=3)
    assert res.counters["filtered"] == len(pk) and res.counters["accepted"] == 0 and res.blocks == [0, 0, 0]


@pytest.mark.parametrize("name", sorted(C.geometry_cases()))
def test_geometry_streams_have_their_edge_and_parse_clean(name):
    ts = C.geometry_cases()[name]
    res = R.parse(ts, C.PID, C.PLPS1)
    _expect_clean(res, ts, [C.bbframes(C.L1, C.NFRAMES * C.F1)], C.NPKT1)
    rows = ts.reshape(-1, 188)
    pusi = [r for r in rows if r[1] & 0x40]
    ptr = [int(r[4]) if (r[3] >> 4) & 3 == 1 else int(r[5 + r[4]]) for r in pusi]
    if name == "pointer_0":
        assert ptr.count(0) >= 2
    if name == "pointer_182":
        assert 182 in ptr
    if name == "af_0_and_182":
        afl = [int(r[4]) for r in rows if (r[3] >> 4) & 3 == 3]
        assert 0 in afl and 182 in afl
    if name == "afc10_mid_packet":
        assert res.counters["ts_no_payload"] == 2
    bb = res.packets[res.packets["packet_type"] == 0]
    if name.startswith("header_split"):
        # BBFRAME packet 1 starts j bytes before a TS packet's end: its header continues in the next TS packet
        assert bb[1]["ts_byte"] % 188 == 188 - int(name[-1])
    if name.startswith("crc_split") or name == "ends_at_payload_end":
        # BBFRAME packet 2's last byte, found by walking its T bytes through the TS payloads from ts_byte
        def payload_of(i):
            c, off, pusi, _ = R.classify(ts, i, C.PID)
            return 188 * i + off + pusi
        x, i, left = int(bb[2]["ts_byte"]), int(bb[2]["ts_index"]), 10 + C.L1 + 3
        tail = []                                     # (TS index, offset in the TS packet) of the last 4 bytes
        while left:
            if x == 188 * (i + 1):
                i += 1
                x = payload_of(i)
            if left <= 4:
                tail.append((i, x % 188))
            x += 1
            left -= 1
        if name == "ends_at_payload_end":
            assert tail[3][1] == 187 and len({t[0] for t in tail}) == 1
        else:
            j = int(name[-1])
            assert [t[0] - tail[0][0] for t in tail] == [0] * j + [1] * (4 - j)     # the CRC split after byte j
            assert tail[j - 1][1] == 187
    # three starts in one TS packet
    per_ts = np.bincount(res.packets["ts_index"])
    assert per_ts.max() >= 3


def test_malformations_give_the_expected_counters():
    n_ts = len(C.clean_ts()) // 188
    blocks = C.NFRAMES * C.F1

    def run(name):
        ts = C.malformed(name)
        return ts, R.parse(ts, C.PID, C.PLPS1)

    ts, r = run("flipped_bit")
    assert r.counters == dict(ZERO, ts_contributing=n_ts, crc_errors=1, accepted=C.NPKT1 - 1) and r.blocks == [5]
    bb = r.packets[r.packets["packet_type"] == 0]
    assert list(bb["block"]) == [0, 1, -1, 2, 3, 4] and bb[2]["flags"] == 3      # later ranks shift down
    want = np.delete(C.bbframes(C.L1, blocks).reshape(-1, C.L1), 2, axis=0).reshape(-1)
    np.testing.assert_array_equal(r.bbframes[0], want)

    # a lost / unusable mid-packet TS packet: one discontinuity, exactly the straddling packet broken, the parse
    # re-anchored at the next PUSI
    for name, extra in (("dropped", {}), ("bad_sync", dict(ts_bad_sync=1)), ("tei", dict(ts_tei=1)),
                        ("scrambled", dict(ts_scrambled=1))):
        ts, r = run(name)
        assert r.counters == dict(ZERO, ts_contributing=n_ts - 1, discontinuities=1, broken=1,
                                  accepted=C.NPKT1 - 1, **extra), name
        assert r.blocks == [blocks - 1] and len(r.packets) == C.NPKT1 and r.resume == (len(ts), 0)
    ts, r = run("duplicated")
    assert r.counters == dict(ZERO, ts_contributing=n_ts + 1, discontinuities=1, broken=1, accepted=C.NPKT1 - 1)

    ts, r = run("wrong_length")
    assert r.counters == dict(ZERO, ts_contributing=r.counters["ts_contributing"], len_errors=1, accepted=C.NPKT1)
    assert r.blocks == [blocks - 1]
    ts, r = run("unmapped_plp")
    assert r.counters == dict(ZERO, ts_contributing=n_ts, other_plp=1, accepted=C.NPKT1) and r.blocks == [blocks - 1]

    # a length that points past the buffer: the packet is incomplete, the prefix ends before it and the resume
    # position names it
    ts, r = run("huge_len_last")
    assert len(r.packets) == C.NPKT1 and r.blocks == [blocks] and r.counters["accepted"] == C.NPKT1
    assert r.resume[0] < len(ts) and r.counters["ts_contributing"] == r.resume[0] // 188
    again = R.parse(ts, C.PID, C.PLPS1, start=r.resume)
    assert len(again.packets) == 0 and again.resume == r.resume

    ts, r = run("all_ff")
    assert r.counters == dict(ZERO, ts_bad_sync=40) and len(r.packets) == 0 and r.resume == (len(ts), 0)
    ts, r = run("no_pusi")
    assert r.counters == dict(ZERO, ts_contributing=len(ts) // 188,
                              discontinuities=r.counters["discontinuities"]) and len(r.packets) == 0
    assert r.counters["discontinuities"] > 0 and r.resume == (len(ts), 0)

    # a pointer_field that contradicts the previous packet's length: the packet it should point to is not found,
    # what it points to instead fails its checks, and the parse re-anchors
    ts, r = run("pointer")
    c = r.counters
    clean = R.parse(C.clean_ts(), C.PID, C.PLPS1)
    assert r.resume == (len(ts), 0) and c["discontinuities"] == 0 and c["bad_pointers"] == 0
    # the packets that start in the edited TS packet are lost; every other packet of the clean stream is accepted,
    # at its place and in order; whatever else the moved pointer made a start fails a check
    moved = int(np.nonzero(ts != C.clean_ts())[0][0]) // 188
    keep = clean.packets[clean.packets["ts_index"] != moved]
    assert 0 < len(keep) < C.NPKT1
    ok = r.packets[r.packets["flags"] == 15]
    np.testing.assert_array_equal(ok[["ts_byte", "packet_count", "packet_type"]],
                                  keep[["ts_byte", "packet_count", "packet_type"]])
    assert c["accepted"] == len(keep) and c["broken"] + c["crc_errors"] == len(r.packets) - len(keep) >= 1
    assert r.blocks == [int((keep["packet_type"] == 0).sum())]


def test_capacity_cuts_and_resume():
    ts = C.clean_ts()
    whole = R.parse(ts, C.PID, C.PLPS1)
    for k in range(0, 7):
        r = R.parse(ts, C.PID, C.PLPS1, caps=[k])
        assert r.blocks == [k]
        np.testing.assert_array_equal(r.bbframes[0], whole.bbframes[0][:k * C.L1])
        if k < 6:
            first_out = np.nonzero(whole.packets["block"] == k)[0][0]
            assert len(r.packets) == first_out
            np.testing.assert_array_equal(r.packets, whole.packets[:first_out])
        rest = R.parse(ts, C.PID, C.PLPS1, start=r.resume)
        assert len(r.packets) + len(rest.packets) == C.NPKT1
        np.testing.assert_array_equal(np.concatenate([r.bbframes[0], rest.bbframes[0]]), whole.bbframes[0])
        assert {n: r.counters[n] + rest.counters[n] for n in r.counters} == whole.counters
    for m in (0, 1, 2, 5, C.NPKT1):
        r = R.parse(ts, C.PID, C.PLPS1, max_packets=m)
        np.testing.assert_array_equal(r.packets, whole.packets[:m])
        # inside the run of three timestamp packets the resume position skips the ones already emitted
        if m in (1, 2):
            assert r.resume == (0, m)


def test_every_split_point_resumes_to_the_whole():
    ts = C.clean_ts(foreign_every=3)
    whole = R.parse(ts, C.PID, C.PLPS1)
    n = len(ts) // 188
    for cut in range(0, n + 1):
        outs, recs, cnt, by_type, pos = R.parse_chunked(ts, C.PID, C.PLPS1, [188 * cut])
        np.testing.assert_array_equal(outs[0], whole.bbframes[0])
        np.testing.assert_array_equal(recs, whole.packets)
        assert cnt == whole.counters and by_type == whole.by_type and pos == whole.resume, cut
    rng = np.random.default_rng(5)
    for _ in range(20):
        cuts = sorted(rng.integers(0, n + 1, 4))
        outs, recs, cnt, by_type, pos = R.parse_chunked(ts, C.PID, C.PLPS1, [188 * int(c) for c in cuts],
                                                        max_packets=int(rng.integers(1, 6)))
        # max_packets stops a call early: the last call may leave a rest
        rest = R.parse(ts, C.PID, C.PLPS1, start=pos)
        np.testing.assert_array_equal(np.concatenate([outs[0], rest.bbframes[0]])[:len(whole.bbframes[0])],
                                      whole.bbframes[0][:len(outs[0]) + len(rest.bbframes[0])])
        np.testing.assert_array_equal(recs[["ts_byte", "packet_count", "flags"]],
                                      whole.packets[:len(recs)][["ts_byte", "packet_count", "flags"]])
