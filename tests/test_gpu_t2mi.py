"""GPU: the T2-MI deframer (dvbt2ll_t2mi_*, csrc/t2mi_kernels.hip) against the sequential parser of tests/t2mi_ref.py
(proven by tests/test_cpu_t2mi.py): the packet table record for record, every counter, the resume position and the
output bytes, all exact.  Every device run here has its TS inside a larger poisoned array and its outputs inside
poisoned arrays with guard regions; the guards and the bytes past each output's last block must stay untouched.  No
test looks for a fault: malformed streams check counters and untouched guards."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS, MPLP_CONFIGS, KBCH
import bbch_cases as BC
import bbf_ref as BR
import oracle_lib as O
import t2mi_cases as C
import t2mi_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1)


def _deframer(plps=C.PLPS1, max_ts_bytes=188 * 256, max_packets=256, **kw):
    return dvbt2ll.T2miDeframer(C.PID, plps=plps, max_ts_bytes=max_ts_bytes, max_packets=max_packets, **kw)


_STREAM = []


def _side_stream():
    """a torch stream with a handle of its own: torch's default stream has handle 0, which the C ABI reads as "the
    handle's own stream" (a non-blocking one), and then the fills and the copy of the TS below and the deframer's
    kernels would not be ordered -- with a TS of a hundred megabytes the deframer reads it half copied"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def device_run(de, ts, start=(0, 0), caps=None, misalign=3, stream=None, full_blocks=8):
    """one run_device with everything inside poisoned arrays; returns the result with bbframes filled in, after
    checking the guards.  caps None: room for full_blocks blocks per output"""
    import torch
    st = _side_stream() if stream is None else stream
    caps = [full_blocks] * de.nplp if caps is None else list(caps)
    with torch.cuda.stream(st):
        buf = torch.full((2 * GUARD + len(ts) + 16,), POISON, dtype=torch.uint8, device="cuda")
        off = GUARD + misalign
        buf[off:off + len(ts)] = torch.from_numpy(np.ascontiguousarray(ts)).cuda()
        outs, offs = [], []
        for k, (_, L) in enumerate(de.plps):
            outs.append(torch.full((2 * GUARD + caps[k] * L + 16,), POISON, dtype=torch.uint8, device="cuda"))
            offs.append(GUARD + (k * 5 + 1) % 16)
        de.run_device(buf.data_ptr() + off, len(ts), [o.data_ptr() + a for o, a in zip(outs, offs)], caps,
                      start=start, stream=st.cuda_stream)
    res = de.result()
    st.synchronize()
    res.bbframes = []
    for k, (_, L) in enumerate(de.plps):
        o, a = outs[k].cpu().numpy(), offs[k]
        n = res.blocks[k] * L
        assert res.blocks[k] <= caps[k]
        assert (o[:a] == POISON).all() and (o[a + n:] == POISON).all(), "output %d written outside its blocks" % k
        res.bbframes.append(o[a:a + n].copy())
    got = buf.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + len(ts):] == POISON).all()
    np.testing.assert_array_equal(got[off:off + len(ts)], ts)
    return res


def same(res, ref, ctx=""):
    assert res.resume == ref.resume, (ctx, res.resume, ref.resume)
    assert res.counters == ref.counters, (ctx, res.counters, ref.counters)
    assert res.blocks == ref.blocks and res.by_type == ref.by_type, (ctx, res.blocks, ref.blocks, res.by_type)
    assert len(res.packets) == len(ref.packets), (ctx, len(res.packets), len(ref.packets))
    bad = np.nonzero(res.packets != ref.packets.astype(dvbt2ll.t2mi.PACKET_DTYPE))[0]
    assert bad.size == 0, "%s: records %s differ: %s / %s" % (ctx, bad[:4], res.packets[bad[:2]], ref.packets[bad[:2]])
    for k, (got, want) in enumerate(zip(res.bbframes, ref.bbframes)):
        np.testing.assert_array_equal(got, want, err_msg="%s output %d" % (ctx, k))


def check(de, ts, ctx, plps=C.PLPS1, **kw):
    stream_id = kw.pop("stream_id", -1)
    ref_kw = {k: v for k, v in kw.items() if k in ("start", "caps")}
    if "caps" not in ref_kw:
        ref_kw["caps"] = [8] * len(plps)      # device_run's default room
    ref = R.parse(ts, C.PID, plps, max_packets=de.max_packets, stream_id=stream_id, **ref_kw)
    res = device_run(de, ts, **kw)
    same(res, ref, ctx)
    return res, ref


@pytest.fixture(scope="module")
def de1(gpu):
    return _deframer()


def test_record_layout_matches_the_reference():
    assert dvbt2ll.t2mi.PACKET_DTYPE == R.REC


# ---------------------------------------------------------------------------------------- 1. clean streams, the chain
def _chain_iq(ch, bbf_dev, n):
    import torch
    iq = torch.zeros((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if ch.nplp == 1:
        ch.run_device(bbf_dev[0].data_ptr(), 0, bbf_dev[0].numel(), 0, n, iq.data_ptr(), st)
    else:
        ch.run_plps([b.data_ptr() for b in bbf_dev], [0] * ch.nplp, [b.numel() for b in bbf_dev], 0, n,
                    iq.data_ptr(), st)
    torch.cuda.synchronize()
    return iq.cpu().numpy().reshape(-1)


@pytest.mark.parametrize("name", ["cfg1q", "nm8"])
def test_clean_single_plp_feeds_the_chain_to_the_ts_path_iq(gpu, name):
    """the oracle's BBFRAMEs (those its bbheaderbch built from the synthetic TS) through encapsulation and the
    deframer, on the device into a Chain in BBFRAME input: the TS path's IQ, bit for bit.  cfg1q: L = 879 (odd),
    F = 2; nm8: the NM sweep shape, 8 blocks per frame"""
    import torch
    cfg = CONFIGS["cfg1q"] if name == "cfg1q" else BC.SWEEPS["nm"][0]
    n, F, L = 3, cfg.fecblocks, BR.bbframe_len(cfg)
    assert L == 879 and F == (2 if name == "cfg1q" else 8)
    bbf = BR.oracle_bbframes(cfg, 0, n)
    ts = R.ts_mux(R.encapsulate([(0, bbf, L, F)], n, timestamps=3), C.PID, foreign_every=4)
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    want = ch.run(0, n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    de = dvbt2ll.T2miDeframer(C.PID, chain=ch, max_ts_bytes=len(ts), max_packets=64)
    assert de.plps == [(0, L)]
    ts_d = torch.from_numpy(ts).cuda()
    out = torch.zeros(n * F * L, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    de.run_device(ts_d.data_ptr(), len(ts), [out.data_ptr()], [n * F], stream=st)
    got = _chain_iq(ch, [out], n)        # same stream: no synchronise between deframer and chain
    res = de.result()
    res.bbframes = [out.cpu().numpy()]
    same(res, R.parse(ts, C.PID, [(0, L)]), name)
    np.testing.assert_array_equal(res.bbframes[0], bbf)
    assert de.interleaving_frames(0, res) == [F] * n
    assert np.array_equal(_bits(got), _bits(want))
    assert ch.bbheader_errors() == 0


def test_clean_three_plps_feed_the_multi_plp_chain(gpu):
    """mplp3_4k: three different L, one PLP in HEM; PLP_IDs 0, 1, 2 interleaved frame by frame in one TS"""
    import torch
    m = MPLP_CONFIGS["mplp3_4k"]
    n = 2
    _, bb_bits, _ = O.mplp_cells(m, 0, n)
    bbf, plps = [], []
    for k, p in enumerate(m.plps):
        kb = KBCH[(p.framesize, p.rate)]
        bits = np.concatenate(bb_bits[k]).reshape(n * p.fecblocks, -1)[:, :kb]
        bbf.append(np.packbits(bits ^ BR.prbs_bits(kb)[None, :], axis=1).reshape(-1))
        plps.append((k, bbf[k], kb // 8, p.fecblocks))
    assert len({p[2] for p in plps}) == 3
    ts = R.ts_mux(R.encapsulate(plps, n, timestamps=1), C.PID, cc0=7)
    ch = dvbt2ll.Chain(m, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    direct = _chain_iq(ch, [torch.from_numpy(b).cuda() for b in bbf], n)
    de = dvbt2ll.T2miDeframer(C.PID, chain=ch, max_ts_bytes=len(ts), max_packets=256)
    assert de.plps == [(k, p[2]) for k, p in enumerate(plps)]
    res, ref = check(de, ts, "mplp3_4k", plps=de.plps, caps=[n * p[3] for p in plps])
    for k in range(3):
        np.testing.assert_array_equal(res.bbframes[k], bbf[k])
        assert de.interleaving_frames(k, res) == [plps[k][3]] * n
    got = _chain_iq(ch, [torch.from_numpy(b).cuda() for b in res.bbframes], n)
    assert np.array_equal(_bits(got), _bits(direct))


# ---------------------------------------------------------------------------------------- 2. packet geometry
@pytest.mark.parametrize("name", sorted(C.geometry_cases()))
def test_packet_geometry(gpu, de1, name):
    ts = C.geometry_cases()[name]
    res, ref = check(de1, ts, name)
    assert res.blocks == [C.NFRAMES * C.F1] and res.counters["accepted"] == C.NPKT1
    np.testing.assert_array_equal(res.bbframes[0], C.bbframes(C.L1, C.NFRAMES * C.F1))


# ---------------------------------------------------------------------------------------- 3. malformations
@pytest.mark.parametrize("name", C.MALFORMATIONS)
def test_malformations(gpu, de1, name):
    ts = C.malformed(name)
    res, ref = check(de1, ts, name)
    if name == "flipped_bit":
        assert res.counters["crc_errors"] == 1 and res.blocks == [5]
    if name in ("dropped", "duplicated", "bad_sync", "tei"):
        assert res.counters["broken"] == 1 and res.counters["discontinuities"] == 1


def test_payload_len_ffff_is_incomplete_not_a_wild_read(gpu, de1):
    """the buffer's last packet claims 8192 payload bytes: nothing past the TS is read (the run sits at the end of
    its allocation's used part), the prefix ends before it, and a later call from the resume position agrees"""
    ts = C.malformed("huge_len_last")
    res, ref = check(de1, ts, "huge len", misalign=0)
    assert res.resume[0] < len(ts)
    check(de1, ts, "huge len resumed", start=res.resume)


# ---------------------------------------------------------------------------------------- 4. bounds, capacities
@pytest.mark.parametrize("k", [0, 1, 3, 5, 6])
def test_output_capacity_cut_and_continue(gpu, de1, k):
    ts = C.clean_ts()
    whole = R.parse(ts, C.PID, C.PLPS1)
    res, ref = check(de1, ts, "cap %d" % k, caps=[k])
    assert res.blocks == [k]
    rest, _ = check(de1, ts, "cap %d rest" % k, start=res.resume)
    np.testing.assert_array_equal(np.concatenate([res.bbframes[0], rest.bbframes[0]]), whole.bbframes[0])
    assert len(res.packets) + len(rest.packets) == C.NPKT1


@pytest.mark.parametrize("m", [1, 2, 5, 17])
def test_table_capacity_cut_and_continue(gpu, m):
    ts = C.clean_ts()
    de = _deframer(max_packets=m)
    pos, recs, out = (0, 0), [], []
    for _ in range(C.NPKT1 // m + 2):
        res, ref = check(de, ts, "table %d at %s" % (m, pos), start=pos)
        assert len(res.packets) <= m
        recs.append(res.packets)
        out.append(res.bbframes[0])
        pos = res.resume
    whole = R.parse(ts, C.PID, C.PLPS1)
    assert pos == whole.resume
    np.testing.assert_array_equal(np.concatenate(out), whole.bbframes[0])
    np.testing.assert_array_equal(np.concatenate(recs)["ts_byte"], whole.packets["ts_byte"])


# ---------------------------------------------------------------------------------------- 5. resume and chunking
def test_chunked_calls_equal_the_single_call(gpu, de1):
    """cuts at TS-packet boundaries: right after the TS packet that holds more than three starts (the next start
    lies in it too, so the resume position has a skip), before anything (twice: an empty call keeps the position),
    mid-packet: the chained calls' outputs, tables and summed counters are the single call's"""
    ts = C.clean_ts(foreign_every=3)
    whole = R.parse(ts, C.PID, C.PLPS1)
    n = len(ts) // 188
    three = int(np.argmax(np.bincount(whole.packets["ts_index"]) >= 3))
    for cuts in ([three + 1], [0, 0, 1, 2, n - 1], [5, 6, 7, 20]):
        pos, recs, out, cnt = (0, 0), [], [], {}
        for end in [188 * c for c in cuts] + [len(ts)]:
            res, ref = check(de1, ts[:end], "chunks %s to %d" % (cuts, end), start=pos)
            recs.append(res.packets)
            out.append(res.bbframes[0])
            for key, v in res.counters.items():
                cnt[key] = cnt.get(key, 0) + v
            pos = res.resume
        np.testing.assert_array_equal(np.concatenate(out), whole.bbframes[0])
        allrecs = np.concatenate(recs)
        assert len(allrecs) == C.NPKT1
        np.testing.assert_array_equal(allrecs[["ts_index", "ts_byte", "packet_count", "flags"]],
                                      whole.packets[["ts_index", "ts_byte", "packet_count", "flags"]].astype(
                                          allrecs[["ts_index", "ts_byte", "packet_count", "flags"]].dtype))
        assert cnt == whole.counters and pos == whole.resume


def test_more_than_one_scan_tile(gpu):
    """1100 TS packets and 1500 T2-MI packets: the device-wide scans span two tiles of 1024"""
    pk = [R.timestamp_packet(i & 255, i) for i in range(1500)] + list(C.base_packets())
    ts = R.ts_mux(pk, C.PID, foreign_every=1, af={q: 150 for q in range(0, 400, 2)})
    assert len(ts) // 188 > 1024
    de = _deframer(max_ts_bytes=len(ts), max_packets=2048)
    res, ref = check(de, ts, "two tiles")
    assert len(res.packets) == len(pk) and res.blocks == [C.NFRAMES * C.F1]


# ---------------------------------------------------------------------------------------- 6. launch forms
def test_run_host_and_stream_id_filter(gpu):
    ts = C.clean_ts()
    de = _deframer()
    res = de.run(ts)
    same(res, R.parse(ts, C.PID, C.PLPS1), "run_host")
    res = de.run(ts, caps=[3])
    same(res, R.parse(ts, C.PID, C.PLPS1, caps=[3]), "run_host cap 3")
    pk = list(C.base_packets()) + R.encapsulate([(5, C.bbframes(C.L1, 2, seed=4), C.L1, 2)], 1, stream_id=3)
    ts = R.ts_mux(pk, C.PID)
    for sid in (-1, 0, 3, 6):
        f = _deframer(stream_id=sid)
        check(f, ts, "stream_id %d" % sid, stream_id=sid)


def test_two_handles_on_two_streams(gpu):
    import torch
    a, b = _deframer(), _deframer()
    ts_a, ts_b = C.clean_ts(), C.clean_ts(foreign_every=1, cc0=5)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in range(2):
        ra = device_run(a, ts_a, stream=sa)
        rb = device_run(b, ts_b, stream=sb)
        same(ra, R.parse(ts_a, C.PID, C.PLPS1), "handle a")
        same(rb, R.parse(ts_b, C.PID, C.PLPS1), "handle b")


def test_refusals_launch_nothing(gpu):
    import torch
    ts = C.clean_ts()
    de = _deframer(max_ts_bytes=len(ts))
    L = dvbt2ll.lib()
    for plps in ([], [(k, 879) for k in range(9)], [(1, 879), (1, 879)], [(1, 880)], [(1, 0)]):
        with pytest.raises(dvbt2ll.DVBT2Error):
            _deframer(plps=plps)
    ts_d = torch.from_numpy(ts).cuda()
    out = torch.full((8 * C.L1,), POISON, dtype=torch.uint8, device="cuda")
    before = de.run(ts).counters
    for length, start, ptrs, caps in ((len(ts) - 1, (0, 0), [out.data_ptr()], [8]),
                                      (len(ts) + 188, (0, 0), [out.data_ptr()], [8]),
                                      (len(ts), (0, -1), [out.data_ptr()], [8]),
                                      (len(ts), (94, 0), [out.data_ptr()], [8]),
                                      (len(ts), (len(ts) + 188, 0), [out.data_ptr()], [8]),
                                      (len(ts), (0, 0), [None], [8]),
                                      (len(ts), (0, 0), [out.data_ptr()], [-1])):
        with pytest.raises(dvbt2ll.DVBT2Error):
            de.run_device(ts_d.data_ptr(), length, ptrs, caps, start=start)
    with pytest.raises(dvbt2ll.DVBT2Error):
        de.run_device(0, len(ts), [out.data_ptr()], [8])
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert de.result().counters == before        # the last real run's result still stands
    assert L.dvbt2ll_t2mi_get_result(None, None) == -1


# ---------------------------------------------------------------------------------------- 7. the command-line tool
TOOL = Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "dvbt2ll" / "dvbt2ll_tx"


def _tool(*args):
    return subprocess.run([str(TOOL)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_single_plp_equals_bbframe_input(gpu, tmp_path):
    """dvbt2ll_tx --input t2mi on a written file: the IQ file of --input bbframe on the same BBFRAMEs, byte for
    byte (cfg1q, 3 frames in batches of 2: one call's blocks feed two runs); the counters are printed"""
    cfg = CONFIGS["cfg1q"]
    n, F, L = 3, cfg.fecblocks, BR.bbframe_len(cfg)
    bbf = BR.oracle_bbframes(cfg, 0, n)
    (tmp_path / "in.bbf").write_bytes(bbf.tobytes())
    ts = R.ts_mux(R.encapsulate([(5, bbf, L, F)], n, timestamps=3), 0x321, foreign_every=2)
    (tmp_path / "in.ts").write_bytes(ts.tobytes())
    r = _tool("--preset", "cfg1q", "--input", "bbframe", "--in", tmp_path / "in.bbf", "--out", tmp_path / "a.iq",
              "--batch", 2)
    assert r.returncode == 0, r.stderr
    r = _tool("--preset", "cfg1q", "--input", "t2mi", "--pid", "0x321", "--plp-id", 5, "--in", tmp_path / "in.ts",
              "--out", tmp_path / "b.iq", "--batch", 2)
    assert r.returncode == 0, r.stderr
    a, b = (tmp_path / "a.iq").read_bytes(), (tmp_path / "b.iq").read_bytes()
    assert len(a) == n * dvbt2ll.Chain(cfg, max_frames=1).iq_per_frame * 8 and a == b
    ref = R.parse(ts, 0x321, [(5, L)])
    assert "%d T2 frames" % n in r.stderr and "accepted %d," % ref.counters["accepted"] in r.stderr
    assert "crc_errors 0," in r.stderr and "foreign %d," % ref.counters["ts_foreign"] in r.stderr
    assert " 5:%d(" % (n * F) in r.stderr


def test_cli_multi_plp_equals_run_plps(gpu, tmp_path):
    """--mplp mplp3_4k --input t2mi: one TS file for all three PLPs (PLP_IDs 7, 1, 4 mapped with --plp-id) gives
    the IQ of the Python chain's run_plps on the same BBFRAMEs"""
    import torch
    m = MPLP_CONFIGS["mplp3_4k"]
    n, ids = 2, (7, 1, 4)
    _, bb_bits, _ = O.mplp_cells(m, 0, n)
    bbf, plps = [], []
    for k, p in enumerate(m.plps):
        kb = KBCH[(p.framesize, p.rate)]
        bits = np.concatenate(bb_bits[k]).reshape(n * p.fecblocks, -1)[:, :kb]
        bbf.append(np.packbits(bits ^ BR.prbs_bits(kb)[None, :], axis=1).reshape(-1))
        plps.append((ids[k], bbf[k], kb // 8, p.fecblocks))
    ch = dvbt2ll.Chain(m, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    want = _chain_iq(ch, [torch.from_numpy(b).cuda() for b in bbf], n)
    (tmp_path / "in.ts").write_bytes(R.ts_mux(R.encapsulate(plps, n, timestamps=1), 4096).tobytes())
    r = _tool("--mplp", "mplp3_4k", "--input", "t2mi", "--plp-id", 7, "--plp-id", 1, "--plp-id", 4,
              "--in", tmp_path / "in.ts", "--out", tmp_path / "o.iq", "--batch", 1)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer((tmp_path / "o.iq").read_bytes(), np.float32)
    assert np.array_equal(_bits(got), _bits(want))


def test_cli_refuses_a_short_interleaving_frame(gpu, tmp_path):
    """the second interleaving frame has F - 1 blocks: a clear message, a non-zero exit"""
    cfg = BC.SWEEPS["nm"][0]
    n, F, L = 3, cfg.fecblocks, BR.bbframe_len(cfg)
    pk = R.encapsulate([(0, BR.oracle_bbframes(cfg, 0, n), L, F)], n, timestamps=1)
    bb = C.bbframe_indices(pk)
    del pk[bb[F + 3]]                      # a block of frame 1 that is not its first
    (tmp_path / "in.ts").write_bytes(R.ts_mux(pk, 4096).tobytes())
    r = _tool("--preset", "cfg1", "--set", "rate=0", "--input", "t2mi", "--in", tmp_path / "in.ts", "--out", tmp_path / "o.iq")
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert "interleaving frame of %d FEC blocks" % (F - 1) in r.stderr and "PLP_NUM_BLOCKS" in r.stderr
    assert "accepted %d," % len(pk) in r.stderr        # the counters are printed on refusal too
