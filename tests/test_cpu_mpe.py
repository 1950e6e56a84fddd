"""CPU: the MPE reference (tests/mpe_ref.py) that the GPU encapsulator is compared with -- CRC known answers, receiver
after encapsulator gives back the valid PDUs with their MACs, hand-derived packets, the multicast MAC mapping, the
resume property at every split point, capacity cuts, the flush forms, skipped PDUs -- and the C ABI's refusals without
a GPU."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _MpeParams, _MpePos, _MpeResult
import ule_ref
import mpe_cases as C
import mpe_ref as R

MAC = bytes([0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B])


def test_crc_known_answer_and_the_ule_reference():
    assert R.crc32(b"123456789") == 0x0376E6E7
    assert R.crc32_table(b"123456789") == 0x0376E6E7
    rng = np.random.default_rng(2)
    for n in (0, 1, 17, 40, 300):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        assert R.crc32(d) == R.crc32_table(d) == ule_ref.crc32(d) == ule_ref.crc32_table(d)
    s = R.section(b"\x45" * 5, MAC)
    assert R.crc32(s) == 0          # the CRC over a whole section, CRC_32 included, is 0


def _whole(pdus, packing=1, **kw):
    pdu, off = R.pack(pdus)
    return pdu, off, R.encap(pdu, off, pid=C.PID, packing=packing, flush=True, **kw)


def _pk(ts, k):
    return ts.reshape(-1, 188)[k]


@pytest.mark.parametrize("packing", [1, 0])
@pytest.mark.parametrize("mac_mode", [0, 1])
def test_receiver_after_encapsulator_is_the_valid_pdus(mac_mode, packing):
    for name, pdus in C.cases().items():
        crc = R.crc32_table if name == "max" else R.crc32
        pdu, off, r = _whole(pdus, packing, mac_mode=mac_mode, crc=crc)
        assert R.receive(r.ts, C.PID, 0, crc) == R.valid_pdus(pdu, off, MAC, mac_mode), name
        assert r.resume == (len(pdus), 0, r.counters["ts_packets"] & 15) and r.counters["flushed"] == 1, name
        assert r.counters["sections"] == len(pdus), name
        if name[0] in "Rf":
            assert r.counters["mapped_macs"] == (2 if name[0] == "R" else 1) * mac_mode, name
    # the sizes and positions the cases are named for
    assert len(R.section(C.cases()["min"][0], MAC)) == 17
    assert len(R.section(C.cases()["max"][1], MAC, R.crc32_table)) == 4096
    if packing:
        for Rl in C.R_VALUES:
            # packet 1 begins with Rl bytes left: a pointer_field of Rl, or no PUSI from 183 on
            _, _, r = _whole(C.r_case(Rl), 1)
            p1 = _pk(r.ts, 1) if Rl else None
            if 0 < Rl <= 182:
                assert p1[1] == 0x41 and p1[4] == Rl
            elif Rl:
                assert p1[1] == 0x01
        for f in C.FREE_VALUES:
            _, _, r = _whole(C.free_case(f), 1)
            p0, p1 = _pk(r.ts, 0), _pk(r.ts, 1)
            assert p0[1] == 0x41 and p0[4] == 0
            if f:
                assert p0[188 - f] == 0x3E                      # the next section starts with f bytes free
                assert p1[1] == 0x41 and p1[4] == 30 + 16 - f   # ... and runs on behind a pointer_field
            else:
                assert p1[1] == 0x41 and p1[4] == 0 and p1[5] == 0x3E


def test_known_answer_17_byte_section_and_the_mac_byte_order():
    """one 1-byte PDU 45, MAC 02:00:48:55:4c:4b: section 3E B0 0E 4B 4C C1 00 00 55 48 00 02 45 + CRC; one packet:
    PUSI, pointer_field 0, the section, 166 x FF"""
    _, _, r = _whole([b"\x45"])
    p = _pk(r.ts, 0)
    body = [0x3E, 0xB0, 0x0E, 0x4B, 0x4C, 0xC1, 0x00, 0x00, 0x55, 0x48, 0x00, 0x02, 0x45]
    assert len(r.ts) == 188 and list(p[:5]) == [0x47, 0x41, 0x00, 0x10, 0x00]
    assert list(p[5:18]) == body
    assert int.from_bytes(p[18:22].tobytes(), "big") == R.crc32(bytes(body))
    assert (p[22:] == 0xFF).all() and len(p[22:]) == 166
    assert r.counters == dict(pdus_in=1, sections=1, skipped_len=0, skipped_type=0, mapped_macs=0, ts_packets=1,
                              pusi_packets=1, pad_bytes=166, flushed=1)
    # without the flush the packet is not determined: nothing is emitted, nothing is consumed
    pdu, off = R.pack([b"\x45"])
    r = R.encap(pdu, off, pid=C.PID, start=(0, 0, 7))
    assert len(r.ts) == 0 and r.resume == (0, 0, 7) and r.counters["pdus_in"] == 0 and r.counters["flushed"] == 0
    # another address, a 2-byte IPv6 PDU: section_length 15
    pdu, off = R.pack([b"\x60\x01"])
    r = R.encap(pdu, off, pid=0x1234, mac=bytes([1, 2, 3, 4, 5, 6]), flush=True)
    assert list(r.ts[:18]) == [0x47, 0x52, 0x34, 0x10, 0x00, 0x3E, 0xB0, 0x0F, 6, 5, 0xC1, 0, 0, 4, 3, 2, 1, 0x60]


def test_known_answer_183_left_and_182_left_with_a_start_in_the_last_byte():
    """a section of 366 bytes: packet 0 holds pointer_field 0 and 183 bytes, packet 1 has no PUSI: 183 bytes and one
    FF; the next section starts packet 2 behind pointer_field 0.  With 365 bytes packet 1 is PUSI, pointer_field 182,
    the 182 bytes, and the next section's table_id in the last byte; packet 2 points behind the rest of that section"""
    pdus = C.r_case(183)
    _, _, r = _whole(pdus)
    S = R.section(pdus[0], MAC)
    assert len(S) == 366
    p0, p1, p2 = _pk(r.ts, 0), _pk(r.ts, 1), _pk(r.ts, 2)
    assert list(p0[:5]) == [0x47, 0x41, 0x00, 0x10, 0x00] and p0[5:].tobytes() == S[:183]
    assert list(p1[:4]) == [0x47, 0x01, 0x00, 0x11] and p1[4:187].tobytes() == S[183:] and p1[187] == 0xFF
    assert list(p2[:8]) == [0x47, 0x41, 0x00, 0x12, 0x00, 0x3E, 0xB0, 40 + 13]
    pdus = C.r_case(182)
    _, _, r = _whole(pdus)
    S0, S1, S2 = (R.section(p, MAC) for p in pdus)
    assert (len(S0), len(S1), len(S2)) == (365, 56, 41)
    p0, p1, p2 = _pk(r.ts, 0), _pk(r.ts, 1), _pk(r.ts, 2)
    assert list(p0[:5]) == [0x47, 0x41, 0x00, 0x10, 0x00] and p0[5:].tobytes() == S0[:183]
    assert list(p1[:5]) == [0x47, 0x41, 0x00, 0x11, 182] and p1[5:187].tobytes() == S0[183:] and p1[187] == 0x3E
    assert list(p2[:5]) == [0x47, 0x41, 0x00, 0x12, 55] and p2[5:60].tobytes() == S1[1:]
    assert p2[60:101].tobytes() == S2 and (p2[101:] == 0xFF).all()
    assert r.counters["ts_packets"] == 3 and r.counters["pusi_packets"] == 3 and r.counters["pad_bytes"] == 87


def test_known_answer_ten_and_twelve_smallest_sections():
    """ten 17-byte sections: pointer_field 0 and 170 bytes, all ten start in the one packet, 13 x FF.  With twelve the
    eleventh starts in the 13 free bytes and packet 1 points behind its last 4 bytes, where the twelfth starts"""
    pdus = [bytes([0x40 + k]) for k in range(12)]
    S = [R.section(p, MAC) for p in pdus]
    _, _, r = _whole(pdus[:10])
    p0 = _pk(r.ts, 0)
    assert r.counters["ts_packets"] == 1 and p0[1] == 0x41 and p0[4] == 0
    for k in range(10):
        assert p0[5 + 17 * k:5 + 17 * (k + 1)].tobytes() == S[k]
    assert (p0[175:] == 0xFF).all() and r.counters["pad_bytes"] == 13
    _, _, r = _whole(pdus)
    p0, p1 = _pk(r.ts, 0), _pk(r.ts, 1)
    assert p0[:175].tobytes() == _pk(_whole(pdus[:10])[2].ts, 0)[:175].tobytes() and p0[175:].tobytes() == S[10][:13]
    assert list(p1[:5]) == [0x47, 0x41, 0x00, 0x11, 4] and p1[5:9].tobytes() == S[10][13:]
    assert p1[9:26].tobytes() == S[11] and (p1[26:] == 0xFF).all()
    assert r.counters["ts_packets"] == 2 and r.counters["pad_bytes"] == 162


def test_known_answer_no_packing_and_flush_tail():
    """packing 0, a section of 200 bytes: PUSI, pointer_field 0, 183 bytes; then no PUSI, 17 bytes, 167 x FF; the next
    section starts a packet of its own.  packing 1, the same section alone, flushed: the second packet has no PUSI and
    no pointer_field"""
    pdus = [C.ip(184, 1), C.ip(20, 2)]
    _, _, r = _whole(pdus, 0)
    S = R.section(pdus[0], MAC)
    p0, p1, p2 = _pk(r.ts, 0), _pk(r.ts, 1), _pk(r.ts, 2)
    assert len(S) == 200 and p0[1] == 0x41 and p0[4] == 0 and p0[5:].tobytes() == S[:183]
    assert p1[1] == 0x01 and p1[4:21].tobytes() == S[183:] and (p1[21:] == 0xFF).all()
    assert p2[1] == 0x41 and p2[4] == 0 and p2[5:41].tobytes() == R.section(pdus[1], MAC) and (p2[41:] == 0xFF).all()
    assert r.counters == dict(pdus_in=2, sections=2, skipped_len=0, skipped_type=0, mapped_macs=0, ts_packets=3,
                              pusi_packets=2, pad_bytes=167 + 183 - 36, flushed=1)
    # flush changes nothing but flushed
    pdu, off = R.pack(pdus)
    a = R.encap(pdu, off, pid=C.PID, packing=0)
    np.testing.assert_array_equal(a.ts, r.ts)
    assert a.resume == r.resume and a.counters["flushed"] == 0
    _, _, r = _whole(pdus[:1], 1)
    p1 = _pk(r.ts, 1)
    assert r.counters["ts_packets"] == 2 and p1[1] == 0x01 and p1[4:21].tobytes() == S[183:] and (p1[21:] == 0xFF).all()
    # a section takes ceil((n + 1) / 184) packets
    for p in (1, 167, 168, 351, 352, 4080):
        _, _, r = _whole([C.ip(p, p)], 0, crc=R.crc32_table)
        assert r.counters["ts_packets"] == -(-(p + 16 + 1) // 184)


def test_multicast_mac_mapping():
    v4 = C.ip(28, 1, 0x45, bytes([239, 1, 2, 3]))
    v4hi = C.ip(20, 2, 0x45, bytes([224, 0x81, 2, 3]))          # bit 23 of the group is dropped
    v6 = C.ip(40, 3, 0x60, C.V6_GROUP)
    uni4 = C.ip(28, 4, 0x45, bytes([10, 0, 0, 1]))
    uni6 = C.ip(40, 5, 0x60, bytes.fromhex("20010db8000000000000000000001234"))
    short4 = C.ip(19, 6, 0x45, bytes([239, 1, 2]))              # an IPv4 PDU of 19 bytes: no destination to read
    short6 = C.ip(39, 7, 0x60, C.V6_GROUP)
    edge = [C.ip(20, 8, 0x45, bytes([223, 1, 2, 3])), C.ip(20, 9, 0x45, bytes([240, 1, 2, 3]))]
    pdus = [v4, v4hi, v6, uni4, uni6, short4, short6] + edge
    pdu, off, r = _whole(pdus, 1, mac_mode=1)
    want = [bytes.fromhex("01005e010203"), bytes.fromhex("01005e010203"), bytes.fromhex("3333ff001234")] + [MAC] * 6
    got = R.receive(r.ts, C.PID, 0)
    assert [m for m, _ in got] == want and [d for _, d in got] == pdus
    assert r.counters["mapped_macs"] == 3
    _, _, r = _whole(pdus, 0, mac_mode=0)
    assert [m for m, _ in R.receive(r.ts, C.PID, 0)] == [MAC] * 9 and r.counters["mapped_macs"] == 0
    # the mapped address lies in the header as any other: last byte first
    _, _, r = _whole([v6], 1, mac_mode=1)
    assert list(r.ts[8:10]) == [0x34, 0x12] and list(r.ts[13:17]) == [0x00, 0xFF, 0x33, 0x33]


@pytest.mark.parametrize("packing", [1, 0])
def test_every_split_point_resumes_to_the_whole(packing):
    pdus = C.mixed(40, 3, 1, 120)
    pdus[11] = C.ip(700, 11)
    pdus[20] = C.ip(30, 20, 0x50)      # skipped by its nibble
    pdu, off = R.pack(pdus)
    whole = R.encap(pdu, off, pid=C.PID, mac_mode=1, packing=packing, start=(0, 0, 5), flush=True)
    for k in range(41):
        a = R.encap(pdu[:off[k]], off[:k + 1], pid=C.PID, mac_mode=1, packing=packing, start=(0, 0, 5))
        b = R.encap(pdu, off, pid=C.PID, mac_mode=1, packing=packing, start=a.resume, flush=True)
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert b.resume == whole.resume
        for n in R.COUNTERS[:-1]:
            assert a.counters[n] + b.counters[n] == whole.counters[n], (k, n)
    assert whole.counters["mapped_macs"] > 0


@pytest.mark.parametrize("packing", [1, 0])
def test_capacity_cuts_with_continuation(packing):
    pdus = C.free_case(2) + C.r_case(367) + C.mixed(12, 4)
    pdu, off = R.pack(pdus)
    whole = R.encap(pdu, off, pid=C.PID, packing=packing, flush=True)
    inside = 0
    for cap in range(whole.counters["ts_packets"] + 1):
        a = R.encap(pdu, off, pid=C.PID, packing=packing, cap=cap, flush=True)
        assert a.counters["ts_packets"] == cap and a.counters["flushed"] == (cap == whole.counters["ts_packets"])
        np.testing.assert_array_equal(a.ts, whole.ts[:188 * cap])
        b = R.encap(pdu, off, pid=C.PID, packing=packing, start=a.resume, flush=True)
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert b.resume == whole.resume == (len(pdus), 0, whole.counters["ts_packets"] & 15)
        inside += 0 < a.resume[1] < 12
    assert inside >= packing           # packing: one cut falls inside a straddling header


def test_flush_forms():
    pdus = C.mixed(9, 6)
    pdu, off = R.pack(pdus)
    a = R.encap(pdu, off, pid=C.PID)                 # a partial PUSI packet stays behind
    f = R.encap(pdu, off, pid=C.PID, flush=True)
    assert f.counters["ts_packets"] == a.counters["ts_packets"] + 1 and a.resume[0] < 9 and f.resume[0] == 9
    last = f.ts.reshape(-1, 188)[-1]
    used = 184 - (f.counters["pad_bytes"] - a.counters["pad_bytes"])
    assert last[1] == 0x41 and 18 <= used <= 183 and (last[4 + used:] == 0xFF).all()
    # one byte free and nothing behind it: held back without the flush, one FF with it
    pdus = [C.ip(182 - 16, 1)]
    pdu, off = R.pack(pdus)
    a, f = R.encap(pdu, off, pid=C.PID), R.encap(pdu, off, pid=C.PID, flush=True)
    assert a.counters["ts_packets"] == 0 and a.resume == (0, 0, 0)
    assert f.counters["ts_packets"] == 1 and f.counters["pad_bytes"] == 1 and f.ts[187] == 0xFF
    # nothing left: the flush adds no packet
    pdus = [C.ip(183 - 16, 1)]
    pdu, off = R.pack(pdus)
    a, f = R.encap(pdu, off, pid=C.PID), R.encap(pdu, off, pid=C.PID, flush=True)
    np.testing.assert_array_equal(a.ts, f.ts)
    assert a.resume == f.resume == (1, 0, 1) and (a.counters["flushed"], f.counters["flushed"]) == (0, 1)
    # the flush's last packet holds a section's end only: no PUSI, no pointer_field; held back without the flush
    pdus = [C.ip(183 + 60 - 16, 2)]
    pdu, off = R.pack(pdus)
    a, f = R.encap(pdu, off, pid=C.PID), R.encap(pdu, off, pid=C.PID, flush=True)
    assert a.counters["ts_packets"] == 1 and a.resume == (0, 183, 1)
    assert f.counters["ts_packets"] == 2 and f.ts[188 + 1] == 0x01 and f.counters["pusi_packets"] == 1
    # trailing skipped PDUs are consumed by the flush, and stay behind the open packet without it
    pdus = C.mixed(5, 7) + [C.ip(9, 1, 0x50), C.ip(9, 2, 0x10)]
    pdu, off = R.pack(pdus)
    a, f = R.encap(pdu, off, pid=C.PID), R.encap(pdu, off, pid=C.PID, flush=True)
    assert f.resume[0] == 7 and f.counters["skipped_type"] == 2 and f.counters["pdus_in"] == 7
    assert a.resume[0] < 5 and a.counters["pdus_in"] == a.resume[0] and a.counters["skipped_type"] == 0


def test_skipped_pdus():
    pdus = C.mixed(10, 8)
    pdus[2] = C.ip(12, 2, 0x50)                       # nibble 5
    pdus[6] = C.ip(4081, 6, 0x50)                     # one byte too long, and a bad nibble: the length is judged first
    pdus[7] = C.ip(4080, 7)                           # the longest
    pdu, off = R.pack(pdus)
    off = off.copy()
    off[5] = off[4]                                   # PDU 4 is empty (and PDU 5 begins where it did)
    off[10] = len(pdu) + 1                            # PDU 9 reaches past the buffer
    r = R.encap(pdu, off, pid=C.PID, flush=True, crc=R.crc32_table)
    assert r.counters["skipped_type"] == 1 and r.counters["skipped_len"] == 3 and r.counters["sections"] == 6
    assert r.counters["pdus_in"] == 10 and r.resume[0] == 10
    assert R.receive(r.ts, C.PID, 0, R.crc32_table) == R.valid_pdus(pdu, off)
    assert [R.classify(pdu, off, i) for i in (2, 4, 6, 7, 9)] == ["type", "len", "len", "ok", "len"]


def test_receiver_refuses_what_the_encapsulator_never_sends():
    pdus = C.r_case(1)
    _, _, r = _whole(pdus)
    assert len(R.receive(r.ts, C.PID, 0)) == 3
    for at, msg in ((4 + 188, "pointer"), (3 + 188, "continuity"), (40, "CRC")):
        bad = r.ts.copy()
        bad[at] ^= 0x01
        with pytest.raises(AssertionError):
            R.receive(bad, C.PID, 0)


def _params(**kw):
    p = _MpeParams()
    p.pid, p.mac_mode, p.packing, p.max_pdu_bytes, p.max_pdus = 0x100, 0, 1, 1 << 16, 1 << 10
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_capi_refuses_bad_parameters_before_the_device():
    L = dvbt2ll.lib()
    for n in ("create", "run_device", "get_result", "run_host", "destroy"):
        assert hasattr(L, "dvbt2ll_mpe_" + n) and "dvbt2ll_mpe_" + n in dvbt2ll.EXPORTS
    h = ctypes.c_void_p()
    bad = [_params(pid=-1), _params(pid=0x1FFF), _params(mac_mode=2), _params(mac_mode=-1), _params(packing=2),
           _params(packing=-1), _params(max_pdu_bytes=0), _params(max_pdu_bytes=1 << 31), _params(max_pdus=0),
           _params(max_pdus=(1 << 24) + 1)]
    for p in bad:
        assert L.dvbt2ll_mpe_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value
    assert L.dvbt2ll_mpe_create(None, 0, ctypes.byref(h)) == -1
    assert L.dvbt2ll_mpe_create(ctypes.byref(_params()), 0, None) == -1
    pos, res = _MpePos(), _MpeResult()
    assert L.dvbt2ll_mpe_run_device(None, None, 1, None, 1, ctypes.byref(pos), None, 1, 0, None) == -1
    assert L.dvbt2ll_mpe_run_host(None, None, 1, None, 1, ctypes.byref(pos), None, 1, 0, ctypes.byref(res)) == -1
    assert L.dvbt2ll_mpe_get_result(None, ctypes.byref(res)) == -1
    L.dvbt2ll_mpe_destroy(None)
    assert ctypes.sizeof(_MpeParams) == 40 and ctypes.sizeof(_MpeResult) == 88
    assert dvbt2ll.lib().dvbt2ll_abi_version() == 2


def test_capi_edevice_without_a_gpu():
    L = dvbt2ll.lib()
    if L.dvbt2ll_device_count() > 0:
        pytest.skip("a GPU is visible")
    h = ctypes.c_void_p()
    for p in (_params(), _params(mac_mode=1, packing=0)):
        assert L.dvbt2ll_mpe_create(ctypes.byref(p), 0, ctypes.byref(h)) == -3 and not h.value   # EDEVICE
    with pytest.raises(dvbt2ll.DVBT2Error):
        dvbt2ll.MpeEncapsulator()
