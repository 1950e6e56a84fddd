"""CPU: the ULE reference (tests/ule_ref.py) that the GPU encapsulator is compared with -- CRC known answers, receiver
after encapsulator gives back the valid PDUs, hand-derived packets, the resume property at every split point,
capacity cuts, the flush forms, skipped PDUs -- and the C ABI's refusals without a GPU."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _UleParams, _UlePos, _UleResult
import t2mi_ref
import ule_cases as C
import ule_ref as R


def test_crc_known_answer_and_the_deframers():
    assert R.crc32(b"123456789") == 0x0376E6E7
    assert R.crc32_table(b"123456789") == 0x0376E6E7
    rng = np.random.default_rng(2)
    for n in (0, 1, 9, 40, 300):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        assert R.crc32(d) == R.crc32_table(d) == t2mi_ref.crc32_bitwise(d.tobytes()) == t2mi_ref.crc32_table(d.tobytes())


def _whole(pdus, d_bit, packing, **kw):
    pdu, off = R.pack(pdus)
    return pdu, off, R.encap(pdu, off, pid=C.PID, d_bit=d_bit, packing=packing, flush=True, **kw)


@pytest.mark.parametrize("packing", [1, 0])
@pytest.mark.parametrize("d_bit", [0, 1])
def test_receiver_after_encapsulator_is_the_valid_pdus(d_bit, packing):
    for name, pdus in C.cases(d_bit).items():
        crc = R.crc32_table if name == "max" else R.crc32
        pdu, off, r = _whole(pdus, d_bit, packing, crc=crc)
        assert R.receive(r.ts, C.PID, 0, crc) == R.valid_pdus(pdu, off, None, d_bit), name
        assert r.resume == (len(pdus), 0, r.counters["ts_packets"] & 15) and r.counters["flushed"] == 1, name
        assert r.counters["sndus"] == len(pdus), name
    # the sizes the cases are named for
    assert len(R.sndu(C.cases(1)["min"][0], 0x0800, 1, R.MAC)) == 9
    big = R.sndu(C.max_sndu(d_bit), 0x0800, d_bit, R.MAC, R.crc32_table)
    assert ((big[0] & 0x7F) << 8 | big[1]) == 32767 and len(big) == 32771
    pdu, off, r = _whole([C.max_sndu(d_bit)], d_bit, packing, crc=R.crc32_table)
    body = r.ts.reshape(-1, 188)[:, 4:]
    got = np.concatenate([body[0, 1:], body[1:].reshape(-1)])[:32771]   # behind PP 0, then packets without PUSI
    assert got.tobytes() == big and r.counters["sndus"] == 1


def _pk(ts, k):
    return ts.reshape(-1, 188)[k]


def test_known_answer_nine_byte_sndu_flushed():
    """one 1-byte PDU 45, no address: SNDU 80 05 08 00 45 + CRC; one packet: PUSI, PP 0, the SNDU, 174 x FF"""
    _, _, r = _whole([b"\x45"], 1, 1)
    p = _pk(r.ts, 0)
    assert len(r.ts) == 188 and list(p[:5]) == [0x47, 0x41, 0x00, 0x10, 0x00]
    assert list(p[5:10]) == [0x80, 0x05, 0x08, 0x00, 0x45]
    assert int.from_bytes(p[10:14].tobytes(), "big") == R.crc32(bytes([0x80, 0x05, 0x08, 0x00, 0x45]))
    assert (p[14:] == 0xFF).all() and r.counters["pad_bytes"] == 174 and r.counters["pusi_packets"] == 1
    # without the flush the packet is not determined: nothing is emitted, nothing is consumed
    pdu, off = R.pack([b"\x45"])
    r = R.encap(pdu, off, pid=C.PID, d_bit=1, start=(0, 0, 7))
    assert len(r.ts) == 0 and r.resume == (0, 0, 7) and r.counters["pdus_in"] == 0 and r.counters["flushed"] == 0


def test_known_answer_183_and_182_left():
    """an SNDU of 366 bytes: packet 0 holds PP 0 and 183 bytes, packet 1 has no PUSI: 183 bytes and one FF; the next
    SNDU starts packet 2 behind PP 0.  With 365 bytes packet 1 ends FF FF, the End Indicator"""
    for R_left in (183, 182):
        pdus = C.r_case(R_left, 0)
        pdu, off, r = _whole(pdus, 0, 1)
        S = R.sndu(pdus[0], 0x0800, 0, R.MAC)
        assert len(S) == 183 + R_left
        p0, p1, p2 = _pk(r.ts, 0), _pk(r.ts, 1), _pk(r.ts, 2)
        assert list(p0[:5]) == [0x47, 0x41, 0x00, 0x10, 0x00] and p0[5:].tobytes() == S[:183]
        assert list(p1[:4]) == [0x47, 0x01, 0x00, 0x11] and p1[4:4 + R_left].tobytes() == S[183:]
        assert (p1[4 + R_left:] == 0xFF).all() and len(p1[4 + R_left:]) == 184 - R_left
        assert list(p2[:5]) == [0x47, 0x41, 0x00, 0x12, 0x00] and p2[5:7].tobytes() == bytes([0x00, 40 + 10])
        assert p2[7:9].tobytes() == b"\x86\xdd"   # the second PDU is IPv6


def test_known_answer_payload_pointer_and_one_free_byte():
    """R = 2: packet 1 is PUSI, PP 2, the SNDU's last 2 bytes, then the next SNDU from payload byte 3.  An SNDU of
    182 bytes leaves one byte free: FF, and the next SNDU starts the next packet"""
    pdus = C.r_case(2, 0)
    _, _, r = _whole(pdus, 0, 1)
    S0, S1, S2 = (R.sndu(p, t, 0, R.MAC) for p, t in zip(pdus, (0x0800, 0x86DD, 0x0800)))
    p1 = _pk(r.ts, 1)
    assert list(p1[:5]) == [0x47, 0x41, 0x00, 0x11, 2] and p1[5:7].tobytes() == S0[-2:]
    assert p1[7:7 + len(S1)].tobytes() == S1 and p1[7 + len(S1):7 + len(S1) + len(S2)].tobytes() == S2
    used = 3 + len(S1) + len(S2)
    assert (p1[4 + used:] == 0xFF).all() and r.counters["ts_packets"] == 2
    assert r.counters["pad_bytes"] == 184 - used
    pdus = C.free_case(1, 0)
    _, _, r = _whole(pdus, 0, 1)
    p0, p1 = _pk(r.ts, 0), _pk(r.ts, 1)
    assert p0[4] == 0 and p0[5:187].tobytes() == R.sndu(pdus[0], 0x0800, 0, R.MAC) and p0[187] == 0xFF
    assert list(p1[:5]) == [0x47, 0x41, 0x00, 0x11, 0x00]


def test_known_answer_no_packing_and_flush_tail():
    """packing 0, an SNDU of 200 bytes: PUSI, PP 0, 183 bytes; then no PUSI, 17 bytes, 167 x FF; the next SNDU starts
    a packet of its own.  packing 1, the same SNDU alone, flushed: the second packet has no PUSI and no PP"""
    pdus = [C.ip(186, 1), C.ip(20, 2)]
    _, _, r = _whole(pdus, 0, 0)
    S = R.sndu(pdus[0], 0x0800, 0, R.MAC)
    p0, p1, p2 = _pk(r.ts, 0), _pk(r.ts, 1), _pk(r.ts, 2)
    assert len(S) == 200 and p0[1] == 0x41 and p0[4] == 0 and p0[5:].tobytes() == S[:183]
    assert p1[1] == 0x01 and p1[4:21].tobytes() == S[183:] and (p1[21:] == 0xFF).all()
    assert p2[1] == 0x41 and p2[4] == 0 and (p2[5 + 34:] == 0xFF).all()
    assert r.counters == dict(pdus_in=2, sndus=2, skipped_len=0, skipped_type=0, ts_packets=3, pusi_packets=2,
                              pad_bytes=167 + 183 - 34, flushed=1)
    _, _, r = _whole(pdus[:1], 0, 1)
    p1 = _pk(r.ts, 1)
    assert r.counters["ts_packets"] == 2 and p1[1] == 0x01 and p1[4:21].tobytes() == S[183:] and (p1[21:] == 0xFF).all()


@pytest.mark.parametrize("packing", [1, 0])
def test_every_split_point_resumes_to_the_whole(packing):
    pdus = C.mixed(40, 3, 1, 120)
    pdus[11] = C.ip(700, 11)
    pdus[20] = C.ip(30, 20, 0x50)      # skipped by its nibble
    pdu, off = R.pack(pdus)
    whole = R.encap(pdu, off, pid=C.PID, packing=packing, start=(0, 0, 5), flush=True)
    for k in range(41):
        a = R.encap(pdu[:off[k]], off[:k + 1], pid=C.PID, packing=packing, start=(0, 0, 5))
        b = R.encap(pdu, off, pid=C.PID, packing=packing, start=a.resume, flush=True)
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert b.resume == whole.resume
        for n in R.COUNTERS[:-1]:
            assert a.counters[n] + b.counters[n] == whole.counters[n], (k, n)


@pytest.mark.parametrize("packing", [1, 0])
def test_capacity_cuts_with_continuation(packing):
    pdus = C.r_case(367, 0) + C.mixed(12, 4)
    pdu, off = R.pack(pdus)
    whole = R.encap(pdu, off, pid=C.PID, packing=packing, flush=True)
    for cap in range(whole.counters["ts_packets"] + 1):
        a = R.encap(pdu, off, pid=C.PID, packing=packing, cap=cap, flush=True)
        assert a.counters["ts_packets"] == cap and a.counters["flushed"] == (cap == whole.counters["ts_packets"])
        np.testing.assert_array_equal(a.ts, whole.ts[:188 * cap])
        b = R.encap(pdu, off, pid=C.PID, packing=packing, start=a.resume, flush=True)
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert b.resume == whole.resume == (len(pdus), 0, whole.counters["ts_packets"] & 15)


def test_flush_forms():
    pdus = C.mixed(9, 6)
    pdu, off = R.pack(pdus)
    a = R.encap(pdu, off, pid=C.PID)                 # a partial PUSI packet stays behind
    f = R.encap(pdu, off, pid=C.PID, flush=True)
    assert f.counters["ts_packets"] == a.counters["ts_packets"] + 1 and a.resume[0] < 9 and f.resume[0] == 9
    last = f.ts.reshape(-1, 188)[-1]
    used = 184 - (f.counters["pad_bytes"] - a.counters["pad_bytes"])
    assert last[1] == 0x41 and 2 <= used <= 182 and (last[4 + used:] == 0xFF).all()
    # nothing left: the flush adds no packet
    pdus = [C.ip(183 - 14, 1)]
    pdu, off = R.pack(pdus)
    a, f = R.encap(pdu, off, pid=C.PID), R.encap(pdu, off, pid=C.PID, flush=True)
    np.testing.assert_array_equal(a.ts, f.ts)
    assert a.resume == f.resume == (1, 0, 1) and (a.counters["flushed"], f.counters["flushed"]) == (0, 1)
    # trailing skipped PDUs are consumed by the flush, and stay behind the open packet without it
    pdus = C.mixed(5, 7) + [C.ip(9, 1, 0x50), C.ip(9, 2, 0x10)]
    pdu, off = R.pack(pdus)
    a, f = R.encap(pdu, off, pid=C.PID), R.encap(pdu, off, pid=C.PID, flush=True)
    assert f.resume[0] == 7 and f.counters["skipped_type"] == 2 and f.counters["pdus_in"] == 7
    assert a.resume[0] < 5 and a.counters["pdus_in"] == a.resume[0] and a.counters["skipped_type"] == 0


def test_skipped_pdus():
    pdus = C.mixed(10, 8)
    pdus[2] = C.ip(12, 2, 0x50)                       # nibble 5
    pdus[6] = C.ip(32767 - 14 + 4 + 1, 6)             # one byte too long for the Length field
    pdu, off = R.pack(pdus)
    off = off.copy()
    off[5] = off[4]                                   # PDU 4 is empty (and PDU 5 begins where it did)
    off[10] = len(pdu) + 1                            # PDU 9 reaches past the buffer
    r = R.encap(pdu, off, pid=C.PID, flush=True, crc=R.crc32_table)
    assert r.counters["skipped_type"] == 1 and r.counters["skipped_len"] == 3 and r.counters["sndus"] == 6
    assert r.counters["pdus_in"] == 10 and r.resume[0] == 10
    assert R.receive(r.ts, C.PID, 0, R.crc32_table) == R.valid_pdus(pdu, off)
    # explicit types: no nibble is looked at
    types = np.arange(10, dtype=np.uint16) + 0x1000
    r = R.encap(pdu, off, types, pid=C.PID, flush=True, crc=R.crc32_table)
    assert r.counters["skipped_type"] == 0 and r.counters["sndus"] == 7
    assert [t for t, _, _ in R.receive(r.ts, C.PID, 0, R.crc32_table)] == [0x1000 + i for i in (0, 1, 2, 3, 5, 7, 8)]


def _params(**kw):
    p = _UleParams()
    p.pid, p.d_bit, p.packing, p.max_pdu_bytes, p.max_pdus = 0x100, 0, 1, 1 << 16, 1 << 10
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_capi_refuses_bad_parameters_before_the_device():
    L = dvbt2ll.lib()
    for n in ("create", "run_device", "get_result", "run_host", "destroy"):
        assert hasattr(L, "dvbt2ll_ule_" + n) and "dvbt2ll_ule_" + n in dvbt2ll.EXPORTS
    h = ctypes.c_void_p()
    bad = [_params(pid=-1), _params(pid=0x1FFF), _params(d_bit=2), _params(packing=2), _params(packing=-1),
           _params(max_pdu_bytes=0), _params(max_pdu_bytes=1 << 31), _params(max_pdus=0),
           _params(max_pdus=(1 << 24) + 1)]
    for p in bad:
        assert L.dvbt2ll_ule_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value
    assert L.dvbt2ll_ule_create(None, 0, ctypes.byref(h)) == -1
    assert L.dvbt2ll_ule_create(ctypes.byref(_params()), 0, None) == -1
    if L.dvbt2ll_device_count() == 0:
        for p in (_params(), _params(d_bit=1, packing=0)):
            assert L.dvbt2ll_ule_create(ctypes.byref(p), 0, ctypes.byref(h)) == -3 and not h.value   # EDEVICE
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.UleEncapsulator()
    pos, res = _UlePos(), _UleResult()
    assert L.dvbt2ll_ule_run_device(None, None, 1, None, None, 1, ctypes.byref(pos), None, 1, 0, None) == -1
    assert L.dvbt2ll_ule_run_host(None, None, 1, None, None, 1, ctypes.byref(pos), None, 1, 0, ctypes.byref(res)) == -1
    assert L.dvbt2ll_ule_get_result(None, ctypes.byref(res)) == -1
    L.dvbt2ll_ule_destroy(None)
    assert ctypes.sizeof(_UleParams) == 40 and ctypes.sizeof(_UleResult) == 80
    assert dvbt2ll.lib().dvbt2ll_abi_version() == 2
