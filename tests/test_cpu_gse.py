"""CPU: the GSE rules of include/dvbt2ll_hip.h as tests/gse_ref.py restates them -- hand-derived byte strings, the
receiver's round trip, the placement edges, chained calls, capacity cuts, flush forms, Frag IDs -- and the C ABI's
refusals, which need no device."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _GseParams, _GsePos, _GseResult
import gse_cases as C
import gse_ref as R


def test_crc32_check_value():
    assert R.crc32(b"123456789") == 0x0376E6E7
    assert R.crc32_table(b"123456789") == 0x0376E6E7
    data = C.ip(777, 1)
    assert R.crc32(data) == R.crc32_table(data)


@pytest.mark.parametrize("kbch", C.KBCHS)
@pytest.mark.parametrize("label", C.LABELS)
def test_receiver_of_encapsulator_is_the_valid_pdus(kbch, label):
    L = len(label)
    pdus = C.mixed(60, 3, 1, 300) + [C.ip(4090 - L, 4), C.ip(9, 5, 0x50), C.ip(1500, 6, 0x60), C.ip(4091 - L, 7)]
    pdus += C.mixed(30, 8, 200, 1500)
    pdu, off = R.pack(pdus)
    r = R.encap(pdu, off, kbch=kbch, label=label, flush=True, crc=R.crc32_table)
    assert R.receive(r.bb, kbch, L, crc=R.crc32_table) == R.valid_pdus(pdu, off, label=label)
    assert r.counters["skipped_type"] == 1 and r.counters["skipped_len"] == 1 and r.resume[0] == len(pdus)
    assert r.counters["complete"] + r.counters["fragmented"] == len(pdus) - 2
    assert r.counters["pad_bytes"] + sum(
        int.from_bytes(f[4:6].tobytes(), "big") // 8 for f in r.bb.reshape(-1, kbch // 8)) == \
        r.counters["bbframes"] * C.D_of(kbch)


def _frame(kbch, field):
    D = C.D_of(kbch)
    h = bytes([0xB0, 0, 0, 0, (8 * len(field)) >> 8, (8 * len(field)) & 255, 0, 0, 0])
    return h + bytes([R.crc8(h)]) + field + bytes(D - len(field))


def test_hand_derived_frames():
    kbch = 3072                                   # D = 374
    # 1. one complete packet in a flushed frame, no label: S 1, E 1, LT 10 -> E0 | Length >> 8; Length = 2 + 3;
    #    Protocol Type 0800 (nibble 4); the PDU.  7 bytes: DFL = 56 = 0x0038
    p = bytes([0x45, 0x01, 0x02])
    pdu, off = R.pack([p])
    r = R.encap(pdu, off, kbch=kbch, label=b"", flush=True)
    field = bytes([0xE0, 0x05, 0x08, 0x00]) + p
    assert r.bb.tobytes() == _frame(kbch, field)
    assert r.bb[:9].tobytes() == bytes([0xB0, 0, 0, 0, 0, 0x38, 0, 0, 0])
    assert r.counters == dict(pdus_in=1, complete=1, fragmented=0, gse_packets=1, skipped_len=0, skipped_type=0,
                              bbframes=1, pad_bytes=367, flushed=1) and r.resume == (1, 0, 1)
    assert R.encap(pdu, off, kbch=kbch, label=b"").counters["bbframes"] == 0
    # the same with a 3-byte label: LT 01 -> D0; Length = 2 + 3 + 3
    r = R.encap(pdu, off, kbch=kbch, label=b"\x0a\x0b\x0c", flush=True)
    assert r.bb[10:20].tobytes() == bytes([0xD0, 0x08, 0x08, 0x00, 0x0A, 0x0B, 0x0C]) + p
    # 2. 400 bytes at u = 0: 4 + 400 > 374, so a first fragment fills the frame: piece = 374 - 7 = 367; S 1, E 0,
    #    LT 10 -> A0 | 372 >> 8 = A1, 74; Frag ID 5; Total Length 2 + 400 = 0192; 0800; 367 bytes.  Then rem = 33,
    #    33 + 7 <= 374: the end fragment, S 0, E 1, LT 11 -> 70, Length 1 + 33 + 4 = 0x26; Frag ID; 33 bytes; the CRC
    #    over 0192 0800 and the PDU
    p = C.ip(400, 2)
    pdu, off = R.pack([p])
    r = R.encap(pdu, off, kbch=kbch, label=b"", start=(0, 0, 5), flush=True)
    f0 = bytes([0xA1, 0x74, 0x05, 0x01, 0x92, 0x08, 0x00]) + p[:367]
    crc = R.crc32(bytes([0x01, 0x92, 0x08, 0x00]) + p).to_bytes(4, "big")
    f1 = bytes([0x70, 0x26, 0x05]) + p[367:] + crc
    assert len(f0) == 374 and r.bb.tobytes() == _frame(kbch, f0) + _frame(kbch, f1)
    assert r.counters["fragmented"] == 1 and r.counters["gse_packets"] == 2 and r.counters["pad_bytes"] == 374 - 40
    # 3. 800 bytes: piece 367, rem 433; 433 + 7 > 374: a continuation with min(371, 432) = 371 bytes, S 0, E 0,
    #    LT 11 -> 30 | 372 >> 8 = 31, 74; rem 62: the end fragment, Length 1 + 62 + 4 = 0x43
    p = C.ip(800, 3, 0x60)
    pdu, off = R.pack([p])
    r = R.encap(pdu, off, kbch=kbch, label=b"", flush=True)
    crc = R.crc32(bytes([0x03, 0x22, 0x86, 0xDD]) + p).to_bytes(4, "big")
    want = _frame(kbch, bytes([0xA1, 0x74, 0x00, 0x03, 0x22, 0x86, 0xDD]) + p[:367])
    want += _frame(kbch, bytes([0x31, 0x74, 0x00]) + p[367:738])
    want += _frame(kbch, bytes([0x70, 0x43, 0x00]) + p[738:] + crc)
    assert r.bb.tobytes() == want and r.counters["gse_packets"] == 3
    # 4. 736 bytes: piece 367, rem 369 = D - 5: 369 + 7 > 374, and the continuation takes min(371, 368) = 368 bytes
    #    (Length 369 = 0x171), leaving 3 bytes unused, so that the end fragment carries one byte (Length 6)
    p = C.ip(736, 4)
    pdu, off = R.pack([p])
    r = R.encap(pdu, off, kbch=kbch, label=b"", flush=True)
    crc = R.crc32(bytes([0x02, 0xE2, 0x08, 0x00]) + p).to_bytes(4, "big")
    want = _frame(kbch, bytes([0xA1, 0x74, 0x00, 0x02, 0xE2, 0x08, 0x00]) + p[:367])
    want += _frame(kbch, bytes([0x31, 0x71, 0x00]) + p[367:735])
    want += _frame(kbch, bytes([0x70, 0x06, 0x00]) + p[735:] + crc)
    assert r.bb.tobytes() == want
    assert int.from_bytes(r.bb[384 + 4:384 + 6].tobytes(), "big") == 8 * 371


@pytest.mark.parametrize("kbch", C.KBCHS)
@pytest.mark.parametrize("label", C.LABELS)
def test_placement_edges(kbch, label):
    L, D = len(label), C.D_of(kbch)
    kw = dict(kbch=kbch, label=label, crc=R.crc32_table)
    for name, pdus in C.cases(kbch, L).items():
        pdu, off = R.pack(pdus)
        r = R.encap(pdu, off, flush=True, **kw)
        assert R.receive(r.bb, kbch, L, crc=R.crc32_table) == R.valid_pdus(pdu, off, label=label), name
        bb = r.bb.reshape(-1, kbch // 8)
        dfl = [int.from_bytes(f[4:6].tobytes(), "big") // 8 for f in bb]
        if name.startswith("free "):
            i = len(pdus) - 3                      # the PDU under test
            free = {"0": 0, "1": 1, "7+L": 7 + L, "8+L": 8 + L, "3+L+len": 3 + L + 100, "4+L+len": 4 + L + 100,
                    "5+L+len": 5 + L + 100}[name[5:]]
            frag = 8 + L <= free < 4 + L + 100
            assert r.counters["fragmented"] == int(frag), name
            if free >= 4 + L + 100:                # complete, in the first frame
                assert D - free + 4 + L + 100 <= dfl[0] <= D, name
            else:
                assert dfl[0] == (D if frag else D - free), name
            if 0 < free < 8 + L:                   # closed as it is: the PDU starts the next frame
                assert bb[1][10] >> 6 == 3 and r.counters["pad_bytes"] >= free
            assert i >= 1
        if name.startswith("rem "):
            rem = {"D-8": D - 8, "D-7": D - 7, "D-6": D - 6, "D-3": D - 3, "D-2": D - 2, "2D": 2 * D}[name[4:]]
            assert bb[0][10 + D - 12 - L] >> 4 == (0x8 | (0 if L == 6 else 1 if L == 3 else 2)), name
            if rem <= D - 7:
                assert bb[1][10] >> 4 == 0x7 and dfl[1] >= rem + 7, name
            else:
                assert bb[1][10] >> 4 == 0x3 and dfl[1] == 3 + min(D - 3, rem - 1) and D - dfl[1] <= 4, name
        if name == "len 1, max":
            assert r.counters["skipped_len"] == 0 and r.counters["complete"] + r.counters["fragmented"] == 4
        if name == "too long, empty":
            assert r.counters["skipped_len"] == 2 and r.counters["complete"] == 2


def test_every_split_of_40_pdus():
    kbch, label = 3072, C.LABELS[1]
    pdus = C.mixed(40, 9, 1, 500)
    pdus[7] = C.ip(20, 7, 0x50)
    pdu, off = R.pack(pdus)
    whole = R.encap(pdu, off, kbch=kbch, label=label, start=(0, 0, 250), flush=True)
    assert whole.counters["fragmented"] > 5
    for k in range(41):
        a = R.encap(pdu[:off[k]], off[:k + 1], kbch=kbch, label=label, start=(0, 0, 250))
        b = R.encap(pdu, off, kbch=kbch, label=label, start=a.resume, flush=True)
        np.testing.assert_array_equal(np.concatenate([a.bb, b.bb]), whole.bb)
        assert b.resume == whole.resume and a.resume[0] <= k
        for name in R.COUNTERS[:-1]:
            assert a.counters[name] + b.counters[name] == whole.counters[name], (k, name)


def test_capacity_cuts_mid_pdu():
    kbch, label = 3072, C.LABELS[2]
    pdus = C.mixed(5, 10, 20, 90) + [C.ip(1500, 1)] + C.mixed(8, 11, 100, 400)
    pdu, off = R.pack(pdus)
    whole = R.encap(pdu, off, kbch=kbch, label=label, flush=True)
    n = whole.counters["bbframes"]
    mids = set()
    for cap in range(n + 1):
        a = R.encap(pdu, off, kbch=kbch, label=label, cap=cap, flush=True)
        assert a.counters["bbframes"] == cap and a.counters["flushed"] == int(cap == n)
        mids.add(a.resume[1] > 0)
        b = R.encap(pdu, off, kbch=kbch, label=label, start=a.resume, flush=True)
        np.testing.assert_array_equal(np.concatenate([a.bb, b.bb]), whole.bb)
        for name in R.COUNTERS[:-1]:
            assert a.counters[name] + b.counters[name] == whole.counters[name], (cap, name)
    assert mids == {True, False}
    # a pdu_byte that names no byte 1 .. len - 1 of a valid PDU is taken as 0
    for bad in (len(pdus[0]), 5000):
        np.testing.assert_array_equal(R.encap(pdu, off, kbch=kbch, label=label, start=(0, bad, 0), flush=True).bb,
                                      whole.bb)


def test_flush_forms():
    kbch = 3072
    pdu, off = R.pack(C.mixed(4, 12))
    a, f = R.encap(pdu, off, kbch=kbch), R.encap(pdu, off, kbch=kbch, flush=True)
    assert (a.counters["bbframes"], f.counters["bbframes"]) == (0, 1) and a.resume == (0, 0, 0) and f.resume == (4, 0, 4)
    assert (a.counters["pdus_in"], f.counters["flushed"]) == (0, 1)
    # u = 0 at the end: the flush writes no frame
    pdu, off = R.pack(C.fill(374, 6))
    a, f = R.encap(pdu, off, kbch=kbch), R.encap(pdu, off, kbch=kbch, flush=True)
    np.testing.assert_array_equal(a.bb, f.bb)
    assert a.resume == f.resume == (1, 0, 1) and f.counters["flushed"] == 0 and f.counters["bbframes"] == 1
    # the flush frame does not fit the capacity
    pdu, off = R.pack(C.fill(374, 6) + C.mixed(3, 13))
    c = R.encap(pdu, off, kbch=kbch, cap=1, flush=True)
    assert c.counters["flushed"] == 0 and c.resume == (1, 0, 1)
    # trailing skipped PDUs are consumed with the flush, and stay behind the open frame without it
    pdu, off = R.pack(C.mixed(3, 14) + [C.ip(9, 1, 0x50)])
    a, f = R.encap(pdu, off, kbch=kbch), R.encap(pdu, off, kbch=kbch, flush=True)
    assert a.resume[0] == 0 and f.resume[0] == 4 and f.counters["skipped_type"] == 1
    r = R.encap(np.zeros(0, np.uint8), np.zeros(1, np.uint32), kbch=kbch, flush=True)
    assert r.counters["bbframes"] == 0 and r.resume == (0, 0, 0)


def test_frag_ids_wrap_and_chain():
    kbch = 3072
    pdus = [C.ip(500, k) for k in range(8)]
    pdu, off = R.pack(pdus)
    whole = R.encap(pdu, off, kbch=kbch, label=b"", start=(0, 0, 252), flush=True)
    ids = [int(f[12]) for f in whole.bb.reshape(-1, 384) if f[10] >> 6 == 2]     # first fragments at a frame's start
    assert 255 in ids + [int(whole.bb[384 * k + 12]) for k in range(8)] and whole.resume == (8, 0, 4)
    seen = set()
    for f in whole.bb.reshape(-1, 384):
        pos, dfl = 0, int.from_bytes(f[4:6].tobytes(), "big") // 8
        while pos < dfl:
            S, E = f[10 + pos] >> 7, (f[10 + pos] >> 6) & 1
            if not (S and E):
                seen.add(int(f[12 + pos]))
            pos += 2 + (((int(f[10 + pos]) & 15) << 8) | int(f[11 + pos]))
    assert {252, 253, 254, 255, 0, 1, 2, 3} >= seen and {255, 0} <= seen
    a = R.encap(pdu, off, kbch=kbch, label=b"", start=(0, 0, 252), cap=6, flush=True)
    assert a.resume[2] == (252 + a.resume[0]) & 255
    b = R.encap(pdu, off, kbch=kbch, label=b"", start=a.resume, flush=True)
    np.testing.assert_array_equal(np.concatenate([a.bb, b.bb]), whole.bb)
    assert R.receive(whole.bb, kbch, 0) == R.valid_pdus(pdu, off, label=b"")


def _params(**kw):
    p = _GseParams()
    p.kbch, p.sis_mis, p.label_len, p.max_pdu_bytes, p.max_pdus = 7032, 1, 6, 1 << 16, 1 << 10
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_capi_refuses_bad_parameters_before_the_device():
    L = dvbt2ll.lib()
    for n in ("create", "params_from_chain", "run_device", "get_result", "run_host", "destroy"):
        assert hasattr(L, "dvbt2ll_gse_" + n) and "dvbt2ll_gse_" + n in dvbt2ll.EXPORTS
    h = ctypes.c_void_p()
    bad = [_params(kbch=7040), _params(kbch=0, framesize=2), _params(kbch=0, framesize=1, rate=6), _params(kbch=-8),
           _params(label_len=1), _params(label_len=4), _params(label_len=-1), _params(label_len=7),
           _params(sis_mis=2), _params(sis_mis=0, isi=256), _params(max_pdu_bytes=0), _params(max_pdu_bytes=1 << 31),
           _params(max_pdus=0), _params(max_pdus=(1 << 24) + 1)]
    for p in bad:
        assert L.dvbt2ll_gse_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value
    assert L.dvbt2ll_gse_create(None, 0, ctypes.byref(h)) == -1
    assert L.dvbt2ll_gse_create(ctypes.byref(_params()), 0, None) == -1
    if L.dvbt2ll_device_count() == 0:
        for p in (_params(), _params(kbch=3072, label_len=0), _params(kbch=0, framesize=1, rate=5, label_len=3)):
            assert L.dvbt2ll_gse_create(ctypes.byref(p), 0, ctypes.byref(h)) == -3 and not h.value   # EDEVICE
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.GseEncapsulator(kbch=7032)
    pos, res = _GsePos(), _GseResult()
    assert L.dvbt2ll_gse_run_device(None, None, 1, None, None, 1, ctypes.byref(pos), None, 1, 0, None) == -1
    assert L.dvbt2ll_gse_run_host(None, None, 1, None, None, 1, ctypes.byref(pos), None, 1, 0, ctypes.byref(res)) == -1
    assert L.dvbt2ll_gse_get_result(None, ctypes.byref(res)) == -1
    assert L.dvbt2ll_gse_params_from_chain(None, 0, ctypes.byref(_params())) == -1
    L.dvbt2ll_gse_destroy(None)
    assert ctypes.sizeof(_GseParams) == 48 and ctypes.sizeof(_GseResult) == 88
    assert dvbt2ll.lib().dvbt2ll_abi_version() == 2
    assert dvbt2ll.gse.frame_bound(10000, 10, 374, 6) == (10000 + 100) // 354 + 2
