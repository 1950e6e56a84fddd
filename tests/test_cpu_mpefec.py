"""CPU: the MPE-FEC reference (tests/mpefec_ref.py) that the GPU encapsulator is compared with -- Reed-Solomon known
answers and syndromes, receiver after encapsulator for every rows value, the MPE reference's own receiver on the same
TS, erasure recovery, hand-derived bytes of a tiny frame, the resume property at every split / capacity / max_frames
cut -- and the C ABI's refusals without a GPU."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _MpeFecParams, _MpeFecPos, _MpeFecResult
import mpe_ref
import mpefec_cases as C
import mpefec_ref as R

KNOWN = {
    "d190": "c10aff3a80b7738c99935bc5dbdddc8e1c7815a49306cc28e6b60e79308f4de451552ba210c3a323959a2384646433b00ba186d084f4b0c0dde8ab7d9be4f2f5",
    "d0": "8f2f0f0e27c062c4ca5b54f829383db2c9124491f65405aa3c95ed09cb2846e596f7f1b0f3182c7cbc51d7bcc65656a4e8807fc5b8c68ee8a03d9c70cd58968b",
    "ramp": "d40c2afe1ad9bbf60e8ab7e310fb65af12490b5b9da773ff6c1a1d17b09b8da735faefb2a18b5b27de78f6d61ceb003abebf5a94d5b40a016972d48b3c7e2281",
    "ff": "5dd3f3e4cf0c8d929a70ba251945f2e7b68f12f078b259be3e0023b18e8576f09728255e3dcf18d9dbfaebe9983c9868a022ba924c3da8604cfb57ef62d1b6c8",
}


def test_reed_solomon_known_answers():
    d = np.zeros((191, 4), np.int64)
    d[190, 0] = 1
    d[0, 1] = 1
    d[:, 2] = (7 * np.arange(191) + 3) & 0xFF
    d[:, 3] = 0xFF
    par = R.rs_parity(d)
    for col, name in enumerate(("d190", "d0", "ramp", "ff")):
        assert par[:, col].tobytes().hex() == KNOWN[name], name
    assert R.G[0] == 0xF5 == int(R.EXP[2016 % 255]) and 2016 % 255 == 231 and R.G[64] == 1
    assert [R.G[63 - k] for k in range(64)] == list(bytes.fromhex(KNOWN["d190"]))


def test_syndromes_of_random_rows_are_zero_and_the_crc_is_the_mpe_references():
    d = np.random.default_rng(1).integers(0, 256, (191, 40), dtype=np.uint8)
    code = np.concatenate([d, R.rs_parity(d)])
    assert not R.syndromes(code).any()
    code[17, 3] ^= 0x40
    s = R.syndromes(code)
    assert s[:, 3].all() and not np.delete(s, 3, axis=1).any()
    for n in (0, 1, 17, 300):
        b = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        assert R.crc32_fast(b) == mpe_ref.crc32(b)


@pytest.mark.parametrize("rows", R.ROWS)
def test_receiver_after_encapsulator_is_the_valid_datagrams(rows):
    """every D of DS with every K of KS (K below 64 on a full table: puncturing), in both packing values and MAC modes:
    U = C, C - 1 with a miss by one byte, one datagram, a straddled column; then the MPE reference's own receiver,
    unchanged, reads the same datagrams from the same TS"""
    for n, (D, K) in enumerate((D, K) for D in C.DS for K in C.KS):
        for name, pdus in C.frame_cases(rows, D).items():
            mac_mode, packing = (n + (rows >> 8)) & 1, ((n + (rows >> 8)) >> 1) & 1
            pdu, off = R.pack(pdus)
            r = R.encap(pdu, off, rows=rows, D=D, K=K, pid=C.PID, mac_mode=mac_mode, packing=packing, flush=True,
                        start=(0, 0, 0, 3, 4095))
            frames = R.receive(r.ts, K, C.PID, 3, 4095)
            want = R.valid_pdus(pdu, off, rows, D)
            assert [d for f in frames for d in f.datagrams] == want and all(f.ok for f in frames), (D, K, name)
            assert [f.delta_t for f in frames] == [(4095 + k) & 0xFFF for k in range(len(frames))]
            assert r.counters["frames"] == len(frames) and r.counters["fec_sections"] == K * len(frames)
            assert r.resume == (len(pdus), 0, 0, (3 + r.counters["ts_packets"]) & 15, (4095 + len(frames)) & 0xFFF)
            # a receiver that knows nothing of MPE-FEC drops table_id 78 and reads every datagram
            plain = mpe_ref.receive(_without_fec(r.ts), C.PID, None, R.crc32_fast)
            assert [d for _, d in plain] == want
            macs = [mpe_ref.mac_of(d, R.MAC, mac_mode)[0] for d in want]
            assert [(m[4], m[5]) for m, _ in plain] == [(m[4], m[5]) for m in macs]
            if name == "full":
                assert len(frames) == 2 and sum(len(d) for d in frames[0].datagrams) == D * rows
            if name == "minus1":
                assert len(frames) == 2 and sum(len(d) for d in frames[0].datagrams) == D * rows - 1


def _without_fec(ts):
    """the packets that hold MPE sections only (packing 0: every section has packets of its own), or all of them with
    the MPE-FEC sections cut out and re-packed by the reference packer"""
    secs = R._sections(ts, C.PID, None, R.crc32_fast, False)
    keep = [(s, (0, k)) for k, s in enumerate(secs) if s[0] == 0x3E]
    pk, _ = R.pack_sections(keep, 0, 1, True)
    out = np.full((len(pk), 188), 0xFF, np.uint8)
    for p, (u, payload, _) in enumerate(pk):
        out[p, :4] = [0x47, (u << 6) | (C.PID >> 8), C.PID & 255, 0x10 | (p & 15)]
        out[p, 4:4 + len(payload)] = np.frombuffer(payload, np.uint8)
    # the RT word lies where the plain MPE section has MAC_address_4 .. 1: the MPE receiver reads it as such
    return out.reshape(-1)


def test_erasure_recovery_up_to_k_columns():
    """rows 256, K 8: TS packets deleted from one frame so that at most 8 data columns are unreliable are repaired;
    with 9 the receiver reports failure"""
    rows, K = 256, 8
    pdus = [C.ip4(700, k) for k in range(20)]
    pdu, off = R.pack(pdus)
    r = R.encap(pdu, off, rows=rows, D=191, K=K, pid=C.PID, flush=True)
    ts = r.ts.reshape(-1, 188)
    assert R.receive(r.ts, K, C.PID)[0].datagrams == pdus

    def lose(*spans):
        gone = np.concatenate([np.arange(a, b) for a, b in spans])
        return np.delete(ts, gone, axis=0).reshape(-1)

    # packets 8 .. 11 hold parts of two datagrams (addresses 700 .. 2099: columns 2 .. 8)
    f = R.receive(lose((8, 12)), K, C.PID, lossy=True)[0]
    assert f.ok and f.bad_columns == 6 and f.datagrams == pdus
    # one packet more, and two that hold MPE-FEC sections: K unreliable columns, RS columns among them
    f = R.receive(lose((8, 13), (len(ts) - 6, len(ts) - 4)), K, C.PID, lossy=True)[0]
    assert f.ok and f.bad_columns == K and f.datagrams == pdus
    # K + 1: the receiver reports failure
    f = R.receive(lose((8, 16)), K, C.PID, lossy=True)[0]
    assert not f.ok and f.bad_columns == K + 1
    code = np.concatenate([np.zeros((191, 4), np.uint8), np.zeros((64, 4), np.uint8)])
    assert R.erasure_fill(code, list(range(65))) is None


def test_hand_derived_bytes_of_a_tiny_frame():
    """rows 256, D 1, K 2, datagrams of 100 and 50 bytes, delta_t 5: RT words 00500000 and 00580064, the MPE-FEC header
    78 B1 0D BE FF FF kk 01 and RT 00500000 / 005C0100, padding_columns 190"""
    a, b = C.ip(100, 1), C.ip(50, 2)
    pdu, off = R.pack([a, b])
    r = R.encap(pdu, off, rows=256, D=1, K=2, pid=C.PID, packing=0, flush=True, start=(0, 0, 0, 0, 5))
    secs = R._sections(r.ts, C.PID, 0, R.crc32_fast, False)
    assert [len(s) for s in secs] == [116, 66, 272, 272]
    assert secs[0][:12] == bytes([0x3E, 0xB0, 113, 0x4B, 0x4C, 0xC1, 0, 0, 0x00, 0x50, 0x00, 0x00]) and secs[0][12:-4] == a
    assert secs[1][:12] == bytes([0x3E, 0xB0, 63, 0x4B, 0x4C, 0xC1, 0, 0, 0x00, 0x58, 0x00, 0x64]) and secs[1][12:-4] == b
    assert secs[2][:12] == bytes([0x78, 0xB1, 0x0D, 190, 0xFF, 0xFF, 0, 1, 0x00, 0x50, 0x00, 0x00])
    assert secs[3][:12] == bytes([0x78, 0xB1, 0x0D, 190, 0xFF, 0xFF, 1, 1, 0x00, 0x5C, 0x01, 0x00])
    A = np.zeros((191, 256), np.uint8)
    A[0, :150] = np.frombuffer(a + b, np.uint8)
    par = R.rs_parity(A)
    assert secs[2][12:-4] == par[0].tobytes() and secs[3][12:-4] == par[1].tobytes()
    assert r.counters == dict(pdus_in=2, sections=2, fec_sections=2, frames=1, skipped_len=0, skipped_type=0,
                              mapped_macs=0, ts_packets=1 + 1 + 2 + 2, pusi_packets=4, pad_bytes=6 * 184 - 4 - 726,
                              flushed=1)
    # an open frame without a flush: nothing, and nothing consumed
    r = R.encap(pdu, off, rows=256, D=1, K=2, pid=C.PID, start=(0, 0, 0, 7, 5))
    assert len(r.ts) == 0 and r.resume == (0, 0, 0, 7, 5) and r.counters["pdus_in"] == 0


def _kw(packing, **kw):
    return dict(rows=256, D=2, K=3, pid=C.PID, mac_mode=1, packing=packing, **kw)


@pytest.mark.parametrize("packing", [1, 0])
def test_every_split_capacity_and_max_frames_cut_resumes_to_the_whole(packing):
    pdus = C.small_frames(40, 3)
    pdus[20] = C.ip(30, 20, 0x50)      # skipped by its nibble
    pdu, off = R.pack(pdus)
    st = (0, 0, 0, 5, 4094)
    whole = R.encap(pdu, off, start=st, flush=True, **_kw(packing))
    assert whole.counters["frames"] > 8 and whole.counters["mapped_macs"] > 0
    for k in range(41):                # every split of the list as two chained calls
        a = R.encap(pdu[:off[k]], off[:k + 1], start=st, **_kw(packing))
        b = R.encap(pdu, off, start=a.resume, flush=True, **_kw(packing))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert b.resume == whole.resume
        for n in R.COUNTERS[:-1]:
            assert a.counters[n] + b.counters[n] == whole.counters[n], (k, n)
    seen = set()
    for cap in range(whole.counters["ts_packets"] + 1):     # every capacity: cuts at and inside every section
        a = R.encap(pdu, off, start=st, cap=cap, flush=True, **_kw(packing))
        assert a.counters["ts_packets"] == cap
        b = R.encap(pdu, off, start=a.resume, flush=True, **_kw(packing))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert b.resume == whole.resume
        m = len(R.partition(pdu, off, a.resume[0], 256, 2, True)[0][0][2]) if a.resume[0] < 40 else 0
        seen.add("fec" if a.resume[1] >= m and a.resume[2] > 12 else "fec header" if a.resume[1] >= m and
                 0 < a.resume[2] < 12 else "boundary" if a.resume[2] == 0 else "mpe")
    assert seen >= ({"fec", "boundary", "mpe", "fec header"} if packing else {"fec", "boundary"}), seen
    for mf in (1, 2, 3, 7):            # max_frames cuts
        rs = [R.encap(pdu, off, start=st, flush=True, max_frames=mf, **_kw(packing))]
        while not rs[-1].counters["flushed"]:
            assert len(rs) < 40 and rs[-1].counters["frames"] <= mf
            rs.append(R.encap(pdu, off, start=rs[-1].resume, flush=True, max_frames=mf, **_kw(packing)))
        np.testing.assert_array_equal(np.concatenate([r.ts for r in rs]), whole.ts)
        assert rs[-1].resume == whole.resume
        for n in R.COUNTERS[:-1]:
            assert sum(r.counters[n] for r in rs) == whole.counters[n], (mf, n)


def _params(**kw):
    p = _MpeFecParams()
    p.pid, p.mac_mode, p.packing, p.max_pdu_bytes, p.max_pdus = 0x100, 0, 1, 1 << 16, 1 << 10
    p.rows, p.data_columns, p.rs_columns, p.max_frames = 256, 191, 64, 4
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_capi_refuses_bad_parameters_before_the_device():
    L = dvbt2ll.lib()
    for n in ("create", "run_device", "get_result", "run_host", "destroy"):
        assert hasattr(L, "dvbt2ll_mpefec_" + n) and "dvbt2ll_mpefec_" + n in dvbt2ll.EXPORTS
    h = ctypes.c_void_p()
    bad = [_params(pid=-1), _params(pid=0x1FFF), _params(mac_mode=2), _params(packing=2), _params(packing=-1),
           _params(max_pdu_bytes=0), _params(max_pdu_bytes=1 << 31), _params(max_pdus=0),
           _params(max_pdus=(1 << 24) + 1), _params(rows=0), _params(rows=257), _params(rows=1280),
           _params(data_columns=0), _params(data_columns=192), _params(rs_columns=0), _params(rs_columns=65),
           _params(max_frames=0), _params(max_frames=(1 << 16) + 1)]
    for p in bad:
        assert L.dvbt2ll_mpefec_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value
    assert L.dvbt2ll_mpefec_create(None, 0, ctypes.byref(h)) == -1
    assert L.dvbt2ll_mpefec_create(ctypes.byref(_params()), 0, None) == -1
    pos, res = _MpeFecPos(), _MpeFecResult()
    assert L.dvbt2ll_mpefec_run_device(None, None, 1, None, 1, ctypes.byref(pos), None, 1, 0, None) == -1
    assert L.dvbt2ll_mpefec_run_host(None, None, 1, None, 1, ctypes.byref(pos), None, 1, 0, ctypes.byref(res)) == -1
    assert L.dvbt2ll_mpefec_get_result(None, ctypes.byref(res)) == -1
    L.dvbt2ll_mpefec_destroy(None)
    assert ctypes.sizeof(_MpeFecParams) == 56 and ctypes.sizeof(_MpeFecPos) == 24 and ctypes.sizeof(_MpeFecResult) == 112
    assert dvbt2ll.lib().dvbt2ll_abi_version() == 2


def test_capi_edevice_without_a_gpu():
    L = dvbt2ll.lib()
    if L.dvbt2ll_device_count() > 0:
        pytest.skip("a GPU is visible")
    h = ctypes.c_void_p()
    for p in (_params(), _params(mac_mode=1, packing=0, rows=1024, rs_columns=1)):
        assert L.dvbt2ll_mpefec_create(ctypes.byref(p), 0, ctypes.byref(h)) == -3 and not h.value   # EDEVICE
    with pytest.raises(dvbt2ll.DVBT2Error):
        dvbt2ll.MpeFecEncapsulator()
