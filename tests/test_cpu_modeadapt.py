"""CPU: the mode-adapter reference (tests/modeadapt_ref.py) that the GPU adapter is compared with -- receiver after
adapter gives back the filtered TS, npd = 0 is the oracle's HEM BBFRAME stream, hand-derived known answers, the
resume property at every split point -- and the C ABI's refusals without a GPU."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, KBCH, ts_packets
from dvbt2ll._lib import _ModeAdaptParams, _ModeAdaptPos, _ModeAdaptResult
import bbch_cases as BC
import bbf_ref as BR
import modeadapt_cases as C
import modeadapt_ref as R


def test_crc8_is_the_oracles():
    rng = np.random.default_rng(1)
    for n in (0, 1, 9, 40):
        d = rng.integers(0, 256, n, dtype=np.uint8)
        assert R.crc8(d) == BR.crc8(d)


@pytest.mark.parametrize("kbch", [C.KBCH_SHORT14, C.KBCH_ODD])
@pytest.mark.parametrize("place", [0, 1, 2])
@pytest.mark.parametrize("run", C.RUNS)
def test_receiver_after_adapter_is_the_filtered_ts(run, place, kbch):
    """null runs of every interesting length at the buffer's start, middle and end: the receiver restores the TS
    (less the trailing nulls the flush dropped, which no BBFRAME mentions)"""
    ts = C.run_stream(run, place)
    r = R.adapt(ts, kbch, flush=True)
    dropped = r.counters["nulls_dropped_at_flush"]
    assert dropped == (run % 256 if place == 2 else 0)
    np.testing.assert_array_equal(R.receive(r.bbframes, kbch), R.filtered(ts)[:len(ts) - 188 * dropped])
    assert r.counters["nulls_kept"] == run // 256 and r.counters["selected"] == 24
    assert r.counters["nulls_deleted"] == run - run // 256 - dropped
    assert r.counters["packets_in"] == len(ts) // 188 and r.resume == (len(ts) // 188, 0, 0)
    assert BR.header_errors(kbch // 8, r.bbframes) == 0


def test_receiver_with_a_mask_and_without_deletion():
    ts = C.two_pid_stream()
    for pids in ([C.PID_A], [C.PID_B], [C.PID_A, C.PID_B]):
        m = R.mask_of(pids)
        r = R.adapt(ts, C.KBCH_SHORT14, mask=m, sis=False, isi=3, flush=True)
        assert r.bbframes[0] == 0xD4 and r.bbframes[1] == 3
        want = R.filtered(ts, 1, m)
        np.testing.assert_array_equal(R.receive(r.bbframes, C.KBCH_SHORT14),
                                      want[:len(ts) - 188 * r.counters["nulls_dropped_at_flush"]])
    r = R.adapt(ts, C.KBCH_ODD, npd=0, flush=True)
    np.testing.assert_array_equal(R.receive(r.bbframes, C.KBCH_ODD), R.filtered(ts, 0))


# the oracle builds no short 1/4 BBFRAME (its smallest Kbch is 5232, T2-Lite's short 1/3): that one anchors npd = 0
# at the small end, normal 3/4 (L = 6051) is the odd-L 64800 code
HEM_SMALL = CONFIGS["cfg1"].with_(rate=E.C1_3, fecblocks=3, inputmode=E.INPUTMODE_HIEFF)
HEM_ODD = CONFIGS["cfg4"].with_(rate=E.C3_4, fecblocks=2, inputmode=E.INPUTMODE_HIEFF)


@pytest.mark.parametrize("cfg", [HEM_SMALL, HEM_ODD], ids=["short-5232", "normal-48408"])
def test_npd0_is_the_oracles_hem_bbframe_stream(cfg):
    kbch = KBCH[(cfg.framesize, cfg.rate)]
    assert kbch == min(KBCH.values()) or (kbch // 8) % 2 == 1
    n = 4
    want = BR.oracle_bbframes(cfg, 0, n)
    nb = n * cfg.fecblocks
    ts = ts_packets(0, nb * (kbch - 80) // 8 // 187 + 2)
    r = R.adapt(ts, kbch, npd=0, cap=nb)
    np.testing.assert_array_equal(r.bbframes, want)
    syncd = r.bbframes.reshape(nb, -1)[:, 7:9]
    assert len({bytes(s) for s in syncd}) > 1          # the SYNCD phase moves


def test_known_answers_three_packets():
    """three selected packets, kbch 3072 (D = 374), 564 unit-stream bytes: frame 0 holds unit 0 and bytes 0 .. 185 of
    unit 1, SYNCD 0; the flush frame holds the 190 bytes left: bytes 186, 187 of unit 1, then unit 2, SYNCD 16"""
    ts = C.stream([(C.PID_A, 3)])
    r = R.adapt(ts, 3072, flush=True)
    f = r.bbframes.reshape(-1, 384)
    assert len(f) == 2 and r.counters["flushed"] == 1
    # F4: TS, SIS, CCM, NPD; UPL 0; DFL 2992 = 0x0BB0; SYNC 0; SYNCD 0; CRC-8 of F4 00 00 00 0B B0 00 00 00, XOR 1
    assert list(f[0][:9]) == [0xF4, 0, 0, 0, 0x0B, 0xB0, 0, 0, 0]
    assert f[0][9] == R.crc8([0xF4, 0, 0, 0, 0x0B, 0xB0, 0, 0, 0]) ^ 1
    np.testing.assert_array_equal(f[0][10:197], ts[1:188])
    assert f[0][197] == 0 and f[0][198] == ts[189]              # unit 0's DNP, then packet 1's byte 1
    # the flush frame: 3 * 188 - 374 = 190 bytes, DFL 1520 = 0x05F0; unit 2 begins 2 bytes in
    assert list(f[1][:9]) == [0xF4, 0, 0, 0, 0x05, 0xF0, 0, 0, 16]
    assert f[1][10] == ts[187 + 188] and f[1][11] == 0 and f[1][12] == ts[2 * 188 + 1]
    assert not f[1][10 + 190:].any()
    # without the flush: one frame, and the position is byte 186 of packet 1's unit
    r = R.adapt(ts, 3072)
    assert len(r.bbframes) == 384 and r.resume == (1, 186, 0) and r.counters["packets_in"] == 1
    # a data field no unit begins in: resume 184 bytes into a unit with 4 bytes left to flush
    r = R.adapt(ts[:188], 3072, start=(0, 184, 7), flush=True)
    assert list(r.bbframes[:9]) == [0xF4, 0, 0, 0, 0, 32, 0, 0xFF, 0xFF] and r.bbframes[13] == 7


def test_known_answers_kept_null():
    """one selected packet, 300 nulls, one selected: the null at r = 255 is transmitted with DNP 255 as the null
    packet, the last packet has DNP 300 - 256 = 44"""
    ts = C.stream([(C.PID_A, 1), (C.PID_NULL, 300), (C.PID_A, 1)])
    r = R.adapt(ts, 3072, flush=True)
    assert r.counters == dict(packets_in=302, selected=2, nulls_deleted=299, nulls_kept=1, nulls_dropped_at_flush=0,
                              sync_errors=0, bbframes=2, flushed=1)
    data = np.concatenate([f[10:] for f in r.bbframes.reshape(-1, 384)])[:3 * 188].reshape(3, 188)
    assert list(data[:, 187]) == [0, 255, 44]
    np.testing.assert_array_equal(data[1][:187], R.NULL_PACKET[1:])
    np.testing.assert_array_equal(data[2][:187], ts[301 * 188 + 1:])
    # a foreign packet in the kept position is sent as the null packet too
    ts = C.stream([(C.PID_A, 1), (C.PID_FOREIGN, 300), (C.PID_A, 1)])
    r2 = R.adapt(ts, 3072, mask=R.mask_of([C.PID_A]), flush=True)
    np.testing.assert_array_equal(r2.bbframes, r.bbframes)


def test_every_split_point_resumes_to_the_whole():
    ts = C.split_stream()
    n = len(ts) // 188
    for kbch, npd in ((C.KBCH_SHORT14, 1), (C.KBCH_SHORT14, 0), (5232, 1)):
        whole = R.adapt(ts, kbch, npd=npd, flush=True)
        for cut in range(n + 1):
            out, tot, pos = R.adapt_chunked(ts, kbch, [cut], npd=npd)
            np.testing.assert_array_equal(out, whole.bbframes, err_msg="cut %d" % cut)
            assert tot == whole.counters and pos == (n, 0, 0), (cut, tot, whole.counters)
    ts = C.long_run_stream()
    whole = R.adapt(ts, C.KBCH_SHORT14, flush=True)
    rng = np.random.default_rng(2)
    for cuts in [[258], [259], [300], [3 + 511], [3 + 512]] + [sorted(rng.integers(0, 710, 3)) for _ in range(20)]:
        out, tot, pos = R.adapt_chunked(ts, C.KBCH_SHORT14, [int(c) for c in cuts])
        np.testing.assert_array_equal(out, whole.bbframes, err_msg=str(cuts))
        assert tot == whole.counters, (cuts, tot, whole.counters)


def test_capacity_cut_then_continue():
    ts = C.run_stream(257, 1)
    whole = R.adapt(ts, C.KBCH_SHORT14, flush=True)
    for k in range(whole.counters["bbframes"] + 1):
        a = R.adapt(ts, C.KBCH_SHORT14, cap=k, flush=True)
        assert a.counters["bbframes"] == min(k, whole.counters["bbframes"])
        b = R.adapt(ts, C.KBCH_SHORT14, start=a.resume, flush=True)
        np.testing.assert_array_equal(np.concatenate([a.bbframes, b.bbframes]), whole.bbframes)
        assert {n: a.counters[n] + b.counters[n] for n in R.COUNTERS} == whole.counters


# ---------------------------------------------------------------------------------------- the C ABI without a GPU
def _params(**kw):
    p = _ModeAdaptParams()
    p.kbch, p.sis_mis, p.npd, p.max_ts_bytes = 3072, 1, 1, 188 * 64
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_capi_refuses_bad_parameters_before_the_device():
    L = dvbt2ll.lib()
    for n in ("create", "params_from_chain", "run_device", "get_result", "run_host", "destroy"):
        assert hasattr(L, "dvbt2ll_modeadapt_" + n)
    h = ctypes.c_void_p()
    mask = (ctypes.c_uint8 * 1024)()
    bad = [_params(kbch=3073), _params(kbch=0, framesize=0, rate=9), _params(kbch=0, framesize=2, rate=0),
           _params(npd=0, pid_mask=ctypes.addressof(mask)), _params(npd=2), _params(sis_mis=0, isi=256),
           _params(max_ts_bytes=187), _params(max_ts_bytes=188 * 3 + 1), _params(max_ts_bytes=1 << 31)]
    for p in bad:
        assert L.dvbt2ll_modeadapt_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value
    assert L.dvbt2ll_modeadapt_create(None, 0, ctypes.byref(h)) == -1
    if L.dvbt2ll_device_count() == 0:
        for p in (_params(), _params(kbch=0, framesize=1, rate=3), _params(pid_mask=ctypes.addressof(mask))):
            assert L.dvbt2ll_modeadapt_create(ctypes.byref(p), 0, ctypes.byref(h)) == -3 and not h.value   # EDEVICE
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.ModeAdapter(kbch=3072)
    # null handles and pointers
    pos, res = _ModeAdaptPos(), _ModeAdaptResult()
    assert L.dvbt2ll_modeadapt_run_device(None, None, 188, ctypes.byref(pos), None, 1, 0, None) == -1
    assert L.dvbt2ll_modeadapt_run_host(None, None, 187, ctypes.byref(pos), None, 1, 0, ctypes.byref(res)) == -1
    assert L.dvbt2ll_modeadapt_get_result(None, ctypes.byref(res)) == -1
    assert L.dvbt2ll_modeadapt_params_from_chain(None, 0, ctypes.byref(_params())) == -1
