"""T2-MI output without a GPU: the reference framer (tests/t2mi_out_ref.py) against the independent receiver
t2mi_ref.parse, its closed-form packet count, the edges its aux sweep must contain, the numpy restatement for long
streams, and the C ABI's refusals."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _T2miOutParams, _T2miOutPos, _T2miOutResult
import t2mi_out_ref as O
import t2mi_ref as R

SMALL = [(O.Shape([(0, O.LB_SMALL, F)]), n) for F in (1, 2, 3) for n in (1, 2, 5)] + \
        [(O.Shape([(9, O.LB_ODD, F)]), n) for F in (1, 2) for n in (1, 3)] + \
        [(sh, n) for sh in O.EDGE_SHAPES + [O.THREE_PLPS] for n in (1, 2, 4)]


@pytest.mark.parametrize("sh", O.EDGE_SHAPES + [O.THREE_PLPS, O.Shape([(0, O.LB_SMALL, 2)])])
def test_parse_returns_every_bbframe(sh):
    n, start = 4, (29, 250, 13)
    bb, aux = sh.inputs(n)
    ts, nxt, cnt, by_type = O.frame(sh, bb, aux, n, start)
    res = R.parse(ts, sh.pid, [(p[0], p[1]) for p in sh.plps])
    assert len(res.packets) == n * sh.P == cnt["t2mi_packets"]
    assert (res.packets["flags"] == R.F_COMPLETE | R.F_CONSISTENT | R.F_CRC_OK | R.F_ACCEPTED).all()
    for k in R.TS_COUNTERS + R.PKT_COUNTERS:
        want = len(ts) // 188 if k == "ts_contributing" else n * sh.P if k == "accepted" else 0
        assert res.counters[k] == want, k
    for k, p in enumerate(sh.plps):
        np.testing.assert_array_equal(res.bbframes[k], bb[k])
        assert R.interleaving_frames(res.packets, k) == [p[2]] * n
    assert res.by_type == by_type and res.resume == (len(ts), 0)
    assert (res.packets["packet_count"] == (250 + np.arange(n * sh.P)) & 255).all()
    assert (res.packets["t2mi_stream_id"] == sh.stream_id).all()
    fr = 29 + np.repeat(np.arange(n), sh.P)
    assert (res.packets["superframe_idx"] == (fr // sh.fps) & 15).all()
    bbp = res.packets["packet_type"] == 0
    assert (res.packets["frame_idx"][bbp] == (fr % sh.fps)[bbp]).all()
    assert nxt == (29 + n, (250 + n * sh.P) & 255, (13 + len(ts) // 188) & 15)


def test_closed_form_ts_packet_count():
    shapes = [s for s, _ in SMALL[::3]] + [s for s, _ in O.aux_sweep_cases()[::7]]
    for sh in shapes:
        bb, aux = sh.inputs(6)
        for n in range(1, 7):
            assert O.ts_packets(sh, n) == len(O.frame(sh, bb, aux, n)[0]) // 188, (sh.aux, sh.plps, n)


def test_aux_sweep_contains_every_edge():
    """the case list the GPU test reuses: every pointer_field 0 .. 182 (so every entry state), the shortened
    183-byte packet without PUSI, three or more starts inside one TS packet, final stuffing 0, 1, 2 and > 100"""
    ptrs, short, most, final = set(), 0, 0, set()
    for sh, n in O.aux_sweep_cases():
        bb, aux = sh.inputs(n)
        e = O.edges_of(O.frame(sh, bb, aux, n)[0])
        ptrs |= e["pointers"]
        short += e["shortened"]
        most = max(most, e["most_starts"])
        final.add(e["final_stuff"])
    assert ptrs == set(range(183))
    assert short >= 1 and most >= 3
    assert {0, 1, 2} <= final and max(final) > 100


def test_numpy_restatement_equals_the_sequential_framer():
    for sh, n in SMALL + O.aux_sweep_cases():
        bb, aux = sh.inputs(n, seed=n)
        start = (7 * n, 251, 14)
        a, b = O.frame(sh, bb, aux, n, start), O.frame_numpy(sh, bb, aux, n, start)
        np.testing.assert_array_equal(a[0], b[0], err_msg=str((sh.plps, sh.aux, n)))
        assert a[1:] == b[1:]


def test_numpy_restatement_sees_a_dropped_carry():
    """the long-stream shape, shortened: without the carry of d from frame to frame the bytes differ"""
    sh = O.Shape([(0, O.LB_SMALL, 1)])
    bb, aux = sh.inputs(40)
    good, bad = O.frame_numpy(sh, bb, aux, 40)[0], O.frame_numpy(sh, bb, aux, 40, carry=False)[0]
    np.testing.assert_array_equal(good, O.frame(sh, bb, aux, 40)[0])
    assert len(bad) != len(good) or not np.array_equal(bad, good)
    assert np.array_equal(bad[:188 * 3], good[:188 * 3])       # the first frame is laid out alike


def _params(**kw):
    p = _T2miOutParams()
    p.pid, p.nplp, p.frames_per_superframe, p.max_frames = 0x1000, 1, 2, 4
    p.plp_id[0], p.bbframe_bytes[0], p.blocks_per_frame[0] = 0, 654, 1
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                if k == "aux":
                    p.aux[i].packet_type, p.aux[i].payload_bits, p.aux[i].after = x
                else:
                    getattr(p, k)[i] = x
        else:
            setattr(p, k, v)
    return p


def test_capi_refuses_bad_parameters_before_the_device():
    L = dvbt2ll.lib()
    for n in ("create", "params_from_chain", "ts_packets", "run_device", "get_result", "run_host", "destroy"):
        assert hasattr(L, "dvbt2ll_t2mi_out_" + n) and "dvbt2ll_t2mi_out_" + n in dvbt2ll.EXPORTS
    h = ctypes.c_void_p()
    bad = [_params(pid=-1), _params(pid=0x1FFF), _params(nplp=0), _params(nplp=9), _params(bbframe_bytes=[655]),
           _params(bbframe_bytes=[0]), _params(blocks_per_frame=[0]), _params(plp_id=[256]),
           _params(nplp=2, plp_id=[4, 4], bbframe_bytes=[654, 654], blocks_per_frame=[1, 1]),
           _params(naux=5), _params(naux=-1), _params(naux=1, aux=[(0x20, 0, 0)]), _params(naux=1, aux=[(0x20, 65536, 0)]),
           _params(naux=1, aux=[(256, 8, 0)]), _params(naux=1, aux=[(0x20, 8, 2)]), _params(t2mi_stream_id=8),
           _params(frames_per_superframe=0), _params(frames_per_superframe=257), _params(max_frames=0),
           _params(max_frames=1 << 23)]
    for i, p in enumerate(bad):
        assert L.dvbt2ll_t2mi_out_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value, i
    assert L.dvbt2ll_t2mi_out_create(None, 0, ctypes.byref(h)) == -1
    assert L.dvbt2ll_t2mi_out_create(ctypes.byref(_params()), 0, None) == -1
    if L.dvbt2ll_device_count() == 0:
        for p in (_params(), _params(naux=4, aux=[(0x20, 88, 0), (0x10, 203, 0), (1, 1, 1), (2, 65535, 1)])):
            assert L.dvbt2ll_t2mi_out_create(ctypes.byref(p), 0, ctypes.byref(h)) == -3 and not h.value   # EDEVICE
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.T2miFramer(0x1000, plps=[(0, 654, 1)])
    with pytest.raises(dvbt2ll.DVBT2Error):
        dvbt2ll.T2miFramer(0x1000, plps=[(0, 654, 1)], aux=[(0x20, 8, 0)] * 5)
    pos, res = _T2miOutPos(), _T2miOutResult()
    assert L.dvbt2ll_t2mi_out_run_device(None, None, None, 0, None, ctypes.byref(pos), 1, None, 1, None) == -1
    assert L.dvbt2ll_t2mi_out_run_host(None, None, None, 0, None, ctypes.byref(pos), 1, None, 1, ctypes.byref(res)) == -1
    assert L.dvbt2ll_t2mi_out_get_result(None, ctypes.byref(res)) == -1
    assert L.dvbt2ll_t2mi_out_ts_packets(None, 1) == -1
    assert L.dvbt2ll_t2mi_out_params_from_chain(None, None, ctypes.byref(_params())) == -1
    L.dvbt2ll_t2mi_out_destroy(None)
    assert ctypes.sizeof(_T2miOutParams) == 168 and ctypes.sizeof(_T2miOutResult) == 2104
    assert dvbt2ll.lib().dvbt2ll_abi_version() == 2
