"""GPU: the MISO pair chain (dvbt2ll_chain_create_miso_pair): both transmitter groups of one service from one FEC
+ map pass.  The expectation is the two single-group handles (MISO_TX1 and MISO_TX2_PROCESSED, each pinned to
the model by test_gpu_miso.py / test_gpu_chain.py), compared bit for bit; two shapes also check group 2 against
the 9.1 rule over the oracle and the CPU model of the GPU IFFT, so the pair path does not rest solely on code that
shares its planner."""
import ctypes
import dataclasses

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll import enums as E
from dvbt2ll._lib import check as _check
from dvbt2ll.configs import MPLP_CONFIGS, IF_CONFIGS, MISO_TX2_PROCESSED, ts_for_frames
import oracle_lib as O
from test_gpu_miso import CHAIN, chain_cfg, oracle_processed, _check_frames

pytestmark = pytest.mark.gpu


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int16) if x.dtype == np.int16 else x.view(np.uint32)


def _same(got, want, ctx):
    a, b = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert a.shape == b.shape, (ctx, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %s" % (ctx, bad.size, a.size, bad[:5])


def _tx1(cfg):
    return cfg.with_(misogroup=E.MISO_TX1)


def _tx2(cfg):
    return cfg.with_(misogroup=MISO_TX2_PROCESSED)


def _pair(cfg, max_frames):
    ch = dvbt2ll.Chain(_tx1(cfg), max_frames=max_frames, miso_pair=True)
    assert ch.ngroups == 2
    return ch


@pytest.fixture(scope="module")
def small(gpu):
    """the launch-form cases' shape with its pair handle, its two single-group handles and their two frames"""
    cfg = chain_cfg("4k_short_np2")
    n = 2
    pair = _pair(cfg, 2 * n)
    one = [dvbt2ll.Chain(c, max_frames=2 * n) for c in (_tx1(cfg), _tx2(cfg))]
    assert [c.ngroups for c in one] == [1, 1]
    want = {s: [c.run(0, n, seed=s) for c in one] for s in (1, 2)}
    return dict(cfg=cfg, n=n, pair=pair, one=one, want=want, per=pair.iq_per_frame)


@pytest.mark.parametrize("name", CHAIN)
def test_pair_equals_the_two_handles(gpu, name):
    cfg = chain_cfg(name)
    n = 2
    pair = _pair(cfg, n)
    g1, g2 = pair.run_groups(0, n)
    _same(g1, dvbt2ll.Chain(_tx1(cfg), max_frames=n).run(0, n), name + " group 1")
    _same(g2, dvbt2ll.Chain(_tx2(cfg), max_frames=n).run(0, n), name + " group 2")
    assert not np.array_equal(_bits(g1), _bits(g2))
    if name in ("4k_short_np2", "32k_pp2_tr_ext"):   # group 2 against the rule over the oracle
        ref, pg = oracle_processed(_tx2(cfg), 0, n)
        _check_frames(g2, pair.iq_per_frame, ref, pg, _tx2(cfg), name + " pair group 2")
    info = pair.info
    assert info == dvbt2ll.Chain(_tx1(cfg), max_frames=n).info


def _mplp_ts(m, first, n):
    from test_gpu_mplp import _device_ts
    bufs, bases, lens = _device_ts(m, first, n)
    return bufs, bases, lens


def _run_plps_pair(pair, m, first, n, groups=(True, True)):
    import torch
    bufs, bases, lens = _mplp_ts(m, first, n)
    out = [torch.empty((n * pair.iq_per_frame, 2), dtype=torch.float32, device="cuda") if g else None for g in groups]
    pair.run_plps_groups([b.data_ptr() for b in bufs], bases, lens, first, n,
                         [o.data_ptr() if o is not None else 0 for o in out], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy().view(np.complex64).reshape(-1) for o in out]


def _mplp_case(m, n):
    from test_gpu_mplp import _run
    m = m.with_(preamble=E.PREAMBLE_T2_MISO)
    pair = _pair(m, n)
    assert pair.nplp == len(m.plps)
    g1, g2 = _run_plps_pair(pair, m, 0, n)
    _same(g1, _run(dvbt2ll.Chain(_tx1(m), max_frames=n), _tx1(m), 0, n), m.name + " group 1")
    _same(g2, _run(dvbt2ll.Chain(_tx2(m), max_frames=n), _tx2(m), 0, n), m.name + " group 2")


def test_pair_multi_plp(gpu):
    _mplp_case(MPLP_CONFIGS["mplp2_8k"], 2)


def test_pair_frame_classes(gpu):
    m = IF_CONFIGS["ij2_4k_single"]
    m = m.with_(plps=(dataclasses.replace(m.plps[0], fecblocks=4, tiblocks=2),))
    assert m.unit_frames == 2
    _mplp_case(m, 2)


def test_pair_first_frame_above_zero(gpu):
    cfg = chain_cfg("4k_short_l1_16qam_v131")
    assert cfg.t2frames == 2
    g1, g2 = _pair(cfg, 2).run_groups(1, 2)
    _same(g1, dvbt2ll.Chain(_tx1(cfg), max_frames=2).run(1, 2), "first_frame 1 group 1")
    _same(g2, dvbt2ll.Chain(_tx2(cfg), max_frames=2).run(1, 2), "first_frame 1 group 2")


def _device_ts(cfg, n, seeds):
    import torch
    tss = [ts_for_frames(cfg, 0, n, seed=s) for s in seeds]
    assert all(t[1] == tss[0][1] and len(t[0]) == len(tss[0][0]) for t in tss)
    return torch.from_numpy(np.stack([t[0] for t in tss])).cuda(), tss[0][1], len(tss[0][0])


def test_pair_two_stream_batch(gpu, small):
    import torch
    n, per, pair = small["n"], small["per"], small["pair"]
    ts_d, base, ln = _device_ts(small["cfg"], n, (1, 2))
    out = [torch.empty((2 * n * per, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
    pair.run_groups_device(ts_d.data_ptr(), ts_d.stride(0), 2, base, ln, 0, n, [o.data_ptr() for o in out],
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for g in range(2):
        got = out[g].cpu().numpy().view(np.complex64).reshape(2, n * per)
        for s in range(2):
            _same(got[s], small["want"][s + 1][g], "group %d stream %d" % (g + 1, s))


def test_pair_odd_offsets(gpu, small):
    """an odd sample offset into a larger buffer, a different one for each group (the one-sample IQ stores)"""
    import torch
    n, per, pair = small["n"], small["per"], small["pair"]
    ts_d, base, ln = _device_ts(small["cfg"], n, (1,))
    offs = (1, 3)
    bufs = [torch.zeros((n * per + 8, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
    assert all(b.data_ptr() % 16 == 0 for b in bufs)
    pair.run_groups_device(ts_d.data_ptr(), 0, 1, base, ln, 0, n, [b.data_ptr() + 8 * o for b, o in zip(bufs, offs)],
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for g in range(2):
        got = bufs[g].cpu().numpy().view(np.complex64).reshape(-1)
        o = offs[g]
        _same(got[o:o + n * per], small["want"][1][g], "group %d at offset %d" % (g + 1, o))
        assert (got[:o] == 0).all() and (got[o + n * per:] == 0).all()


def test_pair_single_group_runs(gpu, small):
    """group 1 only and group 2 only (the other pointer NULL) equal the both-groups run"""
    n, pair = small["n"], small["pair"]
    g1, none = pair.run_groups(0, n, groups=(True, False))
    assert none is None
    _same(g1, small["want"][1][0], "group 1 alone")
    none, g2 = pair.run_groups(0, n, groups=(False, True))
    assert none is None
    _same(g2, small["want"][1][1], "group 2 alone")


def test_pair_sc16_gain(gpu, small):
    n, pair, one = small["n"], small["pair"], small["one"]
    try:
        for c in [pair] + one:
            c.set_output(0.2, dvbt2ll.IQ_SC16)
        g1, g2 = pair.run_groups(0, n)
        assert g1.dtype == np.int16 and g2.dtype == np.int16
        _same(g1, one[0].run(0, n), "sc16 group 1")
        _same(g2, one[1].run(0, n), "sc16 group 2")
    finally:
        for c in [pair] + one:
            c.set_output(1.0, dvbt2ll.IQ_CF32)


def test_pair_two_slots_alternating_streams(gpu, small):
    """set_slots(2), three back-to-back calls alternating two streams: a slot reused on the other stream waits
    for both OFDM launches of its previous run; every call's output checked"""
    import torch
    n, per, pair = small["n"], small["per"], small["pair"]
    ts = [_device_ts(small["cfg"], n, (s,)) for s in (1, 2, 1)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = [[torch.zeros((n * per, 2), dtype=torch.float32, device="cuda") for _ in range(2)] for _ in range(3)]
    torch.cuda.synchronize()
    pair.set_slots(2)
    try:
        for k in range(3):
            ts_d, base, ln = ts[k]
            pair.run_groups_device(ts_d.data_ptr(), 0, 1, base, ln, 0, n, [o.data_ptr() for o in out[k]],
                                   streams[k % 2].cuda_stream)
        torch.cuda.synchronize()
    finally:
        pair.set_slots(1)
    for k, seed in enumerate((1, 2, 1)):
        for g in range(2):
            _same(out[k][g].cpu().numpy().view(np.complex64).reshape(-1), small["want"][seed][g],
                  "call %d group %d" % (k, g + 1))


def test_pair_sync_errors_counted_once(gpu):
    cfg = chain_cfg("4k_short_np2")
    pair = _pair(cfg, 1)
    ts, base = ts_for_frames(cfg, 0, 1)
    ts = ts.copy()
    assert base == 0
    hit = [188 * k for k in (1, 3, 4)]     # packets whose sync byte the first frame consumes
    assert all(ts[i] == 0x47 for i in hit)
    ts[hit] = 0x48
    bb = O.BB(*cfg.bb_args())
    _, cons = bb.work(ts, cfg.fecblocks)
    assert cons > 188 * 5 and bb.sync_errors() == 3
    assert pair.sync_errors() == 0
    pair.run_groups(0, 1, ts=ts, ts_base=base)
    assert pair.sync_errors() == 3
    one = dvbt2ll.Chain(_tx1(cfg), max_frames=1)
    one.run(0, 1, ts=ts, ts_base=base)
    assert one.sync_errors() == 3


def test_pair_timing_and_debug_hooks(gpu, small):
    """set_timing: one FEC and one LDPC + map launch per run, stage 2 accumulating both OFDM launches as one
    interval; the debug hooks return group 1's slot order"""
    n, pair, one = small["n"], small["pair"], small["one"]
    pair.set_timing(True)
    try:
        pair.run_groups(0, n)
        ms, cnt = pair.timing()
    finally:
        pair.set_timing(False)
    assert cnt[:3] == [1, 1, 1] and all(m > 0 for m in ms[:3])
    # a group-2-only run: stage 2 is then the second launch alone, so the interval reaches past it (an interval
    # closed after group 1's launch would be empty here); and a group-1-only run
    for groups in ((False, True), (True, False)):
        pair.set_timing(True)
        try:
            pair.run_groups(0, n, groups=groups)
            ms1, cnt1 = pair.timing()
        finally:
            pair.set_timing(False)
        assert cnt1[:3] == [1, 1, 1] and ms1[2] > 0, groups
    S = pair.info["stream_items"]
    one[0].run(0, n)
    pair.run_groups(0, n)
    np.testing.assert_array_equal(pair.debug_cell_pairs(S), one[0].debug_cell_pairs(S))
    _same(pair.debug_cells(S), one[0].debug_cells(S), "debug cells")


def test_pair_refusals(gpu, small):
    """each refusal raises with nothing launched, and a following valid run is still bit-exact"""
    import torch
    cfg, n, per, pair, one = small["cfg"], small["n"], small["per"], small["pair"], small["one"]
    ts_d, base, ln = _device_ts(cfg, n, (1,))
    iq = [torch.zeros((n * per + 2, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
    st = torch.cuda.current_stream().cuda_stream
    p = [b.data_ptr() for b in iq]
    E_ = dvbt2ll.DVBT2Error
    # the single-output run calls on a pair handle
    with pytest.raises(E_):
        pair.run_device(ts_d.data_ptr(), base, ln, 0, n, p[0], st)
    with pytest.raises(E_):
        pair.run_streams(ts_d.data_ptr(), 0, 1, base, ln, 0, n, p[0], st)
    with pytest.raises(E_):
        pair.run_plps([ts_d.data_ptr()], [base], [ln], 0, n, p[0], st)
    with pytest.raises(E_):
        pair.run(0, n)
    host_out = np.zeros(n * per, np.complex64)
    host_in, host_base = ts_for_frames(cfg, 0, n)
    vp = ctypes.c_void_p
    with pytest.raises(E_):                                   # dvbt2ll_chain_run_plps_host
        _check(dvbt2ll.lib().dvbt2ll_chain_run_plps_host(
            pair._h, (vp * 1)(host_in.ctypes.data), (ctypes.c_int64 * 1)(host_base),
            (ctypes.c_int64 * 1)(len(host_in)), 0, n, host_out.ctypes.data_as(vp)), "run plps host")
    assert not host_out.any()
    host_ts, hb = ts_for_frames(cfg, 0, n)
    host_iq = np.zeros(n * per, np.complex64)
    with pytest.raises(E_):
        pair.run_host_pipelined(host_ts, hb, 0, n, host_iq)
    with pytest.raises(E_):
        pair.host_submit(host_ts.ctypes.data, hb, len(host_ts), 0, n, host_iq.ctypes.data)
    assert not host_iq.any()
    # graph mode
    with pytest.raises(E_):
        pair.set_graph(True)
    pair.set_graph(False)
    # the *_groups calls on an ordinary handle
    with pytest.raises(E_):
        one[0].run_groups_device(ts_d.data_ptr(), 0, 1, base, ln, 0, n, p, st)
    with pytest.raises(E_):
        one[1].run_plps_groups([ts_d.data_ptr()], [base], [ln], 0, n, p, st)
    # both pointers NULL; a misaligned pointer (either group)
    with pytest.raises(E_):
        pair.run_groups_device(ts_d.data_ptr(), 0, 1, base, ln, 0, n, [0, 0], st)
    with pytest.raises(E_):
        pair.run_groups_device(ts_d.data_ptr(), 0, 1, base, ln, 0, n, [p[0] + 4, p[1]], st)
    with pytest.raises(E_):
        pair.run_groups_device(ts_d.data_ptr(), 0, 1, base, ln, 0, n, [p[0], p[1] + 4], st)
    torch.cuda.synchronize()
    assert all(not b.any().item() for b in iq)   # nothing was launched
    # create: misogroup must be MISO_TX1, the preamble a MISO one; misogroup 3 keeps failing everywhere
    for bad in (_tx2(cfg), cfg.with_(misogroup=E.MISO_TX2), cfg.with_(misogroup=3),
                _tx1(cfg).with_(preamble=E.PREAMBLE_T2_SISO)):
        with pytest.raises(E_):
            dvbt2ll.Chain(bad, max_frames=1, miso_pair=True)
    with pytest.raises(E_):
        dvbt2ll.Chain(cfg.with_(misogroup=3), max_frames=1)
    # a valid run after all that
    g1, g2 = pair.run_groups(0, n)
    _same(g1, small["want"][1][0], "after refusals group 1")
    _same(g2, small["want"][1][1], "after refusals group 2")
    _same(one[0].run(0, n), small["want"][1][0], "ordinary handle after refusals")
