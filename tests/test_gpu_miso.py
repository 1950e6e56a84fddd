"""GPU: MISO processing of transmitter group 2's payload cells (EN 302 755 9.1; misogroup =
MISO_TX2_PROCESSED) through the C ABI: the fused chain's scatter mode (the OFDM kernels' MISO instantiations:
selector bit of the slot bins, of the indirect L1-post entries, host-flipped direct aux values) and the
pilotgen block's gather mode.  Expected values: the 9.1 rule in numpy (tests/miso_ref.py) on the unmodified
oracle's frame mapper cells, through the oracle's pilot stage (group 2) and the CPU model of the GPU IFFT.

PARITY UNPINNED: the reference has no MISO processing block.  Every misogroup = 2 case differs from the
unprocessed group 2 output (asserted), whose own expectation is checked next to it."""
import dataclasses
import types

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll import enums as E
from dvbt2ll.configs import MPLP_CONFIGS, IF_CONFIGS, MISO_TX2_PROCESSED, ts_for_frames
import iq_check
import miso_ref as MR
import ofdm_cases as C
import oracle_lib as O
from test_cpu_miso import MISO, SINGLE, BASE, _fit, single_cfg
from test_gpu_chain import _check_chain

pytestmark = pytest.mark.gpu

# the chain's shapes: test_cpu_miso's (1K, 2K with BPSK L1, 4K short with N_P2 = 2, 4K with 16-QAM L1 and v1.3.1
# L1 scrambling, T2-Lite, 8K, 16K TR, 32K TR, 32K extended rotated 256-QAM with EQ) and 32K TR extended
CHAIN = list(SINGLE) + ["32k_pp2_tr_ext"]
EXTRA = {"32k_pp2_tr_ext": dict(SINGLE["32k_pp2_tr"], carriermode=E.CARRIERS_EXTENDED)}


def chain_cfg(name):
    if name in SINGLE:
        return single_cfg(name)
    over = dict(MISO)
    over.update(EXTRA[name])
    return _fit(BASE.with_(**over))


def oracle_processed(cfg, first, nframes, seed=1):
    """the expected carriers of frames [first, first + nframes) of a processed single-PLP configuration"""
    ts, _ = ts_for_frames(cfg, 0, first + nframes, seed)
    F = cfg.fecblocks
    bb, ld, im = O.BB(*cfg.bb_args()), O.LDPC(cfg.framesize, cfg.rate), O.IM(*cfg.im_args())
    fm, pg = O.FM(*cfg.fm_args()), O.PG(*MR.tx2_args(cfg))
    off, out = 0, []
    for k in range(first + nframes):
        bits, cons = bb.work(ts[off:], F)
        off += cons
        mapped = fm.work(im.work(ld.work(bits, F), F))   # (every frame: the oracle's FRAME_IDX advances per call)
        if k >= first:
            out.append(MR.expected_carriers(mapped, cfg, pg))
    return out, pg


def _check_frames(iq, per, ref, pg, cfg, ctx, gain=1.0, fmt=0):
    for k, car in enumerate(ref):
        f = iq[k * per:(k + 1) * per]
        iq_check.check_frame_exact(f, car, MR.tx2_args(cfg), pg.guard, pg.normalization, "%s frame %d" % (ctx, k),
                                   gain=gain, fmt=fmt)
        if fmt == 0 and gain == 1.0:
            iq_check.check_frame(f, car, pg.vlength, pg.guard, pg.normalization, pg.p1(), "%s frame %d" % (ctx, k))


@pytest.mark.parametrize("name", CHAIN)
def test_chain_iq_processed(gpu, name):
    """two consecutive frames (two FRAME_IDX values' L1-post cells): bit-exact against the model, within
    iq_check's float64 bounds; and not the unprocessed group 2 frame"""
    cfg = chain_cfg(name)
    ref, pg = oracle_processed(cfg, 0, 2)
    ch = dvbt2ll.Chain(cfg, max_frames=2)
    iq = ch.run(0, 2)
    _check_frames(iq, ch.iq_per_frame, ref, pg, cfg, name)
    plain = dvbt2ll.Chain(cfg.with_(misogroup=E.MISO_TX2), max_frames=1).run(0, 1)
    assert not np.array_equal(plain.view(np.uint32), iq[:ch.iq_per_frame].view(np.uint32))


@pytest.mark.parametrize("name", CHAIN)
def test_chain_iq_group2_unprocessed_as_before(gpu, name):
    """the same configurations with misogroup = 1: the oracle's own group 2 frame, as before"""
    _check_chain(chain_cfg(name).with_(misogroup=E.MISO_TX2), 1)


def test_chain_first_frame_above_zero(gpu):
    """frames 1 and 2 of a two-frame superframe (FRAME_IDX 1, then 0) computed alone"""
    cfg = chain_cfg("4k_short_l1_16qam_v131")
    assert cfg.t2frames == 2
    ref, pg = oracle_processed(cfg, 1, 2)
    ch = dvbt2ll.Chain(cfg, max_frames=2)
    _check_frames(ch.run(1, 2), ch.iq_per_frame, ref, pg, cfg, "first_frame 1")


def _run_plps(ch, m, first, n):
    from test_gpu_mplp import _run
    return _run(ch, m, first, n)


def _oracle_mplp(m, n):
    cells, _, _ = O.mplp_cells(m, 0, n)
    fm, pg = O.FMM(m), O.PG(*MR.tx2_args(m))
    return [MR.expected_carriers(fm.work(c), m, pg) for c in cells], pg


def test_chain_multi_plp(gpu):
    """a two-PLP MISO frame: the kernels' MULTI + MISO instantiation"""
    m = MPLP_CONFIGS["mplp2_8k"].with_(**MISO)
    ref, pg = _oracle_mplp(m, 2)
    ch = dvbt2ll.Chain(m, max_frames=2)
    assert ch.nplp == 2
    _check_frames(_run_plps(ch, m, 0, 2), ch.iq_per_frame, ref, pg, m, "mplp2_8k")


def test_chain_frame_classes(gpu):
    """FRAME_INTERVAL 2 over one launch unit: the even frame carries the PLP, the odd one dummy cells only"""
    m = IF_CONFIGS["ij2_4k_single"].with_(**MISO)
    m = m.with_(plps=(dataclasses.replace(m.plps[0], fecblocks=4, tiblocks=2),))
    assert m.unit_frames == 2
    ref, pg = _oracle_mplp(m, 2)
    ch = dvbt2ll.Chain(m, max_frames=2)
    _check_frames(_run_plps(ch, m, 0, 2), ch.iq_per_frame, ref, pg, m, "ij2_4k")


@pytest.mark.parametrize("name", ["4k_short_np2", "32k_pp2_tr"])
def test_chain_launch_forms(gpu, name):
    """a 2-stream batch, hipGraph mode, sc16 with gain 0.2 and an odd sample offset, against the direct cf32 run
    (itself against the model in test_chain_iq_processed); sc16 also against its model"""
    import torch
    cfg = chain_cfg(name)
    n = 2
    ch = dvbt2ll.Chain(cfg, max_frames=2 * n)
    per = ch.iq_per_frame
    direct = [ch.run(0, n, seed=s) for s in (1, 2)]
    # 2-stream batch, stream-major
    tss = [ts_for_frames(cfg, 0, n, seed=s) for s in (1, 2)]
    assert tss[0][1] == tss[1][1] and len(tss[0][0]) == len(tss[1][0])
    ts_d = torch.from_numpy(np.stack([t[0] for t in tss])).cuda()
    iq_d = torch.empty((2 * n * per, 2), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ch.run_streams(ts_d.data_ptr(), ts_d.stride(0), 2, tss[0][1], len(tss[0][0]), 0, n, iq_d.data_ptr(), st)
    torch.cuda.synchronize()
    got = iq_d.cpu().numpy().view(np.complex64).reshape(2, n * per)
    for s in range(2):
        np.testing.assert_array_equal(got[s].view(np.uint32), direct[s].view(np.uint32), err_msg="stream %d" % s)
    # an odd sample offset (the one-sample IQ stores)
    buf = torch.zeros((n * per + 4, 2), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ch.run_device(ts_d.data_ptr(), tss[0][1], len(tss[0][0]), 0, n, buf.data_ptr() + 8, st)
    torch.cuda.synchronize()
    odd = buf.cpu().numpy().view(np.complex64).reshape(-1)
    np.testing.assert_array_equal(odd[1:1 + n * per].view(np.uint32), direct[0].view(np.uint32))
    assert odd[0] == 0 and (odd[1 + n * per:] == 0).all()
    # hipGraph mode: capture, then relaunch
    ch.set_graph(True)
    for _ in range(2):
        np.testing.assert_array_equal(ch.run(0, n).view(np.uint32), direct[0].view(np.uint32))
    ch.set_graph(False)
    # sc16, gain 0.2: the direct run's samples through the output step, and the model's
    ch.set_output(0.2, dvbt2ll.IQ_SC16)
    sc = ch.run(0, n)
    want = np.clip(np.rint((direct[0].view(np.float32) * np.float32(0.2)) * np.float32(32767)), -32768,
                   32767).astype(np.int16)
    np.testing.assert_array_equal(sc.reshape(-1), want)
    ref, pg = oracle_processed(cfg, 0, n)
    _check_frames(sc, per, ref, pg, cfg, name + " sc16", gain=0.2, fmt=1)


# ---------------------------------------------------------------- the pilotgen block (gather mode)
def _pg_namespace(args):
    keys = ("carriermode", "fftsize", "pilotpattern", "guardinterval", "numdatasyms", "paprmode", "version",
            "preamble", "misogroup", "equalization", "bandwidth", "vlength")
    ns = types.SimpleNamespace(**dict(zip(keys, args)))
    ns.pg_args = lambda: tuple(args)
    return ns


def _words_equal(got, want, ctx):
    a, b = np.ascontiguousarray(got).view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    assert a.shape == b.shape, (ctx, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %s" % (ctx, bad.size, a.size, bad[:5])


@pytest.mark.parametrize("entry", ["4k_t2lite_miso_tx2", "32k_pp2_miso_tx2_tr"])
def test_pilotgen_block_processed(gpu, entry):
    """the drop-in block with misogroup = 2 on the cfg grid's MISO arguments: the carriers hook as bit patterns
    (zeros and -0 cells come out with the rule's signed zeros) and the frame's IQ against the model"""
    a = list(C.PG_BY_NAME[entry])
    assert a[8] == E.MISO_TX2
    pg = O.PG(*a)
    p1 = pg.p1()
    plain = dvbt2ll.pilotgenp1insert_cc(*a)
    a[8] = MISO_TX2_PROCESSED
    ns = _pg_namespace(a)
    blk = dvbt2ll.pilotgenp1insert_cc(*a)
    assert blk.output_multiple() == pg.output_items and blk.active_items() == pg.active_items
    for s in ("zeros", "first_cell", "neg_zero", "random"):
        ctx = "%s / %s" % (entry, s)
        cells = C.spectrum_cells(s, pg.active_items)
        want = MR.expected_carriers(cells, ns, pg)
        _words_equal(blk.debug_carriers(cells, pg.num_symbols, pg.vlength), want, ctx + " carriers")
        iq = np.zeros(pg.output_items, np.complex64)
        assert blk.general_work([cells], [iq]) == pg.output_items
        _words_equal(iq, O.model_frame(want, pg.guard, pg.normalization, p1), ctx)
        # misogroup = 1 beside it: the oracle's own group 2 carriers
        _words_equal(plain.debug_carriers(cells, pg.num_symbols, pg.vlength), pg.carriers(cells), ctx + " group 2")
    assert not np.array_equal(want.view(np.uint32), pg.carriers(cells).view(np.uint32))


def test_create_refuses_bad_values(gpu):
    ok = chain_cfg("4k_short_np2")
    for bad in (ok.with_(preamble=E.PREAMBLE_T2_SISO), ok.with_(misogroup=3), ok.with_(misogroup=-1)):
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.Chain(bad, max_frames=1)
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.pilotgenp1insert_cc(*bad.pg_args())
    m = MPLP_CONFIGS["mplp2_8k"].with_(misogroup=MISO_TX2_PROCESSED)   # SISO preamble
    with pytest.raises(dvbt2ll.DVBT2Error):
        dvbt2ll.Chain(m, max_frames=1)
