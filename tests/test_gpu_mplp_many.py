"""GPU: the multi-PLP frames of tests/mplp_cases.py (4-8 PLPs, shared constellation tables, per-symbol PLP runs
shorter than one aligned load, a PLP skipped between two present ones; test_cpu_mplp_cases.py proves each claim on
the CPU) through the fused chain, its launch modes, the drop-in blocks and the MISO pair chain, bit-exact against
the oracle as test_gpu_mplp.py / test_gpu_ti.py / test_gpu_miso.py check their frames.

PARITY UNPINNED for nplp > 1 (the reference carries one PLP)."""
import ctypes
import functools

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll import enums as E
from dvbt2ll.configs import MISO_TX2_PROCESSED, ts_for_frames
import iq_check
import mplp_cases as MC
import oracle_lib as O
from test_gpu_mplp import _run, oracle_frames

pytestmark = pytest.mark.gpu

NAMES = list(MC.CASES)


@functools.lru_cache(maxsize=None)
def _ref(name, n):
    """the oracle's frames 0 .. n - 1 of a case, computed once and shared (read only)"""
    return oracle_frames(MC.CASES[name], n)


def _check_iq(iq, per, frames, pg, m, ctx):
    for k, (car, _) in enumerate(frames):
        f = iq[k * per:(k + 1) * per]
        iq_check.check_frame(f, car, pg.vlength, pg.guard, pg.normalization, pg.p1(), "%s frame %d" % (ctx, k))
        iq_check.check_frame_exact(f, car, m.pg_args(), pg.guard, pg.normalization, "%s frame %d" % (ctx, k))


@pytest.mark.parametrize("name", NAMES)
def test_many_chain_iq(gpu, name):
    """TS of every PLP -> IQ over two launch units (two T2 frames; four for skip_8k: both frame classes twice),
    every frame bit-exact against the CPU model of the GPU IFFT on the oracle's carriers and within SURVEY
    8(c)'s bounds of a float64 IFFT"""
    m = MC.CASES[name]
    n = 2 * m.unit_frames
    ref, pg, _, _ = _ref(name, n)
    ch = dvbt2ll.Chain(m, max_frames=n)
    assert ch.nplp == m.nplp and ch.unit_frames == m.unit_frames
    _check_iq(_run(ch, m, 0, n), ch.iq_per_frame, ref, pg, m, name)


@pytest.mark.parametrize("name", MC.MANY)
def test_many_chain_codewords(gpu, name):
    """every PLP's packed codewords (MIS BBHEADER with ISI = PLP_ID 0 .. 7, BCH, LDPC, parity interleave) equal
    the oracle's bbheaderbch (orc_bb_set_isi) + ldpc output"""
    import plan_probe as PP
    m = MC.CASES[name]
    _, _, _, cws = _ref(name, 2)
    ch = dvbt2ll.Chain(m, max_frames=1)
    ch.debug_keep_codewords()
    _run(ch, m, 0, 1)
    for k, p in enumerate(m.plps):
        got = ch.debug_plp_codewords(k, p.fecblocks)
        fp = PP.fec_plan(p.framesize, p.rate, p.constellation)
        nbch, q = fp["nbch"], fp["q"]
        nldpc = 64800 if p.framesize else 16200
        cw = cws[k][0].reshape(p.fecblocks, nldpc).copy()
        if fp["parity_il"]:
            t, s = np.divmod(np.arange(nldpc - nbch), 360)
            cw[:, nbch:] = cw[:, nbch + q * s + t]
        want = np.packbits(cw, axis=1)
        bad = np.nonzero((got[:, :nldpc // 8] != want).any(axis=1))[0]
        assert bad.size == 0, (name, "plp", k, bad.tolist())


def test_shared_launch_modes(gpu):
    """many8_8k_shared: frame 1 alone equals frame 1 of a batch; hipGraph mode, two replays; the sc16 output
    step against the numpy rounding of the cf32 samples"""
    name = "many8_8k_shared"
    m = MC.CASES[name]
    ref, pg, _, _ = _ref(name, 2)
    ch = dvbt2ll.Chain(m, max_frames=2)
    batch = _run(ch, m, 0, 2)
    per = ch.iq_per_frame
    _check_iq(batch, per, ref, pg, m, name)
    one = _run(ch, m, 1, 1)
    np.testing.assert_array_equal(one.view(np.uint32), batch[per:2 * per].view(np.uint32))
    ch.set_graph(True)
    for _ in range(2):
        np.testing.assert_array_equal(_run(ch, m, 0, 2).view(np.uint32), batch.view(np.uint32))
    ch.set_graph(False)
    ch.set_output(0.2, dvbt2ll.IQ_SC16)
    sc = _run(ch, m, 0, 2, fmt=dvbt2ll.IQ_SC16)
    want = np.clip(np.rint((batch.view(np.float32) * np.float32(0.2)) * np.float32(32767)), -32768,
                   32767).astype(np.int16)
    np.testing.assert_array_equal(sc.reshape(-1), want)


def test_all_pairs_blocks(gpu):
    """many8_8k_all through the drop-in blocks: eight per-PLP bbheaderbch (set_isi) -> ldpc -> interleavermod, the
    multi-PLP framemapper with eight ports (the block path's L1-post encoder at 1309 bits), pilotgen; each stage
    bit-exact against the oracle, two frames"""
    name = "many8_8k_all"
    m = MC.CASES[name]
    ref, pg, bits, cws = _ref(name, 2)
    cells_o, _, _ = O.mplp_cells(m, 0, 2)
    fmb = dvbt2ll.framemapper_mplp_cc(m)
    pgb = dvbt2ll.pilotgenp1insert_cc(*m.pg_args())
    assert fmb.output_multiple() == O.FMM(m).mapped_items
    assert fmb.forecast(fmb.output_multiple()) == [fmb.stream_items(k) for k in range(m.nplp)]
    chains = []
    for k, p in enumerate(m.plps):
        bb = dvbt2ll.bbheaderbch_bb(*p.bb_args())
        bb.set_isi(k)
        chains.append((bb, dvbt2ll.ldpc_bb(p.framesize, p.rate), dvbt2ll.interleavermod_bc(*p.im_args()),
                       ts_for_frames(p, 0, 2, seed=k + 1)[0]))
    offs = [0] * m.nplp
    for f in range(2):
        ports = []
        for k, (p, (bb, ld, im, ts)) in enumerate(zip(m.plps, chains)):
            F = p.fecblocks
            b = np.zeros(F * bb.output_multiple(), np.uint8)
            bb.general_work([ts[offs[k]:]], [b])
            offs[k] += bb.last_consumed
            np.testing.assert_array_equal(b, bits[k][f], err_msg="bb plp %d frame %d" % (k, f))
            c = np.zeros(F * ld.output_multiple(), np.uint8)
            ld.general_work([b], [c])
            np.testing.assert_array_equal(c, cws[k][f], err_msg="ldpc plp %d frame %d" % (k, f))
            x = np.zeros(F * im.output_multiple(), np.complex64)
            im.general_work([c], [x])
            assert len(x) == fmb.stream_items(k)
            ports.append(x)
        np.testing.assert_array_equal(np.concatenate(ports).view(np.uint32), cells_o[f].view(np.uint32))
        mapped = np.zeros(fmb.output_multiple(), np.complex64)
        assert fmb.general_work(ports, [mapped]) == len(mapped)
        assert fmb.last_consumed == [len(x) for x in ports]
        np.testing.assert_array_equal(mapped.view(np.uint32), ref[f][1].view(np.uint32), err_msg="frame %d" % f)
        iq = np.zeros(pgb.output_multiple(), np.complex64)
        pgb.general_work([mapped], [iq])
        iq_check.check_frame_exact(iq, ref[f][0], m.pg_args(), pg.guard, pg.normalization, "%s blocks %d" % (name, f))


def test_shared_miso_pair(gpu):
    """many8_8k_shared with a MISO preamble through the pair chain (chain_build_group2 over eight PLPs): group 1
    against the oracle's MISO_TX1 frame, group 2 against the 9.1 rule over the oracle, and both against the two
    single-group handles bit for bit (test_gpu_miso_pair._mplp_case)"""
    from test_gpu_miso import _oracle_mplp, _check_frames
    from test_gpu_miso_pair import _pair, _run_plps_pair, _same, _tx1, _tx2
    m = MC.CASES["many8_8k_shared"].with_(preamble=E.PREAMBLE_T2_MISO)
    n = 2
    pair = _pair(m, n)
    assert pair.nplp == 8
    g1, g2 = _run_plps_pair(pair, m, 0, n)
    per = pair.iq_per_frame
    ref1, pg1, _, _ = oracle_frames(_tx1(m), n)
    _check_iq(g1, per, ref1, pg1, _tx1(m), "pair group 1")
    ref2, pg2 = _oracle_mplp(_tx2(m), n)
    _check_frames(g2, per, ref2, pg2, _tx2(m), "pair group 2")
    _same(g1, _run(dvbt2ll.Chain(_tx1(m), max_frames=n), _tx1(m), 0, n), "group 1 against its own handle")
    _same(g2, _run(dvbt2ll.Chain(_tx2(m), max_frames=n), _tx2(m), 0, n), "group 2 against its own handle")


def test_tiny_miso_processed(gpu):
    """the MISO frame with a one-slot run inside a quad (mplp_cases.TINY_MISO), misogroup MISO_TX2_PROCESSED:
    scatter_slots<MISO> with the selector bit, against the 9.1 rule over the oracle"""
    from test_gpu_miso import _oracle_mplp, _check_frames
    m = MC.TINY_MISO
    assert m.misogroup == MISO_TX2_PROCESSED
    ref, pg = _oracle_mplp(m, 2)
    ch = dvbt2ll.Chain(m, max_frames=2)
    _check_frames(_run(ch, m, 0, 2), ch.iq_per_frame, ref, pg, m, m.name)


def test_all_pairs_l1post_across_frame_idx_wrap(gpu):
    """many8_8k_all in a superframe of three T2 frames, frames T - 2 .. T + 1 in one launch: the 1309-bit
    L1-post's FRAME_IDX and CRC-32 across the wrap"""
    m = MC.CASES["many8_8k_all"].with_(t2frames=3)
    first, n = m.t2frames - 2, 4
    ref, pg, _, _ = oracle_frames(m, first + n)
    ch = dvbt2ll.Chain(m, max_frames=n)
    iq = _run(ch, m, first, n)
    per = ch.iq_per_frame
    for k in range(n):
        iq_check.check_frame_exact(iq[k * per:(k + 1) * per], ref[first + k][0], m.pg_args(), pg.guard,
                                   pg.normalization, "frame %d" % (first + k))


def test_nine_plps_refused_eight_created(gpu):
    """the raw parameter array of test_cpu_mplp_cases with nplp = 8 creates a chain of eight PLPs; nplp = 9 is
    refused with nothing created"""
    from test_cpu_mplp_cases import raw_chain_params
    m = MC.CASES["many8_8k_all"]
    L = dvbt2ll.lib()
    h = ctypes.c_void_p()
    p = raw_chain_params(m, 8)
    assert L.dvbt2ll_chain_create_mplp(ctypes.byref(p), 0, ctypes.byref(h)) == 0 and h.value
    assert L.dvbt2ll_chain_num_plps(h) == 8
    L.dvbt2ll_chain_destroy(h)
    h = ctypes.c_void_p()
    p = raw_chain_params(m, 9)
    r = L.dvbt2ll_chain_create_mplp(ctypes.byref(p), 0, ctypes.byref(h))
    assert L.dvbt2ll_strerror(r) == b"invalid parameter combination" and not h.value
    with pytest.raises(AssertionError):
        dvbt2ll.Chain(m.with_(plps=m.plps + m.plps[:1]), max_frames=1)
