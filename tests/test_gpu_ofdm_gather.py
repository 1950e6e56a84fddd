"""GPU: the OFDM kernels' gather mode (the drop-in pilotgenp1insert_cc block: t2_kernels.hip ofdm32_kernel's
direct-load branch with eq(v, 32, 1, 0) and Dft<32>, ofdm_kernel / sub_ifft's non-inv BinSource) across the
parameter space, the inverse-sinc EQ multiply at every FFT size, and cells QAM data never produces.

The block API takes arbitrary complex cells, so it is where the IFFT can be fed adversarial spectra.  Every
expected value comes from the CPU oracle (carriers) and the CPU model of the kernels' IFFT
(oracle/ifft_model.c) or a float64 IFFT; tests/test_cpu_ofdm_cases.py proves the cases and the bound classes.
The two chain configs at the end run EQ through the fused chain's scatter mode at N <= 16K."""
import numpy as np
import pytest

import dvbt2ll
import iq_check
import ofdm_cases as C
import oracle_lib as O
from test_gpu_chain import _check_chain

pytestmark = pytest.mark.gpu


def _oracle(args):
    return O.PG(*args)


def _frame(blk, pg, cells):
    iq = np.zeros(pg.output_items, np.complex64)
    assert blk.general_work([cells], [iq]) == pg.output_items
    assert blk.last_consumed == pg.active_items
    return iq


def _assert_words_equal(got, want, ctx):
    a, b = got.view(np.uint32).reshape(-1), want.view(np.uint32).reshape(-1)
    assert a.shape == b.shape, (ctx, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %s" % (ctx, bad.size, a.size, bad[:5])


@pytest.mark.parametrize("k", range(len(C.PG_GRID)), ids=[n for n, _ in C.PG_GRID])
def test_gather_grid(gpu, k):
    """every PG_GRID entry through the block: carriers (the carriers-only hook: gather rows, EQ) bit-exact, the
    frame's IQ bit-exact against the CPU model and within the 8(c) bounds of a float64 IFFT, the block's item
    counts the oracle's"""
    name, args = C.PG_GRID[k]
    pg = _oracle(args)
    blk = dvbt2ll.pilotgenp1insert_cc(*args)
    assert blk.output_multiple() == pg.output_items
    assert blk.active_items() == pg.active_items
    cells = C.cells("random", pg.active_items, k)
    want_car = pg.carriers(cells)
    got_car = blk.debug_carriers(cells, pg.num_symbols, pg.vlength)
    _assert_words_equal(got_car, want_car, "gather carriers " + name)
    iq = _frame(blk, pg, cells)
    iq_check.check_frame_exact(iq, want_car, args, pg.guard, pg.normalization, "gather " + name)
    iq_check.check_frame(iq, want_car, pg.vlength, pg.guard, pg.normalization, pg.p1(), "gather " + name)


@pytest.mark.parametrize("entry", C.SPECTRUM_ENTRIES)
def test_gather_spectra(gpu, entry):
    """per FFT size (and its EQ entry): every kept spectrum through one handle -- carriers bit-exact, IQ bit-exact
    against the CPU model, and within the float64 bound its class assigns (absolute, or 2 x pocketfft measured
    here on the same carriers)"""
    args = C.PG_BY_NAME[entry]
    pg = _oracle(args)
    blk = dvbt2ll.pilotgenp1insert_cc(*args)
    p1 = pg.p1()
    for s in C.kept_spectra(entry):
        ctx = "gather %s / %s" % (entry, s)
        cells = C.spectrum_cells(s, pg.active_items)
        want_car = pg.carriers(cells)
        _assert_words_equal(blk.debug_carriers(cells, pg.num_symbols, pg.vlength), want_car, ctx + " carriers")
        iq = _frame(blk, pg, cells)
        _assert_words_equal(iq, O.model_frame(want_car, pg.guard, pg.normalization, p1), ctx)
        iq_check.check_p1(iq[:2048], p1, ctx)
        m, f = C.check_class_bound(C.IQ_CLASS[entry][s], iq[2048:], want_car, pg.vlength, pg.guard, pg.normalization,
                                   ctx)
        print("%s %s: IQ rel %.3g max %.3g, pocketfft rel %.3g max %.3g" % (ctx, C.IQ_CLASS[entry][s], *m, *f))


@pytest.mark.parametrize("entry", ["1k_pp4_gi116", "32k_pp8_19_128"])
def test_gather_handle_reuse(gpu, entry):
    """two general_work calls on one handle, random cells then zeros: the second frame is the pilots-only frame
    of the model, bit for bit -- nothing of the first call survives in the handle's reused device buffers or in
    the kernels' LDS"""
    args = C.PG_BY_NAME[entry]
    pg = _oracle(args)
    blk = dvbt2ll.pilotgenp1insert_cc(*args)
    p1 = pg.p1()
    first = None
    for s in ("random", "zeros"):
        cells = C.spectrum_cells(s, pg.active_items)
        iq = _frame(blk, pg, cells)
        _assert_words_equal(iq, O.model_frame(pg.carriers(cells), pg.guard, pg.normalization, p1),
                            "reuse %s call %s" % (entry, s))
        if first is None:
            first = iq
    assert not np.array_equal(first, iq)
    # and the hook after a full run, on the same buffers
    cells = C.spectrum_cells("first_cell", pg.active_items)
    _assert_words_equal(blk.debug_carriers(cells, pg.num_symbols, pg.vlength), pg.carriers(cells), "reuse carriers")


@pytest.mark.parametrize("name", [n for n, _ in C.CHAIN_EQ])
def test_chain_eq_small_fft(gpu, name):
    """EQ through the fused chain at N <= 16K: sub_ifft's isinc multiply on the values read back from the LDS
    scatter (before this, EQ ran at 32K only)"""
    cfg = C.chain_eq_cfg(name)
    assert cfg.equalization and cfg.vlength <= 16384
    _check_chain(cfg, 2)
