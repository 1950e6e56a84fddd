"""CPU: the cases of tests/ofdm_cases.py do what they claim, before the GPU tests rely on them.

  * every PG_GRID entry is a configuration the oracle and the planner both accept, and the planner's gather
    rows (what ofdm_kernel / ofdm32_kernel read in gather mode) give the oracle's carriers bit for bit;
  * the spectra are what their names say (finite, normal numbers only);
  * for every (spectrum entry, spectrum) the CPU model of the kernels (oracle/ifft_model.c) is put against a
    float64 IFFT and numpy's complex64 pocketfft on the same carriers; the pair's class -- tight (absolute
    SURVEY 8(c) bounds) or peaky (2 x pocketfft) -- is what ofdm_cases.IQ_CLASS says, and the model meets it.

No GPU needed."""
import functools

import numpy as np
import pytest

import iq_check
import ofdm_cases as C
import oracle_lib as O
import plan_probe as PP
from test_cpu_plan import BASE, GRID, _apply, grid_cfg

IDS = [n for n, _ in C.PG_GRID]


def test_grid_covers_what_it_claims():
    """distinct argument sets; the feature grid's and the bench configs' pilotgen arguments are all there (as
    grid_cfg gives them); the added points: EQ at 1K, 8K, 16K (one off 8 MHz), both T2GI sizes with their own
    guard intervals, 32K 19/128, 16K 1/4, 1K 1/16, 2K 1/32, MISO TX2 at 2K, PAPR TR at 8K, T2-Lite at 16K, each
    with at most 4 data symbols"""
    from dvbt2ll import enums as E
    from dvbt2ll.configs import CONFIGS
    args = [a for _, a in C.PG_GRID]
    assert len(set(args)) == len(args) and len(set(IDS)) == len(IDS)
    for name, over in GRID[:6]:     # the rest alike: pg_args() carries neither fecblocks nor tiblocks
        assert tuple(grid_cfg(over).pg_args()) == tuple(BASE.with_(**over).pg_args())
    for _, over in GRID:
        assert tuple(int(a) for a in BASE.with_(**over).pg_args()) in args
    for n in ("cfg1", "cfg1q", "cfg2", "cfg3", "cfg4", "cfg5"):
        assert tuple(int(a) for a in CONFIGS[n].pg_args()) in args
    # (carriermode, fftsize, pilotpattern, guardinterval, numdatasyms, paprmode, version, preamble, misogroup,
    #  equalization, bandwidth, vlength)
    extra = [C.PG_BY_NAME[n] for n, _ in C.EXTRA]
    assert all(a[4] <= 4 for a in extra)
    eq = {a[11]: a[10] for a in extra if a[9]}
    assert set(eq) == {1024, 8192, 16384} and any(bw != E.BANDWIDTH_8_0_MHZ for bw in eq.values())

    def has(**kw):
        idx = dict(fftsize=1, guardinterval=3, paprmode=5, preamble=7, misogroup=8)
        return any(all(a[idx[k]] == v for k, v in kw.items()) for a in extra)

    assert has(fftsize=E.FFTSIZE_16K_T2GI, guardinterval=E.GI_19_128)
    assert has(fftsize=E.FFTSIZE_32K_T2GI, guardinterval=E.GI_19_256)
    assert has(fftsize=E.FFTSIZE_32K, guardinterval=E.GI_19_128)
    assert has(fftsize=E.FFTSIZE_16K, guardinterval=E.GI_1_4)
    assert has(fftsize=E.FFTSIZE_1K, guardinterval=E.GI_1_16)
    assert has(fftsize=E.FFTSIZE_2K, guardinterval=E.GI_1_32)
    assert has(fftsize=E.FFTSIZE_2K, preamble=E.PREAMBLE_T2_MISO, misogroup=E.MISO_TX2)
    assert has(fftsize=E.FFTSIZE_8K, paprmode=E.PAPR_TR)
    assert has(fftsize=E.FFTSIZE_16K, preamble=E.PREAMBLE_T2_LITE_SISO)
    # spectrum entries: every FFT size, and the EQ entry of every size that has one
    sizes = {C.pg_fft(C.PG_BY_NAME[e]) for e in C.SPECTRUM_ENTRIES}
    assert sizes == {1024, 2048, 4096, 8192, 16384, 32768}
    eq_sizes = {C.pg_fft(a) for a in args if C.pg_eq(a)}
    assert {C.pg_fft(C.PG_BY_NAME[e]) for e in C.SPECTRUM_ENTRIES if C.pg_eq(C.PG_BY_NAME[e])} == eq_sizes
    for N in sizes:     # at most one spectrum left out per FFT size
        assert len({s for e, ss in C.LEFT_OUT.items() if C.pg_fft(C.PG_BY_NAME[e]) == N for s in ss}) <= 1


@pytest.mark.parametrize("k", range(len(C.PG_GRID)), ids=IDS)
def test_grid_entry_plans_and_matches_oracle(k):
    """O.PG creates, the planner's pilot plan builds, and its gather rows applied to random cells (with the
    inverse-sinc factors where EQ is on) are the oracle's carriers, bit for bit"""
    name, args = C.PG_GRID[k]
    pg = O.PG(*args)
    plan = PP.pilot_plan(args)
    assert plan is not None, "the planner refuses " + name
    assert (plan["active"], plan["Nsym"], plan["G"], plan["N"]) == (pg.active_items, pg.num_symbols, pg.guard, pg.vlength)
    assert plan["Nsym"] * (plan["N"] + plan["G"]) + 2048 == pg.output_items
    assert plan["eq"] == C.pg_eq(args)
    cells = C.cells("random", plan["active"], k)
    want = pg.carriers(cells)
    aux = np.zeros(16, np.complex64)
    aux[1:13] = plan["pilot_values"]
    N = plan["N"]
    kk = np.arange(N)
    used = np.zeros(plan["active"], bool)
    for j in range(plan["Nsym"]):
        code = plan["bin_map"][j]
        used[code[code >= 0]] = True
        row = _apply(code, cells, aux)
        bins = np.empty(N, np.complex64)
        bins[(kk + N // 2) % N] = row
        if plan["eq"]:
            bins = (bins.view(np.float32).reshape(-1, 2) * plan["isinc"][:, None]).view(np.complex64).reshape(-1)
        np.testing.assert_array_equal(bins.view(np.uint32), want[j].view(np.uint32), err_msg="%s symbol %d" % (name, j))
    assert used.all()       # every input cell lands on a carrier (first_cell / last_cell are seen)
    assert abs(plan["norm"] - pg.normalization) == 0


def test_spectra_are_what_they_say():
    n = 1001
    for i, s in enumerate(C.SPECTRA):
        c = C.cells(s, n, i)
        f = c.view(np.float32)
        assert np.isfinite(f).all()
        assert ((f == 0) | (np.abs(f) >= np.finfo(np.float32).tiny)).all(), s    # no denormals
        np.testing.assert_array_equal(C.cells(s, n, i).view(np.uint32), c.view(np.uint32))   # deterministic
    z = C.cells("zeros", n, 0).view(np.uint32)
    assert not z.any()
    assert (C.cells("neg_zero", n, 0).view(np.uint32) == 0x80000000).all()
    for s, at in (("first_cell", 0), ("last_cell", n - 1)):
        c = C.cells(s, n, 0)
        assert c[at] == np.complex64(1 + 0.5j) and np.count_nonzero(c) == 1
    a = C.cells("alternating", n, 0)
    assert (a[0::2] == 1).all() and (a[1::2] == -1).all()
    assert (C.cells("constant", n, 0) == np.complex64(0.7 - 0.7j)).all()
    w = np.abs(C.cells("wide_range", 20000, 3).astype(np.complex128))
    assert 2.0 ** -20 * 0.999 <= w.min() < 2.0 ** -19 and 2.0 ** 9 < w.max() <= 2.0 ** 10 * 1.001
    lg = np.log2(w)
    assert abs(np.mean(lg) + 5) < 0.3 and abs(np.std(lg) - 30 / np.sqrt(12)) < 0.3      # log-uniform
    r = C.cells("random", 20000, 4).astype(np.complex128)
    assert abs(np.mean(np.abs(r) ** 2) - 1) < 0.03 and abs(np.mean(r)) < 0.03


@pytest.mark.parametrize("name,over", C.CHAIN_EQ, ids=[n for n, _ in C.CHAIN_EQ])
def test_chain_eq_configs_plan(name, over):
    """the chain-mode EQ configs carry a FEC block, have EQ on at N <= 16K, and the fused chain's layout and aux
    lists for them rebuild the oracle's carriers (test_cpu_plan's checks on these two points)"""
    import test_cpu_plan as TP
    cfg = C.chain_eq_cfg(name)
    assert cfg.equalization and cfg.vlength <= 16384 and cfg.fecblocks >= 1
    assert PP.pilot_plan(cfg.pg_args())["eq"] == 1
    TP.test_chain_cell_layout_matches_oracle(name, over)
    TP.test_chain_aux_lists_match_cmap(name, over)
    TP.test_l1post_plan_matches_host_encoder(name, over)


PAIRS = [(e, s) for e in C.SPECTRUM_ENTRIES for s in C.SPECTRA]


@functools.lru_cache(maxsize=None)
def _measure(entry, spectrum):
    """worst (rel rms, max / rms) over the frame's symbols of the model and of pocketfft"""
    args = C.PG_BY_NAME[entry]
    pg = O.PG(*args)
    car = pg.carriers(C.spectrum_cells(spectrum, pg.active_items))
    y = O.model_symbols(car, pg.guard, pg.normalization)
    return C.worst_errors(y, car, pg.vlength, pg.guard, pg.normalization)


def test_classification_literal():
    """ofdm_cases.IQ_CLASS is the classification measured here (the GPU tests apply the same rule)"""
    got = {e: {s: C.classify(*_measure(e, s)[1]) for s in C.SPECTRA} for e in C.SPECTRUM_ENTRIES}
    assert got == C.IQ_CLASS


@pytest.mark.parametrize("entry,spectrum", [p for p in PAIRS if p[1] in C.kept_spectra(p[0])],
                         ids=["%s-%s" % p for p in PAIRS if p[1] in C.kept_spectra(p[0])])
def test_model_meets_class_bound(entry, spectrum):
    """tight pairs: the model within the absolute 8(c) bounds of the float64 IFFT; peaky pairs: within 2 x
    pocketfft's two errors"""
    m, f = _measure(entry, spectrum)
    cls = C.IQ_CLASS[entry][spectrum]
    lim = C.class_limits(cls, f)
    print("%s %s %s: model rel %.3g max %.3g, pocketfft rel %.3g max %.3g" % (entry, spectrum, cls, *m, *f))
    assert m[0] <= lim[0] and m[1] <= lim[1], (entry, spectrum, cls, m, f, lim)


def test_left_out_pairs_miss_their_bound():
    """the pairs ofdm_cases.LEFT_OUT drops are findings about the model, not conveniences: each one misses the
    bound its class assigns (so it cannot be tested bit-exactly against the model AND against float64), and it
    comes back into the tests as soon as the model meets it.
    Measured: 8k_pp7_eq_7mhz / alternating (tight): model rel rms 2.12e-7, max 1.09e-5 of rms (bound 1e-5; 2 x
    pocketfft would be 6.7e-6); pocketfft rel rms 1.36e-7, max 3.33e-6.  The worst sample is the 42 x rms peak of
    the frame closing symbol, 2.6e-7 off relative to its own magnitude."""
    for entry, spectra in C.LEFT_OUT.items():
        for s in spectra:
            m, f = _measure(entry, s)
            lim = C.class_limits(C.IQ_CLASS[entry][s], f)
            print("%s %s: model rel %.3g max %.3g, pocketfft rel %.3g max %.3g" % (entry, s, *m, *f))
            assert m[0] > lim[0] or m[1] > lim[1], "%s / %s meets its bound now: take it out of LEFT_OUT" % (entry, s)
            # still a sane IFFT: within 4 x pocketfft
            assert m[0] <= 4 * f[0] and m[1] <= 4 * f[1]
