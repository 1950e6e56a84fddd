"""Case construction shared by tests/test_cpu_ofdm_cases.py (which proves on the CPU what the cases claim) and
the GPU tests of the OFDM kernels' less-travelled paths (t2_kernels.hip ofdm_kernel / ofdm32_kernel):
tests/test_gpu_ofdm_gather.py (the pilotgen block's gather mode, EQ at every size, arbitrary cells) and
tests/test_gpu_iq_dest.py (IQ destinations at odd sample offsets, write bounds).

  * PG_GRID: pilotgenp1insert argument sets (name, pg_args), deduplicated by pg_args;
  * SPECTRA: named generators of the block's input cells, f(active_items, rng) -> complex64: inputs an IFFT
    never sees from QAM data (no denormals, no NaN / Inf: flush behaviour is not their subject);
  * SPECTRUM_ENTRIES: per FFT size one PG_GRID entry, and the EQ entry of that size where there is one;
  * IQ_CLASS: for every (spectrum entry, spectrum) the float64 bound the IQ is held to -- the absolute
    SURVEY 8(c) bounds, or twice the error of an FFTW-class float IFFT where the signal is peaky;
    test_cpu_ofdm_cases.py asserts this literal is what it measures;
  * CHAIN_EQ: two full chain configs with EQ at N <= 16K.

Importable without a GPU.
"""
import numpy as np

from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS
import iq_check
from test_cpu_plan import BASE, BENCH_CFGS, GRID, grid_cfg

# ---------------------------------------------------------------------------------------------- PG_GRID
# points the feature grid and the bench configs leave out: EQ below 32K, the T2GI FFT sizes' own guard
# intervals, the remaining (FFT size, GI) corners, MISO TX2 / PAPR TR / T2-Lite at other sizes.  Pilot patterns
# are the ones EN 302 755 table 59 allows for the (FFT size, GI); none had to be replaced: the planner and the
# oracle accept every combination below.
EXTRA = [
    ("1k_pp2_eq", dict(fftsize=E.FFTSIZE_1K, pilotpattern=E.PILOT_PP2, guardinterval=E.GI_1_8, numdatasyms=4,
                       equalization=E.EQUALIZATION_ON)),
    ("8k_pp7_eq_7mhz", dict(fftsize=E.FFTSIZE_8K, pilotpattern=E.PILOT_PP7, guardinterval=E.GI_1_32, numdatasyms=3,
                            equalization=E.EQUALIZATION_ON, bandwidth=E.BANDWIDTH_7_0_MHZ)),
    ("16k_pp4_ext_eq", dict(fftsize=E.FFTSIZE_16K, pilotpattern=E.PILOT_PP4, guardinterval=E.GI_1_16, numdatasyms=2,
                            carriermode=E.CARRIERS_EXTENDED, equalization=E.EQUALIZATION_ON)),
    ("16k_t2gi_pp2_19_128", dict(fftsize=E.FFTSIZE_16K_T2GI, pilotpattern=E.PILOT_PP2, guardinterval=E.GI_19_128,
                                 numdatasyms=3)),
    ("32k_t2gi_pp4_19_256", dict(fftsize=E.FFTSIZE_32K_T2GI, pilotpattern=E.PILOT_PP4, guardinterval=E.GI_19_256,
                                 numdatasyms=2)),
    ("32k_pp8_19_128", dict(fftsize=E.FFTSIZE_32K, pilotpattern=E.PILOT_PP8, guardinterval=E.GI_19_128,
                            numdatasyms=2)),
    ("16k_pp1_gi14", dict(fftsize=E.FFTSIZE_16K, pilotpattern=E.PILOT_PP1, guardinterval=E.GI_1_4, numdatasyms=4)),
    ("1k_pp4_gi116", dict(fftsize=E.FFTSIZE_1K, pilotpattern=E.PILOT_PP4, guardinterval=E.GI_1_16, numdatasyms=4)),
    ("2k_pp7_gi132", dict(fftsize=E.FFTSIZE_2K, pilotpattern=E.PILOT_PP7, guardinterval=E.GI_1_32, numdatasyms=4)),
    ("2k_pp1_miso_tx2", dict(fftsize=E.FFTSIZE_2K, pilotpattern=E.PILOT_PP1, guardinterval=E.GI_1_4, numdatasyms=4,
                             preamble=E.PREAMBLE_T2_MISO, misogroup=E.MISO_TX2)),
    ("8k_pp3_tr", dict(fftsize=E.FFTSIZE_8K, pilotpattern=E.PILOT_PP3, guardinterval=E.GI_1_8, numdatasyms=4,
                       paprmode=E.PAPR_TR)),
    ("16k_t2lite_pp5", dict(fftsize=E.FFTSIZE_16K, pilotpattern=E.PILOT_PP5, guardinterval=E.GI_1_16, numdatasyms=3,
                            preamble=E.PREAMBLE_T2_LITE_SISO)),
]


def _pg_grid():
    # grid_cfg only settles fecblocks / tiblocks, which pg_args() does not carry: BASE.with_(**over) gives the
    # same arguments without the planner's capacity search (test_cpu_ofdm_cases checks they are equal)
    pts = [(n, BASE.with_(**o).pg_args()) for n, o in GRID] + [(n, CONFIGS[n].pg_args()) for n in BENCH_CFGS] + \
          [(n, BASE.with_(**o).pg_args()) for n, o in EXTRA]
    seen, out = set(), []
    for name, args in pts:
        args = tuple(int(a) for a in args)
        if args not in seen:
            seen.add(args)
            out.append((name, args))
    return out


PG_GRID = _pg_grid()
PG_BY_NAME = dict(PG_GRID)


def pg_fft(args):
    return int(args[11])


def pg_eq(args):
    return int(args[9])


# ---------------------------------------------------------------------------------------------- SPECTRA
def _one(n, at):
    c = np.zeros(n, np.complex64)
    c[at] = 1 + 0.5j
    return c


def _wide_range(n, rng):
    mag = np.exp2(rng.uniform(-20.0, 10.0, n))
    return (mag * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, n))).astype(np.complex64)


def _neg_zero(n, rng):
    c = np.empty(2 * n, np.float32)
    c[:] = -0.0
    return c.view(np.complex64)


SPECTRA = {
    "zeros": lambda n, rng: np.zeros(n, np.complex64),                       # pilots only
    "first_cell": lambda n, rng: _one(n, 0),
    "last_cell": lambda n, rng: _one(n, n - 1),
    "neg_zero": _neg_zero,
    "alternating": lambda n, rng: np.where(np.arange(n) % 2 == 0, 1.0, -1.0).astype(np.complex64),
    "constant": lambda n, rng: np.full(n, 0.7 - 0.7j, np.complex64),
    "wide_range": _wide_range,
    "random": lambda n, rng: (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) *
                             np.float32(np.sqrt(0.5)),
}


def cells(spectrum, active_items, seed):
    """the cells of `spectrum` for a block consuming active_items per frame (deterministic in seed)"""
    c = SPECTRA[spectrum](active_items, np.random.default_rng(seed))
    assert c.dtype == np.complex64 and c.shape == (active_items,)
    return c


# per FFT size: a small non-EQ entry and, where PG_GRID has one, the EQ entry (few symbols each)
SPECTRUM_ENTRIES = ["1k_pp4_gi116", "1k_pp2_eq", "2k_pp7_gi132", "4k_grc", "8k_pp3_tr", "8k_pp7_eq_7mhz",
                    "16k_t2lite_pp5", "16k_pp4_ext_eq", "32k_pp8_19_128", "32k_pp7_eq"]
# SPECTRA left out of a spectrum entry because the CPU model of the kernels misses its bound there (at most one
# per FFT size; test_cpu_ofdm_cases.test_left_out_pairs_miss_their_bound keeps the figures honest).
#   8k_pp7_eq_7mhz / alternating: the frame closing symbol carries no scattered pilots, so the +1, -1 cells are
#   contiguous carriers and add up to one sample of 42 x rms.  The model is 2.6e-7 off relative to that sample
#   (about 2 ulp: the kernels' twiddles are products of table values, each within a few ulp), pocketfft 0.8e-7:
#   max error 1.09e-5 of rms against 3.33e-6, beyond the absolute 1e-5 and the 2 x cap alike.  A finding about
#   the model's (= the kernels') twiddle accuracy at a coherent peak, not about gather mode or EQ.
LEFT_OUT = {"8k_pp7_eq_7mhz": ("alternating",)}


def spectrum_cells(spectrum, active_items):
    """the cells the classification was measured on (seed = the spectrum's position in SPECTRA)"""
    return cells(spectrum, active_items, list(SPECTRA).index(spectrum))


def kept_spectra(entry):
    return [s for s in SPECTRA if s not in LEFT_OUT.get(entry, ())]


# ---------------------------------------------------------------------------------------------- IQ bound
TIGHT, PEAKY = "tight", "peaky"
PEAKY_FACTOR = 2.0   # the project's recorded worst ratio to pocketfft is 1.74 (profiles/r6_r6i_summary.md), plus headroom


def classify(f32_rel, f32_max):
    """tight: an FFTW-class float IFFT stays within half of the absolute 8(c) bounds on these carriers, so the
    absolute bounds apply; peaky: the signal's max / rms is so large (energy in a few samples) that it does not,
    and the bound is PEAKY_FACTOR x that IFFT's own two errors"""
    return TIGHT if f32_rel <= iq_check.REL_RMS_MAX / 2 and f32_max <= iq_check.MAX_REL_MAX / 2 else PEAKY


def symbol_errors(y, carriers, N, G, norm):
    """(rel rms, max / rms) of one symbol y against the float64 IFFT, and the same of numpy's complex64 pocketfft"""
    want = iq_check.symbol_reference(carriers, N, G, norm)
    return iq_check.errors(y, want), iq_check.f32_reference_errors(carriers, N, G, norm, want)


def worst_errors(iq_symbols, carriers, N, G, norm):
    """over the symbols of a frame (iq_symbols: the frame without its P1): the worst (rel, max) of the IQ and of
    pocketfft; each error is relative to its own symbol"""
    m = [0.0, 0.0]
    f = [0.0, 0.0]
    for j in range(carriers.shape[0]):
        (rel, mx), (frel, fmx) = symbol_errors(iq_symbols[j * (N + G):(j + 1) * (N + G)], carriers[j], N, G, norm)
        m = [max(m[0], rel), max(m[1], mx)]
        f = [max(f[0], frel), max(f[1], fmx)]
    return tuple(m), tuple(f)


def class_limits(cls, f32):
    """the (rel rms, max / rms) limits class `cls` assigns, given pocketfft's two errors on the same carriers"""
    if cls == TIGHT:
        return iq_check.REL_RMS_MAX, iq_check.MAX_REL_MAX
    return PEAKY_FACTOR * f32[0], PEAKY_FACTOR * f32[1]


def check_class_bound(cls, iq_symbols, carriers, N, G, norm, ctx):
    """the float64 bound class `cls` assigns to the pair: the worst errors over the frame's symbols against the
    absolute bounds, or against PEAKY_FACTOR x pocketfft's worst on the same carriers"""
    m, f = worst_errors(iq_symbols, carriers, N, G, norm)
    lim = class_limits(cls, f)
    assert m[0] <= lim[0] and m[1] <= lim[1], "%s (%s): IQ rel rms %.3g (<= %.3g), max %.3g of rms (<= %.3g)" % (
        ctx, cls, m[0], lim[0], m[1], lim[1])
    return m, f


# (spectrum entry, spectrum) -> class, as test_cpu_ofdm_cases.test_classification_literal measures it
_T8 = dict.fromkeys(SPECTRA, TIGHT)
IQ_CLASS = {
    "1k_pp4_gi116": {**_T8},
    "1k_pp2_eq": {**_T8},
    "2k_pp7_gi132": {**_T8},
    "4k_grc": {**_T8},
    "8k_pp3_tr": {**_T8, "constant": PEAKY},
    "8k_pp7_eq_7mhz": {**_T8, "constant": PEAKY},
    "16k_t2lite_pp5": {**_T8, "constant": PEAKY},
    "16k_pp4_ext_eq": {**_T8, "alternating": PEAKY, "constant": PEAKY},
    "32k_pp8_19_128": {**_T8, "constant": PEAKY},
    "32k_pp7_eq": {**_T8, "constant": PEAKY},
}

# ---------------------------------------------------------------------------------------------- chain EQ
# EQ through the fused chain's scatter mode at N <= 16K (sub_ifft's isinc multiply after the LDS scatter)
CHAIN_EQ = [
    ("8k_pp7_eq_chain", dict(fftsize=E.FFTSIZE_8K, pilotpattern=E.PILOT_PP7, guardinterval=E.GI_1_32, numdatasyms=3,
                             equalization=E.EQUALIZATION_ON, bandwidth=E.BANDWIDTH_7_0_MHZ)),
    ("2k_pp2_eq_chain", dict(fftsize=E.FFTSIZE_2K, pilotpattern=E.PILOT_PP2, guardinterval=E.GI_1_8, numdatasyms=4,
                             equalization=E.EQUALIZATION_ON, constellation=E.MOD_16QAM, rate=E.C1_2)),
]


def chain_eq_cfg(name):
    return grid_cfg(dict(CHAIN_EQ)[name])
