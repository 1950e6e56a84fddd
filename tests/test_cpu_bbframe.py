"""CPU: BBFRAME input of the chain (dvbt2ll_chain_set_input).  The numpy reference of tests/bbf_ref.py against the
oracle for every code, the header CRC rule on the oracle's own headers, the closed-form input span, and the new
C symbols without a GPU."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, KBCH, bbframe_span
import bbch_cases as C
import bbf_ref as R

CODES = [(1, r) for r in range(6)] + [(0, r) for r in range(8)]


@pytest.mark.parametrize("framesize,rate", CODES)
def test_numpy_reference_matches_oracle(framesize, rate):
    """descramble the oracle's BBFRAMEs, encode them with the independent reference: the oracle's bbheaderbch bits
    (scrambling and BCH parity) come back, for all 14 codes, 3 blocks each"""
    cfg = CONFIGS["cfg3"].with_(framesize=framesize, rate=rate, fecblocks=3)
    bbf = R.oracle_bbframes(cfg, 0, 1)
    assert bbf.size == 3 * KBCH[(framesize, rate)] // 8
    np.testing.assert_array_equal(R.encode_ref(framesize, rate, bbf), C.oracle_bits(cfg, 0, 1))


def test_bbframe_span_closed_form():
    cfg = CONFIGS["cfg3"]
    L, F = 38688 // 8, cfg.fecblocks
    assert L == 4836
    assert bbframe_span(cfg, 0, 1) == (0, F * L)
    assert bbframe_span(cfg, 0, 7) == (0, 7 * F * L)
    assert bbframe_span(cfg, 3, 2) == (3 * F * L, 5 * F * L)
    K = 5000   # above 2^32
    lo, end = bbframe_span(cfg, K, 2)
    assert lo == K * F * L and lo > 1 << 32 and end - lo == 2 * F * L and lo % L == 0
    c1 = C.SWEEPS["nm"][0]
    assert bbframe_span(c1, 2, 4) == (2 * 8 * 879, 6 * 8 * 879)


def test_library_exports_input_symbols_without_gpu():
    lib = dvbt2ll.lib()
    for s in ("dvbt2ll_chain_set_input", "dvbt2ll_chain_get_input", "dvbt2ll_chain_bbheader_errors"):
        assert hasattr(lib, s) and s in dvbt2ll.EXPORTS
    assert (dvbt2ll.INPUT_TS, dvbt2ll.INPUT_BBFRAME) == (0, 1)


def test_set_input_null_handle_is_einval():
    lib = dvbt2ll.lib()
    assert lib.dvbt2ll_chain_set_input(None, 0, 1) == -1   # DVBT2LL_EINVAL
    assert lib.dvbt2ll_chain_get_input(None, 0) == -1
    n = ctypes.c_int64(5)
    assert lib.dvbt2ll_chain_bbheader_errors(None, ctypes.byref(n)) == -1


@pytest.mark.parametrize("name", ["nm", "hem", "nm-inband"])
def test_oracle_headers_satisfy_crc_rule(name):
    """the rule bbheader_errors counts by: byte 9 of every header the oracle builds is the CRC-8 of bytes 0 .. 8 in
    normal mode and that value XOR 1 in high-efficiency mode"""
    cfg, _ = C.SWEEPS[name]
    L = R.bbframe_len(cfg)
    frames = R.oracle_bbframes(cfg, 0, 4).reshape(-1, L)
    assert len(frames) == 4 * cfg.fecblocks
    mode = 1 if cfg.inputmode != E.INPUTMODE_NORMAL else 0
    for f in frames:
        assert R.crc8(f[:9]) ^ mode == int(f[9])
    assert R.header_errors(L, frames) == 0
    bad = frames.copy()
    bad[1, 3] ^= 0x10
    bad[5, 9] ^= 0x02
    bad[6, 9] ^= 0x01   # the mode bit alone: not an error
    assert R.header_errors(L, bad) == 2
