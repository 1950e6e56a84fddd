"""The chain's LDPC + map kernel (t2_kernels.hip ldpc_map_kernel: LDPC, codeword words to LDS over the dead LDPC
areas, map_cells, idx[-1], map_store_quads over the quad table) cell for cell and codeword for codeword against the
oracle, bit-exact, at the cases of tests/lm_cases.py: every code x constellation x rotation, and the TI, FFT-size
and frames-per-run shapes at which the quad store takes its other paths (tests/test_cpu_lm_cases.py proves on the
CPU that the cases reach them; tests/test_cpu_quad_table.py holds the table's contract)."""
import numpy as np
import pytest

import dvbt2ll
import lm_cases as LM

pytestmark = pytest.mark.gpu


def _check(ch, case, first_frame, keep=True, what=""):
    """one run of the case's frames from first_frame: the cells of every frame's data region and (keep) the
    packed codewords equal the oracle's; returns the cells"""
    cfg = case.cfg
    want, want_cw = LM.expected(case, first_frame)
    S = want.shape[1]
    ps = LM.pair_stride(S)
    ch.run(first_frame, case.frames)
    got = ch.debug_cells(case.frames * ps).reshape(case.frames, ps)[:, :S]
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (case.id, what, "cells", len(bad), bad[:8].tolist())
    if keep:
        nb = cfg.fecblocks * case.frames
        cw = ch.debug_codewords(nb)
        badb = np.nonzero((cw[:, :want_cw.shape[1]] != want_cw).any(axis=1))[0]
        assert badb.size == 0, (case.id, what, "codeword blocks", badb.tolist())
    return got.copy()


@pytest.mark.parametrize("case", LM.CODE_MATRIX, ids=[c.id for c in LM.CODE_MATRIX])
def test_ldpc_map_code_matrix(gpu, case):
    """every (framesize, rate) x QPSK .. 256-QAM x rotation off / on, 3 FEC blocks in TI blocks of 1 and 2"""
    ch = dvbt2ll.Chain(case.cfg, max_frames=case.frames)
    ch.debug_keep_codewords()
    _check(ch, case, 0)


@pytest.mark.parametrize("case", LM.SHAPES, ids=[c.id for c in LM.SHAPES])
def test_ldpc_map_shapes(gpu, case):
    """TI shapes, FFT sizes and frames per run on four codes, and on the same handle: a second run at the next
    frames (other TS bytes: wrong if the first run left BCH partial words behind, or if a frame offset leaks),
    the first frames again without the codeword hook (the hook does not perturb the map stage), and without
    rotation every index pair's two bytes equal"""
    ch = dvbt2ll.Chain(case.cfg, max_frames=case.frames)
    ch.debug_keep_codewords()
    first = _check(ch, case, 0, what="first run")
    second = _check(ch, case, case.frames, what="second run")
    assert not np.array_equal(first, second)
    ch.debug_keep_codewords(False)
    again = _check(ch, case, 0, keep=False, what="hook off")
    np.testing.assert_array_equal(again.view(np.uint64), first.view(np.uint64))
    if not case.cfg.rotation:
        S = first.shape[1]
        ps = LM.pair_stride(S)
        pairs = ch.debug_cell_pairs(case.frames * ps).reshape(case.frames, ps)[:, :S]
        assert ((pairs >> 8) == (pairs & 0xFF)).all(), case.id
