"""CPU: the cases of tests/lm_cases.py reach what tests/test_gpu_ldpc_map.py runs them for.  Everything here is
computed from the planner's probed quad tables and plans, without a GPU: a layout change that takes a claimed
shape away from the GPU test fails here."""
import numpy as np
import pytest

from dvbt2ll import enums as E
from dvbt2ll.configs import ts_for_frames
import oracle_lib as O
import plan_probe as PP
import lm_cases as LM


@pytest.fixture(scope="module")
def tables():
    """the probed quad table of every case (cases of one configuration share it)"""
    out, by_cfg = {}, {}
    for c in LM.ALL_CASES:
        key = c.cfg.with_(rotation=0, name="")   # the table does not depend on the rotation
        if key not in by_cfg:
            by_cfg[key] = PP.quad_table(key)
        out[c.id] = by_cfg[key]
    return out


def test_case_lists():
    assert len(LM.CODE_MATRIX) == 112 and len({c.id for c in LM.ALL_CASES}) == len(LM.ALL_CASES)
    seen = {(c.cfg.framesize, c.cfg.rate, c.cfg.constellation, c.cfg.rotation) for c in LM.CODE_MATRIX}
    assert seen == {(fs, r, m, rot) for fs, r in LM.ALL_CODES for m in LM.CONSTS for rot in (0, 1)}
    for c in LM.CODE_MATRIX:
        assert (c.cfg.fecblocks, c.cfg.tiblocks, c.frames) == (3, 2, 1)
    assert len(LM.SHAPES) == 4 * len(LM.TI_SHAPES) + len(LM.FFT_GRID) + len(LM.FRAME_COUNTS)
    ffts = {c.cfg.fftsize for c in LM.SHAPES if "-fft" in c.id}
    assert ffts == {E.FFTSIZE_1K, E.FFTSIZE_2K, E.FFTSIZE_4K, E.FFTSIZE_16K, E.FFTSIZE_32K}


def test_every_case_plans(tables):
    for c in LM.ALL_CASES:
        q = tables[c.id]
        assert q is not None, c.id
        plan = PP.frame_plan(c.cfg.fm_args())
        assert plan is not None and (q["rows"], q["unit"]) == (c.cfg.fecblocks, 1), c.id
        ti = (plan["ti_on"], plan["ti_small"], plan["ti_big"], plan["ti_nsmall"])
        if c in LM.CODE_MATRIX:
            assert ti == (1, 1, 2, 1), c.id   # one small TI block of 1 FEC block and one big of 2


def test_map_modes():
    """the shape codes' map_cells paths: mode 2 with R = 2025 rows (no multiple of 16), QPSK's mode 0"""
    fs, rate, const, rot = LM.SHAPE_CODES["s256r"]
    mp = PP.map_plan(fs, rate, const, rot)
    assert (mp["mode"], mp["R"], mp["R"] % 16 != 0) == (2, 2025, True)
    fs, rate, const, rot = LM.SHAPE_CODES["nqpskr"]
    assert PP.map_plan(fs, rate, const, rot)["mode"] == 0
    assert {PP.map_plan(*c.cfg.im_args())["mode"] for c in LM.CODE_MATRIX} == {0, 1, 2}


def test_round_counts(tables):
    """rounds of MQ * NW = 36 chunks per block: QPSK normal 127 chunks (4 rounds), 16-QAM normal 64 (2), 64-QAM
    normal 43 (2), 256-QAM normal 32 (1, clamped); a block of 8100 cells or fewer has at most 32 chunks"""
    for c in LM.SHAPES:
        key = c.id.split("-")[0]
        nch = LM.chunk_counts(tables[c.id])
        assert {LM.round_count(x) for x in nch} == {LM.ROUNDS[key]}, (c.id, nch)
        assert (nch % (LM.MQ * LM.NW) != 0).all()   # the last round is clamped
    want = {E.MOD_QPSK: (127, 4), E.MOD_16QAM: (64, 2), E.MOD_64QAM: (43, 2), E.MOD_256QAM: (32, 1)}
    for c in LM.CODE_MATRIX:
        nch = LM.chunk_counts(tables[c.id])
        if c.cfg.framesize == E.FECFRAME_NORMAL:
            n, rounds = want[c.cfg.constellation]
            assert (nch == n).all() and LM.round_count(n) == rounds, (c.id, nch)
        if tables[c.id]["cs"] <= 8100:
            assert nch.max() <= 32, (c.id, nch)


def test_chunk_counts_differ(tables):
    """at least one case has a block whose chunk count differs from its neighbour's (1K: 8, 9, 9)"""
    differ = [c.id for c in LM.ALL_CASES if len(set(LM.chunk_counts(tables[c.id]).tolist())) > 1]
    assert "s256r-fft1k" in differ
    assert LM.chunk_counts(tables["s256r-fft1k"]).tolist() == [8, 9, 9]


def test_partial_quads(tables):
    """the 2-byte edge stores: taken over all cases each of the four slot-flag bits occurs both set and clear in
    partial quads, the patterns that occur are the listed ones, some case has none and some block more than 16"""
    seen, counts = set(), {}
    for c in LM.ALL_CASES:
        pat, per_row = LM.partial_patterns(tables[c.id])
        seen |= set(int(x) for x in pat)
        counts[c.id] = per_row
    assert tuple(sorted(seen)) == LM.PARTIAL_PATTERNS
    for s in range(4):
        assert any(p >> s & 1 for p in seen) and any(not (p >> s & 1) for p in seen), s
    assert any(v.sum() == 0 for v in counts.values())
    assert any(v.max() > 16 for v in counts.values())
    assert counts["s256r-fft1k"].tolist() == [1, 17, 17]
    # without time interleaving (tiblocks = 0) whole blocks follow each other: only a block's ends can be partial
    for c in LM.SHAPES:
        if c.cfg.tiblocks == 0:
            assert counts[c.id].max() <= 2, c.id


def test_layouts_reached(tables):
    """the FFT cases take the split (32K) and the unsplit layouts"""
    split = {c.id: PP.chain_layout(c.cfg)["split"] for c in LM.SHAPES if "-fft" in c.id}
    assert split == {"s256r-fft1k": 0, "s256r-fft2k": 0, "s256r-fft4k": 0, "s256r-fft16k": 0, "s256r-fft32k": 1}


def test_xcd_major_cases():
    """frames per run: 5, 20 and 45 blocks behind 8, 8 and 16 L1-post workgroups; xcd_major is the identity below
    16 blocks and a non-identity permutation from 20 on (q = 2, tail of 4)"""
    got = {}
    for c in LM.SHAPES:
        if "-frames" not in c.id:
            continue
        n = c.cfg.fecblocks * c.frames
        perm = [LM.xcd_major(i, n) for i in range(n)]
        assert sorted(perm) == list(range(n))
        got[c.frames] = (n, LM.l1_workgroups(c.frames), perm == list(range(n)))
    assert got == {1: (5, 8, True), 4: (20, 8, False), 9: (45, 16, False)}
    assert all([LM.xcd_major(i, n) for i in range(n)] == list(range(n)) for n in range(16))
    perm = [LM.xcd_major(i, 20) for i in range(20)]
    assert perm[:16] == [0, 2, 4, 6, 8, 10, 12, 14, 1, 3, 5, 7, 9, 11, 13, 15] and perm[16:] == [16, 17, 18, 19]
    # every other case launches fewer than 16 blocks
    assert all(c.cfg.fecblocks * c.frames < 16 for c in LM.ALL_CASES if "-frames" not in c.id)


def test_oracle_blocks_do_not_depend_on_fecblocks():
    """what lets every case of a code slice one oracle run: without in-band signalling FEC block B's BBFRAME is
    the same whatever the frame's FEC block count, and a longer stream only appends"""
    fs, rate = LM.SHAPE_CODES["s256r"][:2]
    out = []
    for F, n in ((3, 6), (5, 10)):
        cfg = LM.BASE.with_(framesize=fs, rate=rate, fecblocks=F)
        ts, base = ts_for_frames(cfg, 0, 2)
        assert base == 0
        out.append(O.BB(*cfg.bb_args()).work(ts, n)[0].reshape(n, -1))
    np.testing.assert_array_equal(out[0], out[1][:6])
    cw = LM.oracle_codewords(fs, rate)
    assert len(cw) == 90   # 9 frames x 5 blocks, run twice
    kbch = out[0].shape[1]
    np.testing.assert_array_equal(cw[:10, :kbch], out[1])
