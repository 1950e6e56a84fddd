"""Case construction shared by tests/test_cpu_lm_cases.py (which proves on the CPU that the cases reach what they
claim), tests/test_cpu_quad_table.py (the quad table's contract) and tests/test_gpu_ldpc_map.py (which runs them
through the chain's LDPC + map kernel, t2_kernels.hip ldpc_map_kernel).

What the kernel does per FEC block, and what a case must vary to reach it:

  * map_cells by (mode, modulation, cell count): every code x constellation (CODE_MATRIX);
  * idx[-1] = idx[cs - 1] under rotation: rotation on and off for each of them;
  * map_store_quads over the block's row of the quad table in rounds of MQ * NW = 36 chunks of 64 quads, the last
    round clamped (round_count); the 2-byte stores of partial quads (a quad shared with a neighbouring block:
    partial_patterns); blocks whose chunk counts differ: TI shapes, FFT sizes (SHAPES);
  * xcd_major: a permutation of the launch's blocks only from 16 blocks on, after ceil8(frames) L1-post
    workgroups: frames per run (SHAPES).

Oracle results are computed once per code and handed out read-only.
"""
import functools
from collections import namedtuple

import numpy as np

from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, ts_for_frames
import oracle_lib as O
import plan_probe as PP

ALL_CODES = [(1, r) for r in range(6)] + [(0, r) for r in range(8)]   # (framesize, rate)
CONSTS = [E.MOD_QPSK, E.MOD_16QAM, E.MOD_64QAM, E.MOD_256QAM]
CONST_NAME = {E.MOD_QPSK: "qpsk", E.MOD_16QAM: "16qam", E.MOD_64QAM: "64qam", E.MOD_256QAM: "256qam"}
BASE = CONFIGS["cfg4"]   # 8K, PP7, 59 data symbols

# the kernel's round geometry (t2_kernels.hip MQ, FEC_THREADS / 64)
MQ, NW = 9, 4

Case = namedtuple("Case", "id cfg frames code")


def _code_id(fs, rate):
    return "%s%d" % ("n" if fs else "s", rate)


def _matrix():
    out = []
    for fs, rate in ALL_CODES:
        for const in CONSTS:
            for rot in (0, 1):
                cfg = BASE.with_(framesize=fs, rate=rate, constellation=const, rotation=rot, fecblocks=3, tiblocks=2)
                out.append(Case("%s-%s-%s" % (_code_id(fs, rate), CONST_NAME[const], "rot" if rot else "unrot"), cfg, 1,
                                (fs, rate)))
    return out


CODE_MATRIX = _matrix()

# the four codes of the shape cases: (framesize, rate, constellation, rotation)
SHAPE_CODES = {
    "s256r": (E.FECFRAME_SHORT, E.C4_5, E.MOD_256QAM, 1),    # map_cells mode 2, R = 2025 (no multiple of 16)
    "nqpskr": (E.FECFRAME_NORMAL, E.C1_2, E.MOD_QPSK, 1),     # 127 chunks: 4 rounds; idx[-1] under QPSK
    "n16r35": (E.FECFRAME_NORMAL, E.C3_5, E.MOD_16QAM, 1),    # the 3/5 demux; 64 chunks: 2 rounds
    "n64u": (E.FECFRAME_NORMAL, E.C2_3, E.MOD_64QAM, 0),      # 43 chunks: 2 rounds
}
ROUNDS = {"s256r": 1, "nqpskr": 4, "n16r35": 2, "n64u": 2}   # rounds of MQ * NW chunks per block
TI_SHAPES = [(1, 0), (1, 1), (2, 3), (5, 0), (5, 1), (5, 2), (7, 3), (7, 7), (8, 3)]   # (fecblocks, tiblocks)
FRAME_COUNTS = [1, 4, 9]   # x 5 FEC blocks: 5, 20, 45 blocks behind 8, 8, 16 L1-post workgroups
# FFT sizes: the GRID entry (tests/test_cpu_plan.py) that supplies the frame parameters
FFT_GRID = {"1k": "1k_pp1_16qam", "2k": "2k_pp3_qpsk_short", "4k": "4k_grc", "16k": "16k_pp5_tr",
            "32k": "32k_pp4_ext_cfg3like"}


def _code_cfg(base, key, **kw):
    fs, rate, const, rot = SHAPE_CODES[key]
    return base.with_(framesize=fs, rate=rate, constellation=const, rotation=rot, **kw)


def _shapes():
    from test_cpu_plan import GRID, BASE as GRID_BASE
    grid = dict(GRID)
    out = []
    for key in SHAPE_CODES:
        for F, ti in TI_SHAPES:
            out.append(Case("%s-F%d-ti%d" % (key, F, ti), _code_cfg(BASE, key, fecblocks=F, tiblocks=ti), 1,
                            SHAPE_CODES[key][:2]))
    for fft, gname in FFT_GRID.items():
        cfg = _code_cfg(GRID_BASE.with_(**grid[gname]), "s256r", fecblocks=3, tiblocks=2)
        out.append(Case("s256r-fft%s" % fft, cfg, 1, SHAPE_CODES["s256r"][:2]))
    for n in FRAME_COUNTS:
        out.append(Case("s256r-F5-frames%d" % n, _code_cfg(BASE, "s256r", fecblocks=5, tiblocks=2), n,
                        SHAPE_CODES["s256r"][:2]))
    return out


SHAPES = _shapes()
ALL_CASES = CODE_MATRIX + SHAPES

# Every flag pattern of a partial quad (bit s set: slot s belongs to another block) that the cases reach, as
# measured by tests/test_cpu_lm_cases.py from the probed quad tables.  A layout change that drops one fails there.
PARTIAL_PATTERNS = (1, 3, 7, 8, 12, 14)


# ---------------------------------------------------------------- the kernel's geometry, restated
def xcd_major(i, n):
    """t2_kernels.hip xcd_major: launch workgroup i of n -> logical block"""
    q = n >> 3
    return (i & 7) * q + (i >> 3) if i < (q << 3) else i


def l1_workgroups(frames):
    return (frames + 7) & ~7


def chunk_counts(q):
    """64-quad chunks of each row of a probed quad table"""
    return (q["nq"] + 63) >> 6


def round_count(nch):
    """rounds of MQ * NW chunks map_store_quads takes for a block of nch chunks (the last one clamped unless
    nch is a multiple of MQ * NW)"""
    return -(-int(nch) // (MQ * NW))


def slot_entries(q):
    """the table's 16-bit slot entries as [rows, stride, 4]"""
    e = q["quad"]
    return np.stack([e[..., 0] & 0xFFFF, e[..., 0] >> 16, e[..., 1] & 0xFFFF, e[..., 1] >> 16], axis=-1).astype(np.int64)


def partial_patterns(q):
    """flag pattern (bit s: slot s flagged) of every partial quad of the table: a quad below slot_nq with
    some but not all of its slots flagged; returns (patterns, count per row)"""
    ent = slot_entries(q)
    flag = (ent >> 15) & 1
    pat = flag[..., 0] | flag[..., 1] << 1 | flag[..., 2] << 2 | flag[..., 3] << 3
    live = np.arange(q["stride"])[None, :] < q["nq"][:, None]
    part = live & (pat != 0) & (pat != 15)
    return pat[part], part.sum(axis=1)


# ---------------------------------------------------------------- oracle, once per code
def _blocks_needed(code):
    n = 3
    for c in ALL_CASES:
        if c.code == code:
            n = max(n, c.cfg.fecblocks * c.frames * (2 if c in SHAPES else 1))
    return n


@functools.lru_cache(maxsize=None)
def oracle_codewords(framesize, rate):
    """the oracle's bbheaderbch + ldpc output (one bit per byte, [blocks, nldpc]) of the first FEC blocks of the
    synthetic stream, as many as any case of this code needs.  Without in-band signalling a block's BBFRAME does
    not depend on the frame's FEC block count (test_cpu_lm_cases.py checks that), so every case slices this."""
    nb = _blocks_needed((framesize, rate))
    cfg = BASE.with_(framesize=framesize, rate=rate, fecblocks=nb)
    ts, base = ts_for_frames(cfg, 0, 1)
    assert base == 0
    bits, _ = O.BB(*cfg.bb_args()).work(ts, nb)
    cw = O.LDPC(framesize, rate).work(bits, nb).reshape(nb, 64800 if framesize else 16200)
    cw.setflags(write=False)
    return cw


def packed_codewords(framesize, rate, constellation, cw):
    """ldpc output bits [blocks, nldpc] -> the chain's packed interleaver-input codewords: info bits, then the
    parity interleaved [row a][column c] where the constellation has it"""
    fp = PP.fec_plan(framesize, rate, constellation)
    nbch, q = fp["nbch"], fp["q"]
    nldpc = cw.shape[1]
    if fp["parity_il"]:
        t, s = np.divmod(np.arange(nldpc - nbch), 360)
        cw = cw.copy()
        cw[:, nbch:] = cw[:, nbch + q * s + t]
    return np.packbits(cw, axis=1)


@functools.lru_cache(maxsize=8)
def _layout(cfg):
    plan = PP.frame_plan(cfg.fm_args())
    lay = PP.chain_layout(cfg)
    cs, F = plan["cs"], plan["F"]
    r = np.repeat(np.arange(F), cs)
    jj = np.tile(np.arange(cs), F)
    t = (plan["ci_perm"][jj] + plan["ci_shift"][r]) % cs
    return plan["S"], cs, lay["part"][PP.ti_dest(plan, r, t)]


def expected(case, first_frame):
    """what a run of case.frames T2 frames from first_frame leaves: the oracle's cells of each frame in the
    chain's slot order ([frames, S], placed as tests/test_gpu_chain.py test_chain_cells_match_oracle places
    them) and the packed codewords of its FEC blocks"""
    cfg = case.cfg
    F, n = cfg.fecblocks, cfg.fecblocks * case.frames
    cw = oracle_codewords(cfg.framesize, cfg.rate)[first_frame * F:first_frame * F + n]
    assert len(cw) == n
    cells = O.IM(*cfg.im_args()).work(np.ascontiguousarray(cw).reshape(-1), n)
    S, cs, dest = _layout(cfg)
    want = np.zeros((case.frames, S), np.complex64)
    want[:, dest] = cells.reshape(case.frames, F * cs)
    return want, packed_codewords(cfg.framesize, cfg.rate, cfg.constellation, cw)


def pair_stride(S):
    """slots from one T2 frame's data region to the next in the chain's pair buffer (t2_capi.cpp chain_build)"""
    return (S + 7) // 8 * 8
