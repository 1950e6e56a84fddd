"""CPU: the contract of the chain's quad table (t2_plan.h QuadTable, built by build_quad_table for chain_build
and consumed by t2_kernels.hip map_store_quads), probed through t2_plan_probe.cpp.

map_store_quads is emulated in numpy: for row rr of the table, entry n < slot_nq[rr] and each of its four slots s
whose flag bit (0x8000) is clear, destination 4 * (qbase[n / 64] + qoff[n]) + s receives the value of cell j of
block rr.  Scattering random per-cell values through that must give, bit for bit, the frame data region in the
chain's slot order: for the reference's single-PLP frame the array tests/test_cpu_plan.py
test_chain_cell_layout_matches_oracle builds (cell (r, j) at part[ti_dest(r, (ci_perm[j] + ci_shift[r]) % cs)]),
for multi-PLP and interleaving-frame configurations the oracle framemapper's output taken back through the frame
class's gather_d and part (frame f of the launch unit at f * pair_stride).  Beside that, the properties the kernel
relies on without checking them (each a comment at its assertion).
"""
import numpy as np
import pytest

from dvbt2ll.configs import CONFIGS, MPLP_CONFIGS, IF_CONFIGS
import oracle_lib as O
import plan_probe as PP
import lm_cases as LM
import miso_ref
from test_cpu_plan import GRID, BENCH_CFGS, grid_cfg

rng = np.random.default_rng(31)


def _rand(n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def emulate(q, vals, out, hits):
    """map_store_quads over the probed table q for every row: vals [rows, cs] -> out (the unit's pair buffer),
    hits counting the stores per slot.  Returns the chunks that ended early (entries padded in before slot_nq)."""
    stride, cs = q["stride"], q["cs"]
    ent = LM.slot_entries(q)                       # [rows, stride, 4]
    flag, j = (ent >> 15) & 1, ent & 0x7FFF
    n = np.arange(stride)
    early = 0
    for rr in range(q["rows"]):
        nq = int(q["nq"][rr])
        assert 0 < nq <= stride
        f, jj = flag[rr], j[rr]
        # a flagged slot carries j = 0: the kernel reads idx[0] and idx[-1] for it
        assert (jj[f == 1] == 0).all()
        # every stored j is a cell of the block
        assert (jj < cs).all()
        # entries from slot_nq[rr] up to the stride are all 0x80008000 (the clamped rounds load them)
        assert (q["quad"][rr, nq:] == 0x80008000).all()
        empty = f[:nq].all(axis=1)
        quadi = q["qbase"][rr][n[:nq] >> 6].astype(np.int64) + q["qoff"][rr, :nq]
        nch = (nq + 63) >> 6
        valid = (n[:64 * nch] < nq).reshape(nch, 64)
        e = np.ones(64 * nch, bool)
        e[:nq] = empty
        e = e.reshape(nch, 64)
        k = (~e).sum(axis=1)
        # a chunk's real entries come first; entries padded in by an early-ended chunk are empty quads
        assert (k > 0).all() and (np.diff(e.astype(np.int8), axis=1) >= 0).all()
        short = k < valid.sum(axis=1)
        assert not short[valid.sum(axis=1) < 64].any()   # the row's last chunk just ends at slot_nq
        early += int(short.sum())
        # inside a chunk qoff is strictly increasing, and qbase is the quad of its first entry
        off = np.zeros(64 * nch, np.int64)
        off[:nq] = q["qoff"][rr, :nq]
        off = off.reshape(nch, 64)
        assert (off[:, 0] == 0).all() and (np.diff(off, axis=1)[~e[:, 1:]] > 0).all()
        assert (off[e] == 0).all()
        live = (f[:nq] == 0)
        dest = (4 * quadi[:, None] + np.arange(4)[None, :])[live]
        assert dest.min() >= 0 and dest.max() < len(out)
        out[dest] = vals[rr][jj[:nq][live]]
        np.add.at(hits, dest, 1)
    # the uploads' tails (the kernel's clamped loads may read one entry past a row)
    raw = q["raw"]
    assert (raw["quad"][q["rows"] * stride * 2:] == 0x80008000).all()
    return early


def _check_cover(hits, q, Ss):
    """across all blocks of a launch unit every data slot is written exactly once, and no slot outside [0, S) of
    its frame"""
    ps = q["pair_stride"]
    for f in range(q["unit"]):
        S = Ss[f % q["ncls"]]
        h = hits[f * ps:(f + 1) * ps]
        assert (h[:S] == 1).all(), ("frame", f, np.nonzero(h[:S] != 1)[0][:8])
        assert (h[S:] == 0).all(), ("frame", f)


def _single(cfg):
    q = PP.quad_table(cfg)
    assert q is not None
    plan = PP.frame_plan(cfg.fm_args())
    lay = PP.chain_layout(cfg)
    cs, F, S = plan["cs"], plan["F"], plan["S"]
    assert (q["rows"], q["cs"], q["unit"], q["cls_S"], q["pair_stride"]) == (F, cs, 1, [S], LM.pair_stride(S))
    cells = _rand(F * cs)
    r = np.repeat(np.arange(F), cs)
    jj = np.tile(np.arange(cs), F)
    t = (plan["ci_perm"][jj] + plan["ci_shift"][r]) % cs
    data = np.zeros(S, np.complex64)
    data[lay["part"][PP.ti_dest(plan, r, t)]] = cells
    out = np.zeros(q["pair_stride"], np.complex64)
    hits = np.zeros(q["pair_stride"], np.int32)
    early = emulate(q, cells.reshape(F, cs), out, hits)
    _check_cover(hits, q, [S])
    np.testing.assert_array_equal(out[:S].view(np.uint64), data.view(np.uint64))
    return q, early


@pytest.mark.parametrize("name,over", GRID + [(n, None) for n in BENCH_CFGS], ids=[g[0] for g in GRID] + BENCH_CFGS)
def test_quad_table_single_plp(name, over):
    _single(CONFIGS[name] if over is None else grid_cfg(over))


@pytest.mark.parametrize("case", LM.SHAPES, ids=[c.id for c in LM.SHAPES])
def test_quad_table_shape_cases(case):
    _single(case.cfg)


@pytest.mark.parametrize("code", LM.ALL_CODES, ids=[LM._code_id(*c) for c in LM.ALL_CODES])
def test_quad_table_code_matrix(code):
    """the table depends on the cell count and the layout, not on the rotation: the rotated cases of one code"""
    for case in LM.CODE_MATRIX:
        if case.code == code and case.cfg.rotation:
            _single(case.cfg)


def _multi(m):
    """the launch unit of a multi-PLP / interleaving-frame configuration: every PLP's table into one pair buffer"""
    qs = [PP.quad_table(m, k) for k in range(m.nplp)]
    assert all(q is not None for q in qs)
    q0 = qs[0]
    unit, ps, ncls = q0["unit"], q0["pair_stride"], q0["ncls"]
    assert unit == m.unit_frames
    tabs = [miso_ref.chain_tables(m, c) for c in range(ncls)]
    assert [t["S"] for t in tabs] == q0["cls_S"] and ps == LM.pair_stride(max(q0["cls_S"]))
    out = np.zeros(unit * ps, np.complex64)
    hits = np.zeros(unit * ps, np.int32)
    vals, early = [], 0
    for k, (p, q) in enumerate(zip(m.plps, qs)):
        assert (q["unit"], q["pair_stride"], q["cls_S"]) == (unit, ps, q0["cls_S"])
        assert q["F"] == p.fecblocks and q["cycle"] == p.if_frames and q["rows"] == p.fecblocks * (unit // p.if_frames)
        vals.append(_rand(q["rows"] * q["cs"]).reshape(q["rows"], q["cs"]))
        early += emulate(q, vals[k], out, hits)
    _check_cover(hits, q0, q0["cls_S"])
    # the oracle's framemapper over the unit, fed the same cells: PLP k's interleaving frame m' (rows m' F ..
    # m' F + F - 1 of its table) on the T2 frame it starts in
    fm = O.FMM(m)
    for f in range(unit):
        fresh = []
        for k, p in enumerate(m.plps):
            n = fm.consume(k)
            assert n == (p.fecblocks * qs[k]["cs"] if p.starts_if(f) else 0)
            if n:
                mi = f // p.if_frames
                fresh.append(vals[k][mi * p.fecblocks:(mi + 1) * p.fecblocks].reshape(-1))
        mapped = fm.work(np.concatenate(fresh) if fresh else np.zeros(0, np.complex64))
        t = tabs[f % ncls]
        g = t["gather_d"]
        want = np.zeros(t["S"], np.complex64)
        want[t["part"][g[g >= 0]]] = mapped[g >= 0]
        np.testing.assert_array_equal(out[f * ps:f * ps + t["S"]].view(np.uint64), want.view(np.uint64),
                                      err_msg="%s frame %d" % (m.name, f))
    return early


@pytest.mark.parametrize("name", list(MPLP_CONFIGS))
def test_quad_table_mplp(name):
    _multi(MPLP_CONFIGS[name])


# The configurations in which a chunk ends early (a block's next quad lies more than 0xFFFF quads past the chunk's
# first one).  ti1_32k_p2 is not among them: its 390 blocks each touch every TI row, so a block's consecutive quads
# are about 3300 quads apart, also across the boundary of its two T2 frames, and a 64-quad chunk spans about
# 53000 quads at most.  The rule triggers where a PLP's interleaving frame skips T2 frames (ij_mix_8k: frames 3
# and 7 of the unit) or has few quads per T2 frame of a large frame (ti1_32k_p2p4).
EARLY_CHUNKS = {"ij_mix_8k", "ti1_32k_p2p4"}


@pytest.mark.parametrize("name", list(IF_CONFIGS))
def test_quad_table_interleaving_frames(name):
    early = _multi(IF_CONFIGS[name])
    assert (early > 0) == (name in EARLY_CHUNKS), early
