"""CPU: what each case of tests/mplp_cases.py claims, proven before the GPU runs it (test_gpu_mplp_many.py): 4-8
PLPs per T2 frame against the oracle's multi-PLP framemapper, the L1-post at K_sig = 1309, the constellation
tables' shared bases, per-symbol PLP runs shorter than one aligned load of the OFDM kernels' slot scatter, an
empty run between two non-empty ones; and, in numpy on the oracle's carriers, that each kernel mistake these
cases exist to catch changes the frame.

PARITY UNPINNED as test_cpu_mplp.py / test_cpu_ti.py: the reference carries one Type-1 PLP."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _MplpChainParams, _MplpParams
from dvbt2ll.configs import MAX_PLP, PLP_INTS
import mplp_cases as MC
import oracle_lib as O
import plan_probe as PP
from test_cpu_ti import _placement

rng = np.random.default_rng(41)
NAMES = list(MC.CASES)


def _apply(gmap, src, aux):
    return np.where(gmap >= 0, src[np.clip(gmap, 0, None)], aux[np.clip(-gmap - 1, 0, None)]).astype(np.complex64)


def _rand(n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def test_case_list():
    assert NAMES == ["many8_8k_all", "many8_8k_shared", "many6_32k_shared", "tiny_4k_quad", "tiny_16k_sq16",
                     "tiny_32k_octet", "skip_8k"]
    assert [MC.CASES[n].nplp for n in NAMES] == [8, 8, 6, 3, 3, 3, 5]
    a = MC.CASES["many8_8k_all"]
    assert sorted((p.constellation, p.rotation) for p in a.plps) == [(c, r) for c in range(4) for r in range(2)]
    assert sorted({p.fecblocks for p in a.plps}) == [1, 2, 3]
    assert any(p.tiblocks == 0 for p in a.plps) and any(p.inputmode for p in a.plps) and any(p.inband for p in a.plps)
    s = MC.CASES["many6_32k_shared"]
    assert (s.vlength, s.carriermode, s.version, s.l1scrambled, s.l1constellation) == (32768, 1, 2, 1, 2)
    k = MC.CASES["skip_8k"]
    assert k.unit_frames == 2 and [p.frame_interval for p in k.plps] == [1, 2, 1, 2, 1]


# ---------------------------------------------------------------- planner against oracle
@pytest.mark.parametrize("name", NAMES)
def test_case_frame_matches_oracle(name):
    """every mapped cell of the frame for consecutive FRAME_IDX values (past the superframe's wrap) and every
    frame class: the planner's gather map of the frame phase applied to random cells against the oracle's
    multi-PLP framemapper fed the same cells"""
    m = MC.CASES[name]
    fr = PP.frame_plan_mplp(m)
    fm = O.FMM(m)
    assert fr is not None and fr["unit"] == m.unit_frames and fr["nplp"] == m.nplp
    assert (fr["M"], fr["S"], fr["Lp"]) == (fm.mapped_items, fm.stream_items, fm.l1post_cells)
    cur = [np.zeros(p.fecblocks * c, np.complex64) for p, c in zip(m.plps, fr["cs"])]
    for f in range(max(2 * fr["unit"], m.t2frames + 1)):
        fresh = []
        for k, p in enumerate(m.plps):
            n = fm.consume(k)
            assert n == (p.fecblocks * fr["cs"][k] if p.starts_if(f) else 0)
            if n:
                cur[k] = _rand(n)
                fresh.append(cur[k])
        want = fm.work(np.concatenate(fresh) if fresh else np.zeros(0, np.complex64))
        got = _apply(fr["gather_in"][f % fr["unit"]], np.concatenate(cur), fr["aux"][f % m.t2frames])
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg="%s frame %d" % (name, f))


@pytest.mark.parametrize("name", NAMES)
def test_case_l1post(name):
    """K_sig = 350 + 137 (nplp - 1) (1309 bits at eight PLPs), the L1-post cells per frame equal to the
    oracle's, and the signalling bits of every FRAME_IDX equal to the oracle's (orc_fm_l1post_bits)"""
    m = MC.CASES[name]
    fm = O.FMM(m)
    for fidx in range(m.t2frames):
        cells, info = PP.l1post_mplp(m, fidx)
        assert info["nsig"] == 350 + 137 * (m.nplp - 1)
        assert info["Lp"] == fm.l1post_cells == len(cells)
        got, want = PP.l1post_bits_mplp(m, fidx), fm.l1post_bits(fidx)
        assert len(got) == info["nsig"] - 32        # the CRC-32 follows
        np.testing.assert_array_equal(got, want, err_msg="%s FRAME_IDX %d" % (name, fidx))
    if m.nplp == 8:
        assert info["nsig"] == 1309 and (info["nsig"] + 31) // 32 == 41


@pytest.mark.parametrize("name", NAMES)
def test_case_chain_layout(name):
    """test_mplp_chain_layout's invariants for every frame class: part is a permutation, every (symbol, half)
    group's slots are PLP-major, and plp_bnd delimits exactly the slots whose data cells the class's placement
    (8.3.6.3, restated in test_cpu_ti._placement) gives that PLP"""
    m = MC.CASES[name]
    fr = PP.frame_plan_mplp(m)
    P = m.nplp
    ncls = MC.class_tables(m, 0)["ncls"]
    assert ncls == max(p.frame_interval for p in m.plps)
    for cls in range(ncls):
        t = MC.class_tables(m, cls)
        present, start, _, ssi, S = _placement(m, cls, fr["plp_S"])
        assert t["S"] == S and t["nplp"] == P
        plp_of_cell = np.full(S, -1, np.int64)
        for k, p in enumerate(m.plps):
            if not present[k]:
                continue
            c = np.arange(fr["plp_S"][k])
            if p.plp_type == 1:
                pos = start[k] + c
            else:
                ss = fr["plp_S"][k] // m.num_subslices
                pos = start[k] + (c // ss) * ssi + c % ss
            assert np.all(plp_of_cell[pos] == -1)
            plp_of_cell[pos] = k
        assert np.all(plp_of_cell >= 0)
        assert sorted(t["part"].tolist()) == list(range(S))
        plp_of_slot = np.zeros(S, np.int64)
        plp_of_slot[t["part"]] = plp_of_cell
        for j in range(t["Nsym"]):
            a, mid, b = t["d0"][j], t["d0"][j] + t["n0"][j], t["d0"][j] + t["n"][j]
            for h, (lo, hi) in enumerate(((a, mid), (mid, b))):
                bnd = t["bnd"][2 * j + h]
                assert bnd[0] == lo and bnd[P] == hi and np.all(np.diff(bnd) >= 0), (name, cls, j, h)
                for k in range(P):
                    assert np.all(plp_of_slot[bnd[k]:bnd[k + 1]] == k), (name, cls, j, h, k)
                    assert present[k] or bnd[k] == bnd[k + 1]


# ---------------------------------------------------------------- constellation table bases
@pytest.mark.parametrize("name", NAMES)
def test_case_table_bases(name):
    """the first PLP with a (constellation, rotation) pair owns a table, later ones reuse it: at most 1024
    entries (OFDM_MAX_QAM); all eight pairs side by side are exactly 680, the most valid parameters reach"""
    m = MC.CASES[name]
    bases, total = MC.table_bases(m)
    flat, flat_total = MC.table_bases(m, share=False)
    assert total <= MC.OFDM_MAX_QAM
    assert 2 * (4 + 16 + 64 + 256) == 680
    if name == "many8_8k_all":
        assert total == 680 and bases == flat and np.all(np.diff(bases) > 0)
    if name in MC.SHARED:
        assert np.any(np.diff(bases) < 0)                                    # not monotonic
        assert sum(a != b for a, b in zip(bases, flat)) >= 3 and total < flat_total
        k = next(k for k in range(1, m.nplp) if bases[k] != flat[k])         # the first repeat
        assert bases[k] < bases[k - 1]
    # a table per PLP would not fit the worst frame: eight 256-QAM PLPs are 2048 entries, shared 256
    worst = m.with_(plps=tuple(dataclasses.replace(m.plps[0], constellation=MC.Q256, rotation=1) for _ in range(8)))
    assert MC.table_bases(worst, share=False)[1] == 2048 and MC.table_bases(worst)[1] == 256


def test_many8_shared_bases_literal():
    assert MC.table_bases(MC.CASES["many8_8k_shared"]) == ([0, 256, 0, 272, 256, 276, 0, 340], 404)
    assert MC.table_bases(MC.CASES["many8_8k_shared"], share=False)[0] == [0, 256, 272, 528, 532, 548, 612, 868]
    assert MC.table_bases(MC.CASES["many6_32k_shared"]) == ([0, 64, 0, 80, 64, 0], 336)


# ---------------------------------------------------------------- short and empty runs
@pytest.mark.parametrize("name", list(MC.TINY))
def test_tiny_short_run(name):
    """the pinned run lies in plp_bnd where the module says: 1-3 slots (1-7 at 32K), its first slot off the
    quad (octet) alignment, its last in the same quad (octet); with a non-empty neighbour run in the group"""
    m, align = MC.CASES[name], MC.TINY[name]
    cls, g, k, start, n = MC.SHORT_RUN[name]
    t = MC.class_tables(m, cls)
    assert bool(t["split"]) == (align == 8)
    b = t["bnd"][g]
    assert (int(b[k]), int(b[k + 1] - b[k])) == (start, n)
    assert 1 <= n <= align - 1
    assert start % align != 0
    assert start // align == (start + n - 1) // align
    assert MC.is_short_run(start, n, align) and MC.SHORT_RUN[name] in MC.short_runs(m, align)
    others = [int(b[q + 1] - b[q]) for q in range(m.nplp) if q != k]
    assert any(others)
    # the masked slots of the load belong to this group's other PLPs on at least one side
    lo = start // align * align
    assert lo >= b[0] or lo + align <= b[m.nplp]


def test_tiny_miso_short_run():
    """the MISO variant: tiny_4k_quad's MISO layout has no short run, the searched 16K MISO frame has one in its
    processed (misogroup 2) layout, where scatter_slots<MISO> carries the selector in bit 15 of the bins; its
    frame matches the oracle's framemapper"""
    from dvbt2ll.configs import MISO_TX2_PROCESSED
    lost = MC.CASES["tiny_4k_quad"].with_(preamble=MC.TINY_MISO.preamble, misogroup=MISO_TX2_PROCESSED)
    assert MC.short_runs(lost, 4) == []
    m = MC.TINY_MISO
    cls, g, k, start, n = MC.SHORT_RUN_MISO
    t = MC.class_tables(m, cls)
    assert t["miso"] == 1 and not t["split"]
    b = t["bnd"][g]
    assert (int(b[k]), int(b[k + 1] - b[k])) == (start, n)
    assert 1 <= n <= 3 and start % 4 != 0 and start // 4 == (start + n - 1) // 4
    assert MC.SHORT_RUN_MISO in MC.short_runs(m, 4)
    assert (t["inv"] >> 15).any()   # selector bits are in use
    fr, fm = PP.frame_plan_mplp(m), O.FMM(m)
    assert (fr["M"], fr["S"], fr["Lp"]) == (fm.mapped_items, fm.stream_items, fm.l1post_cells)
    for f in range(3):
        cells = _rand(fr["S"])
        got = _apply(fr["gather_in"][0], cells, fr["aux"][f % m.t2frames])
        np.testing.assert_array_equal(got.view(np.uint32), fm.work(cells).view(np.uint32), err_msg="frame %d" % f)


def test_is_short_run_rule():
    assert MC.is_short_run(5, 3, 4) and MC.is_short_run(5, 3, 8) and MC.is_short_run(7, 1, 4)
    assert not MC.is_short_run(4, 2, 4) and not MC.is_short_run(6, 3, 4) and not MC.is_short_run(3, 0, 4)
    assert MC.is_short_run(9, 7, 8) and not MC.is_short_run(9, 8, 8) and not MC.is_short_run(8, 3, 8)


def test_search_finds_the_pinned_4k_frame():
    """the committed search, on the 4K frame (the cheapest planner): its first hit has a short run; the search
    that produced tiny_16k_sq16 and tiny_32k_octet is this function on their frames"""
    from dvbt2ll.configs import CONFIGS
    hits, walked, asked, shortest = MC.search_short_run(CONFIGS["cfg1"], 4, limit=1)
    assert len(hits) == 1 and 0 < asked <= walked
    m, runs = hits[0]
    assert runs and all(MC.is_short_run(a, n, 4) for _, _, _, a, n in runs)
    assert shortest[0] <= 3


def test_skip_empty_run_between_present_plps():
    m = MC.CASES["skip_8k"]
    cls, g, k = MC.SKIPPED_RUN
    t = MC.class_tables(m, cls)
    ln = np.diff(t["bnd"][g])
    assert ln[k] == 0 and ln[:k].any() and ln[k + 1:].any()
    assert (cls, g, k) in MC.skipped_runs(m)
    assert not m.plps[k].starts_if(cls) and m.plps[k - 1].starts_if(cls) and m.plps[k + 1].starts_if(cls)
    # both absent PLPs (a Type-1 and a Type-2 one) are skipped somewhere, and the other class carries them
    assert {q for c, _, q in MC.skipped_runs(m) if c == 0} == {1, 3}
    assert np.diff(MC.class_tables(m, 1)["bnd"], axis=1)[:, [1, 3]].any(axis=0).all()


# ---------------------------------------------------------------- sensitivity: the kernel mistakes, in numpy
@functools.lru_cache(maxsize=None)
def _frame0(name):
    """frame 0 of a case from the oracle: mapped cells, carriers, class 0's tables, and per data slot its mapped
    cell, its PLP and its constellation index pair (real part's index, imaginary part's)"""
    m = MC.CASES[name]
    cells, _, _ = O.mplp_cells(m, 0, 1)
    mapped = O.FMM(m).work(cells[0])
    pg = O.PG(*m.pg_args())
    t = MC.class_tables(m, 0)
    S = t["S"]
    gd = t["gather_d"]
    isd = np.nonzero(gd >= 0)[0]
    cell_of_slot = np.zeros(S, np.int64)
    cell_of_slot[t["part"][gd[isd]]] = isd
    plp_of_slot = np.full(S, -1, np.int64)
    for g, runs in MC.group_runs(t):
        for k, (a, n) in enumerate(runs):
            plp_of_slot[a:a + n] = k
    assert (plp_of_slot >= 0).all()
    bases, total = MC.table_bases(m)
    qall = np.zeros(MC.OFDM_MAX_QAM + 256, np.complex64)   # reads past a small table stay inside the model
    ire, iim = np.zeros(S, np.int64), np.zeros(S, np.int64)
    for k, p in enumerate(m.plps):
        mp = PP.map_plan(p.framesize, p.rate, p.constellation, p.rotation)
        n = 1 << mp["mod"]
        assert n == 4 << (2 * p.constellation)
        lut = mp["lut"][:n]
        qall[bases[k]:bases[k] + n] = lut
        s = np.nonzero(plp_of_slot == k)[0]
        v = mapped[cell_of_slot[s]]
        if p.rotation:     # every point has its own real and its own imaginary part
            assert len(set(lut.real.tolist())) == n and len(set(lut.imag.tolist())) == n
            ore, oim = np.argsort(lut.real), np.argsort(lut.imag)
            ire[s] = ore[np.searchsorted(lut.real[ore], v.real)]
            iim[s] = oim[np.searchsorted(lut.imag[oim], v.imag)]
        else:              # both parts from the same cell
            key = lut.view(np.uint64)
            o = np.argsort(key)
            ire[s] = iim[s] = o[np.clip(np.searchsorted(key[o], v.view(np.uint64)), 0, n - 1)]
    return dict(m=m, mapped=mapped, pg=pg, car=pg.carriers(mapped), t=t, cell_of_slot=cell_of_slot,
                plp_of_slot=plp_of_slot, qall=qall, bases=bases, ire=ire, iim=iim)


def _lookup(fx, slots, base):
    """scatter_slots' lookup of the slots' index pairs in the tables at `base`"""
    q = fx["qall"]
    return (q.real[base + fx["ire"][slots]] + 1j * q.imag[base + fx["iim"][slots]]).astype(np.complex64)


def _changed(fx, slots, values):
    """bins at which the frame's carriers change when the slots hold `values`"""
    mapped = fx["mapped"].copy()
    mapped[fx["cell_of_slot"][slots]] = values
    return int(np.count_nonzero(fx["pg"].carriers(mapped).view(np.uint64) != fx["car"].view(np.uint64)))


@pytest.mark.parametrize("name", NAMES)
def test_model_reproduces_the_oracle(name):
    """the numpy model of the lookup (index pairs recovered from the oracle's cells, the tables laid out at the
    expected bases) gives back every data cell of the oracle's frame bit for bit: the planner's constellation
    tables are the oracle's points, and the sensitivity checks below start from the true frame"""
    fx = _frame0(name)
    for k in range(fx["m"].nplp):
        s = np.nonzero(fx["plp_of_slot"] == k)[0]
        got = _lookup(fx, s, fx["bases"][k])
        np.testing.assert_array_equal(got.view(np.uint32), fx["mapped"][fx["cell_of_slot"][s]].view(np.uint32),
                                      err_msg="%s plp %d" % (name, k))


@pytest.mark.parametrize("name", list(MC.TINY))
def test_sensitive_to_neighbour_table(name):
    """mistake: the short run's slots looked up with the neighbouring run's table base (a run boundary off by
    the masked edge, or plp_qbase indexed by the wrong PLP)"""
    fx = _frame0(name)
    cls, g, k, start, n = MC.SHORT_RUN[name]
    assert cls == 0
    b = fx["t"]["bnd"][g]
    near = [q for q in (k - 1, k + 1) if 0 <= q < fx["m"].nplp and b[q + 1] > b[q]
            and fx["bases"][q] != fx["bases"][k]]
    assert near
    slots = np.arange(start, start + n)
    for q in near:
        assert _changed(fx, slots, _lookup(fx, slots, fx["bases"][q])) >= 1, (name, q)


@pytest.mark.parametrize("name", list(MC.TINY))
def test_sensitive_to_unmasked_load(name):
    """mistake: in_run not applied, so the whole aligned quad / octet of the short run is looked up in the run's
    table and written: the neighbouring PLPs' slots of that load change"""
    fx = _frame0(name)
    align = MC.TINY[name]
    cls, g, k, start, n = MC.SHORT_RUN[name]
    b = fx["t"]["bnd"][g]
    lo = start // align * align
    load = np.arange(max(lo, int(b[0])), min(lo + align, int(b[fx["m"].nplp])))
    extra = load[(load < start) | (load >= start + n)]
    assert extra.size >= 1 and (fx["plp_of_slot"][extra] != k).all()
    assert _changed(fx, extra, _lookup(fx, extra, fx["bases"][k])) >= 1


@pytest.mark.parametrize("name", MC.SHARED)
def test_sensitive_to_unshared_base(name):
    """mistake: a sharing PLP given the base a table of its own would have had (the cumulative sum), while the
    tables are laid out shared"""
    fx = _frame0(name)
    flat, _ = MC.table_bases(fx["m"], share=False)
    moved = [k for k in range(fx["m"].nplp) if flat[k] != fx["bases"][k]]
    assert len(moved) >= 3
    for k in moved:
        s = np.nonzero(fx["plp_of_slot"] == k)[0]
        assert s.size and _changed(fx, s, _lookup(fx, s, flat[k])) >= 1, (name, k)


def test_sensitive_to_skipped_plp():
    """mistake: the empty run of skip_8k's absent PLP 1 not skipped (b > a dropped), its zero-length run
    rounded up to one load: the next PLP's first slots are looked up in PLP 1's table"""
    fx = _frame0("skip_8k")
    cls, g, k = MC.SKIPPED_RUN
    b = fx["t"]["bnd"][g]
    lo = int(b[k]) // 4 * 4
    load = np.arange(max(lo, int(b[0])), min(lo + 4, int(b[fx["m"].nplp])))
    assert load.size and fx["bases"][k] not in {fx["bases"][q] for q in set(fx["plp_of_slot"][load].tolist())}
    assert _changed(fx, load, _lookup(fx, load, fx["bases"][k])) >= 1


# ---------------------------------------------------------------- nine PLPs
def _raw_array(m, nplp):
    """dvbt2ll_mplp_params as ints with nplp written as given (MplpConfig.mplp_array asserts nplp <= 8)"""
    a = list(m.common_args()) + [nplp]
    for k in range(MAX_PLP):
        a += list(m.plps[k % m.nplp].plp_args())
    assert len(a) == 13 + PLP_INTS * MAX_PLP
    return a + [m.num_subslices]


def raw_chain_params(m, nplp, max_frames=1):
    a = _raw_array(m, nplp)
    p = _MplpParams(*a[:13])
    for k in range(MAX_PLP):
        p.plp[k] = type(p.plp[k])(*a[13 + PLP_INTS * k:13 + PLP_INTS * (k + 1)])
    p.num_subslices = a[-1]
    return _MplpChainParams(p, int(m.misogroup), int(m.equalization), int(m.bandwidth), max_frames)


def test_nine_plps_refused():
    """nplp = 9 (> DVBT2LL_MAX_PLP) is refused by the planner and by dvbt2ll_chain_create_mplp before it touches a
    device; the same array with nplp = 8 plans (the GPU suite creates it: test_gpu_mplp_many.py)"""
    m = MC.CASES["many8_8k_all"]
    info = np.zeros(68, np.int32)
    for nplp, ok in ((8, True), (9, False), (0, False)):
        a = np.array(_raw_array(m, nplp), np.int32)
        assert (PP.lib().t2probe_frame_mplp(PP._p(a), PP._p(info), None, None, None) == 0) == ok, nplp
    np.testing.assert_array_equal(_raw_array(m, 8), m.mplp_array())
    with pytest.raises(AssertionError):
        m.with_(plps=m.plps + m.plps[:1]).mplp_array()
    L = dvbt2ll.lib()
    for nplp in (9, 0):
        h = ctypes.c_void_p()
        p = raw_chain_params(m, nplp)
        r = L.dvbt2ll_chain_create_mplp(ctypes.byref(p), 0, ctypes.byref(h))
        assert r != 0 and L.dvbt2ll_strerror(r) == b"invalid parameter combination" and not h.value, nplp
