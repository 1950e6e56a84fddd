"""CPU: MISO processing of transmitter group 2's payload cells (EN 302 755 9.1; misogroup =
MISO_TX2_PROCESSED).  The planner's processed tables, applied on the host in the OFDM kernels' order, against
the 9.1 rule in numpy (tests/miso_ref.py) over the unmodified oracle's frame mapper and pilot stage.

PARITY UNPINNED: the reference has no MISO processing block (only the pilot switch of pilotgenp1insert_cc);
misogroup 0 and 1 are pinned to it as before, and their plans to the digests recorded before this value
existed (tests/golden/miso_plan_digests.json)."""
import dataclasses
import hashlib
import itertools
import json
from pathlib import Path

import numpy as np
import pytest

from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, MPLP_CONFIGS, IF_CONFIGS, MISO_TX2_PROCESSED
import oracle_lib as O
import plan_probe as PP
import miso_ref as MR

GOLDEN = Path(__file__).resolve().parent / "golden" / "miso_plan_digests.json"
BASE = CONFIGS["cfg1"]
MISO = dict(preamble=E.PREAMBLE_T2_MISO, misogroup=MISO_TX2_PROCESSED)


def _u32(x):
    return np.ascontiguousarray(x, np.complex64).view(np.uint32)


# ---------------------------------------------------------------- the helper's known answers
def test_rule_known_answer():
    got = MR.miso_pairs(np.array([1 + 2j, 3 - 4j], np.complex64))
    np.testing.assert_array_equal(_u32(got), _u32(np.array([-3 - 4j, 1 - 2j], np.complex64)))


def test_rule_signed_zeros_as_bit_patterns():
    """-conj(+0 - 0j) = (-0, -0) and conj(-0 + 5j) = (-0, -5): each part keeps or flips its sign bit alone"""
    a = np.zeros(2, np.complex64)
    w = a.view(np.float32)
    w[:] = [-0.0, 5.0, 0.0, -0.0]            # a0 = -0 + 5j, a1 = +0 - 0j
    got = MR.miso_pairs(a).view(np.uint32)
    want = np.array([-0.0, -0.0, -0.0, -5.0], np.float32).view(np.uint32)   # e0 = -conj(a1), e1 = conj(a0)
    np.testing.assert_array_equal(got, want)
    z = MR.miso_pairs(np.zeros(2, np.complex64)).view(np.uint32)            # +0 cells: (-0, +0), (+0, -0)
    np.testing.assert_array_equal(z, np.array([0x80000000, 0, 0, 0x80000000], np.uint32))


def test_rule_rows_are_orthogonal():
    """the Alamouti property: rows (a0, a1) and (e0, e1) of each pair are orthogonal, with equal energy"""
    rng = np.random.default_rng(5)
    a = (rng.integers(-7, 8, 64) + 1j * rng.integers(-7, 8, 64)).astype(np.complex64)   # exact in float32
    e = MR.miso_pairs(a)
    a2, e2 = a.reshape(-1, 2).astype(np.complex128), e.reshape(-1, 2).astype(np.complex128)
    assert (np.sum(a2 * np.conj(e2), axis=1) == 0).all()
    assert (np.sum(np.abs(a2) ** 2, axis=1) == np.sum(np.abs(e2) ** 2, axis=1)).all()


def test_flip_matches_rule():
    """the kernels' selector form (partner cell, one sign flipped) is the rule: even positions selector 1"""
    rng = np.random.default_rng(6)
    a = (rng.standard_normal(10) + 1j * rng.standard_normal(10)).astype(np.complex64)
    p = np.arange(10)
    np.testing.assert_array_equal(_u32(MR.flip(a[p ^ 1], (p & 1) ^ 1)), _u32(MR.miso_pairs(a)))


# ---------------------------------------------------------------- even counts
def test_miso_rows_have_even_symbol_counts():
    """every (FFT, carrier mode, pilot pattern, PAPR, GI) row the cell-count tables hold for a MISO preamble has
    even C_P2, C_DATA and N_FC, so every symbol's payload splits into pairs"""
    ffts = [E.FFTSIZE_1K, E.FFTSIZE_2K, E.FFTSIZE_4K, E.FFTSIZE_8K, E.FFTSIZE_8K_T2GI, E.FFTSIZE_16K,
            E.FFTSIZE_16K_T2GI, E.FFTSIZE_32K, E.FFTSIZE_32K_T2GI]
    rows = 0
    for pre in (E.PREAMBLE_T2_MISO, E.PREAMBLE_T2_LITE_MISO):
        for fft, cm, pp, papr, gi in itertools.product(ffts, range(2), range(8), range(4), range(7)):
            c = PP.cell_counts(fft, cm, pp, papr, gi, pre)
            if c is None:
                continue
            rows += 1
            assert c["C_P2"] % 2 == 0 and c["C_DATA"] % 2 == 0 and c["N_FC"] % 2 == 0, (pre, fft, cm, pp, papr, gi, c)
    assert rows > 500


# ---------------------------------------------------------------- planner against oracle
def _fit(cfg):
    """cfg with 3/4 of the FEC blocks its frame can carry (dummy cells present), as test_cpu_plan's grid"""
    lo, hi = 1, 4000
    assert PP.frame_plan(cfg.with_(fecblocks=1, tiblocks=min(cfg.tiblocks, 1)).fm_args()) is not None
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if PP.frame_plan(cfg.with_(fecblocks=mid, tiblocks=min(cfg.tiblocks, mid)).fm_args()) is None:
            hi = mid - 1
        else:
            lo = mid
    fb = max(1, lo * 3 // 4)
    return cfg.with_(fecblocks=fb, tiblocks=min(cfg.tiblocks, fb))


SINGLE = {
    "1k_pp4": dict(fftsize=E.FFTSIZE_1K, pilotpattern=E.PILOT_PP4, constellation=E.MOD_16QAM, rate=E.C2_5,
                   guardinterval=E.GI_1_16, numdatasyms=8),
    "2k_pp3_l1bpsk": dict(fftsize=E.FFTSIZE_2K, pilotpattern=E.PILOT_PP3, constellation=E.MOD_QPSK, rate=E.C1_3,
                          guardinterval=E.GI_1_4, numdatasyms=6, l1constellation=E.L1_MOD_BPSK),
    # 4K short: N_P2 = 2, the L1 cells zig-zag over both P2 symbols
    "4k_short_np2": dict(),
    "4k_short_l1_16qam_v131": dict(l1constellation=E.L1_MOD_16QAM, version=E.VERSION_131,
                                   l1scrambled=E.L1_SCRAMBLED_ON, pilotpattern=E.PILOT_PP2, guardinterval=E.GI_1_8),
    "4k_t2lite": dict(preamble=E.PREAMBLE_T2_LITE_MISO, pilotpattern=E.PILOT_PP3, guardinterval=E.GI_1_8),
    "8k_pp2": dict(fftsize=E.FFTSIZE_8K, pilotpattern=E.PILOT_PP2, guardinterval=E.GI_1_8, numdatasyms=5),
    "16k_pp5_tr": dict(fftsize=E.FFTSIZE_16K, pilotpattern=E.PILOT_PP5, paprmode=E.PAPR_TR, numdatasyms=3,
                       guardinterval=E.GI_1_8),
    "32k_pp2_tr": dict(fftsize=E.FFTSIZE_32K, pilotpattern=E.PILOT_PP2, paprmode=E.PAPR_TR, guardinterval=E.GI_1_8,
                       numdatasyms=3, framesize=E.FECFRAME_NORMAL, rate=E.C2_3),
    "32k_pp4_ext_eq": dict(fftsize=E.FFTSIZE_32K, pilotpattern=E.PILOT_PP4, carriermode=E.CARRIERS_EXTENDED,
                           guardinterval=E.GI_1_16, numdatasyms=3, framesize=E.FECFRAME_NORMAL, rate=E.C3_5,
                           equalization=E.EQUALIZATION_ON, bandwidth=E.BANDWIDTH_6_0_MHZ),
}


def single_cfg(name):
    over = dict(MISO)
    over.update(SINGLE[name])
    return _fit(BASE.with_(**over))


def _rand(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def _check_scatter(m, cfg_for_counts, frame, mapped, cls):
    t = MR.chain_tables(m, cls)
    assert t is not None and t["miso"] == 1
    pl = PP.pilot_plan(m.pg_args())
    l1, _ = PP.l1post_mplp(m, frame)
    want = MR.expected_carriers(mapped, cfg_for_counts)
    got = MR.scatter_carriers(t, mapped, l1, pl["isinc"] if pl["eq"] else None)
    for j in range(t["Nsym"]):
        np.testing.assert_array_equal(_u32(got[j]), _u32(want[j]), err_msg="frame %d symbol %d" % (frame, j))
    return t, pl, want


@pytest.mark.parametrize("name", list(SINGLE))
def test_planner_tables_match_rule(name):
    """scatter mode (the chain: slot bins with selectors, direct and indirect aux lists, two FRAME_IDX values'
    L1-post cells) and gather mode (the pilotgen block's bin_map) both rebuild, bit for bit, the oracle's group 2
    carriers over the 9.1-coded cells"""
    cfg = single_cfg(name)
    m = MR.as_mplp(cfg)
    fm = O.FMM(m)
    assert fm.mapped_items == O.FM(*cfg.fm_args()).mapped_items
    for frame in range(2):
        mapped = fm.work(_rand(fm.stream_items, 11 + frame))
        t, pl, want = _check_scatter(m, cfg, frame, mapped, 0)
    got = MR.gather_carriers(pl, mapped)
    np.testing.assert_array_equal(_u32(got), _u32(want))
    # the selector of every payload bin: 1 at even positions; data slots carry it in bit 15, bins below 2^15
    assert set(np.unique(t["csel"])) == {0, 2, 3}
    assert ((t["inv"] & 0x7FFF) < t["N"]).all()
    if name == "4k_short_np2":
        counts = MR.symbol_counts(cfg)
        assert len(counts) > 2 and counts[0] == counts[1] and (1840 + t["Lp"]) > counts[0] // 2   # N_P2 = 2
    assert t["ni"] == t["Lp"]   # every L1-post cell is an indirect entry
    if name == "1k_pp4":
        # N_P2 = 16: each P2 symbol starts with 1840 / 16 = 115 L1-pre cells, an odd count, so a pair joins the
        # last L1-pre cell (a direct entry, flipped on the host) with the first L1-post cell (indirect, flipped
        # by the kernel); the L1 cell count as a whole is always even
        npp = PP.cell_counts(cfg.fftsize, cfg.carriermode, cfg.pilotpattern, cfg.paprmode, cfg.guardinterval,
                             cfg.preamble)["N_P2"]
        assert npp == 16 and (1840 // npp) % 2 == 1


def test_32k_pairs_straddle_the_stored_halves():
    """32K: the kernel fills two stored halves in turn (bins of even / odd k >> 10); pairs whose two carriers
    fall in different halves exist, and each cell is streamed with the half of its destination bin"""
    cfg = single_cfg("32k_pp2_tr")
    t = MR.chain_tables(cfg)
    pl = PP.pilot_plan(cfg.pg_args())
    N = t["N"]
    half_of = PP.stored_index(N, 1) >= N // 2            # natural k -> stored half
    straddle = 0
    for j in range(t["Nsym"]):
        code = pl["bin_map"][j].astype(np.int64)
        k = np.nonzero(code >= 0)[0]
        src = code[k] & 0x3FFFFFFF
        kk = np.empty(len(k), np.int64)
        kk[src - src.min()] = k                          # bin taking source cell p
        hp = half_of[kk]
        straddle += int((hp[0::2] != hp[1::2]).sum())
        s0, n, n0 = int(t["d0"][j]), int(t["n"][j]), int(t["n0"][j])
        bins = t["inv"][s0:s0 + n].astype(np.int64) & 0x7FFF
        assert (bins[:n0] < N // 2).all() and (bins[n0:] >= N // 2).all()
    assert straddle > 0


def test_multi_plp_frame():
    """a multi-PLP MISO frame: the PLP-major slot order and plp_bnd follow the destination bins"""
    m = MPLP_CONFIGS["mplp2_8k"].with_(**MISO)
    cells, _, _ = O.mplp_cells(m, 0, 2)
    fm = O.FMM(m)
    for frame in range(2):
        t, _, _ = _check_scatter(m, m, frame, fm.work(cells[frame]), 0)
    assert t["nplp"] == 2
    for g in range(t["Nsym"]):
        b = t["bnd"][2 * g]
        assert b[0] == t["d0"][g] and b[-1] == t["d0"][g] + t["n"][g] and (np.diff(b) >= 0).all()


def test_frame_interval_classes():
    """FRAME_INTERVAL 2: the even frames carry the PLP, the odd ones dummy cells only; each class's tables"""
    m = IF_CONFIGS["ij2_4k_single"].with_(**MISO)
    m = m.with_(plps=(dataclasses.replace(m.plps[0], fecblocks=4, tiblocks=2),))
    t0 = MR.chain_tables(m, 0)
    assert t0 is not None and t0["ncls"] == 2
    cells, _, _ = O.mplp_cells(m, 0, 2)
    fm = O.FMM(m)
    for frame in range(2):
        t, _, _ = _check_scatter(m, m, frame, fm.work(cells[frame]), frame % 2)
    assert t["S"] == 0 and t0["S"] > 0


# ---------------------------------------------------------------- value handling
def test_value_handling():
    ok = single_cfg("4k_short_np2")
    assert PP.pilot_plan(ok.pg_args()) is not None and MR.chain_tables(ok)["miso"] == 1
    for pre in (E.PREAMBLE_T2_SISO, E.PREAMBLE_T2_LITE_SISO):   # 2 needs a MISO preamble
        siso = ok.with_(preamble=pre)
        assert PP.frame_plan(siso.fm_args()) is not None
        assert PP.pilot_plan(siso.pg_args()) is None and MR.chain_tables(siso) is None
    for bad in (3, -1, 1 << 30):
        c = ok.with_(misogroup=bad)
        assert PP.pilot_plan(c.pg_args()) is None and MR.chain_tables(c) is None
    # group 2 without processing is accepted with a SISO preamble as before (the pilots then do not differ)
    assert PP.pilot_plan(BASE.with_(misogroup=E.MISO_TX2).pg_args()) is not None


def plan_digest(cfg):
    """sha256 over the tables the OFDM kernels read: bin_map, the chain layout and the aux lists"""
    pl, lay, al = PP.pilot_plan(cfg.pg_args()), PP.chain_layout(cfg), PP.aux_lists(cfg)
    h = hashlib.sha256()
    for a in (pl["bin_map"], lay["cmap_stored"], lay["inv"], lay["d0"], lay["n"], lay["n0"], lay["part"],
              al["dbin"], al["dval"], al["ind"], al["grp"], al["zrun"], al["auxv"]):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


DIGEST_CFGS = ["4k_short_np2", "4k_t2lite", "8k_pp2", "32k_pp2_tr"]


def digest_cfg(name, group):
    return single_cfg(name).with_(misogroup=group)


@pytest.mark.parametrize("name", DIGEST_CFGS)
@pytest.mark.parametrize("group", [E.MISO_TX1, E.MISO_TX2])
def test_groups_0_and_1_plan_as_before(name, group):
    """misogroup 0 and 1 do not enter the processed branch: their plans hash to the digests recorded from the
    planner before MISO_TX2_PROCESSED existed, and carry no selector"""
    cfg = digest_cfg(name, group)
    want = json.loads(GOLDEN.read_text())
    assert plan_digest(cfg) == want["%s/%d" % (name, group)]
    t = MR.chain_tables(cfg)
    assert t["miso"] == 0 and not t["csel"].any()
    assert plan_digest(cfg) != plan_digest(cfg.with_(misogroup=MISO_TX2_PROCESSED))
