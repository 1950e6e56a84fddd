"""CPU: the MISO pair chain's planner tables (both transmitter groups from one FEC + map pass).  Group 2's layout
over group 1's slot order and the 32K cross lists, applied on the host in the OFDM kernel's order to a pair buffer
filled in group 1's slot order, against the 9.1 rule in numpy (tests/miso_ref.py) over the unmodified oracle's
frame mapper and pilot stage; all comparisons on bit patterns."""
import dataclasses
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from dvbt2ll import enums as E
from dvbt2ll.configs import MPLP_CONFIGS, IF_CONFIGS, MISO_TX2_PROCESSED
import oracle_lib as O
import plan_probe as PP
import miso_ref as MR
import miso_pair_probe as MP
import test_cpu_miso as TM

GOLDEN = Path(__file__).resolve().parent / "golden" / "miso_pair_plan_digests.json"
# test_cpu_miso's shapes (1K .. 32K, T2-Lite, N_P2 = 2 and 16, PAPR TR, extended carriers with EQ) and 32K TR extended
# (PAPR TR and extended carriers together move the active span and with it the straddling pairs)
EXTRA = {"32k_pp2_tr_ext": dict(TM.SINGLE["32k_pp2_tr"], carriermode=E.CARRIERS_EXTENDED)}
SHAPES = list(TM.SINGLE) + list(EXTRA)
K32 = [n for n in SHAPES if n.startswith("32k")]


def shape_cfg(name):
    if name in TM.SINGLE:
        return TM.single_cfg(name)
    over = dict(TM.MISO)
    over.update(EXTRA[name])
    return TM._fit(TM.BASE.with_(**over))


def _u32(x):
    return np.ascontiguousarray(x, np.complex64).view(np.uint32)


def _check_pair(m, cfg_for_counts, frame, mapped, cls):
    """group 2's carriers of one frame from the pair tables over group 1's slots; returns (tables, TX1 tables,
    cross list lengths)"""
    t1 = MR.chain_tables(m.with_(misogroup=E.MISO_TX1), cls)
    t = MP.pair_tables(m, cls)
    assert t1 is not None and t1["miso"] == 0 and t is not None and t["miso"] == 1
    # the same slot ranges: the LDPC + map kernel stores once, through group 1's quad table
    for key in ("part", "d0", "n", "n0", "bnd"):
        np.testing.assert_array_equal(t[key], t1[key], err_msg=key)
    pl = PP.pilot_plan(m.with_(misogroup=MISO_TX2_PROCESSED).pg_args())
    l1, _ = PP.l1post_mplp(m, frame)
    want = MR.expected_carriers(mapped, cfg_for_counts.with_(misogroup=MISO_TX2_PROCESSED))
    got, lens = MP.pair_scatter_carriers(t, MP.group1_slots(t1, mapped), l1, pl["isinc"] if pl["eq"] else None)
    for j in range(t["Nsym"]):
        np.testing.assert_array_equal(_u32(got[j]), _u32(want[j]), err_msg="frame %d symbol %d" % (frame, j))
    assert lens.max(initial=0) == t["xmax"] <= t["xbound"] <= t["xcap"]
    return t, t1, lens


@pytest.mark.parametrize("name", SHAPES)
def test_pair_tables_match_rule(name):
    cfg = shape_cfg(name)
    m = MR.as_mplp(cfg)
    fm = O.FMM(m)
    for frame in range(2):
        mapped = fm.work(TM._rand(fm.stream_items, 21 + frame))
        t, t1, lens = _check_pair(m, cfg, frame, mapped, 0)
    assert set(np.unique(t["csel"])) == {0, 2, 3}
    assert t["ni"] == t["Lp"]
    if name in K32:
        # pairs straddle the stored halves, so some cells are written by the other half's cross list: without
        # them the 32K cases would prove nothing
        assert t["split"] == 1 and lens.max() > 0 and t["skip"].sum() == lens.sum() > 0
        # (a straddling pair puts one cell in each half's list, unless its other cell is an L1 or dummy cell,
        # which the aux lists carry)
        # the bound: the 1024-bin block boundaries inside the active carriers' span, the fftshift wrap included,
        # the band edge (k = N/2) excluded
        pl = PP.pilot_plan(cfg.pg_args())
        N = t["N"]
        act = (pl["bin_map"] != -1).any(axis=0)
        act |= (PP.pilot_plan(cfg.with_(misogroup=E.MISO_TX1).pg_args())["bin_map"] != -1).any(axis=0)
        c = np.nonzero(act[(np.arange(N) - N // 2) % N])[0]           # active carriers, carrier order
        kk = (np.arange(c.min(), c.max()) - N // 2) % N               # k of each carrier but the last
        assert t["xbound"] == int((((kk + 1) % N) % 1024 == 0).sum()) == 27 <= t["xcap"] == 32
    else:
        assert t["split"] == 0 and t["xmax"] == 0 and not t["skip"].any() and len(t["xent"]) == 0
        assert t["xbound"] == 0


def test_pair_part_is_not_the_identity():
    """slots are FEC-block-major and bank-balanced for group 1's bins at every N, so the processed handle's layout
    cannot stand in for the pair's group 2 even at N <= 16K"""
    cfg = TM.single_cfg("8k_pp2")
    t = MP.pair_tables(cfg)
    t2 = MR.chain_tables(cfg)
    assert not np.array_equal(t["part"], np.arange(t["S"]))
    assert not np.array_equal(t["part"], t2["part"]) and not np.array_equal(t["inv"], t2["inv"])


def test_pair_multi_plp_frame():
    m = MPLP_CONFIGS["mplp2_8k"].with_(preamble=E.PREAMBLE_T2_MISO)
    cells, _, _ = O.mplp_cells(m, 0, 2)
    fm = O.FMM(m)
    for frame in range(2):
        t, _, _ = _check_pair(m, m, frame, fm.work(cells[frame]), 0)
    assert t["nplp"] == 2 and t["xmax"] == 0


def test_pair_frame_interval_classes():
    m = IF_CONFIGS["ij2_4k_single"].with_(preamble=E.PREAMBLE_T2_MISO)
    m = m.with_(plps=(dataclasses.replace(m.plps[0], fecblocks=4, tiblocks=2),))
    cells, _, _ = O.mplp_cells(m, 0, 2)
    fm = O.FMM(m)
    S = []
    for frame in range(2):
        t, _, _ = _check_pair(m, m, frame, fm.work(cells[frame]), frame % 2)
        assert t["ncls"] == 2
        S.append(t["S"])
    assert S[0] > 0 and S[1] == 0


def test_pair_cross_entries_name_their_plp():
    """a two-PLP 32K frame: every cross entry's PLP is the one whose slot range holds the slot"""
    base = TM.single_cfg("32k_pp2_tr")
    p0 = MR.as_mplp(base).plps[0]
    fb = max(1, p0.fecblocks // 2)
    m = MR.as_mplp(base).with_(plps=(dataclasses.replace(p0, fecblocks=fb, tiblocks=min(p0.tiblocks, fb)),
                                     dataclasses.replace(p0, fecblocks=fb, tiblocks=min(p0.tiblocks, fb),
                                                         constellation=E.MOD_64QAM)))
    t = MP.pair_tables(m)
    assert t is not None and t["nplp"] == 2 and len(t["xent"]) > 0
    seen = set()
    for j in range(t["Nsym"]):
        s0, n0 = int(t["d0"][j]), int(t["n0"][j])
        for h in range(2):
            x0, xn = t["xgrp"][2 * j + h]
            for slot, _, _, plp in t["xent"][x0:x0 + xn]:
                b = t["bnd"][2 * j + (1 if slot - s0 >= n0 else 0)]    # the half whose run holds the slot
                assert (1 if slot - s0 >= n0 else 0) == 1 - h
                assert b[plp] <= slot < b[plp + 1]
                seen.add(int(plp))
    assert seen == {0, 1}


def test_pair_value_handling():
    ok = TM.single_cfg("4k_short_np2")
    assert MP.pair_tables(ok) is not None
    for pre in (E.PREAMBLE_T2_SISO, E.PREAMBLE_T2_LITE_SISO):   # a pair needs a MISO preamble
        assert MP.pair_tables(ok.with_(preamble=pre)) is None


@pytest.mark.parametrize("name", TM.DIGEST_CFGS)
@pytest.mark.parametrize("group", [E.MISO_TX1, MISO_TX2_PROCESSED])
def test_ordinary_plans_hash_as_before(name, group):
    """the plans of ordinary handles are untouched by the pair planner.  MISO_TX1's hash to the digests recorded
    before MISO processing existed (test_cpu_miso's golden file).  MISO_TX2_PROCESSED's digests (with plp_bnd and
    csel, which the older digest leaves out) were recorded together with the pair planner, from the planner as it
    stood without it; they pin the processed plans from here on."""
    cfg = TM.digest_cfg(name, group)
    if group == E.MISO_TX1:
        assert TM.plan_digest(cfg) == json.loads(TM.GOLDEN.read_text())["%s/%d" % (name, group)]
        return
    want = json.loads(GOLDEN.read_text())
    assert TM.plan_digest(cfg) == want["%s/%d" % (name, group)]
    t = MR.chain_tables(cfg)
    h = hashlib.sha256()
    for k in ("bnd", "csel"):
        h.update(np.ascontiguousarray(t[k]).tobytes())
    assert h.hexdigest() == want["%s/%d/bnd_csel" % (name, group)]
