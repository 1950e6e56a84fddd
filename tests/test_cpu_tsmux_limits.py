"""CPU: what tests/tsmux_limit_cases.py claims of its cases, shown without a GPU: every case passes the host-only
validators (dvbt2ll_tsmux_schedule, dvbt2ll_tsmux_remux_check) and the documented ranges of its positions; the
reference runs on every one; the eight-input cases move every counter they are meant to move and their bytes depend on
every argument a kernel could misread; the long cases have the tile, chunk and trip counts they are named for; the
sweep covers every width and every counter."""
import ctypes
import re
import time
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _TsMuxParams
from dvbt2ll.tsmux import remux_params
import tsmux_limit_cases as L
import tsmux_ref as R
import tsremux_ref as X

W = R.W
FIXED = [L.plain8(), L.remux8(), L.long_emit(), L.long_classify()]
BY_NAME = {c["name"]: c for c in FIXED}
SWEEP = L.sweep()


def _params(kw, max_out):
    p = _TsMuxParams()
    p.n_inputs, p.period, p.fill_input = len(kw["weight"]), kw["period"], kw["fill_input"]
    for i, w in enumerate(kw["weight"]):
        p.weight[i], p.loop[i] = w, kw["loop"][i]
    p.pcr_pid, p.pcr_weight, p.ticks_per_period, p.max_out_packets = (kw["pcr_pid"], kw["pcr_weight"],
                                                                      kw["ticks_per_period"], max_out)
    return p


def _valid(case):
    """the host-only validators, then the ranges include/dvbt2ll_hip.h gives for a run's arguments and positions"""
    kw, name = case["mux"], case["name"]
    n = len(kw["weight"])
    p = _params(kw, max(case["n_out"], 1))
    owner = np.full(kw["period"] + 8, 0xEE, np.uint8)
    assert dvbt2ll.lib().dvbt2ll_tsmux_schedule(ctypes.byref(p), owner.ctypes.data_as(ctypes.c_void_p)) == 0, name
    np.testing.assert_array_equal(owner[:kw["period"]], R.schedule(kw["period"], kw["weight"], kw["pcr_weight"]), name)
    assert (owner[kw["period"]:] == 0xEE).all()
    n_in = [len(x) // 188 for x in case["inputs"]]
    phase, ticks, nxt = case["start"]
    assert len(case["inputs"]) == n and all(len(x) % 188 == 0 for x in case["inputs"]), name
    assert 0 <= case["n_out"] <= 1 << 24 and 0 <= phase < kw["period"] and 0 <= ticks < W, name
    assert all(0 <= nxt[i] <= n_in[i] for i in range(n)) and not any(nxt[n:]), name
    rx = case["remux"]
    if rx is None:
        return
    assert dvbt2ll.lib().dvbt2ll_tsmux_remux_check(ctypes.byref(p), ctypes.byref(remux_params(**rx))) == 0, name
    cc, in_phase, in_ticks = case["rstart"]
    per, tpp = list(rx["in_period"]) + [0] * 8, list(rx["in_ticks_per_period"]) + [0] * 8
    assert all(0 <= v <= 15 for v in cc) and not any(cc[len(rx["track_pid"]):]), name
    for i in range(8):
        assert 0 <= in_phase[i] <= max(per[i], 1) - 1 and 0 <= in_ticks[i] < (W if per[i] else 1), (name, i)
        assert not per[i] or (n_in[i] // per[i] + 1) * tpp[i] <= 1 << 62, (name, i)


def _counts(n_out):
    """tiles, chunks of the second scan round, trips of the emit kernel's workgroup 0, trips of the classify kernel's"""
    tiles = -(-n_out // L.TILE)
    return tiles, -(-tiles // L.SCAN_TILES), -(-tiles // L.MAX_BLOCKS), -(-(-(-tiles // 4)) // L.MAX_BLOCKS)


# ---------------------------------------------------------------------------------------- all cases
def test_the_constants_are_the_kernel_headers_and_the_long_cases_pass_the_grids():
    text = (Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "csrc" / "tsmux_kernels.h").read_text()
    assert int(re.search(r"TSMUX_PKTS = (\d+);", text).group(1)) == L.TILE and re.search(r"TSREMUX_TILE = TSMUX_PKTS;", text)
    assert int(re.search(r"TSREMUX_SCAN_TILES = (\d+);", text).group(1)) == L.SCAN_TILES
    assert int(re.search(r"TSMUX_MAX_BLOCKS = (\d+);", text).group(1)) == L.MAX_BLOCKS
    assert int(re.search(r"TSMUX_IN = (\d+);", text).group(1)) == len(L.N8) == 8
    assert int(re.search(r"TSREMUX_SLOTS = (\d+);", text).group(1)) == 64
    # the emit kernel takes a tile per workgroup trip and the classify kernel four, on grids of at most MAX_BLOCKS
    e, c = BY_NAME["long_emit"]["n_out"], BY_NAME["long_classify"]["n_out"]
    assert e == L.MAX_BLOCKS * L.TILE + L.TILE + 7 and _counts(e) == (2050, 9, 2, 1) and e % L.TILE == 7
    assert c == 4 * L.MAX_BLOCKS * L.TILE + L.TILE + 7 == 524359 and _counts(c) == (8194, 33, 5, 2) and c % L.TILE == 7
    # the longest call of tests/tsremux_cases.py: one trip everywhere, two chunks
    assert _counts(L.TILE * L.SCAN_TILES + L.TILE + 1) == (258, 2, 1, 1)
    # the splits the device test makes of long_emit fall on a trip's and on a chunk's first packet
    assert _counts(L.MAX_BLOCKS * L.TILE)[2] == 1 and _counts(L.TILE * L.SCAN_TILES)[1] == 1


@pytest.mark.parametrize("case", FIXED + SWEEP, ids=[c["name"] for c in FIXED + SWEEP])
def test_case_is_valid_and_the_reference_runs(case):
    _valid(case)
    t0 = time.perf_counter()
    ref, rref = L.reference(case)
    if case["name"] == "long_classify":
        print("long_classify: the reference took %.1f s" % (time.perf_counter() - t0))
    assert len(ref.ts) == case["n_out"] * 188 and (ref.ts[::188] == 0x47).all()
    c = ref.counters
    generated = c["pcr_packets"] + c["null_packets"] - c["sync_errors"] - (rref.counters["dropped"] if rref else 0)
    assert sum(c["consumed"]) + generated == case["n_out"]
    if case["cont"] and case["n_out"] < 1 << 18:
        first = {pid: case["rstart"][0][s] for s, pid in enumerate(case["remux"]["track_pid"]) if pid in case["cont"]}
        nxt = X.check_continuity(ref.ts, pids=case["cont"], first=first)
        assert all(rref.resume[0][s] == nxt[pid] for s, pid in enumerate(case["remux"]["track_pid"]) if pid in nxt)


# ---------------------------------------------------------------------------------------- eight inputs
def _bytes(case, inputs=None, rstart=None, **rx):
    if case["remux"] is None:
        return R.mux(inputs or case["inputs"], case["n_out"], start=case["start"], **case["mux"]).ts
    return X.remux(inputs or case["inputs"], case["n_out"], start=case["start"], rstart=rstart or case["rstart"],
                   **dict(case["remux"], **rx), **case["mux"])[0].ts


def test_plain8_every_input_is_live_and_the_fill_rank_depends_on_the_late_inputs():
    case = BY_NAME["plain8"]
    ref, _ = L.reference(case)
    c = ref.counters
    assert c["consumed"] == (87, 40, 35, 0, 29, 26, 25, 13) and c["dry_slots"] == (0, 25, 17, 40, 10, 0, 1, 0)
    assert c["fill_in_free"] == 87 and c["pcr_packets"] == 26 and c["null_packets"] == 19 and c["sync_errors"] == 0
    assert ref.resume == (11 + 300 - 13 * 23, (W - 40000 + 13 * 23017) % W, (90, 40, 37, 0, 30, 1, 25, 6))
    assert ref.resume[1] < 300000                                     # the clock wrapped inside the call
    ins = case["inputs"]

    def fill_slots(inputs):
        """the slots that carry the fill input's packets, and the bytes"""
        ts = _bytes(case, inputs)
        return [m for m in range(300) if ts[188 * m + 2] == 0x01 and ts[188 * m + 1] == 0x01], ts

    own, ts = fill_slots(ins)
    np.testing.assert_array_equal(ts, ref.ts)
    assert len(own) == 87 and own[-1] < 299                           # the fill input runs dry mid-call
    swapped, ts4 = fill_slots(ins[:4] + [ins[6], ins[5], ins[4], ins[7]])
    one_more, ts3 = fill_slots(ins[:3] + [ins[1][:188]] + ins[4:])
    assert (ts4 != ref.ts).any() and (ts3 != ref.ts).any()
    # not only the swapped inputs' own slots differ: the fill input's packets leave in other slots, because the late
    # inputs run dry elsewhere, and a packet in input 3 takes a slot the fill input had
    assert swapped != own and one_more != own and len(swapped) == len(one_more) == 87


def test_remux8_moves_every_table_and_its_bytes_depend_on_every_argument():
    case = BY_NAME["remux8"]
    ref, rref = L.reference(case)
    c, rc, rx = ref.counters, rref.counters, case["remux"]
    assert len(rx["map"]) == len(rx["track_pid"]) == 64
    assert c["consumed"] == (87, 40, 35, 0, 29, 26, 25, 13) and c["dry_slots"] == (0, 25, 17, 40, 10, 0, 1, 0)
    assert c["fill_in_free"] == 87 and c["pcr_packets"] == 26 and c["null_packets"] == 50 and c["sync_errors"] == 0
    assert rc == dict(remapped=224, dropped=31, cc_rewritten=203, pcr_restamped=7)
    assert all(v > 0 for i, v in enumerate(c["consumed"]) if i != 3)
    cc0, in_phase, in_ticks = case["rstart"]
    moved = [s for s in range(64) if rref.resume[0][s] != cc0[s]]
    assert len(moved) == 39 and {s >> 4 for s in moved} == {0, 1, 2, 3}
    # from (5 s + 3) & 15 the same call rewrites 213 counters; those four words are alike, so the case adds 3 per word
    alike = tuple((5 * s + 3) & 15 for s in range(64))
    assert alike[:16] == alike[16:32] == alike[32:48] == alike[48:]
    lit = X.remux(case["inputs"], 300, start=case["start"], rstart=(alike, in_phase, in_ticks), **rx, **case["mux"])
    assert lit[1].counters == dict(remapped=224, dropped=31, cc_rewritten=213, pcr_restamped=7)
    assert sum(a != b for a, b in zip(lit[1].resume[0], alike)) == 39 and lit[0].counters == c
    for w in range(4):          # every word holds every value, and no two words are alike
        assert sorted(cc0[16 * w:16 * w + 16]) == list(range(16))
        assert all(cc0[16 * w:16 * w + 16] != cc0[16 * v:16 * v + 16] for v in range(w))
    assert rref.resume[1] == (0,) * 7 + ((1 + 13) % 3,) and rref.resume[2] == (0,) * 7 + ((W - 500 + 4 * 1000) % W,)
    # the reference's bytes under perturbed arguments: what a kernel reading the wrong nibble, word, bit or row would give
    perturbed = {
        "counters rotated by one slot": dict(rstart=(cc0[-1:] + cc0[:-1], in_phase, in_ticks)),
        "counter words 1 and 2 swapped": dict(rstart=(cc0[:16] + cc0[32:48] + cc0[16:32] + cc0[48:], in_phase, in_ticks)),
        "restamp_cc[7] cleared": dict(restamp_cc=(1,) * 7 + (0,)),
        "restamp_cc[3..6] cleared": dict(restamp_cc=(1, 1, 1, 0, 0, 0, 0, 1)),
        "input 6's map entries removed": dict(map=tuple(e for e in rx["map"] if e[0] != 6)),
        "one map entry of input 6 removed": dict(map=tuple(e for e in rx["map"] if e[:2] != (6, 0x133))),
        "in_phase[7] = 0": dict(rstart=(cc0, (0,) * 8, in_ticks)),
    }
    for name, kw in perturbed.items():
        assert (_bytes(case, **kw) != ref.ts).any(), name
    for i in range(8):          # and each input's own restamp bit, map row and result word
        if i != 3:
            assert (_bytes(case, restamp_cc=tuple(int(k != i) for k in range(8))) != ref.ts).any(), i
            assert (_bytes(case, map=tuple(e for e in rx["map"] if e[0] != i)) != ref.ts).any(), i


# ---------------------------------------------------------------------------------------- the sweep
def test_sweep_covers_every_width_and_every_counter():
    assert len(SWEEP) == L.SWEEP_CASES == 48 and len({c["name"] for c in SWEEP}) == 48
    refs = [L.reference(c) for c in SWEEP]
    widths = [len(c["mux"]["weight"]) for c in SWEEP]
    assert all(widths.count(n) >= 3 for n in range(1, 9)), widths
    for name in ("fill_in_free", "null_packets", "pcr_packets", "sync_errors"):
        assert sum(r.counters[name] > 0 for r, _ in refs) >= 5, name
    assert sum(any(r.counters["dry_slots"]) for r, _ in refs) >= 5
    for name in X.REMUX_COUNTERS:
        assert sum(rr.counters[name] > 0 for _, rr in refs if rr) >= 5, name
    assert 16 <= sum(c["remux"] is not None for c in SWEEP) <= 32
    assert sum(c["n_out"] > L.TILE for c in SWEEP) >= 10
    assert sum(c["n_out"] == 0 or not any(len(x) for x in c["inputs"]) for c in SWEEP) >= 3
    assert sum(c["mux"]["fill_input"] >= 0 and c["mux"]["weight"][c["mux"]["fill_input"]] == 0 for c in SWEEP) >= 5
    assert sum(any(c["mux"]["loop"]) for c in SWEEP) >= 10 and sum(0 < c["split"] < c["n_out"] for c in SWEEP) >= 30
    # the fill input ran dry mid-call: it had packets, all were taken, and one more would have been taken too
    dry = 0
    for c, (r, _) in zip(SWEEP, refs):
        f = c["mux"]["fill_input"]
        avail = len(c["inputs"][f]) // 188 - c["start"][2][f] if f >= 0 else 0
        if avail > 0 and r.counters["consumed"][f] == avail:
            more = list(c["inputs"])
            more[f] = np.concatenate([more[f], R.NULL])
            dry += R.mux(more, c["n_out"], start=c["start"], **c["mux"]).counters["consumed"][f] == avail + 1
    assert dry >= 5
    # the remux rules the sweep is to mix: merges, drops, entries that never match, both mux clocks
    rxs = [c["remux"] for c in SWEEP if c["remux"] is not None]
    assert sum(len({t for _, _, t in x["map"]} - {0x1FFF}) < sum(t != 0x1FFF for _, _, t in x["map"]) for x in rxs) >= 3
    assert sum(any(f >= 0x7F0 for _, f, _ in x["map"]) for x in rxs) >= 3
    assert sum(x["out_ticks_per_period"] > 0 for x in rxs) >= 3 and sum(any(x["in_period"]) for x in rxs) >= 5
    assert max(len(x["map"]) for x in rxs) == 12 and max(len(x["track_pid"]) for x in rxs) >= 15
