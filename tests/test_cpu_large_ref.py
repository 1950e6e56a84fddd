"""CPU: the fast references of tests/large_ref.py against the sequential ones (tests/modeadapt_ref.py,
tests/t2mi_ref.py) at sizes those can do, and -- in numpy alone -- that the streams tests/test_gpu_large_runs.py
sends to the GPU make the carry of every device-wide scan matter: the exclusive scan of the kernel's input sequence
against the same scan with what earlier rounds carried lost, at an element whose value reaches the output."""
import functools

import numpy as np
import pytest

from dvbt2ll.configs import ts_packets
import large_ref as G
import modeadapt_cases as C
import modeadapt_ref as R
import t2mi_ref as TR


def both(ts, kbch, ctx="", **kw):
    ref, got = R.adapt(ts, kbch, **kw), G.adapt_fast(ts, kbch, **kw)
    assert tuple(got.resume) == tuple(ref.resume), (ctx, kw.get("start"), got.resume, ref.resume)
    assert got.counters == ref.counters, (ctx, got.counters, ref.counters)
    np.testing.assert_array_equal(got.bbframes, ref.bbframes, err_msg=str(ctx))
    return ref


def both_chunked(ts, kbch, cuts, flush=True, **kw):
    """modeadapt_ref.adapt_chunked's calls, each through both adapters"""
    rows = np.asarray(ts, np.uint8).reshape(-1, 188)
    ends = list(cuts) + [len(rows)]
    base, pos = 0, (0, 0, 0)
    for j, end in enumerate(ends):
        end = max(end, base)
        r = both(rows[base:end].reshape(-1), kbch, ("chunk", cuts, j), start=pos, flush=flush and j == len(ends) - 1,
                 **kw)
        base += r.resume[0]
        pos = (0, r.resume[1], r.resume[2])


# ---------------------------------------------------------------------------------------- adapt_fast == adapt
@pytest.mark.parametrize("kbch", [C.KBCH_SHORT14, C.KBCH_ODD])
@pytest.mark.parametrize("place", [0, 1, 2])
def test_adapt_fast_null_runs(place, kbch):
    for run in C.RUNS:
        for flush in (False, True):
            both(C.run_stream(run, place), kbch, (run, place, flush), flush=flush)


def test_adapt_fast_odd_code_runs_and_tiles():
    for run in (0, 255, 256, 600):
        ts = C.stream([(C.PID_A, 70), (C.PID_NULL, run), (C.PID_A, 70)], seed=run)
        both(ts, C.KBCH_ODD, run, flush=True)
        both(ts, C.KBCH_ODD, run)
    ts = C.two_tile_stream()
    both(ts, C.KBCH_SHORT14, "tiles", flush=True)
    r = both(ts, C.KBCH_ODD, "tiles odd", flush=True)
    assert r.counters["sync_errors"] == 3
    r = both(ts, C.KBCH_ODD, "cap 3", cap=3)
    both(ts, C.KBCH_ODD, "rest", start=tuple(r.resume), flush=True)


def test_adapt_fast_masks_and_no_deletion():
    ts = C.two_pid_stream()
    for pids in ([C.PID_A], [C.PID_B], [C.PID_A, C.PID_B]):
        for isi in (3, 5):
            both(ts, C.KBCH_SHORT14, pids, mask=R.mask_of(pids), sis=False, isi=isi, flush=True)
        both(ts, 7032, pids, mask=R.mask_of(pids), sis=False, isi=1, cap=2)
    both(ts, C.KBCH_ODD, "npd 0", npd=0, flush=True)
    both(C.two_pid_stream(groups=12), 7032, "cli", mask=R.mask_of([C.PID_A, C.PID_B]), flush=True)
    for run_pid in (C.PID_NULL, C.PID_FOREIGN):
        for a in (1, 2):
            ts = C.stream([(C.PID_A, a), (run_pid, 300), (C.PID_A, a)])
            both(ts, C.KBCH_SHORT14, "kept", mask=R.mask_of([C.PID_A]), flush=True)
            both(ts, C.KBCH_SHORT14, "kept, no mask", flush=True)
    for kbch, nb in ((5232, 12), (C.KBCH_ODD, 8), (5232, 6), (C.KBCH_ODD, 4)):
        ts = ts_packets(0, nb * (kbch - 80) // 8 // 187 + 2)
        both(ts, kbch, "npd 0 oracle shape", npd=0, cap=nb)
        ts = ts.copy()
        ts[::188 * 3] = 0x46
        both(ts, kbch, "npd 0 bad syncs", npd=0, cap=nb)


def test_adapt_fast_split_points():
    ts = C.split_stream()
    n = len(ts) // 188
    for kbch, npd in ((C.KBCH_SHORT14, 1), (C.KBCH_SHORT14, 0), (5232, 1)):
        both(ts, kbch, "whole", npd=npd, flush=True)
        for cut in range(n + 1):
            both_chunked(ts, kbch, [cut], npd=npd)
    ts = C.long_run_stream()
    both(ts, C.KBCH_SHORT14, "long run", flush=True)
    rng = np.random.default_rng(2)
    cuts = [[258], [259], [300], [3 + 511], [3 + 512]] + [sorted(rng.integers(0, 710, 3)) for _ in range(20)]
    for c in cuts + [[2], [100], [3 + 255], [3 + 256], [3 + 700]]:
        both_chunked(ts, C.KBCH_SHORT14, [int(x) for x in c])


def test_adapt_fast_capacity_and_flush_edges():
    ts = C.run_stream(257, 1)
    whole = both(ts, C.KBCH_SHORT14, "whole", flush=True)
    for k in range(whole.counters["bbframes"] + 1):
        a = both(ts, C.KBCH_SHORT14, "cap %d" % k, cap=k, flush=True)
        both(ts, C.KBCH_SHORT14, "cap %d rest" % k, start=a.resume, flush=True)
    exact = C.stream([(C.PID_A, 187)], seed=2)
    both(exact, C.KBCH_SHORT14, "exact", flush=True)
    both(exact, C.KBCH_SHORT14, "exact, no flush")
    both(C.stream([(C.PID_A, 188)], seed=2), C.KBCH_SHORT14, "partial", flush=True)
    trailing = C.stream([(C.PID_A, 187), (C.PID_NULL, 9)], seed=2)
    both(trailing, C.KBCH_SHORT14, "trailing nulls", flush=True)
    both(trailing, C.KBCH_SHORT14, "trailing nulls, no flush")
    both(C.stream([(C.PID_NULL, 40)]), C.KBCH_SHORT14, "only nulls", flush=True)
    r = both(exact[:188], C.KBCH_SHORT14, "no unit begins", start=(0, 184, 7), flush=True)
    assert list(r.bbframes[7:9]) == [0xFF, 0xFF]
    three = C.stream([(C.PID_A, 3)])
    both(three, 3072, "three", flush=True)
    both(three, 3072, "three, no flush")
    both(three, 3072, "at the end", start=(3, 0, 0), flush=True)
    both(three, 3072, "at the end, no flush", start=(3, 0, 0))


@functools.lru_cache(maxsize=None)
def small_ts():
    return G.big_ts(8, round_tiles=160)


def test_adapt_fast_on_the_big_streams_structure():
    """big_ts at tile size 8 and a round of 160 tiles (2575 packets): both runs, the kept nulls on packets R and
    2R, foreign PIDs, bad sync bytes, trailing nulls; both codes, a cut past 2R with its continuation, npd 0"""
    ts, mk = small_ts()
    assert mk["n"] == len(ts) // 188 <= 3000
    mask = R.mask_of(mk["pids"])
    for kbch in (C.KBCH_SHORT14, C.KBCH_ODD):
        whole = both(ts, kbch, "big %d" % kbch, mask=mask, flush=True)
        assert whole.counters["nulls_dropped_at_flush"] == 4 and whole.counters["sync_errors"] == 5
        both(ts, kbch, "big, no flush", mask=mask)
    sel, tx, t, dnp = G.classify_ts(ts.reshape(-1, 188), 1, mask)
    assert tx[mk["R"]] and not sel[mk["R"]] and tx[2 * mk["R"]] and not sel[2 * mk["R"]]     # the kept nulls
    units_to_2R = int(tx[:2 * mk["R"] + 2].sum())
    cap = units_to_2R * 188 // 374 + 1
    a = both(ts, C.KBCH_SHORT14, "cut", mask=mask, cap=cap, flush=True)
    assert a.resume[0] > 2 * mk["R"] and a.counters["bbframes"] == cap
    both(ts[188 * a.resume[0]:], C.KBCH_SHORT14, "rest", mask=mask, start=(0,) + tuple(a.resume[1:]), flush=True)
    both(ts[:188 * (mk["R"] + 8 + 1)], C.KBCH_SHORT14, "npd 0", npd=0, flush=True)
    ts, mk = G.big_ts(8)                   # the round of 256 tiles as well: 4111 packets
    both(ts, C.KBCH_SHORT14, "256 tiles", mask=mask, flush=True)


# ---------------------------------------------------------------------------------------- big_t2mi == parse
def same_t2mi(exp, ref, ctx):
    assert exp.resume == ref.resume, (ctx, exp.resume, ref.resume)
    assert exp.counters == ref.counters, (ctx, exp.counters, ref.counters)
    assert exp.blocks == ref.blocks and exp.by_type == ref.by_type, (ctx, exp.blocks, ref.blocks)
    assert len(exp.packets) == len(ref.packets), (ctx, len(exp.packets), len(ref.packets))
    for name in TR.REC.names:
        np.testing.assert_array_equal(exp.packets[name], ref.packets[name], err_msg="%s %s" % (ctx, name))
    for k, (a, b) in enumerate(zip(exp.bbframes, ref.bbframes)):
        np.testing.assert_array_equal(a, b, err_msg="%s output %d" % (ctx, k))


@functools.lru_cache(maxsize=None)
def small_t2mi():
    return G.big_t2mi(8)


def test_big_t2mi_expected_is_what_the_parser_finds():
    ts, exp = small_t2mi()
    whole = TR.parse(ts, G.T2_PID, G.PLPS)
    same_t2mi(exp.call(), whole, "whole")
    c = whole.counters
    assert (c["crc_errors"], c["other_plp"], c["len_errors"], c["broken"]) == (1, 1, 1, 0)
    assert c["ts_foreign"] == c["ts_null"] == c["ts_no_payload"] == 7
    assert c["ts_contributing"] == exp.ncontributing > 2 * exp.R and exp.npackets > exp.R + 1
    for j in exp.malformed.values():
        assert j > exp.R and exp.ts_index[j] > 2 * exp.R
    assert int(np.bincount(whole.packets["ts_index"]).max()) >= 8          # a burst: many starts in one TS packet


def test_big_t2mi_cuts_in_the_far_region():
    """a table capacity and an output capacity that cut past T2-MI packet R (in a burst: the resume position has a
    skip), each with its continuation"""
    ts, exp = small_t2mi()
    M = exp.npackets - 3 * (G.BURST + 3) + 7
    assert exp.R < M < exp.npackets and exp.within[M] > 0
    a = TR.parse(ts, G.T2_PID, G.PLPS, max_packets=M)
    same_t2mi(exp.call(max_packets=M), a, "table cut")
    assert a.resume == exp.start(M) and a.resume[1] > 0
    same_t2mi(exp.call(M, max_packets=M), TR.parse(ts, G.T2_PID, G.PLPS, start=a.resume, max_packets=M), "table rest")
    jcut = exp.npackets - 2 * (G.BURST + 3) + G.BURST + 1                   # PLP B's first block of frame -2
    assert exp.table["out_index"][jcut] == 1 and jcut > exp.R
    caps = [1 << 30, int(exp.rank[1][jcut])]
    b = TR.parse(ts, G.T2_PID, G.PLPS, caps=caps)
    same_t2mi(exp.call(caps=caps), b, "output cut")
    assert len(b.packets) == jcut and b.resume == exp.start(jcut)
    same_t2mi(exp.call(jcut), TR.parse(ts, G.T2_PID, G.PLPS, start=b.resume), "output rest")


# ---------------------------------------------------------------------------------------- the carries matter
@functools.lru_cache(maxsize=None)
def gpu_ts():
    return G.big_ts(1024)


@functools.lru_cache(maxsize=None)
def gpu_t2mi():
    return G.big_t2mi(1024)


def test_mode_adapter_scans_need_their_carries():
    """big_ts(1024).  Max-scan (input: index + 1 of a selected packet, else 0): a null past R, and one past 2R, whose
    last selected packet lies before the boundary is kept with the carry and deleted without (or the reverse).
    Sum-scan (input: transmitted flags): a transmitted packet past each boundary gets another unit index."""
    ts, mk = gpu_ts()
    R_ = mk["R"]
    assert R_ == 262144 and mk["n"] == 2 * R_ + 1024 + 7
    rows = ts.reshape(-1, 188)
    sel, tx, t, dnp = G.classify_ts(rows, 1, R.mask_of(mk["pids"]))
    i = np.arange(len(rows))
    for at, (b, e) in ((R_, mk["run1"]), (2 * R_, mk["run2"])):
        assert b < at - 2 * 1024 and e >= at + 1024 and e - b >= 3 * 1024 and not sel[b:e].any()
        true, lost = G.scan_dropping_carry(np.where(sel, i + 1, 0), at, np.maximum)
        nulls = np.flatnonzero(~sel & (i >= at) & (true < at))
        kept_true = ((nulls - true[nulls]) & 255) == 255
        kept_lost = ((nulls - lost[nulls]) & 255) == 255
        assert (kept_true != kept_lost).any() and kept_true[nulls == at].all()      # packet `at` is a kept null
        np.testing.assert_array_equal(kept_true, tx[nulls])
        true, lost = G.scan_dropping_carry(tx.astype(np.int64), at)
        sent = np.flatnonzero(tx & (i >= at))
        assert sent.size and (true[sent] != lost[sent]).all()


def test_t2mi_scans_need_their_carries():
    """big_t2mi(1024).  Scan A (per TS packet: payload length and contributing flag, packed): contributing packets
    past TS packets R and 2R.  Scan B (starts per contributing packet): packets with starts past compact index R and
    2R.  Scan C (per T2-MI packet and output: carries a block): blocks of both outputs past T2-MI packet R."""
    ts, exp = gpu_t2mi()
    R_ = exp.R
    assert R_ == 262144 and exp.nts >= exp.ncontributing >= 2 * R_ + 1 and exp.npackets >= R_ + 1
    a = np.zeros(exp.nts, np.uint64)
    a[exp.tsidx] = (exp.payload_len.astype(np.uint64) << np.uint64(32)) | np.uint64(1)
    b = np.zeros(exp.nts, np.int64)
    b[:exp.ncontributing] = exp.starts_per_contributing
    for at in (R_, 2 * R_):
        true, lost = G.scan_dropping_carry(a, at)
        hit = exp.tsidx[exp.tsidx >= at]
        assert hit.size and (true[hit] != lost[hit]).all()
        assert (exp.tsidx[at - 100:at + 100] != np.arange(at - 100, at + 100)).all()     # compact index != TS index
        true, lost = G.scan_dropping_carry(b, at)
        hit = np.flatnonzero((b > 0) & (np.arange(exp.nts) >= at))
        assert hit.size and (true[hit] != lost[hit]).all()
    for o in range(2):
        c = (exp.table["out_index"] == o).astype(np.int64)
        true, lost = G.scan_dropping_carry(c, R_)
        hit = np.flatnonzero((c > 0) & (np.arange(exp.npackets) > R_))
        assert hit.size and (true[hit] != lost[hit]).all()
        np.testing.assert_array_equal(true[c > 0], exp.table["block"][c > 0])
    for j in exp.malformed.values():
        assert j > R_ and exp.ts_index[j] > 2 * R_ and (exp.table["out_index"][j + 1:] >= 0).any()
