"""GPU: the mode adapter and the T2-MI deframer at the smallest sizes at which their device-wide scans take a second
and a third round and their capped grids loop.  Both files share one three-launch scan whose middle kernel
(modeadapt_scan_tiles / t2mi_scan_tiles) takes the tile sums 256 at a time and carries a running total from trip to
trip: the second trip begins at element R = 256 * 1024 = 262 144, the third (a carry built from a carry) at 2R.

The sequential references cannot do these sizes; the expected results come from tests/large_ref.py (adapt_fast, and
big_t2mi's result by construction), which tests/test_cpu_large_ref.py proves against them at small sizes, and which
the same module shows to depend on every scan's carry at exactly these streams.  Every run goes through the device_run
of tests/test_gpu_modeadapt.py / tests/test_gpu_t2mi.py: TS and outputs inside poisoned arrays with guards.  Each test's
docstring names the carries and loops it is the pin for."""
import functools

import numpy as np
import pytest

import dvbt2ll
import large_ref as G
import modeadapt_cases as C
import modeadapt_ref as MR
from test_gpu_modeadapt import device_run as ma_run, same as ma_same
from test_gpu_t2mi import device_run as t2mi_run, same as t2mi_same

pytestmark = pytest.mark.gpu

R = G.ROUND_TILES * 1024


# ---------------------------------------------------------------------------------------- mode adapter
@functools.lru_cache(maxsize=None)
def big_ts():
    ts, mk = G.big_ts(1024)
    assert mk["R"] == R and len(ts) == 188 * (2 * R + 1024 + 7)
    return ts, mk, MR.mask_of(mk["pids"])


@functools.lru_cache(maxsize=None)
def whole_ref(kbch):
    ts, mk, mask = big_ts()
    return G.adapt_fast(ts, kbch, mask=mask, flush=True)


def adapter(kbch, nbytes, **kw):
    return dvbt2ll.ModeAdapter(kbch=kbch, max_ts_bytes=nbytes, **kw)


def test_modeadapt_npd0_second_round(gpu):
    """the first R + 1024 + 1 packets without deletion (emit<false>, U = 187), short 1/4.  Second trips: the sum-scan's
    carry in modeadapt_scan_tiles (every unit index past packet R), modeadapt_count's loop (capped at 1024 x 256
    packets), and 32 trips of modeadapt_emit<false>'s loop (capped at 4096 workgroups, one BBFRAME each, the LDS
    header rewritten between barriers)"""
    ts = big_ts()[0][:188 * (R + 1024 + 1)]
    ad = adapter(C.KBCH_SHORT14, len(ts), npd=0)
    ref = G.adapt_fast(ts, C.KBCH_SHORT14, npd=0, flush=True)
    assert ref.counters["bbframes"] > 32 * 4096
    ma_same(ma_run(ad, ts, flush=True), ref, "npd 0")


def test_modeadapt_short_quarter_three_rounds(gpu):
    """2R + 1024 + 7 packets under a two-PID mask, short 1/4, flush: about 259 000 BBFRAMEs.  The max-scan's carry
    (MaMax in modeadapt_scan_tiles) into the second and third round: null runs of more than 3 x 1024 packets lie
    across packets R and 2R with whole tiles of nulls on both sides, so which null is kept (packets R and 2R are)
    and every DNP after them come from the carried maximum.  The sum-scan's carry and carry of a carry: every unit
    index past R and 2R.  64 trips of modeadapt_emit<true>'s loop over 4096 workgroups; three of modeadapt_count's"""
    ts, mk, mask = big_ts()
    ref = whole_ref(C.KBCH_SHORT14)
    assert ref.counters["bbframes"] > 63 * 4096 and ref.counters["sync_errors"] == 5
    assert ref.counters["nulls_kept"] >= 2 * 9 and ref.counters["nulls_dropped_at_flush"] == 4
    ad = adapter(C.KBCH_SHORT14, len(ts), pids=list(mk["pids"]))
    ma_same(ma_run(ad, ts, flush=True), ref, "3072")


def test_modeadapt_odd_code_three_rounds(gpu):
    """the same stream, normal 3/4 (L = 6051: the store alignment moves from BBFRAME to BBFRAME): more than
    2 x 4096 BBFRAMEs, so modeadapt_emit<true>'s workgroups make a second and third trip with the long frame too; the
    scans' carries as above"""
    ts, mk, mask = big_ts()
    ref = whole_ref(C.KBCH_ODD)
    assert ref.counters["bbframes"] > 2 * 4096
    ad = adapter(C.KBCH_ODD, len(ts), pids=list(mk["pids"]))
    ma_same(ma_run(ad, ts, flush=True, misalign=1), ref, "48408")


def test_modeadapt_capacity_cut_past_2R_then_continuation(gpu):
    """a capacity that ends the call on a packet past 2R: the resume position (modeadapt_count reads unit[] at an
    index that the sum-scan's carry of a carry produced) and the counters of three trips of modeadapt_count's
    loop; then the rest from that position on ts[resume:]: together the whole-stream result"""
    ts, mk, mask = big_ts()
    whole = whole_ref(C.KBCH_SHORT14)
    tx = G.classify_ts(ts.reshape(-1, 188), 1, mask)[1]
    cap = int(tx[:2 * R + 2].sum()) * 188 // 374 + 1
    ref_a = G.adapt_fast(ts, C.KBCH_SHORT14, mask=mask, cap=cap, flush=True)
    assert ref_a.resume[0] > 2 * R and ref_a.counters["bbframes"] == cap and ref_a.counters["flushed"] == 0
    ad = adapter(C.KBCH_SHORT14, len(ts), pids=list(mk["pids"]))
    a = ma_run(ad, ts, cap=cap, flush=True)
    ma_same(a, ref_a, "cut")
    rest = ts[188 * a.resume.ts_packet:]
    start = (0, a.resume.unit_byte, a.resume.dnp)
    b = ma_run(ad, rest, start=start, flush=True, misalign=2)
    ma_same(b, G.adapt_fast(rest, C.KBCH_SHORT14, mask=mask, start=start, flush=True), "rest")
    np.testing.assert_array_equal(np.concatenate([a.bbframes, b.bbframes]), whole.bbframes)
    assert {n: a.counters[n] + b.counters[n] for n in MR.COUNTERS} == whole.counters


# ---------------------------------------------------------------------------------------- T2-MI
@functools.lru_cache(maxsize=None)
def big_t2mi():
    ts, exp = G.big_t2mi(1024)
    assert exp.R == R and exp.ncontributing >= 2 * R + 1 and exp.npackets >= R + 1
    return np.array(ts), exp        # a writable copy: torch.from_numpy warns about read-only arrays


def deframer(ts, max_packets):
    return dvbt2ll.T2miDeframer(G.T2_PID, plps=G.PLPS, max_ts_bytes=len(ts), max_packets=max_packets)


def room(exp):
    return [int(g[-1]) + 2 for g in exp.rank]


def test_t2mi_whole_run_three_rounds(gpu):
    """more than 2R contributing TS packets, more than R T2-MI packets, two PLPs (L = 6051 and 879), the table larger
    than the packet count.  Carries in t2mi_scan_tiles: scan A (stream offsets and compact indices of every
    contributing packet past TS packets R and 2R; foreign, null and adaptation-field-only packets before both, so
    compact index != TS index), scan B (the table position of every start in a contributing packet past R and 2R),
    scan C as T2miV8 (the rank of every block past T2-MI packet R, after a CRC error, an unlisted PLP_ID and a
    length error that lie past packet R and TS packet 2R).  Loops past their grid caps: t2mi_check (4096 x 4
    wavefronts), t2mi_emit (4096 workgroups), t2mi_cut and t2mi_count_ts (1024 x 256 each)"""
    ts, exp = big_t2mi()
    want = exp.call()
    assert want.counters["crc_errors"] == want.counters["other_plp"] == want.counters["len_errors"] == 1
    assert exp.npackets > 16 * 16384 and exp.nts > 2 * 262144
    res = t2mi_run(deframer(ts, exp.npackets + 1000), ts, caps=room(exp))
    t2mi_same(res, want, "whole")


def _continued(de, ts, exp, first, j_cut, **kw):
    """the call `first` must end before packet j_cut; the next one from its resume position must give the rest"""
    want = exp.call(**kw)
    assert len(want.packets) == j_cut and want.resume == exp.start(j_cut)
    t2mi_same(first, want, "cut")
    rest = t2mi_run(de, ts, start=first.resume, caps=room(exp), misalign=1)
    t2mi_same(rest, exp.call(j_cut, max_packets=de.max_packets), "rest")
    tab = rest.packets.copy()
    for o in range(2):
        tab["block"][tab["out_index"] == o] += first.blocks[o]
        np.testing.assert_array_equal(np.concatenate([first.bbframes[o], rest.bbframes[o]]), exp.outputs[o])
    both = np.concatenate([first.packets, tab])
    assert (both == exp.table.astype(both.dtype)).all()


def test_t2mi_table_cut_past_R_then_continuation(gpu):
    """max_packets between R and the packet count, ending inside a burst of timestamp packets: the cut and the
    resume position's skip (t2mi_resume: cut + skip - nst[k], nst from scan B's carry) past T2-MI packet R, the
    TS-level counters of t2mi_count_ts's second and third trip; the continuation starts past TS packet 2R"""
    ts, exp = big_t2mi()
    M = exp.npackets - 3 * (G.BURST + 3) + 7
    assert R < M < exp.npackets and exp.within[M] > 0 and exp.ts_index[M] > 2 * R
    de = deframer(ts, M)
    first = t2mi_run(de, ts, caps=room(exp))
    assert first.resume[1] > 0
    _continued(de, ts, exp, first, M, max_packets=M)


def test_t2mi_output_cut_past_R_then_continuation(gpu):
    """PLP B's capacity ends at a block whose T2-MI packet lies past R: t2mi_cut compares ranks that scan C carried
    into its second round (and makes the second trip of its own loop to get there)"""
    ts, exp = big_t2mi()
    jcut = exp.npackets - 2 * (G.BURST + 3) + G.BURST + 1
    assert exp.table["out_index"][jcut] == 1 and jcut > R
    caps = [room(exp)[0], int(exp.rank[1][jcut])]
    de = deframer(ts, exp.npackets + 1000)
    first = t2mi_run(de, ts, caps=caps)
    assert first.blocks[1] == caps[1]
    _continued(de, ts, exp, first, jcut, caps=caps)
