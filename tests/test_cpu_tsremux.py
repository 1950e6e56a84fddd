"""CPU: the host side of the multiplexer's remux (dvbt2ll_tsmux_remux_check) and tests/tsremux_ref.py's own properties:
the reference against the independent checker on every case, chaining at every split, two hand-derived known answers."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _TsMuxParams, _TsMuxRemux, _TsMuxRemuxPos, _TsMuxRemuxResult
from dvbt2ll.tsmux import remux_params
import tsmux_cases as C
import tsmux_ref as R
import tsremux_cases as XC
import tsremux_ref as X

CASES = XC.cases()


def _params(kw, max_out=1 << 16):
    p = _TsMuxParams()
    p.n_inputs, p.period, p.fill_input = len(kw["weight"]), kw["period"], kw["fill_input"]
    for i, w in enumerate(kw["weight"]):
        p.weight[i], p.loop[i] = w, kw["loop"][i]
    p.pcr_pid, p.pcr_weight, p.ticks_per_period, p.max_out_packets = (kw["pcr_pid"], kw["pcr_weight"],
                                                                      kw["ticks_per_period"], max_out)
    return p


def _check(p, **kw):
    return dvbt2ll.lib().dvbt2ll_tsmux_remux_check(ctypes.byref(p), ctypes.byref(remux_params(**kw)))


def test_the_cases_shapes_follow_the_kernel_headers_constants():
    text = (Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "csrc" / "tsmux_kernels.h").read_text()
    pkts = int(re.search(r"TSMUX_PKTS = (\d+);", text).group(1))
    assert re.search(r"TSREMUX_TILE = TSMUX_PKTS;", text) and pkts == XC.TILE
    assert int(re.search(r"TSREMUX_SCAN_TILES = (\d+);", text).group(1)) == XC.SCAN_TILES


def test_remux_check_accepts_the_cases_and_refuses_bad_configurations():
    for case in CASES:
        assert _check(_params(case["mux"]), **case["remux"]) == 0, case["name"]
    plain = _params(XC._mux(7, (3, 2)))
    own = _params(XC._mux(7, (3, 2), pcr_pid=0x1FF, pcr_weight=1, ticks_per_period=7001))
    assert _check(plain) == 0 and _check(own, out_ticks_per_period=7001) == 0
    assert _check(plain, map=[(0, 5, 6)] * 1 + [(1, 5, 6)], track_pid=range(64), out_ticks_per_period=(1 << 36) - 1) == 0
    assert _check(plain, map=[(k % 2, k, 0x1FFF) for k in range(64)], in_period=[65536, 1],
                  in_ticks_per_period=[1, (1 << 36) - 1]) == 0
    bad = [(plain, dict(map=[(0, 5, 6), (0, 5, 7)])),                        # (input, from) twice
           (plain, dict(track_pid=[7, 8, 7])),                                # a tracked PID twice
           (own, dict(map=[(0, 5, 0x1FF)])),                                  # a target equal to pcr_pid
           (own, dict(track_pid=[0x1FF])),                                    # a tracked PID equal to pcr_pid
           (plain, dict(map=[(2, 5, 6)])), (plain, dict(map=[(-1, 5, 6)])),   # an input index >= n_inputs
           (plain, dict(map=[(0, 0x2000, 6)])), (plain, dict(map=[(0, 5, 0x2000)])), (plain, dict(map=[(0, -1, 6)])),
           (plain, dict(track_pid=[0x1FFF])), (plain, dict(track_pid=[-1])),
           (plain, dict(restamp_cc=[2])), (plain, dict(restamp_cc=[0, 0, 1])),
           (plain, dict(in_period=[0], in_ticks_per_period=[5])), (plain, dict(in_period=[65537], in_ticks_per_period=[5])),
           (plain, dict(in_period=[-1], in_ticks_per_period=[5])), (plain, dict(in_period=[3], in_ticks_per_period=[0])),
           (plain, dict(in_period=[3], in_ticks_per_period=[1 << 36])),
           (plain, dict(in_period=[0, 0, 3], in_ticks_per_period=[0, 0, 5])),
           (own, dict(out_ticks_per_period=7000)),                            # contradicts the handle's
           (plain, dict(out_ticks_per_period=1 << 36)), (plain, dict(out_ticks_per_period=-1))]
    for k, (p, kw) in enumerate(bad):
        assert _check(p, **kw) == -1, (k, kw)
    for n_map, n_track in ((65, 0), (0, 65), (-1, 0), (0, -1)):
        x = remux_params()
        x.n_map, x.n_track = n_map, n_track
        assert dvbt2ll.lib().dvbt2ll_tsmux_remux_check(ctypes.byref(plain), ctypes.byref(x)) == -1
    L = dvbt2ll.lib()
    assert L.dvbt2ll_tsmux_remux_check(None, ctypes.byref(remux_params())) == -1
    assert L.dvbt2ll_tsmux_remux_check(ctypes.byref(plain), None) == -1
    plain.period = 0
    assert _check(plain) == -1                                                # params the schedule refuses
    pos, res = _TsMuxRemuxPos(), _TsMuxRemuxResult()
    assert L.dvbt2ll_tsmux_set_remux(None, ctypes.byref(remux_params())) == -1
    assert L.dvbt2ll_tsmux_get_remux_result(None, ctypes.byref(res)) == -1
    assert L.dvbt2ll_tsmux_run_device_remux(None, None, None, None, ctypes.byref(pos), None, 1, None) == -1
    for n in ("remux_check", "set_remux", "run_device_remux", "get_remux_result", "run_host_remux"):
        assert "dvbt2ll_tsmux_" + n in dvbt2ll.EXPORTS
    assert (ctypes.sizeof(_TsMuxRemux), ctypes.sizeof(_TsMuxRemuxPos), ctypes.sizeof(_TsMuxRemuxResult)) == (1168, 352, 384)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_passes_the_checker(case):
    res, rres = X.remux(case["inputs"], case["n_out"], start=case["start"], rstart=case["rstart"], **case["remux"],
                        **case["mux"])
    first = {pid: case["rstart"][0][s] for s, pid in enumerate(case["remux"]["track_pid"]) if pid in case["cont"]}
    nxt = X.check_continuity(res.ts, pids=case["cont"], first=first)
    for s, pid in enumerate(case["remux"]["track_pid"]):
        if pid in case["cont"] and pid in nxt:
            assert rres.resume[0][s] == nxt[pid], (case["name"], hex(pid))
    tpp = case["mux"]["ticks_per_period"] if case["mux"]["pcr_pid"] >= 0 else case["remux"]["out_ticks_per_period"]
    const = X.check_pcr(res.ts, case["mux"]["period"], tpp, case["start"][:2], pids=case["pcr"])
    assert set(const) == set(case["pcr"])
    if case["cont"] or case["pcr"]:
        assert rres.counters["cc_rewritten"] + rres.counters["pcr_restamped"] > 0


def _sum(parts):
    return {k: sum(p[k] for p in parts) if not isinstance(parts[0][k], tuple) else
            tuple(sum(v) for v in zip(*[p[k] for p in parts])) for k in parts[0]}


def test_reference_chains_at_every_split():
    case = XC.all_case()
    kw = dict(case["remux"], **case["mux"])
    whole, rwhole = X.remux(case["inputs"], 200, start=case["start"], rstart=case["rstart"], **kw)
    assert min(rwhole.counters.values()) > 0 and whole.counters["sync_errors"] == 1
    for k in range(201):
        a, ra = X.remux(case["inputs"], k, start=case["start"], rstart=case["rstart"], **kw)
        b, rb = X.remux(case["inputs"], 200 - k, start=a.resume, rstart=ra.resume, **kw)
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts, err_msg=str(k))
        assert b.resume == whole.resume and rb.resume == rwhole.resume, k
        assert _sum([a.counters, b.counters]) == whole.counters and _sum([ra.counters, rb.counters]) == rwhole.counters, k


def test_a_three_packet_loop_over_five_laps_counts_from_0_to_14():
    """hand-derived: three packets of one PID, counters 7, 7, 7, read round and round for 15 slots from cc 0 leave
    with 0 .. 14, and the next one would take 15"""
    car = C.stream(3, 0x102)
    car.reshape(-1, 188)[:, 3] = 0x17
    res, rres = X.remux([car], 15, track_pid=[0x102], restamp_cc=[1], period=1, weight=(1,), loop=(1,))
    assert [int(p[3]) for p in res.ts.reshape(-1, 188)] == [0x10 | k for k in range(15)]
    assert rres.resume[0][0] == 15 and rres.counters["cc_rewritten"] == 14       # the packet that took 7 kept its nibble
    assert res.resume == (0, 0, (0,) * 8) and res.counters["consumed"] == (15,)


def test_exact_input_pcrs_leave_with_one_offset_and_unrestamped_ones_do_not():
    """hand-derived: input PCRs of exactly c + T_in(j) leave with PCR_out - T_out(m) = c on every PCR packet, exactly:
    PCR_out = PCR_in + T_out - T_in = c + T_out.  Without restamping the same input fails the check"""
    c = 123456789
    for own in (True, False):
        case = XC.pcr_case(own, c=c)
        res, rres = X.remux(case["inputs"], case["n_out"], start=case["start"], rstart=case["rstart"], **case["remux"],
                            **case["mux"])
        const = X.check_pcr(res.ts, 7, 7001, case["start"][:2], pids=(0x101, 0x102))
        assert const == {0x101: c, 0x102: 5} and rres.counters["pcr_restamped"] > 20
        plain = R.mux(case["inputs"], case["n_out"], start=case["start"], **case["mux"])
        with pytest.raises(AssertionError):
            X.check_pcr(plain.ts, 7, 7001, case["start"][:2], pids=(0x101,))
    # one value by hand: P = 1, the mux clock 100 per slot from 1000; the input's clock 30 per 3 packets from phase 1,
    # 500: packet j = 4 lies at 500 + 1 x 30 + floor(2 x 30 / 3) = 550 and leaves in slot 4 at 1400
    ts = C.stream(5, 0x101)
    p = ts.reshape(-1, 188)
    p[4, 3:6] = (0x30, 7, 0x10)
    X.put_pcr(p[4], 9000 + 550)
    res, _ = X.remux([ts], 5, in_period=[3], in_ticks_per_period=[30], out_ticks_per_period=100, period=1, weight=(1,),
                     start=(0, 1000, (0,) * 8), rstart=((0,) * 64, (1,) + (0,) * 7, (500,) + (0,) * 7))
    assert X.pcr_of(res.ts.reshape(-1, 188)[4]) == 9000 + 1400
    with pytest.raises(AssertionError):
        bad = res.ts.copy()
        bad[188 * 3 + 3] ^= 1
        X.check_continuity(bad)
