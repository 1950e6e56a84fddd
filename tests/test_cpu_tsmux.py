"""CPU: the host side of the TS multiplexer (dvbt2ll_tsmux_schedule, dvbt2ll_tsmux_ticks_per_period, dvbt2ll_psi_build)
against tests/tsmux_ref.py -- the schedule tables, the PAT known answer, the carousel's structure through the
independent checker, the refusals -- and the reference multiplexer's own properties (chained calls, fill, loop)."""
import ctypes

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll._lib import _TsMuxParams, _TsMuxPos, _TsMuxResult, _PsiParams
from dvbt2ll.tsmux import psi_params
import tsmux_cases as C
import tsmux_ref as R


def _params(period=7, weight=(3, 2), loop=None, fill_input=-1, pcr_pid=-1, pcr_weight=0, tpp=0, max_out=1 << 16, n=None):
    p = _TsMuxParams()
    p.n_inputs, p.period, p.fill_input = len(weight) if n is None else n, period, fill_input
    for i, w in enumerate(weight):
        p.weight[i] = w
        p.loop[i] = (loop or [0] * len(weight))[i]
    p.pcr_pid, p.pcr_weight, p.ticks_per_period, p.max_out_packets = pcr_pid, pcr_weight, tpp, max_out
    return p


def _schedule(p):
    owner = np.full(p.period + 8, 0xEE, np.uint8)
    st = dvbt2ll.lib().dvbt2ll_tsmux_schedule(ctypes.byref(p), owner.ctypes.data_as(ctypes.c_void_p))
    assert (owner[p.period:] == 0xEE).all()
    return st, owner[:p.period]


@pytest.mark.parametrize("name,period,weight,pcr_weight", C.SCHEDULES, ids=[s[0] for s in C.SCHEDULES])
def test_schedule_is_the_sorted_due_times(name, period, weight, pcr_weight):
    fill = weight.index(0) if 0 in weight else -1
    p = _params(period, weight, fill_input=fill, pcr_pid=0x1FF if pcr_weight else -1, pcr_weight=pcr_weight,
                tpp=1000 if pcr_weight else 0)
    st, got = _schedule(p)
    assert st == 0
    np.testing.assert_array_equal(got, R.schedule(period, weight, pcr_weight))
    w = list(weight) + [pcr_weight]
    w.append(period - sum(w))
    assert [int((got == e).sum()) for e in range(len(w))] == w      # every owner has its weight


def test_schedule_known_answers():
    """P = 7, weights 3 and 2, one PCR slot, one null slot: due times 0 (all four owners, in owner order), 1/3, 1/2,
    2/3"""
    assert list(R.schedule(7, (3, 2), 1)) == [0, 1, 2, 3, 0, 1, 0]
    assert list(_schedule(_params(7, (3, 2), pcr_pid=0x20, pcr_weight=1, tpp=7))[1]) == [0, 1, 2, 3, 0, 1, 0]
    assert list(R.schedule(1, (1,))) == [0]
    assert list(R.schedule(4, (2, 2))) == [0, 1, 0, 1]                # equal due times go to the lower owner first
    assert list(R.schedule(6, (1,))) == [0, 2, 2, 2, 2, 2]            # owner 2: null


def test_schedule_and_create_refuse_bad_parameters():
    L = dvbt2ll.lib()
    bad = [_params(n=0), _params(n=9), _params(period=0), _params(period=65537), _params(weight=(3, 5)),   # above P
           _params(weight=(3, 0)), _params(weight=(3, -1)), _params(weight=(3, 0), fill_input=0),          # 0 not on the fill
           _params(fill_input=2), _params(fill_input=-2), _params(loop=(0, 2)),
           _params(loop=(1, 0), fill_input=0),                                                             # a looping fill input
           _params(pcr_pid=0x1FFF, pcr_weight=1, tpp=5), _params(pcr_pid=-2), _params(pcr_pid=5, pcr_weight=0, tpp=5),
           _params(pcr_pid=5, pcr_weight=3, tpp=5), _params(pcr_pid=5, pcr_weight=1, tpp=0),
           _params(pcr_pid=5, pcr_weight=1, tpp=1 << 36), _params(pcr_pid=-1, pcr_weight=1),
           _params(pcr_pid=-1, tpp=5), _params(max_out=0), _params(max_out=(1 << 24) + 1)]
    h = ctypes.c_void_p()
    for k, p in enumerate(bad):
        assert _schedule(p)[0] == -1, k
        assert L.dvbt2ll_tsmux_create(ctypes.byref(p), 0, ctypes.byref(h)) == -1 and not h.value, k
    ok = [_params(weight=(3, 0), fill_input=1), _params(pcr_pid=0x1FFE, pcr_weight=2, tpp=(1 << 36) - 1),
          _params(period=65536, weight=(65536,)), _params(period=1, weight=(1,), max_out=1 << 24)]
    for p in ok:
        assert _schedule(p)[0] == 0
    assert L.dvbt2ll_tsmux_schedule(None, (ctypes.c_uint8 * 8)()) == -1
    assert L.dvbt2ll_tsmux_schedule(ctypes.byref(_params()), None) == -1
    assert L.dvbt2ll_tsmux_create(None, 0, ctypes.byref(h)) == -1
    assert L.dvbt2ll_tsmux_create(ctypes.byref(_params()), 0, None) == -1
    pos, res = _TsMuxPos(), _TsMuxResult()
    assert L.dvbt2ll_tsmux_run_device(None, None, None, ctypes.byref(pos), None, 1, None) == -1
    assert L.dvbt2ll_tsmux_run_host(None, None, None, ctypes.byref(pos), None, 1, ctypes.byref(res)) == -1
    assert L.dvbt2ll_tsmux_get_result(None, ctypes.byref(res)) == -1
    L.dvbt2ll_tsmux_destroy(None)
    for n in ("schedule", "ticks_per_period", "create", "run_device", "get_result", "run_host", "destroy"):
        assert "dvbt2ll_tsmux_" + n in dvbt2ll.EXPORTS
    assert "dvbt2ll_psi_build" in dvbt2ll.EXPORTS
    assert (ctypes.sizeof(_TsMuxParams), ctypes.sizeof(_TsMuxPos), ctypes.sizeof(_TsMuxResult)) == (104, 80, 240)
    assert ctypes.sizeof(_PsiParams) == 8 * (16 + 8 * 76) + 12
    assert L.dvbt2ll_abi_version() == 2


def test_create_is_edevice_without_a_gpu():
    L = dvbt2ll.lib()
    if L.dvbt2ll_device_count() > 0:
        pytest.skip("a GPU is visible")
    h = ctypes.c_void_p()
    assert L.dvbt2ll_tsmux_create(ctypes.byref(_params()), 0, ctypes.byref(h)) == -3 and not h.value
    with pytest.raises(dvbt2ll.DVBT2Error):
        dvbt2ll.TsMux(7, [3, 2])


def test_ticks_per_period_for_two_rates():
    """a period of 10 packets at 4 Mbit/s lasts 10 x 1504 / 4e6 s = 101520 ticks exactly; at 7.2 Mbit/s one of 7 lasts
    39480 ticks exactly; at 6 999 999 bit/s it is 40608.0058, rounded; x.5 rounds up"""
    f = dvbt2ll.ticks_per_period
    assert f(10, 4000000) == 101520
    assert f(7, 7200000) == 39480
    assert f(7, 6999999) == round(7 * 1504 * 27e6 / 6999999) == 40608
    assert f(1, 2 * 1504 * 27000000) == 1 and f(1, 2 * 1504 * 27000000 + 1) == 0    # 0.5 rounds up, below it down
    assert f(65536, 1000) == 65536 * 1504 * 27000
    L = dvbt2ll.lib()
    assert [L.dvbt2ll_tsmux_ticks_per_period(*a) for a in ((0, 5), (65537, 5), (4, 0), (4, -3))] == [-1] * 4


# ---------------------------------------------------------------------------------------- PSI
def _build(tsid, version, programs, cap=None):
    p = psi_params(tsid, version, programs)
    L = dvbt2ll.lib()
    n = L.dvbt2ll_psi_build(ctypes.byref(p), None, 0)
    if n < 0 or cap == "count":
        return n
    out = np.full((n if cap is None else cap) * 188 + 16, 0xEE, np.uint8)
    got = L.dvbt2ll_psi_build(ctypes.byref(p), out.ctypes.data_as(ctypes.c_void_p), n if cap is None else cap)
    if got < 0:
        assert (out == 0xEE).all()
        return got
    assert got == n and (out[n * 188:] == 0xEE).all()
    return out[:n * 188]


def test_pat_known_answer():
    """tsid 1, version 0, programme 1 on PMT PID 0x1000: the PAT section 00 B0 0D 00 01 C1 00 00 00 01 F0 00 2A B1 04
    B2, the one widely seen from ffmpeg's muxer"""
    want = bytes.fromhex("00B00D0001C100000001F0002AB104B2")
    assert R.pat_section(1, 0, C.PROGRAMS_ONE) == want and R.crc32(want) == 0
    ts = _build(1, 0, C.PROGRAMS_ONE).reshape(-1, 188)
    assert len(ts) == 32                                  # 16 rounds of PAT + PMT
    for r in range(16):
        p = ts[2 * r]
        assert list(p[:5]) == [0x47, 0x40, 0x00, 0x10 | r, 0x00] and p[5:21].tobytes() == want and (p[21:] == 0xFF).all()
        q = ts[2 * r + 1]
        assert list(q[:5]) == [0x47, 0x50, 0x00, 0x10 | r, 0x00]
    pmt = bytes.fromhex("02B0120001C10000FFFFF0000DE101F000")
    assert ts[1][5:5 + len(pmt)].tobytes() == pmt
    assert ts[1][5 + len(pmt):9 + len(pmt)].tobytes() == R.crc32(pmt).to_bytes(4, "big") and (ts[1][9 + len(pmt):] == 0xFF).all()


def test_psi_equals_the_reference_and_loops_seamlessly():
    for tsid, version, programs in ((1, 0, C.PROGRAMS_ONE), (0xBEEF, 31, C.programs_big())):
        ts = _build(tsid, version, programs)
        np.testing.assert_array_equal(ts, R.psi(tsid, version, programs))
        # two laps in a row: every PID's counter runs on from the loop's last packet into its first
        two = R.check_ts(np.concatenate([ts, ts]), cc={0: 0})
        one = R.check_ts(ts)
        assert all(v == 0 for v in one["cc"].values())    # a multiple of 16 packets on every PID
        assert two["pat"] == dict(tsid=tsid, version=version,
                                  programs=[(g["program_number"], g["pmt_pid"]) for g in programs])
        for g in programs:
            m = two["pmts"][g["program_number"]]
            assert m["pcr_pid"] == g.get("pcr_pid", 0x1FFF) and m["version"] == version
            assert m["streams"] == [(e["stream_type"], e["pid"], bytes(e.get("descriptors", b""))) for e in g["streams"]]
    big = R.pmt_section(31, C.programs_big()[1])
    assert len(big) == 12 + 8 * 69 + 4 and one["pids"][0x1FFE] == 16 * 4      # the large PMT spans four packets
    assert one["pids"][0] == 16 and one["pids"][0x1F0] == 16


def test_checker_refuses_a_broken_carousel():
    ts = _build(1, 0, C.programs_big())
    for at, what in ((188 * 2 + 40, "CRC"), (188 * 3 + 3, "continuity")):
        bad = ts.copy()
        bad[at] ^= 0x01
        with pytest.raises(AssertionError):
            R.check_ts(bad, cc={0: 0})


def test_psi_build_refuses_bad_parameters():
    def prog(**kw):
        g = dict(program_number=1, pmt_pid=0x100, streams=[dict(stream_type=6, pid=0x101)])
        g.update(kw)
        return g
    bad = [(-1, 0, [prog()]), (65536, 0, [prog()]), (1, 32, [prog()]), (1, -1, [prog()]), (1, 0, []),
           (1, 0, [prog(program_number=0)]), (1, 0, [prog(program_number=65536)]), (1, 0, [prog(pmt_pid=0x0F)]),
           (1, 0, [prog(pmt_pid=0x1FFF)]), (1, 0, [prog(pcr_pid=0x2000)]), (1, 0, [prog(pcr_pid=-1)]),
           (1, 0, [prog(), prog(program_number=2)]),                                 # the PMT PID repeats
           (1, 0, [prog(streams=[dict(stream_type=256, pid=1)])]), (1, 0, [prog(streams=[dict(stream_type=6, pid=0x2000)])])]
    for k, a in enumerate(bad):
        assert _build(*a) == -1, k
    p = psi_params(1, 0, [prog()])
    p.programs[0].n_streams = 9
    assert dvbt2ll.lib().dvbt2ll_psi_build(ctypes.byref(p), None, 0) == -1
    p.programs[0].n_streams = 1
    p.programs[0].streams[0].descriptor_len = 65
    assert dvbt2ll.lib().dvbt2ll_psi_build(ctypes.byref(p), None, 0) == -1
    p = psi_params(1, 0, [prog()])
    p.n_programs = 9
    assert dvbt2ll.lib().dvbt2ll_psi_build(ctypes.byref(p), None, 0) == -1
    assert dvbt2ll.lib().dvbt2ll_psi_build(None, None, 0) == -1
    assert _build(1, 0, [prog()], cap="count") == 32
    assert _build(1, 0, [prog()], cap=31) == -1                                      # too small a capacity
    assert _build(1, 0, [prog(pmt_pid=0x10 + k, program_number=1 + k) for k in range(8)], cap="count") == 16 * 9
    with pytest.raises(dvbt2ll.DVBT2Error):
        dvbt2ll.psi_build(1, 0, [prog(pmt_pid=5)])
    np.testing.assert_array_equal(dvbt2ll.psi_build(1, 0, [prog()]), R.psi(1, 0, [prog()]))


# ---------------------------------------------------------------------------------------- the reference multiplexer
def test_reference_mux_hand_derived():
    """P = 7, table 0 1 P N 0 1 0 from phase 5: slots 5, 6, then whole periods.  Input 1 has one packet, so its second
    slot is dry; without a fill input it carries a null packet"""
    a, b = C.stream(5, 0x101), C.stream(1, 0x102)
    r = R.mux([a, b], 9, 7, (3, 2), pcr_pid=0x1FF, pcr_weight=1, ticks_per_period=700, start=(5, 1000, (0,) * 8))
    ts, A, B = r.ts.reshape(-1, 188), a.reshape(-1, 188), b.reshape(-1, 188)
    want = [B[0], A[0], A[1], R.NULL, R.pcr_packet(0x1FF, 1700 + 200), R.NULL, A[2], R.NULL, A[3]]
    for k, w in enumerate(want):
        np.testing.assert_array_equal(ts[k], w, err_msg=str(k))
    assert r.resume == (0, 1000 + 2 * 700, (4, 1, 0, 0, 0, 0, 0, 0))
    assert r.counters == dict(fill_in_free=0, pcr_packets=1, null_packets=3, sync_errors=0, consumed=(4, 1),
                              dry_slots=(0, 2))
    assert list(R.pcr_packet(0x1FF, 1900)[:12]) == [0x47, 0x01, 0xFF, 0x20, 0xB7, 0x10, 0, 0, 0, 0x03, 0x7E, 100]
    # with input 0 as the fill input it also takes the null slot and input 1's dry slots
    f = R.mux([a, b], 9, 7, (3, 2), fill_input=0, pcr_pid=0x1FF, pcr_weight=1, ticks_per_period=700,
              start=(5, 1000, (0,) * 8))
    got = [int.from_bytes(p[4:8].tobytes(), "big") if p[2] == 1 else -1 for p in f.ts.reshape(-1, 188)]
    assert got == [-1, 0, 1, 2, -1, 3, 4, -1, -1] and f.counters["fill_in_free"] == 2
    assert f.counters["dry_slots"] == (1, 2) and f.counters["null_packets"] == 2


def test_reference_mux_chains_at_every_split():
    ins = [C.stream(20, 0x101), C.stream(9, 0x102), C.stream(16, 0x103)]    # 16 packets loop seamlessly
    kw = dict(period=10, weight=(0, 3, 2), loop=(0, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=2,
              ticks_per_period=1003)
    start = (7, R.W - 2500, (0, 0, 2, 0, 0, 0, 0, 0))
    whole = R.mux(ins, 60, start=start, **kw)
    for k in range(61):
        a = R.mux(ins, k, start=start, **kw)
        b = R.mux(ins, 60 - k, start=a.resume, **kw)
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert b.resume == whole.resume
        for n in R.COUNTERS:
            assert a.counters[n] + b.counters[n] == whole.counters[n]
        for n in ("consumed", "dry_slots"):
            assert tuple(x + y for x, y in zip(a.counters[n], b.counters[n])) == whole.counters[n]
    chk = R.check_ts(whole.ts)
    assert len(chk["pcrs"]) == whole.counters["pcr_packets"] == 12 and whole.counters["consumed"][0] == 20
