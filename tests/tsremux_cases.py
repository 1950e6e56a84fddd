"""Shapes for the remux tests (tests/test_cpu_tsremux.py, tests/test_gpu_tsremux.py): streams with several PIDs, packets
without payload, adaptation fields and exact PCRs, and the cases both tests run.  TILE and SCAN_TILES are
TSREMUX_TILE and TSREMUX_SCAN_TILES of csrc/tsmux_kernels.h (tests/test_cpu_tsremux.py reads them from the header)."""
import numpy as np

import tsmux_cases as C
import tsremux_ref as X

TILE = 64            # output packets per row of payload counts
SCAN_TILES = 256     # tiles per workgroup of the scan's first round: a call of more tiles needs the second round
W = X.W


def mixed(n, pids, seed=0):
    """n packets whose PIDs are drawn from pids, every counter random: a stream that needs restamping"""
    rng = np.random.default_rng(77 + seed)
    p = C.stream(n, 0x100, seed).reshape(-1, 188)
    pid = np.asarray(pids)[rng.integers(0, len(pids), n)]
    p[:, 1], p[:, 2], p[:, 3] = pid >> 8, pid & 255, 0x10 | rng.integers(0, 16, n)
    return p.reshape(-1)


def no_payload(ts, idx):
    """packet idx becomes adaptation field only (adaptation_field_control 2, 183 stuffing bytes), counter kept"""
    p = ts.reshape(-1, 188)
    for k in idx:
        p[k, 3] = 0x20 | (p[k, 3] & 15)
        p[k, 4], p[k, 5], p[k, 6:] = 183, 0x00, 0xFF
    return ts


def t_in(j, in_period, tpp, phase=0, ticks=0):
    dq, r = divmod(phase + j, in_period)
    return ticks + dq * tpp + r * tpp // in_period


def pcr_stream(n, pid, in_period, tpp, c, phase=0, ticks=0, every=3, seed=0):
    """n packets on pid; every `every`-th has an 8-byte adaptation field with PCR = c + T_in(j) exactly, for the input
    clock (in_period, tpp) from (phase, ticks); the packet after it has an adaptation field of length 0, the one after
    that one of 3 bytes with PCR_flag clear but the same bytes behind it"""
    ts = C.stream(n, pid, seed)
    p = ts.reshape(-1, 188)
    for j in range(0, n, every):
        p[j, 3], p[j, 4], p[j, 5] = 0x30 | (p[j, 3] & 15), 7, 0x10
        X.put_pcr(p[j], c + t_in(j, in_period, tpp, phase, ticks))
        if j + 1 < n:
            p[j + 1, 3], p[j + 1, 4] = 0x30 | (p[j + 1, 3] & 15), 0
        if j + 2 < n and every > 2:
            p[j + 2, 3], p[j + 2, 4], p[j + 2, 5] = 0x30 | (p[j + 2, 3] & 15), 3, 0x00
    return ts


def _case(name, inputs, n_out, mux, remux, start=(0, 0, (0,) * 8), rstart=None, cont=(), pcr=()):
    """cont: the PIDs the continuity checker must pass on; pcr: the PIDs whose PCR offset must be constant"""
    r = list(X.RSTART) if rstart is None else list(rstart)
    r = (tuple(r[0]) + (0,) * (64 - len(r[0])), tuple(r[1]) + (0,) * (8 - len(r[1])), tuple(r[2]) + (0,) * (8 - len(r[2])))
    return dict(name=name, inputs=inputs, n_out=n_out, mux=mux, remux=remux, start=start, rstart=r, cont=tuple(cont),
                pcr=tuple(pcr))


def _mux(period, weight, loop=None, fill_input=-1, pcr_pid=-1, pcr_weight=0, ticks_per_period=0):
    return dict(period=period, weight=tuple(weight), loop=tuple(loop or [0] * len(weight)), fill_input=fill_input,
                pcr_pid=pcr_pid, pcr_weight=pcr_weight, ticks_per_period=ticks_per_period)


def _remux(map=(), track_pid=(), restamp_cc=(), in_period=(), in_ticks_per_period=(), out_ticks_per_period=0):
    return dict(map=tuple(map), track_pid=tuple(track_pid), restamp_cc=tuple(restamp_cc), in_period=tuple(in_period),
                in_ticks_per_period=tuple(in_ticks_per_period), out_ticks_per_period=out_ticks_per_period)


PIDS64 = tuple(0x400 + 3 * k for k in range(64))


def remap_case():
    """inputs 0 and 1 on one PID mapped apart; input 2's two PIDs mapped onto one, which is tracked; input 0's PID 1AA
    dropped; an entry for a PID that never occurs; a bad-sync packet on a mapped PID"""
    a = C.stream(30, 0x101)
    a.reshape(-1, 188)[4::7, 1:3] = (0x01, 0xAA)
    b = C.stream(30, 0x101, seed=1)
    b[188 * 3] = 0x48
    c = mixed(20, (0x110, 0x111), seed=2)
    return _case("remap", [a, b, c], 70, _mux(5, (2, 2, 1)),
                 _remux(map=[(1, 0x101, 0x201), (2, 0x110, 0x300), (2, 0x111, 0x300), (0, 0x1AA, 0x1FFF),
                             (0, 0x555, 0x556)], track_pid=[0x300], restamp_cc=[0, 0, 1]),
                 rstart=([9], [], []), cont=(0x300,))   # the PIDs of inputs 0 and 1 have gaps: a drop, a bad sync


def tiles_case(n_out, cc=15):
    """64 tracked PIDs interleaved in one input with random counters, every slot starting at cc; packets without
    payload at the call's first and last packet and at the first and last packet of a tile"""
    ts = no_payload(mixed(2 * TILE + 9, PIDS64), [k for k in (0, TILE - 1, TILE, n_out - 1) if k < 2 * TILE + 9])
    return _case("tiles %d" % n_out, [ts], n_out, _mux(1, (1,)), _remux(track_pid=PIDS64, restamp_cc=[1]),
                 rstart=([cc] * 64, [], []), cont=PIDS64)


def absent_case():
    """three tracked PIDs over three tiles and a bit; 0x123 occurs in the first and third tile only"""
    ts = mixed(3 * TILE + 5, (0x121, 0x122, 0x123), seed=3)
    p = ts.reshape(-1, 188)
    mid = p[TILE:2 * TILE]
    mid[mid[:, 2] == 0x23, 2] = 0x21
    return _case("absent from a tile", [ts], 3 * TILE + 5, _mux(1, (1,)),
                 _remux(track_pid=(0x121, 0x122, 0x123), restamp_cc=[1]), rstart=([3, 15, 7], [], []),
                 cont=(0x121, 0x122, 0x123))


def carousel_case():
    """a 3-packet carousel over more than 17 laps beside an input that shares its PID but is not restamped"""
    mux = _mux(5, (2, 2), loop=(0, 1), fill_input=0)
    car = mixed(3, (0x102,), seed=4)
    return _case("carousel", [mixed(80, (0x101, 0x102), seed=5), car], 140, mux,
                 _remux(map=[(0, 0x102, 0x103)], track_pid=(0x102, 0x103), restamp_cc=(0, 1)),
                 start=(1, 0, (0, 2) + (0,) * 6), rstart=([5, 6], [], []), cont=(0x102,))


def shared_case():
    """input 0 (restamp_cc 0) and input 1 (restamp_cc 1) both on the tracked PID: input 0's packets are left alone
    and not counted, so the PID's continuity is broken on purpose and only the reference is asked"""
    return _case("shared tracked PID", [C.stream(40, 0x102, cc=3), mixed(40, (0x102,), seed=6)], 75, _mux(2, (1, 1)),
                 _remux(track_pid=(0x102,), restamp_cc=(0, 1)), rstart=([12], [], []))


def second_round_case():
    """more tiles than one workgroup of the scan's first round covers, a tile and a packet more: loop inputs keep the
    buffers small; input 0's PCRs are restamped as well (they repeat every lap, so they are not exact)"""
    n_out = TILE * SCAN_TILES + TILE + 1
    a = no_payload(mixed(7, (0x131, 0x132, 0x133), seed=7), [2])
    a.reshape(-1, 188)[5, 3:6] = (0x30 | 4, 7, 0x10)
    return _case("second scan round", [a, mixed(3, (0x132,), seed=8)], n_out,
                 _mux(3, (2, 1), loop=(1, 1)),
                 _remux(track_pid=(0x131, 0x132, 0x133), restamp_cc=(1, 1), in_period=[7], in_ticks_per_period=[70001],
                        out_ticks_per_period=30011),
                 start=(2, W - 50000, (3, 1) + (0,) * 6), rstart=([15, 0, 9], [6], [W - 9]),
                 cont=(0x131, 0x132, 0x133))


def pcr_case(own_pcr_pid=True, c=123456789, ticks=777, out_ticks=12345):
    """input 0 with exact PCRs (in_period 11, a clock that does not divide) through the weighted schedule from phase
    5, on a handle with a PCR PID of its own or with out_ticks_per_period; input 1 has in_period 1"""
    mux = _mux(7, (3, 2), pcr_pid=0x1FF, pcr_weight=1, ticks_per_period=7001) if own_pcr_pid else _mux(7, (3, 2))
    a = pcr_stream(40, 0x101, 11, 12345, c, phase=4, ticks=ticks)
    b = pcr_stream(30, 0x102, 1, 4003, 5, ticks=W - 6 * 4003, every=2, seed=1)
    return _case("pcr, %s" % ("own PCR PID" if own_pcr_pid else "out_ticks_per_period"), [a, b], 85, mux,
                 _remux(in_period=(11, 1), in_ticks_per_period=(12345, 4003),
                        out_ticks_per_period=0 if own_pcr_pid else 7001),
                 start=(5, out_ticks, (0,) * 8), rstart=([], [4, 0], [ticks, W - 6 * 4003]), pcr=(0x101, 0x102))


def pcr_wrap_case():
    """the input's clock, the PCR values and the mux clock all pass W inside the call; in_period 65536"""
    tpp = (1 << 36) - 1
    a = pcr_stream(50, 0x101, 65536, tpp, W - 3000, phase=65530, ticks=W - 5, every=1)
    return _case("pcr across the wrap", [a], 50, _mux(1, (1,), pcr_pid=-1),
                 _remux(in_period=[65536], in_ticks_per_period=[tpp], out_ticks_per_period=100), start=(0, W - 2500, (0,) * 8),
                 rstart=([], [65530], [W - 5]), pcr=(0x101,))


def pcr_fill_case():
    """the fill input (weight 0) restamped: its rank is the claim rank; input 1 runs dry and a carousel with PCRs
    loops several laps (its PCRs repeat, so only the fill input's offset is constant)"""
    mux = _mux(10, (0, 3, 2), loop=(0, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=2, ticks_per_period=1003)
    a = pcr_stream(60, 0x101, 5, 997, 42, phase=2, ticks=W - 4000, every=4)
    car = pcr_stream(3, 0x103, 3, 100, 0, every=1)
    return _case("pcr, fill and loop", [a, C.stream(9, 0x102), car], 120, mux,
                 _remux(in_period=(5, 0, 3), in_ticks_per_period=(997, 0, 100)), start=(7, W - 2500, (0, 0, 2) + (0,) * 5),
                 rstart=([], [2, 0, 1], [W - 4000, 0, 50]), pcr=(0x101,))


def all_case():
    """the 200-slot call of the chaining tests: remap, continuity and PCR restamping at once, a fill input, a dry
    input with a bad-sync packet, a carousel, PCR packets of the handle's own"""
    mux = _mux(10, (0, 3, 2), loop=(0, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=2, ticks_per_period=1003)
    a = pcr_stream(70, 0x101, 5, 997, 42, phase=2, ticks=W - 4000, every=4)
    b = no_payload(mixed(40, (0x101, 0x120), seed=9), [0, 11, 39])
    b[188 * 7] = 0x46
    car = mixed(3, (0x103,), seed=10)
    return _case("all three", [a, b, car], 200, mux,
                 _remux(map=[(1, 0x101, 0x102), (1, 0x120, 0x1FFF)], track_pid=(0x102, 0x103, 0x101),
                        restamp_cc=(1, 1, 1), in_period=(5,), in_ticks_per_period=(997,)),
                 start=(7, W - 2500, (0, 0, 2) + (0,) * 5), rstart=([15, 3, 8], [2], [W - 4000]),
                 cont=(0x101, 0x102, 0x103), pcr=(0x101,))


def cases():
    return [remap_case(), tiles_case(TILE), tiles_case(TILE + 1), tiles_case(2 * TILE + 9, cc=0), absent_case(),
            carousel_case(), shared_case(), second_round_case(), pcr_case(True), pcr_case(False), pcr_wrap_case(),
            pcr_fill_case(), all_case()]
