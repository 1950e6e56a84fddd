"""The remux of the TS multiplexer (dvbt2ll_tsmux_*_remux; include/dvbt2ll_hip.h states the rules) restated sequentially
on top of tsmux_ref.mux, and a checker that knows none of those rules.

remux()             tsmux_ref.mux is run on stand-in packets that only say "packet k of input i", which gives the slot
                    walk's outcome; a second walk over the slots then carries a dict of continuity counters, a running
                    position and clock per input and the running mux clock, and applies, per packet, sync check ->
                    remap -> continuity restamp -> PCR restamp.  No ranks, no prefix counts, no tiles.
check_continuity()  per PID: a payload packet's counter is the previous one + 1, a packet without payload repeats it
check_pcr()         per PID with PCRs: PCR - slot time is one constant (mod W)
"""
from typing import NamedTuple

import numpy as np

import tsmux_ref as R

W = R.W
REMUX_COUNTERS = ("remapped", "dropped", "cc_rewritten", "pcr_restamped")
RSTART = ((0,) * 64, (0,) * 8, (0,) * 8)


class RemuxResult(NamedTuple):
    resume: tuple         # (cc: 64 entries, in_phase: 8, in_ticks: 8)
    counters: dict


def pcr_of(p):
    """the PCR of a packet in 27 MHz ticks, or None (the rule of tsmux_ref.check_ts)"""
    if p[3] & 0x20 and p[4] >= 7 and p[5] & 0x10:
        v = int.from_bytes(bytes(p[6:12]), "big")
        return (v >> 15) * 300 + (v & 0x1FF)
    return None


def put_pcr(p, ticks):
    base, ext = divmod(ticks % W, 300)
    p[6:12] = list(((base << 15) | (0x3F << 9) | ext).to_bytes(6, "big"))


def remux(inputs, n_out, map=(), track_pid=(), restamp_cc=(), in_period=(), in_ticks_per_period=(),
          out_ticks_per_period=0, start=(0, 0, (0,) * 8), rstart=RSTART, **kw):
    """returns (tsmux_ref.Result, RemuxResult)"""
    n = len(kw["weight"])
    ins = [np.asarray(x, np.uint8).reshape(-1, 188) for x in inputs]
    pad = lambda v: list(v) + [0] * (8 - len(v))
    restamp_cc, in_period, in_tpp = pad(restamp_cc), pad(in_period), pad(in_ticks_per_period)
    # the slot walk on stand-ins: 47, then 00 (a generated null packet has FF there, a PCR packet B7), input, index
    tags = []
    for i, x in enumerate(ins):
        t = np.zeros((len(x), 188), np.uint8)
        t[:, 0], t[:, 5] = 0x47, i
        for b in range(4):
            t[:, 6 + b] = (np.arange(len(x)) >> (8 * b)) & 255
        tags.append(t.reshape(-1))
    tpp = kw.get("ticks_per_period", 0) if kw.get("pcr_pid", -1) >= 0 else out_ticks_per_period
    walk = R.mux(tags, n_out, start=start, **dict(kw, ticks_per_period=tpp if kw.get("pcr_pid", -1) >= 0 else 0))
    c = dict(walk.counters)
    rc = dict.fromkeys(REMUX_COUNTERS, 0)
    mapping = {(i, f): t for i, f, t in map}
    slot_of = {pid: s for s, pid in enumerate(track_pid)}
    cc = [int(v) for v in rstart[0]]
    phase, ticks = [int(v) for v in rstart[1]], [int(v) for v in rstart[2]]
    slot, clock = int(start[0]), int(start[1])
    period = kw["period"]
    out = walk.ts.reshape(-1, 188).copy()
    for m in range(n_out):
        t_out = (clock + slot * tpp // period) % W
        slot += 1
        if slot == period:
            slot, clock = 0, (clock + tpp) % W
        if out[m][4] != 0:
            continue                                    # a generated null or PCR packet
        i = int(out[m][5])
        p = ins[i][int.from_bytes(bytes(out[m][6:10]), "little")].copy()
        t_in = None
        if in_tpp[i]:
            t_in = ticks[i] + phase[i] * in_tpp[i] // in_period[i]
            phase[i] += 1
            if phase[i] == in_period[i]:
                phase[i], ticks[i] = 0, (ticks[i] + in_tpp[i]) % W
        if p[0] != 0x47:
            out[m] = R.NULL
            c["sync_errors"] += 1
            c["null_packets"] += 1
            continue
        pid = ((int(p[1]) & 0x1F) << 8) | int(p[2])
        if (i, pid) in mapping:
            pid = mapping[(i, pid)]
            if pid == 0x1FFF:
                out[m] = R.NULL
                rc["dropped"] += 1
                c["null_packets"] += 1
                continue
            p[1], p[2] = (int(p[1]) & 0xE0) | (pid >> 8), pid & 255
            rc["remapped"] += 1
        if restamp_cc[i] and pid in slot_of:
            s = slot_of[pid]
            if p[3] & 0x10:
                new, cc[s] = cc[s], (cc[s] + 1) & 15
            else:
                new = (cc[s] - 1) & 15
            rc["cc_rewritten"] += new != (int(p[3]) & 15)
            p[3] = (int(p[3]) & 0xF0) | new
        if t_in is not None and pcr_of(p) is not None:
            put_pcr(p, pcr_of(p) + t_out - t_in)
            rc["pcr_restamped"] += 1
        out[m] = p
    res = R.Result(out.reshape(-1), (slot, clock, walk.resume[2]), c)
    return res, RemuxResult((tuple(cc), tuple(phase), tuple(ticks)), rc)


# ---------------------------------------------------------------------------------------- the checker
def check_continuity(ts, pids=None, first=None):
    """per PID (all but 1FFF, or those given): every payload packet's counter is the previous packet's + 1, every
    packet without payload has the previous one's.  first: {pid: the counter expected of its first payload packet}.
    Returns {pid: the counter the next payload packet must have}"""
    last = {pid: (v - 1) & 15 for pid, v in (first or {}).items()}
    for k, p in enumerate(np.asarray(ts, np.uint8).reshape(-1, 188)):
        pid = ((int(p[1]) & 0x1F) << 8) | int(p[2])
        if pid == 0x1FFF or (pids is not None and pid not in pids):
            continue
        v = int(p[3]) & 15
        if p[3] & 0x10:
            assert pid not in last or v == (last[pid] + 1) & 15, "continuity on PID %#x at packet %d" % (pid, k)
            last[pid] = v
        elif pid in last:
            assert v == last[pid], "a packet without payload moved the counter of PID %#x at packet %d" % (pid, k)
        else:
            last[pid] = v
    return {pid: (v + 1) & 15 for pid, v in last.items()}


def check_pcr(ts, period, ticks_per_period, start=(0, 0), pids=None):
    """per PID that carries PCRs: PCR - the time of the packet's slot is the same on every packet, mod W.  Returns
    {pid: that constant}"""
    const = {}
    for k, p in enumerate(np.asarray(ts, np.uint8).reshape(-1, 188)):
        pid = ((int(p[1]) & 0x1F) << 8) | int(p[2])
        v = pcr_of(p)
        if v is None or pid == 0x1FFF or (pids is not None and pid not in pids):
            continue
        dc, t = divmod(start[0] + k, period)
        d = (v - (start[1] + dc * ticks_per_period + t * ticks_per_period // period)) % W
        assert const.setdefault(pid, d) == d, "PCR offset on PID %#x at packet %d: %d, was %d" % (pid, k, d, const[pid])
    return const
