"""Cases that take the TS multiplexer and its remux to their widths (tests/test_cpu_tsmux_limits.py proves on the CPU
what they claim, tests/test_gpu_tsmux_limits.py runs them on the device): eight live inputs, 64 map entries beside 64
tracked PIDs with start counters that differ from nibble to nibble and from word to word, calls past the emit and the
classify kernel's grids, and a seeded sweep of generated parameter sets.  A case is a dict as tsremux_cases._case
makes it; a plain case has remux None.  MAX_BLOCKS is TSMUX_MAX_BLOCKS of csrc/tsmux_kernels.h, TILE and SCAN_TILES are
tsremux_cases' (the CPU test reads all three from the header)."""
import numpy as np

import tsmux_cases as C
import tsmux_ref as R
import tsremux_cases as XC
import tsremux_ref as X

TILE, SCAN_TILES, W = XC.TILE, XC.SCAN_TILES, XC.W
MAX_BLOCKS = 2048     # the grids' cap: the emit kernel takes a tile per workgroup trip, the classify kernel four
SWEEP_SEED = 2        # the first seed at which the reference meets test_cpu_tsmux_limits.py's coverage conditions
SWEEP_CASES = 48

_REF = {}


def reference(case):
    """(tsmux_ref.Result, tsremux_ref.RemuxResult or None), computed once per case name and shared by every test of the
    process; nobody writes to it"""
    if case["name"] not in _REF:
        if case["remux"] is None:
            _REF[case["name"]] = (R.mux(case["inputs"], case["n_out"], start=case["start"], **case["mux"]), None)
        else:
            _REF[case["name"]] = X.remux(case["inputs"], case["n_out"], start=case["start"], rstart=case["rstart"],
                                         **case["remux"], **case["mux"])
    return _REF[case["name"]]


# ---------------------------------------------------------------------------------------- eight inputs
N8 = (90, 40, 37, 0, 30, 3, 25, 11)
START8 = (11, W - 40000, (3, 0, 2, 0, 1, 2, 0, 4))


def mux8():
    """P = 23: 20 slots of inputs 1 .. 7, two of the PCR generator, one null; input 0 is the weightless fill input"""
    return XC._mux(23, (0, 5, 4, 3, 3, 2, 2, 1), loop=(0, 0, 0, 0, 0, 1, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=2,
                   ticks_per_period=23017)


def plain8():
    """every input on a PID of its own; input 3 is empty and goes in as a null pointer"""
    ins = [C.stream(n, 0x101 + i, seed=i) for i, n in enumerate(N8)]
    return XC._case("plain8", ins, 300, mux8(), None, start=START8)


def cc8(s):
    """the start counter of slot s: the 16 slots of a word hold all 16 values, and the four words differ (5 s + 3 alone
    repeats from word to word, so exchanging two words would not show)"""
    return (5 * s + 3 + 3 * (s >> 4)) & 15


def remux8():
    """plain8's multiplexer with every table full: input k carries PIDs 0x100 + 8 k + j with random counters, input 7 a
    PCR stream on 0x138; 64 map entries, (k, 0x100 + 8 k + j) -> 0x400 + 8 k + j and j = 7 dropped; all 64 targets
    tracked, every input restamped; input 7's PCRs restamped from in_phase 1"""
    ins = [XC.mixed(n, tuple(0x100 + 8 * k + j for j in range(8)), seed=20 + k) for k, n in enumerate(N8[:7])]
    ins.append(XC.pcr_stream(11, 0x138, 3, 1000, 77, phase=1, ticks=W - 500, every=2))
    entries = [(k, 0x100 + 8 * k + j, 0x1FFF if j == 7 else 0x400 + 8 * k + j) for k in range(8) for j in range(8)]
    track = tuple(0x400 + 8 * k + j for k in range(8) for j in range(8))
    rx = XC._remux(map=entries, track_pid=track, restamp_cc=(1,) * 8, in_period=(0,) * 7 + (3,),
                   in_ticks_per_period=(0,) * 7 + (1000,))
    return XC._case("remux8", ins, 300, mux8(), rx, start=START8,
                    rstart=([cc8(s) for s in range(64)], (0,) * 7 + (1,), (0,) * 7 + (W - 500,)), cont=track)


# ---------------------------------------------------------------------------------------- past the grids
def long_emit():
    """MAX_BLOCKS x TILE + TILE + 7 slots: 2050 tiles, so the emit kernel's workgroups 0 and 1 take a second trip, the
    last of them a tile of 7, and the second scan round runs over nine chunks.  Eight loop inputs of 3 .. 48 packets on
    two PIDs each, all 16 PIDs tracked from distinct counters; a packet without payload; input 6's second PID merged
    onto its first; input 2's PCRs restamped (in_period 7) against out_ticks_per_period, both clocks a few thousand
    ticks before W"""
    n_out = MAX_BLOCKS * TILE + TILE + 7
    ins = [XC.mixed(n, (0x200 + 2 * k, 0x201 + 2 * k), seed=20 + k) for k, n in enumerate((3, 5, 7, 11, 16, 23, 37, 48))]
    XC.no_payload(ins[4], [9])
    ins[2].reshape(-1, 188)[5, 3:6] = (0x30 | 4, 7, 0x10)
    rx = XC._remux(map=[(6, 0x20D, 0x20C)], track_pid=tuple(range(0x200, 0x210)), restamp_cc=(1,) * 8,
                   in_period=(0, 0, 7), in_ticks_per_period=(0, 0, 70001), out_ticks_per_period=30011)
    return XC._case("long_emit", ins, n_out, XC._mux(11, (2, 1, 1, 2, 1, 1, 1, 1), loop=(1,) * 8), rx,
                    start=(9, W - 3000, (2, 0, 6, 10, 0, 22, 5, 48)),
                    rstart=([(7 * s + 2) & 15 for s in range(16)], (0, 0, 4), (0, 0, W - 4000)),
                    cont=tuple(range(0x200, 0x20D)) + (0x20E, 0x20F))


def long_classify():
    """4 x MAX_BLOCKS x TILE + TILE + 7 slots: 8194 tiles, so the classify kernel's workgroups 0 and 1 take a second
    trip, the last wave of it a tile of 7, and the second scan round runs over 33 chunks.  The two loop inputs, the
    remux and the positions of tsremux_cases.second_round_case"""
    case = XC.second_round_case()
    case.update(name="long_classify", n_out=4 * MAX_BLOCKS * TILE + TILE + 7)
    return case


# ---------------------------------------------------------------------------------------- the sweep
def _split_weights(rng, parts, total):
    """parts positive integers that sum to at most total, each at least 1"""
    w = [1] * parts
    if parts:
        for k in rng.integers(0, parts, int(rng.integers(0, total - parts + 1))):
            w[k] += 1
    return w


def sweep_case(seed, k):
    """generated case k: only parameter sets include/dvbt2ll_hip.h documents as valid"""
    rng = np.random.default_rng([seed, k])
    n = int(rng.integers(1, 9))
    with_remux = bool(rng.integers(0, 2))
    f = int(rng.integers(0, n)) if rng.random() < 0.6 else -1
    f_weightless = f >= 0 and rng.random() < 0.5
    with_pcr = rng.random() < 0.5
    weighted = [i for i in range(n) if not (i == f and f_weightless)]
    need = len(weighted) + with_pcr
    P = int(rng.integers(max(need, 1), 41))
    parts = _split_weights(rng, need, P)
    weight = [0] * n
    for i, w in zip(weighted, parts):
        weight[i] = w
    pcr_pid = 0x1E00 + int(rng.integers(0, 256)) if with_pcr else -1
    tpp = ((1 << 36) - 1 if rng.random() < 0.1 else int(rng.integers(1, 300000))) if with_pcr else 0
    loop = [int(i != f and rng.random() < 0.35) for i in range(n)]
    mux = XC._mux(P, weight, loop=loop, fill_input=f, pcr_pid=pcr_pid, pcr_weight=parts[-1] if with_pcr else 0,
                  ticks_per_period=tpp)
    n_out = 0 if rng.random() < 1 / 12 else int(rng.integers(1, 401))
    all_empty = rng.random() < 1 / 16
    n_in = []
    for i in range(n):
        share = n_out * weight[i] // P
        how = rng.random()
        n_in.append(0 if all_empty or how < 0.15 else int(rng.integers(0, min(share, 60) + 1)) if how < 0.45 else
                    int(rng.integers(0, 61)))
    # the inputs: plain streams, or for a remux 1 .. 3 PIDs with random counters (now and then input 0's first PID as
    # well) and packets without payload, or a PCR stream with a clock of its own
    in_period, in_tpp, in_phase, in_ticks, pids, ins = [0] * n, [0] * n, [0] * n, [0] * n, [], []
    for i in range(n):
        if not with_remux:
            pids.append((0x101 + i,))
            ins.append(C.stream(n_in[i], 0x101 + i, seed=k))
        elif rng.random() < 0.35:
            in_period[i] = 65536 if rng.random() < 0.1 else int(rng.integers(1, 13))
            in_tpp[i] = (1 << 36) - 1 if rng.random() < 0.1 else int(rng.integers(1, 200000))
            in_phase[i] = int(rng.integers(0, in_period[i]))
            in_ticks[i] = W - int(rng.integers(1, 5000)) if rng.random() < 0.5 else int(rng.integers(0, W))
            pids.append((0x100 + 16 * i,))
            ins.append(XC.pcr_stream(n_in[i], 0x100 + 16 * i, in_period[i], in_tpp[i], int(rng.integers(0, W)),
                                     phase=in_phase[i], ticks=in_ticks[i], every=int(rng.integers(1, 5)), seed=k))
        else:
            own = [0x100 + 16 * i + j for j in range(int(rng.integers(1, 4)))]
            if i and rng.random() < 0.2:
                own.append(pids[0][0])
            pids.append(tuple(own))
            ts = XC.mixed(n_in[i], pids[i], seed=100 * k + i)
            ins.append(XC.no_payload(ts, rng.integers(0, n_in[i], 2) if n_in[i] else []))
    nxt = [int(rng.integers(0, m + 1)) for m in n_in]
    if rng.random() < 0.25 and any(n_in):
        i = int(rng.choice([i for i in range(n) if n_in[i]]))
        ins[i][188 * ((nxt[i] + int(rng.integers(0, 4))) % n_in[i])] = 0x48
    clock = W - int(rng.integers(1, 200000)) if rng.random() < 0.5 else int(rng.integers(0, W))
    start = (int(rng.integers(0, P)), clock, tuple(nxt) + (0,) * (8 - n))
    rx, rstart = None, None
    if with_remux:
        pairs = [(i, p) for i in range(n) for p in pids[i]] + [(int(rng.integers(0, n)), 0x7F0 + j) for j in range(3)]
        entries, targets = [], []
        for a in rng.permutation(len(pairs))[:int(rng.integers(0, 13))]:
            how = rng.random()
            to = (0x1FFF if how < 0.2 else 0x300 + len(entries) if how < 0.6 or not (targets or entries) else
                  int(rng.choice(targets + [p for _, p in pairs[:-3]])))     # a merge: onto a target or an input's PID
            entries.append(pairs[a] + (to,))
            if to != 0x1FFF:
                targets.append(to)
        leaving = sorted(set(targets) | {p for _, p in pairs[:-3]}) + [0x600, 0x601, 0x1FFE, 0]
        track = [int(leaving[a]) for a in rng.permutation(len(leaving))[:int(rng.integers(0, 21))]]
        out_tpp = int(rng.choice([0, tpp])) if with_pcr else int(rng.integers(0, 300000))
        rx = XC._remux(map=entries, track_pid=track, restamp_cc=[int(v) for v in rng.integers(0, 2, n)],
                       in_period=in_period, in_ticks_per_period=in_tpp, out_ticks_per_period=out_tpp)
        rstart = ([int(v) for v in rng.integers(0, 16, len(track))], in_phase, in_ticks)
    case = XC._case("sweep %02d" % k, ins, n_out, mux, rx, start=start, rstart=rstart)
    case["split"] = int(rng.integers(0, n_out + 1))
    return case


def sweep(seed=SWEEP_SEED):
    return [sweep_case(seed, k) for k in range(SWEEP_CASES)]
