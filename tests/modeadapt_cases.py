"""Transport streams for the mode-adapter tests (tests/test_cpu_modeadapt.py, tests/test_gpu_modeadapt.py): seeded,
built once per argument set and handed out read-only."""
import functools

import numpy as np

from dvbt2ll.configs import ts_packets

PID_A, PID_B, PID_FOREIGN, PID_NULL = 0x100, 0x101, 0x200, 0x1FFF
KBCH_SHORT14 = 3072       # short 1/4: L = 384, D = 374, fewer than two units per BBFRAME
KBCH_ODD = 48408          # normal 3/4: L = 6051, the odd-L 64800 code
RUNS = (0, 1, 254, 255, 256, 257, 511, 512, 600)


def _ro(a):
    a.setflags(write=False)
    return a


def stream(pattern, seed=7):
    """pattern: a sequence of (PID, packets): the synthetic TS's packets with their PIDs set in turn"""
    n = sum(c for _, c in pattern)
    rows = ts_packets(0, n, seed).reshape(n, 188).copy()
    pids = np.concatenate([np.full(c, p) for p, c in pattern]).astype(np.int64)
    rows[:, 1] = (rows[:, 1] & 0xE0) | (pids >> 8)
    rows[:, 2] = pids & 255
    return rows.reshape(-1)


@functools.lru_cache(maxsize=None)
def run_stream(run, place, body=24):
    """a null run of the given length at the buffer's start (0), middle (1) or end (2) of `body` selected packets"""
    pat = {0: [(PID_NULL, run), (PID_A, body)], 1: [(PID_A, body // 2), (PID_NULL, run), (PID_A, body - body // 2)],
           2: [(PID_A, body), (PID_NULL, run)]}[place]
    return _ro(stream(pat, seed=run + place))


@functools.lru_cache(maxsize=None)
def two_tile_stream():
    """2200 packets, three scan tiles of 1024: a run of 600 nulls across the first tile boundary (its kept nulls on
    either side), a kept null exactly at packet 1024 + 1023 (a run from 1792), bad sync bytes"""
    pat = [(PID_A, 700), (PID_NULL, 600), (PID_A, 492), (PID_NULL, 300), (PID_A, 108)]
    assert pat[0][1] + 255 < 1024 < pat[0][1] + 511 and 1792 + 255 == 2047
    ts = stream(pat, seed=3)
    ts[188 * 5] = 0x46
    ts[188 * 1023] = 0x00
    ts[188 * 1500] = 0xFF
    return _ro(ts)


@functools.lru_cache(maxsize=None)
def two_pid_stream(groups=75):
    """PIDs A, A, A, A, B, foreign in turn, a few null packets between the groups"""
    pat = []
    for g in range(groups):
        pat += [(PID_A, 4), (PID_B, 1), (PID_FOREIGN, 1)] + ([(PID_NULL, g % 3)] if g % 3 else [])
    return _ro(stream(pat, seed=11))


@functools.lru_cache(maxsize=None)
def split_stream():
    """about 40 packets with short and long gaps"""
    return _ro(stream([(PID_A, 5), (PID_NULL, 3), (PID_A, 10), (PID_NULL, 12), (PID_A, 8), (PID_NULL, 2)], seed=5))


@functools.lru_cache(maxsize=None)
def long_run_stream():
    """a run of 700 nulls between selected packets: kept nulls at packets 3 + 255 and 3 + 511"""
    return _ro(stream([(PID_A, 3), (PID_NULL, 700), (PID_A, 6)], seed=9))
