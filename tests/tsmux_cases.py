"""Shapes for the TS multiplexer tests (tests/test_cpu_tsmux.py, tests/test_gpu_tsmux.py): input streams whose packets
can be told apart, the schedule cases, the PSI cases."""
import numpy as np

PIDS = (0x101, 0x102, 0x103, 0x104)


def stream(n, pid, seed=0, cc=0):
    """n packets on pid with a running continuity counter; the payload's first 4 bytes are the packet's index, the
    rest is seeded noise, so that any packet taken from the wrong place shows"""
    rng = np.random.default_rng(1000 * pid + seed)
    p = rng.integers(0, 256, (n, 188), dtype=np.uint8)
    k = np.arange(n)
    p[:, 0], p[:, 1], p[:, 2], p[:, 3] = 0x47, pid >> 8, pid & 255, 0x10 | ((cc + k) & 15)
    for b in range(4):
        p[:, 4 + b] = (k >> (8 * (3 - b))) & 255
    return p.reshape(-1)


# (name, period, weights, pcr_weight)
SCHEDULES = (
    ("one slot", 1, (1,), 0),
    ("seven", 7, (3, 2), 1),
    ("ties", 12, (3, 3, 3), 3),
    ("ties, unequal", 12, (2, 4, 6), 0),
    ("booked", 10, (5, 3), 2),
    ("largest", 65536, (1, 65534), 0),
    ("largest, fill weight 0", 65536, (0, 4097), 1),
)

PROGRAMS_ONE = [dict(program_number=1, pmt_pid=0x1000, streams=[dict(stream_type=0x0D, pid=0x101)])]


def programs_big():
    """two programmes; the second's PMT has 8 streams of 64 descriptor bytes and spans four packets"""
    rng = np.random.default_rng(5)
    big = [dict(stream_type=0x80 + k, pid=0x200 + k, descriptors=rng.integers(0, 256, 64, dtype=np.uint8).tobytes())
           for k in range(8)]
    return [dict(program_number=7, pmt_pid=0x1F0, pcr_pid=0x1F1,
                 streams=[dict(stream_type=0x0D, pid=0x101, descriptors=bytes([0x13, 0x01, 0x05]))]),
            dict(program_number=65535, pmt_pid=0x1FFE, pcr_pid=0x1FFF, streams=big)]
