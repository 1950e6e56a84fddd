"""PDU lists for the MPE-FEC tests (tests/test_cpu_mpefec.py, tests/test_gpu_mpefec.py): every case is a list of byte
strings."""
import numpy as np

from mpe_cases import PID, OVER, V4_GROUP, V6_GROUP, ip, mixed  # noqa: F401

SHAPES = ((1, 1), (3, 2), (191, 64))        # (D, K) pairs: every D and every K of DS and KS once
DS, KS = (1, 3, 191), (1, 2, 64)            # the CPU tests take their product


def exact(total, seed, lo=20, hi=300):
    """datagrams of lo .. hi bytes (the last one whatever is left, at least 1) that sum to total exactly; every fifth
    goes to a multicast group"""
    r = np.random.default_rng(seed)
    out, left = [], total
    while left > 0:
        L = min(left, int(r.integers(lo, hi + 1)))
        if 0 < left - L < 1:
            L = left
        k = len(out)
        first = 0x60 if k % 7 == 3 else 0x45
        out.append(ip(L, seed * 1000 + k, first, (V6_GROUP if first == 0x60 else V4_GROUP) if k % 5 == 1 else None))
        left -= L
    return out


def frame_cases(rows, D):
    """U = C, U = C - 1 with a datagram that misses by one byte, one datagram, a datagram that straddles a column"""
    C = D * rows
    hi = min(300, C)
    c = {"full": exact(C, rows + D, 20, hi) + [ip(10, 1)],
         "minus1": exact(C - 1, rows + D + 1, 20, hi) + [ip(2, 2)],          # 2 bytes do not fit: one byte too many
         "one": [ip(min(C, 300), 3)]}
    if D > 1:
        c["straddle"] = [ip(rows - 10, 4), ip(20, 5), ip(rows - 5, 6, 0x60)] + [ip(40, 7)]
    return c


def ip4(length, seed):
    """a datagram whose IPv4 total-length field states its length (the lossy receiver reads repaired datagrams by it)"""
    b = bytearray(ip(length, seed))
    b[2:4] = length.to_bytes(2, "big")
    return bytes(b)


def small_frames(n, seed, lo=60, hi=250):
    """n datagrams of lo .. hi bytes: with rows 256 and D in 1 .. 3 a few of them fill a frame"""
    return mixed(n, seed, lo, hi)
