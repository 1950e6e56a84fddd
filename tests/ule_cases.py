"""PDU lists for the ULE tests (tests/test_cpu_ule.py, tests/test_gpu_ule.py): every case is a list of byte strings."""
import numpy as np

PID = 0x100


def ip(length, seed=0, first=0x45):
    """a PDU of length bytes whose first nibble says IPv4 (0x45), IPv6 (0x60) or neither"""
    r = np.random.default_rng(1000 + seed).integers(0, 256, length, dtype=np.uint8)
    r[0] = first
    return r.tobytes()


def over(d_bit):
    """SNDU bytes around a PDU: D / Length, Type, the destination address, the CRC"""
    return 8 if d_bit else 14


R_VALUES = (0, 1, 2, 181, 182, 183, 184, 185, 367, 368)
FREE_VALUES = (0, 1, 2)


def r_case(R, d_bit):
    """the first SNDU has 183 + R bytes: it fills packet 0 behind the Payload Pointer and packet 1 begins with R
    bytes of it left; two short ones follow (one IPv6)"""
    return [ip(183 + R - over(d_bit), R), ip(40, R + 1, 0x60), ip(25, R + 2)]


def free_case(f, d_bit):
    """the first SNDU ends with f bytes free in its PUSI packet"""
    return [ip(183 - f - over(d_bit), 50 + f), ip(30, 60 + f), ip(17, 70 + f, 0x60)]


def cases(d_bit):
    c = {"R%d" % R: r_case(R, d_bit) for R in R_VALUES}
    c.update({"free%d" % f: free_case(f, d_bit) for f in FREE_VALUES})
    c["min"] = [ip(1, 80), ip(1, 81, 0x60), ip(2, 82)]                 # with d_bit = 1: the 9-byte SNDU
    # Length 32767 -- with d_bit = 1 that Length field reads FF FF, the End Indicator, at a receiver: the round trip
    # there takes Length 32766, and max_sndu() is compared as bytes only
    c["max"] = [ip(7, 83), ip(32767 - d_bit - over(d_bit) + 4, 84), ip(9, 85)]
    return c


def max_sndu(d_bit):
    """the PDU whose SNDU has Length 32767"""
    return ip(32767 - over(d_bit) + 4, 84)


def mixed(n, seed, lo=1, hi=40):
    r = np.random.default_rng(seed)
    return [ip(int(L), seed * 100000 + k, 0x60 if k % 7 == 3 else 0x45) for k, L in enumerate(r.integers(lo, hi + 1, n))]
