"""PDU lists for the MPE tests (tests/test_cpu_mpe.py, tests/test_gpu_mpe.py): every case is a list of byte strings."""
import numpy as np

PID = 0x100
OVER = 16           # section bytes around a datagram: the 12-byte header and the CRC_32

UNI4 = bytes([10, 0, 0, 1])
V4_GROUP = bytes([239, 1, 2, 3])                                        # -> 01:00:5e:01:02:03
V6_GROUP = bytes.fromhex("ff0200000000000000000001ff001234")            # ff02::1:ff00:1234 -> 33:33:ff:00:12:34


def ip(length, seed=0, first=0x45, dst=None):
    """a PDU of length bytes whose first nibble says IPv4 (0x45), IPv6 (0x60) or neither; dst: the destination
    address written where the header has it (as much of it as the PDU holds)"""
    r = np.random.default_rng(1000 + seed).integers(0, 256, length, dtype=np.uint8)
    r[0] = first
    if dst is not None:
        at = 16 if first >> 4 == 4 else 24
        d = np.frombuffer(bytes(dst), np.uint8)[:max(0, length - at)]
        r[at:at + len(d)] = d
    return r.tobytes()


R_VALUES = (0, 1, 182, 183, 184, 185, 367, 368)
FREE_VALUES = (0, 1, 2, 11, 12)


def r_case(R):
    """the first section has 183 + R bytes: it fills packet 0 behind the pointer_field and packet 1 begins with R
    bytes of it left; two short ones follow (an IPv6 multicast, an IPv4 multicast)"""
    return [ip(183 + R - OVER, R, 0x45, UNI4), ip(40, R + 1, 0x60, V6_GROUP), ip(25, R + 2, 0x45, V4_GROUP)]


def free_case(f):
    """the first section ends with f bytes free in its PUSI packet: the next header starts in the last byte (1),
    straddles (2, 11), just fits (12) or begins a packet (0)"""
    return [ip(183 - f - OVER, 50 + f, 0x45, UNI4), ip(30, 60 + f, 0x45, V4_GROUP), ip(17, 70 + f, 0x60)]


def cases():
    c = {"R%d" % R: r_case(R) for R in R_VALUES}
    c.update({"free%d" % f: free_case(f) for f in FREE_VALUES})
    c["min"] = [ip(1, 80), ip(1, 81, 0x60), ip(2, 82)]                  # the 17-byte section
    c["max"] = [ip(7, 83), ip(4080, 84), ip(9, 85, 0x60)]               # the 4096-byte section
    return c


def mixed(n, seed, lo=1, hi=40):
    """n PDUs of lo .. hi bytes; every seventh IPv6, every fifth to a multicast group where it is long enough"""
    r = np.random.default_rng(seed)
    out = []
    for k, L in enumerate(r.integers(lo, hi + 1, n)):
        first = 0x60 if k % 7 == 3 else 0x45
        dst = (V6_GROUP if first == 0x60 else V4_GROUP) if k % 5 == 1 else None
        out.append(ip(int(L), seed * 100000 + k, first, dst))
    return out
