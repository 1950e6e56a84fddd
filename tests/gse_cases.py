"""PDU lists for the GSE tests (tests/test_cpu_gse.py, tests/test_gpu_gse.py): every case is a list of byte strings."""
import numpy as np

KBCHS = (3072, 7032, 32208, 58192)        # D = 374, 869, 4016 (below one maximal packet), 7264 (above it)
LABELS = (b"", bytes([0x0A, 0x0B, 0x0C]), bytes([0x02, 0x00, 0x47, 0x53, 0x45, 0x31]))


def D_of(kbch):
    return (kbch - 80) // 8


def ip(length, seed=0, first=0x45):
    """a PDU of length bytes whose first nibble says IPv4 (0x45), IPv6 (0x60) or neither"""
    r = np.random.default_rng(2000 + seed).integers(0, 256, length, dtype=np.uint8)
    r[0] = first
    return r.tobytes()


def fill(u, L, seed=0):
    """PDUs whose complete packets take exactly u bytes from a frame's start (u = 0, or u >= 5 + L)"""
    assert u == 0 or u >= 5 + L
    out = []
    while u:
        p = min(u, 4 + L + 1400)
        if 0 < u - p < 5 + L:
            p -= 5 + L
        out.append(ip(p - 4 - L, seed + len(out), 0x60 if len(out) % 2 else 0x45))
        u -= p
    return out


FREES = ("0", "1", "7+L", "8+L", "3+L+len", "4+L+len", "5+L+len")
REMS = ("D-8", "D-7", "D-6", "D-3", "D-2", "2D")
EDGE_LEN = 100


def free_case(D, L, name):
    """a PDU of EDGE_LEN bytes meets a frame with free bytes left; two short ones follow"""
    free = {"0": 0, "1": 1, "7+L": 7 + L, "8+L": 8 + L, "3+L+len": 3 + L + EDGE_LEN, "4+L+len": 4 + L + EDGE_LEN,
            "5+L+len": 5 + L + EDGE_LEN}[name]
    return fill(D - free, L, 10) + [ip(EDGE_LEN, 20), ip(40, 21, 0x60), ip(25, 22)]


def rem_case(D, L, name):
    """a PDU's first fragment takes 5 bytes, so that it is open with rem bytes left at the next frame's start; None
    where no PDU is that long"""
    rem = {"D-8": D - 8, "D-7": D - 7, "D-6": D - 6, "D-3": D - 3, "D-2": D - 2, "2D": 2 * D}[name]
    if rem + 5 > 4090 - L:
        return None
    return fill(D - 7 - L - 5, L, 30) + [ip(rem + 5, 40), ip(40, 41, 0x60), ip(25, 42)]


def cases(kbch, L):
    D = D_of(kbch)
    c = {"free " + f: free_case(D, L, f) for f in FREES}
    c.update({"rem " + r: rem_case(D, L, r) for r in REMS if rem_case(D, L, r) is not None})
    c["len 1, max"] = [ip(1, 50), ip(4090 - L, 51), ip(1, 52, 0x60), ip(7, 53)]
    c["too long, empty"] = [ip(9, 54), ip(4091 - L, 55), b"", ip(9, 56)]
    return c


def mixed(n, seed, lo=1, hi=40):
    r = np.random.default_rng(seed)
    return [ip(int(L), seed * 100000 + k, 0x60 if k % 7 == 3 else 0x45) for k, L in enumerate(r.integers(lo, hi + 1, n))]
