"""BBFRAME input of the chain (dvbt2ll_chain_set_input, DVBT2LL_INPUT_BBFRAME): test inputs and an independent
reference, shared by tests/test_cpu_bbframe.py (which proves the reference against the oracle) and
tests/test_gpu_bbframe.py.

  * oracle_bbframes: the BBFRAMEs the oracle's bbheaderbch built for a run of frames, descrambled and packed: a
    valid BBFRAME stream whose encoding must be what the TS path produces;
  * encode_ref: BB scrambling + systematic BCH in numpy / Python integers, the parity as the remainder of a
    division by the generator polynomial rebuilt from the standard's minimal polynomials (std_tables.bch_generator,
    as tests/test_cpu_oracle.py uses it) -- nothing of the library's or the oracle's BCH;
  * header_errors: the rule dvbt2ll_chain_bbheader_errors counts by, from the oracle's CRC-8.

Results are computed once per argument set and handed out read-only.
"""
import functools

import numpy as np

from dvbt2ll.configs import KBCH
import bbch_cases as C
import oracle_lib as O
import std_tables as T


def kbch(framesize, rate):
    return KBCH[(framesize, rate)]


def bbframe_len(cfg):
    """L: bytes of one BBFRAME"""
    return kbch(cfg.framesize, cfg.rate) // 8


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def prbs_bits(n):
    b = np.zeros(n, np.uint8)
    O.lib().orc_bb_prbs(O._p(b), n)
    return _ro(b)


@functools.lru_cache(maxsize=None)
def oracle_bbframes(cfg, first_frame, nframes):
    """the unscrambled BBFRAMEs of frames [first_frame, first_frame + nframes) as the oracle's bbheaderbch built them
    from the synthetic TS: L bytes per FEC block, back to back"""
    k = kbch(cfg.framesize, cfg.rate)
    nb = nframes * cfg.fecblocks
    bits = C.oracle_bits(cfg, first_frame, nframes).reshape(nb, -1)
    return _ro(np.packbits(bits[:, :k] ^ prbs_bits(k)[None, :], axis=1).reshape(-1))


@functools.lru_cache(maxsize=None)
def _bch_table(framesize, P):
    """byte-wise division table of the generator g (degree P): entry v = (v x^P) mod g as an integer"""
    g = T.bch_generator(framesize == 1, P)   # highest power first
    gi = int("".join(str(int(b)) for b in g), 2)
    top = 1 << P
    tab = []
    for v in range(256):
        r = v << P
        for bit in range(P + 7, P - 1, -1):
            if (r >> bit) & 1:
                r ^= gi << (bit - P)
        assert r < top
        tab.append(r)
    return tab


def bch_parity(framesize, P, msg_bytes):
    """the P parity bits (an integer, first transmitted bit = MSB) of the message bytes: (m(x) x^P) mod g(x)"""
    tab = _bch_table(framesize, P)
    mask, sh = (1 << P) - 1, P - 8
    r = 0
    for b in msg_bytes:
        r = ((r << 8) & mask) ^ tab[(r >> sh) ^ b]
    return r


def encode_ref(framesize, rate, bbframes):
    """bbframes: packed unscrambled BBFRAMEs (a multiple of L bytes) -> nbch bits per block, flat uint8: the
    scrambled BBFRAME followed by its BCH parity (what bbch_cases.pack_codewords takes)"""
    k = kbch(framesize, rate)
    nbch, _ = T.fec(framesize, rate)
    P, L = nbch - k, k // 8
    assert P % 8 == 0 and k % 8 == 0
    frames = np.asarray(bbframes, np.uint8).reshape(-1, L)
    scr = frames ^ np.packbits(prbs_bits(k))[None, :]
    out = np.zeros((len(frames), nbch), np.uint8)
    out[:, :k] = np.unpackbits(scr, axis=1)
    for i, row in enumerate(scr):
        par = bch_parity(framesize, P, row.tolist())
        out[i, k:] = np.unpackbits(np.frombuffer(par.to_bytes(P // 8, "big"), np.uint8))
    return out.reshape(-1)


def crc8(data):
    data = bytes(bytearray(data))
    return int(O.lib().orc_crc8_dvbs2(data, len(data)))


def header_errors(L, bbframes):
    """the BBFRAMEs whose byte 9 is neither the CRC-8 of bytes 0 .. 8 nor that value XOR 1 (the HEM mode bit)"""
    frames = np.asarray(bbframes, np.uint8).reshape(-1, L)
    return sum(1 for f in frames if (crc8(f[:9]) ^ int(f[9])) & 0xFE)
