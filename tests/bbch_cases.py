"""Case construction shared by tests/test_cpu_bbch_cases.py (which proves the inputs do what they claim) and
tests/test_gpu_bbch_edges.py (which runs them through the fused BB/BCH kernel, t2_kernels.hip bbch_kernel).

The kernel derives every BBFRAME from closed-form stream geometry (bb_geom, mod188, the per-lane cursors);
the reference (and the oracle) keep running state instead.  Restated here in Python integers:

  * block_geom: bb_geom for absolute FEC block B;
  * sync_count: the sync bytes a run of frames consumes (the reference's "Transport Stream sync error!" sites,
    bbheaderbch_bb_impl.cc:675-677, 703-705), closed form;
  * ts_span: the TS bytes the chain API demands for a run (t2_capi.cpp ts_span);
  * shifted_run: a small frame k whose real bytes are declared to sit at a large frame K's stream position,
    so that the oracle (which only runs from the stream start) can check offsets past 2^31, 2^32 and 2^40.

Oracle results are computed once per case and handed out read-only.
"""
import functools
import math

import numpy as np

from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, KBCH, payload_pos, ts_for_frames, ts_packets
import oracle_lib as O

BAD_SYNC = 0x46


def is_hem(cfg):
    return cfg.inputmode != E.INPUTMODE_NORMAL


def has_inband(cfg):
    return cfg.inband != E.INBAND_OFF


def pay_full(cfg):
    """payload bytes of a BBFRAME without the in-band field"""
    return (KBCH[(cfg.framesize, cfg.rate)] - 80) // 8


def frame_payload(cfg):
    """payload bytes per T2 frame: F BBFRAME payloads less the 13 in-band type B bytes of the first"""
    return cfg.fecblocks * pay_full(cfg) - (13 if has_inband(cfg) else 0)


def packet_period(cfg):
    """payload bytes per TS packet: 188 (NM: the sync slot carries the CRC-8) or 187 (HEM: the sync byte is dropped)"""
    return 187 if is_hem(cfg) else 188


def block_geom(cfg, B):
    """bb_geom (t2_kernels.hip) for absolute FEC block B: first payload index J0, payload bytes, padding bits,
    stream position of the first payload byte, and count0 = the reference's `count` at block start"""
    F, pay = cfg.fecblocks, pay_full(cfg)
    npad_before, padding = 0, 0
    if has_inband(cfg):
        npad_before = (B + F - 1) // F
        padding = 104 if B % F == 0 else 0
    npay = pay - padding // 8
    J0 = B * pay - 13 * npad_before
    hem = is_hem(cfg)
    pos0 = payload_pos(J0, hem)
    if hem:
        count0 = 0 if J0 == 0 else (payload_pos(J0 - 1, True) + 1) % 188
    else:
        count0 = pos0 % 188
    return dict(J0=J0, npay=npay, padding=padding, pos0=pos0, count0=count0)


def first_sync_offset(cfg, B):
    """payload byte offset (BBFRAME byte 10 + this) of the first sync position of block B: the NM slot that
    carries a CRC-8, or in HEM the payload byte in front of which a sync byte was dropped"""
    m = packet_period(cfg)
    return (m - block_geom(cfg, B)["J0"] % m) % m


def multiples_in(lo, hi, m):
    """number of multiples of m in [lo, hi)"""
    return (hi + m - 1) // m - (lo + m - 1) // m


def sync_count(cfg, first_frame, nframes):
    """sync bytes the reference consumes while it encodes T2 frames [first_frame, first_frame + nframes): a sync
    byte is consumed together with the payload byte after it (NM: its slot), so they are the payload indices J
    in the frames' range with J = 0 mod the packet period (NM: J is the stream position)"""
    P = frame_payload(cfg)
    return multiples_in(first_frame * P, (first_frame + nframes) * P, packet_period(cfg))


def ts_span(cfg, first_frame, nframes):
    """[lo, end) of the stream the chain demands for the run (t2_capi.cpp ts_span): from the packet before the
    first one touched through the last consumed byte (HEM: through the sync byte in front of the next payload
    byte when the run ends on a packet boundary)"""
    P = frame_payload(cfg)
    start, e = first_frame * P, (first_frame + nframes) * P
    if is_hem(cfg):
        start = 188 * (start // 187) + start % 187
        e = 188 * (e // 187) + e % 187 + 1
    lo = (start // 188) * 188 - 188 if start >= 188 else 0
    return lo, e


def stream_slice(lo, end, seed=1):
    """bytes [lo, end) of the synthetic stream (lo on a packet boundary)"""
    assert lo % 188 == 0
    return ts_packets(lo // 188, (end - lo + 187) // 188, seed)[:end - lo].copy()


def corrupt_syncs(ts, base):
    """a copy with every sync byte (stream position = 0 mod 188) set to 0x46"""
    assert base % 188 == 0
    bad = np.array(ts, np.uint8, copy=True)
    bad[::188] = BAD_SYNC
    return bad


# ------------------------------------------------------------------------------------------------ configs
_C1, _C4 = CONFIGS["cfg1"], CONFIGS["cfg4"]

# Residue sweeps (cfg1's 4K frame, 3 data symbols, 8 short FEC blocks of 2025 256-QAM cells each, as cfg1
# carries): a code whose BBFRAME payload is coprime to the packet period, so consecutive blocks visit every
# start phase.  NM: rate 1/2, 869 bytes, gcd(869, 188) = 1; HEM: rate 3/5, 1184 bytes, gcd(1184, 187) = 1.
# In-band type B shortens every frame's first payload by 13 bytes; the frame counts are the smallest multiple
# of 4 that still covers every phase (test_cpu_bbch_cases asserts the coverage).
SWEEPS = {
    "nm": (_C1.with_(rate=E.C1_2), 24),
    "hem": (_C1.with_(rate=E.C3_5, inputmode=E.INPUTMODE_HIEFF), 24),
    "nm-inband": (_C1.with_(rate=E.C1_2, inband=E.INBAND_ON, tsrate=12345678), 32),
    "hem-inband": (_C1.with_(rate=E.C3_5, inputmode=E.INPUTMODE_HIEFF, inband=E.INBAND_ON, tsrate=12345678), 160),
}
SPLIT = (5, 7)   # a sweep as three calls: frames [0, 5), [5, 12), [12, n)

# 64800-bit blocks (cfg4's 8K frame, rate 3/5, 16-QAM, 3 blocks): the BBFRAME is 152 32-byte chunks, so the
# kernel's split of K into BCH_KS slices falls mid-BBFRAME
NORMAL = {
    "nm": (_C4.with_(rate=E.C3_5, fecblocks=3), 2),
    "hem": (_C4.with_(rate=E.C3_5, fecblocks=3, inputmode=E.INPUTMODE_HIEFF), 2),
}

# Stream offsets: cfg1 itself (rate 4/5, 1544 payload bytes) in the four input modes, two frames per run
OFFSET_CFGS = {
    "nm": _C1,
    "hem": _C1.with_(inputmode=E.INPUTMODE_HIEFF),
    "nm-inband": _C1.with_(inband=E.INBAND_ON, tsrate=12345678),
    "hem-inband": _C1.with_(inputmode=E.INPUTMODE_HIEFF, inband=E.INBAND_ON, tsrate=12345678),
}
OFFSET_FRAMES = 2
BOUNDARIES = {"2^31": 1 << 31, "2^32": 1 << 32, "2^40": 1 << 40}
OFFSET_CASES = [(m, b) for m in OFFSET_CFGS for b in BOUNDARIES]
IQ_OFFSET_CASES = [("nm-inband", "2^32"), ("hem", "2^40")]   # whole-IQ checks: one NM, one HEM
GRAPH_OFFSET_CASE = ("hem-inband", "2^32")

# Tight TS slices: (config, first frame), one frame each.  The window ends inside the last 16-byte piece's
# fetch in every case (the kernel's bytewise edge path at the high end).  Frame 10 in NM starts 4 bytes into a
# packet, so the CRC prologue of its first block (from 208 bytes before the payload) starts 16 bytes before
# the window, which begins one packet before the first one touched: the edge path at the low end, mid-stream.
TIGHT_CASES = {
    "nm": (_C1, 5),
    "nm-low-edge": (_C1, 10),
    "hem": (_C1.with_(inputmode=E.INPUTMODE_HIEFF), 5),
}
TIGHT_FRAMES = 1


# ------------------------------------------------------------------------------------------------ offsets
def consumed_range(cfg, first_frame, nframes):
    """[first, last] stream positions of the payload bytes of the run"""
    P, hem = frame_payload(cfg), is_hem(cfg)
    return payload_pos(first_frame * P, hem), payload_pos((first_frame + nframes) * P - 1, hem)


def repeat_frames(cfg):
    """frames after which the stream phase (position mod the packet period) and FRAME_IDX both repeat"""
    m = packet_period(cfg)
    a = m // math.gcd(frame_payload(cfg), m)
    return a * cfg.t2frames // math.gcd(a, cfg.t2frames)


def large_frame(cfg, boundary, nframes=OFFSET_FRAMES):
    """the frame K whose run [K, K + nframes) has `boundary` strictly inside its consumed bytes (2^31, 2^32:
    frame K starts below it, frame K + 1 lies above it), or, for 2^40, lies wholly above it"""
    P, hem = frame_payload(cfg), is_hem(cfg)
    K = (boundary * 187 // 188 if hem else boundary) // P
    while payload_pos(K * P, hem) >= boundary:
        K -= 1
    while payload_pos((K + 1) * P, hem) < boundary:
        K += 1
    return K + 1 if boundary >= 1 << 40 else K


def shifted_run(cfg, K, nframes=OFFSET_FRAMES):
    """frames [K, K + n) of the stream, whose bytes are declared to be those of frames [k, k + n): k = K mod
    repeat_frames, so every block keeps its packet phase, in-band phase and FRAME_IDX, and the stream positions
    differ by a whole number D of packets.  Returns k, D, the TS buffer of frames [k, k + n) and the base to
    declare for it"""
    per, P = repeat_frames(cfg), frame_payload(cfg)
    k = K % per
    if is_hem(cfg):
        assert (K - k) * P % 187 == 0
        D = 188 * ((K - k) * P // 187)
    else:
        D = (K - k) * P
    ts, base = ts_for_frames(cfg, k, nframes)
    return k, D, ts, base + D


# ------------------------------------------------------------------------------------------------ oracle
def _ro(a):
    a.setflags(write=False)
    return a


def pack_codewords(cfg, bits, nb):
    """the chain's packed interleaver-input codewords from the oracle's bbheaderbch output: LDPC, then the
    parity interleaved [row a][column c] where the constellation has it (as test_chain_codewords_all_codes)"""
    import plan_probe as PP
    fp = PP.fec_plan(cfg.framesize, cfg.rate, cfg.constellation)
    nbch, q = fp["nbch"], fp["q"]
    nldpc = 64800 if cfg.framesize else 16200
    cw = O.LDPC(cfg.framesize, cfg.rate).work(bits, nb).reshape(nb, nldpc)
    if fp["parity_il"]:
        t, s = np.divmod(np.arange(nldpc - nbch), 360)
        cw = cw.copy()
        cw[:, nbch:] = cw[:, nbch + q * s + t]
    return np.packbits(cw, axis=1)


def codeword_mismatches(cfg, got, want):
    """indices of the blocks whose packed codeword bytes differ"""
    nbytes = (64800 if cfg.framesize else 16200) // 8
    return np.nonzero((got[:, :nbytes] != want).any(axis=1))[0].tolist()


@functools.lru_cache(maxsize=None)
def _oracle_run(cfg, first_frame, nframes, corrupt):
    """the oracle from the stream start: bbheaderbch only over frames [0, first_frame) (they carry count / crc /
    fec_block), then frames [first_frame, first_frame + nframes).  Returns their bbheaderbch bits, the sync
    warnings of those frames alone, and the TS buffer used"""
    ts, base = ts_for_frames(cfg, 0, first_frame + nframes)
    assert base == 0
    if corrupt:
        ts = corrupt_syncs(ts, 0)
    bb = O.BB(*cfg.bb_args())
    F, off = cfg.fecblocks, 0
    for _ in range(first_frame):
        _, c = bb.work(ts[off:], F)
        off += c
    before = bb.sync_errors()
    bits, _ = bb.work(ts[off:], nframes * F)
    return _ro(bits), bb.sync_errors() - before, _ro(ts)


def oracle_bits(cfg, first_frame, nframes, corrupt=False):
    return _oracle_run(cfg, first_frame, nframes, bool(corrupt))[0]


def oracle_sync_errors(cfg, first_frame, nframes):
    """the oracle's warning count over the frames when every sync byte of the stream is 0x46"""
    return _oracle_run(cfg, first_frame, nframes, True)[1]


@functools.lru_cache(maxsize=None)
def oracle_codewords(cfg, first_frame, nframes, corrupt=False):
    """packed codewords of frames [first_frame, first_frame + nframes), one row per FEC block"""
    return _ro(pack_codewords(cfg, oracle_bits(cfg, first_frame, nframes, corrupt), nframes * cfg.fecblocks))


def oracle_carriers(cfg, first_frame, nframes):
    """the oracle chain's pre-IFFT carriers of frames [first_frame, first_frame + nframes) and its pilotgen
    (the framemapper is started at first_frame: its state is the frame number)"""
    F = cfg.fecblocks
    bits = oracle_bits(cfg, first_frame, nframes)
    ld, im = O.LDPC(cfg.framesize, cfg.rate), O.IM(*cfg.im_args())
    fm, pg = O.FM(*cfg.fm_args()), O.PG(*cfg.pg_args())
    O.lib().orc_fm_seek(fm.h, first_frame)
    nb = bits.size // (nframes * F)
    out = []
    for f in range(nframes):
        fb = bits[f * F * nb:(f + 1) * F * nb]
        out.append(pg.carriers(fm.work(im.work(ld.work(fb, F), F))))
    return out, pg
