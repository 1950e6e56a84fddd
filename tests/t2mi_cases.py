"""Test streams for the T2-MI deframer, shared by tests/test_cpu_t2mi.py (which checks what the reference parser
makes of them against hand-derived numbers) and tests/test_gpu_t2mi.py (which compares the GPU with that parser).
Every stream is built once from a fixed seed and handed out read-only."""
import functools

import numpy as np

import t2mi_ref as R

PID = 0x1234
L1, F1 = 879, 2          # cfg1q: short 1/2, two blocks per interleaving frame
NFRAMES = 3


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def bbframes(L, nblocks, seed=0):
    b = np.random.default_rng(1000 * L + seed).integers(0, 256, nblocks * L, dtype=np.uint8)
    return _ro(b)


@functools.lru_cache(maxsize=None)
def base_packets(timestamps=3):
    """3 frames of one PLP (plp_id 5): per frame `timestamps` timestamp packets back to back (21 bytes each: three
    starts in one TS packet), an L1-current packet of 203 bits (padded), F1 BBFRAME packets"""
    return tuple(R.encapsulate([(5, bbframes(L1, NFRAMES * F1), L1, F1)], NFRAMES, timestamps=timestamps))


PLPS1 = [(5, L1)]
NPKT1 = NFRAMES * (3 + 1 + F1)


def clean_ts(**kw):
    return R.ts_mux(list(base_packets()), PID, **kw)


def with_packets(edit, **kw):
    """the base stream with its packet list edited before multiplexing"""
    pk = list(base_packets())
    edit(pk)
    return R.ts_mux(pk, PID, **kw)


def bbframe_indices(packets):
    return [i for i, p in enumerate(packets) if p[0] == 0]


def mid_packet_ts_index(ts, which=1):
    """a TS packet of PID with no PUSI whose neighbours are also inside one BBFRAME packet"""
    n = len(ts) // 188
    hits = [i for i in range(1, n - 1)
            if all(R.classify(ts, j, PID)[0] == "ts_contributing" and not R.classify(ts, j, PID)[2]
                   for j in (i - 1, i, i + 1))]
    return hits[which]


def malformed(name):
    """-> (ts, note)"""
    ts = clean_ts()
    if name == "flipped_bit":
        def edit(pk):
            i = bbframe_indices(pk)[2]
            b = bytearray(pk[i])
            b[100] ^= 0x10
            pk[i] = bytes(b)
        return with_packets(edit)
    if name == "dropped":
        i = mid_packet_ts_index(ts)
        return np.delete(ts.reshape(-1, 188), i, axis=0).reshape(-1)
    if name == "duplicated":
        i = mid_packet_ts_index(ts)
        return np.insert(ts.reshape(-1, 188), i, ts.reshape(-1, 188)[i], axis=0).reshape(-1)
    if name == "bad_sync":
        ts[188 * mid_packet_ts_index(ts)] = 0x48
        return ts
    if name == "tei":
        ts[188 * mid_packet_ts_index(ts) + 1] |= 0x80
        return ts
    if name == "scrambled":
        ts[188 * mid_packet_ts_index(ts) + 3] |= 0x40
        return ts
    if name == "pointer":
        # the second PUSI packet with AFC 01 that starts a BBFRAME packet: its pointer_field moved by 5
        n = len(ts) // 188
        hits = [i for i in range(n) if R.classify(ts, i, PID)[2] and ts[188 * i + 3] >> 4 & 3 == 1]
        ts[188 * hits[2] + 4] += 5
        return ts
    if name == "wrong_length":
        def edit(pk):
            i = bbframe_indices(pk)[3]
            pk[i] = R.bbframe_packet(pk[i][1], pk[i][6], 5, pk[i][8] >> 7, bbframes(L1, 1, seed=9)[:L1 - 1])
        return with_packets(edit)
    if name == "unmapped_plp":
        def edit(pk):
            i = bbframe_indices(pk)[3]
            pk[i] = R.bbframe_packet(pk[i][1], pk[i][6], 77, pk[i][8] >> 7, pk[i][9:9 + L1])
        return with_packets(edit)
    if name == "huge_len_last":
        def edit(pk):
            pk.append(bytes([0x00, 0xEE, 0x00, 0x00, 0xFF, 0xFF]) + bytes(40))
        return with_packets(edit)
    if name == "all_ff":
        return np.full(188 * 40, 0xFF, np.uint8)
    if name == "no_pusi":
        rows = ts.reshape(-1, 188)
        keep = [i for i in range(len(rows)) if not R.classify(ts, i, PID)[2]]
        return rows[keep].reshape(-1).copy()
    raise KeyError(name)


MALFORMATIONS = ("flipped_bit", "dropped", "duplicated", "bad_sync", "tei", "scrambled", "pointer", "wrong_length",
                 "unmapped_plp", "huge_len_last", "all_ff", "no_pusi")


def geometry_cases():
    """name -> ts; tests/test_cpu_t2mi.py asserts that each stream has the edge it is named for"""
    pk = list(base_packets())
    st = R.packet_starts(pk)
    bb = bbframe_indices(pk)
    out = {}
    # a T2-MI header split after each of its bytes 1..5, the CRC after each of its bytes 1..3
    s = st[bb[1]]
    e = st[bb[2]] + len(pk[bb[2]])
    for j in range(1, 6):
        out["header_split_%d" % j] = dict(cuts=[s + j])
    for j in range(1, 4):
        out["crc_split_%d" % j] = dict(cuts=[e - 4 + j])
    out["ends_at_payload_end"] = dict(cuts=[e])
    out["pointer_0"] = dict(cuts=[s])
    out["pointer_182"] = dict(cuts=[s - 182])
    out["af_0_and_182"] = dict(af={6: 0, 8: 182, 9: 100})
    out["afc10_mid_packet"] = dict(afc10_before=[7, 8])
    out["foreign_between_all"] = dict(foreign_every=1)
    out["cc_start_13"] = dict(cc0=13)
    return {k: R.ts_mux(pk, PID, **v) for k, v in out.items()}
