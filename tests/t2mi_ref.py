"""T2-MI input (dvbt2ll_t2mi_*, csrc/t2mi_kernels.hip): an encapsulator that builds test streams and a sequential
parser that is the definition of what the GPU deframer must return.  The reference project has no T2-MI code, so
nothing here or in the library is compared with it: parity is pinned by this restatement and by known answers
(PARITY UNPINNED).  Shared by tests/test_cpu_t2mi.py and tests/test_gpu_t2mi.py.

Wire format (ETSI TS 102 773 over DVB data piping), as include/dvbt2ll_hip.h states it:
  TS packet    0x47 | TEI PUSI prio PID[12:8] | PID[7:0] | scrambling(2) AFC(2) CC(4) | [AF length a, a bytes] | payload
  T2-MI packet packet_type(8) packet_count(8) superframe_idx(4) rfu(9) t2mi_stream_id(3) payload_len(16, bits)
               | ceil(payload_len / 8) payload bytes | CRC-32/MPEG-2 of everything before it, big-endian
  type 0x00    frame_idx(8) plp_id(8) intl_frame_start(1) rfu(7) | BBFRAME (kbch bits)
"""
import bisect

import numpy as np

POLY = 0x04C11DB7
MAX_PLP = 8

# record layout of the packet table (dvbt2ll_t2mi_packet)
REC = np.dtype([("ts_index", "<u4"), ("ts_byte", "<u4"), ("packet_type", "u1"), ("packet_count", "u1"),
                ("superframe_idx", "u1"), ("t2mi_stream_id", "u1"), ("payload_len", "<u2"), ("flags", "u1"),
                ("intl_frame_start", "u1"), ("frame_idx", "u1"), ("plp_id", "u1"), ("out_index", "i1"),
                ("reserved", "u1"), ("block", "<i4")])
assert REC.itemsize == 24
F_COMPLETE, F_CONSISTENT, F_CRC_OK, F_ACCEPTED = 1, 2, 4, 8

TS_COUNTERS = ("ts_contributing", "ts_foreign", "ts_null", "ts_tei", "ts_scrambled", "ts_bad_sync", "ts_no_payload",
               "discontinuities", "bad_pointers")
PKT_COUNTERS = ("broken", "crc_errors", "filtered", "len_errors", "other_plp", "accepted")


# ------------------------------------------------------------------------------------------------ CRC-32/MPEG-2
def crc32_bitwise(data, crc=0xFFFFFFFF):
    for b in bytes(data):
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ POLY) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return crc


CRC_TABLE = [crc32_bitwise(bytes([v]), 0) for v in range(256)]


def crc32_table(data, crc=0xFFFFFFFF):
    for b in bytes(data):
        crc = ((crc << 8) & 0xFFFFFFFF) ^ CRC_TABLE[(crc >> 24) ^ b]
    return crc


def gf_mul(a, b):
    """a(x) b(x) mod G(x), bit 31 = x^31"""
    r = 0
    for i in range(31, -1, -1):
        r = ((r << 1) ^ POLY) & 0xFFFFFFFF if r & 0x80000000 else r << 1
        if (b >> i) & 1:
            r ^= a
    return r


XPOW = [0x100]                      # XPOW[i] = x^(8 2^i) mod G
for _ in range(15):
    XPOW.append(gf_mul(XPOW[-1], XPOW[-1]))


def xpow8(n):
    """x^(8 n) mod G"""
    r, i = 1, 0
    while n:
        if n & 1:
            r = gf_mul(r, XPOW[i])
        n >>= 1
        i += 1
    return r


def crc32_combine(data, lanes=64):
    """the kernel's formulation: `lanes` contiguous chunks, each through the byte table (chunk 0 from 0xFFFFFFFF,
    the others from 0), chunk l's register multiplied by x^(8 x bytes after it), all XORed"""
    data = bytes(data)
    c = -(-len(data) // lanes) if data else 0
    out = 0
    for l in range(lanes):
        lo, hi = min(l * c, len(data)), min((l + 1) * c, len(data))
        r = crc32_table(data[lo:hi], 0xFFFFFFFF if l == 0 else 0)
        out ^= gf_mul(r, xpow8(len(data) - hi))
    return out


# ------------------------------------------------------------------------------------------------ encapsulation
def t2mi_packet(ptype, count, payload, payload_bits=None, superframe_idx=0, stream_id=0):
    payload = bytes(payload)
    bits = 8 * len(payload) if payload_bits is None else payload_bits
    assert (bits + 7) // 8 == len(payload) and bits < 65536
    hdr = bytes([ptype & 255, count & 255, (superframe_idx & 15) << 4, stream_id & 7, bits >> 8, bits & 255])
    body = hdr + payload
    return body + crc32_table(body).to_bytes(4, "big")     # the parser checks with the bitwise form


def bbframe_packet(count, frame_idx, plp_id, intl_frame_start, bbframe, **kw):
    return t2mi_packet(0x00, count, bytes([frame_idx & 255, plp_id & 255, 0x80 if intl_frame_start else 0])
                       + bytes(bytearray(bbframe)), **kw)


def timestamp_packet(count, value=0, **kw):
    return t2mi_packet(0x20, count, int(value).to_bytes(11, "big"), **kw)   # 88 payload bits


def l1_packet(count, bits=203, seed=1, **kw):
    """an L1-current packet whose payload_len is no multiple of 8: the last byte zero-padded"""
    n = (bits + 7) // 8
    body = bytearray(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes())
    if bits % 8:
        body[-1] &= (0xFF << (8 - bits % 8)) & 0xFF
    return t2mi_packet(0x10, count, body, payload_bits=bits, **kw)


def encapsulate(plps, nframes, timestamps=1, l1=True, count0=0, stream_id=0):
    """plps: [(plp_id, bbframes (flat uint8), L, F)].  Per T2 frame: `timestamps` timestamp packets back to back, an
    L1-current packet, then every PLP's F BBFRAMEs (the first with intl_frame_start).  Returns the T2-MI packets."""
    out, cnt = [], count0
    for f in range(nframes):
        for _ in range(timestamps):
            out.append(timestamp_packet(cnt, f, superframe_idx=f >> 1, stream_id=stream_id))
            cnt += 1
        if l1:
            out.append(l1_packet(cnt, seed=f, superframe_idx=f >> 1, stream_id=stream_id))
            cnt += 1
        for plp_id, bbf, L, F in plps:
            for b in range(F):
                blk = f * F + b
                out.append(bbframe_packet(cnt, f, plp_id, b == 0, bbf[blk * L:(blk + 1) * L], superframe_idx=f >> 1,
                                          stream_id=stream_id))
                cnt += 1
    return out


def packet_starts(packets):
    s, out = 0, []
    for p in packets:
        out.append(s)
        s += len(p)
    return out


def ts_header(pid, pusi, afc, cc, tei=0, scr=0):
    return bytes([0x47, (tei << 7) | (pusi << 6) | (pid >> 8), pid & 255, (scr << 6) | (afc << 4) | (cc & 15)])


def ts_mux(packets, pid, cc0=0, af=None, cuts=(), afc10_before=(), foreign_every=0, foreign_pid=0x100):
    """T2-MI packets -> TS bytes (uint8 array).
    af            {q: a}: PID packet number q (counting payload-carrying PID packets) gets an adaptation field of
                  length a (0..182), so at most 183 - a payload bytes
    cuts          stream offsets at which a TS payload must end (the packet before is shortened by stuffing)
    afc10_before  PID packet numbers before which an adaptation-field-only packet (AFC 10, CC not advanced) goes
    foreign_every k > 0: after every k-th PID packet one packet of foreign_pid and one null packet
    The last packet is stuffed to its length.  PUSI is set exactly where a T2-MI packet starts."""
    af = dict(af or {})
    stream = b"".join(packets)
    starts = packet_starts(packets)
    cuts = sorted(set(int(c) for c in cuts if 0 < c < len(stream)) | {len(stream)})
    out, pos, q, cc, fcc = [], 0, 0, cc0 & 15, 0
    while pos < len(stream):
        if q in afc10_before:
            out.append(ts_header(pid, 0, 2, (cc - 1) & 15) + bytes([183, 0]) + b"\xff" * 182)
        cap = 184 if q not in af else 183 - af[q]          # payload bytes, a pointer_field included
        to_cut = cuts[bisect.bisect_right(cuts, pos)] - pos
        i = bisect.bisect_left(starts, pos)
        nxt = starts[i] if i < len(starts) else None
        pusi = nxt is not None and nxt < pos + min(cap - 1, to_cut)
        n = min(cap - 1, to_cut) if pusi else min(cap, to_cut)
        if not pusi and nxt is not None and nxt < pos + n:
            n = nxt - pos            # the next packet would start on this packet's last byte: leave it to the next one
        assert n >= 1, "PID packet %d cannot carry a pointer_field and a byte" % q
        body = (bytes([nxt - pos]) if pusi else b"") + stream[pos:pos + n]
        stuff = 184 - len(body)
        if stuff == 0:
            pkt = ts_header(pid, int(pusi), 1, cc) + body
        else:
            a = stuff - 1
            pkt = ts_header(pid, int(pusi), 3, cc) + bytes([a]) + (b"\x00" + b"\xff" * (a - 1) if a else b"") + body
        assert len(pkt) == 188
        out.append(pkt)
        pos += n
        q += 1
        cc = (cc + 1) & 15
        if foreign_every and q % foreign_every == 0:
            out.append(ts_header(foreign_pid, 0, 1, fcc) + bytes(184))
            out.append(ts_header(0x1FFF, 0, 1, 0) + b"\xff" * 184)
            fcc = (fcc + 1) & 15
    return np.frombuffer(b"".join(out), np.uint8).copy()


# ------------------------------------------------------------------------------------------------ the parser
class Result:
    """what one deframer call returns"""

    def __init__(self):
        self.bbframes = []          # per output: uint8 array of the blocks written, L bytes each
        self.packets = np.zeros(0, REC)
        self.counters = {}
        self.blocks = []
        self.by_type = {}
        self.resume = (0, 0)


def classify(ts, i, pid):
    """TS packet i -> (class, payload offset in the packet, pusi, cc); class 0 = contributing"""
    b = ts[188 * i:188 * i + 188]
    if b[0] != 0x47:
        return "ts_bad_sync", 0, 0, 0
    p = ((int(b[1]) & 0x1F) << 8) | int(b[2])
    if p == 0x1FFF:
        return "ts_null", 0, 0, 0
    if p != pid:
        return "ts_foreign", 0, 0, 0
    if b[1] & 0x80:
        return "ts_tei", 0, 0, 0
    if b[3] & 0xC0:
        return "ts_scrambled", 0, 0, 0
    afc = (int(b[3]) >> 4) & 3
    off = 4 if afc == 1 else 5 + int(b[4]) if afc == 3 else 188
    if off >= 188:
        return "ts_no_payload", 0, 0, 0
    return "ts_contributing", off, (int(b[1]) >> 6) & 1, int(b[3]) & 15


def parse(ts, pid, plps, start=(0, 0), caps=None, max_packets=1 << 30, stream_id=-1):
    """The definition.  ts: uint8 array, a multiple of 188 bytes; plps: [(plp_id, L)]; start: (ts_offset, skip) in
    this buffer's coordinates; caps: per output capacity in blocks (None: unbounded)."""
    ts = np.asarray(ts, np.uint8)
    assert len(ts) % 188 == 0 and start[0] % 188 == 0 and 0 <= start[0] <= len(ts) and start[1] >= 0
    n, i0 = len(ts) // 188, start[0] // 188
    caps = [1 << 30] * len(plps) if caps is None else list(caps)
    stream, org, disc, anchors, cls = bytearray(), [], {}, [], {}
    prev_cc = None
    for i in range(i0, n):
        c, off, pusi, cc = classify(ts, i, pid)
        cls[i] = [c]
        if c != "ts_contributing":
            continue
        if prev_cc is not None and cc != (prev_cc + 1) & 15:
            disc[len(stream)] = True
            cls[i].append("discontinuities")
        prev_cc = cc
        lo = 188 * i + off
        if pusi:
            p, lo = int(ts[lo]), lo + 1
            plen = 188 * (i + 1) - lo
            if p >= plen:
                cls[i].append("bad_pointers")
            else:
                anchors.append((i, len(stream) + p, len(stream) + plen))
        for x in range(lo, 188 * (i + 1)):     # byte by byte
            stream.append(int(ts[x]))
            org.append(x)
    S = len(stream)

    def length_at(s):
        return 10 + (((stream[s + 4] << 8) | stream[s + 5]) + 7) // 8 if s + 6 <= S else None

    starts = []     # (stream offset, ts index, number within its TS packet)
    for i, s, end in anchors:
        k = 0
        while True:
            starts.append((s, i, k))
            k += 1
            T = length_at(s)
            if T is None or s + T >= end:
                break
            s += T
    starts = starts[start[1]:]
    discs = sorted(disc)
    ids = [p[0] for p in plps]
    res = Result()
    cnt = dict.fromkeys(TS_COUNTERS + PKT_COUNTERS, 0)
    ranks = [0] * len(plps)
    outs = [bytearray() for _ in plps]
    recs = []
    stop = None
    for j, (s, i, k) in enumerate(starts):
        T = length_at(s)
        if T is None or s + T > S or len(recs) >= max_packets:
            stop = j
            break
        consistent = not (j + 1 < len(starts) and starts[j + 1][0] < s + T)
        d = bisect.bisect_right(discs, s)
        if d < len(discs) and discs[d] < s + T:
            consistent = False
        pkt = bytes(stream[s:s + T])
        crc_ok = crc32_bitwise(pkt[:-4]) == int.from_bytes(pkt[-4:], "big")
        sid = pkt[3] & 7
        accepted = consistent and crc_ok and (stream_id < 0 or sid == stream_id)
        plen = (pkt[4] << 8) | pkt[5]
        r = np.zeros((), REC)
        r["ts_index"], r["ts_byte"] = i, org[s]
        r["packet_type"], r["packet_count"], r["superframe_idx"], r["t2mi_stream_id"] = pkt[0], pkt[1], pkt[2] >> 4, sid
        r["payload_len"] = plen
        r["flags"] = F_COMPLETE | (F_CONSISTENT if consistent else 0) | (F_CRC_OK if crc_ok else 0) | (
            F_ACCEPTED if accepted else 0)
        r["out_index"], r["block"] = -1, -1
        what = None
        if pkt[0] == 0 and plen >= 24:
            r["frame_idx"], r["plp_id"], r["intl_frame_start"] = pkt[6], pkt[7], pkt[8] >> 7
        if not consistent:
            what = "broken"
        elif not crc_ok:
            what = "crc_errors"
        elif not accepted:
            what = "filtered"
        elif pkt[0] == 0:
            pl = pkt[7] if plen >= 24 else -1
            if pl not in ids:
                what = "other_plp"
            else:
                o = ids.index(pl)
                L = plps[o][1]
                if plen != 24 + 8 * L:
                    what = "len_errors"
                elif ranks[o] >= caps[o]:
                    stop = j
                    break
                else:
                    r["out_index"], r["block"] = o, ranks[o]
                    ranks[o] += 1
                    outs[o] += pkt[9:9 + L]
        if accepted:
            cnt["accepted"] += 1
        if what:
            cnt[what] += 1
        res.by_type[pkt[0]] = res.by_type.get(pkt[0], 0) + 1
        recs.append(r)
    if i0 == n:
        res.resume, iend = (start[0], start[1]), n      # nothing to look at: the position stands
    elif stop is None:
        res.resume, iend = (len(ts), 0), n
    else:
        res.resume, iend = (188 * starts[stop][1], starts[stop][2]), starts[stop][1]
    for i in range(i0, iend):
        for c in cls[i]:
            cnt[c] += 1
    res.counters = cnt
    res.blocks = ranks
    res.bbframes = [np.frombuffer(bytes(o), np.uint8) for o in outs]
    res.packets = np.array(recs, REC) if recs else np.zeros(0, REC)
    return res


def parse_chunked(ts, pid, plps, bounds, **kw):
    """chained calls: call c sees ts[:bounds[c]] (a multiple of 188) and starts at the previous resume position;
    returns the concatenated outputs, tables (as returned, in ts coordinates) and summed counters"""
    pos = (0, 0)
    outs = [[] for _ in plps]
    recs, cnt, by_type = [], {}, {}
    done = [0] * len(plps)
    for end in list(bounds) + [len(ts)]:
        r = parse(ts[:end], pid, plps, start=pos, **kw)
        p = r.packets.copy()
        for o, b in enumerate(r.bbframes):
            outs[o].append(b)
            p["block"][p["out_index"] == o] += done[o]     # a call's ranks count from 0
            done[o] += r.blocks[o]
        recs.append(p)
        for k, v in r.counters.items():
            cnt[k] = cnt.get(k, 0) + v
        for k, v in r.by_type.items():
            by_type[k] = by_type.get(k, 0) + v
        pos = r.resume
    return [np.concatenate(o) for o in outs], np.concatenate(recs), cnt, by_type, pos


def interleaving_frames(packets, out_index):
    """block counts between consecutive intl_frame_start = 1 packets of one output (the last run included)"""
    p = packets[(packets["out_index"] == out_index) & (packets["block"] >= 0)]
    at = np.nonzero(p["intl_frame_start"])[0]
    return [int(b - a) for a, b in zip(at, list(at[1:]) + [len(p)])]
