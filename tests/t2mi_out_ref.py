"""T2-MI output (dvbt2ll_t2mi_out_*, csrc/t2mi_out_kernels.hip): the definition of what the GPU framer must write.

frame()        the sequential framer: t2mi_ref.t2mi_packet / bbframe_packet per packet, t2mi_ref.ts_mux for the TS layer.
frame_numpy()  a restatement for long streams: the packets built as arrays, the TS layer laid out from the closed-form
               positions (every TS packet's stream position follows from the packet start before it).  carry=False is
               a deliberately wrong variant that forgets where the previous T2 frame ended inside its TS packet: the
               tests show the comparison sees that.
Shared by tests/test_cpu_t2mi_out.py and tests/test_gpu_t2mi_out.py; the case lists are here too.
"""
import numpy as np

import t2mi_ref as R

PID = 0x1000


class Shape:
    """the constants of a handle: plps [(plp_id, Lb, F)], aux [(packet_type, payload_bits, after)]"""

    def __init__(self, plps, aux=(), fps=2, stream_id=0, pid=PID):
        self.plps, self.aux, self.fps, self.stream_id, self.pid = list(plps), list(aux), fps, stream_id, pid
        self.aux_bytes = [(b + 7) // 8 for _, b, _ in self.aux]
        self.aux_off = [int(x) for x in np.cumsum([0] + [n + 3 for n in self.aux_bytes])[:-1]]   # gaps between them
        self.aux_stride = sum(n + 3 for n in self.aux_bytes) + 5
        # (kind, index, block) per packet of a frame
        self.order = [("aux", a, 0) for a, s in enumerate(self.aux) if s[2] == 0]
        self.order += [("plp", k, b) for k, p in enumerate(self.plps) for b in range(p[2])]
        self.order += [("aux", a, 0) for a, s in enumerate(self.aux) if s[2] == 1]
        self.lengths = [10 + (self.aux_bytes[i] if kind == "aux" else 3 + self.plps[i][1]) for kind, i, _ in self.order]
        self.P, self.B = len(self.order), sum(self.lengths)

    def inputs(self, nframes, seed=1, dirty=True):
        """random BBFRAMEs per PLP and an auxiliary buffer whose gaps and pad bits are set (dirty)"""
        rng = np.random.default_rng(seed)
        bb = [rng.integers(0, 256, nframes * F * L, dtype=np.uint8) for _, L, F in self.plps]
        n = max(1, (nframes - 1) * self.aux_stride + sum(x + 3 for x in self.aux_bytes))
        aux = rng.integers(0, 256, n, dtype=np.uint8)
        if not dirty:
            for f in range(nframes):
                for a, (_, bits, _) in enumerate(self.aux):
                    if bits % 8:
                        aux[f * self.aux_stride + self.aux_off[a] + self.aux_bytes[a] - 1] &= (0xFF << (8 - bits % 8)) & 0xFF
        return bb, aux

    def aux_payload(self, aux, f, a):
        o = f * self.aux_stride + self.aux_off[a]
        b = bytearray(aux[o:o + self.aux_bytes[a]].tobytes())
        bits = self.aux[a][1]
        if bits % 8:
            b[-1] &= (0xFF << (8 - bits % 8)) & 0xFF        # the pad bits are forced to zero
        return bytes(b)


def packets(sh, bb, aux, nframes, start=(0, 0, 0)):
    """the call's T2-MI packets in order"""
    out, cnt = [], start[1]
    for f in range(nframes):
        fr = start[0] + f
        kw = dict(superframe_idx=(fr // sh.fps) & 15, stream_id=sh.stream_id)
        for kind, i, b in sh.order:
            if kind == "aux":
                out.append(R.t2mi_packet(sh.aux[i][0], cnt, sh.aux_payload(aux, f, i), payload_bits=sh.aux[i][1], **kw))
            else:
                plp_id, L, F = sh.plps[i]
                blk = f * F + b
                out.append(R.bbframe_packet(cnt, fr % sh.fps, plp_id, b == 0, bb[i][blk * L:(blk + 1) * L], **kw))
            cnt += 1
    return out


def counters_of(ts, npackets, nframes):
    """TS-level counters read back from the bytes themselves"""
    t = np.asarray(ts, np.uint8).reshape(-1, 188)
    afc = (t[:, 3] >> 4) & 3
    stuff = np.where(afc == 3, t[:, 4].astype(np.int64) + 1, 0)
    return dict(frames=nframes, t2mi_packets=npackets, ts_packets=len(t), pusi_packets=int(((t[:, 1] >> 6) & 1).sum()),
                stuffing_bytes=int(stuff.sum()))


def frame(sh, bb, aux, nframes, start=(0, 0, 0)):
    """the definition: (ts bytes, next position, counters, by_type)"""
    pk = packets(sh, bb, aux, nframes, start)
    ts = R.ts_mux(pk, sh.pid, cc0=start[2]) if pk else np.zeros(0, np.uint8)
    by_type = {}
    for p in pk:
        by_type[p[0]] = by_type.get(p[0], 0) + 1
    nxt = (start[0] + nframes, (start[1] + len(pk)) & 255, (start[2] + len(ts) // 188) & 15)
    return ts, nxt, counters_of(ts, len(pk), nframes), by_type


# ------------------------------------------------------------------------------------------------ closed form
def ts_packets(sh, nframes):
    """the TS packets of a call, from the packet lengths alone"""
    q, pos, s = 0, 0, 0
    for T in sh.lengths * nframes:
        s += T
        q, pos = _advance(q, pos, s)
    return q + (1 if s > pos else 0)


def _advance(q, pos, s):
    """(q, pos): the PUSI packet holding the previous start carries [pos, pos + 183); the same for the start at s"""
    if s - pos <= 182:
        return q, pos
    m, rem = divmod(s - pos - 183, 184)
    if rem <= 182:
        return q + 1 + m, pos + 183 + 184 * m
    return q + 2 + m, s          # the packet before is shortened to 183 bytes


_CRC_TAB = np.array(R.CRC_TABLE, np.uint32)


def _crc_rows(rows):
    """CRC-32/MPEG-2 of every row of a 2-D uint8 array"""
    crc = np.full(len(rows), 0xFFFFFFFF, np.uint32)
    for c in range(rows.shape[1]):
        crc = (crc << np.uint32(8)) ^ _CRC_TAB[(crc >> np.uint32(24)) ^ rows[:, c]]
    return crc


def stream_numpy(sh, bb, aux, nframes, start=(0, 0, 0)):
    """the call's T2-MI byte stream: one (nframes, T) array per packet of the frame, CRCs by columns"""
    fr = start[0] + np.arange(nframes)
    out = np.zeros((nframes, sh.B), np.uint8)
    at = 0
    for j, (kind, i, b) in enumerate(sh.order):
        T = sh.lengths[j]
        p = out[:, at:at + T]
        bits = sh.aux[i][1] if kind == "aux" else 24 + 8 * sh.plps[i][1]
        p[:, 0] = sh.aux[i][0] if kind == "aux" else 0
        p[:, 1] = (start[1] + np.arange(nframes) * sh.P + j) & 255
        p[:, 2] = ((fr // sh.fps) & 15) << 4
        p[:, 3], p[:, 4], p[:, 5] = sh.stream_id, bits >> 8, bits & 255
        if kind == "aux":
            n = sh.aux_bytes[i]
            idx = (np.arange(nframes) * sh.aux_stride + sh.aux_off[i])[:, None] + np.arange(n)[None, :]
            p[:, 6:6 + n] = np.asarray(aux)[idx]
            if bits % 8:
                p[:, 5 + n] &= (0xFF << (8 - bits % 8)) & 0xFF
        else:
            plp_id, L, F = sh.plps[i]
            p[:, 6], p[:, 7], p[:, 8] = fr % sh.fps, plp_id, 0x80 if b == 0 else 0
            p[:, 9:9 + L] = np.asarray(bb[i])[:nframes * F * L].reshape(nframes, F, L)[:, b, :]
        crc = _crc_rows(p[:, :T - 4])
        for k in range(4):
            p[:, T - 4 + k] = (crc >> np.uint32(8 * (3 - k))) & 255
        at += T
    return out.reshape(-1)


def _layout(starts, E, rec, base=0):
    """the TS packets of a stream of E bytes whose packets start at `starts` (starts[0] = 0), appended to rec as
    (stream position, bytes carried, PUSI, pointer_field); base is added to the positions"""
    q_pos, ptr = 0, 0                # the open PUSI packet: it carries [q_pos, q_pos + 183)
    for s in list(starts[1:]) + [None]:
        end = s is None
        if end:
            s = E
        if s - q_pos <= (183 if end else 182):
            if end:
                rec.append((base + q_pos, s - q_pos, 1, ptr))
            continue
        rec.append((base + q_pos, 183, 1, ptr))
        pos1 = q_pos + 183
        m, rem = divmod(s - pos1, 184)
        rec.extend((base + pos1 + 184 * k, 184, 0, 0) for k in range(m))
        if end:
            if rem:
                rec.append((base + pos1 + 184 * m, rem, 0, 0))
        elif rem <= 182:
            q_pos, ptr = pos1 + 184 * m, rem
        else:                        # the start would lie on the packet's last byte: 183 bytes, then the start
            rec.append((base + pos1 + 184 * m, 183, 0, 0))
            q_pos, ptr = s, 0


def frame_numpy(sh, bb, aux, nframes, start=(0, 0, 0), carry=True):
    """frame() restated: the same four results.  carry=False is the wrong variant that lays every T2 frame out as if
    it began a TS packet: the offset d at which the previous frame ended inside its TS packet is dropped"""
    stream = stream_numpy(sh, bb, aux, nframes, start)
    E = len(stream)
    off = np.concatenate(([0], np.cumsum(sh.lengths)[:-1]))
    rec = []
    if carry:
        _layout((np.arange(nframes)[:, None] * sh.B + off[None, :]).reshape(-1).tolist(), E, rec)
    else:
        for f in range(nframes):
            _layout(off.tolist(), sh.B, rec, base=f * sh.B)
    pos_l, n_l, pusi_l, ptr_l = zip(*rec) if rec else ((), (), (), ())
    pos_a, n_a = np.array(pos_l, np.int64), np.array(n_l, np.int64)
    pusi_a, ptr_a = np.array(pusi_l, np.int64), np.array(ptr_l, np.int64)
    N = len(pos_a)
    ts = np.full((N, 188), 0xFF, np.uint8)
    stuff = 184 - n_a - pusi_a
    ts[:, 0] = 0x47
    ts[:, 1] = (pusi_a << 6) | (sh.pid >> 8)
    ts[:, 2] = sh.pid & 255
    ts[:, 3] = (np.where(stuff > 0, 3, 1) << 4) | ((start[2] + np.arange(N)) & 15)
    col = np.arange(188)[None, :]
    data_c = (188 - n_a)[:, None]
    src = pos_a[:, None] + (col - data_c)
    body = col >= data_c
    ts[body] = stream[np.clip(src, 0, E - 1)][body]
    has_ptr = pusi_a == 1
    ts[has_ptr, (187 - n_a)[has_ptr]] = ptr_a[has_ptr]
    st = stuff > 0
    ts[st, 4] = (stuff - 1)[st]
    ts[stuff > 1, 5] = 0
    ts = ts.reshape(-1)
    G = nframes * sh.P
    by_type = {}
    for kind, i, _ in sh.order:
        t = sh.aux[i][0] if kind == "aux" else 0
        by_type[t] = by_type.get(t, 0) + nframes
    nxt = (start[0] + nframes, (start[1] + G) & 255, (start[2] + N) & 15)
    return ts, nxt, counters_of(ts, G, nframes), by_type


# ------------------------------------------------------------------------------------------------ case lists
LB_SMALL, LB_ODD = 654, 6051        # kbch 5232 (the smallest code the deframer takes) and 48408

# the aux sweep: the length of the slot before a single Lb = 654 BBFRAME runs over 1 .. 190 bytes and some bit lengths
# with pad bits; two short fixed slots follow the BBFRAME, so that they and the next frame's first packet can start
# inside one TS packet.  (shape, nframes) per case
AUX_SWEEP_BITS = [8 * n for n in range(1, 191)] + [1, 7, 9, 43, 203, 1001, 1515]


def aux_sweep_cases():
    return [(Shape([(0, LB_SMALL, 1)], aux=[(0x20, bits, 0), (0x10, 8, 1), (0x21, 12, 1)]), 1 + i % 4)
            for i, bits in enumerate(AUX_SWEEP_BITS)]


# four slots, with pad bits, before and after the BBFRAMEs
EDGE_SHAPES = [
    Shape([(3, LB_SMALL, 1)], aux=[(0x20, 88, 0), (0x10, 203, 0), (0x21, 12, 0), (0x30, 5, 1)]),
    Shape([(3, LB_SMALL, 2)], aux=[(0x20, 8, 0), (0x10, 8, 0), (0x11, 8, 0), (0x12, 8, 0)]),
]

THREE_PLPS = Shape([(7, 879, 2), (0, LB_SMALL, 1), (200, 1194, 3)], aux=[(0x20, 88, 0), (0x10, 203, 1)], fps=3,
                   stream_id=5)


def edges_of(ts, pid=PID):
    """what a framed TS exhibits: pointer values, shortened non-PUSI packets, the most starts inside one TS packet,
    the final packet's stuffing"""
    t = np.asarray(ts, np.uint8).reshape(-1, 188)
    afc = (t[:, 3] >> 4) & 3
    stuff = np.where(afc == 3, t[:, 4].astype(np.int64) + 1, 0)
    pusi = ((t[:, 1] >> 6) & 1).astype(bool)
    ptr = t[np.arange(len(t)), 4 + stuff][pusi]
    res = R.parse(ts, pid, [])
    per_ts = np.bincount(res.packets["ts_index"], minlength=len(t))
    return dict(pointers=set(int(p) for p in ptr), shortened=int(((stuff[:-1] == 1) & ~pusi[:-1]).sum()),
                most_starts=int(per_ts.max()), final_stuff=int(stuff[-1]))
