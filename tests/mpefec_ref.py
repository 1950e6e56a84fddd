"""MPE-FEC (this project's reading of EN 301 192 clause 9: MPE sections with real-time parameters, then Reed-Solomon
columns in MPE-FEC sections) restated sequentially for the tests of dvbt2ll_mpefec_* (include/dvbt2ll_hip.h states
the rules):

encap()    the encapsulator: one frame buffer and one section at a time, then tests/mpe_ref.py's sequential packer
           restated over a list of sections; RS by polynomial division with log / antilog tables, vectorised over the
           rows only
receive()  an independent receiver: the TS and section layer of ISO/IEC 13818-1 for table_ids 3E and 78, datagrams
           placed by their address, frames delimited by the boundary flags, delta_t / section_number / padding_columns
           / ascending addresses checked, the syndromes of every row by Horner evaluation (no code shared with the
           encoder), and an erasure decoder that solves for known bad columns over GF(2^8)

Nothing here looks at the GPU code's passes."""
import zlib
from typing import NamedTuple

import numpy as np

import mpe_ref as M

MAC = M.MAC
COUNTERS = ("pdus_in", "sections", "fec_sections", "frames", "skipped_len", "skipped_type", "mapped_macs",
            "ts_packets", "pusi_packets", "pad_bytes", "flushed")
ROWS = (256, 512, 768, 1024)

_REV8 = bytes(int("{:08b}".format(v)[::-1], 2) for v in range(256))


def crc32_fast(data):
    """the sections' CRC (generator 0x04C11DB7, initial value 0xFFFFFFFF, no reflection, no final XOR) through zlib's
    reflected CRC-32 of the bit-reversed bytes (tests/test_cpu_mpefec.py proves it equal to mpe_ref.crc32)"""
    c = zlib.crc32(bytes(data).translate(_REV8)) ^ 0xFFFFFFFF
    return int("{:032b}".format(c)[::-1], 2)


# ------------------------------------------------------------------------------------------------ GF(2^8), 0x11D
EXP = np.zeros(510, np.int64)
LOG = np.zeros(256, np.int64)
_x = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _x
    LOG[_x] = _i
    _x = (_x << 1) ^ (0x11D if _x & 0x80 else 0)


def gmul(a, b):
    """element-wise product of two arrays (or scalars) over GF(2^8)"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    return np.where((a == 0) | (b == 0), 0, EXP[LOG[a] + LOG[b]])


def generator():
    """g(x) = prod (x + lambda^i), i = 0 .. 63: coefficients g_0 .. g_64 (g_64 = 1)"""
    g = [1]
    for i in range(64):
        r = int(EXP[i])
        n = [0] * (len(g) + 1)
        for k, c in enumerate(g):
            n[k + 1] ^= c
            n[k] ^= int(gmul(c, r))
        g = n
    return g


G = generator()


def rs_parity(d):
    """d: (191, R) data symbols, row c = d_c -> (64, R): par_0 .. par_63, the remainder of sum d_c x^(254 - c) by g,
    par_k the coefficient of x^(63 - k)"""
    d = np.asarray(d, np.int64)
    par = np.zeros((64, d.shape[1]), np.int64)
    gk = np.array([G[63 - k] for k in range(64)], np.int64)[:, None]
    for c in range(191):
        fb = d[c] ^ par[0]
        par[:-1] = par[1:]
        par[-1] = 0
        par ^= gmul(gk, fb[None, :])
    return par.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the encapsulator
class Result(NamedTuple):
    ts: np.ndarray        # uint8, 188 bytes per packet
    resume: tuple         # (pdu, section, section_byte, cc, frame)
    counters: dict


pack = M.pack


def classify(pdu, off, i, rows, D):
    k = M.classify(pdu, off, i)
    if k == "ok" and int(off[i + 1]) - int(off[i]) > min(M.MAX_PDU, D * rows):
        return "len"
    return k


def rt_word(delta_t, tb, fb, address):
    return ((delta_t & 0xFFF) << 20 | int(tb) << 19 | int(fb) << 18 | address).to_bytes(4, "big")


def mpe_section(data, mac, rt, crc):
    n = 12 + len(data) + 4
    sl = n - 3
    s = bytes([0x3E, 0xB0 | (sl >> 8), sl & 255, mac[5], mac[4], 0xC1, 0, 0]) + rt + bytes(data)
    return s + crc(s).to_bytes(4, "big")


def fec_section(col, k, K, pad, rt, crc):
    L = len(col) + 13
    s = bytes([0x78, 0xB0 | (L >> 8), L & 255, pad, 0xFF, 0xFF, k, K - 1]) + rt + bytes(col)
    return s + crc(s).to_bytes(4, "big")


def partition(pdu, off, first, rows, D, flush):
    """the frames of the PDUs from first on: ([(first index, end index, [the valid indices])], where what is left
    begins: the open frame's first index, or n_pdus)"""
    n_pdus, C = len(off) - 1, D * rows
    frames, s, members, U = [], first, [], 0
    for i in range(first, n_pdus):
        if classify(pdu, off, i, rows, D) != "ok":
            continue
        p = int(off[i + 1]) - int(off[i])
        if U + p > C:                     # it does not fit: the frame is closed just behind its last datagram
            frames.append((s, members[-1] + 1, members))
            s, members, U = members[-1] + 1, [], 0
        members.append(i)
        U += p
    if members and flush:
        frames.append((s, members[-1] + 1, members))
        s, members = members[-1] + 1, []
    return frames, (s if members else n_pdus)


_FRAMES = {}


def frame_sections(pdu, off, members, rows, K, delta_t, mac, mac_mode, crc):
    """the m + K sections of one closed frame.  A frame met again (the chained-call tests meet each many times) is
    taken from a table keyed by everything that goes into it"""
    datas = tuple(pdu[int(off[i]):int(off[i + 1])].tobytes() for i in members)
    key = (datas, rows, K, delta_t & 0xFFF, bytes(mac), mac_mode, crc)
    if key not in _FRAMES:
        if len(_FRAMES) > 2048:
            _FRAMES.clear()
        _FRAMES[key] = _frame_sections(pdu, off, members, rows, K, delta_t, mac, mac_mode, crc)
    return _FRAMES[key]


def _frame_sections(pdu, off, members, rows, K, delta_t, mac, mac_mode, crc):
    A = np.zeros(191 * rows, np.uint8)
    U, out = 0, []
    for j, i in enumerate(members):
        data = pdu[int(off[i]):int(off[i + 1])].tobytes()
        m, mapped = M.mac_of(data, mac, mac_mode)
        out.append(mpe_section(data, m, rt_word(delta_t, j == len(members) - 1, 0, U), crc))
        A[U:U + len(data)] = np.frombuffer(data, np.uint8)
        U += len(data)
    par = rs_parity(A.reshape(191, rows))
    pad = 191 - -(-U // rows)
    for k in range(K):
        out.append(fec_section(par[k].tobytes(), k, K, pad, rt_word(delta_t, k == K - 1, k == K - 1, k * rows), crc))
    return out


def pack_sections(secs, s_byte, packing, flush):
    """tests/mpe_ref.py's sequential packer over a list of (bytes, label): the packets [(PUSI, payload, (label,
    byte))] and the position left behind when the end is reached without a flush (None: nothing)"""
    pkts, cur, cur_pos, left = [], None, None, None
    for idx, (S, lab) in enumerate(secs):
        k = s_byte if idx == 0 else 0
        nxt = idx + 1 < len(secs)
        if not packing:
            first = k == 0
            while k < len(S):
                take = min(183 if first else 184, len(S) - k)
                pkts.append((1, b"\0" + S[k:k + take], (lab, k)) if first else (0, S[k:k + take], (lab, k)))
                k += take
                first = False
            continue
        if k == 0:
            if cur is None:
                cur, cur_pos = bytearray([0]), (lab, 0)
            take = min(184 - len(cur), len(S))
            cur += S[:take]
            k = take
        while True:
            if cur is not None:
                if len(cur) == 184:
                    pkts.append((1, bytes(cur), cur_pos))
                    cur = None
                elif k == len(S):
                    if not nxt:
                        if flush:
                            pkts.append((1, bytes(cur), cur_pos))
                        else:
                            left = cur_pos
                        cur = None
                    break
            if k == len(S):
                break
            R = len(S) - k
            if R >= 183:
                pkts.append((0, S[k:k + 184], (lab, k)))
                k = min(len(S), k + 184)
            elif nxt:
                cur, cur_pos = bytearray([R]) + S[k:], (lab, k)
                k = len(S)
            else:
                if flush:
                    pkts.append((0, S[k:], (lab, k)))
                else:
                    left = (lab, k)
                k = len(S)
    return pkts, left


def encap(pdu, off, rows=256, D=191, K=64, pid=0x100, mac=MAC, mac_mode=0, packing=1, start=(0, 0, 0, 0, 0), cap=None,
          max_frames=1 << 16, flush=False, crc=crc32_fast):
    pdu = np.asarray(pdu, np.uint8)
    n_pdus = len(off) - 1
    s_pdu, s_sec, s_byte, s_cc, s_frame = (int(x) for x in start)
    frames, rest = partition(pdu, off, s_pdu, rows, D, flush)
    F = min(len(frames), int(max_frames))
    look = F < len(frames)          # a closed frame past max_frames: its sections decide the packet frame F - 1 ends in
    secs = []
    for f in range(F + look):
        fs = frame_sections(pdu, off, frames[f][2], rows, K, s_frame + f, mac, mac_mode, crc)
        secs += [(S, (f, j)) for j, S in enumerate(fs)]
    if F:
        m0 = len(frames[0][2])
        if s_sec < 0 or s_sec >= m0 + K:          # inconsistent: taken as 0
            s_sec = s_byte = 0
        if s_byte < 0 or s_byte >= len(secs[s_sec][0]):
            s_byte = 0
        secs = secs[s_sec:]
    pkts, left = pack_sections(secs, s_byte if F else 0, packing, bool(flush) and not look) if F else ([], None)
    E = len(pkts)
    if look:                        # no packet that begins behind frame F - 1's last byte
        E = sum(1 for pk in pkts if pk[2][0][0] < F)
    if cap is not None:
        E = min(int(cap), E)
    cc = (s_cc + E) & 15
    if not F:
        fr = 0
        resume = (s_pdu, start[1], start[2], cc, s_frame & 0xFFF) if rest < n_pdus else (n_pdus, 0, 0, cc, s_frame & 0xFFF)
        resume = tuple(int(x) for x in resume)
    else:
        pos = pkts[E][2] if E < len(pkts) else left
        if pos is not None:
            (fr, j), k = pos
            resume = (frames[fr][0], j, k, cc, (s_frame + fr) & 0xFFF)
        else:
            fr = F
            resume = (rest, 0, 0, cc, (s_frame + F) & 0xFFF)
    ts = np.full((E, 188), 0xFF, np.uint8)
    pad = pusi = 0
    for p, (u, payload, _) in enumerate(pkts[:E]):
        ts[p, :4] = [0x47, (u << 6) | (pid >> 8), pid & 255, 0x10 | ((s_cc + p) & 15)]
        ts[p, 4:4 + len(payload)] = np.frombuffer(payload, np.uint8)
        pad += 184 - len(payload)
        pusi += u
    r_pdu = resume[0]
    kinds = [classify(pdu, off, i, rows, D) for i in range(s_pdu, r_pdu)]
    mapped = 0
    for i in range(s_pdu, r_pdu):
        if kinds[i - s_pdu] == "ok":
            mapped += M.mac_of(pdu[int(off[i]):int(off[i + 1])].tobytes(), mac, mac_mode)[1]
    c = dict(pdus_in=len(kinds), sections=kinds.count("ok"), fec_sections=fr * K, frames=fr,
             skipped_len=kinds.count("len"), skipped_type=kinds.count("type"), mapped_macs=mapped, ts_packets=E,
             pusi_packets=pusi, pad_bytes=pad, flushed=int(bool(flush) and r_pdu == n_pdus))
    return Result(ts.reshape(-1), resume, c)


def packet_bound(pdu_len, n, rows, D, K, packing, max_frames):
    """include/dvbt2ll_hip.h: the packets that PDUs lying side by side cannot exceed"""
    F = min(max_frames, n, 2 * pdu_len // (D * rows + 1) + 2)
    total = pdu_len + 16 * n + F * K * (rows + 16)
    return total // 183 + 2 if packing else total // 184 + n + F * K + 1


def valid_pdus(pdu, off, rows, D, first=0):
    pdu = np.asarray(pdu, np.uint8)
    return [pdu[int(off[i]):int(off[i + 1])].tobytes() for i in range(first, len(off) - 1)
            if classify(pdu, off, i, rows, D) == "ok"]


# ------------------------------------------------------------------------------------------------ the receiver
def _gf_mul_slow(a, b):
    """shift-and-add product (the receiver's own arithmetic)"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = (a << 1) ^ (0x11D if a & 0x80 else 0)
        b >>= 1
    return r


_MULT = None


def _mult():
    """the 256 x 256 product table, from the shift-and-add product"""
    global _MULT
    if _MULT is None:
        t = np.zeros((256, 256), np.uint8)
        for a in range(256):
            for b in range(a, 256):
                t[a, b] = t[b, a] = _gf_mul_slow(a, b)
        _MULT = t
    return _MULT


def _alpha(e):
    v = 1
    for _ in range(e % 255):
        v = _gf_mul_slow(v, 2)
    return v


def syndromes(code):
    """code: (255, R) symbols, row c the coefficient of x^(254 - c) -> (64, R): the polynomial at lambda^0 .. 63, by
    Horner"""
    T = _mult()
    code = np.asarray(code, np.uint8)
    out = np.zeros((64, code.shape[1]), np.uint8)
    for i in range(64):
        a = _alpha(i)
        acc = np.zeros(code.shape[1], np.uint8)
        for c in range(255):
            acc = T[a][acc] ^ code[c]
        out[i] = acc
    return out


def _gf_inv(a):
    T = _mult()
    return int(np.nonzero(T[a] == 1)[0][0])


def erasure_fill(code, bad):
    """code with the columns in bad unknown: solves sum_j e_j X_j^i = S_i (i below len(bad)) and fills them in; None
    where there are more than 64 or the filled rows are no codewords"""
    bad = sorted(set(bad))
    if len(bad) > 64:
        return None
    T = _mult()
    code = np.array(code, np.uint8)
    code[bad] = 0
    S = syndromes(code)
    t = len(bad)
    if t:
        X = [_alpha(254 - c) for c in bad]
        Mx = [[1] * t]
        for i in range(1, t):
            Mx.append([int(T[Mx[-1][j]][X[j]]) for j in range(t)])
        rhs = S[:t].copy()
        for col in range(t):                      # Gauss-Jordan; the right side is a row of symbols per equation
            piv = next(r for r in range(col, t) if Mx[r][col])
            Mx[col], Mx[piv] = Mx[piv], Mx[col]
            rhs[[col, piv]] = rhs[[piv, col]]
            inv = _gf_inv(Mx[col][col])
            Mx[col] = [int(T[inv][v]) for v in Mx[col]]
            rhs[col] = T[inv][rhs[col]]
            for r in range(t):
                if r != col and Mx[r][col]:
                    f = Mx[r][col]
                    Mx[r] = [a ^ int(T[f][b]) for a, b in zip(Mx[r], Mx[col])]
                    rhs[r] ^= T[f][rhs[col]]
        for j, c in enumerate(bad):
            code[c] = rhs[j]
    return code if not syndromes(code).any() else None


class Frame(NamedTuple):
    delta_t: int
    datagrams: list       # [bytes]: as received, or (lossy) as read out of the repaired table
    macs: list            # (MAC_address_6, MAC_address_5) per received MPE section
    bad_columns: int      # the unreliable data and RS columns that were repaired
    ok: bool              # False: too many unreliable columns


def _sections(ts, pid, cc, crc, lossy):
    """ISO/IEC 13818-1 section reassembly: the sections whose CRC is 0.  lossy: a continuity error drops the section
    in progress and the stream is picked up at the next pointer_field; else it raises"""
    ts = np.asarray(ts, np.uint8).reshape(-1, 188)
    out, buf = [], None

    def feed(seg, may_start):
        nonlocal buf
        pos = 0
        while pos < len(seg):
            if buf is None:
                if seg[pos] == 0xFF:
                    assert all(b == 0xFF for b in seg[pos:]), "stuffing"
                    return
                assert may_start, "a section starts where no pointer_field points"
                buf = bytearray()
            want = 3 if len(buf) < 3 else 3 + (((buf[1] & 15) << 8) | buf[2])
            take = min(want - len(buf), len(seg) - pos)
            buf += seg[pos:pos + take]
            pos += take
            if len(buf) >= 3 and len(buf) == 3 + (((buf[1] & 15) << 8) | buf[2]):
                s, buf = bytes(buf), None
                assert len(s) <= 4096 and crc(s) == 0, "CRC"
                out.append(s)

    for p in ts:
        assert p[0] == 0x47 and not p[1] & 0x80
        if (((int(p[1]) & 0x1F) << 8) | int(p[2])) != pid:
            continue
        assert p[3] >> 4 == 1, "adaptation field control"
        if cc is not None and (p[3] & 15) != cc:
            assert lossy, "continuity"
            buf = None
        cc = ((p[3] & 15) + 1) & 15
        pay = bytes(p[4:])
        if p[1] & 0x40:
            ptr = pay[0]
            assert ptr <= 182, "pointer_field points outside the packet"
            if buf is not None:
                feed(pay[1:1 + ptr], False)
                assert buf is None, "the pointer_field contradicts the section in progress"
            feed(pay[1 + ptr:], True)
        elif buf is not None:
            feed(pay, False)
    assert buf is None or lossy, "the stream ends inside a section"
    return out


def _ip_length(b):
    """the length an IP header states (lossy receive reads the datagrams out of the repaired table by it)"""
    if len(b) >= 4 and b[0] >> 4 == 4:
        return int.from_bytes(b[2:4], "big")
    if len(b) >= 6 and b[0] >> 4 == 6:
        return 40 + int.from_bytes(b[4:6], "big")
    return 0


def receive(ts, K, pid=0x100, cc=0, delta_t=0, crc=crc32_fast, lossy=False):
    """-> [Frame].  Strict (lossy False): every rule of the stream is asserted and every row's 64 syndromes are
    computed (the punctured RS columns are solved for first when K < 64).  lossy: packets may be missing; what was not
    received is marked unreliable byte by byte, and the columns holding such bytes are repaired"""
    out = []
    rows = None
    dgs, macs, addr, closed_table, fec, pad = [], [], 0, False, {}, None
    for s in _sections(ts, pid, cc, crc, lossy):
        assert s[1] >> 4 == 0xB
        rt = int.from_bytes(s[8:12], "big")
        dt, tb, fb, a = rt >> 20, (rt >> 19) & 1, (rt >> 18) & 1, rt & 0x3FFFF
        if s[0] == 0x3E:
            assert s[5] == 0xC1 and s[6] == 0 and s[7] == 0 and not fb
            assert dt == delta_t & 0xFFF, "delta_t"
            assert not closed_table and not fec, "an MPE section behind the table boundary"
            assert a == addr or (lossy and a > addr), "address"
            dgs.append((a, s[12:-4]))
            macs.append((s[3], s[4]))
            addr = a + len(s) - 16
            closed_table = bool(tb)
            continue
        assert s[0] == 0x78 and s[4] == 0xFF and s[5] == 0xFF and s[7] == K - 1
        assert dt == delta_t & 0xFFF, "delta_t"
        r = len(s) - 16
        assert r in ROWS and (rows is None or rows == r)
        rows = r
        k = s[6]
        assert a == k * rows and k < K and (k == len(fec) or (lossy and k > len(fec) and k not in fec))
        assert closed_table or lossy, "an MPE-FEC section before the table boundary"
        assert pad is None or pad == s[3]
        pad = s[3]
        assert tb == fb == (k == K - 1)
        fec[k] = np.frombuffer(s[12:-4], np.uint8)
        if not fb:
            continue
        # the frame is complete: the table, byte-wise reliability, the repair
        ncol = 191 - pad
        A = np.zeros(191 * rows, np.uint8)
        known = np.zeros(191 * rows, bool)
        known[ncol * rows:] = True
        for a0, d in dgs:
            assert a0 + len(d) <= ncol * rows
            A[a0:a0 + len(d)] = np.frombuffer(d, np.uint8)
            known[a0:a0 + len(d)] = True
        if closed_table:
            known[addr:] = True
            assert -(-addr // rows) == ncol, "padding_columns"
        code = np.zeros((255, rows), np.uint8)
        code[:191] = A.reshape(191, rows)
        bad = [c for c in range(191) if not known[c * rows:(c + 1) * rows].all()]
        lost = len(bad)
        for k2 in range(64):
            if k2 in fec:
                code[191 + k2] = fec[k2]
            else:
                bad.append(191 + k2)
                lost += k2 < K
        assert lossy or lost == 0
        fixed = erasure_fill(code, bad)
        if fixed is None:
            out.append(Frame(delta_t & 0xFFF, [d for _, d in dgs], macs, lost, False))
        else:
            got = [d for _, d in dgs]
            if lost:
                flat, got, at = fixed[:191].reshape(-1).tobytes(), [], 0
                while at < ncol * rows and _ip_length(flat[at:at + 6]):
                    got.append(flat[at:at + _ip_length(flat[at:at + 6])])
                    at += len(got[-1])
            out.append(Frame(delta_t & 0xFFF, got, macs, lost, True))
        delta_t += 1
        dgs, macs, addr, closed_table, fec, pad = [], [], 0, False, {}, None
    assert lossy or (not dgs and not fec), "the stream ends inside a frame"
    return out
