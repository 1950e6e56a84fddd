"""ULE (RFC 4326) restated sequentially for the tests of dvbt2ll_ule_* (include/dvbt2ll_hip.h states the rules):

encap()    the encapsulator: one SNDU at a time, one packet buffer, a plain loop; its CRC is bitwise
receive()  an independent receiver after RFC 4326 section 7: Payload Pointer handling, End Indicator, continuity
           and CRC checks; it returns (type, dest, pdu) per SNDU

Nothing here looks at the GPU code's passes: no scan, no state maps, no search."""
from typing import NamedTuple

import numpy as np

POLY = 0x04C11DB7
MAC = bytes([0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B])   # the flowgraph's destination address
COUNTERS = ("pdus_in", "sndus", "skipped_len", "skipped_type", "ts_packets", "pusi_packets", "pad_bytes", "flushed")


def crc32(data, crc=0xFFFFFFFF):
    """CRC-32 of generator 0x04C11DB7, initial value 0xFFFFFFFF, no reflection, no final XOR: bit by bit"""
    for b in bytes(data):
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ POLY) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return crc


_TAB = None


def crc32_table(data, crc=0xFFFFFFFF):
    """the same CRC through a byte table (for the large cases; tests/test_cpu_ule.py proves it equal to crc32)"""
    global _TAB
    if _TAB is None:
        _TAB = []
        for v in range(256):
            c = v << 24
            for _ in range(8):
                c = ((c << 1) ^ POLY) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
            _TAB.append(c)
    for b in bytes(data):
        crc = ((crc << 8) & 0xFFFFFFFF) ^ _TAB[(crc >> 24) ^ b]
    return crc


class Result(NamedTuple):
    ts: np.ndarray        # uint8, 188 bytes per packet
    resume: tuple         # (pdu, sndu_byte, cc)
    counters: dict


def pack(pdus):
    """a list of byte strings -> (the PDU buffer, the offset table)"""
    off = np.zeros(len(pdus) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pdus])
    return np.frombuffer(b"".join(bytes(p) for p in pdus), np.uint8).copy(), off


def classify(pdu, off, i, types, d_bit):
    """PDU i: ("ok", type), ("len", 0) or ("type", 0); the length is judged first"""
    o0, o1 = int(off[i]), int(off[i + 1])
    if o1 <= o0 or o1 > len(pdu) or (0 if d_bit else 6) + (o1 - o0) + 4 > 32767:
        return "len", 0
    if types is not None:
        return "ok", int(types[i])
    nib = int(pdu[o0]) >> 4
    if nib == 4:
        return "ok", 0x0800
    if nib == 6:
        return "ok", 0x86DD
    return "type", 0


def sndu(data, typ, d_bit, dest, crc=crc32):
    length = (0 if d_bit else 6) + len(data) + 4
    s = bytes([(d_bit << 7) | (length >> 8), length & 255, typ >> 8, typ & 255])
    if not d_bit:
        s += bytes(dest)
    s += bytes(data)
    return s + crc(s).to_bytes(4, "big")


def encap(pdu, off, types=None, pid=0x100, d_bit=0, dest=MAC, packing=1, start=(0, 0, 0), cap=None, flush=False,
          crc=crc32):
    pdu = np.asarray(pdu, np.uint8)
    n_pdus = len(off) - 1
    s_pdu, s_byte, s_cc = (int(x) for x in start)
    kinds = {i: classify(pdu, off, i, types, d_bit) for i in range(s_pdu, n_pdus)}
    valid = [i for i in range(s_pdu, n_pdus) if kinds[i][0] == "ok"]
    pkts = []       # (PUSI, the payload bytes before the FF fill, the position (pdu, sndu_byte) the packet begins at)
    cur = None      # the open PUSI packet: its payload so far, PP included; cur_pos: the position it begins at
    cur_pos = None
    left = None     # the position of what stays behind when the end is reached without a flush
    for idx, i in enumerate(valid):
        S = sndu(pdu[int(off[i]):int(off[i + 1])].tobytes(), kinds[i][1], d_bit, dest, crc)
        k = s_byte if idx == 0 and i == s_pdu and s_byte < len(S) else 0
        nxt = idx + 1 < len(valid)
        if not packing:
            first = k == 0
            while k < len(S):
                take = min(183 if first else 184, len(S) - k)
                pkts.append((1, b"\0" + S[k:k + take], (i, k)) if first else (0, S[k:k + take], (i, k)))
                k += take
                first = False
            continue
        if k == 0:      # a new SNDU: behind the open packet's bytes, or behind a Payload Pointer of 0
            if cur is None:
                cur, cur_pos = bytearray([0]), (i, 0)
            take = min(184 - len(cur), len(S))
            cur += S[:take]
            k = take
        while True:
            if cur is not None:
                if len(cur) >= 183:         # full, or one byte free: FF, closed
                    pkts.append((1, bytes(cur), cur_pos))
                    cur = None
                elif k == len(S):           # the SNDU ended with two or more bytes free
                    if not nxt:
                        if flush:
                            pkts.append((1, bytes(cur), cur_pos))
                        else:
                            left = cur_pos
                        cur = None
                    break
            if k == len(S):
                break
            R = len(S) - k                  # a packet begins inside the SNDU
            if R >= 182:
                pkts.append((0, S[k:k + 184], (i, k)))
                k = min(len(S), k + 184)
            elif nxt:
                cur, cur_pos = bytearray([R]) + S[k:], (i, k)
                k = len(S)
            else:
                if flush:
                    pkts.append((0, S[k:], (i, k)))
                else:
                    left = (i, k)
                k = len(S)
    E = len(pkts) if cap is None else min(int(cap), len(pkts))
    if E < len(pkts):
        r_pdu, r_byte = pkts[E][2]
    elif left is not None:
        r_pdu, r_byte = left
    else:
        r_pdu, r_byte = n_pdus, 0
    ts = np.full((E, 188), 0xFF, np.uint8)
    pad = pusi = 0
    for p, (u, payload, _) in enumerate(pkts[:E]):
        ts[p, :4] = [0x47, (u << 6) | (pid >> 8), pid & 255, 0x10 | ((s_cc + p) & 15)]
        ts[p, 4:4 + len(payload)] = np.frombuffer(payload, np.uint8)
        pad += 184 - len(payload)
        pusi += u
    before = [kinds[i][0] for i in range(s_pdu, r_pdu)]
    c = dict(pdus_in=len(before), sndus=before.count("ok"), skipped_len=before.count("len"),
             skipped_type=before.count("type"), ts_packets=E, pusi_packets=pusi, pad_bytes=pad,
             flushed=int(bool(flush) and r_pdu == n_pdus))
    return Result(ts.reshape(-1), (r_pdu, r_byte, (s_cc + E) & 15), c)


def receive(ts, pid=0x100, cc=None, crc=crc32, open_end=False):
    """RFC 4326 section 7 on the packets of pid: [(type, dest or None, pdu bytes)].  Raises AssertionError on a
    continuity error, a Payload Pointer that contradicts the SNDU in progress, an SNDU start in a packet without
    PUSI, a CRC error, or (unless open_end) a stream that ends inside an SNDU; the encapsulator's output has none"""
    ts = np.asarray(ts, np.uint8).reshape(-1, 188)
    out = []
    cur, need = None, 0     # the SNDU in progress and the bytes it still lacks
    for p in ts:
        assert p[0] == 0x47 and not p[1] & 0x80
        if (((int(p[1]) & 0x1F) << 8) | int(p[2])) != pid:
            continue
        assert p[3] >> 4 == 1, "adaptation field control"
        if cc is not None:
            assert (p[3] & 15) == cc, "continuity"
        cc = ((p[3] & 15) + 1) & 15
        pay = bytes(p[4:])
        pusi = bool(p[1] & 0x40)
        pos = 0
        if pusi:
            pp = pay[0]
            assert pp <= 182
            if cur is not None:
                assert need == pp, "the Payload Pointer contradicts the SNDU in progress"
            pos = 1 if cur is not None else 1 + pp   # nothing in progress: the bytes before the first start are skipped
        elif cur is None:
            continue            # idle: a packet without PUSI and nothing in progress is ignored
        started = 0
        while True:
            if cur is not None:
                take = min(need, 184 - pos)
                cur += pay[pos:pos + take]
                pos += take
                need -= take
                if need:
                    break       # runs on into the next packet
                body, got = bytes(cur[:-4]), int.from_bytes(cur[-4:], "big")
                assert crc(body) == got, "CRC"
                d = body[0] >> 7
                typ = (body[2] << 8) | body[3]
                out.append((typ, None, body[4:]) if d else (typ, body[4:10], body[10:]))
                cur = None
            if 184 - pos < 2:
                break           # no room for a Length field: one byte is discarded
            length = (pay[pos] << 8) | pay[pos + 1]
            if length == 0xFFFF:
                break           # the End Indicator: idle until the next PUSI
            assert pusi, "an SNDU starts in a packet without PUSI"
            if started == 0:
                assert pos == 1 + pay[0], "the first SNDU starts where the Payload Pointer says"
            started += 1
            cur, need = bytearray(), 4 + (length & 0x7FFF)
    assert cur is None or open_end, "the stream ends inside an SNDU"
    return out


def valid_pdus(pdu, off, types=None, d_bit=0, dest=MAC, first=0):
    """what receive() must return for the PDUs from first on"""
    out = []
    for i in range(first, len(off) - 1):
        kind, typ = classify(pdu, off, i, types, d_bit)
        if kind == "ok":
            data = np.asarray(pdu, np.uint8)[int(off[i]):int(off[i + 1])].tobytes()
            out.append((typ, None if d_bit else bytes(dest), data))
    return out
