"""GSE (TS 102 606-1, as include/dvbt2ll_hip.h states the rules) restated sequentially for the tests of dvbt2ll_gse_*:

encap()    the encapsulator: one PDU at a time, one frame buffer, a plain loop; its CRC is bitwise
receive()  an independent receiver: BBFRAME header CRC-8, DFL, the packets of each data field, reassembly by Frag ID,
           Total Length and CRC-32; it returns (type, label, pdu) per PDU

Nothing here looks at the GPU code's passes: no tables, no chain, no search."""
from typing import NamedTuple

import numpy as np

POLY = 0x04C11DB7
LABEL = bytes([0x02, 0x00, 0x47, 0x53, 0x45, 0x31])
COUNTERS = ("pdus_in", "complete", "fragmented", "gse_packets", "skipped_len", "skipped_type", "bbframes", "pad_bytes",
            "flushed")
LT_OF = {6: 0, 3: 1, 0: 2}


def crc32(data, crc=0xFFFFFFFF):
    """CRC-32/MPEG-2: generator 0x04C11DB7, initial value 0xFFFFFFFF, MSB first, no final XOR: bit by bit"""
    for b in bytes(data):
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ POLY) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return crc


_TAB = None


def crc32_table(data, crc=0xFFFFFFFF):
    """the same CRC through a byte table (for the large cases; tests/test_cpu_gse.py proves it equal to crc32)"""
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


def crc8(data):
    """the BBHEADER's CRC-8, generator x^8 + x^7 + x^6 + x^4 + x^2 + 1, bit by bit"""
    c = 0
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0xD5) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


class Result(NamedTuple):
    bb: np.ndarray        # uint8, kbch / 8 bytes per BBFRAME
    resume: tuple         # (pdu, pdu_byte, frag_id)
    counters: dict


def pack(pdus):
    """a list of byte strings -> (the PDU buffer, the offset table)"""
    off = np.zeros(len(pdus) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pdus])
    return np.frombuffer(b"".join(bytes(p) for p in pdus), np.uint8).copy(), off


def classify(pdu, off, i, types, L):
    """PDU i: ("ok", type), ("len", 0) or ("type", 0); the length is judged first"""
    o0, o1 = int(off[i]), int(off[i + 1])
    if o1 <= o0 or o1 > len(pdu) or o1 - o0 > 4090 - L:
        return "len", 0
    if types is not None:
        return "ok", int(types[i])
    nib = int(pdu[o0]) >> 4
    if nib == 4:
        return "ok", 0x0800
    if nib == 6:
        return "ok", 0x86DD
    return "type", 0


def _head(S, E, lt, nbytes):
    return bytes([(S << 7) | (E << 6) | (lt << 4) | (nbytes >> 8), nbytes & 255])


def header(kbch, sis_mis, isi, used):
    h = bytes([0xB0 if sis_mis else 0x90, 0 if sis_mis else isi, 0, 0, (8 * used) >> 8, (8 * used) & 255, 0, 0, 0])
    return h + bytes([crc8(h)])


def encap(pdu, off, types=None, kbch=7032, label=LABEL, sis_mis=1, isi=0, start=(0, 0, 0), cap=None, flush=False,
          crc=crc32):
    """label: 6, 3 or 0 bytes.  Returns the emitted BBFRAMEs, the resume position and the counters"""
    pdu = np.asarray(pdu, np.uint8)
    label = bytes(label or b"")
    L, D, n_pdus = len(label), (kbch - 80) // 8, len(off) - 1
    lt = LT_OF[L]
    s_pdu, s_byte, s_fid = (int(x) for x in start)
    kinds = {i: classify(pdu, off, i, types, L) for i in range(s_pdu, n_pdus)}
    frames = []     # closed frames: (data-field bytes, the position (pdu, pdu_byte) the frame begins at, GSE packets)
    cur, cur_pos, cur_pk = bytearray(), None, 0
    fragmented = set()

    def close():
        nonlocal cur, cur_pos, cur_pk
        frames.append((bytes(cur), cur_pos, cur_pk))
        cur, cur_pos, cur_pk = bytearray(), None, 0

    def put(packet, pos):
        nonlocal cur_pos, cur_pk
        if not cur:
            cur_pos = pos
        cur.extend(packet)
        cur_pk += 1
        assert len(cur) <= D
        if len(cur) == D:
            close()

    first_valid = True
    for i in range(s_pdu, n_pdus):
        if kinds[i][0] != "ok":
            continue
        data = pdu[int(off[i]):int(off[i + 1])].tobytes()
        typ, fid = kinds[i][1], (s_fid + i - s_pdu) & 255
        body = bytes([typ >> 8, typ & 255]) + label + data            # what follows Total Length in a first fragment
        total = (2 + L + len(data)).to_bytes(2, "big")
        sent = s_byte if first_valid and i == s_pdu and 1 <= s_byte <= len(data) - 1 else 0
        first_valid = False
        if sent == 0:
            free = D - len(cur)
            if free < 4 + L + len(data) and free < 8 + L:
                close()                                                # the frame as it is; fresh at u = 0
                free = D
            if free >= 4 + L + len(data):
                put(_head(1, 1, lt, 2 + L + len(data)) + body, (i, 0))
                continue
            piece = free - 7 - L
            assert 1 <= piece < len(data) - 2
            put(_head(1, 0, lt, free - 2) + bytes([fid]) + total + body[:2 + L + piece], (i, 0))
            sent = piece
        fragmented.add(i)
        while True:                                                    # open, at u = 0
            assert not cur
            rem = len(data) - sent
            if rem + 7 <= D:
                put(_head(0, 1, 3, 5 + rem) + bytes([fid]) + data[sent:] + crc(total + body).to_bytes(4, "big"),
                    (i, sent))
                break
            piece = min(D - 3, rem - 1)
            put(_head(0, 0, 3, 1 + piece) + bytes([fid]) + data[sent:sent + piece], (i, sent))
            if cur:
                close()                                                # at most 4 bytes stay unused
            sent += piece
    det = list(frames)
    if cur and flush:
        det.append((bytes(cur), cur_pos, cur_pk))
    E = len(det) if cap is None else min(int(cap), len(det))
    if E < len(det):
        r_pdu, r_byte = det[E][1]
    elif cur and not flush:
        r_pdu, r_byte = cur_pos
    else:
        r_pdu, r_byte = n_pdus, 0
    bb = np.zeros((E, kbch // 8), np.uint8)
    pad = pk = 0
    for f, (field, _, npk) in enumerate(det[:E]):
        bb[f, :10] = np.frombuffer(header(kbch, sis_mis, isi, len(field)), np.uint8)
        bb[f, 10:10 + len(field)] = np.frombuffer(field, np.uint8)
        pad += D - len(field)
        pk += npk
    before = list(range(s_pdu, r_pdu))
    ks = [kinds[i][0] for i in before]
    nfrag = sum(1 for i in before if i in fragmented)
    c = dict(pdus_in=len(before), complete=ks.count("ok") - nfrag, fragmented=nfrag, gse_packets=pk,
             skipped_len=ks.count("len"), skipped_type=ks.count("type"), bbframes=E, pad_bytes=pad,
             flushed=int(bool(flush) and bool(cur) and E == len(det)))
    return Result(bb.reshape(-1), (r_pdu, r_byte, (s_fid + r_pdu - s_pdu) & 255), c)


def receive(bb, kbch, label_len, sis_mis=1, isi=0, crc=crc32, open_end=False):
    """the BBFRAMEs' PDUs: [(type, label, pdu bytes)].  Raises AssertionError on a header CRC-8 error, a header field
    other than the GSE normal-mode ones, a packet that crosses the data field, a fragment without its predecessor, a
    Frag ID other than the open one, a Total Length or CRC-32 mismatch, or (unless open_end) an end inside a PDU"""
    Lb, D = kbch // 8, (kbch - 80) // 8
    bb = np.asarray(bb, np.uint8).reshape(-1, Lb)
    out = []
    open_ = None    # (frag id, total length, bytes so far: protocol type, label, pdu)
    for f in bb:
        h = bytes(f[:10])
        assert crc8(h[:9]) == h[9], "CRC-8"
        assert h[0] == (0xB0 if sis_mis else 0x90) and h[1] == (0 if sis_mis else isi)
        assert h[2:4] == b"\0\0" and h[6:9] == b"\0\0\0", "UPL, SYNC, SYNCD"
        dfl = (h[4] << 8) | h[5]
        assert dfl % 8 == 0 and dfl // 8 <= D
        field, rest = bytes(f[10:10 + dfl // 8]), bytes(f[10 + dfl // 8:])
        assert not any(rest), "padding"
        pos = 0
        while pos < len(field):
            assert pos + 2 <= len(field)
            S, E, lt = field[pos] >> 7, (field[pos] >> 6) & 1, (field[pos] >> 4) & 3
            glen = ((field[pos] & 15) << 8) | field[pos + 1]
            assert pos + 2 + glen <= len(field), "a packet crosses the data field"
            p = field[pos + 2:pos + 2 + glen]
            pos += 2 + glen
            if S and E:
                assert open_ is None and lt == LT_OF[label_len]
                out.append(((p[0] << 8) | p[1], p[2:2 + label_len], p[2 + label_len:]))
            elif S:
                assert open_ is None and lt == LT_OF[label_len]
                open_ = (p[0], (p[1] << 8) | p[2], bytearray(p[3:]))
            else:
                assert open_ is not None and lt == 3 and p[0] == open_[0], "Frag ID"
                if not E:
                    open_[2].extend(p[1:])
                    continue
                assert len(p) >= 6, "an end fragment carries a PDU byte"
                open_[2].extend(p[1:-4])
                body = bytes(open_[2])
                assert len(body) == open_[1], "Total Length"
                assert crc(open_[1].to_bytes(2, "big") + body) == int.from_bytes(p[-4:], "big"), "CRC-32"
                out.append(((body[0] << 8) | body[1], body[2:2 + label_len], body[2 + label_len:]))
                open_ = None
    assert open_ is None or open_end, "the stream ends inside a PDU"
    return out


def valid_pdus(pdu, off, types=None, label=LABEL, first=0):
    """what receive() must return for the PDUs from first on"""
    out = []
    label = bytes(label or b"")
    for i in range(first, len(off) - 1):
        kind, typ = classify(pdu, off, i, types, len(label))
        if kind == "ok":
            out.append((typ, label, np.asarray(pdu, np.uint8)[int(off[i]):int(off[i + 1])].tobytes()))
    return out
