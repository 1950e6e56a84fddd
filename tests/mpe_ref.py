"""MPE (EN 301 192 clause 7: IP datagrams in DSM-CC datagram_sections) restated sequentially for the tests of
dvbt2ll_mpe_* (include/dvbt2ll_hip.h states the rules):

encap()    the encapsulator: one section at a time, one packet buffer, a plain loop; its CRC is bitwise
receive()  an independent section receiver after ISO/IEC 13818-1 (2.4.4.1 pointer_field, 2.4.4.11 private_section,
           Annex A CRC): it follows PUSI / pointer_field and the continuity counter, takes table_id FF as stuffing to
           the packet's end, reassembles by section_length and requires the CRC over the whole section to be 0; it
           returns (mac, datagram) per section

Nothing here looks at the GPU code's passes: no scan, no state maps, no search."""
from typing import NamedTuple

import numpy as np

POLY = 0x04C11DB7
MAC = bytes([0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B])
MAX_PDU = 4080
COUNTERS = ("pdus_in", "sections", "skipped_len", "skipped_type", "mapped_macs", "ts_packets", "pusi_packets",
            "pad_bytes", "flushed")


def crc32(data, crc=0xFFFFFFFF):
    """CRC-32 of generator 0x04C11DB7, initial value 0xFFFFFFFF, no reflection, no final XOR: bit by bit"""
    for b in bytes(data):
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ POLY) & 0xFFFFFFFF if crc & 0x80000000 else (crc << 1) & 0xFFFFFFFF
    return crc


_TAB = None


def crc32_table(data, crc=0xFFFFFFFF):
    """the same CRC through a byte table (for the large cases; tests/test_cpu_mpe.py proves it equal to crc32)"""
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
    resume: tuple         # (pdu, section_byte, cc)
    counters: dict


def pack(pdus):
    """a list of byte strings -> (the PDU buffer, the offset table)"""
    off = np.zeros(len(pdus) + 1, np.uint32)
    off[1:] = np.cumsum([len(p) for p in pdus])
    return np.frombuffer(b"".join(bytes(p) for p in pdus), np.uint8).copy(), off


def classify(pdu, off, i):
    """PDU i: "ok", "len" or "type"; the length is judged first"""
    o0, o1 = int(off[i]), int(off[i + 1])
    if o1 <= o0 or o1 > len(pdu) or o1 - o0 > MAX_PDU:
        return "len"
    return "ok" if int(pdu[o0]) >> 4 in (4, 6) else "type"


def mac_of(data, mac=MAC, mac_mode=0):
    """(the section's MAC, whether it came from the datagram's multicast destination)"""
    if mac_mode:
        if data[0] >> 4 == 4 and len(data) >= 20 and 224 <= data[16] <= 239:
            return bytes([0x01, 0x00, 0x5E, data[17] & 0x7F, data[18], data[19]]), True
        if data[0] >> 4 == 6 and len(data) >= 40 and data[24] == 0xFF:
            return bytes([0x33, 0x33]) + bytes(data[36:40]), True
    return bytes(mac), False


def section(data, mac, crc=crc32):
    """the datagram_section of one datagram: table_id 3E, section_syntax_indicator 1, no LLC/SNAP, section 0 of 0"""
    n = 12 + len(data) + 4
    sl = n - 3
    s = bytes([0x3E, 0xB0 | (sl >> 8), sl & 255, mac[5], mac[4], 0xC1, 0, 0, mac[3], mac[2], mac[1], mac[0]])
    s += bytes(data)
    return s + crc(s).to_bytes(4, "big")


def encap(pdu, off, pid=0x100, mac=MAC, mac_mode=0, packing=1, start=(0, 0, 0), cap=None, flush=False, crc=crc32):
    pdu = np.asarray(pdu, np.uint8)
    n_pdus = len(off) - 1
    s_pdu, s_byte, s_cc = (int(x) for x in start)
    kinds = {i: classify(pdu, off, i) for i in range(s_pdu, n_pdus)}
    valid = [i for i in range(s_pdu, n_pdus) if kinds[i] == "ok"]
    mapped = {}
    pkts = []       # (PUSI, the payload bytes before the FF fill, the position (pdu, section_byte) the packet begins at)
    cur = None      # the open PUSI packet: its payload so far, pointer_field included; cur_pos: where it begins
    cur_pos = None
    left = None     # the position of what stays behind when the end is reached without a flush
    for idx, i in enumerate(valid):
        data = pdu[int(off[i]):int(off[i + 1])].tobytes()
        m, mapped[i] = mac_of(data, mac, mac_mode)
        S = section(data, m, crc)
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
        if k == 0:      # a new section: behind the open packet's bytes (one free byte is enough), or behind pointer 0
            if cur is None:
                cur, cur_pos = bytearray([0]), (i, 0)
            take = min(184 - len(cur), len(S))
            cur += S[:take]
            k = take
        while True:
            if cur is not None:
                if len(cur) == 184:         # full: closed
                    pkts.append((1, bytes(cur), cur_pos))
                    cur = None
                elif k == len(S):           # the section ended with free bytes
                    if not nxt:
                        if flush:
                            pkts.append((1, bytes(cur), cur_pos))
                        else:
                            left = cur_pos
                        cur = None
                    break
            if k == len(S):
                break
            R = len(S) - k                  # a packet begins inside the section
            if R >= 183:                    # 184, or 183 and FF: no pointer could point inside the packet
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
    before = [kinds[i] for i in range(s_pdu, r_pdu)]
    c = dict(pdus_in=len(before), sections=before.count("ok"), skipped_len=before.count("len"),
             skipped_type=before.count("type"), mapped_macs=sum(1 for i in range(s_pdu, r_pdu) if mapped.get(i)),
             ts_packets=E, pusi_packets=pusi, pad_bytes=pad, flushed=int(bool(flush) and r_pdu == n_pdus))
    return Result(ts.reshape(-1), (r_pdu, r_byte, (s_cc + E) & 15), c)


def receive(ts, pid=0x100, cc=None, crc=crc32, open_end=False):
    """ISO/IEC 13818-1 section reassembly on the packets of pid: [(mac, datagram)].  Raises AssertionError on a
    continuity error, a pointer_field that contradicts the section in progress or points outside the packet, a section
    that starts where none may, a CRC error, a section that is no datagram_section of the form built here, or (unless
    open_end) a stream that ends inside a section; the encapsulator's output has none"""
    ts = np.asarray(ts, np.uint8).reshape(-1, 188)
    out = []
    buf = None      # the section in progress; its length is known once three bytes are in

    def feed(seg, may_start):
        """a run of payload bytes; returns after the packet's stuffing began"""
        nonlocal buf
        pos = 0
        while pos < len(seg):
            if buf is None:
                if seg[pos] == 0xFF:        # table_id FF: stuffing to the end of the packet
                    assert all(b == 0xFF for b in seg[pos:]), "stuffing"
                    return
                assert may_start, "a section starts where no pointer_field points"
                buf = bytearray()
            if len(buf) < 3:
                take = min(3 - len(buf), len(seg) - pos)
            else:
                take = min(3 + (((buf[1] & 15) << 8) | buf[2]) - len(buf), len(seg) - pos)
            buf += seg[pos:pos + take]
            pos += take
            if len(buf) >= 3 and len(buf) == 3 + (((buf[1] & 15) << 8) | buf[2]):
                s = bytes(buf)
                buf = None
                assert len(s) <= 4096 and crc(s) == 0, "CRC"
                assert s[0] == 0x3E and s[1] >> 4 == 0xB and s[5] == 0xC1 and s[6] == 0 and s[7] == 0
                out.append((bytes([s[11], s[10], s[9], s[8], s[4], s[3]]), s[12:-4]))

    for p in ts:
        assert p[0] == 0x47 and not p[1] & 0x80
        if (((int(p[1]) & 0x1F) << 8) | int(p[2])) != pid:
            continue
        assert p[3] >> 4 == 1, "adaptation field control"
        if cc is not None:
            assert (p[3] & 15) == cc, "continuity"
        cc = ((p[3] & 15) + 1) & 15
        pay = bytes(p[4:])
        if p[1] & 0x40:
            ptr = pay[0]
            assert ptr <= 182, "pointer_field points outside the packet"
            if buf is not None:             # the section in progress ends exactly where the pointer points
                feed(pay[1:1 + ptr], False)
                assert buf is None, "the pointer_field contradicts the section in progress"
            feed(pay[1 + ptr:], True)
        elif buf is not None:
            feed(pay, False)
    assert buf is None or open_end, "the stream ends inside a section"
    return out


def valid_pdus(pdu, off, mac=MAC, mac_mode=0, first=0):
    """what receive() must return for the PDUs from first on"""
    out = []
    for i in range(first, len(off) - 1):
        if classify(pdu, off, i) == "ok":
            data = np.asarray(pdu, np.uint8)[int(off[i]):int(off[i + 1])].tobytes()
            out.append((mac_of(data, mac, mac_mode)[0], data))
    return out
