"""Mode adaptation with null-packet deletion (dvbt2ll_modeadapt_*, include/dvbt2ll_hip.h; EN 302 755 5.1.4, 5.1.7):
a sequential restatement that the GPU adapter is compared with byte for byte, and an independent receiver.

  * adapt: walks the TS packet by packet with a running DNP counter and a byte FIFO, cuts the FIFO into data
    fields and writes the high-efficiency-mode BBHEADERs.  No scans, no compaction: nothing of the kernels'
    formulation;
  * receive: parses BBFRAMEs by DFL and SYNCD alone, cuts the user packets, reinserts the deleted null packets and
    restores the sync byte.  receive(adapt(ts)) must be filtered(ts): the TS with every unselected packet replaced
    by the null packet.

The reference sets NPD = 0 (bbheader:272-325): npd = 1 is PARITY UNPINNED and pinned here; npd = 0 is pinned to the
oracle's HEM BBFRAMEs by tests/test_cpu_modeadapt.py.
"""
from dataclasses import dataclass, field

import numpy as np

NULL_PID = 0x1FFF
NULL_PACKET = np.array([0x47, 0x1F, 0xFF, 0x10] + [0xFF] * 184, np.uint8)
COUNTERS = ("packets_in", "selected", "nulls_deleted", "nulls_kept", "nulls_dropped_at_flush", "sync_errors",
            "bbframes", "flushed")


def crc8(data):
    """CRC-8 of DVB-S2 / T2 (generator x^8 + x^7 + x^6 + x^4 + x^2 + 1 = 0xD5), MSB first, zero start, bit by bit"""
    r = 0
    for b in bytes(bytearray(data)):
        for n in range(7, -1, -1):
            fb = ((r >> 7) ^ (b >> n)) & 1
            r = (r << 1) & 0xFF
            if fb:
                r ^= 0xD5
    return r


def pid_of(pkt):
    return ((int(pkt[1]) & 0x1F) << 8) | int(pkt[2])


def mask_of(pids):
    """the 1024-byte selection mask of a PID list: PID p is bit p & 7 of byte p >> 3"""
    m = np.zeros(1024, np.uint8)
    for p in pids:
        m[p >> 3] |= 1 << (p & 7)
    return m


def selected(pkt, npd, mask):
    if not npd:
        return True
    p = pid_of(pkt)
    if p == NULL_PID:
        return False
    return True if mask is None else bool((int(mask[p >> 3]) >> (p & 7)) & 1)


def filtered(ts, npd=1, mask=None):
    """the TS a receiver restores: every unselected packet replaced by the null packet, every sync byte 0x47"""
    out = np.array(ts, np.uint8).reshape(-1, 188).copy()
    for row in out:
        if not selected(row, npd, mask):
            row[:] = NULL_PACKET
        row[0] = 0x47
    return out.reshape(-1)


def header(D_bits, dfl_bits, syncd_bits, npd, sis=True, isi=0):
    """the 10 BBHEADER bytes in high-efficiency mode: MATYPE (TS, SIS/MIS, CCM, ISSYI 0, NPD, EXT 0; ISI), UPL 0,
    DFL, SYNC 0, SYNCD, CRC-8 XOR MODE (1)"""
    h = [0xC0 | (0x20 if sis else 0) | 0x10 | (4 if npd else 0), 0 if sis else isi, 0, 0, dfl_bits >> 8,
         dfl_bits & 255, 0, syncd_bits >> 8, syncd_bits & 255]
    return h + [crc8(h) ^ 1]


@dataclass
class Result:
    bbframes: np.ndarray
    resume: tuple
    counters: dict = field(default_factory=dict)


def adapt(ts, kbch, npd=1, mask=None, sis=True, isi=0, start=(0, 0, 0), cap=None, flush=False):
    """one call of the adapter on the whole packets of ts from start = (ts_packet, unit_byte, dnp); cap: output
    capacity in BBFRAMEs (None: unbounded)"""
    rows = np.asarray(ts, np.uint8).reshape(-1, 188)
    n = len(rows)
    s0, ub0, dnp0 = start
    D, L, U = (kbch - 80) // 8, kbch // 8, 188 if npd else 187
    fifo = bytearray()
    units = []            # (offset of the unit's byte 0 in the FIFO, packet index, DNP)
    kind = {}             # packet index -> "sel" / "kept" / "del"
    dnp = 0               # nulls deleted since the last transmitted packet
    for i in range(s0, n):
        pkt = rows[i]
        sel = selected(pkt, npd, mask)
        forced = i == s0 and (ub0 > 0 or dnp0 > 0)
        if forced:
            dnp = dnp0
        elif not sel and dnp < 255:
            dnp += 1
            kind[i] = "del"
            continue
        # transmitted: a selected packet, or the null after 255 deleted ones (sent as the null packet)
        kind[i] = "sel" if sel else "kept"
        body = (pkt if sel else NULL_PACKET)[1:].tobytes() + (bytes([dnp]) if npd else b"")
        skip = ub0 if i == s0 else 0
        units.append((len(fifo) - skip, i, dnp))
        fifo += body[skip:]
        dnp = 0
    whole, rem = divmod(len(fifo), D)
    cap = whole + 1 if cap is None else cap
    flushed = bool(flush) and whole + (1 if rem else 0) <= cap
    nfr = min(whole, cap)
    emitted = len(fifo) if flushed else nfr * D
    out = bytearray()
    starts = [u[0] for u in units if u[0] >= 0]
    for k in range(nfr + (1 if flushed and rem else 0)):
        nbytes = min(D, len(fifo) - k * D)
        first = [x for x in starts if k * D <= x < k * D + nbytes]
        syncd = 8 * (first[0] - k * D) if first else 0xFFFF
        out += bytes(header(8 * D, 8 * nbytes, syncd, npd, sis, isi)) + fifo[k * D:k * D + nbytes] + bytes(D - nbytes)
    # resume: the unit holding the first byte not emitted
    if flushed:
        resume = (n, 0, 0)
    else:
        resume = None
        for off, i, d in units:
            if off + U > emitted:
                resume = (i, emitted - off, d)
                break
        if resume is None:
            resume = (units[-1][1] + 1 if units else s0, 0, 0)
    last_tx = units[-1][1] if units else s0 - 1
    c = dict.fromkeys(COUNTERS, 0)
    for i in range(s0, resume[0]):
        c["packets_in"] += 1
        c["sync_errors"] += int(rows[i][0] != 0x47)
        if kind[i] == "sel":
            c["selected"] += 1
        elif kind[i] == "kept":
            c["nulls_kept"] += 1
        elif flushed and i > last_tx:
            c["nulls_dropped_at_flush"] += 1
        else:
            c["nulls_deleted"] += 1
    c["bbframes"] = len(out) // L
    c["flushed"] = int(flushed and rem > 0)
    return Result(np.frombuffer(bytes(out), np.uint8), resume, c)


def adapt_chunked(ts, kbch, cuts, flush=True, caps=None, **kw):
    """the calls of a caller that receives the TS in pieces ending at packet indices cuts (then the whole): each
    call's buffer is the stream from the previous resume packet to the piece's end; returns (bytes, summed counters,
    the last resume in whole-stream packet indices)"""
    rows = np.asarray(ts, np.uint8).reshape(-1, 188)
    ends = list(cuts) + [len(rows)]
    base, pos, out, tot = 0, (0, 0, 0), [], dict.fromkeys(COUNTERS, 0)
    for j, end in enumerate(ends):
        end = max(end, base)
        last = j == len(ends) - 1
        r = adapt(rows[base:end].reshape(-1), kbch, start=pos, flush=flush and last,
                  cap=None if caps is None else caps[j], **kw)
        out.append(r.bbframes)
        for key in COUNTERS:
            tot[key] += r.counters[key]
        base += r.resume[0]
        pos = (0, r.resume[1], r.resume[2])
    return np.concatenate(out), tot, (base, pos[1], pos[2])


def receive(bbframes, kbch):
    """BBFRAMEs -> the TS: units cut by DFL and SYNCD, DNP null packets before each, sync bytes restored.  Checks
    each header's CRC-8 / MODE, UPL, SYNC and that SYNCD points where the running unit ends"""
    L = kbch // 8
    frames = np.asarray(bbframes, np.uint8).reshape(-1, L)
    out, pending, U = [], bytearray(), None

    def emit(unit):
        if unit:
            out.extend([NULL_PACKET] * (unit[187] if len(unit) == 188 else 0))
            out.append(np.frombuffer(b"\x47" + bytes(unit[:187]), np.uint8))

    for f in frames:
        assert f[0] & 0xC0 == 0xC0 and f[0] & 0x10 and not f[0] & 0x0B, "MATYPE-1 %02x" % f[0]
        assert crc8(f[:9]) ^ 1 == f[9], "CRC-8 XOR MODE"
        assert not f[2] and not f[3] and not f[6], "UPL / SYNC are zero in high-efficiency mode"
        npd = (int(f[0]) >> 2) & 1
        U = 188 if npd else 187
        dfl, syncd = (int(f[4]) << 8) | int(f[5]), (int(f[7]) << 8) | int(f[8])
        assert dfl % 8 == 0 and dfl <= kbch - 80
        data = f[10:10 + dfl // 8].tobytes()
        assert not f[10 + dfl // 8:].any(), "padding is zero"
        if syncd == 0xFFFF:      # no unit begins here: the data field continues the running unit
            assert pending and len(pending) + len(data) <= U
            pending += data
        else:                    # the running unit ends SYNCD bits in; a new one begins there
            assert syncd % 8 == 0 and syncd // 8 < len(data)
            pending += data[:syncd // 8]
            assert len(pending) in (0, U), "SYNCD %d leaves a unit of %d bytes" % (syncd, len(pending))
            emit(pending)
            pending = bytearray(data[syncd // 8:])
        while len(pending) >= U:
            emit(pending[:U])
            pending = pending[U:]
    assert not pending, "%d bytes of a cut unit at the end" % len(pending)
    return np.concatenate(out) if out else np.zeros(0, np.uint8)
