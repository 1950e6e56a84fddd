"""The TS multiplexer and the PSI builder restated sequentially for the tests of dvbt2ll_tsmux_* and dvbt2ll_psi_build
(include/dvbt2ll_hip.h states the rules):

schedule()  the table: every (due time, owner) pair as a fractions.Fraction, sorted
mux()       the multiplexer: it walks the slots one by one with a running position per input and a running clock; no
            prefix counts, no ranks, no closed forms
psi()       the PAT / PMT carousel, section by section
check_ts()  an independent checker after ISO/IEC 13818-1: per-PID continuity, section reassembly with CRC on the PSI
            PIDs, PAT -> PMT, the PCRs decoded

Nothing here looks at how the GPU code resolves a slot."""
from fractions import Fraction
from typing import NamedTuple

import numpy as np

from mpe_ref import crc32_table as crc32

W = (1 << 33) * 300           # the 27 MHz clock wraps here
NULL = np.array([0x47, 0x1F, 0xFF, 0x10] + [0xFF] * 184, np.uint8)
COUNTERS = ("fill_in_free", "pcr_packets", "null_packets", "sync_errors")


def schedule(period, weight, pcr_weight=0):
    """owner per table slot: input i, len(weight) for the PCR generator, len(weight) + 1 for null"""
    w = list(weight) + [pcr_weight]
    w.append(period - sum(w))
    assert w[-1] >= 0
    pairs = sorted((Fraction(k, w[e]), e) for e in range(len(w)) for k in range(w[e]))
    return np.array([e for _, e in pairs], np.uint8)


def pcr_packet(pid, ticks):
    base, ext = divmod(ticks, 300)
    v = (base << 15) | (0x3F << 9) | ext
    p = np.full(188, 0xFF, np.uint8)
    p[:6] = [0x47, pid >> 8, pid & 255, 0x20, 183, 0x10]
    p[6:12] = list(v.to_bytes(6, "big"))
    return p


class Result(NamedTuple):
    ts: np.ndarray        # uint8, 188 bytes per packet
    resume: tuple         # (phase, pcr_ticks, next: 8 entries)
    counters: dict


def mux(inputs, n_out, period, weight, loop=None, fill_input=-1, pcr_pid=-1, pcr_weight=0, ticks_per_period=0,
        start=(0, 0, (0,) * 8)):
    n = len(weight)
    loop = [0] * n if loop is None else list(loop)
    ins = [np.asarray(x, np.uint8).reshape(-1, 188) for x in inputs]
    table = schedule(period, weight, pcr_weight)
    slot, clock, nxt = int(start[0]), int(start[1]), [int(x) for x in list(start[2])[:n]]
    consumed, dry = [0] * n, [0] * n
    c = dict.fromkeys(COUNTERS, 0)
    out = np.empty((n_out, 188), np.uint8)
    f = fill_input

    def take(i):
        """input i's next packet, or a null packet in its place when its sync byte is bad"""
        if loop[i]:
            pk = ins[i][nxt[i] % len(ins[i])]
            nxt[i] = (nxt[i] % len(ins[i]) + 1) % len(ins[i])
        else:
            pk = ins[i][nxt[i]]
            nxt[i] += 1
        consumed[i] += 1
        if pk[0] != 0x47:
            c["sync_errors"] += 1
            c["null_packets"] += 1
            return NULL
        return pk

    for m in range(n_out):
        e = int(table[slot])
        free = False
        if e == n:
            out[m] = pcr_packet(pcr_pid, (clock + slot * ticks_per_period // period) % W)
            c["pcr_packets"] += 1
        elif e > n or e == f:
            free = True
        elif (len(ins[e]) > 0) if loop[e] else (nxt[e] < len(ins[e])):
            out[m] = take(e)
        else:
            dry[e] += 1
            free = True
        if free:
            if f >= 0 and nxt[f] < len(ins[f]):
                out[m] = take(f)
                c["fill_in_free"] += e != f
            else:
                out[m] = NULL
                c["null_packets"] += 1
                if e == f:
                    dry[f] += 1
        slot += 1
        if slot == period:
            slot = 0
            clock = (clock + ticks_per_period) % W
    nxt = [x % len(ins[i]) if loop[i] and len(ins[i]) else x for i, x in enumerate(nxt)]
    c["consumed"], c["dry_slots"] = tuple(consumed), tuple(dry)
    return Result(out.reshape(-1), (slot, clock, tuple(nxt) + (0,) * (8 - n)), c)


# ---------------------------------------------------------------------------------------- PSI
def _section(head, body):
    n = len(head) - 3 + len(body) + 4
    s = bytes([head[0], 0xB0 | (n >> 8), n & 255]) + bytes(head[3:]) + bytes(body)
    return s + crc32(s).to_bytes(4, "big")


def pat_section(tsid, version, programs):
    body = b"".join(bytes([g["program_number"] >> 8, g["program_number"] & 255, 0xE0 | (g["pmt_pid"] >> 8),
                           g["pmt_pid"] & 255]) for g in programs)
    return _section([0x00, 0, 0, tsid >> 8, tsid & 255, 0xC1 | (version << 1), 0, 0], body)


def pmt_section(version, g):
    pcr = g.get("pcr_pid", 0x1FFF)
    body = bytes([0xE0 | (pcr >> 8), pcr & 255, 0xF0, 0x00])
    for e in g.get("streams", []):
        d = bytes(e.get("descriptors", b""))
        body += bytes([e["stream_type"], 0xE0 | (e["pid"] >> 8), e["pid"] & 255, 0xF0 | (len(d) >> 8), len(d) & 255]) + d
    return _section([0x02, 0, 0, g["program_number"] >> 8, g["program_number"] & 255, 0xC1 | (version << 1), 0, 0], body)


def psi(tsid, version, programs, rounds=16):
    """the carousel: per round the PAT, then every programme's PMT; a counter per PID runs on across the rounds"""
    secs = [(0, pat_section(tsid, version, programs))] + [(g["pmt_pid"], pmt_section(version, g)) for g in programs]
    cc = {}
    out = []
    for _ in range(rounds):
        for pid, s in secs:
            data = b"\0" + s
            for k in range(0, len(data), 184):
                p = np.full(188, 0xFF, np.uint8)
                p[:4] = [0x47, (0x40 if k == 0 else 0) | (pid >> 8), pid & 255, 0x10 | cc.get(pid, 0)]
                cc[pid] = (cc.get(pid, 0) + 1) & 15
                chunk = data[k:k + 184]
                p[4:4 + len(chunk)] = np.frombuffer(chunk, np.uint8)
                out.append(p)
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------- the checker
def _sections(ts, pid):
    """the sections on pid, reassembled after 2.4.4: PUSI / pointer_field, section_length, FF stuffing; every CRC is
    checked.  A section still open at the end is dropped"""
    out, buf = [], None
    for p in ts:
        if (((int(p[1]) & 0x1F) << 8) | int(p[2])) != pid or not (p[3] & 0x10):
            continue
        assert (p[3] >> 4) == 1, "PSI packets carry no adaptation field here"
        pay = bytes(p[4:])
        segs = []
        if p[1] & 0x40:
            ptr = pay[0]
            assert ptr <= 182
            segs = [(pay[1:1 + ptr], False), (pay[1 + ptr:], True)]
        elif buf is not None:
            segs = [(pay, False)]
        for seg, may_start in segs:
            pos = 0
            while pos < len(seg):
                if buf is None:
                    if not may_start:     # the tail of a section that began before the stream did
                        break
                    if seg[pos] == 0xFF:
                        assert not seg[pos:].strip(b"\xff"), "stuffing"
                        break
                    buf = bytearray()
                need = 3 - len(buf) if len(buf) < 3 else 3 + (((buf[1] & 15) << 8) | buf[2]) - len(buf)
                take = min(need, len(seg) - pos)
                buf += seg[pos:pos + take]
                pos += take
                if len(buf) >= 3 and len(buf) == 3 + (((buf[1] & 15) << 8) | buf[2]):
                    assert crc32(bytes(buf)) == 0, "CRC of a section on PID %#x" % pid
                    out.append(bytes(buf))
                    buf = None
            assert may_start or buf is None or not p[1] & 0x40, "the pointer_field contradicts the section in progress"
    return out


def parse_pat(s):
    assert s[0] == 0x00 and s[1] >> 4 == 0xB and s[5] & 1 and s[6] == 0 and s[7] == 0
    body = s[8:-4]
    assert len(body) % 4 == 0
    return dict(tsid=(s[3] << 8) | s[4], version=(s[5] >> 1) & 31,
                programs=[((body[k] << 8) | body[k + 1], ((body[k + 2] & 0x1F) << 8) | body[k + 3])
                          for k in range(0, len(body), 4)])


def parse_pmt(s):
    assert s[0] == 0x02 and s[1] >> 4 == 0xB and s[5] & 1 and s[6] == 0 and s[7] == 0
    pil = ((s[10] & 15) << 8) | s[11]
    body = s[12 + pil:-4]
    streams, k = [], 0
    while k < len(body):
        n = ((body[k + 3] & 15) << 8) | body[k + 4]
        streams.append((body[k], ((body[k + 1] & 0x1F) << 8) | body[k + 2], bytes(body[k + 5:k + 5 + n])))
        k += 5 + n
    assert k == len(body)
    return dict(program_number=(s[3] << 8) | s[4], version=(s[5] >> 1) & 31, pcr_pid=((s[8] & 0x1F) << 8) | s[9],
                streams=streams)


def check_ts(ts, cc=None):
    """parses a TS: sync bytes; per PID the continuity of the packets with a payload (cc: {pid: the counter expected
    first}); the PAT on PID 0 and the PMTs it names, every section's CRC; the PCRs.  Returns dict(pat, pmts: {program
    number: parsed PMT}, pids: {pid: packets}, pcrs: [(packet index, pid, 27 MHz ticks)], cc: the counters expected next)"""
    ts = np.asarray(ts, np.uint8).reshape(-1, 188)
    cc = dict(cc or {})
    pids, pcrs = {}, []
    for k, p in enumerate(ts):
        assert p[0] == 0x47 and not p[1] & 0x80, "sync / transport_error at packet %d" % k
        pid = ((int(p[1]) & 0x1F) << 8) | int(p[2])
        pids[pid] = pids.get(pid, 0) + 1
        if pid == 0x1FFF:
            continue
        afc = (p[3] >> 4) & 3
        assert afc in (1, 2, 3)
        if afc & 1:
            if pid in cc:
                assert (p[3] & 15) == cc[pid], "continuity on PID %#x at packet %d" % (pid, k)
            cc[pid] = ((p[3] & 15) + 1) & 15
        if afc & 2 and p[4] >= 7 and p[5] & 0x10:
            v = int.from_bytes(bytes(p[6:12]), "big")
            assert (v >> 9) & 0x3F == 0x3F and (v & 0x1FF) < 300
            pcrs.append((k, pid, (v >> 15) * 300 + (v & 0x1FF)))
    res = dict(pat=None, pmts={}, pids=pids, pcrs=pcrs, cc=cc)
    pats = _sections(ts, 0)
    if pats:
        assert all(s == pats[0] for s in pats)
        res["pat"] = parse_pat(pats[0])
        for number, pmt_pid in res["pat"]["programs"]:
            secs = _sections(ts, pmt_pid)
            if secs:
                assert all(s == secs[0] for s in secs)
                res["pmts"][number] = parse_pmt(secs[0])
                assert res["pmts"][number]["program_number"] == number
    return res
