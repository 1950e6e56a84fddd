"""TS multiplexer (dvbt2ll_tsmux_* in include/dvbt2ll_hip.h): up to 8 device buffers of TS packets -- the output of a
ULE / MPE / MPE-FEC encapsulator, a PSI carousel, any TS -- merged on the GPU into one constant-bit-rate TS, with null
packets where nothing is due and PCR packets if asked for; and psi_build (dvbt2ll_psi_build): the PAT / PMT carousel
that lets a receiver find the streams.

PARITY UNPINNED (the reference has no multiplexer): pinned to tests/tsmux_ref.py's sequential restatement and its TS
checker.

Example: an encapsulator's device output and a PSI carousel -> one TS, everything on torch's stream

    psi = dvbt2ll.psi_build(1, 0, [dict(program_number=1, pmt_pid=0x1000, streams=[dict(stream_type=0x0D, pid=0x100)])])
    mux = dvbt2ll.TsMux(period=20, weight=[18, 1], loop=[0, 1], fill_input=0, max_out_packets=n_out)
    mux.run_device([ts_d.data_ptr(), psi_d.data_ptr()], [n_ts, len(psi) // 188], out_d.data_ptr(), n_out, stream=st)
    res = mux.result()                     # synchronises: counters, resume position
"""
import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import (lib, check, DVBT2Error, _TsMuxParams, _TsMuxPos, _TsMuxResult, _PsiParams, TSMUX_INPUTS,
                   PSI_DESCRIPTOR_BYTES, _TsMuxRemux, _TsMuxRemuxPos, _TsMuxRemuxResult, TSMUX_MAP, TSMUX_TRACK)

COUNTERS = ("fill_in_free", "pcr_packets", "null_packets", "sync_errors")
REMUX_COUNTERS = ("remapped", "dropped", "cc_rewritten", "pcr_restamped")
PCR_WRAP = (1 << 33) * 300


class TsMuxPos(NamedTuple):
    """a position: the table slot of the next output packet, the 27 MHz clock at the start of that slot's period, each
    input's next packet in the buffer passed"""
    phase: int = 0
    pcr_ticks: int = 0
    next: tuple = (0,) * TSMUX_INPUTS


class TsRemuxPos(NamedTuple):
    """a remux position: cc[s], the counter the next payload packet restamped on tracked PID s takes; in_phase[i] and
    in_ticks[i], where input i's next packet lies in the input's own period and the input's 27 MHz clock at the start
    of that period"""
    cc: tuple = (0,) * TSMUX_TRACK
    in_phase: tuple = (0,) * TSMUX_INPUTS
    in_ticks: tuple = (0,) * TSMUX_INPUTS


@dataclass
class TsRemuxResult:
    """one call's remux result: resume (TsRemuxPos); counters (dict: remapped, dropped, cc_rewritten, pcr_restamped)"""
    resume: TsRemuxPos
    counters: dict


@dataclass
class TsMuxResult:
    """one call's result: resume (TsMuxPos); counters (dict: consumed and dry_slots are tuples per input); ts (uint8
    array; host runs only)"""
    resume: TsMuxPos
    counters: dict
    ts: np.ndarray = None
    remux: TsRemuxResult = None


def ticks_per_period(period, ts_bits_per_second):
    """27 MHz ticks that period slots of a TS of that rate last (dvbt2ll_tsmux_ticks_per_period)"""
    v = lib().dvbt2ll_tsmux_ticks_per_period(int(period), int(ts_bits_per_second))
    if v < 0:
        raise DVBT2Error("ticks_per_period: period outside 1 .. 65536 or a rate that is not positive")
    return int(v)


def _pos(start, n):
    pos = _TsMuxPos()
    pos.phase, pos.pcr_ticks = int(start[0]), int(start[1])
    for i, v in enumerate(list(start[2])[:n]):
        pos.next[i] = int(v)
    return pos


def _padded(v, n):
    v = [int(x) for x in v]
    return v + [0] * (n - len(v))


def remux_params(map=(), track_pid=(), restamp_cc=(), in_period=(), in_ticks_per_period=(), out_ticks_per_period=0):
    """the dvbt2ll_tsmux_remux of: map, (input, from_pid, to_pid) triples (to_pid 0x1FFF drops); track_pid, the output
    PIDs whose continuity counters are kept; restamp_cc, 0 / 1 per input; in_period / in_ticks_per_period per input (0:
    its PCRs pass unchanged); out_ticks_per_period, the mux clock of a handle without a PCR PID"""
    x = _TsMuxRemux()
    if len(map) > TSMUX_MAP or len(track_pid) > TSMUX_TRACK:
        raise ValueError("at most %d map entries and %d tracked PIDs" % (TSMUX_MAP, TSMUX_TRACK))
    x.n_map, x.n_track = len(map), len(track_pid)
    for a, (i, f, t) in enumerate(map):
        x.map[a].input, x.map[a].from_pid, x.map[a].to_pid = int(i), int(f), int(t)
    x.track_pid[:len(track_pid)] = [int(v) for v in track_pid]
    x.restamp_cc[:] = _padded(restamp_cc, TSMUX_INPUTS)
    x.in_period[:] = _padded(in_period, TSMUX_INPUTS)
    x.in_ticks_per_period[:] = _padded(in_ticks_per_period, TSMUX_INPUTS)
    x.out_ticks_per_period = int(out_ticks_per_period)
    return x


def _rpos(rstart):
    pos = _TsMuxRemuxPos()
    pos.cc[:] = _padded(rstart[0], TSMUX_TRACK)
    pos.in_phase[:] = _padded(rstart[1], TSMUX_INPUTS)
    pos.in_ticks[:] = _padded(rstart[2], TSMUX_INPUTS)
    return pos


class TsMux:
    def __init__(self, period, weight, loop=None, fill_input=-1, pcr_pid=-1, pcr_weight=0, ticks_per_period=0,
                 max_out_packets=1 << 16, device=0):
        """weight[i]: input i's slots per period; loop[i]: its buffer is a carousel; fill_input: the input that also
        takes the free slots; pcr_pid / pcr_weight / ticks_per_period: PCR packets per period on that PID, stamped from
        a 27 MHz clock that advances ticks_per_period per period"""
        n = len(weight)
        if not 1 <= n <= TSMUX_INPUTS:
            raise ValueError("1 .. %d inputs" % TSMUX_INPUTS)
        loop = [0] * n if loop is None else list(loop)
        if len(loop) != n:
            raise ValueError("loop has one entry per input")
        p = _TsMuxParams()
        p.n_inputs, p.period, p.fill_input = n, int(period), int(fill_input)
        for i in range(n):
            p.weight[i], p.loop[i] = int(weight[i]), int(loop[i])
        p.pcr_pid, p.pcr_weight, p.ticks_per_period = int(pcr_pid), int(pcr_weight), int(ticks_per_period)
        p.max_out_packets = int(max_out_packets)
        self._h = None
        self._p = p
        self.n_inputs, self.period = n, p.period
        h = ctypes.c_void_p()
        check(lib().dvbt2ll_tsmux_create(ctypes.byref(p), int(device), ctypes.byref(h)), "tsmux create")
        self._h = h

    def schedule(self):
        """the schedule table: period owner indices (input i; n_inputs: the PCR generator; n_inputs + 1: null)"""
        owner = np.zeros(self.period, np.uint8)
        check(lib().dvbt2ll_tsmux_schedule(ctypes.byref(self._p), owner.ctypes.data_as(ctypes.c_void_p)),
              "tsmux schedule")
        return owner

    def _args(self, ptrs, n_in):
        if len(ptrs) != self.n_inputs or len(n_in) != self.n_inputs:
            raise ValueError("one buffer and one packet count per input")
        a = (ctypes.c_void_p * TSMUX_INPUTS)(*[ctypes.c_void_p(int(x) or None) for x in ptrs])
        c = (ctypes.c_int64 * TSMUX_INPUTS)(*[int(x) for x in n_in])
        return a, c

    def run_device(self, in_ptrs, n_in, out_ptr, n_out, start=TsMuxPos(), stream=0):
        """asynchronous on stream: input i's n_in[i] packets at device pointer in_ptrs[i] -> exactly n_out packets at
        out_ptr"""
        a, c = self._args(in_ptrs, n_in)
        pos = _pos(start, self.n_inputs)
        check(lib().dvbt2ll_tsmux_run_device(self._h, a, c, ctypes.byref(pos), ctypes.c_void_p(out_ptr), int(n_out),
                                             ctypes.c_void_p(stream or None)), "tsmux run")

    def _result(self, raw):
        n = self.n_inputs
        c = {k: int(getattr(raw, k)) for k in COUNTERS}
        c["consumed"] = tuple(int(raw.consumed[i]) for i in range(n))
        c["dry_slots"] = tuple(int(raw.dry_slots[i]) for i in range(n))
        nxt = tuple(int(raw.resume.next[i]) for i in range(n)) + (0,) * (TSMUX_INPUTS - n)
        return TsMuxResult(TsMuxPos(int(raw.resume.phase), int(raw.resume.pcr_ticks), nxt), c)

    def result(self):
        """synchronises with the last run: its TsMuxResult (the packets stay on the device)"""
        raw = _TsMuxResult()
        check(lib().dvbt2ll_tsmux_get_result(self._h, ctypes.byref(raw)), "tsmux result")
        return self._result(raw)

    def run_host(self, inputs, n_out, start=TsMuxPos()):
        """host convenience (dvbt2ll_tsmux_run_host): inputs are uint8 arrays of whole packets"""
        arrs = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in inputs]
        a, c = self._args([x.ctypes.data if len(x) else 0 for x in arrs], [len(x) // 188 for x in arrs])
        out = np.zeros(max(1, int(n_out)) * 188, np.uint8)
        raw = _TsMuxResult()
        pos = _pos(start, self.n_inputs)
        check(lib().dvbt2ll_tsmux_run_host(self._h, a, c, ctypes.byref(pos), out.ctypes.data_as(ctypes.c_void_p),
                                           int(n_out), ctypes.byref(raw)), "tsmux run host")
        res = self._result(raw)
        res.ts = out[:int(n_out) * 188]
        return res

    # ------------------------------------------------------------------ remux (dvbt2ll_tsmux_*_remux)
    def set_remux(self, map=(), track_pid=(), restamp_cc=(), in_period=(), in_ticks_per_period=(),
                  out_ticks_per_period=0):
        """once, before the first run: PID remapping, continuity restamping on the tracked PIDs and PCR restamping (see
        remux_params).  The handle is then run with run_device_remux / run_host_remux; the plain calls refuse it"""
        x = remux_params(map, track_pid, restamp_cc, in_period, in_ticks_per_period, out_ticks_per_period)
        check(lib().dvbt2ll_tsmux_set_remux(self._h, ctypes.byref(x)), "tsmux set_remux")

    def run_device_remux(self, in_ptrs, n_in, out_ptr, n_out, start=TsMuxPos(), rstart=TsRemuxPos(), stream=0):
        """run_device on a handle with a remux, from the two positions"""
        a, c = self._args(in_ptrs, n_in)
        pos, rpos = _pos(start, self.n_inputs), _rpos(rstart)
        check(lib().dvbt2ll_tsmux_run_device_remux(self._h, a, c, ctypes.byref(pos), ctypes.byref(rpos),
                                                   ctypes.c_void_p(out_ptr), int(n_out),
                                                   ctypes.c_void_p(stream or None)), "tsmux run remux")

    @staticmethod
    def _remux_result(raw):
        pos = TsRemuxPos(tuple(int(v) for v in raw.resume.cc), tuple(int(v) for v in raw.resume.in_phase),
                         tuple(int(v) for v in raw.resume.in_ticks))
        return TsRemuxResult(pos, {k: int(getattr(raw, k)) for k in REMUX_COUNTERS})

    def remux_result(self):
        """synchronises with the last run: its TsRemuxResult (result() returns the multiplexer's own)"""
        raw = _TsMuxRemuxResult()
        check(lib().dvbt2ll_tsmux_get_remux_result(self._h, ctypes.byref(raw)), "tsmux remux result")
        return self._remux_result(raw)

    def run_host_remux(self, inputs, n_out, start=TsMuxPos(), rstart=TsRemuxPos()):
        """host convenience (dvbt2ll_tsmux_run_host_remux): a TsMuxResult with ts and remux filled in"""
        arrs = [np.ascontiguousarray(x, np.uint8).reshape(-1) for x in inputs]
        a, c = self._args([x.ctypes.data if len(x) else 0 for x in arrs], [len(x) // 188 for x in arrs])
        out = np.zeros(max(1, int(n_out)) * 188, np.uint8)
        raw, rraw = _TsMuxResult(), _TsMuxRemuxResult()
        pos, rpos = _pos(start, self.n_inputs), _rpos(rstart)
        check(lib().dvbt2ll_tsmux_run_host_remux(self._h, a, c, ctypes.byref(pos), ctypes.byref(rpos),
                                                 out.ctypes.data_as(ctypes.c_void_p), int(n_out), ctypes.byref(raw),
                                                 ctypes.byref(rraw)), "tsmux run host remux")
        res = self._result(raw)
        res.ts = out[:int(n_out) * 188]
        res.remux = self._remux_result(rraw)
        return res

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dvbt2ll_tsmux_destroy(self._h)
            self._h = None


def psi_params(transport_stream_id, version, programs):
    """the dvbt2ll_psi_params of: programs, a list of dicts with program_number, pmt_pid, pcr_pid (default 0x1FFF:
    none) and streams, a list of dicts with stream_type, pid and descriptors (bytes, default none)"""
    p = _PsiParams()
    p.transport_stream_id, p.version, p.n_programs = int(transport_stream_id), int(version), len(programs)
    if len(programs) > len(p.programs):
        raise ValueError("at most %d programmes" % len(p.programs))
    for a, g in enumerate(programs):
        q = p.programs[a]
        q.program_number, q.pmt_pid, q.pcr_pid = int(g["program_number"]), int(g["pmt_pid"]), int(g.get("pcr_pid", 0x1FFF))
        streams = g.get("streams", [])
        if len(streams) > len(q.streams):
            raise ValueError("at most %d streams per programme" % len(q.streams))
        q.n_streams = len(streams)
        for b, e in enumerate(streams):
            d = bytes(e.get("descriptors", b""))
            q.streams[b].stream_type, q.streams[b].pid, q.streams[b].descriptor_len = int(e["stream_type"]), int(e["pid"]), len(d)
            if len(d) > PSI_DESCRIPTOR_BYTES:
                raise ValueError("at most %d descriptor bytes per stream" % PSI_DESCRIPTOR_BYTES)
            q.streams[b].descriptors[:len(d)] = list(d)
    return p


def psi_build(transport_stream_id, version, programs):
    """the PAT / PMT carousel of 16 rounds as a uint8 array of whole packets (dvbt2ll_psi_build): a loop input of TsMux"""
    p = psi_params(transport_stream_id, version, programs)
    n = lib().dvbt2ll_psi_build(ctypes.byref(p), None, 0)
    check(min(int(n), 0), "psi build")
    out = np.zeros(int(n) * 188, np.uint8)
    check(min(int(lib().dvbt2ll_psi_build(ctypes.byref(p), out.ctypes.data_as(ctypes.c_void_p), int(n))), 0), "psi build")
    return out
