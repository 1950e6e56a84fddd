"""T2-MI output (dvbt2ll_t2mi_out_* in include/dvbt2ll_hip.h): per-PLP packed BBFRAMEs on the device framed on the
GPU into the transport stream a T2 gateway sends to its modulators (ETSI TS 102 773 over DVB data piping): the inverse
of T2miDeframer.  Whole T2 frames per call; timestamp and L1-current packets are carried as opaque slots.

The reference has no T2-MI code: PARITY UNPINNED -- the output is pinned to tests/t2mi_out_ref.py's sequential framer,
to tests/t2mi_ref.py's parser and to the deframer on the device.

Example: a TS on the device -> BBFRAMEs (mode adapter) -> the gateway's T2-MI TS and the local IQ of the same frames,
everything on torch's stream

    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    ad = dvbt2ll.ModeAdapter(chain=ch, max_ts_bytes=ts_d.numel())
    fr = dvbt2ll.T2miFramer(pid=0x1000, chain=ch, max_frames=n)
    F, Lb = fr.plps[0][2], fr.plps[0][1]
    bb_d = torch.empty(n * F * Lb, dtype=torch.uint8, device="cuda")
    out_d = torch.empty(fr.ts_packets(n) * 188, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream   # inside `with torch.cuda.stream(side)`: handle 0 would mean each
                                                   # handle's own stream, and the three calls would not be ordered
    ad.run_device(ts_d.data_ptr(), ts_d.numel(), bb_d.data_ptr(), n * F, stream=st)
    fr.run_device([bb_d.data_ptr()], n, out_d.data_ptr(), fr.ts_packets(n), stream=st)
    ch.run_device(bb_d.data_ptr(), 0, bb_d.numel(), 0, n, iq_d.data_ptr(), st)
    res = fr.result()                      # synchronises: counters; res.next starts the next call
"""
import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import lib, check, MAX_PLP, T2MI_OUT_MAX_AUX, _T2miOutParams, _T2miOutPos, _T2miOutResult

COUNTERS = ("frames", "t2mi_packets", "ts_packets", "pusi_packets", "stuffing_bytes")


class AuxSlot(NamedTuple):
    """an auxiliary packet of every T2 frame: after = 0 before the frame's BBFRAME packets, 1 after them"""
    packet_type: int
    payload_bits: int
    after: int = 0

    @property
    def nbytes(self):
        return (self.payload_bits + 7) // 8


class T2miOutPos(NamedTuple):
    """where a call starts: the first T2 frame's number, the first packet's packet_count, the first TS packet's
    continuity counter"""
    frame: int = 0
    packet_count: int = 0
    cc: int = 0


@dataclass
class T2miOutResult:
    """one call's result: next (T2miOutPos, the next call's start); counters (dict); by_type {packet_type: packets};
    ts (uint8 array; host runs only)"""
    next: T2miOutPos
    counters: dict
    by_type: dict
    ts: np.ndarray = None


class T2miFramer:
    def __init__(self, pid, plps=None, chain=None, plp_ids=None, frames_per_superframe=None, aux=(), stream_id=0,
                 max_frames=16, device=0):
        """plps: [(plp_id, Lb, F)] with Lb = kbch / 8 and F BBFRAMEs per T2 frame -- or chain: a Chain whose PLP k
        gives Lb and F, with PLP_ID plp_ids[k] (default k) and its frames per superframe.  aux: up to 4 AuxSlot.
        max_frames sizes the tables and scratch: the most T2 frames of one call"""
        L = lib()
        p = _T2miOutParams()
        if chain is not None:
            ids = None if plp_ids is None else (ctypes.c_int * chain.nplp)(*[int(x) for x in plp_ids])
            check(L.dvbt2ll_t2mi_out_params_from_chain(chain._h, ids, ctypes.byref(p)), "t2mi out params from chain")
        else:
            p.nplp = len(plps)
            for k, (plp_id, length, blocks) in enumerate(plps[:MAX_PLP]):
                p.plp_id[k], p.bbframe_bytes[k], p.blocks_per_frame[k] = int(plp_id), int(length), int(blocks)
            p.frames_per_superframe = 2
        if frames_per_superframe is not None:
            p.frames_per_superframe = int(frames_per_superframe)
        aux = [AuxSlot(*a) for a in aux]
        p.naux = len(aux)
        for a, s in enumerate(aux[:T2MI_OUT_MAX_AUX]):
            p.aux[a].packet_type, p.aux[a].payload_bits, p.aux[a].after = int(s[0]), int(s[1]), int(s[2])
        p.pid, p.t2mi_stream_id, p.max_frames = int(pid), int(stream_id), int(max_frames)
        self._h = None
        h = ctypes.c_void_p()
        check(L.dvbt2ll_t2mi_out_create(ctypes.byref(p), int(device), ctypes.byref(h)), "t2mi out create")
        self._h = h
        self.nplp, self.aux, self.pid, self.stream_id = p.nplp, aux, p.pid, p.t2mi_stream_id
        self.plps = [(p.plp_id[k], p.bbframe_bytes[k], p.blocks_per_frame[k]) for k in range(p.nplp)]
        self.frames_per_superframe, self.max_frames = p.frames_per_superframe, p.max_frames

    def ts_packets(self, nframes):
        """the TS packets a call of nframes frames writes: known before the launch"""
        return check(int(lib().dvbt2ll_t2mi_out_ts_packets(self._h, int(nframes))), "t2mi out ts_packets")

    def run_device(self, bb_ptrs, nframes, out_ptr, out_cap_packets, aux_ptr=0, aux_stride=0, aux_off=(),
                   start=T2miOutPos(), stream=0):
        """asynchronous on stream: PLP k's nframes x F BBFRAMEs at device pointer bb_ptrs[k], slot a's payload of
        frame f at aux_ptr + f aux_stride + aux_off[a] -> TS packet q at out_ptr + 188 q"""
        n, na = self.nplp, len(self.aux)
        assert len(bb_ptrs) == n and len(aux_off) == na
        pos = _T2miOutPos(*[int(x) for x in start])
        check(lib().dvbt2ll_t2mi_out_run_device(self._h, (ctypes.c_void_p * n)(*bb_ptrs),
                                                ctypes.c_void_p(aux_ptr or None), int(aux_stride),
                                                (ctypes.c_int64 * na)(*[int(o) for o in aux_off]) if na else None,
                                                ctypes.byref(pos), int(nframes), ctypes.c_void_p(out_ptr or None),
                                                int(out_cap_packets), ctypes.c_void_p(stream or None)), "t2mi out run")

    @staticmethod
    def _result(raw):
        return T2miOutResult(T2miOutPos(int(raw.next.frame), int(raw.next.packet_count), int(raw.next.cc)),
                             {n: int(getattr(raw, n)) for n in COUNTERS},
                             {t: int(raw.by_type[t]) for t in range(256) if raw.by_type[t]})

    def result(self):
        """synchronises with the last run: its T2miOutResult (the packets stay on the device)"""
        raw = _T2miOutResult()
        check(lib().dvbt2ll_t2mi_out_get_result(self._h, ctypes.byref(raw)), "t2mi out result")
        return self._result(raw)

    def run(self, bbframes, nframes, aux=None, aux_stride=0, aux_off=(), start=T2miOutPos()):
        """host convenience (dvbt2ll_t2mi_out_run_host): bbframes a uint8 array per PLP; aux a uint8 array holding
        the slots' payloads as run_device reads them"""
        n, na = self.nplp, len(self.aux)
        bb = [np.ascontiguousarray(b, np.uint8) for b in bbframes]
        assert len(bb) == n and len(aux_off) == na
        for k, (_, length, blocks) in enumerate(self.plps):
            if len(bb[k]) < nframes * blocks * length:
                raise ValueError("PLP %d: %d bytes for %d frames of %d BBFRAMEs" % (k, len(bb[k]), nframes, blocks))
        if na:
            aux = np.ascontiguousarray(aux, np.uint8)
            need = max((nframes - 1) * aux_stride + o + s.nbytes for o, s in zip(aux_off, self.aux)) if nframes else 0
            if len(aux) < need:
                raise ValueError("the auxiliary buffer holds %d bytes, the payloads end at %d" % (len(aux), need))
        cap = self.ts_packets(nframes)
        out = np.zeros(max(1, cap) * 188, np.uint8)
        raw = _T2miOutResult()
        pos = _T2miOutPos(*[int(x) for x in start])
        check(lib().dvbt2ll_t2mi_out_run_host(self._h, (ctypes.c_void_p * n)(*[b.ctypes.data for b in bb]),
                                              aux.ctypes.data_as(ctypes.c_void_p) if na else None, int(aux_stride),
                                              (ctypes.c_int64 * na)(*[int(o) for o in aux_off]) if na else None,
                                              ctypes.byref(pos), int(nframes), out.ctypes.data_as(ctypes.c_void_p),
                                              cap, ctypes.byref(raw)), "t2mi out run host")
        res = self._result(raw)
        res.ts = out[:cap * 188]
        return res

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dvbt2ll_t2mi_out_destroy(self._h)
            self._h = None
