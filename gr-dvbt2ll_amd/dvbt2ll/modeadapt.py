"""Mode adapter (dvbt2ll_modeadapt_* in include/dvbt2ll_hip.h): a transport stream turned on the GPU into one PLP's
high-efficiency-mode BBFRAMEs, with null-packet deletion and an optional PID selection -- the layout a Chain in
INPUT_BBFRAME reads.

With npd=0 the output is the reference's HEM BBFRAME stream; npd=1 is PARITY UNPINNED (the reference sets NPD = 0)
and pinned to tests/modeadapt_ref.py's sequential restatement and receiver.

Example: two PLPs of a multi-PLP Chain from one multi-programme TS on the device, everything on torch's stream

    ch = dvbt2ll.Chain(mcfg, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    ad = [dvbt2ll.ModeAdapter(chain=ch, plp=k, pids=pids[k], max_ts_bytes=ts_d.numel()) for k in range(ch.nplp)]
    st = torch.cuda.current_stream().cuda_stream
    for k, a in enumerate(ad):
        a.run_device(ts_d.data_ptr(), ts_d.numel(), bbf[k].data_ptr(), bbf[k].numel() // a.L, stream=st)
    ch.run_plps([b.data_ptr() for b in bbf], [0] * ch.nplp, [b.numel() for b in bbf], 0, n, iq_d.data_ptr(), st)
    res = ad[0].result()                   # synchronises: counters, resume position
"""
import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import lib, check, _ModeAdaptParams, _ModeAdaptPos, _ModeAdaptResult

COUNTERS = ("packets_in", "selected", "nulls_deleted", "nulls_kept", "nulls_dropped_at_flush", "sync_errors",
            "bbframes", "flushed")


class ModeAdaptPos(NamedTuple):
    """a position in a call's buffer: the packet, the bytes of its unit already emitted, the unit's DNP"""
    ts_packet: int = 0
    unit_byte: int = 0
    dnp: int = 0


@dataclass
class ModeAdaptResult:
    """one call's result: resume (ModeAdaptPos); counters (dict); bbframes (uint8 array; host runs only)"""
    resume: ModeAdaptPos
    counters: dict
    bbframes: np.ndarray = None


def pid_mask(pids):
    """the 1024-byte selection mask of a PID list (PID p is bit p & 7 of byte p >> 3)"""
    m = np.zeros(1024, np.uint8)
    for p in pids:
        if not 0 <= int(p) <= 0x1FFF:
            raise ValueError("PID %r" % (p,))
        m[int(p) >> 3] |= 1 << (int(p) & 7)
    return m


class ModeAdapter:
    def __init__(self, kbch=0, framesize=0, rate=0, chain=None, plp=0, sis_mis=1, isi=0, npd=1, pids=None,
                 mask=None, max_ts_bytes=188 * 4096, device=0):
        """kbch (or framesize / rate) and sis_mis / isi -- or chain, plp: taken from a Chain's PLP.  pids: a list of
        PIDs to select (mask: the 1024-byte mask itself; neither: every PID but 0x1FFF).  max_ts_bytes (rounded up to
        whole TS packets) sizes the scratch: the largest buffer of one call"""
        L = lib()
        p = _ModeAdaptParams()
        p.kbch, p.framesize, p.rate, p.sis_mis, p.isi = int(kbch), int(framesize), int(rate), int(sis_mis), int(isi)
        if chain is not None:
            check(L.dvbt2ll_modeadapt_params_from_chain(chain._h, int(plp), ctypes.byref(p)), "modeadapt params")
        p.npd = int(npd)
        if pids is not None:
            mask = pid_mask(pids)
        keep = None
        if mask is not None:
            keep = np.ascontiguousarray(mask, np.uint8)
            if keep.size != 1024:
                raise ValueError("a PID mask is 1024 bytes")
            p.pid_mask = keep.ctypes.data_as(ctypes.c_void_p)
        p.max_ts_bytes = (int(max_ts_bytes) + 187) // 188 * 188
        self._h = None
        h = ctypes.c_void_p()
        check(L.dvbt2ll_modeadapt_create(ctypes.byref(p), int(device), ctypes.byref(h)), "modeadapt create")
        self._h = h
        self.npd, self.sis_mis, self.isi = p.npd, p.sis_mis, p.isi
        self.max_ts_bytes = p.max_ts_bytes
        self.kbch = p.kbch or _kbch(p.framesize, p.rate)
        self.L, self.D, self.U = self.kbch // 8, self.kbch // 8 - 10, 188 if p.npd else 187

    def run_device(self, ts_ptr, ts_len, out_ptr, out_cap_blocks, start=ModeAdaptPos(), flush=False, stream=0):
        """asynchronous on stream: TS at device pointer ts_ptr -> BBFRAME k at out_ptr + k L"""
        pos = _ModeAdaptPos(*[int(x) for x in start])
        check(lib().dvbt2ll_modeadapt_run_device(self._h, ctypes.c_void_p(ts_ptr), int(ts_len), ctypes.byref(pos),
                                                 ctypes.c_void_p(out_ptr), int(out_cap_blocks), int(bool(flush)),
                                                 ctypes.c_void_p(stream or None)), "modeadapt run")

    @staticmethod
    def _result(raw):
        return ModeAdaptResult(ModeAdaptPos(int(raw.resume.ts_packet), int(raw.resume.unit_byte), int(raw.resume.dnp)),
                               {n: int(getattr(raw, n)) for n in COUNTERS})

    def result(self):
        """synchronises with the last run: its ModeAdaptResult (the BBFRAMEs stay on the device)"""
        raw = _ModeAdaptResult()
        check(lib().dvbt2ll_modeadapt_get_result(self._h, ctypes.byref(raw)), "modeadapt result")
        return self._result(raw)

    def run(self, ts, start=ModeAdaptPos(), cap=None, flush=False):
        """host convenience (dvbt2ll_modeadapt_run_host): ts a uint8 numpy array; cap: capacity in BBFRAMEs
        (default: all the buffer could fill)"""
        ts = np.ascontiguousarray(ts, np.uint8)
        if cap is None:
            cap = len(ts) // self.D + 1
        out = np.zeros(max(1, int(cap)) * self.L, np.uint8)
        raw = _ModeAdaptResult()
        pos = _ModeAdaptPos(*[int(x) for x in start])
        check(lib().dvbt2ll_modeadapt_run_host(self._h, ts.ctypes.data_as(ctypes.c_void_p), len(ts), ctypes.byref(pos),
                                               out.ctypes.data_as(ctypes.c_void_p), int(cap), int(bool(flush)),
                                               ctypes.byref(raw)), "modeadapt run host")
        res = self._result(raw)
        res.bbframes = out[:res.counters["bbframes"] * self.L]
        return res

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dvbt2ll_modeadapt_destroy(self._h)
            self._h = None


def _kbch(framesize, rate):
    from .configs import KBCH
    return KBCH[(framesize, rate)]
