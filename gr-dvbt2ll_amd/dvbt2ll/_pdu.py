"""What the four PDU-batch encapsulators (ule.py, mpe.py, mpefec.py, gse.py) share: one handle of the C ABI's
dvbt2ll_<PREFIX>_* functions, which all take a PDU buffer, its n + 1 offsets, (ULE and GSE) the optional types, a start
position and an output capacity, and all answer with a resume position and counters.  A subclass names its symbols and
types in class attributes, fills the parameters in its __init__ and keeps the signatures of run_device and run."""
import ctypes

import numpy as np

from ._lib import lib, check


class PduEncapsulator:
    PREFIX = None            # "ule": the symbols are dvbt2ll_ule_*, the error texts "ule run"
    CPOS = CRESULT = None    # the ctypes mirrors of dvbt2ll_<PREFIX>_pos / _result
    POS = RESULT = None      # the public NamedTuple and dataclass
    COUNTERS = ()            # the int64 fields of the result, in the order of the header
    HAS_TYPES = False        # the run calls take a type array behind the offsets
    UNITS, OUT = "ts_packets", "ts"   # the counter of output units; the Result field a host run's output goes to
    unit_bytes = 188         # of an output unit (GSE: the instance's Lb)

    def _fn(self, name):
        return getattr(lib(), "dvbt2ll_%s_%s" % (self.PREFIX, name))

    def _create(self, params, device):
        self._h = None
        h = ctypes.c_void_p()
        check(self._fn("create")(ctypes.byref(params), int(device), ctypes.byref(h)), self.PREFIX + " create")
        self._h = h

    def _run_device(self, pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, cap, type_ptr, start, flush, stream):
        pos = self.CPOS(*[int(x) for x in start])
        types = (ctypes.c_void_p(type_ptr or None),) if self.HAS_TYPES else ()
        check(self._fn("run_device")(self._h, ctypes.c_void_p(pdu_ptr), int(pdu_len), ctypes.c_void_p(off_ptr), *types,
                                     int(n_pdus), ctypes.byref(pos), ctypes.c_void_p(out_ptr), int(cap),
                                     int(bool(flush)), ctypes.c_void_p(stream or None)), self.PREFIX + " run")

    @classmethod
    def _result(cls, raw):
        return cls.RESULT(cls.POS(*[int(getattr(raw.resume, f)) for f in cls.POS._fields]),
                          {n: int(getattr(raw, n)) for n in cls.COUNTERS})

    def result(self):
        """synchronises with the last run: its result (the output stays on the device)"""
        raw = self.CRESULT()
        check(self._fn("get_result")(self._h, ctypes.byref(raw)), self.PREFIX + " result")
        return self._result(raw)

    def _run(self, pdu, off, types, start, cap, flush, bound):
        pdu = np.ascontiguousarray(pdu, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        n = len(off) - 1
        if types is not None:
            types = np.ascontiguousarray(types, np.uint16)
            if len(types) != n:
                raise ValueError("one type per PDU")
        if cap is None:
            cap = bound(len(pdu), n)
        keep = pdu if len(pdu) else np.zeros(1, np.uint8)
        out = np.zeros(max(1, int(cap)) * self.unit_bytes, np.uint8)
        raw = self.CRESULT()
        pos = self.CPOS(*[int(x) for x in start])
        tp = (types.ctypes.data_as(ctypes.c_void_p) if types is not None else None,) if self.HAS_TYPES else ()
        check(self._fn("run_host")(self._h, keep.ctypes.data_as(ctypes.c_void_p), len(pdu),
                                   off.ctypes.data_as(ctypes.c_void_p), *tp, n, ctypes.byref(pos),
                                   out.ctypes.data_as(ctypes.c_void_p), int(cap), int(bool(flush)), ctypes.byref(raw)),
              self.PREFIX + " run host")
        res = self._result(raw)
        setattr(res, self.OUT, out[:res.counters[self.UNITS] * self.unit_bytes])
        return res

    def __del__(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None
