"""GSE encapsulator (dvbt2ll_gse_* in include/dvbt2ll_hip.h): a batch of IP datagrams wrapped on the GPU into GSE
packets (TS 102 606-1) and laid into one PLP's normal-mode BBFRAMEs, the layout a Chain's BBFRAME input and
dvbt2ll_tx --input bbframe take as they are.  No TS layer lies between the datagrams and the IQ.

PARITY UNPINNED (the reference has no GSE code): pinned to tests/gse_ref.py's sequential restatement and its receiver
(DESIGN.md 5.18).

Example: datagrams on the device -> BBFRAMEs -> IQ, everything on torch's stream

    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    enc = dvbt2ll.GseEncapsulator(chain=ch, max_pdu_bytes=pdu_d.numel(), max_pdus=n_pdus)
    st = torch.cuda.current_stream().cuda_stream
    enc.run_device(pdu_d.data_ptr(), pdu_d.numel(), off_d.data_ptr(), n_pdus, bb_d.data_ptr(), bb_d.numel() // enc.Lb,
                   flush=True, stream=st)
    ch.run_device(bb_d.data_ptr(), 0, bb_d.numel(), 0, n, iq_d.data_ptr(), st)
    res = enc.result()                     # synchronises: counters, resume position
"""
import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import lib, check, _GseParams, _GsePos, _GseResult
from ._pdu import PduEncapsulator

COUNTERS = ("pdus_in", "complete", "fragmented", "gse_packets", "skipped_len", "skipped_type", "bbframes", "pad_bytes",
            "flushed")
TILE = 256      # GSE_TILE of csrc/gse_kernels.h: PDUs per position table


class GsePos(NamedTuple):
    """a position in a call's PDU list: the PDU, the number of its bytes already sent, its Frag ID"""
    pdu: int = 0
    pdu_byte: int = 0
    frag_id: int = 0


@dataclass
class GseResult:
    """one call's result: resume (GsePos); counters (dict); bb (uint8 array; host runs only)"""
    resume: GsePos
    counters: dict
    bb: np.ndarray = None


def frame_bound(pdu_len, n_pdus, D, label_len):
    """BBFRAMEs that n_pdus PDUs lying side by side in pdu_len bytes cannot exceed: a closed frame holds at least
    D - 14 - L bytes of PDUs and their 4 + L header bytes each"""
    return (int(pdu_len) + (4 + label_len) * int(n_pdus)) // (D - 14 - label_len) + 2


class GseEncapsulator(PduEncapsulator):
    PREFIX, COUNTERS, HAS_TYPES = "gse", COUNTERS, True
    CPOS, CRESULT, POS, RESULT = _GsePos, _GseResult, GsePos, GseResult
    UNITS, OUT = "bbframes", "bb"

    def __init__(self, kbch=0, framesize=0, rate=0, chain=None, plp=0, sis_mis=1, isi=0, label=None,
                 max_pdu_bytes=1 << 22, max_pdus=1 << 16, device=0):
        """kbch (or framesize / rate) and sis_mis / isi -- or chain, plp: taken from a Chain's PLP.  label: 6 or 3
        bytes, or None / empty for none (broadcast).  max_pdu_bytes / max_pdus size the scratch: the largest PDU
        buffer and PDU count of one call"""
        p = _GseParams()
        p.kbch, p.framesize, p.rate, p.sis_mis, p.isi = int(kbch), int(framesize), int(rate), int(sis_mis), int(isi)
        L = lib()
        if chain is not None:
            check(L.dvbt2ll_gse_params_from_chain(chain._h, int(plp), ctypes.byref(p)), "gse params")
        label = bytes(label or b"")
        if len(label) > 6:
            raise ValueError("a label is 6 or 3 bytes, or none")
        p.label_len = len(label)
        p.label[:len(label)] = list(label)
        p.max_pdu_bytes, p.max_pdus = int(max_pdu_bytes), int(max_pdus)
        self._create(p, device)
        self.kbch = p.kbch or _kbch(p.framesize, p.rate)
        self.Lb, self.D = self.kbch // 8, self.kbch // 8 - 10
        self.unit_bytes = self.Lb
        self.label, self.label_len, self.sis_mis, self.isi = label, len(label), p.sis_mis, p.isi
        self.max_pdu_bytes, self.max_pdus = p.max_pdu_bytes, p.max_pdus

    def frame_bound(self, pdu_len, n_pdus):
        """BBFRAMEs that n_pdus PDUs lying side by side in pdu_len bytes cannot exceed.  An offset table whose valid
        PDUs overlap can make more: a capacity of this size then cuts the call, and the resume position says where"""
        return frame_bound(pdu_len, n_pdus, self.D, self.label_len)

    def run_device(self, pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_blocks, type_ptr=0, start=GsePos(),
                   flush=False, stream=0):
        """asynchronous on stream: PDUs at device pointer pdu_ptr, n_pdus + 1 uint32 offsets at off_ptr (uint16
        types at type_ptr, or 0) -> BBFRAME k at out_ptr + Lb k"""
        self._run_device(pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_blocks, type_ptr, start, flush, stream)

    def run(self, pdu, off, types=None, start=GsePos(), cap=None, flush=False):
        """host convenience (dvbt2ll_gse_run_host): pdu a uint8 array, off the n + 1 offsets, types the optional
        n protocol types; cap: capacity in BBFRAMEs (default: frame_bound, all that PDUs lying side by side become)"""
        return self._run(pdu, off, types, start, cap, flush, self.frame_bound)


def _kbch(framesize, rate):
    from .configs import KBCH
    return KBCH[(framesize, rate)]
