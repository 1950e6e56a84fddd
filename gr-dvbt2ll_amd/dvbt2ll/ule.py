"""ULE encapsulator (dvbt2ll_ule_* in include/dvbt2ll_hip.h): a batch of IP datagrams wrapped on the GPU into ULE
SNDUs (RFC 4326) and packed into the 188-byte TS packets a Chain's TS input, a ModeAdapter and dvbt2ll_tx take as they
are -- the data path of the reference flowgraph's source block (gr-ule's ule_source).

PARITY UNPINNED (gr-ule is not part of the reference tree): pinned to tests/ule_ref.py's sequential restatement and
its RFC 4326 receiver.

Example: datagrams on the device -> TS -> IQ, everything on torch's stream

    enc = dvbt2ll.UleEncapsulator(pid=0x100, max_pdu_bytes=pdu_d.numel(), max_pdus=n)
    st = torch.cuda.current_stream().cuda_stream
    enc.run_device(pdu_d.data_ptr(), pdu_d.numel(), off_d.data_ptr(), n, ts_d.data_ptr(), ts_d.numel() // 188,
                   flush=True, stream=st)
    ch.run_device(ts_d.data_ptr(), 0, ts_d.numel(), 0, frames, iq_d.data_ptr(), st)
    res = enc.result()                     # synchronises: counters, resume position
"""
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import _UleParams, _UlePos, _UleResult
from ._pdu import PduEncapsulator

COUNTERS = ("pdus_in", "sndus", "skipped_len", "skipped_type", "ts_packets", "pusi_packets", "pad_bytes", "flushed")
MAC = bytes([0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B])   # the reference flowgraph's destination address


class UlePos(NamedTuple):
    """a position in a call's PDU list: the PDU, the bytes of its SNDU already emitted, the next continuity counter"""
    pdu: int = 0
    sndu_byte: int = 0
    cc: int = 0


@dataclass
class UleResult:
    """one call's result: resume (UlePos); counters (dict); ts (uint8 array; host runs only)"""
    resume: UlePos
    counters: dict
    ts: np.ndarray = None


class UleEncapsulator(PduEncapsulator):
    PREFIX, COUNTERS, HAS_TYPES = "ule", COUNTERS, True
    CPOS, CRESULT, POS, RESULT = _UlePos, _UleResult, UlePos, UleResult

    def __init__(self, pid=0x100, dest=MAC, d_bit=None, packing=1, max_pdu_bytes=1 << 22, max_pdus=1 << 16,
                 device=0):
        """dest: the 6-byte destination address every SNDU carries, or None for none (D = 1; d_bit overrides).
        max_pdu_bytes / max_pdus size the scratch: the largest PDU buffer and PDU count of one call"""
        p = _UleParams()
        p.pid, p.packing = int(pid), int(packing)
        p.d_bit = int(d_bit) if d_bit is not None else int(dest is None)
        if dest is not None:
            if len(bytes(dest)) != 6:
                raise ValueError("a destination address is 6 bytes")
            p.dest[:] = list(bytes(dest))
        p.max_pdu_bytes, p.max_pdus = int(max_pdu_bytes), int(max_pdus)
        self._create(p, device)
        self.pid, self.d_bit, self.packing = p.pid, p.d_bit, p.packing
        self.max_pdu_bytes, self.max_pdus = p.max_pdu_bytes, p.max_pdus

    def packet_bound(self, pdu_len, n_pdus):
        """TS packets that n_pdus PDUs lying side by side in pdu_len bytes cannot exceed.  An offset table whose valid
        PDUs overlap can make more: a capacity of this size then cuts the call, and the resume position says where"""
        total = int(pdu_len) + 14 * int(n_pdus)
        return total // 182 + 2 if self.packing else total // 184 + int(n_pdus) + 1

    def run_device(self, pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_packets, type_ptr=0, start=UlePos(),
                   flush=False, stream=0):
        """asynchronous on stream: PDUs at device pointer pdu_ptr, n_pdus + 1 uint32 offsets at off_ptr (uint16
        types at type_ptr, or 0) -> TS packet k at out_ptr + 188 k"""
        self._run_device(pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_packets, type_ptr, start, flush, stream)

    def run(self, pdu, off, types=None, start=UlePos(), cap=None, flush=False):
        """host convenience (dvbt2ll_ule_run_host): pdu a uint8 array, off the n + 1 offsets, types the optional
        n Type fields; cap: capacity in TS packets (default: packet_bound, all that PDUs lying side by side become)"""
        return self._run(pdu, off, types, start, cap, flush, self.packet_bound)
