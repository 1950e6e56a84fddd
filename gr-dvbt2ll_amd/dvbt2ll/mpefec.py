"""MPE-FEC encapsulator (dvbt2ll_mpefec_* in include/dvbt2ll_hip.h): a batch of IP datagrams grouped on the GPU into
MPE-FEC frames -- MPE sections that carry real-time parameters, then RS(255,191) columns over GF(2^8) in MPE-FEC
sections -- and packed into the 188-byte TS packets a Chain's TS input, a ModeAdapter and dvbt2ll_tx take as they are.
A receiver can rebuild datagrams lost to TS packet errors; one that knows nothing of MPE-FEC still reads every
datagram.

PARITY UNPINNED (the reference has no MPE-FEC code): pinned to tests/mpefec_ref.py's sequential restatement and its
independent receiver.

Example: datagrams on the device -> TS -> IQ, everything on torch's stream

    enc = dvbt2ll.MpeFecEncapsulator(pid=0x100, rows=1024, max_pdu_bytes=pdu_d.numel(), max_pdus=n, max_frames=64)
    st = torch.cuda.current_stream().cuda_stream
    enc.run_device(pdu_d.data_ptr(), pdu_d.numel(), off_d.data_ptr(), n, ts_d.data_ptr(), ts_d.numel() // 188,
                   flush=True, stream=st)
    ch.run_device(ts_d.data_ptr(), 0, ts_d.numel(), 0, frames, iq_d.data_ptr(), st)
    res = enc.result()                     # synchronises: counters, resume position
"""
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import _MpeFecParams, _MpeFecPos, _MpeFecResult
from ._pdu import PduEncapsulator
from .mpe import MAC

COUNTERS = ("pdus_in", "sections", "fec_sections", "frames", "skipped_len", "skipped_type", "mapped_macs",
            "ts_packets", "pusi_packets", "pad_bytes", "flushed")


class MpeFecPos(NamedTuple):
    """a position in a call's PDU list: the first PDU of a frame, the section of that frame, the bytes of that section
    already emitted, the next continuity counter, the frame's 12-bit index"""
    pdu: int = 0
    section: int = 0
    section_byte: int = 0
    cc: int = 0
    frame: int = 0


@dataclass
class MpeFecResult:
    """one call's result: resume (MpeFecPos); counters (dict); ts (uint8 array; host runs only)"""
    resume: MpeFecPos
    counters: dict
    ts: np.ndarray = None


class MpeFecEncapsulator(PduEncapsulator):
    PREFIX, COUNTERS = "mpefec", COUNTERS
    CPOS, CRESULT, POS, RESULT = _MpeFecPos, _MpeFecResult, MpeFecPos, MpeFecResult

    def __init__(self, pid=0x100, rows=1024, data_columns=191, rs_columns=64, mac=MAC, mac_from_dest=False, packing=1,
                 max_pdu_bytes=1 << 22, max_pdus=1 << 16, max_frames=64, device=0):
        """rows: 256, 512, 768 or 1024; data_columns (1 .. 191): the application data columns a frame may fill (fewer:
        a stronger code); rs_columns (1 .. 64): the RS columns sent (fewer: puncturing).  mac / mac_from_dest as the
        MPE encapsulator's.  max_pdu_bytes / max_pdus / max_frames size the scratch: the largest PDU buffer and PDU
        count of one call, and the most frames one call closes (data_columns + rs_columns columns of rows bytes
        each)"""
        p = _MpeFecParams()
        p.pid, p.packing, p.mac_mode = int(pid), int(packing), int(mac_from_dest)
        if len(bytes(mac)) != 6:
            raise ValueError("a MAC address is 6 bytes")
        p.mac[:] = list(bytes(mac))
        p.max_pdu_bytes, p.max_pdus = int(max_pdu_bytes), int(max_pdus)
        p.rows, p.data_columns, p.rs_columns, p.max_frames = int(rows), int(data_columns), int(rs_columns), int(max_frames)
        self._create(p, device)
        self.pid, self.mac, self.mac_mode, self.packing = p.pid, bytes(mac), p.mac_mode, p.packing
        self.rows, self.data_columns, self.rs_columns = p.rows, p.data_columns, p.rs_columns
        self.max_pdu_bytes, self.max_pdus, self.max_frames = p.max_pdu_bytes, p.max_pdus, p.max_frames

    def packet_bound(self, pdu_len, n_pdus):
        """TS packets that n_pdus PDUs lying side by side in pdu_len bytes cannot exceed, MPE-FEC sections included
        (two successive frames hold more than data_columns x rows bytes, which bounds the frames).  An offset table
        whose valid PDUs overlap can make more: a capacity of this size then cuts the call"""
        pdu_len, n = int(pdu_len), int(n_pdus)
        frames = min(self.max_frames, n, 2 * pdu_len // (self.data_columns * self.rows + 1) + 2)
        total = pdu_len + 16 * n + frames * self.rs_columns * (self.rows + 16)
        return total // 183 + 2 if self.packing else total // 184 + n + frames * self.rs_columns + 1

    def run_device(self, pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_packets, start=MpeFecPos(), flush=False,
                   stream=0):
        """asynchronous on stream: PDUs at device pointer pdu_ptr, n_pdus + 1 uint32 offsets at off_ptr -> TS packet
        k at out_ptr + 188 k"""
        self._run_device(pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_packets, 0, start, flush, stream)

    def run(self, pdu, off, start=MpeFecPos(), cap=None, flush=False):
        """host convenience (dvbt2ll_mpefec_run_host): pdu a uint8 array, off the n + 1 offsets; cap: capacity in TS
        packets (default: packet_bound)"""
        return self._run(pdu, off, None, start, cap, flush, self.packet_bound)
