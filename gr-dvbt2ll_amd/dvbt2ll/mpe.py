"""MPE encapsulator (dvbt2ll_mpe_* in include/dvbt2ll_hip.h): a batch of IP datagrams wrapped on the GPU into DSM-CC
datagram_sections (Multi-Protocol Encapsulation, EN 301 192 clause 7) and packed into the 188-byte TS packets a
Chain's TS input, a ModeAdapter and dvbt2ll_tx take as they are -- the encapsulation DVB specifies for IP over a TS,
which deployed IP-over-DVB receivers and TS analysers read.

PARITY UNPINNED (the reference has no MPE code): pinned to tests/mpe_ref.py's sequential restatement and its
ISO/IEC 13818-1 section receiver.

Example: datagrams on the device -> TS -> IQ, everything on torch's stream

    enc = dvbt2ll.MpeEncapsulator(pid=0x100, mac_from_dest=True, max_pdu_bytes=pdu_d.numel(), max_pdus=n)
    st = torch.cuda.current_stream().cuda_stream
    enc.run_device(pdu_d.data_ptr(), pdu_d.numel(), off_d.data_ptr(), n, ts_d.data_ptr(), ts_d.numel() // 188,
                   flush=True, stream=st)
    ch.run_device(ts_d.data_ptr(), 0, ts_d.numel(), 0, frames, iq_d.data_ptr(), st)
    res = enc.result()                     # synchronises: counters, resume position
"""
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from ._lib import _MpeParams, _MpePos, _MpeResult
from ._pdu import PduEncapsulator

COUNTERS = ("pdus_in", "sections", "skipped_len", "skipped_type", "mapped_macs", "ts_packets", "pusi_packets",
            "pad_bytes", "flushed")
MAC = bytes([0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B])   # the default address: the ULE encapsulator's


class MpePos(NamedTuple):
    """a position in a call's PDU list: the PDU, the bytes of its section already emitted, the next continuity
    counter"""
    pdu: int = 0
    section_byte: int = 0
    cc: int = 0


@dataclass
class MpeResult:
    """one call's result: resume (MpePos); counters (dict); ts (uint8 array; host runs only)"""
    resume: MpePos
    counters: dict
    ts: np.ndarray = None


class MpeEncapsulator(PduEncapsulator):
    PREFIX, COUNTERS = "mpe", COUNTERS
    CPOS, CRESULT, POS, RESULT = _MpePos, _MpeResult, MpePos, MpeResult

    def __init__(self, pid=0x100, mac=MAC, mac_from_dest=False, packing=1, max_pdu_bytes=1 << 22, max_pdus=1 << 16,
                 device=0):
        """mac: the 6-byte MAC address the sections carry; mac_from_dest (mac_mode 1): a datagram to an IPv4 / IPv6
        multicast group carries the group's MAC instead.  max_pdu_bytes / max_pdus size the scratch: the largest PDU
        buffer and PDU count of one call"""
        p = _MpeParams()
        p.pid, p.packing, p.mac_mode = int(pid), int(packing), int(mac_from_dest)
        if len(bytes(mac)) != 6:
            raise ValueError("a MAC address is 6 bytes")
        p.mac[:] = list(bytes(mac))
        p.max_pdu_bytes, p.max_pdus = int(max_pdu_bytes), int(max_pdus)
        self._create(p, device)
        self.pid, self.mac, self.mac_mode, self.packing = p.pid, bytes(mac), p.mac_mode, p.packing
        self.max_pdu_bytes, self.max_pdus = p.max_pdu_bytes, p.max_pdus

    def packet_bound(self, pdu_len, n_pdus):
        """TS packets that n_pdus PDUs lying side by side in pdu_len bytes cannot exceed.  An offset table whose valid
        PDUs overlap can make more: a capacity of this size then cuts the call, and the resume position says where"""
        total = int(pdu_len) + 16 * int(n_pdus)
        return total // 183 + 2 if self.packing else total // 184 + int(n_pdus) + 1

    def run_device(self, pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_packets, start=MpePos(), flush=False,
                   stream=0):
        """asynchronous on stream: PDUs at device pointer pdu_ptr, n_pdus + 1 uint32 offsets at off_ptr -> TS packet
        k at out_ptr + 188 k"""
        self._run_device(pdu_ptr, pdu_len, off_ptr, n_pdus, out_ptr, out_cap_packets, 0, start, flush, stream)

    def run(self, pdu, off, start=MpePos(), cap=None, flush=False):
        """host convenience (dvbt2ll_mpe_run_host): pdu a uint8 array, off the n + 1 offsets; cap: capacity in TS
        packets (default: packet_bound, all that PDUs lying side by side become)"""
        return self._run(pdu, off, None, start, cap, flush, self.packet_bound)
