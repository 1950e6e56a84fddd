"""T2-MI input (dvbt2ll_t2mi_* in include/dvbt2ll_hip.h): a gateway's transport stream (ETSI TS 102 773 over DVB data
piping) de-encapsulated on the GPU into per-PLP packed BBFRAME streams, the layout a Chain in INPUT_BBFRAME reads.

The reference has no T2-MI code: PARITY UNPINNED -- the output is pinned to tests/t2mi_ref.py's sequential parser
and to known answers.

Example: feed a Chain from a T2-MI stream on the device, everything on torch's stream

    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    de = dvbt2ll.T2miDeframer(pid=0x1000, chain=ch, max_ts_bytes=ts_d.numel(), max_packets=4096)
    L, F = de.plps[0][1], ch.info["fec_blocks_per_frame"]
    bbf = torch.empty(n * F * L, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    de.run_device(ts_d.data_ptr(), ts_d.numel(), [bbf.data_ptr()], [n * F], stream=st)
    ch.run_device(bbf.data_ptr(), 0, bbf.numel(), 0, n, iq_d.data_ptr(), st)
    res = de.result()                      # synchronises: counters, table, resume position
    assert res.blocks[0] == n * F and de.interleaving_frames(0, res) == [F] * n
"""
import ctypes

import numpy as np

from ._lib import lib, check, MAX_PLP, _T2miParams, _T2miPos, _T2miResult

# one packet-table record (dvbt2ll_t2mi_packet)
PACKET_DTYPE = np.dtype([("ts_index", "<u4"), ("ts_byte", "<u4"), ("packet_type", "u1"), ("packet_count", "u1"),
                         ("superframe_idx", "u1"), ("t2mi_stream_id", "u1"), ("payload_len", "<u2"), ("flags", "u1"),
                         ("intl_frame_start", "u1"), ("frame_idx", "u1"), ("plp_id", "u1"), ("out_index", "i1"),
                         ("reserved", "u1"), ("block", "<i4")])
FLAG_COMPLETE, FLAG_CONSISTENT, FLAG_CRC_OK, FLAG_ACCEPTED = 1, 2, 4, 8
COUNTERS = ("ts_contributing", "ts_foreign", "ts_null", "ts_tei", "ts_scrambled", "ts_bad_sync", "ts_no_payload",
            "discontinuities", "bad_pointers", "broken", "crc_errors", "filtered", "len_errors", "other_plp",
            "accepted")


class T2miResult:
    """one call's result: resume (ts_offset, skip); counters (dict); blocks (per output); by_type {packet_type:
    records}; packets (structured array, PACKET_DTYPE); bbframes (per output uint8 array; host runs only)"""

    def __init__(self, raw, nplp, packets):
        self.resume = (int(raw.resume.ts_offset), int(raw.resume.skip))
        self.counters = {n: int(getattr(raw, n)) for n in COUNTERS}
        self.blocks = [int(raw.blocks[k]) for k in range(nplp)]
        self.by_type = {t: int(raw.by_type[t]) for t in range(256) if raw.by_type[t]}
        self.packets = packets
        self.bbframes = None


class T2miDeframer:
    def __init__(self, pid, plps=None, chain=None, plp_ids=None, max_ts_bytes=188 * 4096, max_packets=4096,
                 stream_id=-1, device=0):
        """plps: [(plp_id, L)] with L = kbch / 8 of that PLP's code -- or chain: a Chain whose PLP k gives output k's
        L, with PLP_ID plp_ids[k] (default k).  max_ts_bytes (rounded up to whole TS packets) and max_packets size
        the scratch: the largest buffer and the most T2-MI packets of one call"""
        L = lib()
        p = _T2miParams()
        if chain is not None:
            ids = None if plp_ids is None else (ctypes.c_int * chain.nplp)(*[int(x) for x in plp_ids])
            check(L.dvbt2ll_t2mi_params_from_chain(chain._h, ids, ctypes.byref(p)), "t2mi params from chain")
        else:
            p.nplp = len(plps)
            for k, (plp_id, length) in enumerate(plps[:MAX_PLP]):
                p.plp_id[k], p.bbframe_bytes[k] = int(plp_id), int(length)
        p.pid, p.stream_id = int(pid), int(stream_id)
        p.max_ts_bytes = (int(max_ts_bytes) + 187) // 188 * 188
        p.max_packets = int(max_packets)
        self._h = None
        h = ctypes.c_void_p()
        check(L.dvbt2ll_t2mi_create(ctypes.byref(p), int(device), ctypes.byref(h)), "t2mi create")
        self._h = h
        self.nplp = p.nplp
        self.plps = [(p.plp_id[k], p.bbframe_bytes[k]) for k in range(p.nplp)]
        self.max_ts_bytes, self.max_packets = p.max_ts_bytes, p.max_packets

    def run_device(self, ts_ptr, ts_len, out_ptrs, out_cap_blocks, start=(0, 0), stream=0):
        """asynchronous on stream: TS at device pointer ts_ptr -> block n of output o at out_ptrs[o] + n L"""
        n = self.nplp
        assert len(out_ptrs) == len(out_cap_blocks) == n
        pos = _T2miPos(int(start[0]), int(start[1]))
        check(lib().dvbt2ll_t2mi_run_device(self._h, ctypes.c_void_p(ts_ptr), int(ts_len), ctypes.byref(pos),
                                            (ctypes.c_void_p * n)(*out_ptrs),
                                            (ctypes.c_int64 * n)(*[int(c) for c in out_cap_blocks]),
                                            ctypes.c_void_p(stream or None)), "t2mi run")

    def _packets(self, count):
        out = np.zeros(count, PACKET_DTYPE)
        if count:
            got = lib().dvbt2ll_t2mi_get_packets(self._h, out.ctypes.data_as(ctypes.c_void_p), count)
            check(int(got), "t2mi packets")
            assert got == count
        return out

    def result(self):
        """synchronises with the last run: its T2miResult (bbframes stay on the device)"""
        raw = _T2miResult()
        check(lib().dvbt2ll_t2mi_get_result(self._h, ctypes.byref(raw)), "t2mi result")
        return T2miResult(raw, self.nplp, self._packets(int(raw.packets)))

    def run(self, ts, start=(0, 0), caps=None):
        """host convenience (dvbt2ll_t2mi_run_host): ts a uint8 numpy array; caps: per output capacity in blocks
        (default: all the buffer could hold)"""
        ts = np.ascontiguousarray(ts, np.uint8)
        n = self.nplp
        if caps is None:
            caps = [len(ts) // self.plps[k][1] + 1 for k in range(n)]
        outs = [np.zeros(max(1, int(caps[k])) * self.plps[k][1], np.uint8) for k in range(n)]
        raw = _T2miResult()
        pos = _T2miPos(int(start[0]), int(start[1]))
        check(lib().dvbt2ll_t2mi_run_host(self._h, ts.ctypes.data_as(ctypes.c_void_p), len(ts), ctypes.byref(pos),
                                          (ctypes.c_void_p * n)(*[o.ctypes.data for o in outs]),
                                          (ctypes.c_int64 * n)(*[int(c) for c in caps]), ctypes.byref(raw)),
              "t2mi run host")
        res = T2miResult(raw, n, self._packets(int(raw.packets)))
        res.bbframes = [outs[k][:res.blocks[k] * self.plps[k][1]] for k in range(n)]
        return res

    @staticmethod
    def interleaving_frames(plp, result, leading=False):
        """block counts between consecutive intl_frame_start = 1 packets written to output plp (the last run of
        blocks included): each must equal the chain's F (dynamic PLP_NUM_BLOCKS is not supported).  Blocks written
        before the call's first intl_frame_start = 1 packet (the tail of an interleaving frame that began in an
        earlier call, after a mid-frame resume) belong to no listed frame: with leading=True the result is
        (their number, the list), so a caller that chains calls can add them to the previous call's last count"""
        p = result.packets
        p = p[(p["out_index"] == plp) & (p["block"] >= 0)]
        at = np.nonzero(p["intl_frame_start"])[0]
        frames = [int(b - a) for a, b in zip(at, list(at[1:]) + [len(p)])]
        return (int(at[0]) if len(at) else len(p), frames) if leading else frames

    def __del__(self):
        if getattr(self, "_h", None):
            lib().dvbt2ll_t2mi_destroy(self._h)
            self._h = None
