#!/usr/bin/env python3
"""GSE-encapsulator timing: encapsulating the PDUs that fill the BBFRAMEs of N frames of a
configuration, beside the ULE handle on the same PDUs, a device-to-device copy of the output bytes and the chain's
stage times (BBFRAME input on the GSE frames, TS input on the ULE packets), the arms alternating, all in one process.
Run three processes and put the outputs next to each other.

  python tools/gse_measure.py --cfg cfg3 --frames 1280 --chunk-frames 160 --pdu-bytes 1500 --reps 5

The PDUs are one chunk's (seeded bytes of --pdu-bytes each) repeated on the GPU side: every chunk lies in memory of
its own and each call encapsulates one chunk from a fresh start.  Before anything is timed, a call on the chunk's
first --check-pdus PDUs is compared whole (bytes, counters, resume position) with tests/gse_ref.py's sequential
encapsulator, and the full call's first frames with that call's.  The events are recorded on the stream the handles
run on.  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gr-dvbt2ll_amd"))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg3")
    ap.add_argument("--frames", type=int, default=1280)
    ap.add_argument("--chunk-frames", type=int, default=160)
    ap.add_argument("--pdu-bytes", type=int, default=1500)
    ap.add_argument("--check-pdus", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import dvbt2ll
    from dvbt2ll.configs import CONFIGS, KBCH
    import gse_ref as R

    assert torch.cuda.is_available(), "needs a GPU"
    cfg = CONFIGS[a.cfg]
    n, cf = a.frames, a.chunk_frames
    assert n % cf == 0
    nchunks = n // cf
    kbch = KBCH[(cfg.framesize, cfg.rate)]
    Lb, D, F = kbch // 8, kbch // 8 - 10, cfg.fecblocks
    blocks = cf * F                                        # BBFRAMEs of one chunk's frames
    L = a.pdu_bytes
    npdu = blocks * D // (L + 10) + 2                      # enough to fill them (a packet adds 10 bytes unfragmented)
    rng = np.random.default_rng(7)
    pdu1 = rng.integers(0, 256, npdu * L, dtype=np.uint8)
    pdu1[::L] = 0x45
    off1 = (np.arange(npdu + 1, dtype=np.uint64) * L).astype(np.uint32)
    enc = dvbt2ll.GseEncapsulator(kbch=kbch, label=R.LABEL, max_pdu_bytes=len(pdu1), max_pdus=npdu)
    ule = dvbt2ll.UleEncapsulator(pid=0x100, packing=1, max_pdu_bytes=len(pdu1), max_pdus=npdu)
    cap = enc.frame_bound(len(pdu1), npdu)
    ucap = ule.packet_bound(len(pdu1), npdu)
    pdu = torch.from_numpy(pdu1).cuda().repeat(nchunks)
    off = torch.from_numpy(off1.view(np.int32)).cuda()
    out = torch.zeros(nchunks * cap * Lb, dtype=torch.uint8, device="cuda")
    ts = torch.zeros(nchunks * ucap * 188, dtype=torch.uint8, device="cuda")
    # a stream with a handle of its own: torch's default stream has handle 0, which the C ABI reads as "the handle's
    # own stream", and then the events below would not bracket the encapsulators' kernels
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(side)
    st = torch.cuda.current_stream().cuda_stream
    assert st != 0

    def gse():
        for c in range(nchunks):
            enc.run_device(pdu.data_ptr() + c * len(pdu1), len(pdu1), off.data_ptr(), npdu,
                           out.data_ptr() + c * cap * Lb, cap, flush=True, stream=st)

    def ule_ts():
        for c in range(nchunks):
            ule.run_device(pdu.data_ptr() + c * len(pdu1), len(pdu1), off.data_ptr(), npdu,
                           ts.data_ptr() + c * ucap * 188, ucap, flush=True, stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the check: a short call against the sequential reference, then the full call's first frames against it
    k = min(a.check_pdus, npdu)
    ref = R.encap(pdu1[:k * L], off1[:k + 1], kbch=kbch, label=R.LABEL, flush=True, crc=R.crc32_table)
    enc.run_device(pdu.data_ptr(), k * L, off.data_ptr(), k, out.data_ptr(), cap, flush=True, stream=st)
    res = enc.result()
    got = out[:res.counters["bbframes"] * Lb].cpu().numpy()
    assert np.array_equal(got, ref.bb) and res.counters == ref.counters and tuple(res.resume) == ref.resume
    gse()
    res = enc.result()
    whole = ref.counters["bbframes"] - 1                   # the short call's frames but its flushed last one
    assert np.array_equal(out[(nchunks - 1) * cap * Lb:][:whole * Lb].cpu().numpy(), ref.bb[:whole * Lb])
    assert res.counters["complete"] + res.counters["fragmented"] == npdu and res.resume.pdu == npdu, res
    frames_out = res.counters["bbframes"]
    assert frames_out >= blocks
    ule_ts()
    ures = ule.result()
    packets = ures.counters["ts_packets"]
    dst = torch.empty(nchunks * frames_out * Lb, dtype=torch.uint8, device="cuda")
    src = out[:dst.numel()]

    def copy():
        dst.copy_(src)

    copy()
    t_g, t_u, t_cp = [], [], []
    for _ in range(a.reps):
        t_g.append(timed(gse))
        t_u.append(timed(ule_ts))
        t_cp.append(timed(copy))

    def stages(ch, buf, stride, nbytes):
        iq = torch.empty((cf * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
        ch.run_device(buf.data_ptr(), 0, nbytes, 0, cf, iq.data_ptr(), st)
        torch.cuda.synchronize()
        ch.set_timing(True)
        for _ in range(a.reps):
            for c in range(nchunks):
                ch.run_device(buf.data_ptr() + c * stride, 0, nbytes, 0, cf, iq.data_ptr(), st)
        torch.cuda.synchronize()
        ms, _ = ch.timing()
        return dict(fec=round(ms[0] / a.reps, 4), map=round(ms[1] / a.reps, 4), ofdm=round(ms[2] / a.reps, 4))

    ch = dvbt2ll.Chain(cfg, max_frames=cf)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    s_bb = stages(ch, out, cap * Lb, blocks * Lb)
    errs = ch.bbheader_errors()
    del ch
    s_ts = stages(dvbt2ll.Chain(cfg, max_frames=cf), ts, ucap * 188, packets * 188)
    med = float(np.median(t_g))
    total = nchunks * frames_out * Lb
    # BBFRAMEs the same datagrams need over ULE and a TS: 187 of each packet's 188 bytes are carried (normal mode)
    ule_frames = -(-packets * 187 // D)
    print(json.dumps(dict(cfg=a.cfg, frames=n, chunk_frames=cf, pdu_bytes=L, pdus=npdu * nchunks, bb_bytes=total,
                          counters_per_chunk=res.counters, bbheader_errors=errs,
                          gse_ms=[round(x, 4) for x in t_g], gse_ms_median=round(med, 4),
                          gse_gbps=round(total / med / 1e6, 2), ule_ms=[round(x, 4) for x in t_u],
                          d2d_copy_ms=[round(x, 4) for x in t_cp], gse_over_copy=round(med / float(np.median(t_cp)), 2),
                          chain_stage_ms_bbframe_input=s_bb, chain_stage_ms_ts_input=s_ts,
                          gse_plus_fec_ms=round(med + s_bb["fec"], 4),
                          ule_plus_ts_fec_ms=round(float(np.median(t_u)) + s_ts["fec"], 4),
                          bbframes_per_chunk_gse=frames_out, bbframes_per_chunk_ule_over_ts=int(ule_frames),
                          time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
