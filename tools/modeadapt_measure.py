#!/usr/bin/env python3
"""Mode-adapter timing: adapting the TS of N frames of a configuration (about one packet in ten a
null packet) beside a device-to-device copy of the same bytes and the chain's BBFRAME-format FEC stage for the same
frames, the arms alternating, all in one process.  Run three processes and put the outputs next to each other.

  python tools/modeadapt_measure.py --cfg cfg3 --frames 1280 --chunk-frames 160 --reps 5

The TS is one chunk's packets (seeded payloads, every tenth a null packet) repeated on the GPU side: every chunk lies
in memory of its own, each call adapts one chunk from a fresh start, and before anything is timed one call's whole
output, counters and resume position are compared with tests/large_ref.py's adapt_fast (the vectorised restatement
that tests/test_cpu_large_ref.py proves against the sequential reference).  Prints one JSON line."""
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import dvbt2ll
    from dvbt2ll.configs import CONFIGS, KBCH, ts_packets
    import large_ref as G

    assert torch.cuda.is_available(), "needs a GPU"
    cfg = CONFIGS[a.cfg]
    kbch, F = KBCH[(cfg.framesize, cfg.rate)], cfg.fecblocks
    L, D = kbch // 8, kbch // 8 - 10
    n, cf = a.frames, a.chunk_frames
    assert n % cf == 0
    nchunks = n // cf
    # one chunk: enough packets for cf frames' BBFRAMEs when nine in ten are transmitted
    units = cf * F * D // 188 + 2
    npk = units * 10 // 9 + 10
    rows = ts_packets(0, npk, 5).reshape(npk, 188).copy()
    rows[:, 1], rows[:, 2] = (rows[:, 1] & 0xE0) | 1, 0x00          # PID 0x100
    rows[9::10, 1], rows[9::10, 2] = rows[9::10, 1] | 0x1F, 0xFF    # every tenth: PID 0x1FFF
    ts1 = rows.reshape(-1)
    ts_bytes = len(ts1)
    ts = torch.from_numpy(ts1).cuda().repeat(nchunks)
    ad = dvbt2ll.ModeAdapter(kbch=kbch, max_ts_bytes=ts_bytes)
    ob = cf * F * L
    out = torch.zeros(nchunks * ob, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(ts)
    ch = dvbt2ll.Chain(cfg, max_frames=cf)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    iq = torch.empty((cf * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
    # a stream with a handle of its own: torch's default stream has handle 0, which the C ABI reads as "the handle's
    # own stream", and then the events below would not bracket the adapter's kernels
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(side)
    st = torch.cuda.current_stream().cuda_stream
    assert st != 0

    def adapt():
        for c in range(nchunks):
            ad.run_device(ts.data_ptr() + c * ts_bytes, ts_bytes, out.data_ptr() + c * ob, cf * F, stream=st)

    def copy():
        dst.copy_(ts)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    adapt()
    copy()
    res = ad.result()
    assert res.counters["bbframes"] == cf * F, res.counters
    # the last call's whole output, counters and resume position against the vectorised reference
    ref = G.adapt_fast(ts1, kbch, cap=cf * F)
    assert np.array_equal(out[(nchunks - 1) * ob:].cpu().numpy(), ref.bbframes)
    assert res.counters == ref.counters and tuple(res.resume) == tuple(ref.resume), (res, ref.counters, ref.resume)
    t_ad, t_cp = [], []
    for _ in range(a.reps):
        t_ad.append(timed(adapt))
        t_cp.append(timed(copy))
    # the chain's FEC stage on the adapted BBFRAMEs, same frames
    ch.run_device(out.data_ptr(), 0, ob, 0, cf, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ch.set_timing(True)
    for _ in range(a.reps):
        for c in range(nchunks):
            ch.run_device(out.data_ptr() + c * ob, 0, ob, 0, cf, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ms, launches = ch.timing()
    fec = ms[0] / a.reps
    total = ts.numel()
    med = float(np.median(t_ad))
    print(json.dumps(dict(cfg=a.cfg, frames=n, chunk_frames=cf, ts_bytes=total, L=L, F=F,
                          packets=npk * nchunks, null_share=round(float((rows[:, 2] == 0xFF).mean()), 3),
                          adapt_ms=[round(x, 4) for x in t_ad], adapt_ms_median=round(med, 4),
                          adapt_gbps=round(total / med / 1e6, 2),
                          d2d_copy_ms=[round(x, 4) for x in t_cp],
                          adapt_over_copy=round(med / float(np.median(t_cp)), 2),
                          chain_stage_ms_for_frames=dict(fec=round(fec, 4), map=round(ms[1] / a.reps, 4),
                                                         ofdm=round(ms[2] / a.reps, 4)),
                          adapt_over_fec=round(med / fec, 2), time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
