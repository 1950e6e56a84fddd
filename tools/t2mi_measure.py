#!/usr/bin/env python3
"""T2-MI deframer timing: the deframe of the T2-MI TS of N frames of a configuration beside a
device-to-device copy of the same bytes and the chain's BBFRAME-format FEC stage for the same frames, the arms
alternating, all in one process.  Run three processes and put the outputs next to each other.

  python tools/t2mi_measure.py --cfg cfg3 --frames 1280 --chunk-frames 160 --reps 5

The TS is built on the GPU side from one frame's encapsulated BBFRAMEs repeated (the deframer's work does not
depend on the BBFRAME contents; packet_count and frame_idx repeat, which nothing checks), so no gigabyte stream
is built in Python.  Prints one JSON line."""
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
    from dvbt2ll.configs import CONFIGS, KBCH
    import t2mi_ref as R

    assert torch.cuda.is_available(), "needs a GPU"
    cfg = CONFIGS[a.cfg]
    L, F = KBCH[(cfg.framesize, cfg.rate)] // 8, cfg.fecblocks
    n, cf = a.frames, a.chunk_frames
    assert n % cf == 0
    # one chunk: cf frames whose TS packets are whole (each frame's packets are multiplexed on their own, the last
    # TS packet stuffed), so the chunk is one frame's TS repeated
    bbf1 = np.random.default_rng(1).integers(0, 256, F * L, dtype=np.uint8)
    ts1 = R.ts_mux(R.encapsulate([(0, bbf1, L, F)], 1, timestamps=1), 0x1000)
    # continuity counters: frame f's packets continue frame f - 1's
    per = len(ts1) // 188
    rows = np.tile(ts1.reshape(per, 188), (cf, 1))
    cc = np.arange(cf * per) & 15
    rows[:, 3] = (rows[:, 3] & 0xF0) | cc
    ts1c = torch.from_numpy(rows.reshape(-1)).cuda()
    ts_bytes = ts1c.numel()
    nchunks = n // cf
    # every chunk in memory of its own (input, output and copy destination), so no chunk is served from a cache
    # that an earlier chunk warmed
    ts = ts1c.repeat(nchunks)
    del ts1c
    pk_per_frame = F + 2
    de = dvbt2ll.T2miDeframer(0x1000, plps=[(0, L)], max_ts_bytes=ts_bytes, max_packets=cf * pk_per_frame + 8)
    out = torch.zeros(nchunks * cf * F * L, dtype=torch.uint8, device="cuda")
    ob = cf * F * L
    dst = torch.empty_like(ts)
    ch = dvbt2ll.Chain(cfg, max_frames=cf)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    ch.set_timing(True)
    iq = torch.empty((cf * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def deframe():
        for c in range(nchunks):
            de.run_device(ts.data_ptr() + c * ts_bytes, ts_bytes, [out.data_ptr() + c * ob], [cf * F], stream=st)

    def copy():
        dst.copy_(ts)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    deframe()
    copy()
    res = de.result()
    assert res.blocks == [cf * F] and res.counters["accepted"] == cf * pk_per_frame, (res.blocks, res.counters)
    assert res.counters["crc_errors"] == res.counters["broken"] == res.counters["discontinuities"] == 0
    assert np.array_equal(out[(nchunks - 1) * ob:(nchunks - 1) * ob + F * L].cpu().numpy(), bbf1)
    t_de, t_cp = [], []
    for _ in range(a.reps):
        t_de.append(timed(deframe))
        t_cp.append(timed(copy))
    # the chain's FEC stage on the deframed BBFRAMEs, same frames
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
    med = float(np.median(t_de))
    print(json.dumps(dict(cfg=a.cfg, frames=n, chunk_frames=cf, ts_bytes=total, L=L, F=F,
                          t2mi_packets=cf * pk_per_frame * nchunks,
                          deframe_ms=[round(x, 4) for x in t_de], deframe_ms_median=round(med, 4),
                          deframe_gbps=round(total / med / 1e6, 2),
                          d2d_copy_ms=[round(x, 4) for x in t_cp],
                          deframe_over_copy=round(med / float(np.median(t_cp)), 2),
                          chain_stage_ms_for_frames=dict(fec=round(fec, 4), map=round(ms[1] / a.reps, 4),
                                                         ofdm=round(ms[2] / a.reps, 4)),
                          deframe_over_fec=round(med / fec, 2), time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
