#!/usr/bin/env python3
"""T2-MI framer timing: framing the BBFRAMEs of N frames of a configuration into the gateway's TS,
beside a device-to-device copy of the same output bytes and the chain's stage times on the same BBFRAMEs (BBFRAME
input), the arms alternating, all in one process.  Run three processes and put the outputs next to each other.

  python tools/t2mi_out_measure.py --cfg cfg3 --frames 1280 --chunk-frames 160 --reps 5

One call frames one chunk; every chunk's BBFRAMEs and output lie in memory of their own.  A timestamp-sized (88 bits)
and an L1-current-sized (203 bits) slot go before each frame's BBFRAMEs, as a gateway's stream has them.  Before
anything is timed the first chunk's output, counters and next position are compared with tests/t2mi_out_ref.py's
numpy restatement.  The events are recorded on an explicit non-default stream, the one the handles run on.  Prints one
JSON line."""
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
    import t2mi_out_ref as O

    assert torch.cuda.is_available(), "needs a GPU"
    cfg = CONFIGS[a.cfg]
    n, cf = a.frames, a.chunk_frames
    assert n % cf == 0
    nchunks = n // cf
    Lb, F = KBCH[(cfg.framesize, cfg.rate)] // 8, cfg.fecblocks
    ch = dvbt2ll.Chain(cfg, max_frames=cf)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    slots = [(0x20, 88, 0), (0x10, 203, 0)]
    fr = dvbt2ll.T2miFramer(O.PID, chain=ch, aux=slots, max_frames=cf)
    assert fr.plps == [(0, Lb, F)]
    sh = O.Shape([(0, Lb, F)], aux=slots, fps=fr.frames_per_superframe)
    # one chunk's BBFRAMEs, repeated per chunk: random bytes (the chain encodes them as they are and counts their
    # header CRCs as errors, which costs it nothing)
    bb1 = np.random.default_rng(11).integers(0, 256, cf * F * Lb, dtype=np.uint8)
    _, aux1 = sh.inputs(cf, seed=3)
    N = fr.ts_packets(cf)
    bb = torch.from_numpy(bb1).cuda().repeat(nchunks)
    aux = torch.from_numpy(aux1).cuda()
    out = torch.zeros(nchunks * N * 188, dtype=torch.uint8, device="cuda")
    # a stream with a handle of its own: torch's default stream has handle 0, which the C ABI reads as "the handle's
    # own stream", and then the events below would not bracket the framer's kernels
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(side)
    st = torch.cuda.current_stream().cuda_stream
    assert st != 0

    def frame():
        for c in range(nchunks):
            fr.run_device([bb.data_ptr() + c * len(bb1)], cf, out.data_ptr() + c * N * 188, N, aux_ptr=aux.data_ptr(),
                          aux_stride=sh.aux_stride, aux_off=sh.aux_off, start=(c * cf, 0, 0), stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    frame()
    res = fr.result()
    ref = O.frame_numpy(sh, [bb1], aux1, cf, (0, 0, 0))
    assert np.array_equal(out[:N * 188].cpu().numpy(), ref[0]), "first call's bytes differ from the restatement"
    last = O.frame_numpy(sh, [bb1], aux1, cf, ((nchunks - 1) * cf, 0, 0))
    assert tuple(res.next) == last[1] and res.counters == last[2] and res.by_type == last[3], res
    dst = torch.empty_like(out)

    def copy():
        dst.copy_(out)

    copy()
    t_f, t_cp = [], []
    for _ in range(a.reps):
        t_f.append(timed(frame))
        t_cp.append(timed(copy))

    iq = torch.empty((cf * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
    ch.run_device(bb.data_ptr(), 0, len(bb1), 0, cf, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ch.set_timing(True)
    for _ in range(a.reps):
        for c in range(nchunks):
            ch.run_device(bb.data_ptr() + c * len(bb1), 0, len(bb1), 0, cf, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ms, _ = ch.timing()
    stages = dict(fec=round(ms[0] / a.reps, 4), map=round(ms[1] / a.reps, 4), ofdm=round(ms[2] / a.reps, 4))
    med = float(np.median(t_f))
    total = nchunks * N * 188
    print(json.dumps(dict(cfg=a.cfg, frames=n, chunk_frames=cf, bbframe_bytes=Lb, blocks_per_frame=F,
                          ts_bytes=total, counters_per_chunk=res.counters,
                          frame_ms=[round(x, 4) for x in t_f], frame_ms_median=round(med, 4),
                          frame_gbps=round(total / med / 1e6, 2), d2d_copy_ms=[round(x, 4) for x in t_cp],
                          frame_over_copy=round(med / float(np.median(t_cp)), 2), chain_stage_ms=stages,
                          slowest_stage="framing" if med > max(stages.values()) else max(stages, key=stages.get),
                          time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
