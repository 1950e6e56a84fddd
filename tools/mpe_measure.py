#!/usr/bin/env python3
"""MPE-encapsulator timing: encapsulating the PDUs that fill the TS of N frames of a configuration
beside a device-to-device copy of the same output bytes and the chain's stage times for those frames, the arms
alternating, all in one process.  Run three processes and put the outputs next to each other.

  python tools/mpe_measure.py --cfg cfg3 --frames 1280 --chunk-frames 160 --pdu-bytes 1500 --packing 1 --reps 5

The PDUs are one chunk's (seeded bytes of --pdu-bytes each) repeated on the GPU side: every chunk lies in memory of
its own and each call encapsulates one chunk from a fresh start.  Before anything is timed, a call on the chunk's
first --check-pdus PDUs is compared whole (bytes, counters, resume position) with tests/mpe_ref.py's sequential
encapsulator, and the full call's first packets with that call's.  The events are recorded on the stream the handle
runs on.  Prints one JSON line."""
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
    ap.add_argument("--packing", type=int, default=1)
    ap.add_argument("--check-pdus", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import dvbt2ll
    from dvbt2ll.configs import CONFIGS, ts_for_frames
    import mpe_ref as R

    assert torch.cuda.is_available(), "needs a GPU"
    cfg = CONFIGS[a.cfg]
    n, cf = a.frames, a.chunk_frames
    assert n % cf == 0
    nchunks = n // cf
    need = len(ts_for_frames(cfg, 0, cf)[0])               # TS bytes of one chunk's frames
    L = a.pdu_bytes
    per = L + 16                                           # section bytes per PDU
    npdu = -(-need // 188) * 184 // (per if a.packing else -(-(per + 1) // 184) * 184) + 2   # enough to fill them
    rng = np.random.default_rng(7)
    pdu1 = rng.integers(0, 256, npdu * L, dtype=np.uint8)
    pdu1[::L] = 0x45
    off1 = (np.arange(npdu + 1, dtype=np.uint64) * L).astype(np.uint32)
    enc = dvbt2ll.MpeEncapsulator(pid=0x100, packing=a.packing, max_pdu_bytes=len(pdu1), max_pdus=npdu)
    cap = enc.packet_bound(len(pdu1), npdu)
    pdu = torch.from_numpy(pdu1).cuda().repeat(nchunks)
    off = torch.from_numpy(off1.view(np.int32)).cuda()
    out = torch.zeros(nchunks * cap * 188, dtype=torch.uint8, device="cuda")
    # a stream with a handle of its own: torch's default stream has handle 0, which the C ABI reads as "the handle's
    # own stream", and then the events below would not bracket the encapsulator's kernels
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(side)
    st = torch.cuda.current_stream().cuda_stream
    assert st != 0

    def encap():
        for c in range(nchunks):
            enc.run_device(pdu.data_ptr() + c * len(pdu1), len(pdu1), off.data_ptr(), npdu,
                           out.data_ptr() + c * cap * 188, cap, flush=True, stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the check: a short call against the sequential reference, then the full call's first packets against it
    k = min(a.check_pdus, npdu)
    ref = R.encap(pdu1[:k * L], off1[:k + 1], pid=0x100, packing=a.packing, flush=True, crc=R.crc32_table)
    enc.run_device(pdu.data_ptr(), k * L, off.data_ptr(), k, out.data_ptr(), cap, flush=True, stream=st)
    res = enc.result()
    got = out[:res.counters["ts_packets"] * 188].cpu().numpy()
    assert np.array_equal(got, ref.ts) and res.counters == ref.counters and tuple(res.resume) == ref.resume
    encap()
    res = enc.result()
    whole = ref.counters["ts_packets"] - 1                 # the short call's packets but its flushed last one
    assert np.array_equal(out[(nchunks - 1) * cap * 188:][:whole * 188].cpu().numpy(), ref.ts[:whole * 188])
    assert res.counters["sections"] == npdu and res.counters["flushed"] == 1 and res.resume.pdu == npdu, res
    packets = res.counters["ts_packets"]
    assert packets * 188 >= need
    dst = torch.empty(nchunks * packets * 188, dtype=torch.uint8, device="cuda")
    src = out[:dst.numel()]

    def copy():
        dst.copy_(src)

    copy()
    t_en, t_cp = [], []
    for _ in range(a.reps):
        t_en.append(timed(encap))
        t_cp.append(timed(copy))
    # the chain's stages on the encapsulated TS, same frames
    ch = dvbt2ll.Chain(cfg, max_frames=cf)
    iq = torch.empty((cf * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
    ch.run_device(out.data_ptr(), 0, packets * 188, 0, cf, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ch.set_timing(True)
    for _ in range(a.reps):
        for c in range(nchunks):
            ch.run_device(out.data_ptr() + c * cap * 188, 0, packets * 188, 0, cf, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ms, launches = ch.timing()
    stages = dict(fec=ms[0] / a.reps, map=ms[1] / a.reps, ofdm=ms[2] / a.reps)
    slowest = max(stages.values())
    med = float(np.median(t_en))
    total = nchunks * packets * 188
    print(json.dumps(dict(cfg=a.cfg, frames=n, chunk_frames=cf, pdu_bytes=L, packing=a.packing,
                          pdus=npdu * nchunks, ts_bytes=total, counters_per_chunk=res.counters,
                          encap_ms=[round(x, 4) for x in t_en], encap_ms_median=round(med, 4),
                          encap_gbps=round(total / med / 1e6, 2), d2d_copy_ms=[round(x, 4) for x in t_cp],
                          encap_over_copy=round(med / float(np.median(t_cp)), 2),
                          chain_stage_ms_for_frames={k: round(v, 4) for k, v in stages.items()},
                          encap_over_slowest_stage=round(med / slowest, 3), time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
