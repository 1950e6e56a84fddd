#!/usr/bin/env python3
"""Remux timing, by the method of tools/tsmux_measure.py: the same call of --packets output packets
(default 805 000) on the same schedule, once on a plain handle and once on a handle with all three remux functions on
-- a remap, 8 tracked PIDs restamped on every input, input 0's PCRs restamped -- the two arms alternating in one
process, HIP events on the handle's stream, 256-byte aligned buffers.  Run three processes.

  python tools/tsremux_measure.py --reps 7

Before anything is timed, a call of --check-packets on the remux handle is compared whole (bytes, both results, both
resume positions) with tests/tsremux_ref.py.  The classify pass reads 4 header bytes of every input packet beside the
table lookups, and the emit pass 12: the extra traffic is at least one 64-byte line per packet, which the floor line
reports.  Prints one JSON line."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "gr-dvbt2ll_amd"))
sys.path.insert(0, str(ROOT / "tests"))

HBM_PEAK = 8.0e12     # bytes/s, the MI355X's HBM3E peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=805000)
    ap.add_argument("--check-packets", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import dvbt2ll
    from dvbt2ll.tsmux import TsRemuxPos
    import tsremux_cases as XC
    import tsremux_ref as X

    assert torch.cuda.is_available(), "needs a GPU"
    n_out = a.packets
    kw = dict(period=1000, weight=(600, 300, 10), loop=(0, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=5,
              ticks_per_period=dvbt2ll.ticks_per_period(1000, 40000000))
    rx = dict(map=[(1, 0x106, 0x108)], track_pid=(0x101, 0x102, 0x103, 0x104, 0x105, 0x108, 0, 0x20),
              restamp_cc=(1, 1, 1), in_period=(700,), in_ticks_per_period=(dvbt2ll.ticks_per_period(700, 28000000),))
    plain = dvbt2ll.TsMux(max_out_packets=n_out, **kw)
    remux = dvbt2ll.TsMux(max_out_packets=n_out, **kw)
    remux.set_remux(**rx)
    psi = dvbt2ll.psi_build(1, 0, [dict(program_number=1, pmt_pid=0x20, pcr_pid=0x1FF,
                                        streams=[dict(stream_type=0x0D, pid=0x101), dict(stream_type=0x0D, pid=0x102)])])
    n_in = [n_out * 7 // 10 + 1000, n_out * 3 // 10 + 1000, len(psi) // 188]     # neither input runs dry
    # 4096-packet seeds repeated: input 0 on four PIDs with a PCR on every 40th packet, input 1 on two
    seed = [XC.mixed(4096, (0x101, 0x102, 0x103, 0x104), seed=20), XC.mixed(4096, (0x105, 0x106), seed=21)]
    p = seed[0].reshape(-1, 188)
    p[::40, 3], p[::40, 4], p[::40, 5] = 0x30 | (p[::40, 3] & 15), 7, 0x10
    for k in range(0, 4096, 40):
        X.put_pcr(p[k], 1000 * k)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(side)
    st = torch.cuda.current_stream().cuda_stream
    assert st != 0
    ins = [torch.from_numpy(seed[k]).cuda().repeat(n_in[k] // 4096 + 1)[:n_in[k] * 188].clone() for k in range(2)]
    ins.append(torch.from_numpy(psi).cuda())
    out = torch.zeros(n_out * 188, dtype=torch.uint8, device="cuda")
    ptrs = [t.data_ptr() for t in ins]

    def run_plain(n=n_out):
        plain.run_device(ptrs, n_in, out.data_ptr(), n, stream=st)

    def run_remux(n=n_out):
        remux.run_device_remux(ptrs, n_in, out.data_ptr(), n, rstart=TsRemuxPos(cc=(15,) * 8 + (0,) * 56), stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    k = min(a.check_packets, n_out)
    host = [np.tile(seed[i], n_in[i] // 4096 + 1)[:n_in[i] * 188] for i in range(2)] + [psi]
    ref, rref = X.remux(host, k, rstart=((15,) * 8 + (0,) * 56, (0,) * 8, (0,) * 8), **rx, **kw)
    run_remux(k)
    res, rres = remux.result(), remux.remux_result()
    assert np.array_equal(out[:k * 188].cpu().numpy(), ref.ts) and res.counters == ref.counters
    assert tuple(res.resume) == ref.resume and rres.counters == rref.counters and tuple(rres.resume) == rref.resume
    run_plain()
    run_remux()
    rres = remux.remux_result()
    t_pl, t_rx = [], []
    for _ in range(a.reps):
        t_pl.append(timed(run_plain))
        t_rx.append(timed(run_remux))
    med = [float(np.median(t)) for t in (t_pl, t_rx)]
    extra = 64 * sum(remux.result().counters["consumed"])          # one line per input packet, read by classify
    print(json.dumps(dict(packets=n_out, remux_counters=rres.counters, plain_ms=[round(x, 4) for x in t_pl],
                          plain_ms_median=round(med[0], 4), remux_ms=[round(x, 4) for x in t_rx],
                          remux_ms_median=round(med[1], 4), remux_over_plain=round(med[1] / med[0], 3),
                          classify_floor_bytes=extra, classify_floor_ms_at_hbm_peak=round(extra / HBM_PEAK * 1e3, 4),
                          time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
