#!/usr/bin/env python3
"""TS-multiplexer timing: one call that writes --packets output packets (default 805 000: 151 MB, the
TS of 160 cfg3 frames that 5.21 measured) from two inputs, a PSI carousel and a PCR generator, with aligned buffers and
with every buffer at an odd alignment of its own, beside a device-to-device copy of the same output bytes, the arms
alternating, all in one process.  Run three processes and put the outputs next to each other.

  python tools/tsmux_measure.py --reps 7

The schedule: period 1000 with 600 slots for input 0 (the fill input, which also takes the 85 null slots), 300 for
input 1, 10 for the carousel and 5 PCR packets, so all slots but the PCR ones read 188 bytes and every slot writes
188: the floor is 376 bytes of HBM traffic per slot.  Before anything is timed, a call of --check-packets is compared
whole (bytes, counters, resume position) with tests/tsmux_ref.py's sequential multiplexer at both alignments.  The
events are recorded on the stream the handle runs on.  Prints one JSON line."""
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
    import tsmux_cases as C
    import tsmux_ref as R

    assert torch.cuda.is_available(), "needs a GPU"
    n_out = a.packets
    kw = dict(period=1000, weight=(600, 300, 10), loop=(0, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=5,
              ticks_per_period=dvbt2ll.ticks_per_period(1000, 40000000))
    mux = dvbt2ll.TsMux(max_out_packets=n_out, **kw)
    psi = dvbt2ll.psi_build(1, 0, [dict(program_number=1, pmt_pid=0x20, pcr_pid=0x1FF,
                                        streams=[dict(stream_type=0x0D, pid=0x101), dict(stream_type=0x0D, pid=0x102)])])
    n_in = [n_out * 7 // 10 + 1000, n_out * 3 // 10 + 1000, len(psi) // 188]     # neither input runs dry
    seed = [C.stream(4096, 0x101), C.stream(4096, 0x102)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(side)
    st = torch.cuda.current_stream().cuda_stream
    assert st != 0
    # every buffer twice: 256-byte aligned (torch's allocation) and at an odd offset of its own
    offs = ((0, 0, 0, 0), (2, 3, 1, 1))       # inputs 0, 1, the carousel, the output
    bufs = []
    for o in offs:
        ins = []
        for k in range(2):
            t = torch.from_numpy(seed[k]).cuda().repeat(n_in[k] // 4096 + 1)[:n_in[k] * 188]
            ins.append(torch.cat([torch.zeros(o[k], dtype=torch.uint8, device="cuda"), t]))
        ins.append(torch.cat([torch.zeros(o[2], dtype=torch.uint8, device="cuda"), torch.from_numpy(psi).cuda()]))
        out = torch.zeros(n_out * 188 + 16, dtype=torch.uint8, device="cuda")
        bufs.append((ins, out, o))

    def run(which, n=n_out):
        ins, out, o = bufs[which]
        mux.run_device([ins[k].data_ptr() + o[k] for k in range(3)], n_in, out.data_ptr() + o[3], n, stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the check: a short call against the sequential reference at both alignments
    k = min(a.check_packets, n_out)
    host = [np.tile(seed[i], n_in[i] // 4096 + 1)[:n_in[i] * 188] for i in range(2)] + [psi]
    ref = R.mux(host, k, **kw)
    for which in (0, 1):
        run(which, k)
        res = mux.result()
        o = bufs[which][2][3]
        got = bufs[which][1][o:o + k * 188].cpu().numpy()
        assert np.array_equal(got, ref.ts) and res.counters == ref.counters and tuple(res.resume) == ref.resume, which
    dst = torch.empty(n_out * 188, dtype=torch.uint8, device="cuda")
    src = bufs[0][1][:n_out * 188]

    def copy():
        dst.copy_(src)

    for which in (0, 1):
        run(which)
    res = mux.result()
    copy()
    t_al, t_un, t_cp = [], [], []
    for _ in range(a.reps):
        t_al.append(timed(lambda: run(0)))
        t_un.append(timed(lambda: run(1)))
        t_cp.append(timed(copy))
    c = res.counters
    moved = 188 * (n_out + sum(c["consumed"]))            # bytes written and input bytes read
    floor = 376 * n_out
    med = [float(np.median(t)) for t in (t_al, t_un, t_cp)]
    print(json.dumps(dict(packets=n_out, out_bytes=n_out * 188, counters=c, floor_bytes=floor, moved_bytes=moved,
                          floor_ms_at_hbm_peak=round(floor / HBM_PEAK * 1e3, 4),
                          aligned_ms=[round(x, 4) for x in t_al], aligned_ms_median=round(med[0], 4),
                          aligned_floor_tbps=round(floor / med[0] / 1e9, 3),
                          aligned_frac_of_floor=round(floor / HBM_PEAK * 1e3 / med[0], 3),
                          unaligned_ms=[round(x, 4) for x in t_un], unaligned_ms_median=round(med[1], 4),
                          unaligned_floor_tbps=round(floor / med[1] / 1e9, 3),
                          unaligned_frac_of_floor=round(floor / HBM_PEAK * 1e3 / med[1], 3),
                          d2d_copy_ms=[round(x, 4) for x in t_cp], mux_over_copy=round(med[0] / med[2], 2),
                          time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
