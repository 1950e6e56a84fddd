#!/usr/bin/env python3
"""MPE-FEC-encapsulator timing, by tools/mpe_measure.py's method: encapsulating the PDUs that fill
the TS of N frames of a configuration with the MPE-FEC handle, beside the plain MPE handle on the same datagrams (it is
the yardstick for what FEC adds) and the chain's stage times for that TS, the arms alternating, all in one process.
Run three processes and put the outputs next to each other.

  python tools/mpefec_measure.py --cfg cfg3 --frames 160 --pdu-bytes 1500 --rows 1024 --reps 5

Before anything is timed, a call on the first --check-pdus PDUs is compared whole (bytes, counters, resume position)
with tests/mpefec_ref.py's sequential encapsulator.  The events are recorded on the stream the handles run on.  Prints
one JSON line."""
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
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--pdu-bytes", type=int, default=1500)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--data-columns", type=int, default=191)
    ap.add_argument("--rs-columns", type=int, default=64)
    ap.add_argument("--check-pdus", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import dvbt2ll
    from dvbt2ll.configs import CONFIGS, ts_for_frames
    import mpefec_ref as R

    assert torch.cuda.is_available(), "needs a GPU"
    cfg = CONFIGS[a.cfg]
    need = len(ts_for_frames(cfg, 0, a.frames)[0])          # TS bytes of the frames
    L, rows, D, K = a.pdu_bytes, a.rows, a.data_columns, a.rs_columns
    # datagram bytes whose sections and RS columns fill them: a frame of D x rows bytes sends K x (rows + 16) more
    share = (L + 16) / L + K * (rows + 16) / (D * rows)
    npdu = int(need / 188 * 184 / share / L) + 2 * (D * rows // L) + 2
    rng = np.random.default_rng(7)
    pdu1 = rng.integers(0, 256, npdu * L, dtype=np.uint8)
    pdu1[::L] = 0x45
    off1 = (np.arange(npdu + 1, dtype=np.uint64) * L).astype(np.uint32)
    frames = npdu // (D * rows // L) + 2
    fec = dvbt2ll.MpeFecEncapsulator(pid=0x100, rows=rows, data_columns=D, rs_columns=K, max_pdu_bytes=len(pdu1),
                                     max_pdus=npdu, max_frames=frames)
    mpe = dvbt2ll.MpeEncapsulator(pid=0x100, max_pdu_bytes=len(pdu1), max_pdus=npdu)
    cap = fec.packet_bound(len(pdu1), npdu)
    pdu = torch.from_numpy(pdu1).cuda()
    off = torch.from_numpy(off1.view(np.int32)).cuda()
    out = torch.zeros(cap * 188, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros(cap * 188, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    torch.cuda.set_stream(side)
    st = torch.cuda.current_stream().cuda_stream
    assert st != 0

    def run_fec():
        fec.run_device(pdu.data_ptr(), len(pdu1), off.data_ptr(), npdu, out.data_ptr(), cap, flush=True, stream=st)

    def run_mpe():
        mpe.run_device(pdu.data_ptr(), len(pdu1), off.data_ptr(), npdu, out2.data_ptr(), cap, flush=True, stream=st)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    k = min(a.check_pdus, npdu)
    ref = R.encap(pdu1[:k * L], off1[:k + 1], rows=rows, D=D, K=K, pid=0x100, max_frames=frames, flush=True)
    fec.run_device(pdu.data_ptr(), k * L, off.data_ptr(), k, out.data_ptr(), cap, flush=True, stream=st)
    res = fec.result()
    got = out[:res.counters["ts_packets"] * 188].cpu().numpy()
    assert np.array_equal(got, ref.ts) and res.counters == ref.counters and tuple(res.resume) == ref.resume
    run_fec()
    res = fec.result()
    assert res.counters["sections"] == npdu and res.counters["flushed"] == 1, res
    packets = res.counters["ts_packets"]
    assert packets * 188 >= need, (packets * 188, need)
    run_mpe()
    mres = mpe.result()
    t_fec, t_mpe = [], []
    for _ in range(a.reps):
        t_fec.append(timed(run_fec))
        t_mpe.append(timed(run_mpe))
    ch = dvbt2ll.Chain(cfg, max_frames=a.frames)
    iq = torch.empty((a.frames * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
    ch.run_device(out.data_ptr(), 0, packets * 188, 0, a.frames, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ch.set_timing(True)
    for _ in range(a.reps):
        ch.run_device(out.data_ptr(), 0, packets * 188, 0, a.frames, iq.data_ptr(), st)
    torch.cuda.synchronize()
    ms, _ = ch.timing()
    stages = dict(fec=ms[0] / a.reps, map=ms[1] / a.reps, ofdm=ms[2] / a.reps)
    med, medm = float(np.median(t_fec)), float(np.median(t_mpe))
    total = packets * 188
    # the RS pass's floors: it reads D and writes K bytes per row, and reads 191 x 64 LDS bytes per row
    nrows = res.counters["frames"] * rows
    print(json.dumps(dict(cfg=a.cfg, frames=a.frames, pdu_bytes=L, rows=rows, data_columns=D, rs_columns=K, pdus=npdu,
                          fec_frames=res.counters["frames"], ts_bytes=total, mpe_ts_bytes=mres.counters["ts_packets"] * 188,
                          mpefec_ms=[round(x, 4) for x in t_fec], mpefec_ms_median=round(med, 4),
                          mpefec_gbps=round(total / med / 1e6, 2), mpe_ms=[round(x, 4) for x in t_mpe],
                          mpe_ms_median=round(medm, 4), fec_adds_ms=round(med - medm, 4),
                          rs_bytes=nrows * (D + K), rs_lds_read_bytes=nrows * 191 * 64,
                          chain_stage_ms_for_frames={k: round(v, 4) for k, v in stages.items()},
                          mpefec_over_slowest_stage=round(med / max(stages.values()), 3),
                          time=time.strftime("%Y-%m-%d %H:%M:%S"))))


if __name__ == "__main__":
    main()
