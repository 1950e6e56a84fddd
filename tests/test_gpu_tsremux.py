"""GPU: the multiplexer's remux (dvbt2ll_tsmux_*_remux; classify, scan and emit kernels of csrc/tsmux_kernels.hip) against
tests/tsremux_ref.py's sequential restatement: bytes, both results and both resume positions, all exact.  Every device
run has each input inside a poisoned array of its own and its output inside a poisoned array with guard regions, at
byte alignments of its own; the guards must stay untouched."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS, ts_for_frames
from dvbt2ll.tsmux import TsRemuxPos
import mpe_cases as MC
import mpe_ref as MR
import tsmux_cases as C
import tsmux_ref as R
import tsremux_cases as XC
import tsremux_ref as X

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
_STREAM = []
_REF = {}
CASES = XC.cases()
BY_NAME = {c["name"]: c for c in CASES}


def _side_stream():
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def handle(case, max_out=None, remux=True):
    """a fresh handle: set_remux is allowed once, before the first run"""
    mux = dvbt2ll.TsMux(max_out_packets=max_out or max(case["n_out"], 1), **case["mux"])
    if remux:
        mux.set_remux(**case["remux"])
    return mux


def device_run(mux, inputs, n_out, start, rstart=None, align=(0, 0)):
    """one run_device_remux (run_device when rstart is None) with everything inside poisoned arrays; returns the
    result with ts and remux filled in, after checking the guards.  align: (the output's byte alignment, the first
    input's; input i lies at the first input's + i)"""
    import torch
    st = _side_stream()
    with torch.cuda.stream(st):
        bufs, ptrs = [], []
        for i, x in enumerate(inputs):
            buf = torch.full((2 * GUARD + len(x) + 16,), POISON, dtype=torch.uint8, device="cuda")
            at = GUARD + (align[1] + i) % 4
            if len(x):
                buf[at:at + len(x)] = torch.from_numpy(np.array(x, np.uint8)).cuda()
            bufs.append((buf, at, len(x)))
            ptrs.append(buf.data_ptr() + at if len(x) else 0)
        out = torch.full((2 * GUARD + n_out * 188 + 16,), POISON, dtype=torch.uint8, device="cuda")
        a = GUARD + align[0]
        n_in = [len(x) // 188 for x in inputs]
        if rstart is None:
            mux.run_device(ptrs, n_in, out.data_ptr() + a, n_out, start=start, stream=st.cuda_stream)
        else:
            mux.run_device_remux(ptrs, n_in, out.data_ptr() + a, n_out, start=start, rstart=rstart, stream=st.cuda_stream)
    res = mux.result()
    if rstart is not None:
        res.remux = mux.remux_result()
    st.synchronize()
    o = out.cpu().numpy()
    assert (o[:a] == POISON).all() and (o[a + n_out * 188:] == POISON).all(), "written outside its packets"
    res.ts = o[a:a + n_out * 188].copy()
    for (buf, at, n), x in zip(bufs, inputs):
        got = buf.cpu().numpy()
        assert (got[:at] == POISON).all() and (got[at + n:] == POISON).all() and (got[at:at + n] == x).all()
    return res


def reference(case):
    """computed once per case and shared"""
    if case["name"] not in _REF:
        _REF[case["name"]] = X.remux(case["inputs"], case["n_out"], start=case["start"], rstart=case["rstart"],
                                     **case["remux"], **case["mux"])
    return _REF[case["name"]]


def same(res, ref, rref, ctx=""):
    assert tuple(res.resume) == tuple(ref.resume), (ctx, res.resume, ref.resume)
    assert res.counters == ref.counters, (ctx, res.counters, ref.counters)
    assert tuple(res.remux.resume) == tuple(rref.resume), (ctx, res.remux.resume, rref.resume)
    assert res.remux.counters == rref.counters, (ctx, res.remux.counters, rref.counters)
    np.testing.assert_array_equal(res.ts, ref.ts, err_msg=str(ctx))


# ---------------------------------------------------------------------------------------- every case of tsremux_cases
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_equals_the_reference(gpu, case):
    """remap (two inputs on one PID mapped apart, two PIDs onto one, a drop, an entry that never matches, a bad-sync
    packet on a mapped PID); continuity (a carousel over 17 laps, 64 PIDs, packets without payload at the call's and a
    tile's first and last packet, a PID absent from a tile, one tile, one tile + 1, a second scan round, start
    counters of 15, an input that is not restamped on a tracked PID); PCR (exact PCRs from phase 5 with either mux
    clock, the wrap of W, in_period 1 and 65536, short and empty adaptation fields, the fill input, a loop input)"""
    ref, rref = reference(case)
    k = CASES.index(case)
    same(device_run(handle(case), case["inputs"], case["n_out"], case["start"], TsRemuxPos(*case["rstart"]),
                    align=(k % 4, (k // 4) % 4)), ref, rref, case["name"])
    if case["name"] == "remap":
        # input 0 has 2 of 5 slots, 28 of the 70: its packets 4, 11, 18 and 25 are the dropped ones
        assert rref.counters["dropped"] == 4 and ref.counters["sync_errors"] == 1 and rref.counters["remapped"] > 20
    if case["name"] == "carousel":
        assert ref.counters["consumed"][1] > 17 * 3
    if case["name"] == "second scan round":
        assert (case["n_out"] + XC.TILE - 1) // XC.TILE > XC.SCAN_TILES and rref.counters["pcr_restamped"] > 1000
    if case["name"] == "tiles 64":
        assert rref.counters["cc_rewritten"] > 32


def test_a_remux_that_does_nothing_gives_the_plain_handles_bytes(gpu):
    case = BY_NAME["all three"]
    plain = device_run(handle(case, remux=False), case["inputs"], 200, case["start"], align=(1, 2))
    same_as = dvbt2ll.TsMux(max_out_packets=200, **case["mux"])
    same_as.set_remux()
    got = device_run(same_as, case["inputs"], 200, case["start"], TsRemuxPos(), align=(2, 1))
    np.testing.assert_array_equal(got.ts, plain.ts)
    np.testing.assert_array_equal(plain.ts, R.mux(case["inputs"], 200, start=case["start"], **case["mux"]).ts)
    assert got.counters == plain.counters and got.resume == plain.resume
    assert got.remux.counters == dict.fromkeys(X.REMUX_COUNTERS, 0) and got.remux.resume == TsRemuxPos()


def _sum(parts):
    return {k: sum(p[k] for p in parts) if not isinstance(parts[0][k], tuple) else
            tuple(sum(v) for v in zip(*[p[k] for p in parts])) for k in parts[0]}


def test_splits_chain_to_the_single_call(gpu):
    case = BY_NAME["all three"]
    ref, rref = reference(case)
    mux = handle(case)
    ins, start, rstart = case["inputs"], case["start"], TsRemuxPos(*case["rstart"])
    for k in range(201):
        a = device_run(mux, ins, k, start, rstart, align=(k % 4, 0))
        b = device_run(mux, ins, 200 - k, a.resume, a.remux.resume, align=(0, k % 4))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), ref.ts, err_msg=str(k))
        assert tuple(b.resume) == tuple(ref.resume) and tuple(b.remux.resume) == tuple(rref.resume), k
        assert _sum([a.counters, b.counters]) == ref.counters, k
        assert _sum([a.remux.counters, b.remux.counters]) == rref.counters, k
    parts, pos, rpos = [], start, rstart
    for n in (63, 64, 73):
        parts.append(device_run(mux, ins, n, pos, rpos, align=(n % 4, 2)))
        pos, rpos = parts[-1].resume, parts[-1].remux.resume
    np.testing.assert_array_equal(np.concatenate([p.ts for p in parts]), ref.ts)
    assert tuple(pos) == tuple(ref.resume) and tuple(rpos) == tuple(rref.resume)
    assert _sum([p.remux.counters for p in parts]) == rref.counters


def test_every_output_alignment_against_every_input_alignment(gpu):
    case = BY_NAME["all three"]
    ref, rref = reference(case)
    mux = handle(case)
    for ao in range(4):
        for ai in range(4):
            same(device_run(mux, case["inputs"], 200, case["start"], TsRemuxPos(*case["rstart"]), align=(ao, ai)), ref,
                 rref, (ao, ai))


def test_run_host_and_refusals_launch_nothing(gpu):
    import torch
    case = BY_NAME["all three"]
    ref, rref = reference(case)
    mux = handle(case)
    ins, start, rstart = case["inputs"], case["start"], TsRemuxPos(*case["rstart"])
    same(mux.run_host_remux(ins, 200, start=start, rstart=rstart), ref, rref, "host")
    with pytest.raises(dvbt2ll.DVBT2Error):
        mux.set_remux()                                                       # after a run, and a second time
    d = [torch.from_numpy(x.copy()).cuda() for x in ins]
    out = torch.full((200 * 188,), POISON, dtype=torch.uint8, device="cuda")
    P, N, Q = [x.data_ptr() for x in d], [len(x) // 188 for x in ins], out.data_ptr()
    with pytest.raises(dvbt2ll.DVBT2Error):
        mux.run_device(P, N, Q, 8, start=start)                               # the plain calls on a remux handle
    with pytest.raises(dvbt2ll.DVBT2Error):
        mux.run_host(ins, 8, start=start)
    bad = [rstart._replace(cc=(16,) + (0,) * 63), rstart._replace(cc=(0, 0, 0, 1) + (0,) * 60),   # past n_track
           rstart._replace(cc=(-1,) + (0,) * 63), rstart._replace(in_phase=(5,) + (0,) * 7),
           rstart._replace(in_phase=(0, 1) + (0,) * 6), rstart._replace(in_ticks=(X.W,) + (0,) * 7),
           rstart._replace(in_ticks=(0, 1) + (0,) * 6)]
    for r in bad:
        with pytest.raises(dvbt2ll.DVBT2Error):
            mux.run_device_remux(P, N, Q, 8, start=start, rstart=r)
    # the 2^62 bound: 2^31 - 1 packets of an input whose every packet lasts 2^36 - 1 ticks
    big = dvbt2ll.TsMux(period=1, weight=[1], max_out_packets=8)
    big.set_remux(in_period=[1], in_ticks_per_period=[(1 << 36) - 1])
    with pytest.raises(dvbt2ll.DVBT2Error):
        big.run_device_remux(P[:1], [(1 << 31) - 1], Q, 8)
    big.run_device_remux(P[:1], [(1 << 26) - 1], Q, 0)                        # 2^26 x (2^36 - 1) < 2^62
    plain = dvbt2ll.TsMux(period=1, weight=[1], max_out_packets=8)
    with pytest.raises(dvbt2ll.DVBT2Error):
        plain.run_device_remux(P[:1], N[:1], Q, 8)                            # no remux was set
    with pytest.raises(dvbt2ll.DVBT2Error):
        plain.remux_result()
    plain.run_device(P[:1], N[:1], Q + 188 * 100, 1)
    with pytest.raises(dvbt2ll.DVBT2Error):
        plain.set_remux()                                                     # after a run
    torch.cuda.synchronize()
    assert bool((out[:188 * 100] == POISON).all())
    after = mux.remux_result()
    assert after.counters == rref.counters and tuple(after.resume) == tuple(rref.resume)   # the last real run's stands


# ---------------------------------------------------------------------------------------- end to end
def _pdus_for(nbytes, seed):
    rng = np.random.default_rng(seed)
    pdus, total = [], 0
    while total < nbytes:
        L = int(rng.choice([40, 64, 200, 576, 1500]))
        pdus.append(MC.ip(L, len(pdus), 0x60 if len(pdus) % 4 == 1 else 0x45))
        total += L + 16
    return pdus


def test_two_mpe_streams_on_one_pid_and_a_short_carousel_end_to_end(gpu):
    """two MpeEncapsulators left on one PID, remapped apart, and a carousel of one round of PAT + PMT + PMT (3 packets,
    so its counters break at every lap unless restamped), all on the device; the checker finds every section whole and
    the continuity unbroken, the MPE receiver recovers every datagram of both, and a ModeAdapter per PID makes the
    BBFRAMEs it makes of the reference's TS"""
    import torch
    pid, pids = 0x101, (0x201, 0x202)
    programs = [dict(program_number=1 + k, pmt_pid=0x30 + k, streams=[dict(stream_type=0x0D, pid=pids[k])]) for k in range(2)]
    psi = dvbt2ll.psi_build(9, 3, programs)[:3 * 188]
    pdus = [_pdus_for(30000, 41), _pdus_for(20000, 42)]
    n_out = 400
    kw = dict(period=20, weight=(9, 7, 1), loop=(0, 0, 1), fill_input=-1, pcr_pid=-1, pcr_weight=0, ticks_per_period=0)
    rx = dict(map=[(0, pid, pids[0]), (1, pid, pids[1])], track_pid=(0, 0x30, 0x31) + pids, restamp_cc=(1, 1, 1))
    mux = dvbt2ll.TsMux(max_out_packets=n_out, **kw)
    mux.set_remux(**rx)
    st = _side_stream()
    with torch.cuda.stream(st):
        ts_d, n_ts, refs = [], [], []
        for k in range(2):
            pdu, off = MR.pack(pdus[k])
            refs.append(MR.encap(pdu, off, pid=pid, flush=True, crc=MR.crc32_table))
            enc = dvbt2ll.MpeEncapsulator(pid=pid, max_pdu_bytes=len(pdu), max_pdus=len(pdus[k]))
            cap = enc.packet_bound(len(pdu), len(pdus[k]))
            pdu_d, off_d = torch.from_numpy(pdu).cuda(), torch.from_numpy(off.view(np.int32)).cuda()
            t = torch.zeros(cap * 188, dtype=torch.uint8, device="cuda")
            enc.run_device(pdu_d.data_ptr(), len(pdu), off_d.data_ptr(), len(pdus[k]), t.data_ptr(), cap, flush=True,
                           stream=st.cuda_stream)
            ts_d.append(t)
            n_ts.append(refs[k].counters["ts_packets"])
        psi_d = torch.from_numpy(psi).cuda()
        out = torch.zeros(n_out * 188, dtype=torch.uint8, device="cuda")
        mux.run_device_remux([ts_d[0].data_ptr(), ts_d[1].data_ptr(), psi_d.data_ptr()], n_ts + [3], out.data_ptr(), n_out,
                             stream=st.cuda_stream)
        ads, bbs = [], []
        for k in range(2):
            ad = dvbt2ll.ModeAdapter(framesize=0, rate=0, kbch=7032, pids=[pids[k]], max_ts_bytes=n_out * 188)
            cap_bb = n_out * 188 // ad.D + 1
            bb = torch.zeros(cap_bb * ad.L, dtype=torch.uint8, device="cuda")
            ad.run_device(out.data_ptr(), n_out * 188, bb.data_ptr(), cap_bb, flush=True, stream=st.cuda_stream)
            ads.append(ad)
            bbs.append(bb)
    res = mux.result()
    res.remux = mux.remux_result()
    st.synchronize()
    ref, rref = X.remux([refs[0].ts, refs[1].ts, psi], n_out, **rx, **kw)
    res.ts = out.cpu().numpy()
    same(res, ref, rref, "end to end")
    assert ref.counters["consumed"][:2] == tuple(n_ts) and ref.counters["consumed"][2] == 20 and rref.counters["cc_rewritten"] > 0
    chk = R.check_ts(res.ts, cc={0: 0, 0x30: 0, 0x31: 0, pids[0]: 0, pids[1]: 0})       # every section whole, every PID continuous
    X.check_continuity(res.ts, first={p: 0 for p in rx["track_pid"]})
    assert chk["pat"] == dict(tsid=9, version=3, programs=[(1, 0x30), (2, 0x31)]) and pid not in chk["pids"]
    found = [chk["pmts"][n]["streams"] for n in (1, 2)]
    assert found == [[(0x0D, pids[0], b"")], [(0x0D, pids[1], b"")]]
    for k in range(2):
        assert [d for _, d in MR.receive(res.ts, pids[k], 0, MR.crc32_table)] == pdus[k]
        got, want = ads[k].result(), ads[k].run(ref.ts, flush=True)
        assert got.counters == want.counters and want.counters["bbframes"] > 0
        np.testing.assert_array_equal(bbs[k].cpu().numpy()[:len(want.bbframes)], want.bbframes)


TOOL = Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "dvbt2ll" / "dvbt2ll_tx"


def test_cli_mux_with_remap_and_restamp_cc(gpu, tmp_path):
    """dvbt2ll_tx --input mpe --mux ...,remap=0x321:0x322,restamp-cc: the counters printed are the reference's summed over
    the tool's calls (whole periods, 8192 slots or more, each on the next window of the encapsulated TS and from the
    last call's two resume positions), and the PMT names the remapped PID"""
    cfg = CONFIGS["cfg1q"]
    pdus = _pdus_for(len(ts_for_frames(cfg, 0, 1)[0]), 43)
    pdu, off = MR.pack(pdus)
    enc = MR.encap(pdu, off, pid=0x321, flush=True, crc=MR.crc32_table).ts
    (tmp_path / "in.mpe").write_bytes(b"".join(len(p).to_bytes(2, "big") + p for p in pdus))
    P, per_call = 12, 12 * (8192 // 12)
    psi = R.psi(1, 0, [dict(program_number=5, pmt_pid=0x44, pcr_pid=0x1FFF, streams=[dict(stream_type=0x90, pid=0x322)])])
    kw = dict(period=P, weight=(8, 1), loop=(0, 1), fill_input=0)
    rx = dict(map=[(0, 0x321, 0x322)], track_pid=(0x322, 0, 0x44), restamp_cc=(1, 1))
    used, pos, rpos, tot, out = 0, (0, 0, (0,) * 8), X.RSTART, dict.fromkeys(X.REMUX_COUNTERS, 0), []
    while used < len(enc) // 188:
        ref, rref = X.remux([enc[used * 188:(used + per_call) * 188], psi], per_call, start=(pos[0], pos[1], (0,) + pos[2][1:]),
                            rstart=rpos, **rx, **kw)
        used, pos, rpos = used + ref.counters["consumed"][0], ref.resume, rref.resume
        tot = {k: tot[k] + rref.counters[k] for k in tot}
        out.append(ref.ts)
    chk = R.check_ts(np.concatenate(out), cc={0: 0, 0x44: 0, 0x322: 0})
    assert chk["pmts"][5]["streams"] == [(0x90, 0x322, b"")] and 0x321 not in chk["pids"]
    r = subprocess.run([str(TOOL), "--preset", "cfg1q", "--input", "mpe", "--pid", "0x321", "--mux",
                        "period=12,weight=8,psi-weight=1,remap=0x321:0x322,restamp-cc", "--program", "5", "--pmt-pid", "0x44",
                        "--stream-type", "0x90", "--in", str(tmp_path / "in.mpe"), "--out", str(tmp_path / "b.iq"),
                        "--batch", "1", "--frames", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert ("remux: remapped %d, dropped 0, cc_rewritten %d, pcr_restamped 0" % (tot["remapped"], tot["cc_rewritten"])) in r.stderr, r.stderr
    # the encapsulator's counters and the 16-round carousel's are right as they come, so restamping rewrites none
    assert tot["remapped"] == len(enc) // 188 and tot["cc_rewritten"] == 0
