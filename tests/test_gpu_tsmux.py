"""GPU: the TS multiplexer (dvbt2ll_tsmux_*, csrc/tsmux_kernels.hip) against tests/tsmux_ref.py's sequential
restatement: bytes, counters and resume position, all exact.  Every device run here has each input inside a poisoned
array of its own and its output inside a poisoned array with guard regions, at byte alignments of its own; the guards
must stay untouched."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS, ts_for_frames
import mpe_cases as MC
import mpe_ref as MR
import tsmux_cases as C
import tsmux_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
PKTS = 64             # TSMUX_PKTS of csrc/tsmux_kernels.h: output packets per workgroup trip
MAX_BLOCKS = 2048     # TSMUX_MAX_BLOCKS of csrc/tsmux_kernels.h: the grid's cap; past MAX_BLOCKS x PKTS packets a
#                       workgroup takes a second trip
START = (0, 0, (0,) * 8)

_STREAM = []


def _side_stream():
    """a torch stream with a handle of its own (torch's default stream has handle 0, which the C ABI reads as "the
    handle's own stream")"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def device_run(mux, inputs, n_out, start=START, align=(0, 0)):
    """one run_device with everything inside poisoned arrays; returns the result with ts filled in, after checking the
    guards.  align: (the output's byte alignment, the first input's; input i lies at the first input's + i)"""
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
        mux.run_device(ptrs, [len(x) // 188 for x in inputs], out.data_ptr() + a, n_out, start=start,
                       stream=st.cuda_stream)
    res = mux.result()
    st.synchronize()
    o = out.cpu().numpy()
    assert (o[:a] == POISON).all() and (o[a + n_out * 188:] == POISON).all(), "written outside its packets"
    res.ts = o[a:a + n_out * 188].copy()
    for (buf, at, n), x in zip(bufs, inputs):
        got = buf.cpu().numpy()
        assert (got[:at] == POISON).all() and (got[at + n:] == POISON).all() and (got[at:at + n] == x).all()
    return res


def same(res, ref, ctx=""):
    assert tuple(res.resume) == tuple(ref.resume), (ctx, res.resume, ref.resume)
    assert res.counters == ref.counters, (ctx, res.counters, ref.counters)
    np.testing.assert_array_equal(res.ts, ref.ts, err_msg=str(ctx))


_MUX = {}


def mux_of(period, weight, loop=None, fill_input=-1, pcr_pid=-1, pcr_weight=0, ticks_per_period=0, max_out=1 << 12):
    """one handle per parameter set, shared by the tests (a handle holds tables only); returns it with the reference's
    keyword arguments"""
    kw = dict(period=period, weight=tuple(weight), loop=tuple(loop or [0] * len(weight)), fill_input=fill_input,
              pcr_pid=pcr_pid, pcr_weight=pcr_weight, ticks_per_period=ticks_per_period)
    key = tuple(kw.values()) + (max_out,)
    if key not in _MUX:
        _MUX[key] = dvbt2ll.TsMux(max_out_packets=max_out, **kw)
    return _MUX[key], kw


def check(mk, inputs, n_out, ctx, start=START, align=(0, 0)):
    mux, kw = mk
    ref = R.mux(inputs, n_out, start=start, **kw)
    res = device_run(mux, inputs, n_out, start=start, align=align)
    same(res, ref, ctx)
    return res, ref


# ---------------------------------------------------------------------------------------- 1. schedules
def test_identity(gpu):
    mk = mux_of(1, (1,))
    a = C.stream(5, 0x101)
    for n_out in (1, 5):
        res, _ = check(mk, [a], n_out, n_out, align=(n_out % 4, 1))
        np.testing.assert_array_equal(res.ts, a[:n_out * 188])
    np.testing.assert_array_equal(mk[0].schedule(), [0])
    res, ref = check(mk, [a], 0, "no slot", start=(0, 7, (2,) + (0,) * 7))
    assert res.resume == (0, 7, (2,) + (0,) * 7)


@pytest.mark.parametrize("short", ["sufficient", "short by one", "empty"])
def test_weighted_schedule_from_phase_five(gpu, short):
    """P = 7, weights 3 and 2, 3 P + 4 slots from phase 5: input 0 owns 11 of them and input 1 seven, the last one of
    input 1 being the call's very last slot"""
    mk = mux_of(7, (3, 2))
    np.testing.assert_array_equal(mk[0].schedule(), R.schedule(7, (3, 2)))
    n_out = 3 * 7 + 4
    table = np.tile(R.schedule(7, (3, 2)), 5)[5:5 + n_out]
    own = [int((table == e).sum()) for e in (0, 1)]
    assert own == [11, 7] and table[-1] == 1
    n1 = {"sufficient": own[1], "short by one": own[1] - 1, "empty": 0}[short]
    ins = [C.stream(own[0], 0x101), C.stream(n1, 0x102)]
    res, ref = check(mk, ins, n_out, short, start=(5, 0, (0,) * 8), align=(1, 2))
    assert ref.counters["dry_slots"] == (0, own[1] - n1) and ref.counters["consumed"] == (own[0], n1)
    if short == "short by one":
        np.testing.assert_array_equal(res.ts[-188:], R.NULL)     # the single dry slot at the very end


def test_fill_takes_nulls_and_dry_slots_then_runs_dry(gpu):
    """P = 10, weights 2 and 3 and five null slots; input 1 dries up after 4 packets; the fill input 0 takes the null
    slots and input 1's dry ones until, mid-call, it has nothing left either.  Then the same with the fill input's
    weight 0"""
    for w0, align in ((2, (2, 3)), (0, (3, 1))):
        mk = mux_of(10, (w0, 3), fill_input=0)
        ins = [C.stream(31, 0x101), C.stream(4, 0x102)]
        res, ref = check(mk, ins, 53, w0, start=(3, 0, (0,) * 8), align=align)
        c = ref.counters
        assert c["consumed"] == (31, 4) and c["fill_in_free"] > 0 and c["dry_slots"][1] > 0 and c["null_packets"] > 0
        assert (c["dry_slots"][0] > 0) == (w0 > 0)
        last_fill = max(k for k in range(53) if res.ts[188 * k + 2] == 0x01)
        assert last_fill < 45                                    # it ran dry mid-call: only null packets follow
        # from a position inside the inputs
        check(mk, ins, 30, (w0, "offset"), start=(9, 0, (5, 2) + (0,) * 6), align=align[::-1])


def test_loop_reads_the_carousel_round_and_round(gpu):
    """a carousel of 3 packets under weight 2 of P = 5, read from next = 2 across more than 16 laps; then an empty one,
    whose slots go to the fill input"""
    mk = mux_of(5, (2, 2), loop=(0, 1), fill_input=0)
    ins = [C.stream(70, 0x101), C.stream(3, 0x102)]
    res, ref = check(mk, ins, 130, "loop", start=(1, 0, (0, 2) + (0,) * 6), align=(1, 0))
    assert ref.counters["consumed"][1] == 52 > 16 * 3 and ref.resume[2][1] == (2 + 52) % 3
    # next = n_in is a position too: the carousel's first packet
    check(mk, ins, 17, "loop from its end", start=(4, 0, (1, 3) + (0,) * 6), align=(2, 2))
    res, ref = check(mk, [ins[0], np.zeros(0, np.uint8)], 40, "empty loop", start=(2, 0, (3,) + (0,) * 7), align=(3, 1))
    assert ref.counters["dry_slots"] == (0, 16) and ref.counters["consumed"] == (40, 0) and ref.resume[2][1] == 0


def test_pcr_wraps_inside_the_call(gpu):
    """pcr_weight 2 in P = 10, 1003 ticks per period (not divisible by P), the clock 5 ticks before its wrap: the PCRs
    rise by the slots' ticks modulo W"""
    mk = mux_of(10, (3,), pcr_pid=0x1ABC, pcr_weight=2, ticks_per_period=1003)
    table = R.schedule(10, (3,), 2)
    res, ref = check(mk, [C.stream(20, 0x101)], 47, "pcr", start=(4, R.W - 5, (0,) * 8), align=(2, 1))
    chk = R.check_ts(res.ts, cc={0x101: 0})
    assert len(chk["pcrs"]) == ref.counters["pcr_packets"] == sum(table[(4 + m) % 10] == 1 for m in range(47))
    for k, pid, ticks in chk["pcrs"]:
        dc, t = divmod(4 + k, 10)
        assert pid == 0x1ABC and ticks == (R.W - 5 + dc * 1003 + t * 1003 // 10) % R.W
    ticks = [t for _, _, t in chk["pcrs"]]
    assert ticks[0] == 596 and all((b - a) % R.W in (501, 502) for a, b in zip(ticks, ticks[1:]))
    assert res.resume[1] == (R.W - 5 + 5 * 1003) % R.W == 5 * 1003 - 5
    # with nothing but a weightless fill input the PCR generator owns table slot 0: a PCR before the wrap, one after
    mk = mux_of(10, (0,), fill_input=0, pcr_pid=0x1ABC, pcr_weight=2, ticks_per_period=1003)
    res, ref = check(mk, [C.stream(20, 0x101)], 12, "pcr, wrap between two", start=(0, R.W - 5, (0,) * 8), align=(0, 3))
    assert [t for _, _, t in R.check_ts(res.ts)["pcrs"]] == [R.W - 5, 496, 998]
    # the largest clock arithmetic: P = 1, the most periods a call can pass, the largest ticks_per_period
    mk = mux_of(1, (0,), fill_input=0, pcr_pid=0, pcr_weight=1, ticks_per_period=(1 << 36) - 1, max_out=1 << 13)
    check(mk, [np.zeros(0, np.uint8)], 1 << 13, "pcr only", start=(0, R.W - 1, (0,) * 8), align=(1, 0))


def test_sync_errors_become_null_packets(gpu):
    mk = mux_of(4, (2, 1), fill_input=1)
    a, b = C.stream(9, 0x101), C.stream(9, 0x102)
    a[188 * 3] = 0x48
    b[188 * 5] = 0x00
    res, ref = check(mk, [a, b], 22, "sync", align=(3, 3))
    assert ref.counters["sync_errors"] == 2 and ref.counters["consumed"] == (9, 9)
    assert ref.counters["null_packets"] == 22 - 18 + 2


def test_every_output_alignment_against_every_input_alignment(gpu):
    """two inputs one byte apart in alignment, a PCR and null packets, a cut of 67 packets: a whole group of 64 and a
    short one"""
    mk = mux_of(9, (4, 2), fill_input=-1, pcr_pid=0x1F0, pcr_weight=1, ticks_per_period=90001)
    ins = [C.stream(40, 0x101), C.stream(12, 0x102)]
    ref = R.mux(ins, 67, start=(2, 12345, (1, 0) + (0,) * 6), **mk[1])
    for ao in range(4):
        for ai in range(4):
            same(device_run(mk[0], ins, 67, start=(2, 12345, (1, 0) + (0,) * 6), align=(ao, ai)), ref, (ao, ai))


def test_splits_chain_to_the_single_call(gpu):
    mk = mux_of(10, (0, 3, 2), loop=(0, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=2, ticks_per_period=1003)
    ins = [C.stream(70, 0x101), C.stream(40, 0x102), C.stream(16, 0x103)]
    ins[1][188 * 7] = 0x46
    start = (7, R.W - 2500, (0, 0, 2) + (0,) * 5)
    whole, _ = check(mk, ins, 200, "whole", start=start, align=(1, 1))
    assert whole.counters["consumed"][:2] == (70, 40) and whole.counters["dry_slots"][1] > 0

    def add(parts):
        tot = {k: sum(p.counters[k] for p in parts) for k in R.COUNTERS}
        for k in ("consumed", "dry_slots"):
            tot[k] = tuple(sum(v) for v in zip(*[p.counters[k] for p in parts]))
        return tot

    for k in range(201):
        a = device_run(mk[0], ins, k, start=start, align=(k % 4, 0))
        b = device_run(mk[0], ins, 200 - k, start=a.resume, align=(0, k % 4))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts, err_msg=str(k))
        assert b.resume == whole.resume and add([a, b]) == whole.counters, k
    parts, pos = [], start
    for n in (63, 64, 73):
        parts.append(device_run(mk[0], ins, n, start=pos, align=(n % 4, 2)))
        pos = parts[-1].resume
    np.testing.assert_array_equal(np.concatenate([p.ts for p in parts]), whole.ts)
    assert pos == whole.resume and add(parts) == whole.counters


def test_past_the_grid_cap_with_the_largest_table(gpu):
    """MAX_BLOCKS x PKTS + PKTS + 7 slots of P = 65536: the workgroups past the cap take a second trip, the last one a
    short one, and the prefix table is at its largest"""
    n_out = MAX_BLOCKS * PKTS + PKTS + 7
    mk = mux_of(65536, (0, 30000, 4097), loop=(0, 0, 1), fill_input=0, pcr_pid=0x1FF, pcr_weight=513,
                ticks_per_period=(1 << 30) + 7, max_out=n_out)
    ins = [C.stream(60000, 0x101), C.stream(50000, 0x102), C.stream(16, 0x103)]
    res, ref = check(mk, ins, n_out, "grid", start=(65000, 5, (10, 20, 3) + (0,) * 5), align=(3, 2))
    c = ref.counters
    assert c["consumed"][0] == 60000 - 10 and c["dry_slots"][1] > 0 and c["null_packets"] > 0 and c["pcr_packets"] > 1000
    np.testing.assert_array_equal(mk[0].schedule(), R.schedule(65536, (0, 30000, 4097), 513))


def test_run_host_and_refusals_launch_nothing(gpu):
    import torch
    mux, kw = mux_of(7, (3, 2), fill_input=1, max_out=64)
    ins = [C.stream(11, 0x101), C.stream(30, 0x102)]
    same(mux.run_host(ins, 40, start=(5, 0, (1, 2) + (0,) * 6)), R.mux(ins, 40, start=(5, 0, (1, 2) + (0,) * 6), **kw), "host")
    before = mux.result()
    d = [torch.from_numpy(x.copy()).cuda() for x in ins]
    out = torch.full((64 * 188,), POISON, dtype=torch.uint8, device="cuda")
    P, N, Q = [x.data_ptr() for x in d], [11, 30], out.data_ptr()
    for args, start in ((([0, P[1]], N, Q, 8), START),                    # a null pointer where n_in > 0
                        ((P, N, 0, 8), START),
                        ((P, N, Q, 65), START),                           # above max_out_packets
                        ((P, N, Q, -1), START),
                        ((P, [-1, 30], Q, 8), START),
                        ((P, [11, 1 << 31], Q, 8), START),
                        ((P, N, Q, 8), (7, 0, (0,) * 8)),                 # phase >= P
                        ((P, N, Q, 8), (-1, 0, (0,) * 8)),
                        ((P, N, Q, 8), (0, R.W, (0,) * 8)),               # pcr_ticks >= W
                        ((P, N, Q, 8), (0, -1, (0,) * 8)),
                        ((P, N, Q, 8), (0, 0, (12, 0) + (0,) * 6)),       # next outside [0, n_in]
                        ((P, N, Q, 8), (0, 0, (0, -1) + (0,) * 6))):
        with pytest.raises(dvbt2ll.DVBT2Error):
            mux.run_device(*args, start=start)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    after = mux.result()
    assert after.counters == before.counters and after.resume == before.resume    # the last real run's result stands
    mux.run_device([0, P[1]], [0, 30], Q, 8)                                          # a null pointer with n_in = 0 is fine
    assert mux.result().counters["consumed"] == (0, 8)


# ---------------------------------------------------------------------------------------- 2. end to end
def _pdus_for(nbytes, seed):
    rng = np.random.default_rng(seed)
    pdus, total = [], 0
    while total < nbytes:
        L = int(rng.choice([40, 64, 200, 576, 1500]))
        pdus.append(MC.ip(L, len(pdus), 0x60 if len(pdus) % 4 == 1 else 0x45))
        total += L + 16
    return pdus


def test_two_mpe_streams_and_a_carousel_end_to_end(gpu):
    """two MpeEncapsulator outputs on different PIDs and a psi_build carousel through the mux, everything on the
    device; the checker finds both PIDs through PAT -> PMT, the MPE receiver recovers every datagram of both, and a
    ModeAdapter with a PID mask turns one of them into the BBFRAMEs it makes of the reference multiplexer's output"""
    import torch
    pids = (0x101, 0x102)
    programs = [dict(program_number=1 + k, pmt_pid=0x30 + k, streams=[dict(stream_type=0x0D, pid=pids[k])]) for k in range(2)]
    psi = dvbt2ll.psi_build(9, 3, programs)
    pdus = [_pdus_for(30000, 31), _pdus_for(20000, 32)]
    st = _side_stream()
    with torch.cuda.stream(st):
        ts_d, n_ts, refs = [], [], []
        for k in range(2):
            pdu, off = MR.pack(pdus[k])
            refs.append(MR.encap(pdu, off, pid=pids[k], flush=True, crc=MR.crc32_table))
            enc = dvbt2ll.MpeEncapsulator(pid=pids[k], max_pdu_bytes=len(pdu), max_pdus=len(pdus[k]))
            cap = enc.packet_bound(len(pdu), len(pdus[k]))
            pdu_d, off_d = torch.from_numpy(pdu).cuda(), torch.from_numpy(off.view(np.int32)).cuda()
            t = torch.zeros(cap * 188, dtype=torch.uint8, device="cuda")
            enc.run_device(pdu_d.data_ptr(), len(pdu), off_d.data_ptr(), len(pdus[k]), t.data_ptr(), cap, flush=True,
                           stream=st.cuda_stream)
            ts_d.append(t)
            n_ts.append(refs[k].counters["ts_packets"])      # the packet counts are the reference's: no round trip
        psi_d = torch.from_numpy(psi).cuda()
        n_out = 400
        mux, kw = mux_of(20, (9, 7, 1), loop=(0, 0, 1), max_out=n_out)
        out = torch.zeros(n_out * 188, dtype=torch.uint8, device="cuda")
        mux.run_device([ts_d[0].data_ptr(), ts_d[1].data_ptr(), psi_d.data_ptr()], n_ts + [len(psi) // 188],
                       out.data_ptr(), n_out, stream=st.cuda_stream)
        ad = dvbt2ll.ModeAdapter(framesize=0, rate=0, kbch=7032, pids=[pids[1]], max_ts_bytes=n_out * 188)
        cap_bb = n_out * 188 // ad.D + 1
        bb = torch.zeros(cap_bb * ad.L, dtype=torch.uint8, device="cuda")
        ad.run_device(out.data_ptr(), n_out * 188, bb.data_ptr(), cap_bb, flush=True, stream=st.cuda_stream)
    res = mux.result()
    st.synchronize()
    ref = R.mux([refs[0].ts, refs[1].ts, psi], n_out, **kw)
    res.ts = out.cpu().numpy()
    same(res, ref, "end to end")
    assert ref.counters["consumed"][:2] == tuple(n_ts) and ref.counters["dry_slots"][0] > 0
    chk = R.check_ts(res.ts, cc={0: 0, pids[0]: 0, pids[1]: 0})
    assert chk["pat"] == dict(tsid=9, version=3, programs=[(1, 0x30), (2, 0x31)])
    found = [chk["pmts"][n]["streams"] for n in (1, 2)]
    assert found == [[(0x0D, pids[0], b"")], [(0x0D, pids[1], b"")]]
    for k in range(2):
        assert [d for _, d in MR.receive(res.ts, found[k][0][1], 0, MR.crc32_table)] == pdus[k]
    got = ad.result()
    want = ad.run(ref.ts, flush=True)
    assert got.counters == want.counters and want.counters["bbframes"] > 0
    np.testing.assert_array_equal(bb.cpu().numpy()[:len(want.bbframes)], want.bbframes)


TOOL = Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "dvbt2ll" / "dvbt2ll_tx"


def test_cli_mux_equals_the_chain_on_the_reference_multiplexers_ts(gpu, tmp_path):
    """dvbt2ll_tx --input mpe --mux on a tiny config: the IQ file of the TS-file input run on the reference
    encapsulator's TS sent through the reference multiplexer with the reference carousel, byte for byte; the tool runs
    the multiplexer in calls of whole periods, 8192 slots or more, until the encapsulated TS is used up"""
    cfg = CONFIGS["cfg1q"]
    n = 2
    need = len(ts_for_frames(cfg, 0, n)[0])
    pdus = _pdus_for(need, 33)
    pdu, off = MR.pack(pdus)
    enc = MR.encap(pdu, off, pid=0x321, flush=True, crc=MR.crc32_table)
    P, per_call = 12, 12 * (8192 // 12)
    psi = R.psi(1, 0, [dict(program_number=5, pmt_pid=0x44, pcr_pid=0x45, streams=[dict(stream_type=0x90, pid=0x321)])])
    tpp = dvbt2ll.ticks_per_period(P, 4000000)
    kw = dict(period=P, weight=(8, 1), loop=(0, 1), fill_input=0, pcr_pid=0x45, pcr_weight=2, ticks_per_period=tpp)
    calls = 1
    while R.mux([enc.ts, psi], calls * per_call, **kw).counters["consumed"][0] < enc.counters["ts_packets"]:
        calls += 1
    ref = R.mux([enc.ts, psi], calls * per_call, **kw)
    assert len(ref.ts) >= need
    (tmp_path / "in.ts").write_bytes(ref.ts.tobytes())
    (tmp_path / "in.mpe").write_bytes(b"".join(len(p).to_bytes(2, "big") + p for p in pdus))

    def tool(*args):
        return subprocess.run([str(TOOL)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)

    r = tool("--preset", "cfg1q", "--in", tmp_path / "in.ts", "--out", tmp_path / "a.iq", "--batch", 2, "--frames", n)
    assert r.returncode == 0, r.stderr
    r = tool("--preset", "cfg1q", "--input", "mpe", "--pid", "0x321", "--mux",
             "period=12,weight=8,psi-weight=1,pcr-pid=0x45,pcr-weight=2,ts-rate=4000000", "--program", 5, "--pmt-pid",
             "0x44", "--stream-type", "0x90", "--in", tmp_path / "in.mpe", "--out", tmp_path / "b.iq", "--batch", 2,
             "--frames", n)
    assert r.returncode == 0, r.stderr
    a, b = (tmp_path / "a.iq").read_bytes(), (tmp_path / "b.iq").read_bytes()
    assert len(a) == n * dvbt2ll.Chain(cfg, max_frames=1).iq_per_frame * 8 and a == b
    c = ref.counters
    assert ("mux: slots %d, consumed %d, psi_packets %d, fill_in_free %d, pcr_packets %d, null_packets %d, "
            "sync_errors 0" % (calls * per_call, c["consumed"][0], c["consumed"][1], c["fill_in_free"], c["pcr_packets"],
                               c["null_packets"])) in r.stderr
    assert tool("--preset", "cfg1q", "--mux", "period=4,weight=1,psi-weight=1", "--in", tmp_path / "in.ts", "--out",
                tmp_path / "c.iq").returncode == 2                      # --mux needs an encapsulating input
