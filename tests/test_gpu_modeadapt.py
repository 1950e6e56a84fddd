"""GPU: the mode adapter (dvbt2ll_modeadapt_*, csrc/modeadapt_kernels.hip) against the sequential adapter of
tests/modeadapt_ref.py (proven by tests/test_cpu_modeadapt.py): output bytes, every counter and the resume position,
all exact.  Every device run here has its TS inside a larger poisoned array and its output inside a poisoned array
with guard regions; the guards and the bytes past the last BBFRAME must stay untouched."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, MPLP_CONFIGS, KBCH, ts_packets
import bbf_ref as BR
import modeadapt_cases as C
import modeadapt_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1)


_STREAM = []


def _side_stream():
    """a torch stream with a handle of its own: torch's default stream has handle 0, which the C ABI reads as "the
    handle's own stream", and then the fills below and the adapter's kernels would not be ordered"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def device_run(ad, ts, start=(0, 0, 0), cap=None, flush=False, misalign=3, stream=None):
    """one run_device with everything inside poisoned arrays; returns the result with bbframes filled in, after
    checking the guards.  cap None: room for all the buffer could fill"""
    import torch
    st = _side_stream() if stream is None else stream
    cap = len(ts) // ad.D + 2 if cap is None else cap
    with torch.cuda.stream(st):
        buf = torch.full((2 * GUARD + len(ts) + 16,), POISON, dtype=torch.uint8, device="cuda")
        off = GUARD + misalign
        buf[off:off + len(ts)] = torch.from_numpy(np.array(ts, np.uint8)).cuda()
        out = torch.full((2 * GUARD + cap * ad.L + 16,), POISON, dtype=torch.uint8, device="cuda")
        a = GUARD + (misalign * 5 + 1) % 16
        ad.run_device(buf.data_ptr() + off, len(ts), out.data_ptr() + a, cap, start=start, flush=flush,
                      stream=st.cuda_stream)
    res = ad.result()
    st.synchronize()
    o = out.cpu().numpy()
    n = res.counters["bbframes"] * ad.L
    assert res.counters["bbframes"] <= cap
    assert (o[:a] == POISON).all() and (o[a + n:] == POISON).all(), "written outside its BBFRAMEs"
    res.bbframes = o[a:a + n].copy()
    got = buf.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + len(ts):] == POISON).all()
    np.testing.assert_array_equal(got[off:off + len(ts)], ts)
    return res


def same(res, ref, ctx=""):
    assert tuple(res.resume) == tuple(ref.resume), (ctx, res.resume, ref.resume)
    assert res.counters == ref.counters, (ctx, res.counters, ref.counters)
    np.testing.assert_array_equal(res.bbframes, ref.bbframes, err_msg=str(ctx))


def check(ad, ts, ctx, mask=None, sis=True, isi=0, **kw):
    ref = R.adapt(ts, ad.kbch, npd=ad.npd, mask=mask, sis=sis, isi=isi,
                  **{k: v for k, v in kw.items() if k in ("start", "cap", "flush")})
    res = device_run(ad, ts, **kw)
    same(res, ref, ctx)
    return res, ref


@pytest.fixture(scope="module")
def ad14(gpu):
    return dvbt2ll.ModeAdapter(kbch=C.KBCH_SHORT14, max_ts_bytes=188 * 2200)


@pytest.fixture(scope="module")
def ad_odd(gpu):
    return dvbt2ll.ModeAdapter(kbch=C.KBCH_ODD, max_ts_bytes=188 * 2200)


# ---------------------------------------------------------------------------------------- 1. null runs, both codes
@pytest.mark.parametrize("place", [0, 1, 2])
@pytest.mark.parametrize("run", C.RUNS)
def test_null_runs_short_quarter(gpu, ad14, run, place):
    """L = 384, D = 374: fewer than two units per BBFRAME, the SYNCD phase moves by 2 per frame"""
    ts = C.run_stream(run, place)
    for flush in (False, True):
        check(ad14, ts, (run, place, flush), flush=flush, misalign=(run + place) % 4)


@pytest.mark.parametrize("run", [0, 255, 256, 600])
def test_null_runs_odd_length_normal_code(gpu, ad_odd, run):
    """L = 6051: the 16-byte boundary of the destination moves from BBFRAME to BBFRAME"""
    assert ad_odd.L % 2 == 1
    ts = C.stream([(C.PID_A, 70), (C.PID_NULL, run), (C.PID_A, 70)], seed=run)
    for mis in (0, 1):
        check(ad_odd, ts, (run, mis), flush=True, misalign=mis)
    check(ad_odd, ts, (run, "no flush"), misalign=2)


def test_three_scan_tiles(gpu, ad14, ad_odd):
    """2200 packets: three tiles of 1024 and the tile-sum pass; a run of 600 nulls across a tile boundary; a kept
    null on a tile's last packet; three bad sync bytes"""
    ts = C.two_tile_stream()
    assert len(ts) // 188 >= 2049
    res, _ = check(ad14, ts, "tiles 3072", flush=True)
    assert res.counters["sync_errors"] == 3 and res.counters["nulls_kept"] == 3
    check(ad_odd, ts, "tiles 48408", flush=True, misalign=1)


# ---------------------------------------------------------------------------------------- 2. selection, no deletion
def test_two_pid_mask_with_foreign_pids_between(gpu):
    ts = C.two_pid_stream()
    for pids in ([C.PID_A, C.PID_B], [C.PID_B]):
        ad = dvbt2ll.ModeAdapter(kbch=C.KBCH_SHORT14, sis_mis=0, isi=5, pids=pids, max_ts_bytes=len(ts))
        res, _ = check(ad, ts, pids, mask=R.mask_of(pids), sis=False, isi=5, flush=True)
        dropped = res.counters["nulls_dropped_at_flush"]
        np.testing.assert_array_equal(R.receive(res.bbframes, C.KBCH_SHORT14),
                                      R.filtered(ts, 1, R.mask_of(pids))[:len(ts) - 188 * dropped])
    # a foreign run longer than 255: the kept packet goes out as the null packet
    ts = C.stream([(C.PID_A, 2), (C.PID_FOREIGN, 300), (C.PID_A, 2)])
    ad = dvbt2ll.ModeAdapter(kbch=C.KBCH_SHORT14, pids=[C.PID_A], max_ts_bytes=len(ts))
    check(ad, ts, "foreign run", mask=R.mask_of([C.PID_A]), flush=True)


HEM_SMALL = CONFIGS["cfg1"].with_(rate=E.C1_3, fecblocks=3, inputmode=E.INPUTMODE_HIEFF)
HEM_ODD = CONFIGS["cfg4"].with_(rate=E.C3_4, fecblocks=2, inputmode=E.INPUTMODE_HIEFF)


@pytest.mark.parametrize("cfg", [HEM_SMALL, HEM_ODD], ids=["short-5232", "normal-48408"])
def test_npd0_is_the_oracles_hem_bbframe_stream(gpu, cfg):
    """without deletion: the oracle's HEM BBFRAMEs of the same TS, byte for byte (its smallest code and the odd-L
    normal one; the oracle builds no short 1/4 BBFRAME)"""
    kbch = KBCH[(cfg.framesize, cfg.rate)]
    n = 2
    nb = n * cfg.fecblocks
    want = BR.oracle_bbframes(cfg, 0, n)
    ts = ts_packets(0, nb * (kbch - 80) // 8 // 187 + 2)
    ad = dvbt2ll.ModeAdapter(framesize=cfg.framesize, rate=cfg.rate, npd=0, max_ts_bytes=len(ts))
    assert ad.kbch == kbch
    res, _ = check(ad, ts, "npd 0", cap=nb)
    np.testing.assert_array_equal(res.bbframes, want)
    ts2 = ts.copy()
    ts2[::188 * 3] = 0x46
    res, _ = check(ad, ts2, "npd 0 bad syncs", cap=nb)
    np.testing.assert_array_equal(res.bbframes, want)
    assert res.counters["sync_errors"] == (res.counters["packets_in"] + 2) // 3


def test_npd0_short_quarter_every_phase(gpu):
    ts = C.split_stream()
    ad = dvbt2ll.ModeAdapter(kbch=C.KBCH_SHORT14, npd=0, max_ts_bytes=len(ts))
    for mis in range(4):
        check(ad, ts, ("npd0", mis), flush=True, misalign=mis)


# ---------------------------------------------------------------------------------------- 3. capacity, chunks, flush
@pytest.mark.parametrize("k", [0, 1, 2, 7])
def test_capacity_cut_then_continuation(gpu, ad14, k):
    ts = C.run_stream(257, 1)
    whole = R.adapt(ts, C.KBCH_SHORT14, flush=True)
    a, _ = check(ad14, ts, "cap %d" % k, cap=k, flush=True)
    assert a.counters["bbframes"] == k and a.counters["flushed"] == 0
    b, _ = check(ad14, ts, "cap %d rest" % k, start=tuple(a.resume), flush=True)
    np.testing.assert_array_equal(np.concatenate([a.bbframes, b.bbframes]), whole.bbframes)
    assert {n: a.counters[n] + b.counters[n] for n in R.COUNTERS} == whole.counters


@pytest.mark.parametrize("cut", [2, 100, 3 + 255, 3 + 256, 3 + 700])
def test_chunked_calls_equal_the_single_call(gpu, ad14, cut):
    """two calls split before packet `cut` of 3 selected, 700 nulls, 6 selected: inside the first packets, inside the
    run (longer than 256), on the kept null at 3 + 255, right after it, at the run's end"""
    ts = C.long_run_stream()
    rows = ts.reshape(-1, 188)
    whole = R.adapt(ts, C.KBCH_SHORT14, flush=True)
    base, pos, out, tot = 0, (0, 0, 0), [], dict.fromkeys(R.COUNTERS, 0)
    for j, end in enumerate((cut, len(rows))):
        res, _ = check(ad14, rows[base:max(end, base)].reshape(-1), ("chunk", cut, j), start=pos, flush=j == 1,
                       misalign=j)
        out.append(res.bbframes)
        for key in tot:
            tot[key] += res.counters[key]
        base += res.resume.ts_packet
        pos = (0, res.resume.unit_byte, res.resume.dnp)
        if cut == 3 + 256 and j == 0:
            assert res.resume.dnp == 255 and base == 3 + 255      # the position is on the kept null
    np.testing.assert_array_equal(np.concatenate(out), whole.bbframes)
    assert tot == whole.counters


def test_flush_partial_exact_and_trailing_nulls(gpu, ad14):
    """187 packets' units are 94 data fields exactly (187 * 188 = 94 * 374): nothing left to flush; one packet more
    leaves a partial frame; trailing nulls are dropped and counted"""
    exact = C.stream([(C.PID_A, 187)], seed=2)
    res, _ = check(ad14, exact, "exact", flush=True)
    assert res.counters["bbframes"] == 94 and res.counters["flushed"] == 0 and res.resume == (187, 0, 0)
    res, _ = check(ad14, exact, "exact, no flush")
    assert res.resume == (187, 0, 0)
    res, _ = check(ad14, C.stream([(C.PID_A, 188)], seed=2), "partial", flush=True)
    assert res.counters["bbframes"] == 95 and res.counters["flushed"] == 1
    res, _ = check(ad14, C.stream([(C.PID_A, 187), (C.PID_NULL, 9)], seed=2), "trailing nulls", flush=True)
    assert res.counters["nulls_dropped_at_flush"] == 9 and res.counters["flushed"] == 0
    res, _ = check(ad14, C.stream([(C.PID_A, 187), (C.PID_NULL, 9)], seed=2), "trailing nulls, no flush")
    assert res.resume == (187, 0, 0) and res.counters["packets_in"] == 187
    res, _ = check(ad14, C.stream([(C.PID_NULL, 40)]), "only nulls", flush=True)
    assert res.counters["bbframes"] == 0 and res.counters["nulls_dropped_at_flush"] == 40
    # a data field no unit begins in: SYNCD 0xFFFF
    res, _ = check(ad14, exact[:188], "no unit begins", start=(0, 184, 7), flush=True)
    assert list(res.bbframes[7:9]) == [0xFF, 0xFF]


def test_run_host(gpu):
    ts = C.two_tile_stream()
    ad = dvbt2ll.ModeAdapter(kbch=C.KBCH_ODD, max_ts_bytes=len(ts))
    same(ad.run(ts, flush=True), R.adapt(ts, C.KBCH_ODD, flush=True), "run_host")
    res = ad.run(ts, cap=3)
    same(res, R.adapt(ts, C.KBCH_ODD, cap=3), "run_host cap 3")
    same(ad.run(ts, start=res.resume, flush=True), R.adapt(ts, C.KBCH_ODD, start=tuple(res.resume), flush=True), "rest")


# ---------------------------------------------------------------------------------------- 4. with the chain
def _chain_iq(ch, bbf_dev, n):
    import torch
    iq = torch.zeros((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if ch.nplp == 1:
        ch.run_device(bbf_dev[0].data_ptr(), 0, bbf_dev[0].numel(), 0, n, iq.data_ptr(), st)
    else:
        ch.run_plps([b.data_ptr() for b in bbf_dev], [0] * ch.nplp, [b.numel() for b in bbf_dev], 0, n,
                    iq.data_ptr(), st)
    torch.cuda.synchronize()
    return iq.cpu().numpy().reshape(-1)


def test_two_handles_two_streams_feed_a_two_plp_chain(gpu):
    """mplp2_8k from one TS: PID A -> PLP 0, PID B -> PLP 1, each adapter on a stream of its own; the chain's IQ is
    that of the reference adapter's BBFRAMEs and every header passes the chain's check"""
    import torch
    m = MPLP_CONFIGS["mplp2_8k"]
    ts = C.two_pid_stream(groups=75)
    ch = dvbt2ll.Chain(m, max_frames=1)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    F = [p.fecblocks for p in m.plps]
    ads = [dvbt2ll.ModeAdapter(chain=ch, plp=k, pids=[pid], max_ts_bytes=len(ts))
           for k, pid in enumerate((C.PID_A, C.PID_B))]
    assert [(a.sis_mis, a.isi) for a in ads] == [(0, 0), (0, 1)]
    refs = [R.adapt(ts, a.kbch, mask=R.mask_of([pid]), sis=False, isi=k, cap=F[k])
            for k, (a, pid) in enumerate(zip(ads, (C.PID_A, C.PID_B)))]
    assert [r.counters["bbframes"] for r in refs] == F
    want = _chain_iq(ch, [torch.from_numpy(r.bbframes.copy()).cuda() for r in refs], 1)
    ts_d = torch.from_numpy(ts.copy()).cuda()
    outs = [torch.zeros(F[k] * a.L, dtype=torch.uint8, device="cuda") for k, a in enumerate(ads)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k, a in enumerate(ads):
        a.run_device(ts_d.data_ptr(), len(ts), outs[k].data_ptr(), F[k], stream=streams[k].cuda_stream)
    for k, a in enumerate(ads):
        res = a.result()
        res.bbframes = outs[k].cpu().numpy()
        same(res, refs[k], "plp %d" % k)
    got = _chain_iq(ch, outs, 1)
    assert np.array_equal(_bits(got), _bits(want))
    assert ch.bbheader_errors() == 0


def test_npd0_single_plp_ends_at_the_ts_paths_hem_iq(gpu):
    """cfg1q in high-efficiency mode: the adapter's BBFRAMEs, on the same stream into a Chain in BBFRAME input, give
    the IQ the chain computes from the TS itself"""
    import torch
    cfg = CONFIGS["cfg1q"].with_(inputmode=E.INPUTMODE_HIEFF)
    n, F = 3, cfg.fecblocks
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    want = ch.run(0, n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    ad = dvbt2ll.ModeAdapter(chain=ch, npd=0, max_ts_bytes=188 * 64)
    assert (ad.kbch, ad.sis_mis) == (7032, 1)
    ts = ts_packets(0, n * F * ad.D // 187 + 2)
    with torch.cuda.stream(_side_stream()):
        ts_d = torch.from_numpy(ts).cuda()
        out = torch.zeros(n * F * ad.L, dtype=torch.uint8, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        assert st != 0
        ad.run_device(ts_d.data_ptr(), len(ts), out.data_ptr(), n * F, stream=st)
        got = _chain_iq(ch, [out], n)         # same stream: no synchronise between adapter and chain
    assert ad.result().counters["bbframes"] == n * F
    assert np.array_equal(_bits(got), _bits(want))
    assert ch.bbheader_errors() == 0


# ---------------------------------------------------------------------------------------- 5. refusals
def test_refusals_launch_nothing(gpu):
    import torch
    ts = C.split_stream()
    for kw in (dict(kbch=3073), dict(kbch=C.KBCH_SHORT14, npd=0, pids=[C.PID_A]), dict(framesize=0, rate=9),
               dict(kbch=C.KBCH_SHORT14, sis_mis=0, isi=256)):
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.ModeAdapter(**kw)
    ad = dvbt2ll.ModeAdapter(kbch=C.KBCH_SHORT14, max_ts_bytes=len(ts))
    ts_d = torch.from_numpy(ts.copy()).cuda()
    out = torch.full((64 * ad.L,), POISON, dtype=torch.uint8, device="cuda")
    before = ad.run(ts).counters
    n = len(ts) // 188
    for length, start, ptr, cap in ((len(ts) - 1, (0, 0, 0), out.data_ptr(), 8),
                                    (len(ts) + 188, (0, 0, 0), out.data_ptr(), 8),
                                    (len(ts), (-1, 0, 0), out.data_ptr(), 8),
                                    (len(ts), (n + 1, 0, 0), out.data_ptr(), 8),
                                    (len(ts), (n, 1, 0), out.data_ptr(), 8),
                                    (len(ts), (0, 188, 0), out.data_ptr(), 8),
                                    (len(ts), (0, 0, 256), out.data_ptr(), 8),
                                    (len(ts), (0, 0, 0), None, 8),
                                    (len(ts), (0, 0, 0), out.data_ptr(), -1)):
        with pytest.raises(dvbt2ll.DVBT2Error):
            ad.run_device(ts_d.data_ptr(), length, ptr, cap, start=start)
    with pytest.raises(dvbt2ll.DVBT2Error):
        ad.run_device(0, len(ts), out.data_ptr(), 8)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert ad.result().counters == before        # the last real run's result still stands


# ---------------------------------------------------------------------------------------- 6. the command-line tool
TOOL = Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "dvbt2ll" / "dvbt2ll_tx"


def _tool(*args):
    return subprocess.run([str(TOOL)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_ts_npd_equals_bbframe_input(gpu, tmp_path):
    """dvbt2ll_tx --input ts-npd --pids on a written TS: the IQ file of --input bbframe on the reference adapter's
    BBFRAMEs, byte for byte (cfg1q, 3 frames in batches of 2); the counters are printed"""
    cfg = CONFIGS["cfg1q"]
    n, F, kbch = 3, cfg.fecblocks, KBCH[(cfg.framesize, cfg.rate)]
    ts = C.two_pid_stream(groups=12)
    pids = [C.PID_A, C.PID_B]
    ref = R.adapt(ts, kbch, mask=R.mask_of(pids), flush=True)
    assert ref.counters["bbframes"] >= n * F
    (tmp_path / "in.bbf").write_bytes(ref.bbframes.tobytes())
    (tmp_path / "in.ts").write_bytes(ts.tobytes())
    r = _tool("--preset", "cfg1q", "--input", "bbframe", "--in", tmp_path / "in.bbf", "--out", tmp_path / "a.iq",
              "--batch", 2, "--frames", n)
    assert r.returncode == 0, r.stderr
    r = _tool("--preset", "cfg1q", "--input", "ts-npd", "--pids", "0x100,0x101", "--in", tmp_path / "in.ts",
              "--out", tmp_path / "b.iq", "--batch", 2, "--frames", n)
    assert r.returncode == 0, r.stderr
    a, b = (tmp_path / "a.iq").read_bytes(), (tmp_path / "b.iq").read_bytes()
    assert len(a) == n * dvbt2ll.Chain(cfg, max_frames=1).iq_per_frame * 8 and a == b
    c = ref.counters
    assert "%d T2 frames" % n in r.stderr
    assert "selected %d, nulls_deleted %d, nulls_kept %d," % (c["selected"], c["nulls_deleted"], c["nulls_kept"]) in r.stderr
    assert "bbframes %d, flushed %d" % (c["bbframes"], c["flushed"]) in r.stderr
