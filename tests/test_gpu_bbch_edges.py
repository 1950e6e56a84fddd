"""GPU: the fused BB/BCH kernel (t2_kernels.hip bbch_kernel) against the oracle where its closed-form stream
geometry can go wrong: every start phase of a BBFRAME in the packet (NM, HEM, with and without in-band type B),
every consumed sync byte corrupted, stream offsets past 2^31, 2^32 and 2^40, and TS slices cut exactly to the
bytes the API demands with poisoned surroundings.  The cases are built in tests/bbch_cases.py;
tests/test_cpu_bbch_cases.py proves they cover what they claim.  Every comparison is exact."""
import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import ts_for_frames
import bbch_cases as C
import iq_check

pytestmark = pytest.mark.gpu


def _chain(cfg, max_frames):
    ch = dvbt2ll.Chain(cfg, max_frames=max_frames)
    ch.debug_keep_codewords()
    return ch


def _assert_codewords(cfg, got, want, ctx):
    bad = C.codeword_mismatches(cfg, got, want)
    assert not bad, "%s: %d of %d codewords differ from the oracle's, blocks %s" % (ctx, len(bad), len(want), bad[:32])


def _assert_same_iq(a, b, ctx):
    np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32), err_msg=ctx)


# ------------------------------------------------------------------------------------------ 1. residue sweep
@pytest.mark.parametrize("name", list(C.SWEEPS))
def test_sweep_codewords_match_oracle(gpu, name):
    """consecutive FEC blocks that visit every start phase (count0 0..187 in NM, J0 mod 187 in HEM), in one launch
    of more than 128 blocks (a second, partly dead tile): every codeword equals the oracle's"""
    cfg, nframes = C.SWEEPS[name]
    ch = _chain(cfg, nframes)
    ch.run(0, nframes)
    got = ch.debug_codewords(nframes * cfg.fecblocks)
    _assert_codewords(cfg, got, C.oracle_codewords(cfg, 0, nframes), name)
    assert ch.sync_errors() == 0


# ------------------------------------------------------------------------------------------ 2. corrupted syncs
CORRUPT = [("sweep-" + n, c, f) for n, (c, f) in C.SWEEPS.items()] + \
          [("normal-" + n, c, f) for n, (c, f) in C.NORMAL.items()]
CORRUPT_IDS = [c[0] for c in CORRUPT]


def _corrupted(cfg, first, n):
    ts, base = ts_for_frames(cfg, first, n)
    return C.corrupt_syncs(ts, base), base


@pytest.mark.parametrize("name,cfg,nframes", CORRUPT, ids=CORRUPT_IDS)
def test_every_sync_corrupted_direct(gpu, name, cfg, nframes):
    """every sync byte of the stream 0x46: a fresh handle counts exactly the sync bytes the frames consume (the
    oracle's warning count), its codewords are the oracle's for that stream and its IQ is its clean run's"""
    want_n = C.oracle_sync_errors(cfg, 0, nframes)
    nb = nframes * cfg.fecblocks
    ch = _chain(cfg, nframes)
    bad, base = _corrupted(cfg, 0, nframes)
    dirty = ch.run(0, nframes, ts=bad, ts_base=base)
    got_n = ch.sync_errors()
    got = ch.debug_codewords(nb)
    print("%s: sync errors %d, oracle %d" % (name, got_n, want_n))
    assert got_n == want_n
    _assert_codewords(cfg, got, C.oracle_codewords(cfg, 0, nframes, True), name)
    clean = ch.run(0, nframes)
    assert ch.sync_errors() == want_n
    _assert_same_iq(dirty, clean, name)


@pytest.mark.parametrize("name,cfg,nframes", CORRUPT, ids=CORRUPT_IDS)
def test_every_sync_corrupted_split_runs(gpu, name, cfg, nframes):
    """the frames as one call on one handle, then as several calls with first_frame > 0 on a second fresh handle:
    the same total, which is the oracle's (a CRC prologue that counted, or a sync byte at a segment start
    counted by both calls, would add to it); every segment counts its closed form and its codewords are the
    oracle's"""
    want_n = C.oracle_sync_errors(cfg, 0, nframes)
    F = cfg.fecblocks
    one = dvbt2ll.Chain(cfg, max_frames=nframes)
    bad, base = _corrupted(cfg, 0, nframes)
    one.run(0, nframes, ts=bad, ts_base=base)
    one_call = one.sync_errors()
    cuts = [0, C.SPLIT[0], sum(C.SPLIT), nframes] if nframes > sum(C.SPLIT) else list(range(nframes + 1))
    segs = [(a, b - a) for a, b in zip(cuts, cuts[1:])]
    assert len(segs) > 1 and all(n > 0 for _, n in segs)
    want = C.oracle_codewords(cfg, 0, nframes, True)
    ch = _chain(cfg, max(n for _, n in segs))
    total = 0
    for f0, n in segs:
        bad, base = _corrupted(cfg, f0, n)
        ch.run(f0, n, ts=bad, ts_base=base)
        now = ch.sync_errors()
        print("%s: frames [%d, %d): sync errors %d, closed form %d" % (name, f0, f0 + n, now - total,
                                                                        C.sync_count(cfg, f0, n)))
        assert now - total == C.sync_count(cfg, f0, n), (f0, n)
        total = now
        _assert_codewords(cfg, ch.debug_codewords(n * F), want[f0 * F:(f0 + n) * F], "%s frames from %d" % (name, f0))
    print("%s: one call %d, %d calls %d, oracle %d" % (name, one_call, len(segs), total, want_n))
    assert total == one_call
    assert total == want_n


@pytest.mark.parametrize("name,cfg,nframes", CORRUPT, ids=CORRUPT_IDS)
def test_every_sync_corrupted_block_api(gpu, name, cfg, nframes):
    """bbheaderbch_bb over the corrupted stream in two general_work calls: the oracle's count and bits"""
    F = cfg.fecblocks
    nb = nframes * F
    bad, base = _corrupted(cfg, 0, nframes)
    assert base == 0
    want = C.oracle_bits(cfg, 0, nframes, True)
    blk = dvbt2ll.bbheaderbch_bb(*cfg.bb_args())
    om = blk.output_multiple()
    assert want.size == nb * om
    first = (C.SPLIT[0] * F + 1) if nb > C.SPLIT[0] * F + 1 else nb // 2   # not a whole number of frames
    got = np.zeros(nb * om, np.uint8)
    blk.general_work([bad], [got[:first * om]])
    blk.general_work([bad[blk.nitems_consumed:]], [got[first * om:]])
    assert blk.sync_errors() == C.oracle_sync_errors(cfg, 0, nframes)
    bad_blocks = np.nonzero((got.reshape(nb, om) != want.reshape(nb, om)).any(axis=1))[0]
    assert bad_blocks.size == 0, ("blocks", bad_blocks[:32].tolist())


# ------------------------------------------------------------------------------------------ 3. stream offsets
@pytest.mark.parametrize("mode,bname", C.OFFSET_CASES, ids=["%s-%s" % c for c in C.OFFSET_CASES])
def test_large_offset_codewords_match_oracle(gpu, mode, bname):
    """frames [K, K + 2) at a stream position around 2^31 / 2^32 or above 2^40, fed the bytes of frames [k, k + 2)
    with the same packet phase, in-band phase and FRAME_IDX (bbch_cases.shifted_run): the codewords are the
    oracle's for frames [k, k + 2); for one NM and one HEM case the whole IQ is the oracle chain's (L1-post
    FRAME_IDX, P1 and the OFDM stage at a large first_frame)"""
    cfg, n = C.OFFSET_CFGS[mode], C.OFFSET_FRAMES
    K = C.large_frame(cfg, C.BOUNDARIES[bname])
    k, D, ts, base = C.shifted_run(cfg, K)
    ctx = "%s %s: frame %d as frame %d" % (mode, bname, K, k)
    ch = _chain(cfg, n)
    iq = ch.run(K, n, ts=ts, ts_base=base)
    _assert_codewords(cfg, ch.debug_codewords(n * cfg.fecblocks), C.oracle_codewords(cfg, k, n), ctx)
    assert ch.sync_errors() == 0
    if (mode, bname) in C.IQ_OFFSET_CASES:
        car, pg = C.oracle_carriers(cfg, k, n)
        per, p1 = ch.iq_per_frame, pg.p1()
        for f in range(n):
            fr = iq[f * per:(f + 1) * per]
            iq_check.check_frame_exact(fr, car[f], cfg.pg_args(), pg.guard, pg.normalization, "%s + %d" % (ctx, f))
            iq_check.check_frame(fr, car[f], pg.vlength, pg.guard, pg.normalization, p1, "%s + %d" % (ctx, f))


def test_large_offset_graph_mode(gpu):
    """the same large-K run through run_device as one hipGraph (first launch and a relaunch): the direct run's IQ"""
    import torch
    mode, bname = C.GRAPH_OFFSET_CASE
    cfg, n = C.OFFSET_CFGS[mode], C.OFFSET_FRAMES
    K = C.large_frame(cfg, C.BOUNDARIES[bname])
    k, D, ts, base = C.shifted_run(cfg, K)
    ref = _chain(cfg, n)
    want = ref.run(K, n, ts=ts, ts_base=base)
    _assert_codewords(cfg, ref.debug_codewords(n * cfg.fecblocks), C.oracle_codewords(cfg, k, n), "direct")
    ch = _chain(cfg, n)
    ch.set_graph(True)
    ts_d = torch.from_numpy(ts).cuda()
    for rep in range(2):
        iq_d = torch.zeros((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
        ch.run_device(ts_d.data_ptr(), base, len(ts), K, n, iq_d.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _assert_same_iq(iq_d.cpu().numpy().reshape(-1), want.view(np.float32), "graph launch %d" % rep)
        _assert_codewords(cfg, ch.debug_codewords(n * cfg.fecblocks), C.oracle_codewords(cfg, k, n), "graph %d" % rep)


# ------------------------------------------------------------------------------------------ 4. tight TS slices
PAD = 4096   # bytes of poison on either side of the slice


def _device_slice(cut, fill, misalign):
    """the slice in the middle of a larger device array filled with `fill`, its first byte `misalign` bytes past a
    16-byte boundary; returns the array (keep it alive) and the interior pointer"""
    import torch
    buf = torch.full((2 * PAD + len(cut) + 16,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    off = PAD + misalign
    buf[off:off + len(cut)] = torch.from_numpy(cut).cuda()
    return buf, buf.data_ptr() + off


@pytest.mark.parametrize("mode", list(C.TIGHT_CASES))
def test_tight_slice_poisoned_surroundings(gpu, mode):
    """a mid-stream frame from exactly the bytes the API demands (t2_capi.cpp ts_span), placed at aligned and
    unaligned addresses inside an array of 0xA5 or 0x00: IQ and codewords equal the run from the generous
    buffer and the oracle's codewords -- no byte outside [ts, ts + ts_len) has any influence"""
    import torch
    (cfg, f0), n = C.TIGHT_CASES[mode], C.TIGHT_FRAMES
    nb = n * cfg.fecblocks
    want_cw = C.oracle_codewords(cfg, f0, n)
    ref = _chain(cfg, n)
    want_iq = ref.run(f0, n)
    _assert_codewords(cfg, ref.debug_codewords(nb), want_cw, "generous buffer")
    lo, end = C.ts_span(cfg, f0, n)
    cut = C.stream_slice(lo, end)
    ch = _chain(cfg, n)
    stream = torch.cuda.current_stream().cuda_stream
    for fill in (0xA5, 0x00):
        for misalign in (0, 1, 7):
            ctx = "%s fill %#x, %d past a 16-byte boundary" % (mode, fill, misalign)
            buf, ptr = _device_slice(cut, fill, misalign)
            iq_d = torch.zeros((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
            ch.run_device(ptr, lo, len(cut), f0, n, iq_d.data_ptr(), stream)
            torch.cuda.synchronize()
            _assert_codewords(cfg, ch.debug_codewords(nb), want_cw, ctx)
            _assert_same_iq(iq_d.cpu().numpy().reshape(-1), want_iq.view(np.float32), ctx)
            del buf
    assert ch.sync_errors() == 0


@pytest.mark.parametrize("mode", list(C.TIGHT_CASES))
def test_slice_one_byte_short_is_refused(gpu, mode):
    """a slice that misses the first or the last byte of the span is refused by the host check and nothing is
    launched (the output buffer keeps its contents, the error count stays)"""
    import torch
    (cfg, f0), n = C.TIGHT_CASES[mode], C.TIGHT_FRAMES
    lo, end = C.ts_span(cfg, f0, n)
    cut = C.stream_slice(lo, end)
    buf, ptr = _device_slice(cut, 0xA5, 0)
    ch = _chain(cfg, n)
    iq_d = torch.full((n * ch.iq_per_frame, 2), 7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    short = [
        # the last byte missing: the span check at the high end (base + len < end)
        (ptr, lo, len(cut) - 1),
        # the first byte missing: the base is then off a packet boundary, which the host refuses as such (as
        # test_chain_rejects_unaligned_ts_base); it does not reach the span check
        (ptr + 1, lo + 1, len(cut) - 1),
        # the shortest cut at the low end that keeps the base on a packet boundary, the packet before the first
        # one touched missing: the span check at the low end (base > lo)
        (ptr + 188, lo + 188, len(cut) - 188)]
    for p, base, length in short:
        with pytest.raises(dvbt2ll.DVBT2Error):
            ch.run_device(p, base, length, f0, n, iq_d.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((iq_d == 7.0).all())
    assert ch.sync_errors() == 0
    ch.run_device(ptr, lo, len(cut), f0, n, iq_d.data_ptr(), stream)   # the exact span is accepted
    torch.cuda.synchronize()
    assert not bool((iq_d == 7.0).all())
