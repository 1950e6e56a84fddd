"""GPU: BBFRAME input of the chain (dvbt2ll_chain_set_input, DVBT2LL_INPUT_BBFRAME; t2_kernels.hip bbch_kernel's
BBFRAME kind).  The oracle's own BBFRAMEs (tests/bbf_ref.py oracle_bbframes) must encode to what the TS path and
the oracle produce; arbitrary BBFRAMEs to what the independent numpy reference (bbf_ref.encode_ref, proven against
the oracle by tests/test_cpu_bbframe.py) produces.  Every comparison is exact."""
import hashlib
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, MPLP_CONFIGS, KBCH, bbframe_span, ts_for_frames
import bbch_cases as C
import bbf_ref as R
import iq_check
import oracle_lib as O
import std_tables as T

pytestmark = pytest.mark.gpu

BBF, TS = dvbt2ll.INPUT_BBFRAME, dvbt2ll.INPUT_TS
NM_CFG = C.SWEEPS["nm"][0]   # cfg1's 4K frame, 8 short blocks, rate 1/2: L = 879, odd


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int16) if x.dtype == np.int16 else x.view(np.uint32)


def _same(got, want, ctx):
    a, b = _bits(got).reshape(-1), _bits(want).reshape(-1)
    assert a.shape == b.shape, (ctx, a.shape, b.shape)
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, "%s: %d of %d words differ, first at %s" % (ctx, bad.size, a.size, bad[:5])


def _assert_codewords(cfg, got, want, ctx):
    bad = C.codeword_mismatches(cfg, got, want)
    assert not bad, "%s: %d of %d codewords differ, blocks %s" % (ctx, len(bad), len(want), bad[:32])


def _chain(cfg, max_frames, fmt=BBF, keep=True):
    ch = dvbt2ll.Chain(cfg, max_frames=max_frames)
    if keep:
        ch.debug_keep_codewords()
    ch.set_input(fmt)
    return ch


def _run_device(ch, dev_ptr, base, length, first, n, fill=None):
    """run_device into a fresh cf32 buffer on torch's stream; returns the device buffer after synchronising"""
    import torch
    iq = torch.full((n * ch.iq_per_frame, 2), 0.0 if fill is None else fill, dtype=torch.float32, device="cuda")
    ch.run_device(dev_ptr, base, length, first, n, iq.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return iq


def _sc16(iq, gain=0.2):
    return np.clip(np.rint((iq.view(np.float32) * np.float32(gain)) * np.float32(32767)), -32768,
                   32767).astype(np.int16)


@pytest.fixture(scope="module")
def nm(gpu):
    """the launch-form cases' shape: its 4 frames of oracle BBFRAMEs and the TS path's IQ of them"""
    cfg, n = NM_CFG, 4
    ts_ch = dvbt2ll.Chain(cfg, max_frames=n)
    want = ts_ch.run(0, n)
    want.setflags(write=False)
    L, F = R.bbframe_len(cfg), cfg.fecblocks
    return dict(cfg=cfg, n=n, want=want, bbf=R.oracle_bbframes(cfg, 0, n), L=L, F=F, per=ts_ch.iq_per_frame)


# ------------------------------------------------------------------------------------------ 1. identity with TS
@pytest.mark.parametrize("name", ["nm", "hem", "nm-inband"])
def test_oracle_bbframes_give_the_ts_path_iq(gpu, name):
    """the oracle's BBFRAMEs of 4 frames (32 consecutive blocks: L = 879 is odd, so they start at every byte phase
    of a 16-byte load; L = 1194 in HEM) in BBFRAME format: the same handle's TS-format IQ and the oracle's carriers
    through the CPU model of the GPU IFFT; no header error, the TS sync counter untouched"""
    cfg, _ = C.SWEEPS[name]
    n, L, F = 4, R.bbframe_len(cfg), cfg.fecblocks
    assert L == (879 if name != "hem" else 1194)
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ts_info = dict(ch.info)
    want = ch.run(0, n)
    syncs = ch.sync_errors()
    assert ch.get_input() == TS
    ch.set_input(BBF)
    assert ch.get_input() == BBF
    assert ch.info["ts_bytes_per_frame"] == F * L and ch.info["payload_bytes_per_block"] == L
    bbf = R.oracle_bbframes(cfg, 0, n)
    assert bbframe_span(cfg, 0, n) == (0, len(bbf))
    got = ch.run(0, n, ts=bbf, ts_base=0)
    _same(got, want, name + " BBFRAME format against TS format")
    car, pg = C.oracle_carriers(cfg, 0, n)
    per = ch.iq_per_frame
    for f in range(n):
        iq_check.check_frame_exact(got[f * per:(f + 1) * per], car[f], cfg.pg_args(), pg.guard, pg.normalization,
                                   "%s frame %d" % (name, f))
    assert ch.bbheader_errors() == 0
    assert ch.sync_errors() == syncs
    ch.set_input(TS)
    assert ch.info == ts_info


# ------------------------------------------------------------------------------------------ 2. K-slice split
def test_normal_blocks_split_mid_bbframe(gpu):
    """64800-bit blocks, L = 4836 = 151 x 32 + 4: the K slices split the BBFRAME mid-way and the last chunk holds 4
    bytes; the kept codewords are the oracle's and the IQ is the TS run's"""
    cfg, n = C.NORMAL["nm"]
    assert R.bbframe_len(cfg) == 4836 and cfg.fecblocks == 3 and n == 2
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ch.debug_keep_codewords()
    want = ch.run(0, n)
    ch.set_input(BBF)
    got = ch.run(0, n, ts=R.oracle_bbframes(cfg, 0, n), ts_base=0)
    _assert_codewords(cfg, ch.debug_codewords(n * cfg.fecblocks), C.oracle_codewords(cfg, 0, n), "normal nm")
    _same(got, want, "normal nm IQ")
    assert ch.bbheader_errors() == 0


# ------------------------------------------------------------------------------------------ 3. arbitrary BBFRAMEs
def _parity_bits(framesize, rate):
    return T.fec(framesize, rate)[0] - KBCH[(framesize, rate)]


def _arbitrary_cases():
    """one code per distinct BCH parity size the standard's 14 codes have among {128, 160, 168, 192} (normal: 192 or
    160, short: 168; no DVB-T2 code has 128), plus rate 3/4 normal (L = 6051, odd), each on a frame of configs.py
    with few blocks: cfg4's 8K frame with 3 normal blocks (as bbch_cases.NORMAL), cfg1's 4K frame with 8 short ones"""
    c1, c4 = CONFIGS["cfg1"], CONFIGS["cfg4"]
    seen, out = set(), []
    for fs, rate in [(1, r) for r in range(6)] + [(0, r) for r in range(8)]:
        P = _parity_bits(fs, rate)
        assert P in (128, 160, 168, 192)
        if P not in seen:
            seen.add(P)
            out.append((c4.with_(rate=rate, fecblocks=3) if fs else c1.with_(rate=rate), "P%d" % P))
    out.append((c4.with_(rate=E.C3_4, fecblocks=3), "3/4-normal"))
    return out


ARBITRARY = _arbitrary_cases()


@pytest.mark.parametrize("cfg,name", ARBITRARY, ids=[a[1] for a in ARBITRARY])
def test_arbitrary_bbframes_match_numpy_reference(gpu, cfg, name):
    """random bytes, header included (no TS produces them): the kept codewords are the numpy reference's, and every
    block whose random header fails the CRC rule is counted"""
    F, L = cfg.fecblocks, R.bbframe_len(cfg)
    if name == "3/4-normal":
        assert L == 6051
    rng = np.random.default_rng(L)
    bbf = rng.integers(0, 256, F * L, dtype=np.uint8)
    ch = _chain(cfg, 1)
    ch.run(0, 1, ts=bbf, ts_base=0)
    want = C.pack_codewords(cfg, R.encode_ref(cfg.framesize, cfg.rate, bbf), F)
    _assert_codewords(cfg, ch.debug_codewords(F), want, name)
    bad = R.header_errors(L, bbf)
    print("%s: %d of %d random headers fail the CRC rule" % (name, bad, F))
    assert ch.bbheader_errors() == bad
    assert ch.sync_errors() == 0


# ------------------------------------------------------------------------------------------ 4. header counter
def test_header_counter_counts_each_bad_bbframe_once(gpu, nm):
    cfg, n, L, F = nm["cfg"], 2, nm["L"], nm["F"]
    nb = n * F
    bbf = np.array(nm["bbf"][:nb * L], copy=True)
    for blk, byte, bit in ((0, 0, 0x80), (5, 9, 0x02), (nb - 1, 4, 0x01)):
        bbf[blk * L + byte] ^= bit
    assert R.header_errors(L, bbf) == 3
    ch = _chain(cfg, n)
    ch.run(0, n, ts=bbf, ts_base=0)
    assert ch.bbheader_errors() == 3
    _assert_codewords(cfg, ch.debug_codewords(nb), C.pack_codewords(cfg, R.encode_ref(cfg.framesize, cfg.rate, bbf), nb),
                      "corrupted headers")
    ch.run(0, n, ts=bbf, ts_base=0)   # a second run counts them again: once per run
    assert ch.bbheader_errors() == 6


# ------------------------------------------------------------------------------------------ 5. offsets
def test_first_frame_offsets_and_refusals(gpu, nm):
    """first_frame > 0 from a buffer holding only that run; a declared position above 2^32 (frame K = k mod t2frames
    has frame k's FRAME_IDX, and BBFRAME input has no other cross-frame state); a ts_base off a BBFRAME boundary
    and a buffer one byte short are refused with nothing launched"""
    import torch
    cfg, L, F, per = nm["cfg"], nm["L"], nm["F"], nm["per"]
    ch = _chain(cfg, 2)
    lo, end = bbframe_span(cfg, 2, 2)
    assert (lo, end) == (2 * F * L, 4 * F * L)
    got = ch.run(2, 2, ts=nm["bbf"][lo:end], ts_base=lo)
    _same(got, nm["want"][2 * per:4 * per], "frames 2, 3 alone")
    K = ((1 << 32) // (F * L) + 2) // cfg.t2frames * cfg.t2frames
    lo, end = bbframe_span(cfg, K, 2)
    assert lo > 1 << 32 and K % cfg.t2frames == 0
    got = ch.run(K, 2, ts=nm["bbf"][:2 * F * L], ts_base=lo)
    _same(got, nm["want"][:2 * per], "frame %d as frame 0" % K)
    assert ch.bbheader_errors() == 0
    dev = torch.from_numpy(np.array(nm["bbf"][:2 * F * L + 1])).cuda()
    iq = torch.full((2 * per, 2), 7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for ptr, base, length in ((dev.data_ptr() + 1, 1, 2 * F * L),        # base off a BBFRAME boundary
                              (dev.data_ptr(), 188, 2 * F * L + 1),      # a packet boundary is none
                              (dev.data_ptr(), 0, 2 * F * L - 1),        # one byte short
                              (dev.data_ptr(), L, 2 * F * L - L)):       # the first BBFRAME missing
        with pytest.raises(dvbt2ll.DVBT2Error):
            ch.run_device(ptr, base, length, 0, 2, iq.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((iq == 7.0).all())
    ch.run_device(dev.data_ptr(), 0, 2 * F * L, 0, 2, iq.data_ptr(), stream)
    torch.cuda.synchronize()
    _same(iq.cpu().numpy().reshape(-1), nm["want"][:2 * per].view(np.float32), "the exact span")


# ------------------------------------------------------------------------------------------ 6. tight buffer end
def test_tight_buffer_end_in_poisoned_allocation(gpu, nm):
    """the run's last byte is the last byte of ts_len, inside a larger 0xA5 array, at aligned and unaligned
    addresses: the last pieces take the bytewise edge path, and the codewords are the oracle's"""
    import torch
    cfg, L, F, n = nm["cfg"], nm["L"], nm["F"], 2
    cut = np.array(nm["bbf"][:n * F * L])
    want = C.oracle_codewords(cfg, 0, n)
    ch = _chain(cfg, n)
    for misalign in (0, 1, 7):
        buf = torch.full((8192 + len(cut) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        off = 4096 + misalign
        buf[off:off + len(cut)] = torch.from_numpy(cut).cuda()
        iq = _run_device(ch, buf.data_ptr() + off, 0, len(cut), 0, n)
        _assert_codewords(cfg, ch.debug_codewords(n * F), want, "%d past a 16-byte boundary" % misalign)
        _same(iq.cpu().numpy().reshape(-1), nm["want"][:n * nm["per"]].view(np.float32), "tight IQ %d" % misalign)
    assert ch.bbheader_errors() == 0


# ------------------------------------------------------------------------------------------ 7. launch forms
def test_stream_batch_with_odd_stride(gpu, nm):
    import torch
    cfg, L, F, per, n = nm["cfg"], nm["L"], nm["F"], nm["per"], 2
    nbytes = n * F * L
    other = np.roll(np.array(nm["bbf"][:nbytes]), 3)   # any bytes are BBFRAMEs
    ch = _chain(cfg, 2 * n, keep=False)
    want1 = ch.run(0, n, ts=other, ts_base=0)
    stride = nbytes + 1
    assert stride % 2 == 1
    host = np.full(2 * stride, 0xA5, np.uint8)
    host[:nbytes] = nm["bbf"][:nbytes]
    host[stride:stride + nbytes] = other
    dev = torch.from_numpy(host).cuda()
    iq = torch.zeros((2 * n * per, 2), dtype=torch.float32, device="cuda")
    ch.run_streams(dev.data_ptr(), stride, 2, 0, nbytes, 0, n, iq.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = iq.cpu().numpy().reshape(2, -1)
    _same(got[0], nm["want"][:n * per].view(np.float32), "stream 0")
    _same(got[1], want1.view(np.float32), "stream 1")


def test_graph_mode_after_a_ts_format_graph(gpu, nm):
    """set_input after a TS-format graph run on the same handle: the next graph runs use the BBFRAME kernel and
    arguments (first launch and a relaunch), and the TS format again afterwards"""
    import torch
    cfg, n, per = nm["cfg"], 2, nm["per"]
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ch.set_graph(True)
    ts, base = ts_for_frames(cfg, 0, n)
    ts_d = torch.from_numpy(ts).cuda()
    want = nm["want"][:n * per].view(np.float32)
    _same(_run_device(ch, ts_d.data_ptr(), base, len(ts), 0, n).cpu().numpy().reshape(-1), want, "TS graph")
    ch.set_input(BBF)
    bbf_d = torch.from_numpy(np.array(nm["bbf"][:n * nm["F"] * nm["L"]])).cuda()
    for rep in range(2):
        got = _run_device(ch, bbf_d.data_ptr(), 0, bbf_d.numel(), 0, n)
        _same(got.cpu().numpy().reshape(-1), want, "BBFRAME graph launch %d" % rep)
    ch.set_input(TS)
    _same(_run_device(ch, ts_d.data_ptr(), base, len(ts), 0, n).cpu().numpy().reshape(-1), want, "TS graph again")
    assert ch.bbheader_errors() == 0 and ch.sync_errors() == 0


def test_sc16_output(gpu, nm):
    cfg, n = nm["cfg"], nm["n"]
    ch = _chain(cfg, n, keep=False)
    ch.set_output(0.2, dvbt2ll.IQ_SC16)
    sc = ch.run(0, n, ts=nm["bbf"], ts_base=0)
    np.testing.assert_array_equal(sc.reshape(-1), _sc16(nm["want"]))


def test_two_slots_on_two_streams(gpu, nm):
    import torch
    cfg, L, F, per = nm["cfg"], nm["L"], nm["F"], nm["per"]
    ch = _chain(cfg, 2, keep=False)
    ch.set_slots(2)
    dev = torch.from_numpy(np.array(nm["bbf"])).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros((2 * per, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    for rep in range(2):
        for c in range(2):
            ch.run_device(dev.data_ptr(), 0, dev.numel(), 2 * c, 2, outs[c].data_ptr(), streams[c].cuda_stream)
    torch.cuda.synchronize()
    for c in range(2):
        _same(outs[c].cpu().numpy().reshape(-1), nm["want"][2 * c * per:(2 * c + 2) * per].view(np.float32),
              "slot %d" % c)


def test_host_paths(gpu, nm):
    """run_host copies exactly the run's BBFRAMEs out of a longer buffer; run_host_pipelined with more chunks than
    ring entries"""
    cfg, n, L, F, per = nm["cfg"], nm["n"], nm["L"], nm["F"], nm["per"]
    ch = _chain(cfg, n, keep=False)
    got = ch.run(1, 2, ts=nm["bbf"], ts_base=0)   # frames 1, 2 of a buffer that holds 0 .. 3
    _same(got, nm["want"][per:3 * per], "run_host mid-buffer")
    iq = np.zeros(n * per, np.complex64)
    assert n > 3   # DVBT2LL_HOST_RING
    ch.run_host_pipelined(nm["bbf"], 0, 0, n, iq, chunk_frames=1)
    _same(iq, nm["want"], "pipelined")
    with pytest.raises(dvbt2ll.DVBT2Error):
        ch.run_host_pipelined(nm["bbf"][:-1], 0, 0, n, iq, chunk_frames=1)
    with pytest.raises(dvbt2ll.DVBT2Error):
        ch.run(0, n, ts=nm["bbf"][L:], ts_base=188)


# ------------------------------------------------------------------------------------------ 8. multi-PLP
def test_multi_plp_mixed_formats(gpu):
    """the 4K multi-PLP frame of test_gpu_mplp.py's set (three PLPs: MIS headers, one of them HEM): PLP 1 alone in
    BBFRAME format beside two TS PLPs, then every PLP in BBFRAME format: the all-TS run's IQ"""
    import torch
    from test_gpu_mplp import _device_ts, _run
    m = MPLP_CONFIGS["mplp3_4k"]
    n = 2
    ch = dvbt2ll.Chain(m, max_frames=n)
    want = _run(ch, m, 0, n)
    _, bb_bits, _ = O.mplp_cells(m, 0, n)
    bbf = []
    for k, p in enumerate(m.plps):
        kb = KBCH[(p.framesize, p.rate)]
        bits = np.concatenate(bb_bits[k]).reshape(n * p.fecblocks, -1)[:, :kb]
        bbf.append(np.packbits(bits ^ R.prbs_bits(kb)[None, :], axis=1).reshape(-1))
        assert bbframe_span(p, 0, n) == (0, len(bbf[k]))
    ts_bufs, ts_bases, ts_lens = _device_ts(m, 0, n)
    bbf_bufs = [torch.from_numpy(b).cuda() for b in bbf]
    for plps in ((1,), (0, 1, 2)):
        for k in plps:
            ch.set_input(BBF, plp=k)
        fmts = [ch.get_input(k) for k in range(m.nplp)]
        assert fmts == [BBF if k in plps else TS for k in range(m.nplp)]
        bufs = [bbf_bufs[k] if k in plps else ts_bufs[k] for k in range(m.nplp)]
        bases = [0 if k in plps else ts_bases[k] for k in range(m.nplp)]
        iq = torch.empty((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
        ch.run_plps([b.data_ptr() for b in bufs], bases, [b.numel() for b in bufs], 0, n, iq.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _same(iq.cpu().numpy().reshape(-1), want.view(np.float32), "PLPs %s in BBFRAME format" % (plps,))
    assert ch.bbheader_errors() == 0
    with pytest.raises(dvbt2ll.DVBT2Error):
        ch.set_input(BBF, plp=m.nplp)
    with pytest.raises(dvbt2ll.DVBT2Error):
        ch.set_input(2)


# ------------------------------------------------------------------------------------------ 9. MISO pair handle
def test_miso_pair_handle(gpu):
    from test_gpu_miso import chain_cfg
    cfg = chain_cfg("4k_short_np2").with_(misogroup=E.MISO_TX1)
    n = 2
    pair = dvbt2ll.Chain(cfg, max_frames=n, miso_pair=True)
    want = pair.run_groups(0, n)
    pair.set_input(BBF)
    bbf = np.array(R.oracle_bbframes(cfg, 0, n))
    got = pair.run_groups(0, n, ts=bbf, ts_base=0)
    for g in range(2):
        _same(got[g], want[g], "group %d" % (g + 1))
    assert pair.bbheader_errors() == 0


# ------------------------------------------------------------------------------------------ 10. 32K
def test_cfg3_golden_iq_digest(gpu):
    """cfg3's fixture frames in BBFRAME format: the golden IQ digest the TS path is checked against"""
    cfg = CONFIGS["cfg3"]
    g = np.load(Path(__file__).resolve().parent / "golden" / "cfg3.npz")
    n = int(g["nframes"])
    ch = _chain(cfg, n, keep=False)
    iq = ch.run(0, n, ts=R.oracle_bbframes(cfg, 0, n), ts_base=0)
    assert hashlib.sha256(np.ascontiguousarray(iq).tobytes()).digest() == g["iq_sha256"].tobytes()
    assert ch.bbheader_errors() == 0


# ------------------------------------------------------------------------------------------ 11. switching back
def test_switching_back_to_ts(gpu, nm):
    cfg, n = nm["cfg"], 2
    ch = _chain(cfg, n, keep=False)
    ch.run(0, n, ts=nm["bbf"][:n * nm["F"] * nm["L"]], ts_base=0)
    ch.set_input(TS, plp=-1)
    assert ch.get_input() == TS
    _same(ch.run(0, n), nm["want"][:n * nm["per"]], "TS again")
    assert ch.sync_errors() == 0
    ts, base = ts_for_frames(cfg, 0, n)
    bad = C.corrupt_syncs(ts, base)
    _same(ch.run(0, n, ts=bad, ts_base=base), nm["want"][:n * nm["per"]], "TS, corrupted syncs")
    assert ch.sync_errors() == C.sync_count(cfg, 0, n)
    assert ch.bbheader_errors() == 0
