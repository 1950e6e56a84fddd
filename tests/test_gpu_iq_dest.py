"""GPU: where the OFDM kernels put the IQ.  Both kernels pick their store path by the destination's address:
sample pairs (IqOut::put2: ofdm_kernel's paired branch, o32_store_pairs) where every symbol starts on a
two-sample boundary, one sample per store (IqOut::put: ofdm_kernel's else branch, o32_store) elsewhere -- that is,
whenever the caller's iq_dev sits an odd number of samples past a 16-byte (cf32) or 8-byte (sc16) boundary, as a
GNU Radio output buffer at an odd item offset or a frame packed into a ring does.  dvbt2ll_chain_run_device /
_run_streams / _run_plps accept any sample-aligned iq_dev (include/dvbt2ll_hip.h) and refuse anything else.

Each run writes into the middle of a byte buffer filled with 0xA5: the samples equal, byte for byte, a run into a
fresh aligned tensor (itself bit-exact against the oracle through the CPU model of the IFFT), and every byte
around the destination is still 0xA5 (the guard-interval wrap store and the 16-byte pair stores sit at the
buffer's ends)."""
import functools
import types

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS, MPLP_CONFIGS, ts_for_frames
import iq_check
from test_cpu_plan import GRID, grid_cfg

pytestmark = pytest.mark.gpu

PAD = 4096
FILL = 0xA5
# name -> (format, gain, bytes per sample)
FORMATS = {"cf32": (dvbt2ll.IQ_CF32, 1.0, 8), "sc16": (dvbt2ll.IQ_SC16, 0.2, 4)}
# cfg1: 4K ofdm_kernel; an 8K grid point; ofdm32_kernel with three and two data symbols (the second with EQ);
# three PLPs: the MULTI instantiation through run_plps
SHAPES = ["cfg1", "8k_pp8_ext_64qam", "32k_pp4_ext_cfg3like", "32k_pp7_eq", "mplp3_4k"]


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module", autouse=True)
def _release_handles():
    """the shapes' chain handles are shared by this module's tests and freed with it"""
    yield
    _reference.cache_clear()
    _shape.cache_clear()


@functools.lru_cache(maxsize=None)
def _shape(name):
    """the shape's chain handle (two frames per run; a multi-PLP launch unit if that is larger), its TS on the
    device, a launcher run(iq_ptr) and the oracle's carriers per frame"""
    torch = _torch()
    if name in MPLP_CONFIGS:
        from test_gpu_mplp import _device_ts, oracle_frames
        cfg = MPLP_CONFIGS[name]
        n = max(2, cfg.unit_frames)
        ch = dvbt2ll.Chain(cfg, max_frames=n)
        assert ch.nplp > 1
        bufs, bases, lens = _device_ts(cfg, 0, n)
        ref, pg, _, _ = oracle_frames(cfg, n)

        def run(ptr):
            ch.run_plps([b.data_ptr() for b in bufs], bases, lens, 0, n, ptr, torch.cuda.current_stream().cuda_stream)
    else:
        from test_gpu_chain import oracle_chain
        cfg = CONFIGS[name] if name in CONFIGS else grid_cfg(dict(GRID)[name])
        n = 2
        ch = dvbt2ll.Chain(cfg, max_frames=n)
        ts, base = ts_for_frames(cfg, 0, n)
        bufs = [torch.from_numpy(ts).cuda()]
        ref, pg = oracle_chain(cfg, n)

        def run(ptr):
            ch.run_device(bufs[0].data_ptr(), base, len(ts), 0, n, ptr, torch.cuda.current_stream().cuda_stream)
    return types.SimpleNamespace(name=name, cfg=cfg, ch=ch, n=n, per=ch.iq_per_frame, run=run, keep=bufs,
                                 carriers=[r[0] for r in ref], pg=pg)


def _aligned(sh, fmt):
    """the run into a fresh tensor's base address, as bytes"""
    torch = _torch()
    f, gain, SB = FORMATS[fmt]
    sh.ch.set_output(gain, f)
    out = torch.empty(sh.n * sh.per * SB, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    sh.run(out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(name, fmt):
    """the aligned run, checked once against the oracle: bit-exact through the CPU model of the GPU IFFT with
    this format's output step"""
    sh = _shape(name)
    f, gain, SB = FORMATS[fmt]
    ref = _aligned(sh, fmt)
    iq = ref.view(np.complex64) if fmt == "cf32" else ref.view(np.int16).reshape(-1, 2)
    for k in range(sh.n):
        iq_check.check_frame_exact(iq[k * sh.per:(k + 1) * sh.per], sh.carriers[k], sh.cfg.pg_args(), sh.pg.guard,
                                   sh.pg.normalization, "%s %s frame %d" % (name, fmt, k), gain=gain, fmt=f)
    ref.setflags(write=False)
    return ref


def _sentinel_buffer(nbytes):
    torch = _torch()
    buf = torch.full((PAD + nbytes + PAD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf


def _check_dest(buf, off, want, ctx):
    """the bytes at [off, off + len(want)) are want; every other byte of the buffer is still the fill"""
    _torch().cuda.synchronize()
    host = buf.cpu().numpy()
    before, got, after = host[:off], host[off:off + len(want)], host[off + len(want):]
    bad = np.nonzero(before != FILL)[0]
    assert bad.size == 0, "%s: %d bytes written before the destination, nearest %d bytes in front" % (
        ctx, bad.size, off - bad[-1])
    bad = np.nonzero(after != FILL)[0]
    assert bad.size == 0, "%s: %d bytes written past the destination, first %d bytes past its end" % (
        ctx, bad.size, bad[0])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d of %d bytes differ from the aligned run, first at sample byte %d" % (
        ctx, bad.size, want.size, bad[0])


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", SHAPES)
def test_iq_destination_offsets(gpu, name, fmt):
    """destinations 0..3 samples past a 16-byte boundary: odd offsets take the one-sample stores, even ones the
    paired stores; the same bytes either way, and nothing outside"""
    sh = _shape(name)
    f, gain, SB = FORMATS[fmt]
    want = _reference(name, fmt)
    sh.ch.set_output(gain, f)
    buf = _sentinel_buffer(want.size)
    for k in (0, 1, 2, 3):
        buf.fill_(FILL)
        off = PAD + k * SB
        sh.run(buf.data_ptr() + off)
        _check_dest(buf, off, want, "%s %s +%d samples" % (name, fmt, k))


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", ["cfg1", "32k_pp7_eq"])
def test_iq_destination_odd_graph_mode(gpu, name, fmt):
    """the odd destination through the hipGraph launch path: first launch (capture) and relaunch (re-armed nodes)"""
    sh = _shape(name)
    f, gain, SB = FORMATS[fmt]
    want = _reference(name, fmt)
    sh.ch.set_output(gain, f)
    buf = _sentinel_buffer(want.size)
    off = PAD + SB
    sh.ch.set_graph(True)
    try:
        for launch in ("first launch", "relaunch"):
            buf.fill_(FILL)
            sh.run(buf.data_ptr() + off)
            _check_dest(buf, off, want, "%s %s graph %s" % (name, fmt, launch))
    finally:
        sh.ch.set_graph(False)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_iq_destination_odd_streams(gpu, fmt):
    """run_streams, 3 streams x 1 frame at an odd sample: iq_samples_per_frame is even, so every stream's frame
    starts at an odd sample; each stream's IQ is the single-stream handle's on that stream's TS"""
    torch = _torch()
    cfg = CONFIGS["cfg1"]
    f, gain, SB = FORMATS[fmt]
    S = 3
    ch = dvbt2ll.Chain(cfg, max_frames=S)
    one = dvbt2ll.Chain(cfg, max_frames=1)
    for c in (ch, one):
        c.set_output(gain, f)
    per = ch.iq_per_frame
    assert per % 2 == 0
    tss = [ts_for_frames(cfg, 0, 1, seed=s + 1) for s in range(S)]
    base, n = tss[0][1], len(tss[0][0])
    stride = (n + 255) // 256 * 256
    host = np.zeros((S, stride), np.uint8)
    for s, (ts, b) in enumerate(tss):
        assert b == base and len(ts) == n
        host[s, :n] = ts
    ts_dev = torch.from_numpy(host.reshape(-1)).cuda()
    want = np.concatenate([one.run(0, 1, ts=ts, ts_base=b).view(np.uint8).reshape(-1) for ts, b in tss])
    assert want.size == S * per * SB
    buf = _sentinel_buffer(want.size)
    off = PAD + SB
    ch.run_streams(ts_dev.data_ptr(), stride, S, base, n, 0, 1, buf.data_ptr() + off,
                   torch.cuda.current_stream().cuda_stream)
    _check_dest(buf, off, want, "cfg1 %s 3 streams +1 sample" % fmt)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", ["cfg1", "mplp3_4k"])
def test_iq_destination_below_sample_alignment_is_refused(gpu, name, fmt):
    """iq_dev half a sample past a sample (4 bytes for cf32, 2 for sc16): DVBT2LL_EINVAL before anything is
    launched -- the buffer keeps its fill, sync_errors() is unchanged -- and the next valid call succeeds"""
    sh = _shape(name)
    f, gain, SB = FORMATS[fmt]
    want = _reference(name, fmt)
    sh.ch.set_output(gain, f)
    buf = _sentinel_buffer(want.size)
    errs = sh.ch.sync_errors()
    for k in (0, 1):
        with pytest.raises(dvbt2ll.DVBT2Error):
            sh.run(buf.data_ptr() + PAD + k * SB + SB // 2)
    _torch().cuda.synchronize()
    assert (buf.cpu().numpy() == FILL).all()
    assert sh.ch.sync_errors() == errs
    sh.run(buf.data_ptr() + PAD + SB)
    _check_dest(buf, PAD + SB, want, "%s %s after a refused call" % (name, fmt))
    assert sh.ch.sync_errors() == errs
