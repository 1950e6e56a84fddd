"""T2-MI output on the GPU (dvbt2ll.T2miFramer) against tests/t2mi_out_ref.py: bytes, counters and next position, all
exact.  Every device run has its inputs inside poisoned arrays and its output inside a poisoned array with guard
regions; the guards and the bytes past the last packet must stay untouched.  No test looks for a fault."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS
import bbf_ref as BR
import t2mi_out_ref as O
import t2mi_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
_STREAM = []


def _side_stream():
    """a torch stream with a handle of its own: handle 0 reads as "the framer's own stream" in the C ABI"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def _framer(sh, max_frames=8):
    return dvbt2ll.T2miFramer(sh.pid, plps=sh.plps, frames_per_superframe=sh.fps, aux=sh.aux, stream_id=sh.stream_id,
                              max_frames=max_frames)


def _place(arr, phase):
    """arr on the device inside a poisoned array, at a 4-byte phase"""
    import torch
    buf = torch.full((2 * GUARD + len(arr) + 16,), POISON, dtype=torch.uint8, device="cuda")
    off = GUARD + phase
    buf[off:off + len(arr)] = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    return buf, off


def device_run(fr, sh, bb, aux, nframes, start=(0, 0, 0), src_phase=1, dst_phase=3, extra_cap=2):
    """one run_device inside poisoned arrays; returns (ts bytes, result) after checking the guards"""
    import torch
    st = _side_stream()
    N = fr.ts_packets(nframes)
    with torch.cuda.stream(st):
        ins = [_place(b, (src_phase + k) % 4) for k, b in enumerate(bb)]
        ax = _place(aux, (src_phase + 2) % 4)
        out = torch.full((2 * GUARD + (N + extra_cap) * 188 + 16,), POISON, dtype=torch.uint8, device="cuda")
        oo = GUARD + dst_phase
        fr.run_device([b.data_ptr() + o for b, o in ins], nframes, out.data_ptr() + oo, N + extra_cap,
                      aux_ptr=ax[0].data_ptr() + ax[1], aux_stride=sh.aux_stride, aux_off=sh.aux_off, start=start,
                      stream=st.cuda_stream)
    res = fr.result()
    st.synchronize()
    o = out.cpu().numpy()
    assert (o[:oo] == POISON).all() and (o[oo + N * 188:] == POISON).all(), "written outside the call's packets"
    for (b, off), src in zip(ins + [ax], list(bb) + [aux]):
        g = b.cpu().numpy()
        assert (g[:off] == POISON).all() and (g[off + len(src):] == POISON).all()
    return o[oo:oo + N * 188].copy(), res


def check(fr, sh, nframes, start=(0, 0, 0), seed=1, ref=O.frame, **kw):
    bb, aux = sh.inputs(nframes, seed=seed)
    ts, nxt, cnt, by_type = ref(sh, bb, aux, nframes, start)
    assert fr.ts_packets(nframes) == len(ts) // 188
    got, res = device_run(fr, sh, bb, aux, nframes, start, **kw)
    bad = np.nonzero(got != ts)[0]
    assert bad.size == 0, "%s %s n=%d: first difference at TS packet %d byte %d" % (
        sh.plps, sh.aux, nframes, bad[0] // 188, bad[0] % 188)
    assert tuple(res.next) == nxt and res.counters == cnt and res.by_type == by_type, (res, nxt, cnt, by_type)
    return got, bb, aux


# ---------------------------------------------------------------------------------------- 1. layout
@pytest.mark.parametrize("Lb", [O.LB_SMALL, O.LB_ODD])
def test_one_plp_every_phase(gpu, Lb):
    for F in (1, 2, 3):
        sh = O.Shape([(4, Lb, F)])
        fr = _framer(sh)
        for n in range(1, 6):
            check(fr, sh, n, start=(n, 17 * n, n), seed=n, src_phase=(n + F) % 4, dst_phase=n % 4)


def test_aux_sweep(gpu):
    """tests/test_cpu_t2mi_out.py asserts that this list holds every entry state and edge"""
    for i, (sh, n) in enumerate(O.aux_sweep_cases()):
        check(_framer(sh, max_frames=4), sh, n, start=(i, i, i & 15), seed=i, src_phase=i % 4, dst_phase=(i // 4) % 4)


def test_three_plps_slots_before_and_after_dirty_pad_bits(gpu):
    sh = O.THREE_PLPS
    assert [p[0] for p in sh.plps] == [7, 0, 200] and sh.aux[1][1] % 8
    fr = _framer(sh)
    for n, ph in ((1, 0), (3, 1), (4, 2), (5, 3)):
        got, bb, aux = check(fr, sh, n, start=(1, 3, 5), seed=n, src_phase=ph, dst_phase=3 - ph)
        res = R.parse(got, sh.pid, [])
        l1 = res.packets[res.packets["packet_type"] == 0x10]
        assert len(l1) == n
        for f, r in enumerate(l1):          # the last payload byte: dirty in the input, its 5 pad bits zero here
            o = f * sh.aux_stride + sh.aux_off[1] + sh.aux_bytes[1] - 1
            assert got[int(r["ts_byte"]) // 188 * 188] == 0x47
            assert sh.aux_payload(aux, f, 1)[-1] == aux[o] & 0xE0
        assert any(aux[f * sh.aux_stride + sh.aux_off[1] + sh.aux_bytes[1] - 1] & 0x1F for f in range(n))
    for sh2 in O.EDGE_SHAPES:
        check(_framer(sh2), sh2, 3, start=(0, 9, 9))


# ---------------------------------------------------------------------------------------- 2. counter wraps
def test_counters_wrap_mid_call(gpu):
    sh = O.Shape([(1, O.LB_SMALL, 2)], aux=[(0x20, 88, 0)], fps=3)
    fr = _framer(sh)
    n = 6                                   # 18 packets, 70 TS packets
    # packet_count 255 -> 0, cc 15 -> 0, frame_idx 2 -> 0 and superframe_idx 15 -> 0 all inside the call
    start = (3 * 15 + 1, 250, 9)
    got, _, _ = check(fr, sh, n, start=start)
    res = R.parse(got, sh.pid, [(1, O.LB_SMALL)])
    pc, sf = res.packets["packet_count"], res.packets["superframe_idx"]
    assert 255 in pc[:-1] and pc[list(pc).index(255) + 1] == 0
    assert sf[0] == 15 and sf[list(sf).index(0) - 1] == 15 and sf[-1] == 1      # 15 -> 0 -> 1
    fi = res.packets["frame_idx"][res.packets["packet_type"] == 0]
    assert list(fi[::2]) == [1, 2, 0, 1, 2, 0]                                   # wraps at frames_per_superframe
    cc = got.reshape(-1, 188)[:, 3] & 15
    assert 15 in cc[:-1] and cc[list(cc).index(15) + 1] == 0
    assert res.counters["discontinuities"] == 0


# ---------------------------------------------------------------------------------------- 3. round trips
def test_deframer_on_the_device_returns_every_plp(gpu):
    import torch
    sh, n = O.THREE_PLPS, 4
    fr = _framer(sh)
    bb, aux = sh.inputs(n)
    N = fr.ts_packets(n)
    st = _side_stream()
    de = dvbt2ll.T2miDeframer(sh.pid, plps=[(p[0], p[1]) for p in sh.plps], max_ts_bytes=N * 188, max_packets=n * sh.P)
    with torch.cuda.stream(st):
        bb_d = [torch.from_numpy(b).cuda() for b in bb]
        aux_d = torch.from_numpy(aux).cuda()
        ts_d = torch.empty(N * 188, dtype=torch.uint8, device="cuda")
        outs = [torch.zeros(len(b), dtype=torch.uint8, device="cuda") for b in bb]
        fr.run_device([b.data_ptr() for b in bb_d], n, ts_d.data_ptr(), N, aux_ptr=aux_d.data_ptr(),
                      aux_stride=sh.aux_stride, aux_off=sh.aux_off, start=(5, 6, 7), stream=st.cuda_stream)
        de.run_device(ts_d.data_ptr(), N * 188, [o.data_ptr() for o in outs], [n * p[2] for p in sh.plps],
                      stream=st.cuda_stream)           # same stream: no synchronise between framer and deframer
    res = de.result()
    st.synchronize()
    assert res.counters["accepted"] == n * sh.P == len(res.packets)
    assert res.counters["discontinuities"] == 0 and res.counters["bad_pointers"] == 0
    assert res.counters["broken"] == res.counters["crc_errors"] == res.counters["len_errors"] == 0
    assert res.blocks == [n * p[2] for p in sh.plps]
    for k in range(3):
        np.testing.assert_array_equal(outs[k].cpu().numpy(), bb[k])
        assert de.interleaving_frames(k, res) == [sh.plps[k][2]] * n


def test_chain_iq_from_deframed_buffers_equals_the_originals(gpu):
    """cfg1q (Lb = 879, F = 2): BBFRAMEs -> T2miFramer -> T2miDeframer -> Chain gives the IQ of the BBFRAMEs themselves"""
    import torch
    cfg, n = CONFIGS["cfg1q"], 3
    F, L = cfg.fecblocks, BR.bbframe_len(cfg)
    bbf = BR.oracle_bbframes(cfg, 0, n)
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    fr = dvbt2ll.T2miFramer(O.PID, chain=ch, max_frames=n)
    assert fr.plps == [(0, L, F)]
    N = fr.ts_packets(n)
    de = dvbt2ll.T2miDeframer(O.PID, chain=ch, max_ts_bytes=N * 188, max_packets=64)
    side = _side_stream()              # handle 0 (torch's default stream) would put each handle on a stream of its own
    st = side.cuda_stream
    with torch.cuda.stream(side):
        src = torch.from_numpy(bbf.copy()).cuda()
        ts_d = torch.empty(N * 188, dtype=torch.uint8, device="cuda")
        back = torch.zeros(n * F * L, dtype=torch.uint8, device="cuda")
        iq = [torch.zeros((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
        ch.run_device(src.data_ptr(), 0, src.numel(), 0, n, iq[0].data_ptr(), st)
        fr.run_device([src.data_ptr()], n, ts_d.data_ptr(), N, stream=st)
        de.run_device(ts_d.data_ptr(), N * 188, [back.data_ptr()], [n * F], stream=st)
        ch.run_device(back.data_ptr(), 0, back.numel(), 0, n, iq[1].data_ptr(), st)
    torch.cuda.synchronize()
    assert fr.result().counters["ts_packets"] == N and de.result().counters["accepted"] == n * F
    np.testing.assert_array_equal(back.cpu().numpy(), bbf)
    assert np.array_equal(iq[0].cpu().numpy().view(np.uint32), iq[1].cpu().numpy().view(np.uint32))
    assert ch.bbheader_errors() == 0
    np.testing.assert_array_equal(ts_d.cpu().numpy(), O.frame(O.Shape([(0, L, F)], fps=fr.frames_per_superframe),
                                                             [bbf], np.zeros(1, np.uint8), n)[0])


def test_two_chained_calls_parse_as_one(gpu):
    sh = O.EDGE_SHAPES[0]
    fr = _framer(sh)
    n1, n2, start = 2, 3, (8, 200, 11)
    bb, aux = sh.inputs(n1 + n2)
    one, _ = device_run(fr, sh, bb, aux, n1 + n2, start)
    a, ra = device_run(fr, sh, bb, aux, n1, start)
    cut = [n1 * p[2] * p[1] for p in sh.plps]
    b, rb = device_run(fr, sh, [x[c:] for x, c in zip(bb, cut)], aux[n1 * sh.aux_stride:], n2, tuple(ra.next))
    np.testing.assert_array_equal(a, O.frame(sh, bb, aux, n1, start)[0])
    plps = [(p[0], p[1]) for p in sh.plps]
    whole, both = R.parse(one, sh.pid, plps), R.parse(np.concatenate([a, b]), sh.pid, plps)
    fields = ["packet_type", "packet_count", "superframe_idx", "t2mi_stream_id", "payload_len", "flags",
              "intl_frame_start", "frame_idx", "plp_id", "out_index", "block"]
    assert len(whole.packets) == len(both.packets) == (n1 + n2) * sh.P
    for f in fields:
        np.testing.assert_array_equal(whole.packets[f], both.packets[f], err_msg=f)
    np.testing.assert_array_equal(whole.bbframes[0], both.bbframes[0])
    assert both.counters["discontinuities"] == 0 and both.counters["accepted"] == (n1 + n2) * sh.P
    assert tuple(rb.next)[:2] == tuple(fr.result().next)[:2] == (start[0] + n1 + n2, (start[1] + (n1 + n2) * sh.P) & 255)
    cc = np.concatenate([a, b]).reshape(-1, 188)[:, 3] & 15
    assert (np.diff(cc.astype(int)) % 16 == 1).all()


# ---------------------------------------------------------------------------------------- 4. robustness
def test_refusals_launch_nothing(gpu):
    import torch
    sh, n = O.EDGE_SHAPES[0], 2
    fr = _framer(sh, max_frames=4)
    bb, aux = sh.inputs(n)
    before = fr.run([bb[0]], n, aux=aux, aux_stride=sh.aux_stride, aux_off=sh.aux_off)
    bb_d, aux_d = torch.from_numpy(bb[0]).cuda(), torch.from_numpy(aux).cuda()
    N = fr.ts_packets(n)
    out = torch.full((N * 188,), POISON, dtype=torch.uint8, device="cuda")
    kw = dict(aux_ptr=aux_d.data_ptr(), aux_stride=sh.aux_stride, aux_off=sh.aux_off)
    for args, k2 in ((([bb_d.data_ptr()], n, out.data_ptr(), N - 1), {}),        # capacity below the exact count
                     (([bb_d.data_ptr()], 5, out.data_ptr(), 1 << 20), {}),       # more than max_frames
                     (([bb_d.data_ptr()], -1, out.data_ptr(), N), {}),
                     (([0], n, out.data_ptr(), N), {}),
                     (([bb_d.data_ptr()], n, 0, N), {}),
                     (([bb_d.data_ptr()], n, out.data_ptr(), N), dict(aux_ptr=0)),
                     (([bb_d.data_ptr()], n, out.data_ptr(), N), dict(aux_stride=-1)),
                     (([bb_d.data_ptr()], n, out.data_ptr(), N), dict(aux_off=[0, -1, 0, 0])),
                     (([bb_d.data_ptr()], n, out.data_ptr(), N), dict(start=(-1, 0, 0))),
                     (([bb_d.data_ptr()], n, out.data_ptr(), N), dict(start=(0, 256, 0))),
                     (([bb_d.data_ptr()], n, out.data_ptr(), N), dict(start=(0, 0, 16)))):
        with pytest.raises(dvbt2ll.DVBT2Error):
            fr.run_device(*args, **{**kw, **k2})
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert fr.result().counters == before.counters          # the last real run's result still stands
    with pytest.raises(dvbt2ll.DVBT2Error):
        fr.ts_packets(5)
    assert fr.ts_packets(0) == 0
    for plps in ([], [(k, 654, 1) for k in range(9)], [(1, 654, 1), (1, 654, 1)], [(1, 655, 1)], [(1, 654, 0)]):
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.T2miFramer(O.PID, plps=plps)


def test_run_host(gpu):
    sh, n, start = O.THREE_PLPS, 3, (2, 254, 15)
    fr = _framer(sh)
    bb, aux = sh.inputs(n)
    res = fr.run(bb, n, aux=aux, aux_stride=sh.aux_stride, aux_off=sh.aux_off, start=start)
    ts, nxt, cnt, by_type = O.frame(sh, bb, aux, n, start)
    np.testing.assert_array_equal(res.ts, ts)
    assert tuple(res.next) == nxt and res.counters == cnt and res.by_type == by_type
    plain = O.Shape([(0, O.LB_SMALL, 1)])
    bb, aux = plain.inputs(2)
    np.testing.assert_array_equal(_framer(plain).run(bb, 2).ts, O.frame(plain, bb, aux, 2)[0])


def test_params_from_chain_refuses_a_multi_frame_interleaving_frame(gpu):
    from dvbt2ll.configs import MPLP_CONFIGS, IF_CONFIGS
    ch = dvbt2ll.Chain(IF_CONFIGS["mix_4k"], max_frames=4)      # PLP 0: TIME_IL_TYPE 1, P_I = 2
    with pytest.raises(dvbt2ll.DVBT2Error):
        dvbt2ll.T2miFramer(O.PID, chain=ch)
    m = MPLP_CONFIGS["mplp3_4k"]
    fr = dvbt2ll.T2miFramer(O.PID, chain=dvbt2ll.Chain(m, max_frames=2), plp_ids=(7, 0, 200))
    assert [(p[0], p[2]) for p in fr.plps] == [(7, m.plps[0].fecblocks), (0, m.plps[1].fecblocks), (200, m.plps[2].fecblocks)]


TOOL = Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "dvbt2ll" / "dvbt2ll_tx"


def _tool(*args):
    return subprocess.run([str(TOOL)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_t2mi_out_and_back(gpu, tmp_path):
    """--input bbframe --t2mi-out writes the reference framer's bytes of the frames it encodes (batch by batch, the
    position carried on); --input t2mi on that file gives the same IQ"""
    cfg, n = CONFIGS["cfg1q"], 3
    F, L = cfg.fecblocks, BR.bbframe_len(cfg)
    bbf = BR.oracle_bbframes(cfg, 0, n)
    (tmp_path / "in.bbf").write_bytes(bbf.tobytes())
    r = _tool("--preset", "cfg1q", "--input", "bbframe", "--in", tmp_path / "in.bbf", "--out", tmp_path / "a.iq",
              "--batch", 2, "--t2mi-out", tmp_path / "gw.ts", "--t2mi-pid", "0x321", "--t2mi-stream-id", 3)
    assert r.returncode == 0, r.stderr
    fps = dvbt2ll.T2miFramer(0x321, chain=dvbt2ll.Chain(cfg, max_frames=1), max_frames=1).frames_per_superframe
    sh = O.Shape([(0, L, F)], fps=fps, stream_id=3, pid=0x321)
    none = np.zeros(1, np.uint8)
    a = O.frame(sh, [bbf], none, 2)
    b = O.frame(sh, [bbf[2 * F * L:]], none, 1, a[1])
    want = np.concatenate([a[0], b[0]])
    got = np.frombuffer((tmp_path / "gw.ts").read_bytes(), np.uint8)
    np.testing.assert_array_equal(got, want)
    assert "t2mi-out: %d T2 frames" % n in r.stderr and "ts_packets %d," % (len(want) // 188) in r.stderr
    r = _tool("--preset", "cfg1q", "--input", "t2mi", "--pid", "0x321", "--in", tmp_path / "gw.ts", "--out",
              tmp_path / "b.iq", "--batch", 2)
    assert r.returncode == 0, r.stderr
    x, y = (tmp_path / "a.iq").read_bytes(), (tmp_path / "b.iq").read_bytes()
    assert len(x) == n * dvbt2ll.Chain(cfg, max_frames=1).iq_per_frame * 8 and x == y


# ---------------------------------------------------------------------------------------- 5. the long stream
def test_long_stream_past_every_grid_cap(gpu):
    """20000 T2 frames of one Lb = 654 BBFRAME: 20000 T2-MI packets and 72609 TS packets in one call.  The caps this
    passes (csrc/t2mi_out_kernels.hip): the CRC pass's grid of CRC_MAX_BLOCKS = 4096 workgroups x 4 wavefronts, one
    packet each (16384 packets per stride); the emit pass's grid of EMIT_MAX_BLOCKS = 2048 workgroups x 4 wavefronts x
    EMIT_RUN = 8 TS packets (65536 TS packets per stride).  Compared with the numpy restatement, which
    tests/test_cpu_t2mi_out.py holds to the sequential framer and shows to see a dropped carry of d."""
    sh, n = O.Shape([(0, O.LB_SMALL, 1)]), 20000
    fr = _framer(sh, max_frames=n)
    assert n * sh.P > 4096 * 4 and fr.ts_packets(n) > 2048 * 4 * 8
    check(fr, sh, n, start=(123456, 77, 5), ref=O.frame_numpy, src_phase=2, dst_phase=1)
