"""GPU: the MPE-FEC encapsulator (dvbt2ll_mpefec_*, csrc/mpefec_kernels.hip) against tests/mpefec_ref.py's sequential
restatement: bytes, counters and resume position, all exact.  Every device run here has its PDUs inside a larger
poisoned array and its output inside a poisoned array with guard regions, at output and PDU-buffer alignments 0 .. 3;
the guards and the bytes past the last packet must stay untouched."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS, ts_for_frames
import mpefec_cases as C
import mpefec_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
TILE = 512          # MF_TILE of csrc/mpefec_kernels.h: sections per tile of the state scan
ROUND = 32 * TILE   # sections one compose round covers
EMIT = 64           # EMIT_PKTS of csrc/mpefec_kernels.hip: packets per emit group
SCAN_TILE = 1024    # SCAN_TILE: PDUs per tile of the 64-bit sum scan.  Its single-workgroup pass over the tile sums takes
                    # a second round at 256 tiles (262 144 PDUs): beyond the 2 x 10^4 PDUs a test here may use, that
                    # round is covered by reading only (it is mpe_kernels.hip's loop, which test_gpu_mpe.py does run)
LANE_MAX = 192      # CRC_LANE_MAX: MPE sections up to here take a lane, longer ones and MPE-FEC sections a wavefront


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1)


_STREAM = []


def _side_stream():
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def device_run(enc, pdu, off, start=(0, 0, 0, 0, 0), cap=None, flush=False, align=(0, 0), stream=None):
    """one run_device with everything inside poisoned arrays; returns the result with ts filled in, after checking
    the guards.  align: (PDU buffer, output) byte alignments.  cap None: packet_bound"""
    import torch
    st = _side_stream() if stream is None else stream
    n = len(off) - 1
    cap = enc.packet_bound(len(pdu), n) if cap is None else cap
    with torch.cuda.stream(st):
        buf = torch.full((2 * GUARD + len(pdu) + 16,), POISON, dtype=torch.uint8, device="cuda")
        at = GUARD + align[0]
        if len(pdu):
            buf[at:at + len(pdu)] = torch.from_numpy(np.array(pdu, np.uint8)).cuda()
        off_d = torch.from_numpy(np.array(off, np.uint32).view(np.int32)).cuda()
        out = torch.full((2 * GUARD + cap * 188 + 16,), POISON, dtype=torch.uint8, device="cuda")
        a = GUARD + align[1]
        enc.run_device(buf.data_ptr() + at, len(pdu), off_d.data_ptr(), n, out.data_ptr() + a, cap, start=start,
                       flush=flush, stream=st.cuda_stream)
    res = enc.result()
    st.synchronize()
    o = out.cpu().numpy()
    nb = res.counters["ts_packets"] * 188
    assert res.counters["ts_packets"] <= cap
    assert (o[:a] == POISON).all() and (o[a + nb:] == POISON).all(), "written outside its packets"
    res.ts = o[a:a + nb].copy()
    got = buf.cpu().numpy()
    assert (got[:at] == POISON).all() and (got[at + len(pdu):] == POISON).all()
    return res


def same(res, ref, ctx=""):
    assert tuple(res.resume) == tuple(ref.resume), (ctx, res.resume, ref.resume)
    assert res.counters == ref.counters, (ctx, res.counters, ref.counters)
    np.testing.assert_array_equal(res.ts, ref.ts, err_msg=str(ctx))


def ref_for(enc, pdu, off, **kw):
    return R.encap(pdu, off, rows=enc.rows, D=enc.data_columns, K=enc.rs_columns, pid=enc.pid, mac=enc.mac,
                   mac_mode=enc.mac_mode, packing=enc.packing, max_frames=enc.max_frames, **kw)


def check(enc, pdu, off, ctx, **kw):
    ref = ref_for(enc, pdu, off, **{k: v for k, v in kw.items() if k in ("start", "cap", "flush")})
    res = device_run(enc, pdu, off, **kw)
    same(res, ref, ctx)
    return res, ref


_ENC = {}


def enc_of(rows, D, K, mac_mode=0, packing=1, max_frames=64, max_pdu_bytes=1 << 20, max_pdus=1 << 12):
    """one handle per shape and mode, shared by the tests (a handle holds scratch only)"""
    key = (rows, D, K, mac_mode, packing, max_frames, max_pdu_bytes, max_pdus)
    if key not in _ENC:
        _ENC[key] = dvbt2ll.MpeFecEncapsulator(pid=C.PID, rows=rows, data_columns=D, rs_columns=K, mac=R.MAC,
                                               mac_from_dest=bool(mac_mode), packing=packing, max_frames=max_frames,
                                               max_pdu_bytes=max_pdu_bytes, max_pdus=max_pdus)
    return _ENC[key]


# ---------------------------------------------------------------------------------------- 1. the frame forms
@pytest.mark.parametrize("mac_mode,packing", [(0, 1), (1, 1), (0, 0), (1, 0)])
def test_frame_cases_rows_256(gpu, mac_mode, packing):
    k = 0
    for D, K in C.SHAPES:
        enc = enc_of(256, D, K, mac_mode, packing)
        for name, pdus in C.frame_cases(256, D).items():
            pdu, off = R.pack(pdus)
            for flush in (True, False):
                k += 1
                check(enc, pdu, off, (D, K, name, flush), flush=flush, align=(k % 4, (k // 4) % 4),
                      start=(0, 0, 0, k & 15, (4090 + k) & 0xFFF))


@pytest.mark.parametrize("rows", [512, 768, 1024])
def test_frame_cases_other_rows(gpu, rows):
    k = 0
    for (D, K), (mac_mode, packing) in zip(C.SHAPES, ((1, 1), (0, 0), (1, 1))):
        enc = enc_of(rows, D, K, mac_mode, packing)
        for name, pdus in C.frame_cases(rows, D).items():
            k += 1
            pdu, off = R.pack(pdus)
            res, _ = check(enc, pdu, off, (D, K, name), flush=True, align=(k % 4, (k + 1) % 4))
            if packing:
                got = [d for f in R.receive(res.ts, K) for d in f.datagrams]
                assert got == R.valid_pdus(pdu, off, rows, D), name


@pytest.mark.parametrize("rows", R.ROWS)
def test_largest_shapes_one_and_two_full_frames(gpu, rows):
    """D 191, K 64 with 1500-byte datagrams: every RS workgroup of a frame (rows / 256 of them), a frame of the
    largest table"""
    enc = enc_of(rows, 191, 64, 1, 1, max_frames=4)
    per = 191 * rows // 1500
    for frames in (1, 2):
        pdus = [C.ip(1500, k, 0x60 if k % 4 == 1 else 0x45, C.V4_GROUP if k % 3 == 0 and k % 4 != 1 else None)
                for k in range(frames * per + 1)]
        pdu, off = R.pack(pdus)
        res, ref = check(enc, pdu, off, (rows, frames), flush=False, align=(1 + frames, frames))
        # without a flush the last closed frame's last packet stays open: the resume position lies in that frame
        assert ref.counters["frames"] == frames - 1 and ref.resume[0] == (frames - 1) * per and ref.resume[1] == per + 63
    res, ref = check(enc, pdu, off, (rows, "flush"), flush=True, align=(0, 3))
    assert ref.counters["frames"] == 3 and ref.counters["flushed"] == 1


# ---------------------------------------------------------------------------------------- 2. frames across boundaries
def _full_frame(m, C_bytes, seed):
    """m datagrams that fill a frame of C_bytes exactly: m - 1 of one byte, then one of the rest"""
    return [bytes([0x45])] * (m - 1) + [C.ip(C_bytes - (m - 1), seed)]


def _across(boundaries, K, C_bytes, m_fill):
    """frames, each filled exactly, such that for every boundary B a frame's last MPE section is item B - 1 and its
    first MPE-FEC section item B"""
    pdus, items, k = [], 0, 0
    for B in boundaries:
        while B - items - (m_fill + K) >= 1:
            pdus += _full_frame(m_fill, C_bytes, k)
            items += m_fill + K
            k += 1
        m = B - items
        assert 1 <= m <= 200
        pdus += _full_frame(m, C_bytes, k)
        items += m + K
        k += 1
    return pdus + _full_frame(3, C_bytes, k) + [C.ip(30, k + 1)]


@pytest.mark.parametrize("D,K", [(1, 64), (2, 1), (3, 64), (1, 1)])
def test_frames_across_tile_and_round_boundaries(gpu, D, K):
    """rows 256: hundreds of frames; a frame's last MPE section and first MPE-FEC section lie across the first two
    tile boundaries of the state scan and across its first compose round"""
    m_fill = 1 if K == 64 else 60
    pdus = _across((TILE, 2 * TILE, ROUND), K, D * 256, m_fill)
    pdu, off = R.pack(pdus)
    parts = R.partition(pdu, off, 0, 256, D, True)[0]
    assert len(parts) > 250 and len(pdus) < 2 * 10 ** 4
    # the items before each frame's first MPE-FEC section
    firsts = np.cumsum([len(f[2]) for f in parts]) + K * np.arange(len(parts))
    assert all(B in firsts for B in (TILE, 2 * TILE, ROUND))
    enc = enc_of(256, D, K, 1, 1, max_frames=512, max_pdus=1 << 15)
    res, ref = check(enc, pdu, off, (D, K), flush=True, align=(D, K % 4))
    assert ref.counters["frames"] == len(parts) and ref.counters["ts_packets"] > 3 * EMIT
    check(enc_of(256, D, K, 0, 0, max_frames=512, max_pdus=1 << 15), pdu, off, (D, K, "packing 0"), flush=False,
          align=(1, 2))


def test_skipped_pdus_at_a_frames_first_and_last_slots(gpu):
    pdus = C.small_frames(60, 31)
    pdu, off = R.pack(pdus)
    parts = R.partition(pdu, off, 0, 256, 3, True)[0]
    assert len(parts) > 6
    for f in parts[1:5]:
        pdus[f[0]] = C.ip(40, f[0], 0x50)                 # the frame's first slot: nibble 5
        pdus[f[1] - 1] = C.ip(40, f[1], 0x10)             # ... and its last
    pdus[parts[5][0]] = C.ip(769, 9)                      # one byte more than D x rows: skipped by its length
    pdu, off = R.pack(pdus)
    enc = enc_of(256, 3, 2, 1, 1)
    res, ref = check(enc, pdu, off, "skips", flush=True, align=(1, 3))
    assert ref.counters["skipped_type"] == 8 and ref.counters["skipped_len"] == 1
    assert [d for f in R.receive(res.ts, 2) for d in f.datagrams] == R.valid_pdus(pdu, off, 256, 3)
    check(enc, pdu, off, "skips, open end", flush=False, align=(2, 0))
    pdu, off = R.pack([C.ip(9, 1, 0x50)] * 3)             # nothing valid at all
    check(enc, pdu, off, "no datagram", flush=True, align=(1, 2))
    check(enc, np.zeros(0, np.uint8), np.zeros(1, np.uint32), "no PDU", flush=True)


@pytest.mark.parametrize("packing", [1, 0])
def test_overlapping_valid_pdus_make_more_frames_than_the_grids_cover(gpu, packing):
    """off = 0, 200, 0, 200, ...: every second PDU is the same 200 bytes and valid, the ones between are skipped.  With
    rows 256, D 1 each is a frame of its own: 150 frames from a 200-byte buffer, where PDUs lying side by side could
    close 3: the gather, RS, MPE-FEC item and emit passes all take several trips"""
    pdu = np.frombuffer(C.ip(200, 30), np.uint8).copy()
    off = np.append(np.tile(np.array([0, 200], np.uint32), 150), np.uint32(0))
    enc = enc_of(256, 1, 64, 0, packing, max_frames=256)
    ref = ref_for(enc, pdu, off, flush=True)
    assert ref.counters["frames"] == 150 and ref.counters["skipped_len"] == 150
    assert ref.counters["ts_packets"] > enc.packet_bound(len(pdu), 300) + 16 * EMIT
    check(enc, pdu, off, "overlap", cap=ref.counters["ts_packets"] + 5, flush=True, align=(1, 3))
    a, _ = check(enc, pdu, off, "overlap, cut", cap=700, flush=True, align=(2, 1))
    b, _ = check(enc, pdu, off, "overlap, rest", cap=ref.counters["ts_packets"], start=a.resume, flush=True,
                 align=(3, 0))
    np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), ref.ts)
    same(enc.run(pdu, off, cap=ref.counters["ts_packets"] + 9, flush=True), ref, "host")


# ---------------------------------------------------------------------------------------- 3. cuts and chains
def _chain(enc, pdu, off, first, ctx, **kw):
    """continues from first until nothing is left; returns the results"""
    out = [first]
    while not out[-1].counters["flushed"]:
        assert len(out) < 40
        r, _ = check(enc, pdu, off, (ctx, len(out)), start=out[-1].resume, flush=True, **kw)
        out.append(r)
    return out


@pytest.mark.parametrize("packing", [1, 0])
def test_capacity_and_max_frames_cuts_with_continuation(gpu, packing):
    pdus = C.small_frames(40, 32)
    pdu, off = R.pack(pdus)
    wide = enc_of(256, 2, 3, 1, packing)
    whole = ref_for(wide, pdu, off, start=(0, 0, 0, 9, 4094), flush=True)
    n = whole.counters["ts_packets"]
    for k, cap in enumerate((0, 1, 2, 5, 6, 7, n // 2, n - 1, n)):
        a, _ = check(wide, pdu, off, ("cut", cap), cap=cap, flush=True, align=(k % 4, (k + 1) % 4),
                     start=(0, 0, 0, 9, 4094))
        b, _ = check(wide, pdu, off, ("rest", cap), start=a.resume, flush=True, align=((k + 2) % 4, k % 4))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert tuple(b.resume) == whole.resume
    for mf in (1, 2, 5):
        enc = enc_of(256, 2, 3, 1, packing, max_frames=mf)
        first, _ = check(enc, pdu, off, ("max_frames", mf), start=(0, 0, 0, 9, 4094), flush=True, align=(mf % 4, 1))
        rs = _chain(enc, pdu, off, first, ("max_frames", mf), align=(1, mf % 4))
        assert len(rs) >= whole.counters["frames"] // mf
        np.testing.assert_array_equal(np.concatenate([r.ts for r in rs]), whole.ts)
        assert tuple(rs[-1].resume) == whole.resume
        for name in R.COUNTERS[:-1]:
            assert sum(r.counters[name] for r in rs) == whole.counters[name], (mf, name)


@pytest.mark.parametrize("packing", [1, 0])
def test_chunked_calls_at_five_splits(gpu, packing):
    pdus = C.small_frames(90, 33)
    pdu, off = R.pack(pdus)
    enc = enc_of(256, 3, 2, 1, packing)
    whole = ref_for(enc, pdu, off, start=(0, 0, 0, 3, 7), flush=True)
    for j, k in enumerate((0, 1, 37, 64, len(pdus))):
        a, _ = check(enc, pdu[:off[k]], off[:k + 1], ("first", k), start=(0, 0, 0, 3, 7), align=(j % 4, (j + 2) % 4))
        b, _ = check(enc, pdu, off, ("second", k), start=a.resume, flush=True, align=((j + 1) % 4, j % 4))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert tuple(b.resume) == whole.resume
        for name in R.COUNTERS[:-1]:
            assert a.counters[name] + b.counters[name] == whole.counters[name], (k, name)
    # an open frame without a flush emits nothing, and a start whose frame is not closed comes back as it is
    one, _ = check(enc, pdu[:off[2]], off[:3], "open frame", start=(0, 1, 5, 3, 7))
    assert one.counters["ts_packets"] == 0 and tuple(one.resume) == (0, 1, 5, 3, 7)
    # inconsistent section / section_byte values are taken as 0
    check(enc, pdu, off, "section past the frame", start=(0, 3 * 256 + 1, 3, 1, 0), flush=True)   # the last one accepted
    check(enc, pdu, off, "byte past the section", start=(0, 1, 4000, 1, 0), flush=True)


def test_frame_ends_at_and_across_a_sum_scan_tile_boundary(gpu):
    """rows 256, D 1: frames of 64 one-datagram-filled slots.  Once 16 frames end exactly at PDU SCAN_TILE, so that
    a frame's sums come from two tiles of the scan; once a frame of 100 PDUs lies across it (PDUs 960 .. 1059), and a
    skipped PDU sits on the tile's last slot"""
    enc = enc_of(256, 1, 1, 1, 1, max_frames=64)
    pdus = []
    for f in range(20):
        pdus += _full_frame(64, 256, f)
    assert len(pdus) > SCAN_TILE
    pdu, off = R.pack(pdus)
    parts = R.partition(pdu, off, 0, 256, 1, True)[0]
    assert SCAN_TILE in [f[1] for f in parts]
    check(enc, pdu, off, "ends at the boundary", flush=True, align=(1, 2))
    pdus = []
    for f in range(15):
        pdus += _full_frame(64, 256, f)
    pdus += _full_frame(100, 256, 15) + _full_frame(64, 256, 16) + [C.ip(30, 17)]
    pdus[SCAN_TILE - 1] = C.ip(1, 0, 0x50)
    pdu, off = R.pack(pdus)
    parts = R.partition(pdu, off, 0, 256, 1, True)[0]
    assert any(f[0] < SCAN_TILE - 1 and f[1] > SCAN_TILE + 1 for f in parts)
    res, ref = check(enc, pdu, off, "across the boundary", flush=True, align=(3, 1))
    assert ref.counters["skipped_type"] == 1
    check(enc, pdu, off, "across the boundary, open end", flush=False, align=(2, 3))


def test_chained_calls_resume_at_a_section_index_above_4160(gpu):
    """rows 1024, D 191, 40-byte datagrams: a frame has 4889 MPE sections, so a call without a flush, whose last
    closed frame's last packet stays open, resumes at section 4889 + 63: the next call takes that start"""
    rows, per = 1024, 191 * 1024 // 40
    n = per + 300
    body = np.random.default_rng(41).integers(0, 256, n * 40, dtype=np.uint8)
    body[::40] = 0x45
    off = (np.arange(n + 1) * 40).astype(np.uint32)
    enc = enc_of(rows, 191, 64, 0, 1, max_frames=2, max_pdus=1 << 13)
    whole = ref_for(enc, body, off, start=(0, 0, 0, 2, 9), flush=True)
    a, _ = check(enc, body, off, "no flush", start=(0, 0, 0, 2, 9), align=(1, 3))
    assert a.resume[0] == 0 and a.resume[1] == per + 63 > 4160
    b, _ = check(enc, body, off, "then flush", start=a.resume, flush=True, align=(2, 1))
    np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
    assert tuple(b.resume) == whole.resume and whole.counters["frames"] == 2
    c, _ = check(enc, body, off, "cut inside an MPE section past 4160", cap=1400, align=(0, 2))
    assert 4160 < c.resume[1] < per
    d, _ = check(enc, body, off, "rest", start=c.resume, flush=True, align=(3, 0))
    np.testing.assert_array_equal(np.concatenate([c.ts, d.ts]), ref_for(enc, body, off, flush=True).ts)


def test_run_host(gpu):
    pdus = C.small_frames(70, 34)
    pdu, off = R.pack(pdus)
    for packing in (1, 0):
        enc = enc_of(256, 3, 64, 1, packing)
        same(enc.run(pdu, off, flush=True), ref_for(enc, pdu, off, flush=True), packing)
        a = enc.run(pdu, off, cap=5, start=(0, 0, 0, 2, 1))
        same(a, ref_for(enc, pdu, off, cap=5, start=(0, 0, 0, 2, 1)), "cap 5")
        same(enc.run(pdu, off, start=a.resume, flush=True), ref_for(enc, pdu, off, start=a.resume, flush=True), "rest")


# ---------------------------------------------------------------------------------------- 4. refusals, streams
def test_refusals_launch_nothing(gpu):
    import torch
    for kw in (dict(pid=0x1FFF), dict(pid=-1), dict(packing=2), dict(max_pdus=0), dict(max_pdu_bytes=1 << 31),
               dict(rows=255), dict(rows=1280), dict(data_columns=0), dict(data_columns=192), dict(rs_columns=0),
               dict(rs_columns=65), dict(max_frames=0), dict(max_frames=(1 << 16) + 1)):
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.MpeFecEncapsulator(**kw)
    with pytest.raises(ValueError):
        dvbt2ll.MpeFecEncapsulator(mac=b"\x01\x02")
    pdu, off = R.pack(C.small_frames(50, 35))
    enc = dvbt2ll.MpeFecEncapsulator(pid=C.PID, rows=256, data_columns=2, rs_columns=2, max_pdu_bytes=len(pdu),
                                     max_pdus=50)
    before = enc.run(pdu, off, flush=True).counters
    pdu_d = torch.from_numpy(pdu.copy()).cuda()
    off_d = torch.from_numpy(off.view(np.int32).copy()).cuda()
    out = torch.full((64 * 188,), POISON, dtype=torch.uint8, device="cuda")
    P, O, Q, L = pdu_d.data_ptr(), off_d.data_ptr(), out.data_ptr(), len(pdu)
    z = (0, 0, 0, 0, 0)
    for args, start in (((P, L + 1, O, 50, Q, 8), z), ((P, -1, O, 50, Q, 8), z), ((P, L, O, 51, Q, 8), z),
                        ((P, L, O, -1, Q, 8), z), ((P, L, O, 50, Q, -1), z),
                        ((P, L, O, 50, Q, 8), (-1, 0, 0, 0, 0)), ((P, L, O, 50, Q, 8), (51, 0, 0, 0, 0)),
                        ((P, L, O, 50, Q, 8), (50, 1, 0, 0, 0)), ((P, L, O, 50, Q, 8), (50, 0, 1, 0, 0)),
                        ((P, L, O, 50, Q, 8), (0, -1, 0, 0, 0)), ((P, L, O, 50, Q, 8), (0, 0, -1, 0, 0)),
                        ((P, L, O, 50, Q, 8), (0, 2 * 256 + 2, 0, 0, 0)),     # past D x rows + K - 1
                        ((P, L, O, 50, Q, 8), (0, 0, 4096, 0, 0)),
                        ((P, L, O, 50, Q, 8), (0, 0, 0, 16, 0)), ((P, L, O, 50, Q, 8), (0, 0, 0, -1, 0)),
                        ((P, L, O, 50, Q, 8), (0, 0, 0, 0, 4096)), ((P, L, O, 50, Q, 8), (0, 0, 0, 0, -1)),
                        ((0, L, O, 50, Q, 8), z), ((P, L, 0, 50, Q, 8), z), ((P, L, O, 50, 0, 8), z)):
        with pytest.raises(dvbt2ll.DVBT2Error):
            enc.run_device(*args, start=start)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert enc.result().counters == before        # the last real run's result still stands


def test_two_handles_two_streams(gpu):
    import torch
    pdus = C.small_frames(120, 36)
    pdu, off = R.pack(pdus)
    encs = [dvbt2ll.MpeFecEncapsulator(pid=C.PID + k, rows=256 * (k + 1), data_columns=3 - k, rs_columns=64 - 60 * k,
                                       mac_from_dest=bool(k), packing=1 - k, max_pdu_bytes=len(pdu),
                                       max_pdus=len(pdus)) for k in range(2)]
    refs = [ref_for(e, pdu, off, flush=True) for e in encs]
    pdu_d = torch.from_numpy(pdu.copy()).cuda()
    off_d = torch.from_numpy(off.view(np.int32).copy()).cuda()
    caps = [e.packet_bound(len(pdu), len(pdus)) for e in encs]
    outs = [torch.zeros(c * 188, dtype=torch.uint8, device="cuda") for c in caps]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k, e in enumerate(encs):
        e.run_device(pdu_d.data_ptr(), len(pdu), off_d.data_ptr(), len(pdus), outs[k].data_ptr(), caps[k], flush=True,
                     stream=streams[k].cuda_stream)
    for k, e in enumerate(encs):
        res = e.result()
        res.ts = outs[k].cpu().numpy()[:res.counters["ts_packets"] * 188]
        same(res, refs[k], "handle %d" % k)


# ---------------------------------------------------------------------------------------- 5. with the chain, the tool
def _pdus_for(nbytes, seed):
    """PDUs (40 .. 1500 bytes) whose datagrams alone are at least nbytes long; some go to multicast groups"""
    rng = np.random.default_rng(seed)
    pdus, total = [], 0
    while total < nbytes:
        L = int(rng.choice([40, 64, 200, 576, 1500]))
        k = len(pdus)
        first = 0x60 if k % 4 == 1 else 0x45
        dst = (C.V6_GROUP if first == 0x60 else C.V4_GROUP) if k % 3 == 0 else None
        pdus.append(C.ip(L, k, first, dst))
        total += L
    return pdus


def test_device_output_straight_into_a_chain(gpu):
    """cfg1q: the encapsulator's device output goes into a Chain's TS input on the same stream, with no synchronise
    between them; the IQ is the Chain's IQ for the reference encapsulator's TS"""
    import torch
    cfg = CONFIGS["cfg1q"]
    n = 3
    need = len(ts_for_frames(cfg, 0, n)[0])
    pdus = _pdus_for(need, 21)
    pdu, off = R.pack(pdus)
    enc = dvbt2ll.MpeFecEncapsulator(pid=C.PID, rows=256, rs_columns=16, mac_from_dest=True, max_pdu_bytes=len(pdu),
                                     max_pdus=len(pdus), max_frames=64)
    ref = ref_for(enc, pdu, off, flush=True)
    assert len(ref.ts) >= need
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    want = ch.run(0, n, ts=ref.ts, ts_base=0)
    cap = enc.packet_bound(len(pdu), len(pdus))
    with torch.cuda.stream(_side_stream()):
        pdu_d = torch.from_numpy(pdu).cuda()
        off_d = torch.from_numpy(off.view(np.int32)).cuda()
        ts_d = torch.zeros(cap * 188, dtype=torch.uint8, device="cuda")
        iq = torch.zeros((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        assert st != 0
        enc.run_device(pdu_d.data_ptr(), len(pdu), off_d.data_ptr(), len(pdus), ts_d.data_ptr(), cap, flush=True,
                       stream=st)
        ch.run_device(ts_d.data_ptr(), 0, len(ref.ts), 0, n, iq.data_ptr(), st)
        torch.cuda.synchronize()
    assert enc.result().counters == ref.counters
    assert np.array_equal(_bits(iq.cpu().numpy()), _bits(want))


TOOL = Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "dvbt2ll" / "dvbt2ll_tx"


def _tool(*args):
    return subprocess.run([str(TOOL)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_mpefec_equals_the_ts_file_input(gpu, tmp_path):
    """dvbt2ll_tx --input mpe-fec on length-prefixed datagrams: the IQ file of the TS-file input run on the reference
    encapsulator's TS, byte for byte (cfg1q, 3 frames in batches of 2); the counters are printed"""
    cfg = CONFIGS["cfg1q"]
    n = 3
    pdus = _pdus_for(len(ts_for_frames(cfg, 0, n)[0]), 22)
    pdus[5] = C.ip(33, 5, 0x50)      # skipped
    pdu, off = R.pack(pdus)
    frames = []
    for extra, kw in ((("--packing", 0, "--rows", 256, "--data-columns", 8, "--rs-columns", 8),
                       dict(packing=0, rows=256, D=8, K=8)),
                      (("--mac-from-dest", "--mac", "0a:0b:0c:0d:0e:0f", "--rows", 512, "--data-columns", 20),
                       dict(mac_mode=1, mac=bytes([10, 11, 12, 13, 14, 15]), rows=512, D=20))):
        ref = R.encap(pdu, off, pid=0x321, flush=True, **kw)
        (tmp_path / "in.ts").write_bytes(ref.ts.tobytes())
        (tmp_path / "in.mpe").write_bytes(b"".join(len(p).to_bytes(2, "big") + p for p in pdus))
        r = _tool("--preset", "cfg1q", "--in", tmp_path / "in.ts", "--out", tmp_path / "a.iq", "--batch", 2,
                  "--frames", n)
        assert r.returncode == 0, r.stderr
        r = _tool("--preset", "cfg1q", "--input", "mpe-fec", "--pid", "0x321", *extra, "--in", tmp_path / "in.mpe",
                  "--out", tmp_path / "b.iq", "--batch", 2, "--frames", n)
        assert r.returncode == 0, r.stderr
        a, b = (tmp_path / "a.iq").read_bytes(), (tmp_path / "b.iq").read_bytes()
        assert len(a) == n * dvbt2ll.Chain(cfg, max_frames=1).iq_per_frame * 8 and a == b
        c = ref.counters
        frames.append(c["frames"])
        assert ("mpe-fec: pdus_in %d, sections %d, fec_sections %d, frames %d, skipped_len %d, skipped_type %d, "
                "mapped_macs %d, ts_packets %d, pusi_packets %d, pad_bytes %d, flushed 1"
                % tuple(c[k] for k in R.COUNTERS[:-1])) in r.stderr
    assert ref.counters["mapped_macs"] > 0 and max(frames) > 1
