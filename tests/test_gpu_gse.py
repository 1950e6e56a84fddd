"""GPU: the GSE encapsulator (dvbt2ll_gse_*, csrc/gse_kernels.hip) against tests/gse_ref.py's sequential restatement:
bytes, counters and resume position, all exact.  Every device run here has its PDUs inside a larger poisoned array
and its output inside a poisoned array with guard regions, at output and PDU-buffer alignments 0 .. 3; the guards and
the bytes past the last frame must stay untouched."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS
import gse_cases as C
import gse_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
TILE = 256              # GSE_TILE of csrc/gse_kernels.h: PDUs per position table
CRC_TRIP = 64 * 4       # GSE_CRC_BLOCKS x 4: fragmented PDUs one trip of the CRC pass covers
COUNT_TRIP = 64 * 256   # GSE_COUNT_BLOCKS x 256: PDUs one trip of the count pass covers


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1)


_STREAM = []


def _side_stream():
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def device_run(enc, pdu, off, types=None, start=(0, 0, 0), cap=None, flush=False, align=(0, 0), stream=None):
    """one run_device with everything inside poisoned arrays; returns the result with bb filled in, after checking
    the guards.  align: (PDU buffer, output) byte alignments.  cap None: room for all the PDUs can become"""
    import torch
    st = _side_stream() if stream is None else stream
    n = len(off) - 1
    cap = enc.frame_bound(len(pdu), n) if cap is None else cap
    with torch.cuda.stream(st):
        buf = torch.full((2 * GUARD + len(pdu) + 16,), POISON, dtype=torch.uint8, device="cuda")
        at = GUARD + align[0]
        if len(pdu):
            buf[at:at + len(pdu)] = torch.from_numpy(np.array(pdu, np.uint8)).cuda()
        off_d = torch.from_numpy(np.array(off, np.uint32).view(np.int32)).cuda()
        typ_d = torch.from_numpy(np.array(types, np.uint16).view(np.int16)).cuda() if types is not None else None
        out = torch.full((2 * GUARD + cap * enc.Lb + 16,), POISON, dtype=torch.uint8, device="cuda")
        a = GUARD + align[1]
        enc.run_device(buf.data_ptr() + at, len(pdu), off_d.data_ptr(), n, out.data_ptr() + a, cap,
                       type_ptr=typ_d.data_ptr() if typ_d is not None else 0, start=start, flush=flush,
                       stream=st.cuda_stream)
    res = enc.result()
    st.synchronize()
    o = out.cpu().numpy()
    nb = res.counters["bbframes"] * enc.Lb
    assert res.counters["bbframes"] <= cap
    assert (o[:a] == POISON).all() and (o[a + nb:] == POISON).all(), "written outside its frames"
    res.bb = o[a:a + nb].copy()
    got = buf.cpu().numpy()
    assert (got[:at] == POISON).all() and (got[at + len(pdu):] == POISON).all()
    return res


def same(res, ref, ctx=""):
    assert tuple(res.resume) == tuple(ref.resume), (ctx, res.resume, ref.resume)
    assert res.counters == ref.counters, (ctx, res.counters, ref.counters)
    np.testing.assert_array_equal(res.bb, ref.bb, err_msg=str(ctx))


def check(enc, pdu, off, ctx, types=None, crc=R.crc32_table, **kw):
    ref = R.encap(pdu, off, types, kbch=enc.kbch, label=enc.label, sis_mis=enc.sis_mis, isi=enc.isi, crc=crc,
                  **{k: v for k, v in kw.items() if k in ("start", "cap", "flush")})
    res = device_run(enc, pdu, off, types, **kw)
    same(res, ref, ctx)
    return res, ref


_ENC = {}


def enc_of(kbch, label, max_pdu_bytes=1 << 21, max_pdus=1 << 11):
    """one handle per mode, shared by the tests (a handle holds scratch only)"""
    key = (kbch, bytes(label), max_pdu_bytes, max_pdus)
    if key not in _ENC:
        _ENC[key] = dvbt2ll.GseEncapsulator(kbch=kbch, label=label, max_pdu_bytes=max_pdu_bytes, max_pdus=max_pdus)
    return _ENC[key]


# ---------------------------------------------------------------------------------------- 1. the placement edges
@pytest.mark.parametrize("kbch", C.KBCHS)
@pytest.mark.parametrize("label", C.LABELS)
def test_placement_edges(gpu, kbch, label):
    enc = enc_of(kbch, label)
    for k, (name, pdus) in enumerate(C.cases(kbch, len(label)).items()):
        pdu, off = R.pack(pdus)
        for flush in (True, False):
            check(enc, pdu, off, (name, flush), flush=flush, align=(k % 4, (k + flush + len(label)) % 4),
                  start=(0, 0, (37 * k) & 255))


# ---------------------------------------------------------------------------------------- 2. tiles, lengths, skips
def _spanning(n, seed, D):
    """n PDUs of 1 .. 40 bytes, with one of 2 D + 50 bytes (at most 1500) on each tile's last slot: it is fragmented
    across the tile boundary whatever the state it meets"""
    pdus = C.mixed(n, seed)
    for t in range(TILE - 1, n, TILE):
        pdus[t] = C.ip(min(2 * D + 50, 1500), t)
    return pdus


def test_three_tiles_and_seven(gpu):
    for j, (kbch, label) in enumerate(((3072, C.LABELS[2]), (7032, C.LABELS[0]))):
        pdus = _spanning(3 * TILE + 7, 11, C.D_of(kbch))
        pdu, off = R.pack(pdus)
        for flush in (False, True):
            _, ref = check(enc_of(kbch, label), pdu, off, (kbch, flush), flush=flush, align=(j + 1, 2 * flush + j))
        assert ref.counters["fragmented"] >= 3


def test_1500_byte_pdus(gpu):
    pdus = [C.ip(1500, k, 0x60 if k % 3 == 0 else 0x45) for k in range(96)] + [C.ip(1499, 7), C.ip(1501, 8)]
    pdu, off = R.pack(pdus)
    check(enc_of(32208, C.LABELS[2]), pdu, off, "1500", flush=True, align=(3, 1))
    check(enc_of(7032, C.LABELS[1]), pdu, off, "1500 short frames", flush=False, align=(2, 3))
    check(enc_of(58192, C.LABELS[0]), pdu, off, "1500 long frames", flush=True, align=(1, 2))


def test_skips_on_tile_edges_and_explicit_types(gpu):
    kbch, label = 7032, C.LABELS[2]
    pdus = _spanning(2 * TILE + 40, 12, C.D_of(kbch))
    for k in (0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 300, len(pdus) - 1):
        pdus[k] = C.ip(20, k, 0x50)              # nibble 5 on a tile's first and last slots
    pdu, off = R.pack(pdus)
    off = off.copy()
    off[TILE + 2] = off[TILE + 1]                # an empty PDU
    off[200] = len(pdu) + 5                      # PDU 199 reaches past the buffer, PDU 200 begins past it
    enc = enc_of(kbch, label)
    res, ref = check(enc, pdu, off, "skips", flush=True, align=(1, 3))
    assert ref.counters["skipped_type"] == 7 and ref.counters["skipped_len"] == 3
    assert R.receive(res.bb, kbch, 6, crc=R.crc32_table) == R.valid_pdus(pdu, off, label=label)
    check(enc, pdu, off, "skips, open end", flush=False, align=(2, 0))
    # explicit types: the nibble is not looked at; inference gives the same bytes where the types say what it infers
    types = (np.arange(len(pdus)) * 7 + 0x0600).astype(np.uint16)
    res, ref = check(enc, pdu, off, "types", types=types, flush=True, align=(0, 1))
    assert ref.counters["skipped_type"] == 0
    good, goff = R.pack(C.mixed(300, 13))
    inferred = np.array([0x86DD if good[o] >> 4 == 6 else 0x0800 for o in goff[:-1]], np.uint16)
    a = device_run(enc, good, goff, None, flush=True, align=(3, 2))
    b = device_run(enc, good, goff, inferred, flush=True, align=(1, 1))
    same(a, b, "inference")


def test_overlapping_valid_pdus_make_more_frames_than_the_buffer_suggests(gpu):
    """off = 0, 2000, 0, 2000, ...: every second PDU is the same 2000 bytes and valid, the ones between are skipped.
    150 of them become about 830 D = 374 frames from a 2000-byte buffer, where PDUs lying side by side could fill
    frame_bound = 15: the emit pass's workgroups take some 55 frames each"""
    kbch, label = 3072, C.LABELS[1]
    pdu = np.frombuffer(C.ip(2000, 30), np.uint8).copy()
    off = np.tile(np.array([0, 2000], np.uint32), 150)
    off = np.append(off, np.uint32(0))
    enc = enc_of(kbch, label)
    ref = R.encap(pdu, off, kbch=kbch, label=label, flush=True, crc=R.crc32_table)
    assert ref.counters["fragmented"] == 150 and ref.counters["skipped_len"] == 150
    assert ref.counters["bbframes"] > 16 * enc.frame_bound(len(pdu), 300)
    res, _ = check(enc, pdu, off, "overlap", cap=1000, flush=True, align=(1, 3))
    assert len(R.receive(res.bb, kbch, 3, crc=R.crc32_table)) == 150
    a, _ = check(enc, pdu, off, "overlap, cut", cap=400, flush=True, align=(2, 1))
    b, _ = check(enc, pdu, off, "overlap, rest", cap=1000, start=a.resume, flush=True, align=(3, 0))
    np.testing.assert_array_equal(np.concatenate([a.bb, b.bb]), ref.bb)
    same(enc.run(pdu, off, cap=5000, flush=True), ref, "host")
    same(enc.run(pdu, off, flush=True), R.encap(pdu, off, kbch=kbch, label=label, flush=True, crc=R.crc32_table,
                                              cap=enc.frame_bound(len(pdu), 300)), "host, default capacity cuts")


# ---------------------------------------------------------------------------------------- 3. cuts and chains
def test_capacity_cut_mid_pdu_and_continuation(gpu):
    kbch, label = 3072, C.LABELS[2]
    pdus = C.mixed(5, 10, 20, 90) + [C.ip(1500, 1)] + C.mixed(30, 14, 1, 300) + [C.ip(900, 5)] + C.mixed(30, 15)
    pdu, off = R.pack(pdus)
    enc = enc_of(kbch, label)
    whole = R.encap(pdu, off, kbch=kbch, label=label, start=(0, 0, 249), flush=True, crc=R.crc32_table)
    n = whole.counters["bbframes"]
    for k, cap in enumerate((0, 1, 2, 3, 4, n // 2, n - 1, n)):
        a, _ = check(enc, pdu, off, ("cut", cap), cap=cap, flush=True, align=(k % 4, (k + 1) % 4), start=(0, 0, 249))
        b, _ = check(enc, pdu, off, ("rest", cap), start=a.resume, flush=True, align=((k + 2) % 4, k % 4))
        np.testing.assert_array_equal(np.concatenate([a.bb, b.bb]), whole.bb)
        assert tuple(b.resume) == whole.resume
    assert any(R.encap(pdu, off, kbch=kbch, label=label, cap=c, flush=True, crc=R.crc32_table).resume[1] > 0
               for c in (1, 2, 3, 4))
    check(enc, pdu, off, "a pdu_byte past the PDU", start=(0, 4000, 1), flush=True)


def test_chunked_calls_at_five_splits(gpu):
    kbch, label = 7032, C.LABELS[0]
    pdus = _spanning(TILE + 90, 16, C.D_of(kbch))
    pdu, off = R.pack(pdus)
    enc = enc_of(kbch, label)
    whole = R.encap(pdu, off, kbch=kbch, label=label, start=(0, 0, 3), flush=True, crc=R.crc32_table)
    for j, k in enumerate((0, 1, 37, TILE, len(pdus))):
        a, _ = check(enc, pdu[:off[k]], off[:k + 1], ("first", k), start=(0, 0, 3), align=(j % 4, (j + 2) % 4))
        b, _ = check(enc, pdu, off, ("second", k), start=a.resume, flush=True, align=((j + 1) % 4, j % 4))
        np.testing.assert_array_equal(np.concatenate([a.bb, b.bb]), whole.bb)
        assert tuple(b.resume) == whole.resume
        for name in R.COUNTERS[:-1]:
            assert a.counters[name] + b.counters[name] == whole.counters[name], (k, name)


def test_flush_forms(gpu):
    kbch, label = 3072, C.LABELS[2]
    enc = enc_of(kbch, label)
    pdu, off = R.pack(C.mixed(9, 6))
    a, _ = check(enc, pdu, off, "open", align=(1, 1))
    f, _ = check(enc, pdu, off, "flushed", flush=True, align=(2, 3))
    assert f.counters["bbframes"] == a.counters["bbframes"] + 1 and f.counters["flushed"] == 1
    pdu, off = R.pack(C.fill(374, 6))                             # u = 0 at the end: the flush adds no frame
    check(enc, pdu, off, "exact", align=(0, 2))
    f, _ = check(enc, pdu, off, "exact, flushed", flush=True, align=(3, 0))
    assert f.counters["flushed"] == 0 and f.counters["bbframes"] == 1
    pdu, off = R.pack(C.fill(374, 6) + C.mixed(3, 13))            # the flush frame does not fit
    check(enc, pdu, off, "no room for the flush frame", cap=1, flush=True, align=(1, 0))
    pdu, off = R.pack(C.mixed(5, 7) + [C.ip(9, 1, 0x50), C.ip(9, 2, 0x10)])   # trailing skipped PDUs
    check(enc, pdu, off, "trailing skips", align=(2, 2))
    check(enc, pdu, off, "trailing skips, flushed", flush=True, align=(0, 3))
    pdu, off = R.pack([C.ip(9, 1, 0x50)] * 3)                     # nothing valid at all
    check(enc, pdu, off, "no packet", flush=True, align=(1, 2))
    check(enc, np.zeros(0, np.uint8), np.zeros(1, np.uint32), "no PDU", flush=True)


def test_run_host_and_mis_header(gpu):
    kbch, label = 7032, C.LABELS[1]
    pdus = _spanning(TILE + 20, 17, C.D_of(kbch))
    pdu, off = R.pack(pdus)
    enc = enc_of(kbch, label)
    kw = dict(kbch=kbch, label=label, crc=R.crc32_table)
    same(enc.run(pdu, off, flush=True), R.encap(pdu, off, flush=True, **kw), "host")
    a = enc.run(pdu, off, cap=5, start=(0, 0, 2))
    same(a, R.encap(pdu, off, cap=5, start=(0, 0, 2), **kw), "cap 5")
    types = np.full(len(pdus), 0x1234, np.uint16)
    same(enc.run(pdu, off, types=types, start=a.resume, flush=True),
         R.encap(pdu, off, types, start=a.resume, flush=True, **kw), "types")
    mis = dvbt2ll.GseEncapsulator(framesize=0, rate=0, sis_mis=0, isi=77, label=label, max_pdu_bytes=len(pdu),
                                  max_pdus=len(pdus))
    assert mis.kbch == 7032
    r = mis.run(pdu, off, flush=True)
    same(r, R.encap(pdu, off, sis_mis=0, isi=77, flush=True, **kw), "MIS")
    assert R.receive(r.bb, kbch, 3, sis_mis=0, isi=77, crc=R.crc32_table) == R.valid_pdus(pdu, off, label=label)


# ---------------------------------------------------------------------------------------- 4. refusals, streams
def test_refusals_launch_nothing(gpu):
    import torch
    for kw in (dict(kbch=7040), dict(kbch=7032, label=b"ab"), dict(kbch=7032, max_pdus=0),
               dict(kbch=7032, max_pdu_bytes=1 << 31), dict(kbch=7032, sis_mis=0, isi=300)):
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.GseEncapsulator(**kw)
    pdu, off = R.pack(C.mixed(50, 18))
    enc = dvbt2ll.GseEncapsulator(kbch=3072, max_pdu_bytes=len(pdu), max_pdus=50)
    before = enc.run(pdu, off, flush=True).counters
    pdu_d = torch.from_numpy(pdu.copy()).cuda()
    off_d = torch.from_numpy(off.view(np.int32).copy()).cuda()
    out = torch.full((64 * 384,), POISON, dtype=torch.uint8, device="cuda")
    P, O, Q = pdu_d.data_ptr(), off_d.data_ptr(), out.data_ptr()
    for args, start in (((P, len(pdu) + 1, O, 50, Q, 8), (0, 0, 0)),      # above max_pdu_bytes
                        ((P, -1, O, 50, Q, 8), (0, 0, 0)),
                        ((P, len(pdu), O, 51, Q, 8), (0, 0, 0)),          # above max_pdus
                        ((P, len(pdu), O, -1, Q, 8), (0, 0, 0)),
                        ((P, len(pdu), O, 50, Q, -1), (0, 0, 0)),         # a negative capacity
                        ((P, len(pdu), O, 50, Q, 8), (-1, 0, 0)),
                        ((P, len(pdu), O, 50, Q, 8), (51, 0, 0)),
                        ((P, len(pdu), O, 50, Q, 8), (0, -1, 0)),
                        ((P, len(pdu), O, 50, Q, 8), (0, 0, 256)),
                        ((P, len(pdu), O, 50, Q, 8), (0, 0, -1)),
                        ((0, len(pdu), O, 50, Q, 8), (0, 0, 0)),          # null pointers
                        ((P, len(pdu), 0, 50, Q, 8), (0, 0, 0)),
                        ((P, len(pdu), O, 50, 0, 8), (0, 0, 0))):
        with pytest.raises(dvbt2ll.DVBT2Error):
            enc.run_device(*args, start=start)
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    assert enc.result().counters == before        # the last real run's result still stands


def test_two_handles_two_streams(gpu):
    import torch
    pdus = _spanning(TILE + 30, 19, 374)
    pdu, off = R.pack(pdus)
    modes = ((3072, C.LABELS[2]), (7032, C.LABELS[0]))
    encs = [dvbt2ll.GseEncapsulator(kbch=k, label=lb, max_pdu_bytes=len(pdu), max_pdus=len(pdus)) for k, lb in modes]
    refs = [R.encap(pdu, off, kbch=k, label=lb, flush=True, crc=R.crc32_table) for k, lb in modes]
    pdu_d = torch.from_numpy(pdu.copy()).cuda()
    off_d = torch.from_numpy(off.view(np.int32).copy()).cuda()
    caps = [e.frame_bound(len(pdu), len(pdus)) for e in encs]
    outs = [torch.zeros(c * e.Lb, dtype=torch.uint8, device="cuda") for c, e in zip(caps, encs)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for k, e in enumerate(encs):
        e.run_device(pdu_d.data_ptr(), len(pdu), off_d.data_ptr(), len(pdus), outs[k].data_ptr(), caps[k], flush=True,
                     stream=streams[k].cuda_stream)
    for k, e in enumerate(encs):
        res = e.result()
        res.bb = outs[k].cpu().numpy()[:res.counters["bbframes"] * e.Lb]
        same(res, refs[k], "handle %d" % k)


# ---------------------------------------------------------------------------------------- 5. past the grid caps
def test_past_the_count_grid(gpu):
    """COUNT_TRIP + TILE + 7 PDUs of 1 .. 6 bytes: the count pass strides, the chain follows 258 tables; a longer PDU
    spans the boundary"""
    n = COUNT_TRIP + TILE + 7
    rng = np.random.default_rng(20)
    lens = rng.integers(1, 7, n)
    lens[COUNT_TRIP - 1] = 1250
    body = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    body[off[:-1]] = np.where(np.arange(n) % 5 == 2, 0x60, 0x45)
    body[off[COUNT_TRIP]] = 0x50                  # a skipped PDU on the trip's first slot
    enc = enc_of(7032, C.LABELS[0], max_pdus=n)
    res, ref = check(enc, body, off, "count", flush=True, align=(3, 3))
    assert ref.counters["complete"] + ref.counters["fragmented"] == n - 1 and ref.counters["skipped_type"] == 1
    check(enc, body, off, "count, cut", cap=ref.counters["bbframes"] - 3, align=(1, 2))


def test_past_one_trip_of_the_crc_pass(gpu):
    """CRC_TRIP + 30 PDUs of 600 bytes in D = 374 frames: every one is fragmented, so the CRC pass's wavefronts take
    a second PDU each"""
    pdus = [C.ip(600, k) for k in range(CRC_TRIP + 30)]
    pdu, off = R.pack(pdus)
    res, ref = check(enc_of(3072, C.LABELS[0]), pdu, off, "crc trips", flush=True, align=(2, 1))
    assert ref.counters["fragmented"] == CRC_TRIP + 30


# ---------------------------------------------------------------------------------------- 6. with the chain, the tool
def _pdus_for(nbytes, seed):
    """PDUs (40 .. 1500 bytes) that fill at least nbytes"""
    rng = np.random.default_rng(seed)
    pdus, total = [], 0
    while total < nbytes + 2000:
        L = int(rng.choice([40, 64, 200, 576, 1500]))
        pdus.append(C.ip(L, len(pdus), 0x60 if len(pdus) % 4 == 1 else 0x45))
        total += L
    return pdus


def test_device_output_straight_into_a_chain(gpu):
    """cfg1q: the encapsulator's device output goes into a Chain's BBFRAME input on the same stream, with no
    synchronise between them; the IQ is the Chain's IQ for the reference encapsulator's BBFRAMEs"""
    import torch
    cfg = CONFIGS["cfg1q"]
    n, F = 3, cfg.fecblocks
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    ch.set_input(dvbt2ll.INPUT_BBFRAME)
    enc = dvbt2ll.GseEncapsulator(chain=ch, label=R.LABEL, max_pdu_bytes=1 << 20, max_pdus=4096)
    assert (enc.kbch, enc.sis_mis) == (7032, 1)
    pdus = _pdus_for(n * F * enc.D, 21)
    pdu, off = R.pack(pdus)
    ref = R.encap(pdu, off, kbch=enc.kbch, label=R.LABEL, cap=n * F, crc=R.crc32_table)
    assert ref.counters["bbframes"] == n * F
    want = ch.run(0, n, ts=ref.bb, ts_base=0)
    with torch.cuda.stream(_side_stream()):
        pdu_d = torch.from_numpy(pdu).cuda()
        off_d = torch.from_numpy(off.view(np.int32)).cuda()
        bb_d = torch.zeros(n * F * enc.Lb, dtype=torch.uint8, device="cuda")
        iq = torch.zeros((n * ch.iq_per_frame, 2), dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        assert st != 0
        enc.run_device(pdu_d.data_ptr(), len(pdu), off_d.data_ptr(), len(pdus), bb_d.data_ptr(), n * F, stream=st)
        ch.run_device(bb_d.data_ptr(), 0, bb_d.numel(), 0, n, iq.data_ptr(), st)
        torch.cuda.synchronize()
    res = enc.result()
    assert res.counters == ref.counters and tuple(res.resume) == ref.resume
    assert np.array_equal(_bits(iq.cpu().numpy()), _bits(want))
    assert ch.bbheader_errors() == 0


TOOL = Path(__file__).resolve().parents[1] / "gr-dvbt2ll_amd" / "dvbt2ll" / "dvbt2ll_tx"


def _tool(*args):
    return subprocess.run([str(TOOL)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_cli_gse_equals_the_bbframe_file_input(gpu, tmp_path):
    """dvbt2ll_tx --input gse on length-prefixed datagrams: the IQ file of the BBFRAME-file input run on the reference
    encapsulator's frames, byte for byte (cfg1q, 3 frames in batches of 2); the counters are printed"""
    cfg = CONFIGS["cfg1q"]
    n = 3
    D = C.D_of(7032)
    pdus = _pdus_for(n * cfg.fecblocks * D, 22)
    pdus[5] = C.ip(33, 5, 0x50)      # skipped
    pdu, off = R.pack(pdus)
    for extra, label in (((), bytes([0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B])), (("--no-label",), b""),
                         (("--label3", "0a:0b:0c"), bytes([10, 11, 12])),
                         (("--label", "0a:0b:0c:0d:0e:0f"), bytes([10, 11, 12, 13, 14, 15]))):
        ref = R.encap(pdu, off, kbch=7032, label=label, flush=True, crc=R.crc32_table)
        (tmp_path / "in.bb").write_bytes(ref.bb.tobytes())
        (tmp_path / "in.gse").write_bytes(b"".join(len(p).to_bytes(2, "big") + p for p in pdus))
        r = _tool("--preset", "cfg1q", "--input", "bbframe", "--in", tmp_path / "in.bb", "--out", tmp_path / "a.iq",
                  "--batch", 2, "--frames", n)
        assert r.returncode == 0, r.stderr
        r = _tool("--preset", "cfg1q", "--input", "gse", *extra, "--in", tmp_path / "in.gse",
                  "--out", tmp_path / "b.iq", "--batch", 2, "--frames", n)
        assert r.returncode == 0, r.stderr
        a, b = (tmp_path / "a.iq").read_bytes(), (tmp_path / "b.iq").read_bytes()
        assert len(a) == n * dvbt2ll.Chain(cfg, max_frames=1).iq_per_frame * 8 and a == b
        c = ref.counters
        assert ("gse: pdus_in %d, complete %d, fragmented %d, gse_packets %d, skipped_len %d, skipped_type %d, "
                "bbframes %d, pad_bytes %d, flushed %d" % tuple(c[k] for k in R.COUNTERS)) in r.stderr


def test_cli_gse_gives_up_where_no_frame_can_complete(gpu, tmp_path):
    """one short datagram, then more zero-length records than a call's table holds: the open frame is held back,
    nothing is consumed and nothing more can be read; the tool says so and ends"""
    (tmp_path / "in.gse").write_bytes(len(C.ip(20)).to_bytes(2, "big") + C.ip(20) + b"\0\0" * 70000)
    r = _tool("--preset", "cfg1q", "--input", "gse", "--in", tmp_path / "in.gse", "--out", tmp_path / "c.iq")
    assert r.returncode == 1 and "no frame completes" in r.stderr
