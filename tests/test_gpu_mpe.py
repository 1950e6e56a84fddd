"""GPU: the MPE encapsulator (dvbt2ll_mpe_*, csrc/mpe_kernels.hip) against tests/mpe_ref.py's sequential restatement:
bytes, counters and resume position, all exact.  Every device run here has its PDUs inside a larger poisoned array
and its output inside a poisoned array with guard regions, at output and PDU-buffer alignments 0 .. 3; the guards and
the bytes past the last packet must stay untouched."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS, ts_for_frames
import mpe_cases as C
import mpe_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 0xA5, 4096
TILE = 512          # MPE_TILE of csrc/mpe_kernels.h: PDUs per tile of the state scan
ROUND = 32 * TILE   # PDUs one compose round covers; the count pass's grid cap is 64 x 256 PDUs, the same number
SCAN_ROUND = 256 * 1024   # PDUs one round of the sum scan's tile pass covers (packing 0)
LANE_MAX = 192      # CRC_LANE_MAX of csrc/mpe_kernels.hip: sections up to here take a lane, longer ones a wavefront


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1)


_STREAM = []


def _side_stream():
    """a torch stream with a handle of its own (torch's default stream has handle 0, which the C ABI reads as "the
    handle's own stream")"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def device_run(enc, pdu, off, start=(0, 0, 0), cap=None, flush=False, align=(0, 0), stream=None):
    """one run_device with everything inside poisoned arrays; returns the result with ts filled in, after checking
    the guards.  align: (PDU buffer, output) byte alignments.  cap None: room for all the PDUs can become"""
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


def check(enc, pdu, off, ctx, crc=R.crc32_table, **kw):
    ref = R.encap(pdu, off, pid=enc.pid, mac=enc.mac, mac_mode=enc.mac_mode, packing=enc.packing, crc=crc,
                  **{k: v for k, v in kw.items() if k in ("start", "cap", "flush")})
    res = device_run(enc, pdu, off, **kw)
    same(res, ref, ctx)
    return res, ref


_ENC = {}


def enc_of(mac_mode, packing, max_pdu_bytes=1 << 20, max_pdus=1 << 12):
    """one handle per mode, shared by the tests (a handle holds scratch only)"""
    key = (mac_mode, packing, max_pdu_bytes, max_pdus)
    if key not in _ENC:
        _ENC[key] = dvbt2ll.MpeEncapsulator(pid=C.PID, mac=R.MAC, mac_from_dest=bool(mac_mode), packing=packing,
                                            max_pdu_bytes=max_pdu_bytes, max_pdus=max_pdus)
    return _ENC[key]


def ref_of(pdu, off, mac_mode=0, packing=1, **kw):
    return R.encap(pdu, off, pid=C.PID, mac_mode=mac_mode, packing=packing, crc=R.crc32_table, **kw)


# ---------------------------------------------------------------------------------------- 1. the packet forms
@pytest.mark.parametrize("packing", [1, 0])
@pytest.mark.parametrize("mac_mode", [0, 1])
def test_r_and_free_byte_cases(gpu, mac_mode, packing):
    enc = enc_of(mac_mode, packing)
    for k, (name, pdus) in enumerate(C.cases().items()):
        pdu, off = R.pack(pdus)
        for flush in (True, False):
            check(enc, pdu, off, (name, flush), flush=flush, align=(k % 4, (k + flush + mac_mode) % 4),
                  start=(0, 0, k & 15))
    pdu, off = R.pack([bytes([0x40 + k]) for k in range(12)])      # eleven sections start in packet 0
    check(enc, pdu, off, "smallest sections", flush=True, align=(1, 2))


# ---------------------------------------------------------------------------------------- 2. tiles, lengths, skips
def _spanning(n, seed):
    """n PDUs of 1 .. 40 bytes, with a 300-byte one on each tile's last slot: its section spans the tile boundary"""
    pdus = C.mixed(n, seed)
    for t in range(TILE - 1, n, TILE):
        pdus[t] = C.ip(300, t)
    return pdus


def _free_after(pdus):
    """the bytes left free in the open packet behind these PDUs' sections (packing 1)"""
    pdu, off = R.pack(pdus)
    return ref_of(pdu, off, flush=True).counters["pad_bytes"] - ref_of(pdu, off).counters["pad_bytes"]


@pytest.mark.parametrize("packing", [1, 0])
def test_three_tiles_and_seven(gpu, packing):
    """a section across every tile boundary; the first tile's last section is stretched until the second tile's first
    header straddles two packets"""
    pdus = _spanning(3 * TILE + 7, 11)
    pdus[TILE - 1] = C.ip(300 + (_free_after(pdus[:TILE]) - 5) % 184, TILE - 1)
    assert 1 <= _free_after(pdus[:TILE]) <= 11
    pdu, off = R.pack(pdus)
    for mac_mode in (0, 1):
        for flush in (False, True):
            check(enc_of(mac_mode, packing), pdu, off, (mac_mode, flush), flush=flush,
                  align=(mac_mode + 1, 2 * flush + mac_mode))


@pytest.mark.parametrize("packing", [1, 0])
def test_long_sections_and_the_crc_threshold(gpu, packing):
    """4080-byte PDUs (a wavefront per CRC), 1500-byte ones, and sections of LANE_MAX - 1, LANE_MAX, LANE_MAX + 1
    bytes: the lane path's last and the wavefront path's first"""
    pdus = [C.ip(4080, k, 0x60 if k % 3 == 0 else 0x45) for k in range(6)]
    pdus += [C.ip(1500, k, 0x60 if k % 3 == 0 else 0x45) for k in range(20)] + [C.ip(1499, 7), C.ip(1501, 8)]
    for k in range(12):
        pdus.append(C.ip(LANE_MAX - C.OVER - 1 + k % 3, 40 + k, 0x60 if k % 2 else 0x45))
    pdu, off = R.pack(pdus)
    check(enc_of(0, packing), pdu, off, "long", flush=True, align=(3, 1))
    check(enc_of(1, packing), pdu, off, "long, mapped", flush=False, align=(2, 3))


@pytest.mark.parametrize("packing", [1, 0])
def test_skips_on_tile_edges(gpu, packing):
    pdus = _spanning(2 * TILE + 40, 12)
    for k in (0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 700, len(pdus) - 1):
        pdus[k] = C.ip(20, k, 0x50)              # nibble 5 on a tile's first and last slots
    pdus[800] = C.ip(4081, 800)                  # one byte too long
    pdu, off = R.pack(pdus)
    off = off.copy()
    off[TILE + 2] = off[TILE + 1]                # an empty PDU
    off[300] = len(pdu) + 5                      # PDU 299 reaches past the buffer, PDU 300 begins past it
    enc = enc_of(1, packing)
    res, ref = check(enc, pdu, off, "skips", flush=True, align=(1, 3))
    assert ref.counters["skipped_type"] == 7 and ref.counters["skipped_len"] == 4
    assert R.receive(res.ts, C.PID, 0, R.crc32_table) == R.valid_pdus(pdu, off, R.MAC, 1)
    check(enc, pdu, off, "skips, open end", flush=False, align=(2, 0))


@pytest.mark.parametrize("packing", [1, 0])
def test_overlapping_valid_pdus_make_more_packets_than_the_buffer_suggests(gpu, packing):
    """off = 0, 2000, 0, 2000, ...: every second PDU is the same 2000 bytes and valid, the ones between are skipped
    (off[i + 1] <= off[i]).  150 of them become about 1650 packets from a 2000-byte buffer, where PDUs lying side by
    side could fill 13 (packet_bound: 39 or 337): the emit pass's workgroups take many groups of 64 packets each and
    the CRC pass's wavefronts several sections each"""
    pdu = np.frombuffer(C.ip(2000, 30), np.uint8).copy()
    off = np.tile(np.array([0, 2000], np.uint32), 150)
    off = np.append(off, np.uint32(0))
    enc = enc_of(0, packing)
    ref = ref_of(pdu, off, 0, packing, flush=True)
    assert ref.counters["sections"] == 150 and ref.counters["skipped_len"] == 150
    assert ref.counters["ts_packets"] > enc.packet_bound(len(pdu), 300) + 16 * 64
    res, _ = check(enc, pdu, off, "overlap", cap=2000, flush=True, align=(1, 3))
    assert len(R.receive(res.ts, C.PID, 0, R.crc32_table)) == 150
    a, _ = check(enc, pdu, off, "overlap, cut", cap=700, flush=True, align=(2, 1))
    b, _ = check(enc, pdu, off, "overlap, rest", cap=2000, start=a.resume, flush=True, align=(3, 0))
    np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), ref.ts)
    # run_host with a capacity far above what its device buffer could be sized to from the buffer's bytes
    same(enc.run(pdu, off, cap=5000, flush=True), ref, "host")
    same(enc.run(pdu, off, flush=True), ref_of(pdu, off, 0, packing, flush=True, cap=enc.packet_bound(len(pdu), 300)),
         "host, default capacity cuts")


# ---------------------------------------------------------------------------------------- 3. cuts and chains
@pytest.mark.parametrize("packing", [1, 0])
def test_capacity_cut_mid_section_and_mid_header_with_continuation(gpu, packing):
    """free_case(2) comes first: its second section's header straddles packets 0 and 1, so a capacity of 1 cuts inside
    the header; r_case(367) behind it is cut inside its datagram"""
    pdus = C.free_case(2) + C.r_case(367) + C.mixed(60, 14) + [C.ip(900, 5)] + C.mixed(30, 15)
    pdu, off = R.pack(pdus)
    enc = enc_of(1, packing)
    whole = ref_of(pdu, off, 1, packing, start=(0, 0, 9), flush=True)
    n = whole.counters["ts_packets"]
    for k, cap in enumerate((0, 1, 2, 3, 4, n // 2, n - 1, n)):
        a, _ = check(enc, pdu, off, ("cut", cap), cap=cap, flush=True, align=(k % 4, (k + 1) % 4), start=(0, 0, 9))
        b, _ = check(enc, pdu, off, ("rest", cap), start=a.resume, flush=True, align=((k + 2) % 4, k % 4))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert tuple(b.resume) == whole.resume
    if packing:
        assert ref_of(pdu, off, 1, 1, cap=1, flush=True).resume[:2] == (1, 2)      # inside the straddling header
    assert any(ref_of(pdu, off, 1, packing, cap=c, flush=True).resume[1] > 12 for c in (2, 3, 4))


@pytest.mark.parametrize("packing", [1, 0])
def test_chunked_calls_at_five_splits(gpu, packing):
    pdus = _spanning(TILE + 90, 16)
    pdu, off = R.pack(pdus)
    enc = enc_of(1, packing)
    whole = ref_of(pdu, off, 1, packing, start=(0, 0, 3), flush=True)
    for j, k in enumerate((0, 1, 37, TILE, len(pdus))):
        a, _ = check(enc, pdu[:off[k]], off[:k + 1], ("first", k), start=(0, 0, 3), align=(j % 4, (j + 2) % 4))
        b, _ = check(enc, pdu, off, ("second", k), start=a.resume, flush=True, align=((j + 1) % 4, j % 4))
        np.testing.assert_array_equal(np.concatenate([a.ts, b.ts]), whole.ts)
        assert tuple(b.resume) == whole.resume
        for name in R.COUNTERS[:-1]:
            assert a.counters[name] + b.counters[name] == whole.counters[name], (k, name)


def test_flush_forms(gpu):
    enc = enc_of(0, 1)
    pdu, off = R.pack(C.mixed(9, 6))
    a, _ = check(enc, pdu, off, "open", align=(1, 1))
    f, _ = check(enc, pdu, off, "flushed", flush=True, align=(2, 3))
    assert f.counters["ts_packets"] == a.counters["ts_packets"] + 1 and f.counters["flushed"] == 1
    pdu, off = R.pack([C.ip(183 - 16, 1)])                     # nothing left: the flush adds no packet
    check(enc, pdu, off, "exact", align=(0, 2))
    check(enc, pdu, off, "exact, flushed", flush=True, align=(3, 0))
    pdu, off = R.pack([C.ip(182 - 16, 1)])                     # one byte free: held back, or one FF
    check(enc, pdu, off, "one free", align=(2, 2))
    r, _ = check(enc, pdu, off, "one free, flushed", flush=True, align=(1, 3))
    assert r.counters["pad_bytes"] == 1
    pdu, off = R.pack([C.ip(183 + 60 - 16, 2)])                # the flush's last packet holds a section's end only
    check(enc, pdu, off, "tail, open", align=(3, 3))
    r, _ = check(enc, pdu, off, "tail", flush=True, align=(1, 0))
    assert r.ts[188 + 1] == 0x01 and r.counters["pusi_packets"] == 1
    pdu, off = R.pack(C.mixed(5, 7) + [C.ip(9, 1, 0x50), C.ip(9, 2, 0x10)])   # trailing skipped PDUs
    check(enc, pdu, off, "trailing skips", align=(2, 2))
    check(enc, pdu, off, "trailing skips, flushed", flush=True, align=(0, 3))
    pdu, off = R.pack([C.ip(9, 1, 0x50)] * 3)                  # nothing valid at all
    check(enc, pdu, off, "no section", flush=True, align=(1, 2))
    check(enc, np.zeros(0, np.uint8), np.zeros(1, np.uint32), "no PDU", flush=True)
    enc0 = enc_of(0, 0)                                        # packing 0: flush changes nothing but flushed
    pdu, off = R.pack(C.mixed(9, 6))
    a, _ = check(enc0, pdu, off, "packing 0, open", align=(1, 0))
    f, _ = check(enc0, pdu, off, "packing 0, flushed", flush=True, align=(0, 1))
    np.testing.assert_array_equal(a.ts, f.ts)


def test_run_host(gpu):
    pdus = _spanning(TILE + 20, 17)
    pdu, off = R.pack(pdus)
    for packing in (1, 0):
        enc = enc_of(1, packing)
        same(enc.run(pdu, off, flush=True), ref_of(pdu, off, 1, packing, flush=True), packing)
        a = enc.run(pdu, off, cap=5, start=(0, 0, 2))
        same(a, ref_of(pdu, off, 1, packing, cap=5, start=(0, 0, 2)), "cap 5")
        same(enc.run(pdu, off, start=a.resume, flush=True), ref_of(pdu, off, 1, packing, start=a.resume, flush=True),
             "rest")


# ---------------------------------------------------------------------------------------- 4. refusals, streams
def test_refusals_launch_nothing(gpu):
    import torch
    for kw in (dict(pid=0x1FFF), dict(pid=-1), dict(packing=2), dict(max_pdus=0), dict(max_pdu_bytes=1 << 31)):
        with pytest.raises(dvbt2ll.DVBT2Error):
            dvbt2ll.MpeEncapsulator(**kw)
    with pytest.raises(ValueError):
        dvbt2ll.MpeEncapsulator(mac=b"\x01\x02")
    pdu, off = R.pack(C.mixed(50, 18))
    enc = dvbt2ll.MpeEncapsulator(pid=C.PID, max_pdu_bytes=len(pdu), max_pdus=50)
    before = enc.run(pdu, off, flush=True).counters
    pdu_d = torch.from_numpy(pdu.copy()).cuda()
    off_d = torch.from_numpy(off.view(np.int32).copy()).cuda()
    out = torch.full((64 * 188,), POISON, dtype=torch.uint8, device="cuda")
    P, O, Q = pdu_d.data_ptr(), off_d.data_ptr(), out.data_ptr()
    for args, start in (((P, len(pdu) + 1, O, 50, Q, 8), (0, 0, 0)),      # above max_pdu_bytes
                        ((P, -1, O, 50, Q, 8), (0, 0, 0)),
                        ((P, len(pdu), O, 51, Q, 8), (0, 0, 0)),          # above max_pdus
                        ((P, len(pdu), O, -1, Q, 8), (0, 0, 0)),
                        ((P, len(pdu), O, 50, Q, -1), (0, 0, 0)),         # a negative capacity
                        ((P, len(pdu), O, 50, Q, 8), (-1, 0, 0)),
                        ((P, len(pdu), O, 50, Q, 8), (51, 0, 0)),
                        ((P, len(pdu), O, 50, Q, 8), (50, 1, 0)),         # section_byte > 0 at n_pdus
                        ((P, len(pdu), O, 50, Q, 8), (0, -1, 0)),
                        ((P, len(pdu), O, 50, Q, 8), (0, 0, 16)),
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
    pdus = _spanning(TILE + 30, 19)
    pdu, off = R.pack(pdus)
    encs = [dvbt2ll.MpeEncapsulator(pid=C.PID + k, mac_from_dest=bool(k), packing=1 - k, max_pdu_bytes=len(pdu),
                                    max_pdus=len(pdus)) for k in range(2)]
    refs = [R.encap(pdu, off, pid=C.PID + k, mac_mode=k, packing=1 - k, flush=True, crc=R.crc32_table) for k in range(2)]
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


# ---------------------------------------------------------------------------------------- 5. past a round
@pytest.mark.parametrize("packing", [1, 0])
def test_past_one_compose_round_and_the_count_grid(gpu, packing):
    """ROUND + TILE + 7 PDUs of 1 .. 6 bytes: the compose pass carries its state into a second round, the count pass
    strides (and, without packing, the sum scan has more than one tile); a longer section spans the round boundary"""
    n = ROUND + TILE + 7
    rng = np.random.default_rng(20)
    lens = rng.integers(1, 7, n)
    lens[ROUND - 1] = 250
    body = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    body[off[:-1]] = np.where(np.arange(n) % 5 == 2, 0x60, 0x45)
    body[off[ROUND]] = 0x50                       # a skipped PDU on the round's first slot
    enc = enc_of(1, packing, max_pdus=n)
    res, ref = check(enc, body, off, "round", flush=True, align=(3, 3))
    assert ref.counters["sections"] == n - 1 and ref.counters["skipped_type"] == 1
    check(enc, body, off, "round, cut", cap=ref.counters["ts_packets"] - 3, align=(1, 2))


def test_past_one_round_of_the_sum_scans_tile_pass(gpu):
    """packing 0, SCAN_ROUND + 1024 + 7 PDUs: the sum scan's single-workgroup pass over the tile sums takes a second
    round.  Nearly all PDUs are empty (skipped), so that the list stays cheap: one in 97 is valid, and so are the ones
    either side of the round boundary"""
    n = SCAN_ROUND + 1024 + 7
    valid = (np.arange(n) % 97 == 5) | (np.abs(np.arange(n) - SCAN_ROUND) <= 3)
    lens = np.where(valid, 30, 0)
    lens[SCAN_ROUND - 1] = 400
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(lens)
    body = np.random.default_rng(23).integers(0, 256, int(off[-1]), dtype=np.uint8)
    body[off[:-1][valid]] = 0x45
    enc = enc_of(0, 0, max_pdus=n)
    res, ref = check(enc, body, off, "scan round", flush=True, align=(2, 1))
    assert ref.counters["sections"] == int(valid.sum()) and ref.counters["skipped_len"] == n - int(valid.sum())
    check(enc, body, off, "scan round, cut", cap=ref.counters["ts_packets"] - 5, align=(1, 0))


# ---------------------------------------------------------------------------------------- 6. with the chain, the tool
def _pdus_for(nbytes, seed):
    """PDUs (40 .. 1500 bytes) whose packed TS is at least nbytes long; some go to multicast groups"""
    rng = np.random.default_rng(seed)
    pdus, total = [], 0
    while total < nbytes + 2000:
        L = int(rng.choice([40, 64, 200, 576, 1500]))
        k = len(pdus)
        first = 0x60 if k % 4 == 1 else 0x45
        dst = (C.V6_GROUP if first == 0x60 else C.V4_GROUP) if k % 3 == 0 else None
        pdus.append(C.ip(L, k, first, dst))
        total += L + 16
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
    ref = ref_of(pdu, off, 1, 1, flush=True)
    assert len(ref.ts) >= need
    ch = dvbt2ll.Chain(cfg, max_frames=n)
    want = ch.run(0, n, ts=ref.ts, ts_base=0)
    enc = dvbt2ll.MpeEncapsulator(pid=C.PID, mac_from_dest=True, max_pdu_bytes=len(pdu), max_pdus=len(pdus))
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


def test_cli_mpe_equals_the_ts_file_input(gpu, tmp_path):
    """dvbt2ll_tx --input mpe on length-prefixed datagrams: the IQ file of the TS-file input run on the reference
    encapsulator's TS, byte for byte (cfg1q, 3 frames in batches of 2), once with --packing 0 and once with
    --mac-from-dest; the counters are printed"""
    cfg = CONFIGS["cfg1q"]
    n = 3
    pdus = _pdus_for(len(ts_for_frames(cfg, 0, n)[0]), 22)
    pdus[5] = C.ip(33, 5, 0x50)      # skipped
    pdu, off = R.pack(pdus)
    for extra, kw in ((("--packing", 0), dict(packing=0)),
                      (("--mac-from-dest", "--mac", "0a:0b:0c:0d:0e:0f"),
                       dict(mac_mode=1, mac=bytes([10, 11, 12, 13, 14, 15])))):
        ref = R.encap(pdu, off, pid=0x321, flush=True, crc=R.crc32_table, **kw)
        (tmp_path / "in.ts").write_bytes(ref.ts.tobytes())
        (tmp_path / "in.mpe").write_bytes(b"".join(len(p).to_bytes(2, "big") + p for p in pdus))
        r = _tool("--preset", "cfg1q", "--in", tmp_path / "in.ts", "--out", tmp_path / "a.iq", "--batch", 2,
                  "--frames", n)
        assert r.returncode == 0, r.stderr
        r = _tool("--preset", "cfg1q", "--input", "mpe", "--pid", "0x321", *extra, "--in", tmp_path / "in.mpe",
                  "--out", tmp_path / "b.iq", "--batch", 2, "--frames", n)
        assert r.returncode == 0, r.stderr
        a, b = (tmp_path / "a.iq").read_bytes(), (tmp_path / "b.iq").read_bytes()
        assert len(a) == n * dvbt2ll.Chain(cfg, max_frames=1).iq_per_frame * 8 and a == b
        c = ref.counters
        assert ("mpe: pdus_in %d, sections %d, skipped_len %d, skipped_type %d, mapped_macs %d, ts_packets %d, "
                "pusi_packets %d, pad_bytes %d, flushed 1" % tuple(c[k] for k in R.COUNTERS[:-1])) in r.stderr
    assert ref.counters["mapped_macs"] > 0
