"""CPU: the inputs of tests/test_gpu_bbch_edges.py do what they claim (tests/bbch_cases.py): the residue sweeps
cover every start phase and the boundary positions, the expected sync-error counts equal the oracle's, the
shifted runs keep every block's phase, and the tight TS spans are the bytes the oracle reads."""
import numpy as np
import pytest

from dvbt2ll.configs import payload_pos, ts_for_frames
import bbch_cases as C
import oracle_lib as O
import plan_probe as PP


def _all_cfgs():
    out = [("sweep-" + n, c) for n, (c, _) in C.SWEEPS.items()]
    out += [("normal-" + n, c) for n, (c, _) in C.NORMAL.items()]
    out += [("offset-" + n, c) for n, c in C.OFFSET_CFGS.items()]
    return out


@pytest.mark.parametrize("name,cfg", _all_cfgs(), ids=[n for n, _ in _all_cfgs()])
def test_frame_carries_the_blocks(name, cfg):
    """the chain refuses a frame that cannot carry fecblocks; the planner builds these"""
    plan = PP.frame_plan(cfg.fm_args())
    assert plan is not None
    assert plan["F"] == cfg.fecblocks and plan["S"] == cfg.fecblocks * plan["cs"]


@pytest.mark.parametrize("name", list(C.SWEEPS))
def test_block_geom_is_the_oracles_state(name):
    """block_geom's count0 and payload length are what the oracle's running state gives: SYNCD of every BBHEADER
    (bits 56..71 before BB scrambling) and the bytes each block consumes"""
    cfg, nframes = C.SWEEPS[name]
    nb = nframes * cfg.fecblocks
    ts, base = ts_for_frames(cfg, 0, nframes)
    bb = O.BB(*cfg.bb_args())
    prbs = np.zeros(80, np.uint8)
    O.lib().orc_bb_prbs(O._p(prbs), 80)
    off = 0
    for B in range(nb):
        g = C.block_geom(cfg, B)
        cursor = 0 if B == 0 else payload_pos(g["J0"] - 1, C.is_hem(cfg)) + 1   # first stream byte not yet consumed
        assert off == cursor, B
        bits, cons = bb.work(ts[off:], 1)
        hdr = bits[:80] ^ prbs
        syncd = int(np.packbits(hdr[56:72]).view(">u2")[0])
        dfl = int(np.packbits(hdr[32:48]).view(">u2")[0])
        assert syncd == (0 if g["count0"] == 0 else 8 * (188 - g["count0"])), B
        assert dfl == 8 * g["npay"], B
        off += cons
    assert off == payload_pos(C.block_geom(cfg, nb)["J0"] - 1, C.is_hem(cfg)) + 1


@pytest.mark.parametrize("name", list(C.SWEEPS))
def test_sweep_covers_every_phase(name):
    cfg, nframes = C.SWEEPS[name]
    m = C.packet_period(cfg)
    nb = nframes * cfg.fecblocks
    assert nb > 128, "a second (partly dead) tile of 128 rows"
    geo = [C.block_geom(cfg, B) for B in range(nb)]
    if C.is_hem(cfg):
        assert {g["J0"] % 187 for g in geo} == set(range(187))
    else:
        assert {g["count0"] for g in geo} == set(range(188))
    # a block whose last payload byte is immediately followed by a sync byte
    assert any((g["J0"] + g["npay"]) % m == 0 for g in geo)
    # a block whose first payload byte is a sync slot (SYNCD = 0), other than the stream's first
    assert any(g["count0"] == 0 for g in geo[1:])
    # a sync position in each of BBFRAME bytes 10 .. 15 (the header piece), with and without the in-band field
    # at the other end of the frame's first block
    offs = {C.first_sync_offset(cfg, B) for B in range(nb)}
    assert set(range(6)) <= offs
    # ... and at both ends of a 16-byte piece, and on the hand-off between two pieces (bytes 15 / 16 of a piece:
    # BBFRAME byte 10 + o with (10 + o) % 16 in {0, 15})
    every = set()
    for B, g in enumerate(geo):
        o = C.first_sync_offset(cfg, B)
        while o < g["npay"]:
            every.add((10 + o) % 16)
            o += m
    assert every == set(range(16))
    # the last payload byte itself a sync position (the `< npay` cuts)
    assert any((g["J0"] + g["npay"] - 1) % m == 0 for g in geo)
    if C.has_inband(cfg):
        first = [g for B, g in enumerate(geo) if B % cfg.fecblocks == 0]
        assert all(g["padding"] == 104 and g["npay"] == C.pay_full(cfg) - 13 for g in first)
        # a sync position within the last 16 payload bytes before the in-band field (the piece both write)
        assert any((g["J0"] + g["npay"] - 1) % m >= m - 16 or (g["J0"] + g["npay"] - 1) % m == 0 for g in first)


def _count_cases():
    out = [("sweep-" + n, c, f) for n, (c, f) in C.SWEEPS.items()]
    return out + [("normal-" + n, c, f) for n, (c, f) in C.NORMAL.items()]


@pytest.mark.parametrize("name,cfg,nframes", _count_cases(), ids=[c[0] for c in _count_cases()])
def test_sync_count_closed_form_is_the_oracles(name, cfg, nframes):
    """every sync byte of the stream corrupted: the oracle counts the closed form (whole run and each segment of
    the split run), and its output bits are the clean stream's"""
    want = C.sync_count(cfg, 0, nframes)
    assert want > 0
    assert C.oracle_sync_errors(cfg, 0, nframes) == want
    np.testing.assert_array_equal(C.oracle_bits(cfg, 0, nframes, True), C.oracle_bits(cfg, 0, nframes, False))
    # clean stream: no warnings
    ts, _ = ts_for_frames(cfg, 0, nframes)
    bb = O.BB(*cfg.bb_args())
    bb.work(ts, nframes * cfg.fecblocks)
    assert bb.sync_errors() == 0
    a, b = (C.SPLIT[0], C.SPLIT[0] + C.SPLIT[1]) if nframes > sum(C.SPLIT) else (1, 1)
    segs = [(0, a), (a, b - a), (b, nframes - b)]
    total = 0
    for f0, n in segs:
        if n == 0:
            continue
        assert C.oracle_sync_errors(cfg, f0, n) == C.sync_count(cfg, f0, n), (f0, n)
        total += C.sync_count(cfg, f0, n)
    assert total == want
    # the consumed range is not the buffer, which starts a packet early: a later segment's buffer holds more
    # corrupted sync bytes than its frames consume
    f0, n = segs[-1]
    ts, base = ts_for_frames(cfg, f0, n)
    assert base > 0 and len(ts) % 188 == 0
    assert len(ts) // 188 > C.sync_count(cfg, f0, n)


def test_normal_frame_slices_split_mid_bbframe():
    """64800-bit case: the kernel cuts the BBFRAME's 32-byte chunks into BCH_KS = 2 K slices; the cut lies inside
    the payload, away from its ends"""
    for cfg, _ in C.NORMAL.values():
        L = C.pay_full(cfg) + 10
        nq = (L + 31) // 32
        cut = 32 * (nq // 2)
        assert 10 + 188 < cut < L - 188


@pytest.mark.parametrize("mode,bname", C.OFFSET_CASES, ids=["%s-%s" % c for c in C.OFFSET_CASES])
def test_shifted_run_preconditions(mode, bname):
    cfg, boundary, n = C.OFFSET_CFGS[mode], C.BOUNDARIES[bname], C.OFFSET_FRAMES
    K = C.large_frame(cfg, boundary)
    k, D, ts, base = C.shifted_run(cfg, K)
    F, m = cfg.fecblocks, C.packet_period(cfg)
    assert D > 0 and D % 188 == 0 and base % 188 == 0
    assert K % cfg.t2frames == k % cfg.t2frames                       # FRAME_IDX
    assert k < C.repeat_frames(cfg) <= 374
    for b in range(n * F):
        small, large = C.block_geom(cfg, k * F + b), C.block_geom(cfg, K * F + b)
        assert small["count0"] == large["count0"]
        assert small["J0"] % m == large["J0"] % m
        assert (small["npay"], small["padding"]) == (large["npay"], large["padding"])   # in-band phase
        assert large["pos0"] - small["pos0"] == D                                       # a whole number of packets
    # the declared buffer is the span the API demands for frames [K, K + n), or wider
    lo, end = C.ts_span(cfg, K, n)
    assert base <= lo and base + len(ts) >= end
    lo_k, end_k = C.ts_span(cfg, k, n)
    assert (lo - lo_k, end - end_k) == (D, D) or lo_k == 0
    first, last = C.consumed_range(cfg, K, n)
    if boundary < 1 << 40:
        assert first < boundary < last                                # strictly inside the run
        assert C.consumed_range(cfg, K, 1)[0] < boundary              # frame K starts below it
        assert C.consumed_range(cfg, K + 1, 1)[0] > boundary          # frame K + 1 lies above it
    else:
        assert first > boundary
    if boundary >= 1 << 32:
        # a wrong multiplier for the high word in mod188 (2^32 = 136 mod 188) would cancel if it were 0 mod 188
        assert (last >> 32) % 188 != 0
        assert any((C.block_geom(cfg, K * F + b)["pos0"] >> 32) % 188 != 0 for b in range(n * F))
    else:
        assert last >> 32 == 0 and last >= 1 << 31                    # needs the 32nd bit, unsigned


def test_offset_cases_cover_what_the_issue_lists():
    modes = {m for m, _ in C.OFFSET_CASES}
    assert modes == set(C.OFFSET_CFGS) and {b for _, b in C.OFFSET_CASES} == set(C.BOUNDARIES)
    assert any(C.has_inband(C.OFFSET_CFGS[m]) for m in modes)
    assert sorted(C.is_hem(C.OFFSET_CFGS[m]) for m, _ in C.IQ_OFFSET_CASES) == [False, True]
    assert C.GRAPH_OFFSET_CASE in C.OFFSET_CASES and all(c in C.OFFSET_CASES for c in C.IQ_OFFSET_CASES)


@pytest.mark.parametrize("mode", list(C.TIGHT_CASES))
def test_tight_span_is_what_the_frames_read(mode):
    """ts_span restated: from the packet before the first one touched through the last consumed byte (+1 in HEM);
    the slice holds exactly those bytes of the stream"""
    (cfg, f0), n = C.TIGHT_CASES[mode], C.TIGHT_FRAMES
    lo, end = C.ts_span(cfg, f0, n)
    first, last = C.consumed_range(cfg, f0, n)
    hem = C.is_hem(cfg)
    touched = first - 1 if hem and first % 188 == 1 else first   # HEM: the sync byte dropped before payload byte 0
    assert lo == (touched // 188) * 188 - 188 and lo > 0
    # HEM: through the byte in front of the next payload byte (the next packet's sync byte when the run ends on a
    # packet boundary)
    assert end == (payload_pos((f0 + n) * C.frame_payload(cfg), True) if hem else last + 1)
    assert last + 1 <= end <= last + 2
    ts, base = ts_for_frames(cfg, f0, n)
    assert base <= lo and base + len(ts) >= end
    cut = C.stream_slice(lo, end)
    assert len(cut) == end - lo
    np.testing.assert_array_equal(cut, ts[lo - base:end - base])
    # High end: the kernel fetches 17 bytes from window offset rel for every 16-byte piece of a BBFRAME (piece
    # P0 = BBFRAME bytes [P0, P0 + 16) holds payload bytes from P0 - 10) and takes its bytewise edge path where
    # rel + 17 > len.  The last block's last piece does.
    F = cfg.fecblocks
    g = C.block_geom(cfg, (f0 + n) * F - 1)
    P0 = 16 * ((g["npay"] + 10 - 1) // 16)
    rel = payload_pos(g["J0"] + P0 - 10, hem) - lo
    assert 0 <= rel < end - lo < rel + 17
    # Low end: the window starts one whole packet before the first one touched, so no payload piece starts
    # before it.  Only the NM CRC prologue, which starts 6 chunks (192 bytes) before a block's first piece at
    # stream position pos0 - 10 - 192 (+ 16 for the odd lanes), can: it does in the low-edge case alone.
    g0 = C.block_geom(cfg, f0 * F)
    before = not hem and g0["pos0"] - 10 - 192 - lo < 0
    assert before == (mode == "nm-low-edge")
    assert not before or -16 <= g0["pos0"] - 10 - 192 - lo
