"""Fast references and stream builders for the sizes at which the device-wide scans of csrc/modeadapt_kernels.hip
and csrc/t2mi_kernels.hip take a second and a third round (tests/test_gpu_large_runs.py).  Plain numpy, proven
against the sequential references at small sizes by tests/test_cpu_large_ref.py.

  * adapt_fast: modeadapt_ref.adapt's contract, vectorised over packets and BBFRAMEs;
  * big_ts: the mode adapter's stream, laid out around the scan's tile size (`scale`) and round (256 tiles);
  * big_t2mi: a T2-MI stream with everything a call must return worked out from what was put in, not by parsing.

A scan round is ROUND_TILES tiles: the one workgroup of *_scan_tiles takes 256 tile sums per trip of its loop and
carries the running total to the next trip.  R = ROUND_TILES * scale is the first element of the second round."""
import numpy as np

import modeadapt_ref as MR
import t2mi_ref as TR

ROUND_TILES = 256
PID_A, PID_B, PID_FOREIGN, PID_NULL = 0x100, 0x101, 0x200, 0x1FFF
SELECTED_PIDS = (PID_A, PID_B)


def _ro(a):
    a.setflags(write=False)
    return a


# ================================================================================================ mode adapter
def _crc8_table():
    t = np.zeros(256, np.uint8)
    for v in range(256):
        c = v
        for _ in range(8):
            c = ((c << 1) ^ 0xD5) & 0xFF if c & 0x80 else (c << 1) & 0xFF
        t[v] = c
    return t


CRC8 = _crc8_table()


def classify_ts(rows, npd=1, mask=None, forced=False):
    """per packet of rows (n, 188): selected, transmitted, and per transmitted packet its index and DNP (the first
    one's DNP is the caller's when forced)"""
    m = len(rows)
    pid = ((rows[:, 1].astype(np.int64) & 0x1F) << 8) | rows[:, 2]
    if npd:
        sel = pid != PID_NULL
        if mask is not None:
            mk = np.asarray(mask, np.uint8)
            sel &= ((mk[pid >> 3] >> (pid & 7).astype(np.uint8)) & 1).astype(bool)
    else:
        sel = np.ones(m, bool)
    anchor = sel.copy()
    if forced and m:
        anchor[0] = True
    idx = np.arange(m)
    last = np.maximum.accumulate(np.where(anchor, idx, -1)) if m else idx
    tx = anchor | (((idx - last - 1) & 255) == 255)     # a null at position 255 mod 256 of its run is kept
    t = np.flatnonzero(tx)
    dnp = np.diff(t, prepend=-1) - 1                    # everything between two transmitted packets was deleted
    return sel, tx, t, dnp


def adapt_fast(ts, kbch, npd=1, mask=None, sis=True, isi=0, start=(0, 0, 0), cap=None, flush=False):
    """modeadapt_ref.adapt, vectorised: the same arguments, the same Result"""
    allrows = np.asarray(ts, np.uint8).reshape(-1, 188)
    n = len(allrows)
    s0, ub0, dnp0 = (int(x) for x in start)
    rows = allrows[s0:]
    m = len(rows)
    D, L, U = (kbch - 80) // 8, kbch // 8, 188 if npd else 187
    forced = m > 0 and (ub0 > 0 or dnp0 > 0)
    sel, tx, t, dnp = classify_ts(rows, npd, mask, forced)
    nu = len(t)
    if forced:
        dnp[0] = dnp0
    units = np.empty((nu, U), np.uint8)
    units[:, :187] = rows[t, 1:]
    units[~sel[t], :187] = MR.NULL_PACKET[1:]
    if npd:
        units[:, 187] = dnp
    skip = ub0 if nu else 0
    fifo = units.reshape(-1)[skip:]
    total = len(fifo)
    whole, rem = divmod(total, D)
    cap = whole + 1 if cap is None else int(cap)
    flushed = bool(flush) and whole + (1 if rem else 0) <= cap
    nfr = min(whole, cap)
    emitted = total if flushed else nfr * D
    tail = 1 if flushed and rem else 0
    nf = nfr + tail
    out = np.zeros((nf, L), np.uint8)
    out[:nfr, 10:] = fifo[:nfr * D].reshape(nfr, D)
    if tail:
        out[nfr, 10:10 + rem] = fifo[nfr * D:]
    # headers: SYNCD is the distance to the first unit that begins in the data field
    k = np.arange(nf, dtype=np.int64)
    nbytes = np.where(k < nfr, D, rem)
    u1 = -(-(k * D + skip) // U)
    x = u1 * U - skip
    syncd = np.where((u1 < nu) & (x < k * D + nbytes), 8 * (x - k * D), 0xFFFF)
    tmpl = MR.header(8 * D, 0, 0, npd, sis, isi)
    H = np.zeros((nf, 10), np.uint8)
    H[:, 0], H[:, 1] = tmpl[0], tmpl[1]
    H[:, 4], H[:, 5] = (8 * nbytes) >> 8, (8 * nbytes) & 255
    H[:, 7], H[:, 8] = syncd >> 8, syncd & 255
    c = np.zeros(nf, np.uint8)
    for q in range(9):
        c = CRC8[c ^ H[:, q]]
    H[:, 9] = c ^ 1
    out[:, :10] = H
    # resume: the unit holding the first byte not emitted
    if flushed:
        resume = (n, 0, 0)
    else:
        u = (emitted + skip) // U
        if u < nu:
            resume = (s0 + int(t[u]), int(emitted - (u * U - skip)), int(dnp[u]))
        else:
            resume = (s0 + int(t[-1]) + 1 if nu else s0, 0, 0)
    iend = resume[0] - s0
    last_tx = int(t[-1]) if nu else -1
    txe, sele = tx[:iend], sel[:iend]
    idle = ~txe
    dropped = idle & (np.arange(iend) > last_tx) if flushed else np.zeros(iend, bool)
    cnt = dict(packets_in=iend, selected=int((txe & sele).sum()), nulls_deleted=int((idle & ~dropped).sum()),
               nulls_kept=int((txe & ~sele).sum()), nulls_dropped_at_flush=int(dropped.sum()),
               sync_errors=int((rows[:iend, 0] != 0x47).sum()), bbframes=nf, flushed=int(flushed and rem > 0))
    return MR.Result(out.reshape(-1), resume, cnt)


def big_ts(scale, round_tiles=ROUND_TILES, seed=21):
    """-> (ts, marks): 2R + scale + 7 packets, R = round_tiles * scale, selected under the mask of SELECTED_PIDS.
      run 1   [b1, e1): nulls and foreign PIDs from 256 q + 255 packets before R to scale + 40 past it, q periods of
              256 with 256 q >= 2 scale: whole tiles without a selected packet on both sides of R, kept nulls at
              b1 + 255 + 256 j, one of them exactly packet R.  b1 = 1 mod 256, so a scan that lost its carry (last
              selected = none) keeps other nulls
      run 2   [b2, 2R + scale): the same before 2R with a kept null exactly on packet 2R, then the whole tile after
      tail    three selected packets (the middle one with a bad sync byte), four trailing nulls
      body    selected PIDs A and B, one packet in two hundred a null or a foreign PID
      bad sync bytes on packets 5, R + 1, 2R (a kept null), 2R + 3 (a deleted one) and 2R + scale + 1
    A kept null on R - 1 as well cannot be: R - 1 and R would lie in one run, whose kept nulls are 256 apart; and
    a run that begins on a multiple of 256 keeps the same nulls whether or not the scan's carry arrives."""
    R = round_tiles * scale
    n = 2 * R + scale + 7
    q = max(2, -(-2 * scale // 256))
    b1, e1 = R - 255 - 256 * q, R + scale + 40
    b2, e2 = 2 * R - 255 - 256 * q, 2 * R + scale
    assert 0 < b1 and e1 < b2, "the round is too short for two runs"
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, (n, 188), dtype=np.uint8)
    pids = rng.choice(np.array([PID_A, PID_A, PID_A, PID_B]), n)
    odd = rng.random(n) < 0.005
    pids[odd] = rng.choice(np.array([PID_NULL, PID_FOREIGN]), int(odd.sum()))
    for b, e in ((b1, e1), (b2, e2)):
        pids[b:e] = rng.choice(np.array([PID_NULL, PID_FOREIGN]), e - b)
        pids[b - 1] = PID_A                    # the run begins where it is said to
    pids[e1] = PID_B
    pids[e2:e2 + 3] = (PID_A, PID_B, PID_A)
    pids[e2 + 3:] = PID_NULL
    rows[:, 0] = 0x47
    rows[:, 1] = (rows[:, 1] & 0xE0) | (pids >> 8)
    rows[:, 2] = pids & 255
    bad = [5, R + 1, 2 * R, 2 * R + 3, 2 * R + scale + 1]
    rows[bad, 0] = (0x46, 0x00, 0xFF, 0x48, 0x46)
    marks = dict(R=R, n=n, run1=(b1, e1), run2=(b2, e2), bad_sync=bad, pids=SELECTED_PIDS)
    return _ro(rows.reshape(-1)), marks


def scan_dropping_carry(x, at, op=np.add):
    """-> (the exclusive scan of x, the same with what the rounds before element `at` carried lost: elements from
    `at` on scanned as if the sequence began there)"""
    x = np.asarray(x)
    zero = np.zeros(1, x.dtype)
    true = np.concatenate([zero, op.accumulate(x)[:-1]])
    y = x.copy()
    y[:at] = 0
    lost = np.concatenate([zero, op.accumulate(y)[:-1]])
    return true, lost


# ================================================================================================ T2-MI
T2_PID = 0x1234
PLP_A, PLP_B, PLP_UNLISTED = (3, 6051), (9, 879), 77       # (plp_id, L): normal 3/4 (odd L), short 1/2
PLPS = [PLP_A, PLP_B]
BURST = 20                    # timestamp packets per frame, back to back: 21 bytes each, eight or nine starts in a
                              # TS packet
PAYLOAD = 183                 # stream bytes in every contributing TS packet but the last


def _crc32_table():
    c = np.arange(256, dtype=np.uint32) << np.uint32(24)
    for _ in range(8):
        c = (c << np.uint32(1)) ^ np.where(c >> np.uint32(31), np.uint32(TR.POLY), np.uint32(0))
    return c


CRC32 = _crc32_table()


def crc32_rows(m):
    """CRC-32/MPEG-2 of every row of m (rows of equal length): one table lookup per byte position on the whole
    column"""
    cols = np.ascontiguousarray(np.asarray(m, np.uint8).T)
    crc = np.full(cols.shape[1], 0xFFFFFFFF, np.uint32)
    for col in cols:
        crc = (crc << np.uint32(8)) ^ CRC32[(crc >> np.uint32(24)) ^ col]
    return crc


def _put_crc(F, lo, hi):
    """columns hi - 4 .. hi of F: the CRC of columns lo .. hi - 4, big-endian"""
    crc = crc32_rows(F[:, lo:hi - 4])
    for q in range(4):
        F[:, hi - 4 + q] = (crc >> np.uint32(24 - 8 * q)) & np.uint32(255)


class Expected:
    """what the deframer must return for the stream of big_t2mi, by construction.  call(j0, max_packets, caps) is
    one call that starts at T2-MI packet j0 (0, or where an earlier call's resume position points)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def start(self, j0):
        return (188 * int(self.ts_index[j0]), int(self.within[j0])) if j0 else (0, 0)

    def call(self, j0=0, max_packets=None, caps=None):
        NP = self.npackets
        j1 = NP if max_packets is None else min(NP, j0 + int(max_packets))
        r0 = [int(g[j0]) for g in self.rank]
        for o, cap in enumerate(caps or []):
            hit = np.flatnonzero((self.table["out_index"][j0:j1] == o) & (self.rank[o][j0:j1] - r0[o] >= cap))
            if hit.size:
                j1 = min(j1, j0 + int(hit[0]))
        res = TR.Result()
        tab = self.table[j0:j1].copy()
        for o in range(len(self.plps)):
            tab["block"][tab["out_index"] == o] -= r0[o]
        res.packets = tab
        res.blocks = [int(g[j1]) - r for g, r in zip(self.rank, r0)]
        res.bbframes = [self.outputs[o][r0[o] * L:(r0[o] + res.blocks[o]) * L] for o, (_, L) in enumerate(self.plps)]
        res.by_type = {int(t): int(c) for t, c in enumerate(np.bincount(tab["packet_type"].astype(np.int64), minlength=1)) if c}
        i0 = int(self.ts_index[j0]) if j0 else 0
        if j1 < NP:
            iend = int(self.ts_index[j1])
            res.resume = (188 * iend, int(self.within[j1]))
        else:
            iend = self.nts
            res.resume = (188 * self.nts, 0)
        cnt = dict.fromkeys(TR.TS_COUNTERS + TR.PKT_COUNTERS, 0)
        per_class = np.bincount(self.ts_class[i0:iend], minlength=7)
        for c, name in enumerate(TR.TS_COUNTERS[:7]):
            cnt[name] = int(per_class[c])
        what = self.what[j0:j1]
        cnt["crc_errors"], cnt["len_errors"] = int((what == 1).sum()), int((what == 3).sum())
        cnt["other_plp"] = int((what == 4).sum())
        cnt["accepted"] = int(((tab["flags"] & TR.F_ACCEPTED) != 0).sum())
        res.counters = cnt
        return res


def big_t2mi(scale, round_tiles=ROUND_TILES, seed=5):
    """-> (ts, Expected).  R = round_tiles * scale.  Frames of BURST timestamp packets, one BBFRAME packet of PLP A
    and two of PLP B, as many as give more than R T2-MI packets and more than 2R contributing TS packets, then eight
    more: of those, frame -6 has a flipped bit in A's BBFRAME (CRC error), frame -5 carries an unlisted PLP_ID in
    A's place, frame -4 a PLP A packet of PLP B's length in B's second place (length error) -- all past T2-MI packet
    R and TS packet 2R, with good blocks of both PLPs after them.
    Every contributing TS packet carries PAYLOAD stream bytes (AFC 01 with a pointer_field where a T2-MI packet
    starts in it, an empty adaptation field otherwise; the last one is stuffed); a foreign, a null and an
    adaptation-field-only packet stand before contributing packet 5 and three times shortly before TS packets R and
    2R, so the compact index differs from the TS index from there on."""
    R = round_tiles * scale
    (idA, LA), (idB, LB) = PLPS
    TA, TB = LA + 13, LB + 13
    FB, PPF = 21 * BURST + TA + 2 * TB, BURST + 3
    nfr = max(-(-(R + 1) // PPF), -(-(2 * R + 1) * PAYLOAD // FB)) + 8
    f_crc, f_plp, f_len = nfr - 6, nfr - 5, nfr - 4
    rng = np.random.default_rng(seed)
    f = np.arange(nfr, dtype=np.int64)
    F = np.zeros((nfr, FB), np.uint8)
    sf = (((f >> 1) & 15) << 4).astype(np.uint8)

    def head(col, ptype, slot, bits):
        F[:, col], F[:, col + 1], F[:, col + 2], F[:, col + 3] = ptype, (f * PPF + slot) & 255, sf, 0
        F[:, col + 4], F[:, col + 5] = bits >> 8, bits & 255

    for i in range(BURST):
        col = 21 * i
        head(col, 0x20, i, 88)
        for q in range(4):
            F[:, col + 13 + q] = (f >> (24 - 8 * q)) & 255        # an 11-byte big-endian value: the frame number
        _put_crc(F, col, col + 21)
    a0 = 21 * BURST
    b0 = (a0 + TA, a0 + TA + TB)
    dataA = rng.integers(0, 256, (nfr, LA), dtype=np.uint8)
    dataB = rng.integers(0, 256, (nfr, 2, LB), dtype=np.uint8)
    plpA = np.full(nfr, idA)
    plpA[f_plp] = PLP_UNLISTED
    head(a0, 0, BURST, 24 + 8 * LA)
    F[:, a0 + 6], F[:, a0 + 7], F[:, a0 + 8] = f & 255, plpA, 0x80
    F[:, a0 + 9:a0 + 9 + LA] = dataA
    _put_crc(F, a0, a0 + TA)
    F[f_crc, a0 + 9 + 1000] ^= 0x10
    plpB = np.full((nfr, 2), idB)
    plpB[f_len, 1] = idA
    for v in range(2):
        head(b0[v], 0, BURST + 1 + v, 24 + 8 * LB)
        F[:, b0[v] + 6], F[:, b0[v] + 7], F[:, b0[v] + 8] = f & 255, plpB[:, v], 0x80 if v == 0 else 0
        F[:, b0[v] + 9:b0[v] + 9 + LB] = dataB[:, v]
        _put_crc(F, b0[v], b0[v] + TB)
    stream = F.reshape(-1)
    S = len(stream)

    # ---- the packet table, per frame and slot, then flat
    def slots(ts, a, b1_, b2_):
        m = np.empty((nfr, PPF), np.int64)
        m[:, :BURST], m[:, BURST], m[:, BURST + 1], m[:, BURST + 2] = ts, a, b1_, b2_
        return m

    okA = (plpA == idA) & (f != f_crc)
    okB = plpB == idB
    T = slots(21, TA, TB, TB).reshape(-1)
    NP = len(T)
    s = np.cumsum(T) - T
    out = slots(-1, np.where(okA, 0, -1), np.where(okB[:, 0], 1, -1), np.where(okB[:, 1], 1, -1)).reshape(-1)
    flags = slots(15, np.where(f == f_crc, 3, 15), 15, 15).reshape(-1)
    what = slots(0, np.where(f == f_crc, 1, np.where(f == f_plp, 4, 0)), 0, np.where(f == f_len, 3, 0)).reshape(-1)
    kp = s // PAYLOAD                                         # the contributing TS packet a T2-MI packet starts in
    full, cl = divmod(S, PAYLOAD)
    nc = full + (1 if cl else 0)
    ins = np.array([5, R - 40, R - 30, R - 20, 2 * R - 60, 2 * R - 45, 2 * R - 30])   # a triple before each
    k = np.arange(nc, dtype=np.int64)
    tsidx = k + 3 * np.searchsorted(ins, k, side="right")
    nts = nc + 3 * len(ins)
    clen = np.full(nc, PAYLOAD)
    if cl:
        clen[-1] = cl
    table = np.zeros(NP, TR.REC)
    table["ts_index"] = tsidx[kp]
    table["ts_byte"] = 188 * tsidx[kp] + 188 - clen[kp] + (s - PAYLOAD * kp)
    table["packet_type"] = slots(0x20, 0, 0, 0).reshape(-1)
    table["packet_count"] = np.arange(NP) & 255
    table["superframe_idx"] = np.repeat((f >> 1) & 15, PPF)
    table["payload_len"] = slots(88, 24 + 8 * LA, 24 + 8 * LB, 24 + 8 * LB).reshape(-1)
    table["flags"] = flags
    table["intl_frame_start"] = slots(0, 1, 1, 0).reshape(-1)
    table["frame_idx"] = slots(0, f & 255, f & 255, f & 255).reshape(-1)
    table["plp_id"] = slots(0, plpA, plpB[:, 0], plpB[:, 1]).reshape(-1)
    table["out_index"] = out
    rank = [np.concatenate([[0], np.cumsum(out == o)]) for o in range(2)]
    table["block"] = np.where(out == 0, rank[0][:-1], np.where(out == 1, rank[1][:-1], -1))
    within = np.arange(NP) - np.searchsorted(kp, kp, side="left")

    # ---- the TS
    rows = np.full((nts, 188), 0xFF, np.uint8)
    first = np.searchsorted(s, PAYLOAD * k, side="left")
    sfirst = s[np.minimum(first, NP - 1)]
    pusi = (first < NP) & (sfirst < PAYLOAD * k + clen)
    ptr = np.where(pusi, sfirst - PAYLOAD * k, 0)
    rows[tsidx, 0] = 0x47
    rows[tsidx, 1] = (pusi.astype(np.int64) << 6) | (T2_PID >> 8)
    rows[tsidx, 2] = T2_PID & 255
    rows[tsidx, 3] = (np.where(pusi, 1, 3) << 4) | (k & 15)
    rows[tsidx, 4] = ptr                                     # the pointer_field, or an adaptation field of length 0
    rows[tsidx[:full], 5:] = stream[:full * PAYLOAD].reshape(full, PAYLOAD)
    if cl:
        last = rows[tsidx[-1]]
        a = (182 if pusi[-1] else 183) - cl
        last[3] = 0x30 | ((nc - 1) & 15)
        last[4:] = 0xFF
        last[4] = a
        if a:
            last[5] = 0
        if pusi[-1]:
            last[187 - cl] = ptr[-1]
        last[188 - cl:] = stream[full * PAYLOAD:]
    ts_class = np.zeros(nts, np.int64)
    for mth, kk in enumerate(ins):
        at = int(kk) + 3 * mth
        rows[at, :4], rows[at, 4:] = (0x47, PID_A >> 8, PID_A & 255, 0x10 | (mth & 15)), 0
        rows[at + 1, :4] = (0x47, 0x1F, 0xFF, 0x10)
        rows[at + 2, :6] = (0x47, T2_PID >> 8, T2_PID & 255, 0x20 | ((int(kk) - 1) & 15), 183, 0)
        ts_class[at:at + 3] = (1, 2, 6)
    outputs = [_ro(dataA[okA].reshape(-1)), _ro(dataB[okB].reshape(-1))]
    exp = Expected(plps=PLPS, npackets=NP, nts=nts, ncontributing=nc, table=table, rank=rank, what=what,
                   within=within, ts_index=table["ts_index"].astype(np.int64), ts_class=ts_class, outputs=outputs,
                   R=R, starts_per_contributing=np.bincount(kp, minlength=nc), payload_len=clen, tsidx=tsidx,
                   malformed=dict(crc=f_crc * PPF + BURST, other_plp=f_plp * PPF + BURST,
                                  length=f_len * PPF + BURST + 2))
    return _ro(rows.reshape(-1)), exp
