"""Multi-PLP frames at the edges the configs of dvbt2ll.configs do not reach (DESIGN 5.10 "Tests"): 4-8 PLPs
per T2 frame, constellation tables shared between PLPs, per-symbol PLP runs shorter than one aligned load of
the OFDM kernels' slot scatter, and a PLP absent between two present ones.  Importable without a GPU:
test_cpu_mplp_cases.py proves on the CPU what each case claims, test_gpu_mplp_many.py runs them.

Short FECFRAMEs (16200 bits: 8100 / 4050 / 2700 / 2025 cells) keep the oracle cheap."""
import itertools

import numpy as np

from dvbt2ll import enums as E
from dvbt2ll.configs import CONFIGS, mplp_from, _plp

QPSK, Q16, Q64, Q256 = E.MOD_QPSK, E.MOD_16QAM, E.MOD_64QAM, E.MOD_256QAM
SHORT_CELLS = {QPSK: 8100, Q16: 4050, Q64: 2700, Q256: 2025}
OFDM_MAX_QAM = 1024   # t2_kernels.h: LDS entries of the OFDM kernels' constellation tables


def short(cfg, constellation, rotation, fecblocks, **kw):
    """a short-FECFRAME rate-1/2 PLP (one TI block unless told otherwise) on cfg's frame"""
    kw.setdefault("tiblocks", 1)
    kw.setdefault("rate", E.C1_2)
    return _plp(cfg, framesize=E.FECFRAME_SHORT, constellation=constellation, rotation=rotation,
                fecblocks=fecblocks, **kw)


def _cases():
    c1, c3, c4 = CONFIGS["cfg1"], CONFIGS["cfg3"], CONFIGS["cfg4"]
    c16 = c4.with_(fftsize=E.FFTSIZE_16K, numdatasyms=7)
    return {
        # every (constellation, rotation) pair once: 2 (4 + 16 + 64 + 256) = 680 table entries, K_sig = 1309
        "many8_8k_all": mplp_from(c4, "many8-8k-all-pairs", [
            short(c4, Q256, 1, 2),
            short(c4, QPSK, 0, 1, tiblocks=0),
            short(c4, Q64, 1, 3, tiblocks=2, rate=E.C3_5),
            short(c4, Q16, 0, 2, inputmode=E.INPUTMODE_HIEFF),
            short(c4, Q256, 0, 3, tiblocks=3, rate=E.C2_3),
            short(c4, QPSK, 1, 1, inband=E.INBAND_ON, tsrate=3333333),
            short(c4, Q64, 0, 1, rate=E.C4_5),
            short(c4, Q16, 1, 3, tiblocks=2, rate=E.C1_3)]),
        # pairs repeating non-adjacently: 256r, 16, 256r, QPSK, 16, 64, 256r, 64r -> bases 0, 256, 0, 272, 256,
        # 276, 0, 340 (per PLP without sharing: 0, 256, 272, 528, 532, 548, 612, 868)
        "many8_8k_shared": mplp_from(c4, "many8-8k-shared-tables", [
            short(c4, Q256, 1, 1),
            short(c4, Q16, 0, 2, tiblocks=2),
            short(c4, Q256, 1, 3, rate=E.C3_4, inputmode=E.INPUTMODE_HIEFF),
            short(c4, QPSK, 0, 1, tiblocks=0),
            short(c4, Q16, 0, 1, rate=E.C2_3, inband=E.INBAND_ON, tsrate=2500000),
            short(c4, Q64, 0, 2),
            short(c4, Q256, 1, 2, rate=E.C4_5, tiblocks=2),
            short(c4, Q64, 1, 1)]),
        # 32K extended (the split kernel): six PLPs, 64r / 16 / 64r / 256 / 16 / 64r, v1.3.1 scrambled 16-QAM L1
        "many6_32k_shared": mplp_from(c3, "many6-32kext-shared-tables", [
            short(c3, Q64, 1, 3, tiblocks=2),
            short(c3, Q16, 0, 2),
            short(c3, Q64, 1, 1, rate=E.C3_5, inputmode=E.INPUTMODE_HIEFF),
            short(c3, Q256, 0, 4, tiblocks=0),
            short(c3, Q16, 0, 3, rate=E.C2_3, inband=E.INBAND_ON, tsrate=6000000),
            short(c3, Q64, 1, 5)]).with_(version=E.VERSION_131, l1scrambled=E.L1_SCRAMBLED_ON,
                                         l1constellation=E.L1_MOD_16QAM, numdatasyms=7),
        # the GRC's 4K frame: a Type-1 256-QAM rotated PLP and two Type-2 PLPs in 3 sub-slices
        "tiny_4k_quad": mplp_from(c1, "tiny-4k-quad", [
            short(c1, Q256, 1, 1),
            short(c1, Q16, 0, 1, plp_type=2),
            short(c1, Q256, 1, 1, plp_type=2)]).with_(num_subslices=3),
        # the same three PLPs (2, 2, 1 blocks) on a 16K frame of 3 data symbols: search_short_run(c16, 4)'s first hit
        "tiny_16k_sq16": mplp_from(c16, "tiny-16k-quad", [
            short(c16, Q256, 1, 2),
            short(c16, Q16, 0, 2, plp_type=2),
            short(c16, Q256, 1, 1, plp_type=2)]).with_(num_subslices=3, numdatasyms=3),
        # cfg3's 32K extended PP4 frame cut to 3 data symbols, 2 / 3 / 3 blocks: search_short_run(cfg3, 8)'s first hit
        "tiny_32k_octet": mplp_from(c3, "tiny-32kext-octet", [
            short(c3, Q256, 1, 2),
            short(c3, Q16, 0, 3, plp_type=2),
            short(c3, Q256, 1, 3, plp_type=2)]).with_(num_subslices=3, numdatasyms=3),
        # 8K: PLP 1 (Type 1) and PLP 3 (Type 2) only in the odd T2 frames; in the even ones PLP 1 is absent
        # between PLPs 0 and 2, PLP 3 between 2 and 4
        "skip_8k": mplp_from(c4, "skip-8k-interval2", [
            short(c4, Q16, 0, 2),
            short(c4, Q256, 1, 2, frame_interval=2, first_frame_idx=1),
            short(c4, Q64, 0, 1, plp_type=2),
            short(c4, Q16, 0, 1, plp_type=2, frame_interval=2, first_frame_idx=1),
            short(c4, Q64, 1, 2, plp_type=2)]).with_(num_subslices=5, numdatasyms=11),
    }


CASES = _cases()
MANY = ["many8_8k_all", "many8_8k_shared", "many6_32k_shared"]
SHARED = ["many8_8k_shared", "many6_32k_shared"]
TINY = {"tiny_4k_quad": 4, "tiny_16k_sq16": 4, "tiny_32k_octet": 8}   # case -> slots per aligned load
# the short run each tiny case exists for: (frame class, group 2 j + h, PLP, first slot, slots)
SHORT_RUN = {"tiny_4k_quad": (0, 2, 2, 3375, 1), "tiny_16k_sq16": (0, 0, 2, 6750, 2),
             "tiny_32k_octet": (0, 3, 1, 21243, 4)}
# skip_8k: (frame class, group, PLP) of an empty run between two non-empty ones
SKIPPED_RUN = (0, 4, 1)


def _tiny_miso():
    """a MISO preamble changes the frame's cell counts, so the MISO variant of tiny_4k_quad has no short run
    (its shortest run: 375 slots).  The same search over MISO frames (search_space on the 16K frame with a MISO
    preamble and misogroup MISO_TX2_PROCESSED, pieces of at most 3 cells in a symbol) gives this one: four
    PLPs, PP4, 3 data symbols"""
    from dvbt2ll.configs import MISO_TX2_PROCESSED
    c16 = CONFIGS["cfg4"].with_(fftsize=E.FFTSIZE_16K)
    return mplp_from(c16, "tiny-16k-quad-miso", [
        short(c16, Q256, 1, 1),
        short(c16, Q16, 0, 1, plp_type=2),
        short(c16, Q256, 1, 2, plp_type=2),
        short(c16, QPSK, 0, 2, plp_type=2)]).with_(num_subslices=3, numdatasyms=3, pilotpattern=E.PILOT_PP4,
                                                  preamble=E.PREAMBLE_T2_MISO, misogroup=MISO_TX2_PROCESSED)


TINY_MISO = _tiny_miso()
SHORT_RUN_MISO = (0, 4, 1, 19574, 1)


# ---------------------------------------------------------------- constellation table bases
def table_bases(m, share=True):
    """the base of each PLP's constellation table among the OFDM kernels' LDS tables and the entries in all:
    the first PLP with a (constellation, rotation) pair owns a table of 2^bits entries, later ones reuse it
    (share=False: a table per PLP, the cumulative sum)"""
    bases, owner, n = [], {}, 0
    for p in m.plps:
        key = (p.constellation, p.rotation)
        if share and key in owner:
            bases.append(owner[key])
            continue
        owner[key] = n
        bases.append(n)
        n += 4 << (2 * p.constellation)
    return bases, n


# ---------------------------------------------------------------- per-group PLP runs
def class_tables(m, cls=0):
    """the chain's tables of frame class cls (t2probe_chain_cls: bnd, d0, n, n0, part, inv, gather_d, ...)"""
    import miso_ref as MR
    return MR.chain_tables(m, cls)


def group_runs(t):
    """every (symbol, half) group's PLP runs of one class's tables: (group, [(start, length) per PLP])"""
    P = t["nplp"]
    for g in range(2 * t["Nsym"]):
        if not t["split"] and g & 1:
            continue
        b = t["bnd"][g]
        yield g, [(int(b[k]), int(b[k + 1] - b[k])) for k in range(P)]


def is_short_run(start, length, align):
    """a run that begins off the alignment and ends inside the same aligned load: both edges of one load
    are masked (scatter_slots: one quad / octet, lastq / lasto = 0)"""
    return 0 < length < align and start % align != 0 and start // align == (start + length - 1) // align


def short_runs(m, align):
    """(class, group, PLP, start, length) of every short run of every frame class"""
    t0 = class_tables(m, 0)
    if t0 is None:
        return []
    out = []
    for cls in range(t0["ncls"]):
        t = t0 if cls == 0 else class_tables(m, cls)
        for g, runs in group_runs(t):
            out += [(cls, g, k, a, n) for k, (a, n) in enumerate(runs) if is_short_run(a, n, align)]
    return out


def min_run(m):
    """the shortest non-empty run of any class"""
    t0 = class_tables(m, 0)
    best = None
    for cls in range(t0["ncls"]):
        t = t0 if cls == 0 else class_tables(m, cls)
        for g, runs in group_runs(t):
            for k, (a, n) in enumerate(runs):
                if n > 0 and (best is None or n < best[4]):
                    best = (cls, g, k, a, n)
    return best


def skipped_runs(m):
    """(class, group, PLP) of every empty run with a non-empty run of a lower and of a higher PLP in its group"""
    t0 = class_tables(m, 0)
    out = []
    for cls in range(t0["ncls"]):
        t = t0 if cls == 0 else class_tables(m, cls)
        for g, runs in group_runs(t):
            ln = [n for _, n in runs]
            out += [(cls, g, k) for k in range(1, len(ln) - 1) if ln[k] == 0 and any(ln[:k]) and any(ln[k + 1:])]
    return out


# ---------------------------------------------------------------- the search for short runs
def symbol_capacities(m):
    """data cells each symbol of m's frame can carry, in frame order (the P2 symbols less their share of the
    L1 signalling, the data symbols, the frame closing symbol), from the planner's cell counts and L1-post size"""
    import plan_probe as PP
    c = PP.cell_counts(m.fftsize, m.carriermode, m.pilotpattern, m.paprmode, m.guardinterval, m.preamble)
    if c is None:
        return None
    try:
        _, info = PP.l1post_mplp(m, 0)
    except AssertionError:
        return None
    l1 = 1840 + info["Lp"]
    nd = m.numdatasyms - (1 if c["N_FC"] else 0)
    return [c["C_P2"] - l1 // c["N_P2"]] * c["N_P2"] + [c["C_DATA"]] * nd + ([c["C_FC"]] if c["N_FC"] else [])


def smallest_overlap(m, caps):
    """the fewest cells (> 0) any PLP piece (a Type-1 PLP, a Type-2 sub-slice) of class 0 shares with a symbol:
    arithmetic on PLP_START / SUB_SLICE_INTERVAL, no planner call.  None: the sub-slices do not divide"""
    edges = np.concatenate([[0], np.cumsum(caps)])
    cells = [p.fecblocks * SHORT_CELLS[p.constellation] * (4 if p.framesize else 1) for p in m.plps]
    pieces, pos = [], 0
    for p, n in zip(m.plps, cells):
        if p.plp_type == 1:
            pieces.append((pos, pos + n))
            pos += n
    t2 = [n for p, n in zip(m.plps, cells) if p.plp_type == 2]
    if any(n % m.num_subslices for n in t2):
        return None
    for _ in range(m.num_subslices):
        for n in t2:
            pieces.append((pos, pos + n // m.num_subslices))
            pos += n // m.num_subslices
    if pos > edges[-1]:
        return None
    best = None
    for a, b in pieces:
        ja, jb = np.searchsorted(edges, a, "right") - 1, np.searchsorted(edges, b, "left") - 1
        for n in (min(b, edges[ja + 1]) - a, b - max(a, edges[jb])):
            if n > 0 and (best is None or n < best):
                best = int(n)
    return best


def search_space(base, align):
    """the candidate frames of the short-run search on base's FFT size: 3 or 4 short-FECFRAME PLPs (PLP 0 Type-1
    256-QAM rotated, then 16-QAM, 256-QAM rotated and QPSK PLPs of either type), 1-3 FEC blocks each, 1-81
    sub-slices, every L1 constellation, pilot patterns PP2 / PP4 / PP7 (those base's guard interval allows),
    both carrier modes, 3 / 4 / 7 data symbols"""
    tail = [(Q16, 0), (Q256, 1), (QPSK, 0)]
    pilots = [base.pilotpattern] + [p for p in (E.PILOT_PP2, E.PILOT_PP4, E.PILOT_PP7) if p != base.pilotpattern]
    for nplp, l1c, pp, cm, nds in itertools.product((3, 4), (E.L1_MOD_64QAM, E.L1_MOD_16QAM, E.L1_MOD_QPSK,
                                                             E.L1_MOD_BPSK), pilots,
                                                    (base.carriermode, 1 - base.carriermode), (3, 4, 7)):
        for types in itertools.product((2, 1), repeat=nplp - 1):
            if 2 not in types:
                continue
            for blocks in itertools.product((1, 2, 3), repeat=nplp):
                plps = [short(base, Q256, 1, blocks[0])]
                plps += [short(base, tail[k][0], tail[k][1], blocks[k + 1], plp_type=types[k])
                         for k in range(nplp - 1)]
                m = mplp_from(base, "search", plps).with_(l1constellation=l1c, pilotpattern=pp, carriermode=cm,
                                                          numdatasyms=nds)
                for nss in range(1, 82):
                    yield m.with_(num_subslices=nss)


def search_short_run(base, align, limit=1, max_overlap=None):
    """walk search_space(base, align) for frames with a short run (is_short_run) in some group.  The planner is
    asked only about frames in which some PLP piece shares at most max_overlap (default 2 align - 2: a split
    symbol halves it) cells with a symbol.  Returns (hits [(config, short_runs)], candidates walked, planner
    calls, the shortest run met (length, config))"""
    max_overlap = max_overlap or 2 * align - 2
    hits, walked, asked, shortest, caps_of = [], 0, 0, None, {}
    for m in search_space(base, align):
        walked += 1
        key = (m.nplp, m.l1constellation, m.pilotpattern, m.carriermode, m.numdatasyms)
        if key not in caps_of:
            caps_of[key] = symbol_capacities(m.with_(num_subslices=1, plps=tuple(
                short(base, Q256, 1, 1) for _ in m.plps)))
        caps = caps_of[key]
        if caps is None:
            continue
        n = smallest_overlap(m, caps)
        if n is None or n > max_overlap or class_tables(m, 0) is None:
            continue
        asked += 1
        best = min_run(m)
        if shortest is None or best[4] < shortest[0]:
            shortest = (best[4], m)
        runs = short_runs(m, align)
        if runs:
            hits.append((m, runs))
            if len(hits) >= limit:
                break
    return hits, walked, asked, shortest
