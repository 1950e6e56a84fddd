"""The MISO pair chain's planner tables for the tests: group 2's layout over group 1's slot order and the 32K cross
lists (gr-dvbt2ll_amd/csrc/t2_plan_probe.cpp t2probe_pair_cls), and their host application in the OFDM kernel's
order."""
import ctypes

import numpy as np

import miso_ref as MR
import plan_probe as PP


def pair_tables(cfg, cls=0):
    """what group 2's OFDM launch of a pair handle reads for the frames of class cls: the keys of
    miso_ref.chain_tables, plus skip (S: the slot is cross-listed, not streamed), xent (entries: slot, bin within
    its half, selector, PLP), xgrp (groups 2 j + h: offset, count), xmax (the longest list), xbound (the planner's
    bound) and xcap (the entries the kernel takes per list).  cfg's misogroup is ignored.  None: refused."""
    m = MR.as_mplp(cfg)
    L = PP.lib()
    L.t2probe_pair_cls.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 19
    p = PP._p
    a = np.array(m.mplp_array(), np.int32)
    g = np.array([0, m.equalization, m.bandwidth], np.int32)
    sz = np.zeros(20, np.int32)
    if L.t2probe_pair_cls(p(a), p(g), cls, p(sz), *([None] * 18)):
        return None
    Nsym, N, S, split, P, ncls, nd, ni, ng, aux_len, l1_lo, Lp, miso, M, unit, nx, xmax, xbound, xcap = (
        int(x) for x in sz[:19])
    t = dict(cmap=np.zeros(Nsym * N, np.int32), inv=np.zeros(max(S, 1), np.uint16), d0=np.zeros(Nsym, np.int32),
             n=np.zeros(Nsym, np.int32), n0=np.zeros(Nsym, np.int32), part=np.zeros(max(S, 1), np.int32),
             bnd=np.zeros(2 * Nsym * (P + 1), np.int32), csel=np.zeros(Nsym * N, np.uint8),
             dbin=np.zeros(max(nd, 1), np.uint16), dval=np.zeros(max(nd, 1), np.complex64),
             ind=np.zeros(max(ni, 1), np.uint32), grp=np.zeros(4 * ng, np.int32), zrun=np.zeros(2 * ng, np.int32),
             gather_d=np.zeros(M, np.int32), aux=np.zeros(aux_len, np.complex64), skip=np.zeros(max(S, 1), np.uint8),
             xent=np.zeros(4 * max(nx, 1), np.int32), xgrp=np.zeros(4 * Nsym, np.int32))
    order = ["cmap", "inv", "d0", "n", "n0", "part", "bnd", "csel", "dbin", "dval", "ind", "grp", "zrun", "gather_d",
             "aux", "skip", "xent", "xgrp"]
    assert L.t2probe_pair_cls(p(a), p(g), cls, p(sz), *[p(t[k]) for k in order]) == 0
    t.update(Nsym=Nsym, N=N, S=S, split=split, nplp=P, ncls=ncls, nd=nd, ni=ni, l1_lo=l1_lo, Lp=Lp, miso=miso, M=M,
             unit=unit, xmax=xmax, xbound=xbound, xcap=xcap)
    for k in ("inv", "part", "skip"):
        t[k] = t[k][:S]
    t["dbin"], t["dval"], t["ind"] = t["dbin"][:nd], t["dval"][:nd], t["ind"][:ni]
    t["cmap"], t["csel"] = t["cmap"].reshape(Nsym, N), t["csel"].reshape(Nsym, N)
    t["grp"], t["zrun"], t["bnd"] = t["grp"].reshape(ng, 4), t["zrun"].reshape(ng, 2), t["bnd"].reshape(2 * Nsym, P + 1)
    t["xent"], t["xgrp"] = t["xent"].reshape(-1, 4)[:nx], t["xgrp"].reshape(2 * Nsym, 2)
    return t


def group1_slots(t1, mapped):
    """the pair buffer's cells in group 1's slot order: frame data index d of mapped cell m (gather_d[m] = d) at
    slot part[d] of the TX1 layout t1 (miso_ref.chain_tables of the MISO_TX1 configuration)"""
    gd = t1["gather_d"]
    slots = np.zeros(max(t1["S"], 1), np.complex64)
    isd = gd >= 0
    slots[t1["part"][gd[isd]]] = mapped[isd]
    return slots


def pair_scatter_carriers(t, slots, l1cells, isinc=None):
    """group 2's fill of every symbol as the OFDM kernel does it over group 1's slots, per stored half: the zero
    run, the direct entries, the indirect L1-post entries, the half's slot stream with the cross-listed slots
    skipped, then the half's cross list.  Checks that every bin is written exactly once (or lies in the zero run),
    that no slot is both streamed and cross-listed and that every slot is used once.  Returns (Nsym x N carriers
    in pilotgen's order, after EQ; the cross lists' lengths per (symbol, half))."""
    N, Nsym, split = t["N"], t["Nsym"], t["split"]
    nsub = N // 2 if split else N
    out = np.zeros((Nsym, N), np.complex64)
    k = np.arange(N)
    used = np.zeros(max(t["S"], 1), np.int32)
    lens = np.zeros((Nsym, 2), np.int32)
    for j in range(Nsym):
        row = np.zeros(N, np.complex64)
        hits = np.zeros(N, np.int32)
        s0, n, n0 = int(t["d0"][j]), int(t["n"][j]), int(t["n0"][j])
        for h in range(2 if split else 1):
            base = h * nsub
            z0, z1 = t["zrun"][2 * j + h]
            hits[base + z0:base + z1] += 1
            d0, dn, i0, ni = t["grp"][2 * j + h]
            b = t["dbin"][d0:d0 + dn].astype(np.int64)
            real = b != 0xFFFF
            row[base + b[real]] = t["dval"][d0:d0 + dn][real]
            np.add.at(hits, base + b[real], 1)
            e = t["ind"][i0:i0 + ni].astype(np.int64)
            row[base + (e & 0x7FFF)] = MR.flip(l1cells[((e >> 15) & 0xFFFF) - 1], e >> 31)
            np.add.at(hits, base + (e & 0x7FFF), 1)
            # the half's own stream (not split: the whole run)
            a0, a1 = (s0, s0 + n) if not split else ((s0, s0 + n0) if h == 0 else (s0 + n0, s0 + n))
            s = np.arange(a0, a1)
            s = s[t["skip"][s] == 0]
            inv = t["inv"][s].astype(np.int64)
            bins = inv & 0x7FFF
            assert ((bins >= base) & (bins < base + nsub)).all(), "symbol %d half %d: a streamed bin of the other half" % (j, h)
            row[bins] = MR.flip(slots[s], inv >> 15)
            np.add.at(hits, bins, 1)
            np.add.at(used, s, 1)
            # the half's cross list
            x0, xn = t["xgrp"][2 * j + h]
            lens[j, h] = xn
            x = t["xent"][x0:x0 + xn].astype(np.int64)
            assert (t["skip"][x[:, 0]] == 1).all()
            assert ((x[:, 0] >= s0) & (x[:, 0] < s0 + n)).all() and (x[:, 1] < nsub).all()
            row[base + x[:, 1]] = MR.flip(slots[x[:, 0]], x[:, 2])
            np.add.at(hits, base + x[:, 1], 1)
            np.add.at(used, x[:, 0], 1)
        assert (hits == 1).all(), "symbol %d: a bin written %d times" % (j, hits[hits != 1][0])
        nat = PP.stored_to_natural(row, N, split)
        car = np.empty(N, np.complex64)
        car[(k + N // 2) % N] = nat
        if isinc is not None:
            car = (car.view(np.float32).reshape(-1, 2) * isinc[:, None]).view(np.complex64).reshape(-1)
        out[j] = car
    assert (used[:t["S"]] == 1).all(), "a slot streamed and cross-listed, or never used"
    return out, lens
