"""MISO processing of transmitter group 2 (EN 302 755 clause 9.1) for the tests: the rule in numpy, the
expected carriers built from the unmodified oracle, and the planner's processed tables applied on the host in
the OFDM kernels' order (gr-dvbt2ll_amd/csrc/t2_plan_probe.cpp t2probe_chain_cls).

The rule: with a_p, p < n, the payload cells of an OFDM symbol in the order the frequency interleaver hands
them to the pilot stage (C_P2 cells of a P2 symbol, C_DATA of a data symbol, N_FC of the frame closing
symbol; n even), group 2 sends e_2i = -conj(a_2i+1) and e_2i+1 = conj(a_2i).  On bits: an even position
takes its partner with the real part's sign bit flipped, an odd position with the imaginary part's, signed
zeros included.  PARITY UNPINNED: the reference has no MISO processing block."""
import ctypes

import numpy as np

from dvbt2ll import enums as E
from dvbt2ll.configs import MISO_TX2_PROCESSED, MplpConfig, mplp_from, _plp
import oracle_lib as O
import plan_probe as PP

SIGN = np.uint32(0x80000000)


def miso_pairs(cells):
    """9.1 on one symbol's payload cells (an even count), on bit patterns"""
    a = np.ascontiguousarray(cells, np.complex64).view(np.uint32).reshape(-1, 2, 2)   # [pair][position][re, im]
    e = np.empty_like(a)
    e[:, 0, 0] = a[:, 1, 0] ^ SIGN   # e_2i = -conj(a_2i+1) = (-x, y)
    e[:, 0, 1] = a[:, 1, 1]
    e[:, 1, 0] = a[:, 0, 0]          # e_2i+1 = conj(a_2i) = (x, -y)
    e[:, 1, 1] = a[:, 0, 1] ^ SIGN
    return e.reshape(-1).view(np.complex64)


def symbol_counts(cfg):
    """payload cells of every symbol of the frame (P2 symbols, data symbols, the frame closing symbol)"""
    c = PP.cell_counts(cfg.fftsize, cfg.carriermode, cfg.pilotpattern, cfg.paprmode, cfg.guardinterval, cfg.preamble)
    assert c is not None
    nd = cfg.numdatasyms - (1 if c["N_FC"] else 0)
    return [c["C_P2"]] * c["N_P2"] + [c["C_DATA"]] * nd + ([c["N_FC"]] if c["N_FC"] else [])


def miso_frame(mapped, cfg):
    """group 2's payload cells of one T2 frame from the frame mapper's output (carrier order)"""
    out, o = [], 0
    for n in symbol_counts(cfg):
        assert n % 2 == 0
        out.append(miso_pairs(mapped[o:o + n]))
        o += n
    assert o == len(mapped)
    return np.concatenate(out)


def tx2_args(cfg):
    """the oracle's pilotgen arguments of a processed configuration: group 2's pilots (MISO_TX2)"""
    a = list(cfg.pg_args())
    assert a[8] == MISO_TX2_PROCESSED
    a[8] = E.MISO_TX2
    return tuple(a)


def expected_carriers(mapped, cfg, pg=None):
    """the carriers of a processed frame: the oracle's pilot stage (group 2) over the 9.1-coded cells"""
    pg = pg or O.PG(*tx2_args(cfg))
    return pg.carriers(miso_frame(mapped, cfg))


def as_mplp(cfg):
    """a T2Config as a one-PLP MplpConfig (the same frame through the multi-PLP entry points)"""
    return cfg if isinstance(cfg, MplpConfig) else mplp_from(cfg, cfg.name, [_plp(cfg)])


# ---------------------------------------------------------------- the planner's tables of one frame class
def chain_tables(cfg, cls=0):
    """what the OFDM kernels' scatter mode reads for the frames of class cls (t2probe_chain_cls)"""
    m = as_mplp(cfg)
    L = PP.lib()
    L.t2probe_chain_cls.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 16
    p = PP._p
    a = np.array(m.mplp_array(), np.int32)
    g = np.array([m.misogroup, m.equalization, m.bandwidth], np.int32)
    sz = np.zeros(16, np.int32)
    r = L.t2probe_chain_cls(p(a), p(g), cls, p(sz), *([None] * 15))
    if r:
        return None
    Nsym, N, S, split, P, ncls, nd, ni, ng, aux_len, l1_lo, Lp, miso, M, unit = (int(x) for x in sz[:15])
    t = dict(cmap=np.zeros(Nsym * N, np.int32), inv=np.zeros(max(S, 1), np.uint16), d0=np.zeros(Nsym, np.int32),
             n=np.zeros(Nsym, np.int32), n0=np.zeros(Nsym, np.int32), part=np.zeros(max(S, 1), np.int32),
             bnd=np.zeros(2 * Nsym * (P + 1), np.int32), csel=np.zeros(Nsym * N, np.uint8),
             dbin=np.zeros(max(nd, 1), np.uint16), dval=np.zeros(max(nd, 1), np.complex64),
             ind=np.zeros(max(ni, 1), np.uint32), grp=np.zeros(4 * ng, np.int32), zrun=np.zeros(2 * ng, np.int32),
             gather_d=np.zeros(M, np.int32), aux=np.zeros(aux_len, np.complex64))
    order = ["cmap", "inv", "d0", "n", "n0", "part", "bnd", "csel", "dbin", "dval", "ind", "grp", "zrun", "gather_d",
             "aux"]
    assert L.t2probe_chain_cls(p(a), p(g), cls, p(sz), *[p(t[k]) for k in order]) == 0
    t.update(Nsym=Nsym, N=N, S=S, split=split, nplp=P, ncls=ncls, nd=nd, ni=ni, l1_lo=l1_lo, Lp=Lp, miso=miso, M=M,
             unit=unit)
    for k in ("inv", "part"):
        t[k] = t[k][:S]
    t["dbin"], t["dval"], t["ind"] = t["dbin"][:nd], t["dval"][:nd], t["ind"][:ni]
    t["cmap"], t["csel"] = t["cmap"].reshape(Nsym, N), t["csel"].reshape(Nsym, N)
    t["grp"], t["zrun"], t["bnd"] = t["grp"].reshape(ng, 4), t["zrun"].reshape(ng, 2), t["bnd"].reshape(2 * Nsym, P + 1)
    return t


def flip(v, sel):
    """the kernels' sign flip: selector 0 (x, -y), selector 1 (-x, y)"""
    w = np.ascontiguousarray(v, np.complex64).view(np.uint32).reshape(-1, 2).copy()
    sel = np.asarray(sel, np.uint32)
    w[:, 0] ^= sel << np.uint32(31)
    w[:, 1] ^= (sel ^ np.uint32(1)) << np.uint32(31)
    return w.reshape(-1).view(np.complex64)


def scatter_carriers(t, mapped, l1cells, isinc=None):
    """the scatter-mode fill of every symbol as the OFDM kernels do it, from the planner's tables alone: the
    zero run, the direct aux quads, the indirect L1-post entries (bin | code << 15, MISO: selector in bit 31 over
    a 16-bit code), then the symbol's data slots through inv (MISO: selector in bit 15); every bin written
    exactly once.  The data slots hold the frame's data cells (frame data index d of mapped cell m with
    gather_d[m] = d, at slot part[d]).  Returns Nsym x N carriers in pilotgen's order (fftshifted, after EQ)."""
    N, Nsym, split, miso = t["N"], t["Nsym"], t["split"], t["miso"]
    nsub = N // 2 if split else N
    gd = t["gather_d"]
    slots = np.zeros(max(t["S"], 1), np.complex64)
    isd = gd >= 0
    slots[t["part"][gd[isd]]] = mapped[isd]
    out = np.zeros((Nsym, N), np.complex64)
    k = np.arange(N)
    for j in range(Nsym):
        row = np.zeros(N, np.complex64)
        hits = np.zeros(N, np.int32)
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
            code = (e >> 15) & 0xFFFF if miso else e >> 15
            v = l1cells[code - 1]
            row[base + (e & 0x7FFF)] = flip(v, e >> 31) if miso else v
            np.add.at(hits, base + (e & 0x7FFF), 1)
        s0, n, n0 = int(t["d0"][j]), int(t["n"][j]), int(t["n0"][j])
        inv = t["inv"][s0:s0 + n].astype(np.int64)
        bins = inv & 0x7FFF if miso else inv
        if split:   # the first n0 slots feed stored half 0, the rest half 1
            assert (bins[:n0] < nsub).all() and (bins[n0:] >= nsub).all()
        else:
            assert n0 == n
        v = slots[s0:s0 + n]
        row[bins] = flip(v, inv >> 15) if miso else v
        np.add.at(hits, bins, 1)
        assert (hits == 1).all(), "symbol %d: a bin written %d times" % (j, hits[hits != 1][0])
        nat = PP.stored_to_natural(row, N, split)
        car = np.empty(N, np.complex64)
        car[(k + N // 2) % N] = nat
        if isinc is not None:
            car = (car.view(np.float32).reshape(-1, 2) * isinc[:, None]).view(np.complex64).reshape(-1)
        out[j] = car
    return out


def gather_carriers(plan, cells):
    """the gather-mode load of the pilotgen block from PilotPlan::bin_map (data codes: partner cell | selector
    << 30 when processed), in pilotgen's order, after EQ"""
    N = plan["N"]
    aux = np.zeros(16, np.complex64)
    aux[1:13] = plan["pilot_values"]
    k = np.arange(N)
    out = np.zeros((plan["Nsym"], N), np.complex64)
    for j in range(plan["Nsym"]):
        code = plan["bin_map"][j].astype(np.int64)
        isd = code >= 0
        row = aux[np.clip(-code - 1, 0, None)].astype(np.complex64)
        row[isd] = flip(cells[code[isd] & 0x3FFFFFFF], code[isd] >> 30)
        car = np.empty(N, np.complex64)
        car[(k + N // 2) % N] = row
        if plan["eq"]:
            car = (car.view(np.float32).reshape(-1, 2) * plan["isinc"][:, None]).view(np.complex64).reshape(-1)
        out[j] = car
    return out
