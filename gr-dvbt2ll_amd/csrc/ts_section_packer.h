// Packing variable-length units (ULE SNDUs, MPE and MPE-FEC sections) into 188-byte TS packets, shared by
// ule_kernels.hip (the state scan only: it keeps an emit of its own), mpe_kernels.hip and mpefec_kernels.hip.  DESIGN.md 5.24 describes it once; in short:
//
// The pointer byte makes a packet's capacity depend on whether a unit starts in it, so where a unit lands depends on
// every unit before it through a small state: q, the payload bytes used in the open PUSI packet (0: none open).  A
// packet with fewer than MINFREE free bytes is closed (ULE: 2, a Length field must fit; sections: 1).  A unit of n
// bytes maps (q, packets completed) to (q', packets completed'), and such maps compose, so the positions come from a
// scan over maps:
//   maps      one workgroup per tile of PK_TILE units; lane q walks the tile from entry state q and stores
//             (packets completed << 8 | exit state)
//   compose   one workgroup; PK_ROUND tile maps at a time are composed by a Hillis-Steele scan in LDS and applied to
//             the running (state, packets), which is carried from round to round: each tile's entry
//   walk      one workgroup per tile walks it from its entry: per unit its first packet and payload offset
//   emit      one workgroup per PK_EMIT_PKTS output packets: a lane per packet finds what the packet begins with (a
//             search in the per-unit first packets) into LDS, then a lane per 16 output bytes gathers TS header /
//             pointer / unit bytes / FF and stores a head up to the first 16-byte boundary, then uint4s
// The bodies are __forceinline__; each block keeps thin __global__ wrappers under its own kernel names.  What a unit's
// bytes are comes from the block, as a Src with byte(j, k) and word(j, k): byte k, and bytes k .. k + 3, of unit j.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace t2 {

constexpr int PK_STATES = 184, PK_TILE = 512, PK_ROUND = 32, PK_COMPOSE_THREADS = 512;
constexpr int PK_PER = (PK_ROUND * PK_STATES + PK_COMPOSE_THREADS - 1) / PK_COMPOSE_THREADS;   // map entries of a round per compose lane
constexpr uint32_t PK_LEN = 0xFFFFu;     // a length word's low bits: the unit's bytes (0: skipped); the rest is the block's
constexpr uint32_t PK_EMIT_PKTS = 64;
constexpr uint32_t PK_THREADS = 256;   // lanes of a maps, walk, emit or count workgroup: the wrappers launch with it

// per unit: its length word, the packet its first byte of this call lies in, that byte's payload offset (0: the unit
// continues an earlier call's)
struct PkUnits {
  const uint32_t *len;
  uint32_t *pkt;
  uint8_t *at;
  uint32_t N;
};

// ------------------------------------------------------------------------------------------ the state scan
// one unit of n bytes (0: skipped) entered in state q with pk packets completed; cont: it continues an earlier call's
// unit, which begins the call's first packet without a pointer.  packing false: every unit starts a packet behind
// pointer 0
template <int MINFREE>
__device__ inline void pk_step(uint32_t n, bool cont, bool packing, uint32_t &q, uint32_t &pk) {
  if (!n) return;
  if (!packing) {
    pk += cont ? (n + 183) / 184 : (n + 184) / 184;
    q = 0;
    return;
  }
  uint32_t rem = n;
  if (!cont) {
    const uint32_t a = q ? q : 1, space = 184 - a;
    if (n <= space) {
      const uint32_t e = a + n;
      if (e >= 185 - MINFREE) { pk++; q = 0; }   // fewer than MINFREE bytes free (FF): the packet is closed
      else q = e;                                // the next unit still starts here
      return;
    }
    pk++;
    rem = n - space;
  }
  pk += rem / 184;
  rem %= 184;
  if (rem == 0) q = 0;
  else if (rem >= 184 - MINFREE) { pk++; q = 0; }   // no pointer can point inside the packet: the rest is FF
  else q = 1 + rem;                                 // PUSI, pointer = rem: the next unit starts behind it
}

// the tile's unit lengths into LDS; the first of the call less the s bytes an earlier call emitted
__device__ inline void pk_tile_lens(const uint32_t *len, uint32_t N, uint32_t base, uint32_t s, uint16_t *ln) {
  for (uint32_t k = threadIdx.x; k < (uint32_t)PK_TILE; k += blockDim.x) {
    const uint32_t i = base + k;
    uint32_t v = i < N ? len[i] & PK_LEN : 0;
    if (i == 0 && v) v -= s;
    ln[k] = (uint16_t)v;
  }
  __syncthreads();
}

template <int MINFREE>
__device__ __forceinline__ void pk_maps_body(const uint32_t *len, uint32_t N, uint32_t s, bool packing, uint32_t *maps) {
  __shared__ uint16_t ln[PK_TILE];
  const uint32_t base = blockIdx.x * PK_TILE;
  pk_tile_lens(len, N, base, s, ln);
  if (threadIdx.x >= (uint32_t)PK_STATES) return;
  uint32_t q = threadIdx.x, pk = 0;
  pk_step<MINFREE>(ln[0], s != 0 && base == 0, packing, q, pk);
  for (int k = 1; k < PK_TILE; k++) pk_step<MINFREE>(ln[k], false, packing, q, pk);
  maps[(size_t)blockIdx.x * PK_STATES + threadIdx.x] = (pk << 8) | q;
}

// total, endq: the packets completed and the state after the last tile
__device__ __forceinline__ void pk_compose_body(const uint32_t *maps, uint32_t ntiles, uint32_t *ent_q, uint32_t *ent_pk,
                                                uint32_t *total_pk, uint32_t *endq) {
  __shared__ uint32_t buf[2][PK_ROUND * PK_STATES];
  const uint32_t total = ntiles * PK_STATES;
  uint32_t cq = 0, cpk = 0;   // the running state: entered the round with
  uint32_t nxt[PK_PER];
#pragma unroll
  for (int k = 0; k < PK_PER; k++) {
    const uint32_t e = threadIdx.x + k * PK_COMPOSE_THREADS;
    nxt[k] = e < total ? maps[e] : e % PK_STATES;
  }
  // the second round (tiles PK_ROUND and up) begins at this loop's second pass: cq / cpk then hold the state and the
  // packets after the tiles before it, and the round's maps were fetched during the round before
  for (uint32_t b = 0; b < ntiles; b += PK_ROUND) {
    uint32_t *A = buf[0], *B = buf[1];
#pragma unroll
    for (int k = 0; k < PK_PER; k++) {
      const uint32_t e = threadIdx.x + k * PK_COMPOSE_THREADS;
      if (e < (uint32_t)(PK_ROUND * PK_STATES)) A[e] = nxt[k];
    }
    if (b + PK_ROUND < ntiles) {
#pragma unroll
      for (int k = 0; k < PK_PER; k++) {
        const uint32_t e = threadIdx.x + k * PK_COMPOSE_THREADS, g = (b + PK_ROUND) * PK_STATES + e;
        nxt[k] = g < total ? maps[g] : e % PK_STATES;   // past the last tile: the identity
      }
    }
    __syncthreads();
    // inclusive scan over the round's tiles: A[t] becomes tiles b .. b + t composed in order
    for (int dd = 1; dd < PK_ROUND; dd <<= 1) {
#pragma unroll
      for (int k = 0; k < PK_PER; k++) {
        const uint32_t e = threadIdx.x + k * PK_COMPOSE_THREADS;
        if (e < (uint32_t)(PK_ROUND * PK_STATES)) {
          const uint32_t t = e / PK_STATES;
          uint32_t v = A[e];
          if (t >= (uint32_t)dd) {
            const uint32_t f = A[e - dd * PK_STATES];               // the tiles before, from this entry state
            v = (f & ~255u) + A[t * PK_STATES + (f & 255u)];        // then these, from the state those leave
          }
          B[e] = v;
        }
      }
      __syncthreads();
      uint32_t *x = A; A = B; B = x;
    }
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)PK_ROUND && b + t < ntiles) {
      uint32_t eq = cq, epk = cpk;
      if (t) {
        const uint32_t f = A[(t - 1) * PK_STATES + cq];
        eq = f & 255u;
        epk = cpk + (f >> 8);
      }
      ent_q[b + t] = eq;
      ent_pk[b + t] = epk;
    }
    const uint32_t f = A[(PK_ROUND - 1) * PK_STATES + cq];
    cq = f & 255u;
    cpk += f >> 8;
    __syncthreads();   // the next round overwrites the buffers
  }
  if (threadIdx.x == 0) {
    *total_pk = cpk;
    *endq = cq;
  }
}

template <int MINFREE>
__device__ __forceinline__ void pk_walk_body(const PkUnits &u, uint32_t s, bool packing, const uint32_t *ent_q,
                                             const uint32_t *ent_pk) {
  __shared__ uint16_t ln[PK_TILE];
  __shared__ uint32_t pk_s[PK_TILE];
  __shared__ uint8_t at_s[PK_TILE];
  const uint32_t base = blockIdx.x * PK_TILE;
  pk_tile_lens(u.len, u.N, base, s, ln);
  if (threadIdx.x == 0) {
    uint32_t q = ent_q[blockIdx.x], pk = ent_pk[blockIdx.x];
    for (int k = 0; k < PK_TILE; k++) {
      const bool cont = k == 0 && base == 0 && s != 0;
      pk_s[k] = pk;
      at_s[k] = (uint8_t)(cont ? 0 : q ? q : 1);
      pk_step<MINFREE>(ln[k], cont, packing, q, pk);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < (uint32_t)PK_TILE; k += PK_THREADS)
    if (base + k < u.N) {
      u.pkt[base + k] = pk_s[k];
      u.at[base + k] = at_s[k];
    }
}

// ------------------------------------------------------------------------------------------ unit bytes
// the four bytes at src (all readable) as one aligned word, or as two joined by a shift where both lie inside
// [lo, hi); false: neither, the caller reads bytes
__device__ inline bool pk_read4(const uint8_t *src, const uint8_t *lo, const uint8_t *hi, uint32_t &w) {
  const uint32_t sh = (uint32_t)((uintptr_t)src & 3);
  const uint8_t *a = src - sh;
  if (sh == 0) {
    w = *(const uint32_t *)a;
    return true;
  }
  if (a >= lo && a + 8 <= hi) {
    const uint32_t l = *(const uint32_t *)a, h = *(const uint32_t *)(a + 4);
    w = (l >> (8 * sh)) | (h << (32 - 8 * sh));
    return true;
  }
  return false;
}

// ------------------------------------------------------------------------------------------ the cut, positions
struct PkCut {
  uint32_t T, q, s;    // packets completed, the end state (an open PUSI packet when not 0), the start's unit byte
  uint32_t E;          // packets emitted
  bool all;            // nothing is left
};

// lim: packets the block allows at most, whatever is determined
__device__ inline PkCut pk_cut(uint32_t T, uint32_t q, uint32_t s, bool flush, uint32_t cap, uint32_t lim = ~0u) {
  PkCut c;
  c.T = T;
  c.q = q;
  c.s = s;
  uint32_t det = T + (q && flush ? 1 : 0);   // the open packet is determined by a flush only
  if (lim < det) det = lim;
  c.E = det < cap ? det : cap;
  c.all = c.E == det && (q == 0 || flush);
  return c;
}

// what packet p begins with: R > 0 bytes left of unit jc, from its byte coff on; jn: the first unit that can start in
// the packet
struct PkPos { uint32_t jc, R, coff, jn; };

__device__ inline PkPos pk_locate(const PkUnits &u, uint32_t s, uint32_t p) {
  uint32_t lo = 0, hi = u.N;   // the first unit whose first packet is p or later
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (u.pkt[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  PkPos ps{0, 0, 0, lo};
  if (p == 0 && s && u.N) {   // the unit an earlier call began
    ps.R = (u.len[0] & PK_LEN) - s;
    ps.coff = s;
    ps.jn = 1;
  } else if (lo > 0) {
    // the unit before is valid (only a valid one moves the packet count): it may run on into p
    const uint32_t j = lo - 1, n = u.len[j] & PK_LEN, sk = j == 0 ? s : 0;
    const uint32_t consumed = (184 - u.at[j]) + 184 * (p - u.pkt[j] - 1);
    ps.jc = j;
    ps.coff = sk + consumed;
    ps.R = n > ps.coff ? n - ps.coff : 0;
  }
  return ps;
}

// the resume position where something is left: the unit jr and its bytes emitted.  The whole workgroup calls it
__device__ __forceinline__ void pk_resume(const PkUnits &u, const PkCut &c, uint32_t &jr, uint32_t &sb) {
  __shared__ uint32_t found;
  const PkPos ps = pk_locate(u, c.s, c.E);
  if (ps.R) {
    jr = ps.jc;
    sb = ps.coff;
    return;
  }
  if (threadIdx.x == 0) found = u.N;
  __syncthreads();
  // the first valid unit from ps.jn on: the workgroup looks at PK_THREADS at a time
  for (uint32_t base = ps.jn; base < u.N; base += PK_THREADS) {
    const uint32_t x = base + threadIdx.x;
    if (x < u.N && (u.len[x] & PK_LEN)) atomicMin(&found, x);
    __syncthreads();
    const uint32_t f = found;
    __syncthreads();
    if (f < u.N) break;
  }
  jr = found;
}

// ------------------------------------------------------------------------------------------ emit
struct PkRec {
  uint32_t jc, jn, jend;   // the continuing unit; the units whose first packet this is: [jn, jend)
  uint16_t R, coff;
  uint8_t pusi, nb;        // PUSI 0: nb unit bytes, the rest FF
};

template <int MINFREE>
__device__ inline PkRec pk_record(const PkUnits &u, const PkCut &c, bool packing, uint32_t p, uint32_t &pad) {
  const PkPos ps = pk_locate(u, c.s, p);
  PkRec q;
  q.jc = ps.jc;
  q.jn = q.jend = ps.jn;
  q.R = (uint16_t)ps.R;
  q.coff = (uint16_t)ps.coff;
  bool pusi;
  if (!packing) pusi = ps.R == 0;
  // packing: what is left fills the packet or leaves no room to point at; the flush's last packet holding nothing but
  // a unit's end has no pointer
  else pusi = !(ps.R >= 184 - MINFREE || (p == c.T && ps.R && c.q == 1 + ps.R));
  q.pusi = pusi;
  q.nb = 0;
  if (!pusi) {
    q.nb = (uint8_t)(ps.R < 184 ? ps.R : 184);
    pad = 184 - q.nb;
  } else {
    uint32_t used = 1 + ps.R, x = ps.jn;
    for (; x < u.N && u.pkt[x] == p; x++) {
      const uint32_t n = u.len[x] & PK_LEN;
      if (n) used = u.at[x] + n < 184 ? u.at[x] + n : 184;
    }
    q.jend = x;
    pad = 184 - used;
  }
  return q;
}

// payload byte b of a packet: true with (j, k) where it is byte k of unit j, else lit is the byte
__device__ inline bool pk_resolve(const PkUnits &u, const PkRec &q, uint32_t b, uint32_t &j, uint32_t &k, uint32_t &lit) {
  lit = 0xFF;
  if (!q.pusi) {
    if (b >= q.nb) return false;
    j = q.jc;
    k = q.coff + b;
    return true;
  }
  if (b == 0) { lit = q.R; return false; }
  if (b < 1u + q.R) {
    j = q.jc;
    k = q.coff + b - 1;
    return true;
  }
  for (uint32_t x = q.jn; x < q.jend; x++) {
    const uint32_t n = u.len[x] & PK_LEN, a = u.at[x];
    if (!n) continue;
    if (a > b) break;
    if (b < a + n) {
      j = x;
      k = b - a;
      return true;
    }
  }
  return false;
}

// byte o of packet p; cc0: the call's first continuity counter
template <class Src>
__device__ inline uint32_t pk_out_byte(const Src &src, const PkUnits &u, const PkRec &q, uint32_t pid, uint32_t cc0,
                                       uint32_t p, uint32_t o) {
  if (o == 0) return 0x47;
  if (o == 1) return ((uint32_t)q.pusi << 6) | (pid >> 8);
  if (o == 2) return pid & 255;
  if (o == 3) return 0x10 | ((cc0 + p) & 15);
  uint32_t j, k, lit;
  if (pk_resolve(u, q, o - 4, j, k, lit)) return src.byte(j, k);
  return lit;
}

// output bytes g .. g + 3 (packets p0 and up: rec)
template <class Src>
__device__ inline uint32_t pk_out_word(const Src &src, const PkUnits &u, const PkRec *rec, uint32_t pid, uint32_t cc0,
                                       uint32_t p0, size_t g) {
  const uint32_t p = (uint32_t)(g / 188), o = (uint32_t)(g - (size_t)p * 188);
  if (o >= 4 && o + 4 <= 188) {
    uint32_t j, k, lit;
    if (pk_resolve(u, rec[p - p0], o - 4, j, k, lit) && k + 4 <= (u.len[j] & PK_LEN)) return src.word(j, k);
  }
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t pp = (uint32_t)((g + q) / 188), oo = (uint32_t)(g + q - (size_t)pp * 188);
    w |= pk_out_byte(src, u, rec[pp - p0], pid, cc0, pp, oo) << (8 * q);
  }
  return w;
}

// The grid covers the packets that PDUs lying side by side can become; where the offsets make valid PDUs overlap and
// the packets are more, a workgroup takes more than one group of PK_EMIT_PKTS: its second trip begins at the loop's
// second pass.  res_pusi, res_pad: the counters of PUSI packets and of FF bytes
template <int MINFREE, class Src>
__device__ __forceinline__ void pk_emit_body(const Src &src, const PkUnits &u, const PkCut &c, bool packing, uint32_t pid,
                                             uint32_t cc0, uint8_t *out, unsigned long long *res_pusi,
                                             unsigned long long *res_pad) {
  __shared__ PkRec rec[PK_EMIT_PKTS];
  __shared__ uint32_t cnt[2];
  for (uint32_t p0 = blockIdx.x * PK_EMIT_PKTS; p0 < c.E; p0 += gridDim.x * PK_EMIT_PKTS) {
    const uint32_t np = c.E - p0 < PK_EMIT_PKTS ? c.E - p0 : PK_EMIT_PKTS;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();   // the trip before no longer reads rec
    if (threadIdx.x < np) {
      uint32_t pad = 0;
      rec[threadIdx.x] = pk_record<MINFREE>(u, c, packing, p0 + threadIdx.x, pad);
      if (rec[threadIdx.x].pusi) atomicAdd(&cnt[0], 1u);
      if (pad) atomicAdd(&cnt[1], pad);
    }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x])
      atomicAdd(threadIdx.x ? res_pad : res_pusi, (unsigned long long)cnt[threadIdx.x]);
    // output bytes [g0, g1): chunk 0 runs up to the first 16-byte boundary, the others are 16 bytes (the last shorter)
    const size_t g0 = (size_t)p0 * 188, g1 = g0 + (size_t)np * 188;
    uint32_t head = (uint32_t)((16 - ((uintptr_t)(out + g0) & 15)) & 15);
    if (head > g1 - g0) head = (uint32_t)(g1 - g0);
    const uint32_t nchunks = 1 + (uint32_t)((g1 - g0 - head + 15) / 16);
    for (uint32_t cidx = threadIdx.x; cidx < nchunks; cidx += PK_THREADS) {
      const size_t lo = cidx ? g0 + head + (size_t)(cidx - 1) * 16 : g0;
      const size_t hi = cidx ? (g1 < lo + 16 ? g1 : lo + 16) : g0 + head;
      if (hi <= lo) continue;
      if (cidx && hi - lo == 16) {
        uint32_t w[4];
        for (uint32_t q = 0; q < 4; q++) w[q] = pk_out_word(src, u, rec, pid, cc0, p0, lo + 4 * q);
        *(uint4 *)(out + lo) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (size_t g = lo; g < hi; g++) {
          const uint32_t p = (uint32_t)(g / 188), o = (uint32_t)(g - (size_t)p * 188);
          out[g] = (uint8_t)pk_out_byte(src, u, rec[p - p0], pid, cc0, p, o);
        }
      }
    }
  }
}

}  // namespace t2
