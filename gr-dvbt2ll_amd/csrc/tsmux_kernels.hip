// TS multiplexer on gfx950: up to 8 device buffers of TS packets -> one constant-bit-rate TS with null and PCR packets.
// Semantics: include/dvbt2ll_hip.h; tests/tsmux_ref.py is the sequential restatement every output is compared with.
//
// The schedule is periodic and fixed at create, so what output packet m carries follows from m alone: its table slot
// gives the owner, and the owner's prefix counts give the rank of the slot among the owner's slots of this call, which
// is the index of the input packet.  A fill input's rank adds the other owners' free slots before m, which are closed
// forms of their ranks too.  So there is no scan and one kernel:
//   resolve   a lane per output packet of the workgroup's TSMUX_PKTS: the table slot, the owner, the ranks (one row of
//             the prefix table: the owners of a slot lie side by side, and neighbouring lanes read neighbouring rows),
//             the source packet's address or the first 12 bytes of a null / PCR packet, into LDS; the sync byte is
//             looked at here; the counters go to LDS and leave the workgroup as one atomic per counter that moved
//   copy      a lane per 16 output bytes: a head up to the output's first 16-byte boundary, then uint4 stores.  188 is
//             no multiple of 16, so a source packet's alignment against the output differs from packet to packet by
//             multiples of 4: where the source is word-aligned against the output the words are loaded as they are,
//             otherwise each is two aligned words joined by a shift; a packet's first and last word, which the aligned
//             pair would read outside the packet, and the words that straddle two packets go byte by byte
// The per-owner values of the launch (weights, packet counts, positions, buffers) are copied from the kernel arguments
// into LDS with constant indices first: indexing the argument structs by the owner would put them into scratch.
//
// A handle with a remux (PID remapping, continuity and PCR restamping; tests/tsremux_ref.py) runs four kernels.  Only a
// packet's continuity counter depends on other packets: on how many earlier packets of its PID carried a payload.
//   classify  a lane per output packet resolves it as above (tsmux_resolve is shared), reads its 4 header bytes, maps
//             the PID, looks up the tracked slot and adds a payload packet to its tile's 64 per-slot counts in LDS; a
//             tile is the TSREMUX_TILE packets of one trip, and its row of 64 bytes goes to a scratch table
//   scan      two rounds: a workgroup per chunk of TSREMUX_SCAN_TILES tiles turns the chunk's rows into exclusive
//             prefixes and leaves the chunk's totals; one workgroup then runs over the chunks, starting at the call's
//             start counters.  Everything is kept mod 256, of which a counter needs the low 4 bits
//   emit      tsmux_mux's remux instantiation: resolve also loads a source packet's first 12 bytes into its record,
//             patches PID, counter and PCR there, and the copy phase takes bytes 0 .. 11 from the record.  The rank
//             inside the tile comes from wave ballots: a tile is one wave
#include "tsmux_kernels.h"

#include <algorithm>

namespace t2 {

namespace {

constexpr uint32_t NULL_HEAD = 0x10FF1F47u;   // 47 1F FF 10
constexpr unsigned long long PCR_WRAP = (1ull << 33) * 300ull;

static_assert(TSREMUX_TILE == 64, "a tile is one wave: the rank inside it comes from 64-lane ballots");

struct TsmuxRec {
  const uint8_t *src;    // the input packet; nullptr: a null or PCR packet made of h, w1, w2 and FF
  uint32_t h, w1, w2;    // its bytes 0 .. 11 as little-endian words (remux: also those of an input packet, patched)
};

// bytes o .. o + 3 of a packet, o + 4 <= 188
template <bool REMUX>
__device__ inline uint32_t tsmux_word(const TsmuxRec &q, uint32_t o) {
  const uint32_t sh = 8 * (o & 3);
  if (!q.src || (REMUX && o < 12)) {
    const uint32_t k = o >> 2;
    const uint32_t lo = k == 0 ? q.h : k == 1 ? q.w1 : k == 2 ? q.w2 : 0xFFFFFFFFu;
    if (!sh) return lo;
    uint32_t hi = k == 0 ? q.w1 : k == 1 ? q.w2 : 0xFFFFFFFFu;
    if (REMUX && q.src && k == 2)   // bytes 12 .. 14 of an input packet
      hi = (uint32_t)q.src[12] | ((uint32_t)q.src[13] << 8) | ((uint32_t)q.src[14] << 16);
    return (lo >> sh) | (hi << (32 - sh));
  }
  const uint8_t *s = q.src + o;
  const uint32_t mis = (uint32_t)((uintptr_t)s & 3);
  if (!mis) return *(const uint32_t *)s;
  if (o >= 4 && o + 8 <= 188) {   // both aligned words lie inside the packet
    const uint8_t *a = s - mis;
    const uint32_t lo = *(const uint32_t *)a, hi = *(const uint32_t *)(a + 4);
    return (lo >> (8 * mis)) | (hi << (32 - 8 * mis));
  }
  return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
}

template <bool REMUX>
__device__ inline uint32_t tsmux_byte(const TsmuxRec &q, uint32_t o) {
  if (q.src && !(REMUX && o < 12)) return q.src[o];
  const uint32_t w = o < 4 ? q.h : o < 8 ? q.w1 : o < 12 ? q.w2 : 0xFFFFFFFFu;
  return (w >> (8 * (o & 3))) & 255;
}

// bytes l .. l + 3 of the trip's output (packet l / 188 of rec)
template <bool REMUX>
__device__ inline uint32_t tsmux_out_word(const TsmuxRec *rec, uint32_t l) {
  const uint32_t p = l / 188, o = l - p * 188;
  if (o + 4 <= 188) return tsmux_word<REMUX>(rec[p], o);
  uint32_t w = 0;
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t pp = (l + k) / 188, oo = l + k - pp * 188;
    w |= tsmux_byte<REMUX>(rec[pp], oo) << (8 * k);
  }
  return w;
}

// the per-owner values of the launch, in LDS
struct TsmuxStaged {
  uint32_t w[TSMUX_OWN], pre0[TSMUX_OWN], nin[TSMUX_IN], next[TSMUX_IN];
  const uint8_t *in[TSMUX_IN];
};

__device__ __forceinline__ void tsmux_stage(const TsmuxDev &d, const TsmuxRun &r, TsmuxStaged &s) {
#pragma unroll
  for (int i = 0; i < TSMUX_OWN; i++)
    if (threadIdx.x == (uint32_t)i) {
      s.w[i] = d.w[i];
      s.pre0[i] = r.pre0[i];
    }
#pragma unroll
  for (int i = 0; i < TSMUX_IN; i++)
    if (threadIdx.x == (uint32_t)(32 + i)) {
      s.nin[i] = r.n_in[i];
      s.next[i] = r.next[i];
      s.in[i] = r.in[i];
    }
}

// what output packet m of the call carries
struct TsmuxPick {
  int e;             // the slot's owner
  int src;           // the input whose packet idx it carries, or -1: a PCR or null packet
  uint32_t idx, j;   // j: the packet's rank among its input's packets in this call (not reduced for a loop input)
  uint32_t dc, t;    // the period of the call and the table slot
};

// COUNT: the slot's counters go to cnt (TSMUX_R_DRY, TSMUX_R_FILL_IN_FREE, TSMUX_R_CONSUMED)
template <bool COUNT>
__device__ __forceinline__ TsmuxPick tsmux_resolve(const TsmuxDev &d, const TsmuxRun &r, const TsmuxStaged &s,
                                                   uint32_t m, uint32_t *cnt) {
  const int n = d.n, no = d.owners, f = d.fill;
  const uint32_t mm = r.phase + m, dc = mm / d.period, t = mm - dc * d.period;
  const int e = d.table[t];
  const uint32_t *row = d.pre + (size_t)t * no;
  // the owner's slots in this call before this one
  auto rank = [&](int x) { return dc * s.w[x] + row[x] - s.pre0[x]; };
  int src = -1;
  uint32_t idx = 0, j = 0;
  bool claim = false;
  if (e == n) {   // the PCR generator
  } else if (e > n || e == f) claim = true;   // null's slot, the fill input's own
  else {
    const uint32_t rr = rank(e), ni = s.nin[e];
    if ((d.loop >> e) & 1) {
      if (ni) { src = e; idx = (s.next[e] + rr) % ni; }
      else claim = true;
    } else if (rr < ni - s.next[e]) { src = e; idx = s.next[e] + rr; }
    else claim = true;
    j = rr;
    if (COUNT && claim) atomicAdd(&cnt[TSMUX_R_DRY + e], 1u);
  }
  if (claim && f >= 0) {
    uint32_t c = rank(f) + rank(n + 1);
    for (int i = 0; i < n; i++) {
      if (i == f) continue;
      const uint32_t rr = rank(i), ni = s.nin[i], av = ni - s.next[i];
      if ((d.loop >> i) & 1) c += ni ? 0 : rr;
      else c += rr > av ? rr - av : 0;
    }
    if (c < s.nin[f] - s.next[f]) {
      src = f;
      idx = s.next[f] + c;
      j = c;
      if (COUNT && e != f) atomicAdd(&cnt[TSMUX_R_FILL_IN_FREE], 1u);
    } else if (COUNT && e == f) atomicAdd(&cnt[TSMUX_R_DRY + f], 1u);
  }
  if (COUNT && src >= 0) atomicAdd(&cnt[TSMUX_R_CONSUMED + src], 1u);
  return TsmuxPick{e, src, idx, j, dc, t};
}

// the 27 MHz clock of table slot t in period dc of the call, mod W
__device__ __forceinline__ unsigned long long tsmux_slot_clock(const TsmuxDev &d, const TsmuxRun &r, uint32_t dc,
                                                               uint32_t t) {
  return (r.pcr_ticks + (unsigned long long)dc * d.tpp + (unsigned long long)t * d.tpp_q + (t * d.tpp_r) / d.period) %
         PCR_WRAP;
}

// the remux values per input, in LDS
struct TsremuxStaged {
  uint32_t period[TSMUX_IN], phase[TSMUX_IN], r[TSMUX_IN];
  unsigned long long tpp[TSMUX_IN], q[TSMUX_IN], ticks[TSMUX_IN];
};

// x and y are null in the plain instantiation, which is the kernel a handle without a remux launches
template <bool REMUX>
__device__ __forceinline__ void tsmux_body(const TsmuxDev &d, const TsmuxRun &r, const TsremuxDev *x,
                                           const TsremuxRun *y) {
  __shared__ TsmuxRec rec[TSMUX_PKTS];
  __shared__ uint32_t cnt[TSMUX_R_WORDS];
  __shared__ TsmuxStaged s;
  __shared__ TsremuxStaged sx;    // remux only
  __shared__ uint32_t rcnt[TSREMUX_R_CC];
  if (threadIdx.x < (uint32_t)TSMUX_R_WORDS) cnt[threadIdx.x] = 0;
  tsmux_stage(d, r, s);
  if constexpr (REMUX) {
    if (threadIdx.x >= 128 && threadIdx.x < 128 + (uint32_t)TSREMUX_R_CC) rcnt[threadIdx.x - 128] = 0;
#pragma unroll
    for (int i = 0; i < TSMUX_IN; i++)
      if (threadIdx.x == (uint32_t)(64 + i)) {
        sx.period[i] = x->in_period[i];
        sx.phase[i] = y->in_phase[i];
        sx.r[i] = x->in_r[i];
        sx.tpp[i] = x->in_tpp[i];
        sx.q[i] = x->in_q[i];
        sx.ticks[i] = y->in_ticks[i];
      }
  }
  const int n = d.n;
  // past TSMUX_MAX_BLOCKS x TSMUX_PKTS packets the workgroup's second trip begins at this loop's second pass
  for (uint32_t p0 = blockIdx.x * TSMUX_PKTS; p0 < r.n_out; p0 += gridDim.x * TSMUX_PKTS) {
    const uint32_t np = r.n_out - p0 < TSMUX_PKTS ? r.n_out - p0 : TSMUX_PKTS;
    __syncthreads();   // the per-owner values are in LDS; the trip before no longer reads rec
    TsmuxRec q{nullptr, NULL_HEAD, 0xFFFFFFFFu, 0xFFFFFFFFu};
    uint32_t key = TSREMUX_NO_SLOT, pay = 0;   // remux: the tracked slot of a packet that is restamped; it has a payload
    if (threadIdx.x < np) {
      const TsmuxPick k = tsmux_resolve<true>(d, r, s, p0 + threadIdx.x, cnt);
      const int e = k.e, src = k.src;
      if (e == n) {   // the PCR generator
        const unsigned long long T = tsmux_slot_clock(d, r, k.dc, k.t);
        const unsigned long long base = T / 300;
        const uint32_t ext = (uint32_t)(T - base * 300);
        q.h = 0x47u | ((uint32_t)(d.pcr_pid >> 8) << 8) | ((uint32_t)(d.pcr_pid & 255) << 16) | (0x20u << 24);
        q.w1 = 0xB7u | (0x10u << 8) | ((uint32_t)((base >> 25) & 255) << 16) | ((uint32_t)((base >> 17) & 255) << 24);
        q.w2 = (uint32_t)((base >> 9) & 255) | ((uint32_t)((base >> 1) & 255) << 8) |
               ((((uint32_t)(base & 1) << 7) | 0x7Eu | (ext >> 8)) << 16) | ((ext & 255u) << 24);
        atomicAdd(&cnt[TSMUX_R_PCR], 1u);
      }
      if (src >= 0) {
        const uint8_t *pk = s.in[src] + (size_t)k.idx * 188;
        if (pk[0] == 0x47) q.src = pk;
        else atomicAdd(&cnt[TSMUX_R_SYNC], 1u);
      }
      if constexpr (REMUX) {
        if (q.src) {   // remap, then the PCR restamp; the counter follows below, where the whole wave takes part
          const uint8_t *pk = q.src;
          uint32_t b[12];
#pragma unroll
          for (int i = 0; i < 12; i++) b[i] = pk[i];
          uint32_t pid = ((b[1] & 0x1Fu) << 8) | b[2];
          const uint32_t mp = x->pid_map[(size_t)src * 8192 + pid];
          if (mp & TSREMUX_ENTRY) {
            pid = mp & 0x1FFFu;
            if (pid == TSREMUX_DROP) {
              q.src = nullptr;   // q is the null packet
              atomicAdd(&rcnt[TSREMUX_R_DROPPED], 1u);
            } else {
              b[1] = (b[1] & 0xE0u) | (pid >> 8);
              b[2] = pid & 255u;
              atomicAdd(&rcnt[TSREMUX_R_REMAPPED], 1u);
            }
          }
          if (q.src) {
            const uint32_t slot = x->slot_of[pid];
            if (((x->restamp_cc >> src) & 1) && slot != TSREMUX_NO_SLOT) {
              key = slot;
              pay = (b[3] >> 4) & 1;
            }
            const uint32_t per = sx.period[src];
            if (per && (b[3] & 0x20u) && b[4] >= 7 && (b[5] & 0x10u)) {
              const unsigned long long v = ((unsigned long long)b[6] << 40) | ((unsigned long long)b[7] << 32) |
                                           ((unsigned long long)b[8] << 24) | ((unsigned long long)b[9] << 16) |
                                           ((unsigned long long)b[10] << 8) | b[11];
              const unsigned long long pcr_in = ((v >> 15) * 300 + (v & 0x1FF)) % PCR_WRAP;
              const uint32_t g = sx.phase[src] + k.j, dq = g / per, rr = g - dq * per;
              const unsigned long long t_in = (sx.ticks[src] + (unsigned long long)dq * sx.tpp[src] +
                                               (unsigned long long)rr * sx.q[src] + (rr * sx.r[src]) / per) % PCR_WRAP;
              const unsigned long long T = (pcr_in + tsmux_slot_clock(d, r, k.dc, k.t) + PCR_WRAP - t_in) % PCR_WRAP;
              const unsigned long long base = T / 300;
              const uint32_t ext = (uint32_t)(T - base * 300);
              b[6] = (uint32_t)(base >> 25) & 255;
              b[7] = (uint32_t)(base >> 17) & 255;
              b[8] = (uint32_t)(base >> 9) & 255;
              b[9] = (uint32_t)(base >> 1) & 255;
              b[10] = ((uint32_t)(base & 1) << 7) | 0x7Eu | (ext >> 8);
              b[11] = ext & 255u;
              atomicAdd(&rcnt[TSREMUX_R_PCR], 1u);
            }
            q.h = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            q.w1 = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
            q.w2 = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
          }
        }
      }
      if (!q.src && e != n) atomicAdd(&cnt[TSMUX_R_NULL], 1u);
      if constexpr (!REMUX) rec[threadIdx.x] = q;
    }
    if constexpr (REMUX) {
      if (threadIdx.x < TSREMUX_TILE) {   // wave 0, all 64 lanes: those past np hold no slot
        // the lanes with this lane's slot, bit by bit of the 7-bit key (TSREMUX_NO_SLOT has bit 6, a slot has not)
        unsigned long long same = ~0ull;
#pragma unroll
        for (int bit = 0; bit < 7; bit++) {
          const bool on = (key >> bit) & 1;
          const unsigned long long m = __ballot(on);
          same &= on ? m : ~m;
        }
        const unsigned long long pays = __ballot(pay != 0);
        if (key != TSREMUX_NO_SLOT) {
          const uint32_t tile = p0 / TSREMUX_TILE;
          const uint32_t before = __popcll(same & pays & ((1ull << threadIdx.x) - 1));
          const uint32_t base = (uint32_t)x->chunks[(size_t)(tile / TSREMUX_SCAN_TILES) * TSREMUX_SLOTS + key] +
                                x->tiles[(size_t)tile * TSREMUX_SLOTS + key];
          const uint32_t cc = (base + before + (pay ? 0u : 15u)) & 15u;
          if (cc != ((q.h >> 24) & 15u)) atomicAdd(&rcnt[TSREMUX_R_CC_REWRITTEN], 1u);
          q.h = (q.h & 0xF0FFFFFFu) | (cc << 24);
        }
        if (threadIdx.x < np) rec[threadIdx.x] = q;
      }
    }
    __syncthreads();
    // output bytes [g0, g0 + nb): chunk 0 runs up to the first 16-byte boundary, the others are 16 bytes (the last shorter)
    uint8_t *out = r.out + (size_t)p0 * 188;
    const uint32_t nb = np * 188;
    uint32_t head = (uint32_t)((16 - ((uintptr_t)out & 15)) & 15);
    if (head > nb) head = nb;
    const uint32_t nchunks = 1 + (nb - head + 15) / 16;
    for (uint32_t cidx = threadIdx.x; cidx < nchunks; cidx += 256) {
      const uint32_t lo = cidx ? head + (cidx - 1) * 16 : 0;
      const uint32_t hi = cidx ? (nb < lo + 16 ? nb : lo + 16) : head;
      if (hi <= lo) continue;
      if (cidx && hi - lo == 16) {
        const uint32_t w0 = tsmux_out_word<REMUX>(rec, lo), w1 = tsmux_out_word<REMUX>(rec, lo + 4);
        const uint32_t w2 = tsmux_out_word<REMUX>(rec, lo + 8), w3 = tsmux_out_word<REMUX>(rec, lo + 12);
        *(uint4 *)(out + lo) = make_uint4(w0, w1, w2, w3);
      } else {
        for (uint32_t l = lo; l < hi; l++) {
          const uint32_t p = l / 188;
          out[l] = (uint8_t)tsmux_byte<REMUX>(rec[p], l - p * 188);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)TSMUX_R_WORDS && cnt[threadIdx.x])
    atomicAdd(&d.res[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
  if constexpr (REMUX) {
    if (threadIdx.x >= 128 && threadIdx.x < 128 + (uint32_t)TSREMUX_R_CC && rcnt[threadIdx.x - 128])
      atomicAdd(&x->res[threadIdx.x - 128], (unsigned long long)rcnt[threadIdx.x - 128]);
  }
}

__global__ __launch_bounds__(256) void tsmux_mux(TsmuxDev d, TsmuxRun r) { tsmux_body<false>(d, r, nullptr, nullptr); }

__global__ __launch_bounds__(256) void tsremux_emit(TsmuxDev d, TsmuxRun r, TsremuxDev x, TsremuxRun y) {
  tsmux_body<true>(d, r, &x, &y);
}

// a wave per tile, four tiles per trip: the payload packets each tracked slot gets in the tile
__global__ __launch_bounds__(256) void tsremux_classify(TsmuxDev d, TsmuxRun r, TsremuxDev x) {
  __shared__ TsmuxStaged s;
  __shared__ uint32_t row[4][TSREMUX_SLOTS];
  tsmux_stage(d, r, s);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t ntiles = (r.n_out + TSREMUX_TILE - 1) / TSREMUX_TILE;
  for (uint32_t t0 = blockIdx.x * 4; t0 < ntiles; t0 += gridDim.x * 4) {
    __syncthreads();   // the per-owner values are in LDS; the trip before has written its rows
    row[wave][lane] = 0;
    __syncthreads();
    const uint32_t tile = t0 + wave, m = tile * TSREMUX_TILE + lane;
    if (tile < ntiles && m < r.n_out) {
      const TsmuxPick k = tsmux_resolve<false>(d, r, s, m, nullptr);
      if (k.src >= 0 && ((x.restamp_cc >> k.src) & 1)) {
        const uint8_t *pk = s.in[k.src] + (size_t)k.idx * 188;
        if (pk[0] == 0x47 && (pk[3] & 0x10)) {
          uint32_t pid = (((uint32_t)pk[1] & 0x1Fu) << 8) | pk[2];
          pid = x.pid_map[(size_t)k.src * 8192 + pid] & 0x1FFFu;   // a dropped packet gets 1FFF, which is never tracked
          const uint32_t slot = x.slot_of[pid];
          if (slot != TSREMUX_NO_SLOT) atomicAdd(&row[wave][slot], 1u);
        }
      }
    }
    __syncthreads();
    if (tile < ntiles) x.tiles[(size_t)tile * TSREMUX_SLOTS + lane] = (uint8_t)row[wave][lane];
  }
}

// round 1, a workgroup per chunk of TSREMUX_SCAN_TILES tiles: a lane per slot and quarter of the chunk sums its rows, the
// quarters' sums are exchanged, and a second sweep leaves each row's exclusive prefix inside the chunk; the chunk's
// totals go to its row of chunks
__global__ __launch_bounds__(256) void tsremux_scan_tiles(TsremuxDev x, uint32_t ntiles) {
  __shared__ uint32_t tot[4][TSREMUX_SLOTS];
  constexpr uint32_t QUARTER = TSREMUX_SCAN_TILES / 4;
  const uint32_t g = threadIdx.x >> 6, col = threadIdx.x & 63;
  const uint32_t first = blockIdx.x * TSREMUX_SCAN_TILES + g * QUARTER;
  const uint32_t last = first + QUARTER < ntiles ? first + QUARTER : ntiles;   // first may lie past ntiles
  uint32_t sum = 0;
  for (uint32_t t = first; t < last; t++) sum += x.tiles[(size_t)t * TSREMUX_SLOTS + col];
  tot[g][col] = sum;
  __syncthreads();
  uint32_t run = 0, all = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    if (k < g) run += tot[k][col];
    all += tot[k][col];
  }
  if (g == 0) x.chunks[(size_t)blockIdx.x * TSREMUX_SLOTS + col] = (uint8_t)all;
  for (uint32_t t = first; t < last; t++) {
    uint8_t *p = x.tiles + (size_t)t * TSREMUX_SLOTS + col;
    const uint32_t v = *p;
    *p = (uint8_t)run;
    run += v;
  }
}

// round 2, one wave: the chunks' totals become each chunk's base, which starts at the call's start counters; the
// call's totals go to the result
__global__ __launch_bounds__(64) void tsremux_scan_chunks(TsremuxDev x, TsremuxRun y, uint32_t nchunks) {
  const uint32_t col = threadIdx.x, k = col >> 4;
  const unsigned long long w = k == 0 ? y.cc[0] : k == 1 ? y.cc[1] : k == 2 ? y.cc[2] : y.cc[3];
  const uint32_t cc0 = (uint32_t)(w >> (4 * (col & 15))) & 15u;
  uint32_t run = cc0;
  for (uint32_t c = 0; c < nchunks; c++) {
    uint8_t *p = x.chunks + (size_t)c * TSREMUX_SLOTS + col;
    const uint32_t v = *p;
    *p = (uint8_t)run;
    run += v;
  }
  x.res[TSREMUX_R_CC + col] = (run - cc0) & 255u;
}

}  // namespace

hipError_t tsmux_launch(const TsmuxDev &d, const TsmuxRun &r, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, TSMUX_R_WORDS * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  if (!r.n_out) return hipSuccess;
  const uint32_t blocks = std::min<uint32_t>(TSMUX_MAX_BLOCKS, (r.n_out + TSMUX_PKTS - 1) / TSMUX_PKTS);
  hipLaunchKernelGGL(tsmux_mux, dim3(blocks), dim3(256), 0, st, d, r);
  return hipGetLastError();
}

hipError_t tsremux_launch(const TsmuxDev &d, const TsremuxDev &x, const TsmuxRun &r, const TsremuxRun &y,
                          hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, TSMUX_R_WORDS * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(x.res, 0, TSREMUX_R_WORDS * sizeof(unsigned long long), st)) != hipSuccess) return e;
  if (!r.n_out) return hipSuccess;
  const uint32_t ntiles = (r.n_out + TSREMUX_TILE - 1) / TSREMUX_TILE;
  const uint32_t nchunks = (ntiles + TSREMUX_SCAN_TILES - 1) / TSREMUX_SCAN_TILES;
  hipLaunchKernelGGL(tsremux_classify, dim3(std::min<uint32_t>(TSMUX_MAX_BLOCKS, (ntiles + 3) / 4)), dim3(256), 0, st, d,
                     r, x);
  hipLaunchKernelGGL(tsremux_scan_tiles, dim3(nchunks), dim3(256), 0, st, x, ntiles);
  hipLaunchKernelGGL(tsremux_scan_chunks, dim3(1), dim3(64), 0, st, x, y, nchunks);
  hipLaunchKernelGGL(tsremux_emit, dim3(std::min<uint32_t>(TSMUX_MAX_BLOCKS, ntiles)), dim3(256), 0, st, d, r, x, y);
  return hipGetLastError();
}

}  // namespace t2
