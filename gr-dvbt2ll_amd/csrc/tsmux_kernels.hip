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
#include "tsmux_kernels.h"

#include <algorithm>

namespace t2 {

namespace {

constexpr uint32_t NULL_HEAD = 0x10FF1F47u;   // 47 1F FF 10
constexpr unsigned long long PCR_WRAP = (1ull << 33) * 300ull;

struct TsmuxRec {
  const uint8_t *src;    // the input packet; nullptr: a null or PCR packet made of h, w1, w2 and FF
  uint32_t h, w1, w2;    // its bytes 0 .. 11 as little-endian words
};

// bytes o .. o + 3 of a packet, o + 4 <= 188
__device__ inline uint32_t tsmux_word(const TsmuxRec &q, uint32_t o) {
  const uint32_t sh = 8 * (o & 3);
  if (!q.src) {
    const uint32_t k = o >> 2;
    const uint32_t lo = k == 0 ? q.h : k == 1 ? q.w1 : k == 2 ? q.w2 : 0xFFFFFFFFu;
    if (!sh) return lo;
    const uint32_t hi = k == 0 ? q.w1 : k == 1 ? q.w2 : 0xFFFFFFFFu;
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

__device__ inline uint32_t tsmux_byte(const TsmuxRec &q, uint32_t o) {
  if (q.src) return q.src[o];
  const uint32_t w = o < 4 ? q.h : o < 8 ? q.w1 : o < 12 ? q.w2 : 0xFFFFFFFFu;
  return (w >> (8 * (o & 3))) & 255;
}

// bytes l .. l + 3 of the trip's output (packet l / 188 of rec)
__device__ inline uint32_t tsmux_out_word(const TsmuxRec *rec, uint32_t l) {
  const uint32_t p = l / 188, o = l - p * 188;
  if (o + 4 <= 188) return tsmux_word(rec[p], o);
  uint32_t w = 0;
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t pp = (l + k) / 188, oo = l + k - pp * 188;
    w |= tsmux_byte(rec[pp], oo) << (8 * k);
  }
  return w;
}

__global__ __launch_bounds__(256) void tsmux_mux(TsmuxDev d, TsmuxRun r) {
  __shared__ TsmuxRec rec[TSMUX_PKTS];
  __shared__ uint32_t cnt[TSMUX_R_WORDS];
  __shared__ uint32_t s_w[TSMUX_OWN], s_pre0[TSMUX_OWN], s_nin[TSMUX_IN], s_next[TSMUX_IN];
  __shared__ const uint8_t *s_in[TSMUX_IN];
  if (threadIdx.x < (uint32_t)TSMUX_R_WORDS) cnt[threadIdx.x] = 0;
#pragma unroll
  for (int i = 0; i < TSMUX_OWN; i++)
    if (threadIdx.x == (uint32_t)i) {
      s_w[i] = d.w[i];
      s_pre0[i] = r.pre0[i];
    }
#pragma unroll
  for (int i = 0; i < TSMUX_IN; i++)
    if (threadIdx.x == (uint32_t)(32 + i)) {
      s_nin[i] = r.n_in[i];
      s_next[i] = r.next[i];
      s_in[i] = r.in[i];
    }
  const int n = d.n, no = d.owners, f = d.fill;
  // past TSMUX_MAX_BLOCKS x TSMUX_PKTS packets the workgroup's second trip begins at this loop's second pass
  for (uint32_t p0 = blockIdx.x * TSMUX_PKTS; p0 < r.n_out; p0 += gridDim.x * TSMUX_PKTS) {
    const uint32_t np = r.n_out - p0 < TSMUX_PKTS ? r.n_out - p0 : TSMUX_PKTS;
    __syncthreads();   // the per-owner values are in LDS; the trip before no longer reads rec
    if (threadIdx.x < np) {
      const uint32_t mm = r.phase + p0 + threadIdx.x, dc = mm / d.period, t = mm - dc * d.period;
      const int e = d.table[t];
      const uint32_t *row = d.pre + (size_t)t * no;
      // the owner's slots in this call before this one
      auto rank = [&](int x) { return dc * s_w[x] + row[x] - s_pre0[x]; };
      int src = -1;
      uint32_t idx = 0;
      bool claim = false;
      TsmuxRec q{nullptr, NULL_HEAD, 0xFFFFFFFFu, 0xFFFFFFFFu};
      if (e == n) {   // the PCR generator
        const unsigned long long T = (r.pcr_ticks + (unsigned long long)dc * d.tpp + (unsigned long long)t * d.tpp_q +
                                      (t * d.tpp_r) / d.period) % PCR_WRAP;
        const unsigned long long base = T / 300;
        const uint32_t ext = (uint32_t)(T - base * 300);
        q.h = 0x47u | ((uint32_t)(d.pcr_pid >> 8) << 8) | ((uint32_t)(d.pcr_pid & 255) << 16) | (0x20u << 24);
        q.w1 = 0xB7u | (0x10u << 8) | ((uint32_t)((base >> 25) & 255) << 16) | ((uint32_t)((base >> 17) & 255) << 24);
        q.w2 = (uint32_t)((base >> 9) & 255) | ((uint32_t)((base >> 1) & 255) << 8) |
               ((((uint32_t)(base & 1) << 7) | 0x7Eu | (ext >> 8)) << 16) | ((ext & 255u) << 24);
        atomicAdd(&cnt[TSMUX_R_PCR], 1u);
      } else if (e > n || e == f) claim = true;   // null's slot, the fill input's own
      else {
        const uint32_t rr = rank(e), ni = s_nin[e];
        if ((d.loop >> e) & 1) {
          if (ni) { src = e; idx = (s_next[e] + rr) % ni; }
          else claim = true;
        } else if (rr < ni - s_next[e]) { src = e; idx = s_next[e] + rr; }
        else claim = true;
        if (claim) atomicAdd(&cnt[TSMUX_R_DRY + e], 1u);
      }
      if (claim && f >= 0) {
        uint32_t c = rank(f) + rank(n + 1);
        for (int i = 0; i < n; i++) {
          if (i == f) continue;
          const uint32_t rr = rank(i), ni = s_nin[i], av = ni - s_next[i];
          if ((d.loop >> i) & 1) c += ni ? 0 : rr;
          else c += rr > av ? rr - av : 0;
        }
        if (c < s_nin[f] - s_next[f]) {
          src = f;
          idx = s_next[f] + c;
          if (e != f) atomicAdd(&cnt[TSMUX_R_FILL_IN_FREE], 1u);
        } else if (e == f) atomicAdd(&cnt[TSMUX_R_DRY + f], 1u);
      }
      if (src >= 0) {
        atomicAdd(&cnt[TSMUX_R_CONSUMED + src], 1u);
        const uint8_t *pk = s_in[src] + (size_t)idx * 188;
        if (pk[0] == 0x47) q.src = pk;
        else atomicAdd(&cnt[TSMUX_R_SYNC], 1u);
      }
      if (!q.src && e != n) atomicAdd(&cnt[TSMUX_R_NULL], 1u);
      rec[threadIdx.x] = q;
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
        const uint32_t w0 = tsmux_out_word(rec, lo), w1 = tsmux_out_word(rec, lo + 4);
        const uint32_t w2 = tsmux_out_word(rec, lo + 8), w3 = tsmux_out_word(rec, lo + 12);
        *(uint4 *)(out + lo) = make_uint4(w0, w1, w2, w3);
      } else {
        for (uint32_t l = lo; l < hi; l++) {
          const uint32_t p = l / 188;
          out[l] = (uint8_t)tsmux_byte(rec[p], l - p * 188);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)TSMUX_R_WORDS && cnt[threadIdx.x])
    atomicAdd(&d.res[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
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

}  // namespace t2
