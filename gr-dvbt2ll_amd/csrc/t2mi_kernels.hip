// T2-MI de-encapsulation (ETSI TS 102 773 over DVB data piping) on gfx950: a device buffer of TS packets -> per-PLP
// packed BBFRAME streams, a packet table and counters.  Semantics: include/dvbt2ll_hip.h; tests/t2mi_ref.py is the
// sequential restatement every output is compared with.
//
// The parse is parallel because every T2-MI packet start is reachable from its own TS packet (the pointer_field
// of a PUSI packet, then the length chain inside that packet's payload only).  Passes of one run, all on the
// caller's stream, sized by host-known upper bounds and cut short by counts kept on the device:
//   classify   one lane per TS packet: class, payload offset, pointer_field
//   scan A     exclusive sums of (payload length, contributing flag): stream offsets, compact indices
//   compact    per contributing packet: stream offset, buffer offset, TS index
//   starts     one lane per contributing packet: discontinuity flag; walks its starts (count, then write after scan B)
//   check      one wavefront per T2-MI packet: CRC-32 (lanes take contiguous chunks through the byte table and
//              combine by multiplying with x^(8 n) mod G), discontinuities and starts inside it, header fields
//   scan C     per-output ranks of the packets that carry a block
//   cut        the emitted prefix: first incomplete packet / output overflow / table overflow (atomicMin)
//   emit       one workgroup per emitted packet: final record, counters, the BBFRAME copy (16-byte stores where the
//              destination allows, bytes at the edges)
//   resume, count_ts   the resume position; TS-level counters of the TS packets before it
#include "t2mi_kernels.h"

#include <algorithm>

#include "crc32_mpeg2.h"
#include "dev_scan.h"
#include "host_util.h"

namespace t2 {

// found by the scan templates through argument-dependent lookup
__host__ __device__ inline T2miV8 operator+(const T2miV8 &a, const T2miV8 &b) {
  T2miV8 r;
#pragma unroll
  for (int i = 0; i < T2MI_MAX_PLP; i++) r.v[i] = a.v[i] + b.v[i];
  return r;
}

namespace {

enum : int { CTL_NC = 0, CTL_S, CTL_NS, CTL_NPTOT, CTL_NP, CTL_CUT, CTL_IEND, CTL_WORDS = 8 };
enum : uint32_t { CLS_MASK = 7, CLS_PUSI = 8, CLS_BADPTR = 1u << 24 };
enum : int { WHY_NONE = 0, WHY_OTHER_PLP = 1, WHY_LEN = 2 };

// ------------------------------------------------------------------------------------------ device-wide scan
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void t2mi_scan_reduce(const T *in, T *tile, uint32_t n,
                                                                 const uint32_t *n_dev) {
  __shared__ T lds[2 * SCAN_THREADS];
  scan_reduce_body(in, tile, n, n_dev, lds);
}
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void t2mi_scan_tiles(T *tile, uint32_t ntiles) {
  __shared__ T lds[2 * SCAN_THREADS];
  scan_tiles_body(tile, ntiles, lds);
}
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void t2mi_scan_apply(T *data, const T *tile, uint32_t n,
                                                                const uint32_t *n_dev) {
  __shared__ T lds[2 * SCAN_THREADS];
  scan_apply_body(data, tile, n, n_dev, lds);
}
template <class T>
hipError_t scan_exclusive(T *data, T *tile, uint32_t n, const uint32_t *n_dev, hipStream_t st) {
  return scan_exclusive(ScanKernels<T>{t2mi_scan_reduce<T>, t2mi_scan_tiles<T>, t2mi_scan_apply<T>}, data, tile, n, n_dev, st);
}

// ------------------------------------------------------------------------------------------ the TS layer
__global__ __launch_bounds__(256) void t2mi_classify(T2miDev d, T2miRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n) return;
  const uint8_t *b = r.ts + (size_t)(r.i0 + i) * 188;
  uint32_t cls, word = 0, plen = 0;
  const uint32_t b1 = b[1], b3 = b[3];
  const uint32_t pid = ((b1 & 0x1F) << 8) | b[2];
  if (b[0] != 0x47) cls = 5;
  else if (pid == 0x1FFF) cls = 2;
  else if (pid != (uint32_t)d.pid) cls = 1;
  else if (b1 & 0x80) cls = 3;
  else if (b3 & 0xC0) cls = 4;
  else {
    const uint32_t afc = (b3 >> 4) & 3;
    uint32_t off = afc == 1 ? 4 : afc == 3 ? 5 + b[4] : 188;
    if (off >= 188) cls = 6;
    else {
      cls = 0;
      word = (b3 & 15) << 4;
      if (b1 & 0x40) {
        const uint32_t p = b[off];
        off++;
        word |= CLS_PUSI | (p << 16);
        if (p >= 188 - off) word |= CLS_BADPTR;
      }
      plen = 188 - off;
      word |= off << 8;
    }
  }
  d.cls[i] = word | cls;
  d.scan_a[i] = cls == 0 ? ((unsigned long long)plen << 32) | 1ull : 0ull;
}

__global__ __launch_bounds__(256) void t2mi_compact(T2miDev d, T2miRun r, uint32_t ntiles_a) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long tot = d.tile_a[ntiles_a];
  const uint32_t nc = (uint32_t)tot, S = (uint32_t)(tot >> 32);
  if (i == 0) {
    d.ctl[CTL_NC] = nc;
    d.ctl[CTL_S] = S;
    d.c_base[nc] = S;
  }
  if (i >= r.n) return;
  const uint32_t w = d.cls[i];
  if ((w & CLS_MASK) != 0) return;
  const unsigned long long a = d.scan_a[i];
  const uint32_t k = (uint32_t)a;
  d.c_base[k] = (uint32_t)(a >> 32);
  d.c_off[k] = (r.i0 + i) * 188 + ((w >> 8) & 255);
  d.c_ts[k] = i;
}

// stream byte x (< the stream length) through the compact packet list; k: a compact index whose base is <= x,
// advanced to the packet holding x
__device__ inline uint32_t stream_byte(const uint8_t *ts, const uint32_t *c_base, const uint32_t *c_off, uint32_t &k,
                                       uint32_t x) {
  while (x >= c_base[k + 1]) k++;
  return ts[c_off[k] + (x - c_base[k])];
}

// the compact packet holding stream byte x >= c_base[k]: no payload is longer than 184 bytes, so the packet
// (x - c_base[k]) / 184 after k starts at or before x
__device__ inline uint32_t locate(const uint32_t *c_base, uint32_t k, uint32_t x) {
  uint32_t kk = k + (x - c_base[k]) / 184;
  while (x >= c_base[kk + 1]) kk++;
  return kk;
}

// WRITE false: discontinuity flags and the number of starts per contributing packet; true (after the scan of those
// numbers): the start list
template <bool WRITE>
__global__ __launch_bounds__(256) void t2mi_starts(T2miDev d, T2miRun r, uint32_t ntiles_b) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  const uint32_t nc = d.ctl[CTL_NC], S = d.ctl[CTL_S];
  if (WRITE && k == 0) {
    const uint32_t ns = d.tile_b[ntiles_b];
    const uint32_t tot = ns > r.skip ? ns - r.skip : 0;
    d.ctl[CTL_NS] = ns;
    d.ctl[CTL_NPTOT] = tot;
    d.ctl[CTL_NP] = min(tot, d.max_packets);
    d.ctl[CTL_CUT] = min(tot, d.max_packets);
  }
  if (k >= r.n) return;
  if (k >= nc) {
    if (!WRITE) d.nst[k] = 0;
    return;
  }
  const uint32_t w = d.cls[d.c_ts[k]];
  if (!WRITE) {
    uint32_t disc = 0;
    if (k > 0) disc = ((w >> 4) & 15) != ((((d.cls[d.c_ts[k - 1]] >> 4) & 15) + 1) & 15);
    d.c_disc[k] = (uint8_t)disc;
  }
  uint32_t count = 0;
  if ((w & CLS_PUSI) && !(w & CLS_BADPTR)) {
    const uint32_t end = d.c_base[k + 1];
    const uint32_t g0 = WRITE ? d.nst[k] : 0;
    uint32_t s = d.c_base[k] + ((w >> 16) & 255);
    for (;;) {
      uint32_t T = 0;
      if (s + 6 <= S) {
        uint32_t kk = k;
        const uint32_t hi = stream_byte(r.ts, d.c_base, d.c_off, kk, s + 4);
        const uint32_t lo = stream_byte(r.ts, d.c_base, d.c_off, kk, s + 5);
        T = 10 + (((hi << 8) | lo) + 7) / 8;
      }
      if (WRITE) {
        const uint32_t g = g0 + count;
        if (g >= r.skip && g - r.skip <= d.max_packets) {   // one past the table: the next start of its last packet
          d.pk_s[g - r.skip] = s;
          d.pk_k[g - r.skip] = k;
          d.pk_T[g - r.skip] = T;
        }
      }
      count++;
      if (T == 0 || s + T >= end) break;
      s += T;
    }
  }
  if (!WRITE) d.nst[k] = count;
}

// ------------------------------------------------------------------------------------------ the T2-MI layer
__global__ __launch_bounds__(256) void t2mi_check(T2miDev d, T2miRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t *xp = d.tab + 256;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nw = gridDim.x * 4;
  const uint32_t np = d.ctl[CTL_NP], nptot = d.ctl[CTL_NPTOT], nc = d.ctl[CTL_NC], S = d.ctl[CTL_S];
  for (uint32_t j = blockIdx.x * 4 + (threadIdx.x >> 6); j < np; j += nw) {
    const uint32_t s = d.pk_s[j], k = d.pk_k[j], T = d.pk_T[j];
    if (T == 0 || s + T > S) {   // incomplete: the emitted prefix ends before it
      if (lane == 0) {
        atomicMin(&d.ctl[CTL_CUT], j);
        d.cand[j] = T2miV8{};
      }
      continue;
    }
    // CRC over all T bytes (0 when the trailing CRC matches): a chunk per lane, joined
    int lo, hi;
    const uint32_t c = crc32m_wave_chunk(lane, T, lo, hi);
    uint32_t crc = 0;
    if (hi > lo) {
      uint32_t x = s + lo;
      const uint32_t xe = s + hi;
      uint32_t kk = locate(d.c_base, k, x);
      while (x < xe) {
        const uint32_t seg_end = min(xe, d.c_base[kk + 1]);
        crc = crc32m_run(crc, r.ts + d.c_off[kk] + (x - d.c_base[kk]), seg_end - x, tab);
        x = seg_end;
        kk++;
      }
    }
    crc = crc32m_wave_join(crc, lane, c, T, xp);
    // a discontinuity inside the packet: at a contributing TS packet after k that begins before s + T
    int bad = 0;
    for (uint32_t kk = k + 1 + lane; kk < nc && d.c_base[kk] < s + T; kk += 64) bad |= d.c_disc[kk];
    bad = __any(bad);
    if (lane == 0) {
      if (j + 1 < nptot && d.pk_s[j + 1] < s + T) bad = 1;   // another start inside it
      uint32_t kk = k, h[9];
      for (int q = 0; q < 9; q++) h[q] = stream_byte(r.ts, d.c_base, d.c_off, kk, s + q);   // T >= 10
      T2miRec rec;
      rec.ts_index = r.i0 + d.c_ts[k];
      rec.ts_byte = d.c_off[k] + (s - d.c_base[k]);
      rec.type = (uint8_t)h[0];
      rec.count = (uint8_t)h[1];
      rec.sf_idx = (uint8_t)(h[2] >> 4);
      rec.stream_id = (uint8_t)(h[3] & 7);
      const uint32_t plen = (h[4] << 8) | h[5];
      rec.payload_len = (uint16_t)plen;
      const bool consistent = !bad, crc_ok = crc == 0;
      const bool accepted = consistent && crc_ok && (d.stream_id < 0 || (int)rec.stream_id == d.stream_id);
      rec.flags = (uint8_t)(1 | (consistent ? 2 : 0) | (crc_ok ? 4 : 0) | (accepted ? 8 : 0));
      const bool bbf = rec.type == 0 && plen >= 24;
      rec.frame_idx = bbf ? (uint8_t)h[6] : 0;
      rec.plp_id = bbf ? (uint8_t)h[7] : 0;
      rec.ifs = bbf ? (uint8_t)(h[8] >> 7) : 0;
      rec.out = -1;
      rec.why = WHY_NONE;
      rec.block = -1;
      T2miV8 cand{};
      if (accepted && rec.type == 0) {
        int o = -1;
        if (bbf)
          for (int q = 0; q < d.nplp; q++)
            if (d.plp_id[q] == (int)h[7]) o = q;
        if (o < 0) rec.why = WHY_OTHER_PLP;
        else if (plen != 24u + 8u * (uint32_t)d.L[o]) rec.why = WHY_LEN;
        else {
          rec.out = (int8_t)o;
          cand.v[o] = 1;
        }
      }
      d.table[j] = rec;
      d.cand[j] = cand;
    }
  }
}

__global__ __launch_bounds__(256) void t2mi_cut(T2miDev d, T2miRun r) {
  const uint32_t np = d.ctl[CTL_NP];
  for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < np; j += gridDim.x * 256) {
    if (d.pk_T[j] == 0 || d.pk_s[j] + d.pk_T[j] > d.ctl[CTL_S]) continue;   // incomplete: no record
    const int o = d.table[j].out;
    if (o >= 0 && d.cand[j].v[o] >= r.cap[o]) atomicMin(&d.ctl[CTL_CUT], j);
  }
}

constexpr int EMIT_HIST = 6 + 256;
__global__ __launch_bounds__(256) void t2mi_emit(T2miDev d, T2miRun r) {
  __shared__ uint32_t hist[EMIT_HIST];
  for (int q = threadIdx.x; q < EMIT_HIST; q += 256) hist[q] = 0;
  __syncthreads();
  const uint32_t cut = d.ctl[CTL_CUT];
  for (uint32_t j = blockIdx.x; j < cut; j += gridDim.x) {
    const int o = d.table[j].out;   // the one field this pass never writes (thread 0 below rewrites why / block)
    const uint32_t rank = o >= 0 ? d.cand[j].v[o] : 0;
    if (threadIdx.x == 0) {
      const T2miRec rec = d.table[j];
      const int what = !(rec.flags & 2) ? 0 : !(rec.flags & 4) ? 1 : !(rec.flags & 8) ? 2
                       : rec.why == WHY_LEN ? 3 : rec.why == WHY_OTHER_PLP ? 4 : -1;
      if (what >= 0) atomicAdd(&hist[what], 1u);
      if (rec.flags & 8) atomicAdd(&hist[5], 1u);
      atomicAdd(&hist[6 + rec.type], 1u);
      d.table[j].why = 0;
      if (o >= 0) d.table[j].block = (int32_t)rank;
    }
    if (o < 0 || rank >= r.cap[o]) continue;   // rank < cap below the cut; the test keeps a wild rank off the output
    // block `rank` of output o: L bytes from stream offset s + 9.  Chunk 0 runs up to the first 16-byte boundary
    // of the destination, the others are 16 bytes (the last one shorter)
    const uint32_t L = (uint32_t)d.L[o], k = d.pk_k[j], src = d.pk_s[j] + 9;
    uint8_t *dst = r.out[o] + (size_t)rank * L;
    const uint32_t head = min(L, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    const uint32_t nchunks = 1 + (L - head + 15) / 16;
    for (uint32_t cidx = threadIdx.x; cidx < nchunks; cidx += 256) {
      const uint32_t lo = cidx ? head + (cidx - 1) * 16 : 0;
      const uint32_t hi = cidx ? min(L, lo + 16) : head;
      if (hi <= lo) continue;
      uint32_t kk = locate(d.c_base, k, src + lo);
      if (hi - lo == 16 && cidx) {
        uint32_t w[4] = {0, 0, 0, 0};
        for (uint32_t q = 0; q < 16; q++)
          w[q >> 2] |= stream_byte(r.ts, d.c_base, d.c_off, kk, src + lo + q) << (8 * (q & 3));
        *(uint4 *)(dst + lo) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (uint32_t q = lo; q < hi; q++) dst[q] = (uint8_t)stream_byte(r.ts, d.c_base, d.c_off, kk, src + q);
      }
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < EMIT_HIST; q += 256)
    if (hist[q]) atomicAdd(&d.res[q < 6 ? T2MI_R_PKT + q : T2MI_R_TYPE + (q - 6)], (unsigned long long)hist[q]);
}

__global__ void t2mi_resume(T2miDev d, T2miRun r, uint32_t ntiles_c) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t cut = d.ctl[CTL_CUT], np = d.ctl[CTL_NP], nptot = d.ctl[CTL_NPTOT];
  uint32_t iend = r.n;
  unsigned long long off = (unsigned long long)(r.i0 + r.n) * 188, skip = 0;
  if (r.n == 0) skip = r.skip;   // nothing to look at: the position stands
  if (cut < nptot) {
    const uint32_t k = d.pk_k[cut];
    iend = d.c_ts[k];
    off = (unsigned long long)(r.i0 + iend) * 188;
    skip = cut + r.skip - d.nst[k];
  }
  d.ctl[CTL_IEND] = iend;
  d.res[T2MI_R_OFFSET] = off;
  d.res[T2MI_R_SKIP] = skip;
  d.res[T2MI_R_PACKETS] = cut;
  const T2miV8 b = cut < np ? d.cand[cut] : d.tile_c[ntiles_c];
  for (int o = 0; o < T2MI_MAX_PLP; o++) d.res[T2MI_R_BLOCKS + o] = o < d.nplp ? b.v[o] : 0;
}

__global__ __launch_bounds__(256) void t2mi_count_ts(T2miDev d, T2miRun r) {
  __shared__ uint32_t hist[9];
  if (threadIdx.x < 9) hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t iend = d.ctl[CTL_IEND];
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < iend; i += gridDim.x * 256) {
    const uint32_t w = d.cls[i];
    atomicAdd(&hist[w & CLS_MASK], 1u);
    if ((w & CLS_MASK) == 0) {
      if (d.c_disc[(uint32_t)d.scan_a[i]]) atomicAdd(&hist[7], 1u);
      if (w & CLS_BADPTR) atomicAdd(&hist[8], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < 9 && hist[threadIdx.x])
    atomicAdd(&d.res[T2MI_R_TS + threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

}  // namespace

void t2mi_host_tables(uint32_t *tab) {
  crc32m_host_tables(tab, T2MI_MAX_T + 1);
}

size_t t2mi_layout(T2miDev &d, void *base) {
  LayoutTaker take{base};
  const size_t n = d.max_ts, mp = d.max_packets;
  take(d.res, T2MI_R_WORDS + CTL_WORDS);   // ctl follows res: one memset clears both
  d.ctl = base ? (uint32_t *)(d.res + T2MI_R_WORDS) : nullptr;
  take(d.cls, n);
  take(d.scan_a, n);
  take(d.tile_a, scan_tiles_of((uint32_t)n) + 1);
  take(d.c_base, n + 1);
  take(d.c_off, n);
  take(d.c_ts, n);
  take(d.c_disc, n);
  take(d.nst, n);
  take(d.tile_b, scan_tiles_of((uint32_t)n) + 1);
  take(d.pk_s, mp + 1);
  take(d.pk_k, mp + 1);
  take(d.pk_T, mp + 1);
  take(d.cand, mp);
  take(d.tile_c, scan_tiles_of((uint32_t)mp) + 1);
  take(d.table, mp);
  take(d.tab, T2MI_TAB_WORDS);
  return take.at;
}

hipError_t t2mi_launch(const T2miDev &d, const T2miRun &r, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, (T2MI_R_WORDS + CTL_WORDS) * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const uint32_t nb = std::max<uint32_t>(1, (r.n + 255) / 256);
  const uint32_t nta = scan_tiles_of(r.n), ntc = scan_tiles_of(d.max_packets);
  hipLaunchKernelGGL(t2mi_classify, dim3(nb), dim3(256), 0, st, d, r);
  if ((e = scan_exclusive(d.scan_a, d.tile_a, r.n, nullptr, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(t2mi_compact, dim3(nb), dim3(256), 0, st, d, r, nta);
  hipLaunchKernelGGL(t2mi_starts<false>, dim3(nb), dim3(256), 0, st, d, r, nta);
  if ((e = scan_exclusive(d.nst, d.tile_b, r.n, nullptr, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(t2mi_starts<true>, dim3(nb), dim3(256), 0, st, d, r, nta);
  hipLaunchKernelGGL(t2mi_check, dim3(blocks_for(d.max_packets, 4, 4096)), dim3(256), 0, st, d, r);
  if ((e = scan_exclusive(d.cand, d.tile_c, d.max_packets, d.ctl + CTL_NP, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(t2mi_cut, dim3(blocks_for(d.max_packets, 256, 1024)), dim3(256), 0, st, d, r);
  hipLaunchKernelGGL(t2mi_emit, dim3(blocks_for(d.max_packets, 1, 4096)), dim3(256), 0, st, d, r);
  hipLaunchKernelGGL(t2mi_resume, dim3(1), dim3(64), 0, st, d, r, ntc);
  hipLaunchKernelGGL(t2mi_count_ts, dim3(blocks_for(r.n, 256, 1024)), dim3(256), 0, st, d, r);
  return hipGetLastError();
}

}  // namespace t2
