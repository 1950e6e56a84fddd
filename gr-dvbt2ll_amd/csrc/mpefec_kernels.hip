// MPE-FEC encapsulation (this project's reading of EN 301 192 clause 9) on gfx950: a device buffer of IP datagrams and
// an offset table -> per closed frame its MPE sections, then Reed-Solomon columns in MPE-FEC sections, in 188-byte TS
// packets.  Semantics: include/dvbt2ll_hip.h; tests/mpefec_ref.py is the sequential restatement every output is
// compared with.  The units ts_section_packer.h packs are a list of sections (items) of two kinds, closed as the MPE
// handle's (MINFREE 1).  Passes of one run, all on the caller's stream:
//   measure    a lane per PDU: validity, the MAC's two header bytes, the length p; (p << 25 | 1) for the sum scan
//   sum scan   64-bit (dev_scan.h): before each PDU the valid bytes and the valid PDUs of the call
//   next       a lane per PDU: where a frame that begins here would end (two binary searches in the sums), and whether
//              the call closes it
//   chain      one lane follows the frames from the start, up to max_frames of them; it also settles the start's
//              section / section_byte and the number of items
//   items      a lane per PDU and a lane per RS column: the section's length, source, header words (RT included)
//   gather     a lane per 4 bytes of the frames' tables (the first D columns; zero behind the datagrams)
//   rs         a workgroup per 256 rows of a frame, a lane per row: the row's 64 parity bytes live in 16 VGPRs; per
//              symbol the feedback byte picks a 64-byte row of a 16 KiB LDS table (128-bit reads) that is added to the
//              parities shifted by one byte
//   maps, compose, walk   the packer's state scan over the items (packing 0 runs it with a step that starts every
//              section in a packet of its own)
//   crc        MPE sections of up to CRC_LANE_MAX bytes a lane each; longer ones and every MPE-FEC section a wavefront
//   emit       the packer's
//   count      the resume position, and the counters of the frames wholly sent
// A closed frame past max_frames is computed as well (the lookahead frame): its sections decide the packet in which
// the frame before it ends, and no packet that begins behind that frame's last byte is emitted.
#include "mpefec_kernels.h"

#include <algorithm>

#include "crc32_mpeg2.h"
#include "dev_scan.h"
#include "host_util.h"
#include "ts_section_packer.h"

namespace t2 {

namespace {

typedef unsigned long long u64;

enum : uint32_t { M_LEN = PK_LEN, M_MAPPED = 1u << 29, M_SKIP_TYPE = 1u << 30, M_SKIP_LEN = 1u << 31 };
enum : uint32_t { I_FEC = 1u << 31 };
// d.ctl: packets completed, the end state, the start's section_byte as taken, long sections, frames computed (the
// lookahead frame included), frames the call may send (0: no lookahead frame, all of them), the start's section as
// taken, items, where what is left begins
enum : int { C_T = 0, C_Q, C_S, C_NLONG, C_F, C_LOOK, C_IS, C_NI, C_REST };
constexpr int KEY_SHIFT = 25;                     // the sums' low bits count the valid PDUs (up to 2^24)
constexpr u64 KEY_COUNT = (1ull << KEY_SHIFT) - 1;
static_assert(MF_MAP_STATES == PK_STATES && MF_TILE == PK_TILE, "the layout is sized for the packer's maps");
constexpr int MINFREE = 1;
constexpr uint32_t CRC_LANE_MAX = 192;
constexpr uint32_t HL = MF_HEADER;
constexpr uint32_t COUNT_BLOCKS = 64;
constexpr uint32_t RS_ROWS = 256;                 // rows (lanes) per workgroup of the RS pass

__device__ inline uint32_t cnt_of(u64 k) { return (uint32_t)(k & KEY_COUNT); }
__device__ inline u64 sum_of(u64 k) { return k >> KEY_SHIFT; }

__global__ __launch_bounds__(SCAN_THREADS) void mf_scan_reduce(const u64 *in, u64 *tile, uint32_t n, const uint32_t *n_dev) {
  __shared__ u64 lds[SCAN_THREADS];
  scan_reduce_body(in, tile, n, n_dev, lds);
}
__global__ __launch_bounds__(SCAN_THREADS) void mf_scan_tiles(u64 *tile, uint32_t ntiles) {
  __shared__ u64 lds[2 * SCAN_THREADS];
  scan_tiles_body(tile, ntiles, lds);
}
__global__ __launch_bounds__(SCAN_THREADS) void mf_scan_apply(u64 *data, const u64 *tile, uint32_t n, const uint32_t *n_dev) {
  __shared__ u64 lds[2 * SCAN_THREADS];
  scan_apply_body(data, tile, n, n_dev, lds);
}
constexpr ScanKernels<u64> MF_SCAN{mf_scan_reduce, mf_scan_tiles, mf_scan_apply};

uint32_t state_tiles_of(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, (n + PK_TILE - 1) / PK_TILE); }
// the items, as the control words count them
__device__ inline PkUnits mf_units(const MfDev &d) { return PkUnits{d.ilen, d.pkt, d.at, d.ctl[C_NI]}; }

// ------------------------------------------------------------------------------------------ measure
// lanes 0 .. n: lane n writes the sums' last entry only
__global__ __launch_bounds__(256) void mf_measure(MfDev d, MfRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i > r.n) return;
  if (i == r.n) { d.pre[i] = 0; return; }
  const uint32_t o0 = r.off[r.i0 + i], o1 = r.off[r.i0 + i + 1];
  const uint32_t C = d.D * d.rows, pmax = C < (uint32_t)MF_MAX_PDU ? C : (uint32_t)MF_MAX_PDU;
  uint32_t p = 0, flags = 0;
  uint32_t m4 = d.mac[4], m5 = d.mac[5];
  if (o1 <= o0 || o1 > r.pdu_len || o1 - o0 > pmax) flags = M_SKIP_LEN;
  else {
    const uint8_t *b = r.pdu + o0;
    const uint32_t nib = b[0] >> 4;
    if (nib != 4 && nib != 6) flags = M_SKIP_TYPE;
    else {
      p = o1 - o0;
      if (d.mac_mode) {   // a multicast destination gives its own MAC (RFC 1112 / RFC 2464)
        if (nib == 4 && p >= 20 && b[16] >= 224 && b[16] <= 239) { m4 = b[18]; m5 = b[19]; flags = M_MAPPED; }
        else if (nib == 6 && p >= 40 && b[24] == 0xFF) { m4 = b[38]; m5 = b[39]; flags = M_MAPPED; }
      }
    }
  }
  d.len[i] = p | flags;
  d.macw[i] = m5 | (m4 << 8);
  d.pre[i] = p ? ((u64)p << KEY_SHIFT) | 1 : 0;
}

// ------------------------------------------------------------------------------------------ frames
// the first index in (lo, hi] whose sum exceeds limit, or hi + 1
__device__ inline uint32_t first_above(const u64 *pre, uint32_t lo, uint32_t hi, u64 limit) {
  uint32_t a = lo + 1, b = hi + 1;
  while (a < b) {
    const uint32_t mid = (a + b) >> 1;
    if (sum_of(pre[mid]) > limit) b = mid;
    else a = mid + 1;
  }
  return a;
}

// a frame that begins at PDU i takes the valid PDUs up to jm - 1, the last index whose sum stays within C; it ends
// just behind the last valid one of them: the first index whose sum is that of jm
__global__ __launch_bounds__(256) void mf_next(MfDev d, MfRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n) return;
  const u64 base = sum_of(d.pre[i]), C = (u64)d.D * d.rows;
  const uint32_t jm = first_above(d.pre, i, r.n, base + C) - 1;   // i <= jm <= n
  const u64 top = sum_of(d.pre[jm]);
  uint32_t e = i;
  if (top > base) e = first_above(d.pre, i, jm, top - 1);         // the first index with the whole sum: <= jm
  const bool closed = e > i && (jm < r.n || r.flush);
  d.end[i] = e | (closed ? 1u << 31 : 0);
}

// the first index in [lo, n) whose count of valid PDUs before it is above c: behind the (c + 1)-th valid PDU
__device__ inline uint32_t first_count_above(const u64 *pre, uint32_t lo, uint32_t n, uint32_t c) {
  uint32_t a = lo, b = n;
  while (a < b) {
    const uint32_t mid = (a + b) >> 1;
    if (cnt_of(pre[mid]) > c) b = mid;
    else a = mid + 1;
  }
  return a;
}

__global__ void mf_chain(MfDev d, MfRun r) {
  if (blockIdx.x || threadIdx.x) return;
  uint32_t s = 0, F = 0;
  while (F < d.max_frames + 1 && s < r.n) {
    const uint32_t v = d.end[s];
    if (!(v >> 31)) break;
    d.fs[F++] = s;
    s = v & 0x7FFFFFFFu;
  }
  d.fs[F] = s;
  const uint32_t look = F > d.max_frames ? d.max_frames : 0;
  uint32_t sec = 0, sb = 0, items = 0;
  if (F) {
    const uint32_t m0 = cnt_of(d.pre[d.fs[1]]);
    sec = r.section;
    sb = r.section_byte;
    if (sec >= m0 + d.K) sec = sb = 0;           // inconsistent: taken as 0
    uint32_t n = d.rows + 16;
    if (sec < m0) {
      const uint32_t j = first_count_above(d.pre, 0, r.n, sec) - 1;   // the PDU of frame 0's section sec
      n = (d.len[j] & M_LEN) + 16;
    }
    if (sb >= n) sb = 0;
    items = cnt_of(d.pre[s]) + F * d.K - sec;
  }
  d.ctl[C_F] = F;
  d.ctl[C_LOOK] = look;
  d.ctl[C_IS] = sec;
  d.ctl[C_S] = sb;
  d.ctl[C_NI] = items;
  d.ctl[C_REST] = d.pre[r.n] > d.pre[s] ? s : r.n;
}

// the frame (0 .. F) whose first index is the last at or before i
__device__ inline uint32_t frame_of_pdu(const uint32_t *fs, uint32_t F, uint32_t i) {
  uint32_t a = 0, b = F;
  while (a < b) {
    const uint32_t mid = (a + b + 1) >> 1;
    if (fs[mid] <= i) a = mid;
    else b = mid - 1;
  }
  return a;
}

// the sections a wavefront's lanes list for the CRC pass: one atomic per wavefront
__device__ inline void list_long(const MfDev &d, bool lng, uint32_t x) {
  const unsigned long long m = __ballot(lng);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == (uint32_t)(__ffsll((long long)m) - 1)) base = atomicAdd(&d.ctl[C_NLONG], (uint32_t)__popcll(m));
  base = __shfl(base, __ffsll((long long)m) - 1);
  if (lng) d.lng[base + __popcll(m & ((1ull << lane) - 1))] = x;
}

__device__ inline uint32_t rt_word_be(uint32_t delta_t, uint32_t tb, uint32_t fb, uint32_t address) {
  const uint32_t rt = ((delta_t & 0xFFFu) << 20) | (tb << 19) | (fb << 18) | address;
  return __builtin_bswap32(rt);   // big-endian in bytes 8 .. 11: the little-endian word's byte 0 is RT's top byte
}

__global__ __launch_bounds__(256) void mf_items_mpe(MfDev d, MfRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t F = d.ctl[C_F], is = d.ctl[C_IS];
  bool take = false, lng = false;
  uint32_t x = 0;
  if (i < r.n && F) {
    const uint32_t w = d.len[i], p = w & M_LEN;
    const uint32_t f = frame_of_pdu(d.fs, F, i);
    const u64 k0 = d.pre[d.fs[f]], ki = d.pre[i];
    const uint32_t j = cnt_of(ki) - cnt_of(k0);
    const uint32_t m = p && f < F ? cnt_of(d.pre[d.fs[f + 1]]) - cnt_of(k0) : 0;   // 0: no section of the call
    const uint32_t seq = cnt_of(ki) + f * d.K;   // in the call's section sequence, from frame 0's section 0
    if (m && seq >= is) {
      x = seq - is;
      take = true;
      const uint32_t n = p + 16, sl = n - 3, mw = d.macw[i];
      d.ilen[x] = n;
      d.isrc[x] = i;
      d.ihdr[3 * (size_t)x] = 0x3Eu | ((0xB0u | (sl >> 8)) << 8) | ((sl & 255u) << 16) | ((mw & 255u) << 24);
      d.ihdr[3 * (size_t)x + 1] = (mw >> 8) | (0xC1u << 8);
      d.ihdr[3 * (size_t)x + 2] = rt_word_be(r.frame + f, j == m - 1, 0, (uint32_t)(sum_of(ki) - sum_of(k0)));
      lng = n > CRC_LANE_MAX;
    }
  }
  list_long(d, take && lng, x);
}

// a lane per RS column of a frame; past the grid a lane takes more than one
__global__ __launch_bounds__(256) void mf_items_fec(MfDev d, MfRun r) {
  const uint32_t F = d.ctl[C_F], is = d.ctl[C_IS], total = F * d.K;
  const uint32_t rounds = (total + gridDim.x * 256 - 1) / (gridDim.x * 256);
  for (uint32_t t = 0; t < rounds; t++) {
    const uint32_t g = (t * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    bool take = false;
    uint32_t x = 0;
    if (g < total) {
      const uint32_t f = g / d.K, k = g - f * d.K;
      const u64 k0 = d.pre[d.fs[f]], k1 = d.pre[d.fs[f + 1]];
      const uint32_t seq = cnt_of(k1) + f * d.K + k;
      if (seq >= is) {
        x = seq - is;
        take = true;
        const uint32_t U = (uint32_t)(sum_of(k1) - sum_of(k0)), L = d.rows + 13, last = k == d.K - 1;
        d.ilen[x] = (d.rows + 16) | I_FEC;
        d.isrc[x] = g;
        d.ihdr[3 * (size_t)x] = 0x78u | ((0xB0u | (L >> 8)) << 8) | ((L & 255u) << 16) |
                                ((191u - (U + d.rows - 1) / d.rows) << 24);
        d.ihdr[3 * (size_t)x + 1] = 0xFFu | (0xFFu << 8) | (k << 16) | ((d.K - 1) << 24);
        d.ihdr[3 * (size_t)x + 2] = rt_word_be(r.frame + f, last, last, k * d.rows);
      }
    }
    list_long(d, take, x);
  }
}

// ------------------------------------------------------------------------------------------ the tables, Reed-Solomon
// a lane per 4 bytes of the frames' first D columns: address a of frame f is byte sum(first index) + a of the valid
// PDUs laid end to end
__global__ __launch_bounds__(256) void mf_gather(MfDev d, MfRun r) {
  const uint32_t F = d.ctl[C_F], wpf = d.D * d.rows / 4;
  const u64 total = (u64)F * wpf;
  for (u64 g = (u64)blockIdx.x * 256 + threadIdx.x; g < total; g += (u64)gridDim.x * 256) {
    const uint32_t f = (uint32_t)(g / wpf), a = (uint32_t)(g - (u64)f * wpf) * 4;
    const uint32_t s = d.fs[f], e = d.fs[f + 1];
    const u64 b0 = sum_of(d.pre[s]);
    const uint32_t U = (uint32_t)(sum_of(d.pre[e]) - b0);
    uint32_t w = 0;
    if (a < U) {
      uint32_t i = first_above(d.pre, s, e, b0 + a) - 1;   // the valid PDU that holds address a: s <= i < e
      u64 lo = sum_of(d.pre[i]), hi = sum_of(d.pre[i + 1]);
      const uint8_t *src = r.pdu + r.off[r.i0 + i];
      for (uint32_t q = 0; q < 4 && a + q < U; q++) {
        const u64 at = b0 + a + q;
        while (at >= hi) {                                 // at < the frame's last sum: i + 1 stays at or below e
          i++;
          lo = hi;
          hi = sum_of(d.pre[i + 1]);
          src = r.pdu + r.off[r.i0 + i];
        }
        w |= (uint32_t)src[at - lo] << (8 * q);
      }
    }
    *(uint32_t *)(d.tbl + (size_t)f * d.D * d.rows + a) = w;
  }
}

// par <- par x + (d + par_0) (g_63 .. g_0): the bytes move down by one, the table's row for the feedback symbol is added
__device__ inline void rs_step(uint32_t (&p)[16], uint32_t sym, const uint4 *T) {
  const uint32_t fb = (sym ^ p[0]) & 255u;
  const uint4 t0 = T[4 * fb], t1 = T[4 * fb + 1], t2 = T[4 * fb + 2], t3 = T[4 * fb + 3];
  const uint32_t t[16] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w, t3.x, t3.y, t3.z, t3.w};
#pragma unroll
  for (int k = 0; k < 15; k++) p[k] = ((p[k] >> 8) | (p[k + 1] << 24)) ^ t[k];
  p[15] = (p[15] >> 8) ^ t[15];
}

// the grid covers the frames that PDUs lying side by side can make; with more a workgroup takes several
__global__ __launch_bounds__(RS_ROWS) void mf_rs(MfDev d) {
  __shared__ uint4 T[MF_RS_WORDS / 4];
  for (uint32_t k = threadIdx.x; k < (uint32_t)MF_RS_WORDS / 4; k += RS_ROWS) T[k] = ((const uint4 *)d.rstab)[k];
  __syncthreads();
  const uint32_t F = d.ctl[C_F], rb = d.rows / RS_ROWS, rows = d.rows, D = d.D, K = d.K;
  for (uint32_t wk = blockIdx.x; wk < F * rb; wk += gridDim.x) {
    const uint32_t f = wk / rb, row = (wk - f * rb) * RS_ROWS + threadIdx.x;
    const uint8_t *src = d.tbl + (size_t)f * D * rows + row;
    uint32_t p[16];
#pragma unroll
    for (int k = 0; k < 16; k++) p[k] = 0;
    uint32_t c = 0;
    for (; c + 4 <= D; c += 4) {   // four columns' symbols are fetched before they are used
      const uint32_t s0 = src[(size_t)c * rows], s1 = src[(size_t)(c + 1) * rows], s2 = src[(size_t)(c + 2) * rows],
                     s3 = src[(size_t)(c + 3) * rows];
      rs_step(p, s0, T);
      rs_step(p, s1, T);
      rs_step(p, s2, T);
      rs_step(p, s3, T);
    }
    for (; c < D; c++) rs_step(p, src[(size_t)c * rows], T);
    for (; c < (uint32_t)MF_DATA_COLS; c++) rs_step(p, 0, T);   // the columns no frame may fill
    uint8_t *dst = d.par + (size_t)f * K * rows + row;
#pragma unroll
    for (int k = 0; k < MF_RS_COLS; k++)
      if ((uint32_t)k < K) dst[(size_t)k * rows] = (uint8_t)(p[k >> 2] >> (8 * (k & 3)));
  }
}

// ------------------------------------------------------------------------------------------ the state scan
__global__ __launch_bounds__(PK_THREADS) void mf_maps(MfDev d) {
  const uint32_t N = d.ctl[C_NI];
  if (blockIdx.x * PK_TILE >= N) return;
  pk_maps_body<MINFREE>(d.ilen, N, d.ctl[C_S], d.packing, d.maps);
}

__global__ __launch_bounds__(PK_COMPOSE_THREADS) void mf_compose(MfDev d) {
  pk_compose_body(d.maps, (d.ctl[C_NI] + PK_TILE - 1) / PK_TILE, d.ent_q, d.ent_pk, &d.ctl[C_T], &d.ctl[C_Q]);
}

__global__ __launch_bounds__(PK_THREADS) void mf_walk(MfDev d) {
  const PkUnits u = mf_units(d);
  if (blockIdx.x * PK_TILE >= u.N) return;
  pk_walk_body<MINFREE>(u, d.ctl[C_S], d.packing, d.ent_q, d.ent_pk);
}

// ------------------------------------------------------------------------------------------ section bytes
__device__ inline uint32_t mf_header_byte(const uint32_t *h, uint32_t k) { return (h[k >> 2] >> (8 * (k & 3))) & 255; }

// what lies behind item x's header: a datagram in the PDU buffer, or an RS column in the parity scratch
__device__ inline const uint8_t *mf_payload(const MfDev &d, const MfRun &r, uint32_t x) {
  return (d.ilen[x] & I_FEC) ? d.par + (size_t)d.isrc[x] * d.rows : r.pdu + r.off[r.i0 + d.isrc[x]];
}

// the packer's source of section bytes
struct MfSrc {
  const MfDev &d;
  const MfRun &r;
  __device__ uint32_t byte(uint32_t j, uint32_t k) const {
    const uint32_t n = d.ilen[j] & M_LEN;
    if (k < HL) return mf_header_byte(d.ihdr + 3 * (size_t)j, k);
    if (k + 4 < n) return mf_payload(d, r, j)[k - HL];
    return (d.icrc[j] >> (8 * (n - 1 - k))) & 255;
  }
  // bytes k .. k + 3 of item j's section (all inside it): a header word; a word of the payload's buffer where all four
  // are payload bytes; bytes otherwise
  __device__ uint32_t word(uint32_t j, uint32_t k) const {
    const uint32_t w0 = d.ilen[j], n = w0 & M_LEN;
    uint32_t w = 0;
    if (k < HL && (k & 3) == 0) return d.ihdr[3 * (size_t)j + (k >> 2)];
    if (k >= HL && k + 8 <= n) {
      const uint8_t *lo = (w0 & I_FEC) ? d.par : r.pdu;
      const uint8_t *hi = (w0 & I_FEC) ? d.par + (size_t)d.ctl[C_F] * d.K * d.rows : r.pdu + r.pdu_len;
      if (pk_read4(mf_payload(d, r, j) + (k - HL), lo, hi, w)) return w;
    }
    for (uint32_t q = 0; q < 4; q++) w |= byte(j, k + q) << (8 * q);
    return w;
  }
};

// ------------------------------------------------------------------------------------------ CRC-32
// section bytes [lo, hi) of a section (hi <= n - 4): the header's (words h), then the payload's
__device__ inline uint32_t crc_span(uint32_t crc, const uint32_t *h, const uint8_t *pay, uint32_t lo, uint32_t hi,
                                    const uint32_t *tab) {
  for (; lo < hi && lo < HL; lo++) crc = crc32m_byte(crc, mf_header_byte(h, lo), tab);
  if (lo < hi) crc = crc32m_run(crc, pay + (lo - HL), hi - lo, tab);
  return crc;
}

__global__ __launch_bounds__(256) void mf_crc_short(MfDev d, MfRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t N = d.ctl[C_NI];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t n = i < N ? d.ilen[i] & M_LEN : 0;
  if (n && n <= CRC_LANE_MAX) d.icrc[i] = crc_span(0xFFFFFFFFu, d.ihdr + 3 * (size_t)i, mf_payload(d, r, i), 0, n - 4, tab);
}

// the listed sections: a wavefront each; past the grid a wavefront takes more than one
__global__ __launch_bounds__(256) void mf_crc_long(MfDev d, MfRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t *xp = d.tab + 256;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t N = d.ctl[C_NI];
  const uint32_t count = d.ctl[C_NLONG] < N ? d.ctl[C_NLONG] : N;
  for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < count; w += gridDim.x * 4) {
    const uint32_t j = d.lng[w];
    if (j >= N) continue;
    const uint32_t nj = d.ilen[j] & M_LEN;
    if (nj <= CRC_LANE_MAX) continue;
    const uint8_t *pay = mf_payload(d, r, j);
    const uint32_t T = nj - 4;
    int lo, hi;
    const uint32_t c = crc32m_wave_chunk(lane, T, lo, hi);
    uint32_t crc = 0;
    if (hi > lo) crc = crc_span(0, d.ihdr + 3 * (size_t)j, pay, (uint32_t)lo, (uint32_t)hi, tab);
    crc = crc32m_wave_join(crc, lane, c, T, xp);
    if (lane == 0) d.icrc[j] = crc;
  }
}

// ------------------------------------------------------------------------------------------ the cut, emit
// the call's flush counts unless a lookahead frame follows; all: nothing of the items is left
__device__ inline PkCut mf_cut(const MfDev &d, const MfRun &r) {
  const uint32_t look = d.ctl[C_LOOK];
  uint32_t lim = ~0u;
  if (look) {   // up to the packet the last frame to send ends in: the one before the lookahead frame's first section
                // where that begins a packet, else the one it starts in (full: the lookahead frame is longer than it)
    const uint32_t x = cnt_of(d.pre[d.fs[look]]) + look * d.K - d.ctl[C_IS];
    lim = d.pkt[x] + (d.at[x] != 1 ? 1 : 0);
  }
  PkCut c = pk_cut(d.ctl[C_T], d.ctl[C_Q], d.ctl[C_S], r.flush && !look, r.cap, lim);
  c.all = c.all && !look;
  return c;
}

__global__ __launch_bounds__(PK_THREADS) void mf_emit(MfDev d, MfRun r) {
  pk_emit_body<MINFREE>(MfSrc{d, r}, mf_units(d), mf_cut(d, r), d.packing, (uint32_t)d.pid, r.cc, r.out, &d.res[MF_R_PUSI],
                        &d.res[MF_R_PAD]);
}

// ------------------------------------------------------------------------------------------ resume, counters
__global__ __launch_bounds__(PK_THREADS) void mf_count(MfDev d, MfRun r) {
  __shared__ uint32_t hist[4];
  if (threadIdx.x < 4) hist[threadIdx.x] = 0;
  __syncthreads();
  const PkCut c = mf_cut(d, r);
  const uint32_t F = d.ctl[C_F], rest = d.ctl[C_REST];
  // the resume position: the PDU (in this run's indices), the section of its frame, that section's bytes emitted, the
  // frames wholly sent
  uint32_t jr, sec = 0, sb = 0, fr = F;
  if (!F) {
    jr = rest;
    fr = 0;
    if (rest < r.n) {   // the frame the start names is not closed in this call: resume = start
      jr = 0;
      sec = r.section;
      sb = r.section_byte;
    }
  } else if (!c.all) {
    const PkPos ps = pk_locate(mf_units(d), c.s, c.E);
    uint32_t x = ps.jn;   // every item is a section: the next one begins the packet when none runs on into it
    if (ps.R) {
      x = ps.jc;
      sb = ps.coff;
    }
    const uint32_t seq = x + d.ctl[C_IS];
    uint32_t a = 0, b = F - 1;   // the last frame whose first section is seq or earlier
    while (a < b) {
      const uint32_t mid = (a + b + 1) >> 1;
      if (cnt_of(d.pre[d.fs[mid]]) + mid * d.K <= seq) a = mid;
      else b = mid - 1;
    }
    fr = a;
    jr = d.fs[a];
    sec = seq - (cnt_of(d.pre[jr]) + a * d.K);
  } else jr = rest;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    d.res[MF_R_PDU] = r.i0 + jr;
    d.res[MF_R_SECTION] = sec;
    d.res[MF_R_SECTION_BYTE] = sb;
    d.res[MF_R_CC] = (r.cc + c.E) & 15;
    d.res[MF_R_FRAME] = (r.frame + fr) & 0xFFFu;
    d.res[MF_R_PDUS_IN] = jr;
    d.res[MF_R_FEC_SECTIONS] = (u64)fr * d.K;
    d.res[MF_R_FRAMES] = fr;
    d.res[MF_R_TS_PACKETS] = c.E;
    d.res[MF_R_FLUSHED] = r.flush && jr == r.n ? 1 : 0;
  }
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < jr; i += gridDim.x * 256) {
    const uint32_t w = d.len[i];
    atomicAdd(&hist[(w & M_LEN) ? 0 : (w & M_SKIP_LEN) ? 1 : 2], 1u);
    if (w & M_MAPPED) atomicAdd(&hist[3], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 4 && hist[threadIdx.x]) {
    const int at[4] = {MF_R_SECTIONS, MF_R_SKIPPED_LEN, MF_R_SKIPPED_TYPE, MF_R_MAPPED};
    atomicAdd(&d.res[at[threadIdx.x]], (unsigned long long)hist[threadIdx.x]);
  }
}

uint32_t gf256_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (; b; b >>= 1) {
    if (b & 1) r ^= a;
    a = (a << 1) ^ ((a & 0x80) ? 0x11Du : 0);
  }
  return r;
}

// the frames that PDUs lying side by side can close, up to most: two successive frames hold more than C bytes
uint64_t frames_estimate(const MfDev &d, uint64_t pdu_len, uint64_t n, uint64_t most) {
  const uint64_t C = (uint64_t)d.D * d.rows;
  return std::min<uint64_t>(std::min<uint64_t>(most, n), 2 * pdu_len / (C + 1) + 2);
}

}  // namespace

void mf_host_tables(uint32_t *tab, uint32_t *rstab) {
  crc32m_host_tables(tab, MF_MAX_SECTION + 1);
  // g(x) = prod (x + 2^i), i = 0 .. 63, over GF(2^8) with 0x11D: g[0] .. g[64]
  uint32_t g[MF_RS_COLS + 1] = {1};
  uint32_t root = 1;
  for (int i = 0; i < MF_RS_COLS; i++) {
    for (int k = i + 1; k > 0; k--) g[k] = g[k - 1] ^ gf256_mul(g[k], root);
    g[0] = gf256_mul(g[0], root);
    root = gf256_mul(root, 2);
  }
  for (uint32_t v = 0; v < 256; v++)
    for (int w = 0; w < 16; w++) {
      uint32_t x = 0;
      for (int b = 0; b < 4; b++) x |= gf256_mul(v, g[63 - (4 * w + b)]) << (8 * b);   // byte k: v g_(63 - k)
      rstab[16 * v + w] = x;
    }
}

size_t mf_layout(MfDev &d, void *base) {
  LayoutTaker take{base};
  const size_t n = std::max<uint32_t>(d.max_pdus, 1), ni = std::max<uint32_t>(d.max_items, 1), nt = state_tiles_of(ni);
  take(d.res, MF_R_WORDS + MF_CTL_WORDS / 2);
  d.ctl = base ? (uint32_t *)(d.res + MF_R_WORDS) : nullptr;
  take(d.len, n);
  take(d.macw, n);
  take(d.pre, n + 1);
  take(d.tile, scan_tiles_of(d.max_pdus + 1) + 1);
  take(d.end, n);
  take(d.fs, (size_t)d.max_frames + 3);
  take(d.ilen, ni);
  take(d.isrc, ni);
  take(d.ihdr, 3 * ni);
  take(d.icrc, ni);
  take(d.lng, ni);
  take(d.pkt, ni);
  take(d.at, ni);
  take(d.maps, (size_t)nt * PK_STATES);
  take(d.ent_q, nt);
  take(d.ent_pk, nt);
  take(d.tab, MF_TAB_WORDS);
  take(d.rstab, MF_RS_WORDS);
  take(d.tbl, ((size_t)d.max_frames + 1) * d.D * d.rows);   // the lookahead frame's as well
  take(d.par, ((size_t)d.max_frames + 1) * d.K * d.rows + 8);
  return take.at;
}

uint64_t mf_packet_estimate(const MfDev &d, uint64_t pdu_len, uint64_t n) {
  const uint64_t F = frames_estimate(d, pdu_len, n, d.max_frames);
  const uint64_t bytes = pdu_len + 16 * n + F * d.K * (d.rows + 16);
  return d.packing ? bytes / 183 + 2 : bytes / 184 + n + F * d.K + 1;
}

uint64_t mf_packet_limit(const MfDev &d, uint64_t pdu_len, uint64_t n) {
  const uint64_t one = std::min<uint64_t>(std::min<uint64_t>(pdu_len, MF_MAX_PDU), (uint64_t)d.D * d.rows) + 16;
  const uint64_t fec = std::min<uint64_t>(d.max_frames, n) * d.K, fn = d.rows + 16;
  return d.packing ? (n * one + fec * fn) / 183 + 2 : n * (one / 184 + 1) + fec * (fn / 184 + 1) + 1;
}

hipError_t mf_launch(const MfDev &d, const MfRun &r, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, (MF_R_WORDS + MF_CTL_WORDS / 2) * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const uint32_t nb = std::max<uint32_t>(1, (r.n + 255) / 256), nb1 = (r.n + 1 + 255) / 256;
  const uint32_t fb = std::min<uint32_t>(d.max_frames + 1, r.n);                  // frames: whatever the offsets say
  const uint32_t fe = (uint32_t)frames_estimate(d, r.pdu_len, r.n, d.max_frames + 1);   // frames: PDUs side by side
  const uint64_t items = (uint64_t)r.n + (uint64_t)fb * d.K;                      // never more sections than this
  const uint32_t nt = state_tiles_of(items);
  hipLaunchKernelGGL(mf_measure, dim3(nb1), dim3(256), 0, st, d, r);
  if ((e = scan_exclusive(MF_SCAN, d.pre, d.tile, r.n + 1, nullptr, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(mf_next, dim3(nb), dim3(256), 0, st, d, r);
  hipLaunchKernelGGL(mf_chain, dim3(1), dim3(64), 0, st, d, r);
  if (fe) {
    hipLaunchKernelGGL(mf_items_mpe, dim3(nb), dim3(256), 0, st, d, r);
    hipLaunchKernelGGL(mf_items_fec, dim3((fe * d.K + 255) / 256), dim3(256), 0, st, d, r);
    const uint64_t gw = (uint64_t)fe * (d.D * d.rows / 4);
    hipLaunchKernelGGL(mf_gather, dim3((uint32_t)std::min<uint64_t>((gw + 255) / 256, 1u << 20)), dim3(256), 0, st, d, r);
    hipLaunchKernelGGL(mf_rs, dim3(fe * (d.rows / RS_ROWS)), dim3(RS_ROWS), 0, st, d);
    hipLaunchKernelGGL(mf_maps, dim3(nt), dim3(PK_THREADS), 0, st, d);
  }
  hipLaunchKernelGGL(mf_compose, dim3(1), dim3(PK_COMPOSE_THREADS), 0, st, d);
  if (fe) {
    hipLaunchKernelGGL(mf_walk, dim3(nt), dim3(PK_THREADS), 0, st, d);
    hipLaunchKernelGGL(mf_crc_short, dim3((uint32_t)((items + 255) / 256)), dim3(256), 0, st, d, r);
    const uint64_t nlong = std::min<uint64_t>(r.n, r.pdu_len / (CRC_LANE_MAX - 15)) + (uint64_t)fe * d.K;
    hipLaunchKernelGGL(mf_crc_long, dim3((uint32_t)((nlong + 3) / 4)), dim3(256), 0, st, d, r);
    const uint64_t est = std::min<uint64_t>(r.cap, mf_packet_estimate(d, r.pdu_len, r.n));
    if (est) hipLaunchKernelGGL(mf_emit, dim3((uint32_t)((est + PK_EMIT_PKTS - 1) / PK_EMIT_PKTS)), dim3(PK_THREADS), 0, st, d, r);
  }
  hipLaunchKernelGGL(mf_count, dim3(std::min(COUNT_BLOCKS, nb)), dim3(PK_THREADS), 0, st, d, r);
  return hipGetLastError();
}

}  // namespace t2
