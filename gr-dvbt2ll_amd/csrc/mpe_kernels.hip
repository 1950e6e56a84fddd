// MPE encapsulation (EN 301 192 clause 7) on gfx950: a device buffer of IP datagrams and an offset table -> DSM-CC
// datagram_sections in 188-byte TS packets.
// Semantics: include/dvbt2ll_hip.h; tests/mpe_ref.py is the sequential restatement every output is compared with.
//
// With packing, the pointer_field byte makes a packet's capacity depend on whether a section starts in it, so where a
// section lands depends on every section before it through a small state: q, the payload bytes used in the open PUSI
// packet (0: none open; otherwise 2 .. 183: a packet with one free byte is still open, since a section may begin in a
// packet's last byte).  A section of n bytes maps (q, packets completed) to (q', packets completed'), and such maps
// compose, so the positions come from a scan over maps.  Passes of one run, all on the caller's stream:
//   measure    one lane per PDU: validity, the MAC, the 12 header bytes as three words, the section length n (packing
//              0: its packet count, for the sum scan)
//   maps       packing 1: one workgroup per tile of MPE_TILE PDUs; lane q walks the tile from entry state q and
//              stores (packets completed << 8 | exit state)
//   compose    packing 1: one workgroup; ST_ROUND tile maps at a time are composed by a Hillis-Steele scan in LDS and
//              applied to the running (state, packets), which is carried from round to round: each tile's entry
//   walk       packing 1: one workgroup per tile walks it from its entry: per PDU its first packet and payload offset
//   sum scan   packing 0: every section starts a packet, so the first packets are an exclusive sum (three launches)
//   crc        sections of up to CRC_LANE_MAX bytes a lane each; the longer ones (listed by measure) a wavefront each:
//              lanes take contiguous chunks through the byte table and the chunks are joined with x^(8 n) mod G
//   emit       one workgroup per EMIT_PKTS output packets: a lane per packet finds what the packet begins with (a
//              search in the per-PDU first packets) into LDS, then a lane per 16 output bytes gathers TS header /
//              pointer / section header / datagram / CRC / FF and stores a head up to the first 16-byte boundary, then
//              uint4s.  A section's header bytes are looked up by their index in the section, so a header that straddles
//              two packets needs no case of its own
//   count      the resume position, and the counters of the PDUs before it
// The cut (the determined packets that capacity allows, the flush packet) is arithmetic on the scan's totals: emit
// and count each work it out for themselves.
#include "mpe_kernels.h"

#include <algorithm>
#include <type_traits>

namespace t2 {

namespace {

constexpr uint32_t MPE_POLY = 0x04C11DB7u;
enum : uint32_t { M_LEN = 0xFFFFu, M_MAPPED = 1u << 29, M_SKIP_TYPE = 1u << 30, M_SKIP_LEN = 1u << 31 };
enum : int { C_T = 0, C_Q = 1, C_S = 2, C_NLONG = 3 };   // d.ctl
constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;
constexpr int ST_Q = MPE_MAP_STATES, ST_TILE = MPE_TILE, ST_ROUND = 32, ST_THREADS = 512;
constexpr int ST_PER = (ST_ROUND * ST_Q + ST_THREADS - 1) / ST_THREADS;   // map entries of a round per compose lane
constexpr uint32_t CRC_LANE_MAX = 192;   // section bytes: a lane up to here, a wavefront above
constexpr uint32_t HL = MPE_HEADER;
constexpr uint32_t EMIT_PKTS = 64;
constexpr uint32_t COUNT_BLOCKS = 64;   // the count pass strides over the PDUs past COUNT_BLOCKS x 256

// ------------------------------------------------------------------------------------------ device-wide sum scan
// (the three-launch structure of modeadapt_kernels.hip: tile sums of 1024, one workgroup over the sums, apply)
__device__ uint32_t block_exclusive(uint32_t v, uint32_t *lds, uint32_t &total) {
  const int t = threadIdx.x;
  uint32_t *a = lds, *b = lds + SCAN_THREADS;
  a[t] = v;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {
    uint32_t x = a[t];
    if (t >= d) x = a[t - d] + x;
    b[t] = x;
    __syncthreads();
    uint32_t *s = a; a = b; b = s;
  }
  total = a[SCAN_THREADS - 1];
  const uint32_t ex = t ? a[t - 1] : 0;
  __syncthreads();
  return ex;
}

__global__ __launch_bounds__(SCAN_THREADS) void mpe_scan_reduce(const uint32_t *in, uint32_t *tile, uint32_t n) {
  __shared__ uint32_t lds[SCAN_THREADS];
  const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t s = 0;
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; q++)
    if (i0 + q < n) s += in[i0 + q];
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int dd = SCAN_THREADS / 2; dd > 0; dd >>= 1) {
    if ((int)threadIdx.x < dd) lds[threadIdx.x] += lds[threadIdx.x + dd];
    __syncthreads();
  }
  if (threadIdx.x == 0) tile[blockIdx.x] = lds[0];
}

// one workgroup: tile sums -> exclusive tile offsets in place, the grand total to tile[ntiles].  The second round
// (tiles 256 and up) begins at the loop's second pass, with the tiles before it in carry.
__global__ __launch_bounds__(SCAN_THREADS) void mpe_scan_tiles(uint32_t *tile, uint32_t ntiles) {
  __shared__ uint32_t lds[2 * SCAN_THREADS];
  uint32_t carry = 0;
  for (uint32_t b = 0; b < ntiles; b += SCAN_THREADS) {
    const uint32_t i = b + threadIdx.x;
    const uint32_t v = i < ntiles ? tile[i] : 0;
    uint32_t total;
    const uint32_t ex = block_exclusive(v, lds, total);
    if (i < ntiles) tile[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) tile[ntiles] = carry;
}

__global__ __launch_bounds__(SCAN_THREADS) void mpe_scan_apply(uint32_t *data, const uint32_t *tile, uint32_t n) {
  __shared__ uint32_t lds[2 * SCAN_THREADS];
  if (blockIdx.x * SCAN_TILE >= n) return;
  const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  uint32_t s = 0;
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; q++) {
    v[q] = i0 + q < n ? data[i0 + q] : 0;
    s += v[q];
  }
  uint32_t total;
  uint32_t run = tile[blockIdx.x] + block_exclusive(s, lds, total);
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; q++) {
    if (i0 + q < n) data[i0 + q] = run;
    run += v[q];
  }
}

uint32_t scan_tiles_of(uint32_t n) { return std::max<uint32_t>(1, (n + SCAN_TILE - 1) / SCAN_TILE); }
uint32_t state_tiles_of(uint32_t n) { return std::max<uint32_t>(1, (n + ST_TILE - 1) / ST_TILE); }

hipError_t scan_exclusive(uint32_t *data, uint32_t *tile, uint32_t n, hipStream_t st) {
  const uint32_t ntiles = scan_tiles_of(n);
  hipLaunchKernelGGL(mpe_scan_reduce, dim3(ntiles), dim3(SCAN_THREADS), 0, st, data, tile, n);
  hipLaunchKernelGGL(mpe_scan_tiles, dim3(1), dim3(SCAN_THREADS), 0, st, tile, ntiles);
  hipLaunchKernelGGL(mpe_scan_apply, dim3(ntiles), dim3(SCAN_THREADS), 0, st, data, tile, n);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ measure
__global__ __launch_bounds__(256) void mpe_measure(MpeDev d, MpeRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < r.n;
  const uint32_t o0 = in ? r.off[r.i0 + i] : 0, o1 = in ? r.off[r.i0 + i + 1] : 0;
  uint32_t n = 0, flags = 0;
  uint32_t m0 = d.mac[0], m1 = d.mac[1], m2 = d.mac[2], m3 = d.mac[3], m4 = d.mac[4], m5 = d.mac[5];
  if (o1 <= o0 || o1 > r.pdu_len || o1 - o0 > (uint32_t)MPE_MAX_PDU) flags = M_SKIP_LEN;
  else {
    const uint8_t *b = r.pdu + o0;
    const uint32_t p = o1 - o0, nib = b[0] >> 4;
    if (nib != 4 && nib != 6) flags = M_SKIP_TYPE;
    else {
      n = HL + p + 4;
      if (d.mac_mode) {   // a multicast destination gives its own MAC (RFC 1112 / RFC 2464)
        if (nib == 4 && p >= 20 && b[16] >= 224 && b[16] <= 239) {
          m0 = 0x01; m1 = 0x00; m2 = 0x5E; m3 = b[17] & 0x7F; m4 = b[18]; m5 = b[19];
          flags = M_MAPPED;
        } else if (nib == 6 && p >= 40 && b[24] == 0xFF) {
          m0 = 0x33; m1 = 0x33; m2 = b[36]; m3 = b[37]; m4 = b[38]; m5 = b[39];
          flags = M_MAPPED;
        }
      }
    }
  }
  // the long sections are listed for the CRC pass (in no order): one atomic per wavefront
  const bool lng = n > CRC_LANE_MAX;
  const unsigned long long m = __ballot(lng);
  if (m) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == (uint32_t)(__ffsll((long long)m) - 1)) base = atomicAdd(&d.ctl[C_NLONG], (uint32_t)__popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1);
    if (lng) d.lng[base + __popcll(m & ((1ull << lane) - 1))] = i;
  }
  if (!in) return;
  // the start's section_byte counts where it names a byte of a valid section
  uint32_t s = 0;
  if (i == 0) {
    if (n && r.section_byte < n) s = r.section_byte;
    d.ctl[C_S] = s;
  }
  d.len[i] = n | flags;
  if (n) {   // table_id, syntax 1 / private 0 / reserved 11 / section_length, MAC 6, 5, C1, section numbers 0 0, MAC 4 .. 1
    const uint32_t sl = n - 3;
    d.hdr[3 * (size_t)i] = 0x3Eu | ((0xB0u | (sl >> 8)) << 8) | ((sl & 255u) << 16) | (m5 << 24);
    d.hdr[3 * (size_t)i + 1] = m4 | (0xC1u << 8);
    d.hdr[3 * (size_t)i + 2] = m3 | (m2 << 8) | (m1 << 16) | (m0 << 24);
  }
  if (!d.packing) {
    d.pkt[i] = n ? (s ? (n - s + 183) / 184 : (n + 184) / 184) : 0;   // packets: pointer and 183 bytes, then 184 each
    d.at[i] = s ? 0 : 1;
  }
}

// ------------------------------------------------------------------------------------------ the state scan
// one section of n bytes (0: a skipped PDU) entered in state q with pk packets completed; cont: it continues an earlier
// call's section, which begins the call's first packet
__device__ inline void mpe_step(uint32_t n, bool cont, uint32_t &q, uint32_t &pk) {
  if (!n) return;
  uint32_t rem = n;
  if (!cont) {
    const uint32_t a = q ? q : 1, space = 184 - a;
    if (n <= space) {
      const uint32_t e = a + n;
      if (e == 184) { pk++; q = 0; }   // it ends on the last byte: the packet is closed
      else q = e;                      // up to 183: with one byte free the next section still starts here
      return;
    }
    pk++;
    rem = n - space;
  }
  pk += rem / 184;
  rem %= 184;
  if (rem == 0) q = 0;
  else if (rem == 183) { pk++; q = 0; }   // 183 + FF: no pointer can point inside the packet
  else q = 1 + rem;                       // PUSI, pointer = rem: the next section starts behind it
}

// the tile's section lengths into LDS; the first of the call less the bytes an earlier call emitted
__device__ inline void mpe_tile_lens(const MpeDev &d, uint32_t N, uint32_t base, uint32_t s, uint16_t *ln) {
  for (uint32_t k = threadIdx.x; k < (uint32_t)ST_TILE; k += blockDim.x) {
    const uint32_t i = base + k;
    uint32_t v = i < N ? d.len[i] & M_LEN : 0;
    if (i == 0 && v) v -= s;
    ln[k] = (uint16_t)v;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void mpe_maps(MpeDev d, uint32_t N) {
  __shared__ uint16_t ln[ST_TILE];
  const uint32_t s = d.ctl[C_S], base = blockIdx.x * ST_TILE;
  mpe_tile_lens(d, N, base, s, ln);
  if (threadIdx.x >= (uint32_t)ST_Q) return;
  uint32_t q = threadIdx.x, pk = 0;
  mpe_step(ln[0], s != 0 && base == 0, q, pk);
  for (int k = 1; k < ST_TILE; k++) mpe_step(ln[k], false, q, pk);
  d.maps[(size_t)blockIdx.x * ST_Q + threadIdx.x] = (pk << 8) | q;
}

__global__ __launch_bounds__(ST_THREADS) void mpe_compose(MpeDev d, uint32_t ntiles) {
  __shared__ uint32_t buf[2][ST_ROUND * ST_Q];
  const uint32_t total = ntiles * ST_Q;
  uint32_t cq = 0, cpk = 0;   // the running state: entered the round with
  uint32_t nxt[ST_PER];
#pragma unroll
  for (int k = 0; k < ST_PER; k++) {
    const uint32_t e = threadIdx.x + k * ST_THREADS;
    nxt[k] = e < total ? d.maps[e] : e % ST_Q;
  }
  // the second round (tiles ST_ROUND and up) begins at this loop's second pass: cq / cpk then hold the state and the
  // packets after the tiles before it, and the round's maps were fetched during the round before
  for (uint32_t b = 0; b < ntiles; b += ST_ROUND) {
    uint32_t *A = buf[0], *B = buf[1];
#pragma unroll
    for (int k = 0; k < ST_PER; k++) {
      const uint32_t e = threadIdx.x + k * ST_THREADS;
      if (e < (uint32_t)(ST_ROUND * ST_Q)) A[e] = nxt[k];
    }
    if (b + ST_ROUND < ntiles) {
#pragma unroll
      for (int k = 0; k < ST_PER; k++) {
        const uint32_t e = threadIdx.x + k * ST_THREADS, g = (b + ST_ROUND) * ST_Q + e;
        nxt[k] = g < total ? d.maps[g] : e % ST_Q;   // past the last tile: the identity
      }
    }
    __syncthreads();
    // inclusive scan over the round's tiles: A[t] becomes tiles b .. b + t composed in order
    for (int dd = 1; dd < ST_ROUND; dd <<= 1) {
#pragma unroll
      for (int k = 0; k < ST_PER; k++) {
        const uint32_t e = threadIdx.x + k * ST_THREADS;
        if (e < (uint32_t)(ST_ROUND * ST_Q)) {
          const uint32_t t = e / ST_Q;
          uint32_t v = A[e];
          if (t >= (uint32_t)dd) {
            const uint32_t f = A[e - dd * ST_Q];               // the tiles before, from this entry state
            v = (f & ~255u) + A[t * ST_Q + (f & 255u)];        // then these, from the state those leave
          }
          B[e] = v;
        }
      }
      __syncthreads();
      uint32_t *x = A; A = B; B = x;
    }
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)ST_ROUND && b + t < ntiles) {
      uint32_t eq = cq, epk = cpk;
      if (t) {
        const uint32_t f = A[(t - 1) * ST_Q + cq];
        eq = f & 255u;
        epk = cpk + (f >> 8);
      }
      d.ent_q[b + t] = eq;
      d.ent_pk[b + t] = epk;
    }
    const uint32_t f = A[(ST_ROUND - 1) * ST_Q + cq];
    cq = f & 255u;
    cpk += f >> 8;
    __syncthreads();   // the next round overwrites the buffers
  }
  if (threadIdx.x == 0) {
    d.ctl[C_T] = cpk;
    d.ctl[C_Q] = cq;
  }
}

__global__ __launch_bounds__(256) void mpe_walk(MpeDev d, uint32_t N) {
  __shared__ uint16_t ln[ST_TILE];
  __shared__ uint32_t pk_s[ST_TILE];
  __shared__ uint8_t at_s[ST_TILE];
  const uint32_t s = d.ctl[C_S], base = blockIdx.x * ST_TILE;
  mpe_tile_lens(d, N, base, s, ln);
  if (threadIdx.x == 0) {
    uint32_t q = d.ent_q[blockIdx.x], pk = d.ent_pk[blockIdx.x];
    for (int k = 0; k < ST_TILE; k++) {
      const bool cont = k == 0 && base == 0 && s != 0;
      pk_s[k] = pk;
      at_s[k] = (uint8_t)(cont ? 0 : q ? q : 1);
      mpe_step(ln[k], cont, q, pk);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < (uint32_t)ST_TILE; k += 256)
    if (base + k < N) {
      d.pkt[base + k] = pk_s[k];
      d.at[base + k] = at_s[k];
    }
}

// ------------------------------------------------------------------------------------------ section bytes
// byte k < HL of a section whose header words are h
__device__ inline uint32_t mpe_header_byte(const uint32_t *h, uint32_t k) { return (h[k >> 2] >> (8 * (k & 3))) & 255; }

// byte k of PDU j's section
__device__ inline uint32_t mpe_section_byte(const MpeDev &d, const MpeRun &r, uint32_t j, uint32_t k) {
  const uint32_t n = d.len[j] & M_LEN;
  if (k < HL) return mpe_header_byte(d.hdr + 3 * (size_t)j, k);
  if (k + 4 < n) return r.pdu[r.off[r.i0 + j] + (k - HL)];
  return (d.crc[j] >> (8 * (n - 1 - k))) & 255;
}

// bytes k .. k + 3 of PDU j's section (all inside it): a header word; one aligned word of the PDU buffer, or two joined
// by a shift, where all four are datagram bytes and the words lie inside the buffer; bytes otherwise
__device__ inline uint32_t mpe_section_word(const MpeDev &d, const MpeRun &r, uint32_t j, uint32_t k) {
  const uint32_t n = d.len[j] & M_LEN;
  if (k < HL && (k & 3) == 0) return d.hdr[3 * (size_t)j + (k >> 2)];
  if (k >= HL && k + 8 <= n) {
    const uint8_t *src = r.pdu + r.off[r.i0 + j] + (k - HL);
    const uint32_t sh = (uint32_t)((uintptr_t)src & 3);
    const uint8_t *a = src - sh;
    if (sh == 0) return *(const uint32_t *)a;
    if (a >= r.pdu && a + 8 <= r.pdu + r.pdu_len) {
      const uint32_t lo = *(const uint32_t *)a, hi = *(const uint32_t *)(a + 4);
      return (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
    }
  }
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++) w |= mpe_section_byte(d, r, j, k + q) << (8 * q);
  return w;
}

// ------------------------------------------------------------------------------------------ CRC-32
__device__ inline uint32_t gf_mul(uint32_t a, uint32_t b) {   // a(x) b(x) mod G, bit 31 = x^31
  uint32_t r = 0;
  for (int i = 31; i >= 0; i--) {
    r = (r << 1) ^ ((r >> 31) ? MPE_POLY : 0u);
    if ((b >> i) & 1) r ^= a;
  }
  return r;
}

__device__ inline uint32_t crc_byte(uint32_t crc, uint32_t b, const uint32_t *tab) {
  return (crc << 8) ^ tab[(crc >> 24) ^ b];
}

// n bytes at p, all inside one PDU: bytes up to a 4-byte boundary, aligned words, the rest
__device__ inline uint32_t crc_run(uint32_t crc, const uint8_t *p, uint32_t n, const uint32_t *tab) {
  while (n && ((uintptr_t)p & 3)) {
    crc = crc_byte(crc, *p++, tab);
    n--;
  }
  for (; n >= 4; n -= 4, p += 4) {
    const uint32_t w = *(const uint32_t *)p;
    crc = crc_byte(crc, w & 255, tab);
    crc = crc_byte(crc, (w >> 8) & 255, tab);
    crc = crc_byte(crc, (w >> 16) & 255, tab);
    crc = crc_byte(crc, w >> 24, tab);
  }
  for (; n; n--) crc = crc_byte(crc, *p++, tab);
  return crc;
}

// section bytes [lo, hi) of a section (hi <= n - 4): the header's (words h), then the datagram's
__device__ inline uint32_t crc_span(uint32_t crc, const uint32_t *h, const uint8_t *pdu, uint32_t lo, uint32_t hi,
                                    const uint32_t *tab) {
  for (; lo < hi && lo < HL; lo++) crc = crc_byte(crc, mpe_header_byte(h, lo), tab);
  if (lo < hi) crc = crc_run(crc, pdu + (lo - HL), hi - lo, tab);
  return crc;
}

// the sections of up to CRC_LANE_MAX bytes: a lane each
__global__ __launch_bounds__(256) void mpe_crc_short(MpeDev d, MpeRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t n = i < r.n ? d.len[i] & M_LEN : 0;
  if (n && n <= CRC_LANE_MAX) d.crc[i] = crc_span(0xFFFFFFFFu, d.hdr + 3 * (size_t)i, r.pdu + r.off[r.i0 + i], 0, n - 4, tab);
}

// the longer ones, as measure listed them: a wavefront each.  The grid covers the most that PDUs lying side by side
// can be; where they overlap and are more, a wavefront takes more than one
__global__ __launch_bounds__(256) void mpe_crc_long(MpeDev d, MpeRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t *xp = d.tab + 256;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t count = d.ctl[C_NLONG] < r.n ? d.ctl[C_NLONG] : r.n;
  for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < count; w += gridDim.x * 4) {
    const uint32_t j = d.lng[w];
    if (j >= r.n) continue;
    const uint32_t nj = d.len[j] & M_LEN, oj = r.off[r.i0 + j];
    if (nj <= CRC_LANE_MAX) continue;
    // the T bytes are padded in front to 64 chunks of c bytes: leading zeros leave a zero register unchanged, so every
    // lane's chunk has the same length and the tree multiplies by x^(8 c 2^m) at level m; the initial 0xFFFFFFFF is
    // added as 0xFFFFFFFF x^(8 T)
    const uint32_t T = nj - 4, c = (T + 63) >> 6, pad = 64 * c - T;
    int lo = (int)(lane * c) - (int)pad, hi = lo + (int)c;
    if (lo < 0) lo = 0;
    uint32_t crc = 0;
    if (hi > lo) crc = crc_span(0, d.hdr + 3 * (size_t)j, r.pdu + oj, (uint32_t)lo, (uint32_t)hi, tab);
    for (int lv = 0; lv < 6; lv++) {
      const uint32_t other = __shfl_xor(crc, 1 << lv);
      const bool right = (lane >> lv) & 1;
      crc = gf_mul(right ? other : crc, xp[c << lv]) ^ (right ? crc : other);
    }
    crc ^= gf_mul(0xFFFFFFFFu, xp[T]);
    if (lane == 0) d.crc[j] = crc;
  }
}

// ------------------------------------------------------------------------------------------ the cut, positions
struct MpeCut {
  uint32_t T, q, s;    // packets completed, the end state (an open PUSI packet when not 0), the start's section_byte
  uint32_t E;          // packets emitted
  bool all;            // nothing is left
};

__device__ inline MpeCut mpe_cut(const MpeDev &d, const MpeRun &r, const uint32_t *total) {
  MpeCut c;
  c.T = *total;
  c.q = d.packing ? d.ctl[C_Q] : 0;
  c.s = d.ctl[C_S];
  const uint32_t det = c.T + (c.q && r.flush ? 1 : 0);   // the open packet is determined by a flush only
  c.E = det < r.cap ? det : r.cap;
  c.all = c.E == det && (c.q == 0 || r.flush);
  return c;
}

// what packet p begins with: R > 0 bytes left of PDU jc's section, from its byte coff on; jn: the first PDU whose section
// can start in the packet
struct MpePos { uint32_t jc, R, coff, jn; };

__device__ inline MpePos mpe_locate(const MpeDev &d, uint32_t N, uint32_t s, uint32_t p) {
  uint32_t lo = 0, hi = N;   // the first PDU whose first packet is p or later
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d.pkt[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  MpePos ps{0, 0, 0, lo};
  if (p == 0 && s && N) {   // the section an earlier call began
    ps.R = (d.len[0] & M_LEN) - s;
    ps.coff = s;
    ps.jn = 1;
  } else if (lo > 0) {
    // the PDU before is valid (only a valid one moves the packet count): its section may run on into p
    const uint32_t j = lo - 1, n = d.len[j] & M_LEN, sk = j == 0 ? s : 0;
    const uint32_t consumed = (184 - d.at[j]) + 184 * (p - d.pkt[j] - 1);
    ps.jc = j;
    ps.coff = sk + consumed;
    ps.R = n > ps.coff ? n - ps.coff : 0;
  }
  return ps;
}

// ------------------------------------------------------------------------------------------ emit
struct MpeRec {
  uint32_t jc, jn, jend;   // the continuing section's PDU; the PDUs whose first packet this is: [jn, jend)
  uint16_t R, coff;
  uint8_t pusi, nb;        // PUSI 0: nb section bytes, the rest FF
};

__device__ inline MpeRec mpe_record(const MpeDev &d, const MpeRun &r, const MpeCut &c, uint32_t p, uint32_t &pad) {
  const MpePos ps = mpe_locate(d, r.n, c.s, p);
  MpeRec q;
  q.jc = ps.jc;
  q.jn = q.jend = ps.jn;
  q.R = (uint16_t)ps.R;
  q.coff = (uint16_t)ps.coff;
  bool pusi;
  if (!d.packing) pusi = ps.R == 0;
  // packing: 183 or more left leave no room to point at; the flush's last packet holding nothing but a section's end
  // has no pointer
  else pusi = !(ps.R >= 183 || (p == c.T && ps.R && c.q == 1 + ps.R));
  q.pusi = pusi;
  q.nb = 0;
  if (!pusi) {
    q.nb = (uint8_t)(ps.R < 184 ? ps.R : 184);
    pad = 184 - q.nb;
  } else {
    uint32_t used = 1 + ps.R, x = ps.jn;
    for (; x < r.n && d.pkt[x] == p; x++) {
      const uint32_t n = d.len[x] & M_LEN;
      if (n) used = d.at[x] + n < 184 ? d.at[x] + n : 184;
    }
    q.jend = x;
    pad = 184 - used;
  }
  return q;
}

// payload byte b of a packet: true with (j, k) where it is byte k of PDU j's section, else lit is the byte
__device__ inline bool mpe_resolve(const MpeDev &d, const MpeRec &q, uint32_t b, uint32_t &j, uint32_t &k,
                                   uint32_t &lit) {
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
    const uint32_t n = d.len[x] & M_LEN, a = d.at[x];
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

__device__ inline uint32_t mpe_out_byte(const MpeDev &d, const MpeRun &r, const MpeRec &q, uint32_t p, uint32_t o) {
  if (o == 0) return 0x47;
  if (o == 1) return ((uint32_t)q.pusi << 6) | ((uint32_t)d.pid >> 8);
  if (o == 2) return (uint32_t)d.pid & 255;
  if (o == 3) return 0x10 | ((r.cc + p) & 15);
  uint32_t j, k, lit;
  if (mpe_resolve(d, q, o - 4, j, k, lit)) return mpe_section_byte(d, r, j, k);
  return lit;
}

// output bytes g .. g + 3 (packets p0 and up: rec)
__device__ inline uint32_t mpe_out_word(const MpeDev &d, const MpeRun &r, const MpeRec *rec, uint32_t p0, size_t g) {
  const uint32_t p = (uint32_t)(g / 188), o = (uint32_t)(g - (size_t)p * 188);
  if (o >= 4 && o + 4 <= 188) {
    uint32_t j, k, lit;
    if (mpe_resolve(d, rec[p - p0], o - 4, j, k, lit) && k + 4 <= (d.len[j] & M_LEN)) return mpe_section_word(d, r, j, k);
  }
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t pp = (uint32_t)((g + q) / 188), oo = (uint32_t)(g + q - (size_t)pp * 188);
    w |= mpe_out_byte(d, r, rec[pp - p0], pp, oo) << (8 * q);
  }
  return w;
}

// The grid covers the packets that PDUs lying side by side can become (mpe_packet_estimate); where the offsets make
// valid PDUs overlap and the packets are more, a workgroup takes more than one group of EMIT_PKTS: its second trip
// begins at the loop's second pass
__global__ __launch_bounds__(256) void mpe_emit(MpeDev d, MpeRun r, const uint32_t *total) {
  __shared__ MpeRec rec[EMIT_PKTS];
  __shared__ uint32_t cnt[2];
  const MpeCut c = mpe_cut(d, r, total);
  for (uint32_t p0 = blockIdx.x * EMIT_PKTS; p0 < c.E; p0 += gridDim.x * EMIT_PKTS) {
    const uint32_t np = c.E - p0 < EMIT_PKTS ? c.E - p0 : EMIT_PKTS;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();   // the trip before no longer reads rec
    if (threadIdx.x < np) {
      uint32_t pad = 0;
      rec[threadIdx.x] = mpe_record(d, r, c, p0 + threadIdx.x, pad);
      if (rec[threadIdx.x].pusi) atomicAdd(&cnt[0], 1u);
      if (pad) atomicAdd(&cnt[1], pad);
    }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x])
      atomicAdd(&d.res[threadIdx.x ? MPE_R_PAD : MPE_R_PUSI], (unsigned long long)cnt[threadIdx.x]);
    // output bytes [g0, g1): chunk 0 runs up to the first 16-byte boundary, the others are 16 bytes (the last shorter)
    const size_t g0 = (size_t)p0 * 188, g1 = g0 + (size_t)np * 188;
    uint32_t head = (uint32_t)((16 - ((uintptr_t)(r.out + g0) & 15)) & 15);
    if (head > g1 - g0) head = (uint32_t)(g1 - g0);
    const uint32_t nchunks = 1 + (uint32_t)((g1 - g0 - head + 15) / 16);
    for (uint32_t cidx = threadIdx.x; cidx < nchunks; cidx += 256) {
      const size_t lo = cidx ? g0 + head + (size_t)(cidx - 1) * 16 : g0;
      const size_t hi = cidx ? (g1 < lo + 16 ? g1 : lo + 16) : g0 + head;
      if (hi <= lo) continue;
      if (cidx && hi - lo == 16) {
        uint32_t w[4];
        for (uint32_t q = 0; q < 4; q++) w[q] = mpe_out_word(d, r, rec, p0, lo + 4 * q);
        *(uint4 *)(r.out + lo) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (size_t g = lo; g < hi; g++) {
          const uint32_t p = (uint32_t)(g / 188), o = (uint32_t)(g - (size_t)p * 188);
          r.out[g] = (uint8_t)mpe_out_byte(d, r, rec[p - p0], p, o);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ resume, counters
__global__ __launch_bounds__(256) void mpe_count(MpeDev d, MpeRun r, const uint32_t *total) {
  __shared__ uint32_t hist[4], found;
  if (threadIdx.x < 4) hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) found = r.n;
  __syncthreads();
  const MpeCut c = mpe_cut(d, r, total);
  uint32_t jr = r.n, sb = 0;   // the resume position: the PDU (in this run's indices), its section's bytes emitted
  if (!c.all) {
    const MpePos ps = mpe_locate(d, r.n, c.s, c.E);
    if (ps.R) {
      jr = ps.jc;
      sb = ps.coff;
    } else {
      // the first valid PDU from ps.jn on: the workgroup looks at 256 at a time
      for (uint32_t base = ps.jn; base < r.n; base += 256) {
        const uint32_t x = base + threadIdx.x;
        if (x < r.n && (d.len[x] & M_LEN)) atomicMin(&found, x);
        __syncthreads();
        const uint32_t f = found;
        __syncthreads();
        if (f < r.n) break;
      }
      jr = found;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    d.res[MPE_R_PDU] = r.i0 + jr;
    d.res[MPE_R_SECTION_BYTE] = sb;
    d.res[MPE_R_CC] = (r.cc + c.E) & 15;
    d.res[MPE_R_PDUS_IN] = jr;
    d.res[MPE_R_TS_PACKETS] = c.E;
    d.res[MPE_R_FLUSHED] = c.all && r.flush ? 1 : 0;
  }
  // past COUNT_BLOCKS x 256 PDUs a lane takes more than one
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < jr; i += gridDim.x * 256) {
    const uint32_t w = d.len[i];
    atomicAdd(&hist[(w & M_LEN) ? 0 : (w & M_SKIP_LEN) ? 1 : 2], 1u);
    if (w & M_MAPPED) atomicAdd(&hist[3], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 4 && hist[threadIdx.x]) {
    const int at[4] = {MPE_R_SECTIONS, MPE_R_SKIPPED_LEN, MPE_R_SKIPPED_TYPE, MPE_R_MAPPED};
    atomicAdd(&d.res[at[threadIdx.x]], (unsigned long long)hist[threadIdx.x]);
  }
}

}  // namespace

void mpe_host_tables(uint32_t *tab) {
  for (uint32_t v = 0; v < 256; v++) {
    uint32_t c = v << 24;
    for (int i = 0; i < 8; i++) c = (c << 1) ^ ((c >> 31) ? MPE_POLY : 0u);
    tab[v] = c;
  }
  uint32_t p = 1;   // x^(8 n) mod G
  for (int n = 0; n <= MPE_MAX_SECTION; n++) {
    tab[256 + n] = p;
    p = (p << 8) ^ tab[p >> 24];
  }
}

size_t mpe_layout(MpeDev &d, void *base) {
  size_t at = 0;
  auto take = [&](auto *&ptr, size_t count) {
    using E = std::remove_reference_t<decltype(*ptr)>;
    at = (at + 255) & ~(size_t)255;
    ptr = base ? (E *)((char *)base + at) : nullptr;
    at += count * sizeof(E);
  };
  const size_t n = std::max<uint32_t>(d.max_pdus, 1), nt = state_tiles_of(d.max_pdus);
  take(d.res, MPE_R_WORDS + 2);
  d.ctl = base ? (uint32_t *)(d.res + MPE_R_WORDS) : nullptr;
  take(d.len, n);
  take(d.hdr, 3 * n);
  take(d.crc, n);
  take(d.lng, n);
  take(d.pkt, n);
  take(d.at, n);
  take(d.tile, scan_tiles_of(d.max_pdus) + 1);
  take(d.maps, nt * ST_Q);
  take(d.ent_q, nt);
  take(d.ent_pk, nt);
  take(d.tab, MPE_TAB_WORDS);
  return at;
}

uint64_t mpe_packet_estimate(const MpeDev &d, uint64_t pdu_len, uint64_t n) {
  const uint64_t bytes = pdu_len + 16 * n;   // a section adds 16 bytes to its datagram
  // packing: every packet but the flush's holds 183 section bytes or more; without: a pointer per section, then 184 a
  // packet
  return d.packing ? bytes / 183 + 2 : bytes / 184 + n + 1;
}

uint64_t mpe_packet_limit(const MpeDev &d, uint64_t pdu_len, uint64_t n) {
  // every PDU may be the whole buffer, or the longest a section takes
  const uint64_t one = std::min<uint64_t>(pdu_len, MPE_MAX_PDU) + 16;
  return d.packing ? n * one / 183 + 2 : n * (one / 184 + 1) + 1;
}

hipError_t mpe_launch(const MpeDev &d, const MpeRun &r, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, (MPE_R_WORDS + 2) * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const uint32_t nb = std::max<uint32_t>(1, (r.n + 255) / 256), nt = state_tiles_of(r.n);
  const uint32_t *total = d.ctl + C_T;
  hipLaunchKernelGGL(mpe_measure, dim3(nb), dim3(256), 0, st, d, r);
  if (d.packing) {
    hipLaunchKernelGGL(mpe_maps, dim3(nt), dim3(256), 0, st, d, r.n);
    hipLaunchKernelGGL(mpe_compose, dim3(1), dim3(ST_THREADS), 0, st, d, nt);
    hipLaunchKernelGGL(mpe_walk, dim3(nt), dim3(256), 0, st, d, r.n);
  } else {
    if ((e = scan_exclusive(d.pkt, d.tile, r.n, st)) != hipSuccess) return e;
    total = d.tile + scan_tiles_of(r.n);
  }
  hipLaunchKernelGGL(mpe_crc_short, dim3(nb), dim3(256), 0, st, d, r);
  // a section past CRC_LANE_MAX bytes has a PDU of more than CRC_LANE_MAX - 16 bytes
  const uint32_t nlong = (uint32_t)std::min<uint64_t>(r.n, r.pdu_len / (CRC_LANE_MAX - 15));
  if (nlong) hipLaunchKernelGGL(mpe_crc_long, dim3((nlong + 3) / 4), dim3(256), 0, st, d, r);
  // emit's grid is sized for PDUs that lie side by side and strides where overlapping ones make more packets
  const uint64_t est = std::min<uint64_t>(r.cap, mpe_packet_estimate(d, r.pdu_len, r.n));
  if (r.cap) hipLaunchKernelGGL(mpe_emit, dim3((uint32_t)((est + EMIT_PKTS - 1) / EMIT_PKTS)), dim3(256), 0, st, d, r, total);
  hipLaunchKernelGGL(mpe_count, dim3(std::min(COUNT_BLOCKS, nb)), dim3(256), 0, st, d, r, total);
  return hipGetLastError();
}

}  // namespace t2
