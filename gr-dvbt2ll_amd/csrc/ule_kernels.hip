// ULE encapsulation (RFC 4326) on gfx950: a device buffer of PDUs and an offset table -> 188-byte TS packets.
// Semantics: include/dvbt2ll_hip.h; tests/ule_ref.py is the sequential restatement every output is compared with.
//
// The units ts_section_packer.h packs are the SNDUs: a packet with fewer than two free bytes is closed, since an SNDU's
// Length field must fit (MINFREE 2).  Passes of one run, all on the caller's stream:
//   measure    one lane per PDU: validity, Type, SNDU length n (packing 0: its packet count, for the sum scan)
//   maps, compose, walk   packing 1: the packer's state scan
//   sum scan   packing 0: every SNDU starts a packet, so the first packets are an exclusive sum (dev_scan.h)
//   crc        SNDUs of up to CRC_LANE_MAX bytes a lane each; the longer ones (listed by measure) a wavefront each
//              (crc32_mpeg2.h)
//   emit       this file's own, of the shape ts_section_packer.h describes: with the shared emit body ule_emit's code
//              came out differently placed and the call measured 0.6 % slower, so ULE keeps the code it had
//   count      the resume position, and the counters of the PDUs before it
// The cut (the determined packets that capacity allows, the flush packet) is arithmetic on the scan's totals: emit
// and count each work it out for themselves.
#include "ule_kernels.h"

#include <algorithm>

#include "crc32_mpeg2.h"
#include "dev_scan.h"
#include "host_util.h"
#include "ts_section_packer.h"

namespace t2 {

namespace {

enum : uint32_t { U_LEN = PK_LEN, U_SKIP_TYPE = 1u << 30, U_SKIP_LEN = 1u << 31 };
enum : int { C_T = 0, C_Q = 1, C_S = 2, C_NLONG = 3 };   // d.ctl
static_assert(ULE_MAP_STATES == PK_STATES && ULE_TILE == PK_TILE, "the layout is sized for the packer's maps");
constexpr int MINFREE = 2;
constexpr uint32_t CRC_LANE_MAX = 192;
constexpr uint32_t COUNT_BLOCKS = 64;   // the count pass strides over the PDUs past COUNT_BLOCKS x 256

__global__ __launch_bounds__(SCAN_THREADS) void ule_scan_reduce(const uint32_t *in, uint32_t *tile, uint32_t n,
                                                                const uint32_t *n_dev) {
  __shared__ uint32_t lds[SCAN_THREADS];
  scan_reduce_body(in, tile, n, n_dev, lds);
}
__global__ __launch_bounds__(SCAN_THREADS) void ule_scan_tiles(uint32_t *tile, uint32_t ntiles) {
  __shared__ uint32_t lds[2 * SCAN_THREADS];
  scan_tiles_body(tile, ntiles, lds);
}
__global__ __launch_bounds__(SCAN_THREADS) void ule_scan_apply(uint32_t *data, const uint32_t *tile, uint32_t n,
                                                               const uint32_t *n_dev) {
  __shared__ uint32_t lds[2 * SCAN_THREADS];
  scan_apply_body(data, tile, n, n_dev, lds);
}
constexpr ScanKernels<uint32_t> ULE_SCAN{ule_scan_reduce, ule_scan_tiles, ule_scan_apply};

uint32_t state_tiles_of(uint32_t n) { return std::max<uint32_t>(1, (n + PK_TILE - 1) / PK_TILE); }
__device__ inline PkUnits ule_units(const UleDev &d, uint32_t N) { return PkUnits{d.len, d.pkt, d.at, N}; }

// ------------------------------------------------------------------------------------------ measure
__global__ __launch_bounds__(256) void ule_measure(UleDev d, UleRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < r.n;
  const uint32_t o0 = in ? r.off[r.i0 + i] : 0, o1 = in ? r.off[r.i0 + i + 1] : 0;
  uint32_t n = 0, flags = 0, type = 0;
  if (o1 <= o0 || o1 > r.pdu_len) flags = U_SKIP_LEN;
  else {
    const uint32_t lenf = (d.d_bit ? 0u : 6u) + (o1 - o0) + 4u;
    if (lenf > 32767u) flags = U_SKIP_LEN;
    else if (r.type) type = r.type[r.i0 + i];
    else {
      const uint32_t nib = r.pdu[o0] >> 4;
      if (nib == 4) type = 0x0800;
      else if (nib == 6) type = 0x86DD;
      else flags = U_SKIP_TYPE;
    }
    if (!flags) n = 4 + lenf;
  }
  // the long SNDUs are listed for the CRC pass (in no order): one atomic per wavefront
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
  // the start's sndu_byte counts where it names a byte of a valid SNDU
  uint32_t s = 0;
  if (i == 0) {
    if (n && r.sndu_byte < n) s = r.sndu_byte;
    d.ctl[C_S] = s;
  }
  d.len[i] = n | flags;
  d.typ[i] = (uint16_t)type;
  if (!d.packing) {
    d.pkt[i] = n ? (s ? (n - s + 183) / 184 : (n + 184) / 184) : 0;   // packets: PP and 183 bytes, then 184 each
    d.at[i] = s ? 0 : 1;
  }
}

// ------------------------------------------------------------------------------------------ the state scan
__global__ __launch_bounds__(PK_THREADS) void ule_maps(UleDev d, uint32_t N) {
  pk_maps_body<MINFREE>(d.len, N, d.ctl[C_S], true, d.maps);
}

__global__ __launch_bounds__(PK_COMPOSE_THREADS) void ule_compose(UleDev d, uint32_t ntiles) {
  pk_compose_body(d.maps, ntiles, d.ent_q, d.ent_pk, &d.ctl[C_T], &d.ctl[C_Q]);
}

__global__ __launch_bounds__(PK_THREADS) void ule_walk(UleDev d, uint32_t N) {
  pk_walk_body<MINFREE>(ule_units(d, N), d.ctl[C_S], true, d.ent_q, d.ent_pk);
}

// ------------------------------------------------------------------------------------------ SNDU bytes
// byte k < header length of an SNDU of n bytes
__device__ inline uint32_t ule_header_byte(const UleDev &d, uint32_t n, uint32_t type, uint32_t k) {
  const uint32_t w = ((uint32_t)d.d_bit << 15) | (n - 4);
  if (k == 0) return w >> 8;
  if (k == 1) return w & 255;
  if (k == 2) return type >> 8;
  if (k == 3) return type & 255;
  return d.dest[k - 4];
}

// byte k of PDU j's SNDU
__device__ inline uint32_t ule_sndu_byte(const UleDev &d, const UleRun &r, uint32_t j, uint32_t k) {
  const uint32_t n = d.len[j] & U_LEN, hl = d.d_bit ? 4 : 10;
  if (k < hl) return ule_header_byte(d, n, d.typ[j], k);
  if (k + 4 < n) return r.pdu[r.off[r.i0 + j] + (k - hl)];
  return (d.crc[j] >> (8 * (n - 1 - k))) & 255;
}

// bytes k .. k + 3 of PDU j's SNDU (all inside it): two aligned words of the PDU buffer where all four are PDU bytes
// and the words lie inside the buffer, bytes otherwise
__device__ inline uint32_t ule_sndu_word(const UleDev &d, const UleRun &r, uint32_t j, uint32_t k) {
  const uint32_t n = d.len[j] & U_LEN, hl = d.d_bit ? 4 : 10;
  if (k >= hl && k + 8 <= n) {
    const uint8_t *src = r.pdu + r.off[r.i0 + j] + (k - hl);
    const uint32_t sh = (uint32_t)((uintptr_t)src & 3);
    const uint8_t *a = src - sh;
    if (sh == 0) return *(const uint32_t *)a;
    if (a >= r.pdu && a + 8 <= r.pdu + r.pdu_len) {
      const uint32_t lo = *(const uint32_t *)a, hi = *(const uint32_t *)(a + 4);
      return (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
    }
  }
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++) w |= ule_sndu_byte(d, r, j, k + q) << (8 * q);
  return w;
}

// ------------------------------------------------------------------------------------------ CRC-32
// SNDU bytes [lo, hi) of an SNDU (hi <= n - 4): the header's, then the PDU's
__device__ inline uint32_t crc_span(const UleDev &d, uint32_t crc, uint32_t n, uint32_t type, const uint8_t *pdu,
                                    uint32_t lo, uint32_t hi, const uint32_t *tab) {
  const uint32_t hl = d.d_bit ? 4 : 10;
  for (; lo < hi && lo < hl; lo++) crc = crc32m_byte(crc, ule_header_byte(d, n, type, lo), tab);
  if (lo < hi) crc = crc32m_run(crc, pdu + (lo - hl), hi - lo, tab);
  return crc;
}

// the SNDUs of up to CRC_LANE_MAX bytes: a lane each
__global__ __launch_bounds__(256) void ule_crc_short(UleDev d, UleRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t n = i < r.n ? d.len[i] & U_LEN : 0;
  if (n && n <= CRC_LANE_MAX) d.crc[i] = crc_span(d, 0xFFFFFFFFu, n, d.typ[i], r.pdu + r.off[r.i0 + i], 0, n - 4, tab);
}

// the longer ones, as measure listed them: a wavefront each.  The grid covers the most that PDUs lying side by side
// can be; where they overlap and are more, a wavefront takes more than one
__global__ __launch_bounds__(256) void ule_crc_long(UleDev d, UleRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t *xp = d.tab + 256;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t count = d.ctl[C_NLONG] < r.n ? d.ctl[C_NLONG] : r.n;
  for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < count; w += gridDim.x * 4) {
    const uint32_t j = d.lng[w];
    if (j >= r.n) continue;
    const uint32_t nj = d.len[j] & U_LEN, tj = d.typ[j], oj = r.off[r.i0 + j];
    if (nj <= CRC_LANE_MAX) continue;
    const uint32_t T = nj - 4;
    int lo, hi;
    const uint32_t c = crc32m_wave_chunk(lane, T, lo, hi);
    uint32_t crc = 0;
    if (hi > lo) crc = crc_span(d, 0, nj, tj, r.pdu + oj, (uint32_t)lo, (uint32_t)hi, tab);
    crc = crc32m_wave_join(crc, lane, c, T, xp);
    if (lane == 0) d.crc[j] = crc;
  }
}

// ------------------------------------------------------------------------------------------ the cut, positions
struct UleCut {
  uint32_t T, q, s;    // packets completed, the end state (an open PUSI packet when not 0), the start's sndu_byte
  uint32_t E;          // packets emitted
  bool all;            // nothing is left
};

__device__ inline UleCut ule_cut(const UleDev &d, const UleRun &r, const uint32_t *total) {
  UleCut c;
  c.T = *total;
  c.q = d.packing ? d.ctl[C_Q] : 0;
  c.s = d.ctl[C_S];
  const uint32_t det = c.T + (c.q && r.flush ? 1 : 0);   // the open packet is determined by a flush only
  c.E = det < r.cap ? det : r.cap;
  c.all = c.E == det && (c.q == 0 || r.flush);
  return c;
}

// what packet p begins with: R > 0 bytes left of PDU jc's SNDU, from its byte coff on; jn: the first PDU whose SNDU
// can start in the packet
struct UlePos { uint32_t jc, R, coff, jn; };

__device__ inline UlePos ule_locate(const UleDev &d, uint32_t N, uint32_t s, uint32_t p) {
  uint32_t lo = 0, hi = N;   // the first PDU whose first packet is p or later
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d.pkt[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  UlePos ps{0, 0, 0, lo};
  if (p == 0 && s && N) {   // the SNDU an earlier call began
    ps.R = (d.len[0] & U_LEN) - s;
    ps.coff = s;
    ps.jn = 1;
  } else if (lo > 0) {
    // the PDU before is valid (only a valid one moves the packet count): its SNDU may run on into p
    const uint32_t j = lo - 1, n = d.len[j] & U_LEN, sk = j == 0 ? s : 0;
    const uint32_t consumed = (184 - d.at[j]) + 184 * (p - d.pkt[j] - 1);
    ps.jc = j;
    ps.coff = sk + consumed;
    ps.R = n > ps.coff ? n - ps.coff : 0;
  }
  return ps;
}

// ------------------------------------------------------------------------------------------ emit
struct UleRec {
  uint32_t jc, jn, jend;   // the continuing SNDU's PDU; the PDUs whose first packet this is: [jn, jend)
  uint16_t R, coff;
  uint8_t pusi, nb;        // PUSI 0: nb SNDU bytes, the rest FF
};

__device__ inline UleRec ule_record(const UleDev &d, const UleRun &r, const UleCut &c, uint32_t p, uint32_t &pad) {
  const UlePos ps = ule_locate(d, r.n, c.s, p);
  UleRec q;
  q.jc = ps.jc;
  q.jn = q.jend = ps.jn;
  q.R = (uint16_t)ps.R;
  q.coff = (uint16_t)ps.coff;
  bool pusi;
  if (!d.packing) pusi = ps.R == 0;
  // packing: 182 or more left fill the packet; the flush's last packet holding nothing but an SNDU's end has no PP
  else pusi = !(ps.R >= 182 || (p == c.T && ps.R && c.q == 1 + ps.R));
  q.pusi = pusi;
  q.nb = 0;
  if (!pusi) {
    q.nb = (uint8_t)(ps.R < 184 ? ps.R : 184);
    pad = 184 - q.nb;
  } else {
    uint32_t used = 1 + ps.R, x = ps.jn;
    for (; x < r.n && d.pkt[x] == p; x++) {
      const uint32_t n = d.len[x] & U_LEN;
      if (n) used = d.at[x] + n < 184 ? d.at[x] + n : 184;
    }
    q.jend = x;
    pad = 184 - used;
  }
  return q;
}

// payload byte b of a packet: true with (j, k) where it is byte k of PDU j's SNDU, else lit is the byte
__device__ inline bool ule_resolve(const UleDev &d, const UleRec &q, uint32_t b, uint32_t &j, uint32_t &k,
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
    const uint32_t n = d.len[x] & U_LEN, a = d.at[x];
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

__device__ inline uint32_t ule_out_byte(const UleDev &d, const UleRun &r, const UleRec &q, uint32_t p, uint32_t o) {
  if (o == 0) return 0x47;
  if (o == 1) return ((uint32_t)q.pusi << 6) | ((uint32_t)d.pid >> 8);
  if (o == 2) return (uint32_t)d.pid & 255;
  if (o == 3) return 0x10 | ((r.cc + p) & 15);
  uint32_t j, k, lit;
  if (ule_resolve(d, q, o - 4, j, k, lit)) return ule_sndu_byte(d, r, j, k);
  return lit;
}

// output bytes g .. g + 3 (packets p0 and up: rec)
__device__ inline uint32_t ule_out_word(const UleDev &d, const UleRun &r, const UleRec *rec, uint32_t p0, size_t g) {
  const uint32_t p = (uint32_t)(g / 188), o = (uint32_t)(g - (size_t)p * 188);
  if (o >= 4 && o + 4 <= 188) {
    uint32_t j, k, lit;
    if (ule_resolve(d, rec[p - p0], o - 4, j, k, lit) && k + 4 <= (d.len[j] & U_LEN)) return ule_sndu_word(d, r, j, k);
  }
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++) {
    const uint32_t pp = (uint32_t)((g + q) / 188), oo = (uint32_t)(g + q - (size_t)pp * 188);
    w |= ule_out_byte(d, r, rec[pp - p0], pp, oo) << (8 * q);
  }
  return w;
}

// The grid covers the packets that PDUs lying side by side can become (ule_packet_estimate); where the offsets make
// valid PDUs overlap and the packets are more, a workgroup takes more than one group of PK_EMIT_PKTS: its second trip
// begins at the loop's second pass
__global__ __launch_bounds__(256) void ule_emit(UleDev d, UleRun r, const uint32_t *total) {
  __shared__ UleRec rec[PK_EMIT_PKTS];
  __shared__ uint32_t cnt[2];
  const UleCut c = ule_cut(d, r, total);
  for (uint32_t p0 = blockIdx.x * PK_EMIT_PKTS; p0 < c.E; p0 += gridDim.x * PK_EMIT_PKTS) {
    const uint32_t np = c.E - p0 < PK_EMIT_PKTS ? c.E - p0 : PK_EMIT_PKTS;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();   // the trip before no longer reads rec
    if (threadIdx.x < np) {
      uint32_t pad = 0;
      rec[threadIdx.x] = ule_record(d, r, c, p0 + threadIdx.x, pad);
      if (rec[threadIdx.x].pusi) atomicAdd(&cnt[0], 1u);
      if (pad) atomicAdd(&cnt[1], pad);
    }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x])
      atomicAdd(&d.res[threadIdx.x ? ULE_R_PAD : ULE_R_PUSI], (unsigned long long)cnt[threadIdx.x]);
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
        for (uint32_t q = 0; q < 4; q++) w[q] = ule_out_word(d, r, rec, p0, lo + 4 * q);
        *(uint4 *)(r.out + lo) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (size_t g = lo; g < hi; g++) {
          const uint32_t p = (uint32_t)(g / 188), o = (uint32_t)(g - (size_t)p * 188);
          r.out[g] = (uint8_t)ule_out_byte(d, r, rec[p - p0], p, o);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ resume, counters
__global__ __launch_bounds__(256) void ule_count(UleDev d, UleRun r, const uint32_t *total) {
  __shared__ uint32_t hist[3], found;
  if (threadIdx.x < 3) hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) found = r.n;
  __syncthreads();
  const UleCut c = ule_cut(d, r, total);
  uint32_t jr = r.n, sb = 0;   // the resume position: the PDU (in this run's indices), its SNDU's bytes emitted
  if (!c.all) {
    const UlePos ps = ule_locate(d, r.n, c.s, c.E);
    if (ps.R) {
      jr = ps.jc;
      sb = ps.coff;
    } else {
      // the first valid PDU from ps.jn on: the workgroup looks at 256 at a time
      for (uint32_t base = ps.jn; base < r.n; base += 256) {
        const uint32_t x = base + threadIdx.x;
        if (x < r.n && (d.len[x] & U_LEN)) atomicMin(&found, x);
        __syncthreads();
        const uint32_t f = found;
        __syncthreads();
        if (f < r.n) break;
      }
      jr = found;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    d.res[ULE_R_PDU] = r.i0 + jr;
    d.res[ULE_R_SNDU_BYTE] = sb;
    d.res[ULE_R_CC] = (r.cc + c.E) & 15;
    d.res[ULE_R_PDUS_IN] = jr;
    d.res[ULE_R_TS_PACKETS] = c.E;
    d.res[ULE_R_FLUSHED] = c.all && r.flush ? 1 : 0;
  }
  // past COUNT_BLOCKS x 256 PDUs a lane takes more than one
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < jr; i += gridDim.x * 256) {
    const uint32_t w = d.len[i];
    atomicAdd(&hist[(w & U_LEN) ? 0 : (w & U_SKIP_LEN) ? 1 : 2], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 3 && hist[threadIdx.x]) {
    const int at[3] = {ULE_R_SNDUS, ULE_R_SKIPPED_LEN, ULE_R_SKIPPED_TYPE};
    atomicAdd(&d.res[at[threadIdx.x]], (unsigned long long)hist[threadIdx.x]);
  }
}

}  // namespace

void ule_host_tables(uint32_t *tab) {
  crc32m_host_tables(tab, ULE_MAX_SNDU + 1);
}

size_t ule_layout(UleDev &d, void *base) {
  LayoutTaker take{base};
  const size_t n = std::max<uint32_t>(d.max_pdus, 1), nt = state_tiles_of(d.max_pdus);
  take(d.res, ULE_R_WORDS + 2);
  d.ctl = base ? (uint32_t *)(d.res + ULE_R_WORDS) : nullptr;
  take(d.len, n);
  take(d.typ, n);
  take(d.crc, n);
  take(d.lng, n);
  take(d.pkt, n);
  take(d.at, n);
  take(d.tile, scan_tiles_of(d.max_pdus) + 1);
  take(d.maps, nt * PK_STATES);
  take(d.ent_q, nt);
  take(d.ent_pk, nt);
  take(d.tab, ULE_TAB_WORDS);
  return take.at;
}

uint64_t ule_packet_estimate(const UleDev &d, uint64_t pdu_len, uint64_t n) {
  const uint64_t bytes = pdu_len + 14 * n;   // no SNDU adds more than 14 bytes to its PDU
  // packing: every packet but the flush's holds 182 SNDU bytes or more; without: a PP per SNDU, then 184 a packet
  return d.packing ? bytes / 182 + 2 : bytes / 184 + n + 1;
}

uint64_t ule_packet_limit(const UleDev &d, uint64_t pdu_len, uint64_t n) {
  // every PDU may be the whole buffer, or the longest an SNDU takes
  const uint64_t one = std::min<uint64_t>(pdu_len, 32763) + 14;
  return d.packing ? n * one / 182 + 2 : n * (one / 184 + 1) + 1;
}

hipError_t ule_launch(const UleDev &d, const UleRun &r, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, (ULE_R_WORDS + 2) * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const uint32_t nb = std::max<uint32_t>(1, (r.n + 255) / 256), nt = state_tiles_of(r.n);
  const uint32_t *total = d.ctl + C_T;
  hipLaunchKernelGGL(ule_measure, dim3(nb), dim3(256), 0, st, d, r);
  if (d.packing) {
    hipLaunchKernelGGL(ule_maps, dim3(nt), dim3(PK_THREADS), 0, st, d, r.n);
    hipLaunchKernelGGL(ule_compose, dim3(1), dim3(PK_COMPOSE_THREADS), 0, st, d, nt);
    hipLaunchKernelGGL(ule_walk, dim3(nt), dim3(PK_THREADS), 0, st, d, r.n);
  } else {
    if ((e = scan_exclusive(ULE_SCAN, d.pkt, d.tile, r.n, nullptr, st)) != hipSuccess) return e;
    total = d.tile + scan_tiles_of(r.n);
  }
  hipLaunchKernelGGL(ule_crc_short, dim3(nb), dim3(256), 0, st, d, r);
  // an SNDU past CRC_LANE_MAX bytes has a PDU of more than CRC_LANE_MAX - 14 bytes
  const uint32_t nlong = (uint32_t)std::min<uint64_t>(r.n, r.pdu_len / (CRC_LANE_MAX - 13));
  if (nlong) hipLaunchKernelGGL(ule_crc_long, dim3((nlong + 3) / 4), dim3(256), 0, st, d, r);
  // emit's grid is sized for PDUs that lie side by side and strides where overlapping ones make more packets
  const uint64_t est = std::min<uint64_t>(r.cap, ule_packet_estimate(d, r.pdu_len, r.n));
  if (r.cap) hipLaunchKernelGGL(ule_emit, dim3((uint32_t)((est + PK_EMIT_PKTS - 1) / PK_EMIT_PKTS)), dim3(256), 0, st, d, r, total);
  hipLaunchKernelGGL(ule_count, dim3(std::min(COUNT_BLOCKS, nb)), dim3(256), 0, st, d, r, total);
  return hipGetLastError();
}

}  // namespace t2