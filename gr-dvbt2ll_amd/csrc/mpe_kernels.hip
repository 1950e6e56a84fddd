// MPE encapsulation (EN 301 192 clause 7) on gfx950: a device buffer of IP datagrams and an offset table -> DSM-CC
// datagram_sections in 188-byte TS packets.
// Semantics: include/dvbt2ll_hip.h; tests/mpe_ref.py is the sequential restatement every output is compared with.
//
// The units ts_section_packer.h packs are the sections: a packet with one free byte is still open, since a section may
// begin in a packet's last byte (MINFREE 1).  Passes of one run, all on the caller's stream:
//   measure    one lane per PDU: validity, the MAC, the 12 header bytes as three words, the section length n (packing
//              0: its packet count, for the sum scan)
//   maps, compose, walk   packing 1: the packer's state scan
//   sum scan   packing 0: every section starts a packet, so the first packets are an exclusive sum (dev_scan.h)
//   crc        sections of up to CRC_LANE_MAX bytes a lane each; the longer ones (listed by measure) a wavefront each
//              (crc32_mpeg2.h)
//   emit       the packer's; a section's header bytes are looked up by their index in the section, so a header that
//              straddles two packets needs no case of its own
//   count      the resume position, and the counters of the PDUs before it
// The cut (the determined packets that capacity allows, the flush packet) is arithmetic on the scan's totals: emit
// and count each work it out for themselves.
#include "mpe_kernels.h"

#include <algorithm>

#include "crc32_mpeg2.h"
#include "dev_scan.h"
#include "host_util.h"
#include "ts_section_packer.h"

namespace t2 {

namespace {

enum : uint32_t { M_LEN = PK_LEN, M_MAPPED = 1u << 29, M_SKIP_TYPE = 1u << 30, M_SKIP_LEN = 1u << 31 };
enum : int { C_T = 0, C_Q = 1, C_S = 2, C_NLONG = 3 };   // d.ctl
static_assert(MPE_MAP_STATES == PK_STATES && MPE_TILE == PK_TILE, "the layout is sized for the packer's maps");
constexpr int MINFREE = 1;
constexpr uint32_t CRC_LANE_MAX = 192;   // section bytes: a lane up to here, a wavefront above
constexpr uint32_t HL = MPE_HEADER;
constexpr uint32_t COUNT_BLOCKS = 64;   // the count pass strides over the PDUs past COUNT_BLOCKS x 256

__global__ __launch_bounds__(SCAN_THREADS) void mpe_scan_reduce(const uint32_t *in, uint32_t *tile, uint32_t n,
                                                                const uint32_t *n_dev) {
  __shared__ uint32_t lds[SCAN_THREADS];
  scan_reduce_body(in, tile, n, n_dev, lds);
}
__global__ __launch_bounds__(SCAN_THREADS) void mpe_scan_tiles(uint32_t *tile, uint32_t ntiles) {
  __shared__ uint32_t lds[2 * SCAN_THREADS];
  scan_tiles_body(tile, ntiles, lds);
}
__global__ __launch_bounds__(SCAN_THREADS) void mpe_scan_apply(uint32_t *data, const uint32_t *tile, uint32_t n,
                                                               const uint32_t *n_dev) {
  __shared__ uint32_t lds[2 * SCAN_THREADS];
  scan_apply_body(data, tile, n, n_dev, lds);
}
constexpr ScanKernels<uint32_t> MPE_SCAN{mpe_scan_reduce, mpe_scan_tiles, mpe_scan_apply};

uint32_t state_tiles_of(uint32_t n) { return std::max<uint32_t>(1, (n + PK_TILE - 1) / PK_TILE); }
__device__ inline PkUnits mpe_units(const MpeDev &d, uint32_t N) { return PkUnits{d.len, d.pkt, d.at, N}; }

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
__global__ __launch_bounds__(PK_THREADS) void mpe_maps(MpeDev d, uint32_t N) {
  pk_maps_body<MINFREE>(d.len, N, d.ctl[C_S], true, d.maps);
}

__global__ __launch_bounds__(PK_COMPOSE_THREADS) void mpe_compose(MpeDev d, uint32_t ntiles) {
  pk_compose_body(d.maps, ntiles, d.ent_q, d.ent_pk, &d.ctl[C_T], &d.ctl[C_Q]);
}

__global__ __launch_bounds__(PK_THREADS) void mpe_walk(MpeDev d, uint32_t N) {
  pk_walk_body<MINFREE>(mpe_units(d, N), d.ctl[C_S], true, d.ent_q, d.ent_pk);
}

// ------------------------------------------------------------------------------------------ section bytes
// byte k < HL of a section whose header words are h
__device__ inline uint32_t mpe_header_byte(const uint32_t *h, uint32_t k) { return (h[k >> 2] >> (8 * (k & 3))) & 255; }

// the packer's source of section bytes
struct MpeSrc {
  const MpeDev &d;
  const MpeRun &r;
  // byte k of PDU j's section
  __device__ uint32_t byte(uint32_t j, uint32_t k) const {
    const uint32_t n = d.len[j] & M_LEN;
    if (k < HL) return mpe_header_byte(d.hdr + 3 * (size_t)j, k);
    if (k + 4 < n) return r.pdu[r.off[r.i0 + j] + (k - HL)];
    return (d.crc[j] >> (8 * (n - 1 - k))) & 255;
  }
  // bytes k .. k + 3 of PDU j's section (all inside it): a header word; a word of the PDU buffer where all four are
  // datagram bytes; bytes otherwise
  __device__ uint32_t word(uint32_t j, uint32_t k) const {
    const uint32_t n = d.len[j] & M_LEN;
    uint32_t w = 0;
    if (k < HL && (k & 3) == 0) return d.hdr[3 * (size_t)j + (k >> 2)];
    if (k >= HL && k + 8 <= n && pk_read4(r.pdu + r.off[r.i0 + j] + (k - HL), r.pdu, r.pdu + r.pdu_len, w)) return w;
    for (uint32_t q = 0; q < 4; q++) w |= byte(j, k + q) << (8 * q);
    return w;
  }
};

// ------------------------------------------------------------------------------------------ CRC-32
// section bytes [lo, hi) of a section (hi <= n - 4): the header's (words h), then the datagram's
__device__ inline uint32_t crc_span(uint32_t crc, const uint32_t *h, const uint8_t *pdu, uint32_t lo, uint32_t hi,
                                    const uint32_t *tab) {
  for (; lo < hi && lo < HL; lo++) crc = crc32m_byte(crc, mpe_header_byte(h, lo), tab);
  if (lo < hi) crc = crc32m_run(crc, pdu + (lo - HL), hi - lo, tab);
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
    const uint32_t T = nj - 4;
    int lo, hi;
    const uint32_t c = crc32m_wave_chunk(lane, T, lo, hi);
    uint32_t crc = 0;
    if (hi > lo) crc = crc_span(0, d.hdr + 3 * (size_t)j, r.pdu + oj, (uint32_t)lo, (uint32_t)hi, tab);
    crc = crc32m_wave_join(crc, lane, c, T, xp);
    if (lane == 0) d.crc[j] = crc;
  }
}

// ------------------------------------------------------------------------------------------ the cut, emit
__device__ inline PkCut mpe_cut(const MpeDev &d, const MpeRun &r, const uint32_t *total) {
  return pk_cut(*total, d.packing ? d.ctl[C_Q] : 0, d.ctl[C_S], r.flush, r.cap);
}

__global__ __launch_bounds__(PK_THREADS) void mpe_emit(MpeDev d, MpeRun r, const uint32_t *total) {
  pk_emit_body<MINFREE>(MpeSrc{d, r}, mpe_units(d, r.n), mpe_cut(d, r, total), d.packing, (uint32_t)d.pid, r.cc, r.out,
                        &d.res[MPE_R_PUSI], &d.res[MPE_R_PAD]);
}

// ------------------------------------------------------------------------------------------ resume, counters
__global__ __launch_bounds__(PK_THREADS) void mpe_count(MpeDev d, MpeRun r, const uint32_t *total) {
  __shared__ uint32_t hist[4];
  if (threadIdx.x < 4) hist[threadIdx.x] = 0;
  __syncthreads();
  const PkCut c = mpe_cut(d, r, total);
  uint32_t jr = r.n, sb = 0;   // the resume position: the PDU (in this run's indices), its section's bytes emitted
  if (!c.all) pk_resume(mpe_units(d, r.n), c, jr, sb);
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
  crc32m_host_tables(tab, MPE_MAX_SECTION + 1);
}

size_t mpe_layout(MpeDev &d, void *base) {
  LayoutTaker take{base};
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
  take(d.maps, nt * PK_STATES);
  take(d.ent_q, nt);
  take(d.ent_pk, nt);
  take(d.tab, MPE_TAB_WORDS);
  return take.at;
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
    hipLaunchKernelGGL(mpe_maps, dim3(nt), dim3(PK_THREADS), 0, st, d, r.n);
    hipLaunchKernelGGL(mpe_compose, dim3(1), dim3(PK_COMPOSE_THREADS), 0, st, d, nt);
    hipLaunchKernelGGL(mpe_walk, dim3(nt), dim3(PK_THREADS), 0, st, d, r.n);
  } else {
    if ((e = scan_exclusive(MPE_SCAN, d.pkt, d.tile, r.n, nullptr, st)) != hipSuccess) return e;
    total = d.tile + scan_tiles_of(r.n);
  }
  hipLaunchKernelGGL(mpe_crc_short, dim3(nb), dim3(256), 0, st, d, r);
  // a section past CRC_LANE_MAX bytes has a PDU of more than CRC_LANE_MAX - 16 bytes
  const uint32_t nlong = (uint32_t)std::min<uint64_t>(r.n, r.pdu_len / (CRC_LANE_MAX - 15));
  if (nlong) hipLaunchKernelGGL(mpe_crc_long, dim3((nlong + 3) / 4), dim3(256), 0, st, d, r);
  // emit's grid is sized for PDUs that lie side by side and strides where overlapping ones make more packets
  const uint64_t est = std::min<uint64_t>(r.cap, mpe_packet_estimate(d, r.pdu_len, r.n));
  if (r.cap) hipLaunchKernelGGL(mpe_emit, dim3((uint32_t)((est + PK_EMIT_PKTS - 1) / PK_EMIT_PKTS)), dim3(PK_THREADS), 0, st, d, r, total);
  hipLaunchKernelGGL(mpe_count, dim3(std::min(COUNT_BLOCKS, nb)), dim3(PK_THREADS), 0, st, d, r, total);
  return hipGetLastError();
}

}  // namespace t2
