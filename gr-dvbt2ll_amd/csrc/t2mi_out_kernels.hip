// T2-MI output (ETSI TS 102 773 over DVB data piping) on gfx950: per-PLP packed BBFRAMEs and opaque auxiliary
// payloads in device memory -> the 188-byte TS packets a T2 gateway sends.  Semantics: include/dvbt2ll_hip.h;
// tests/t2mi_out_ref.py (t2mi_ref.t2mi_packet + t2mi_ref.ts_mux) is the sequential definition every output is compared
// with.
//
// Every packet length is a constant of the handle and every call begins on a TS packet boundary, so where a call's
// g-th T2-MI packet starts (TS packet tq[g], stream byte td[g] of it) depends on g alone: one sequential walk on the
// host at create (t2mo_host_walk) fills both tables for max_frames frames, and no call computes a position.  The
// passes of a run, both on the caller's stream:
//   crc    one wavefront per T2-MI packet: CRC-32/MPEG-2 of header and payload (lanes take contiguous chunks through
//          the byte table and combine by multiplying with x^(8 n) mod G, the form t2mi_kernels.hip checks with)
//   emit   one wavefront per run of EMIT_RUN consecutive TS packets: one search of tq for the first, a walk for the
//          others; lanes write the packet's aligned 32-bit words (source words where all four bytes come from one
//          BBFRAME or auxiliary payload, bytes at the seams and at the packet's unaligned edges)
// Grid caps (both passes stride past them): CRC_MAX_BLOCKS x 4 packets, EMIT_MAX_BLOCKS x 4 x EMIT_RUN TS packets.
#include "t2mi_out_kernels.h"

#include <algorithm>

#include "crc32_mpeg2.h"
#include "host_util.h"

namespace t2 {

namespace {

constexpr uint32_t CRC_MAX_BLOCKS = 4096, EMIT_MAX_BLOCKS = 2048, EMIT_RUN = 8;

// ------------------------------------------------------------------------------------------ one T2-MI packet
// the source bytes of packet pk in frame fc of the call: a BBFRAME, or an auxiliary payload
__device__ inline const uint8_t *pkt_source(const T2moDev &d, const T2moRun &r, const T2moPkt &pk, uint32_t fc) {
  if (pk.src < 8) return r.bb[pk.src] + ((size_t)fc * d.F[pk.src] + pk.blk) * d.Lb[pk.src];
  return r.aux + (size_t)fc * r.aux_stride + r.aux_off[pk.src - 8];
}

// packet bytes [slo, shi) are the source's bytes [0, shi - slo) as they stand: the BBFRAME after frame_idx, plp_id and
// intl_frame_start; an auxiliary payload without a last byte that has pad bits
__device__ inline void pkt_source_span(const T2moPkt &pk, uint32_t &slo, uint32_t &shi) {
  slo = pk.src < 8 ? 9 : 6;
  shi = pk.T - 4 - ((pk.src >= 8 && (pk.bits & 7)) ? 1 : 0);
}

// byte i < T - 4 of packet pk (g-th of the call) in frame fc
__device__ inline uint32_t body_byte(const T2moDev &d, const T2moRun &r, const T2moPkt &pk, uint32_t fc, uint32_t g,
                                     uint32_t i) {
  const uint32_t fr = r.fi0 + fc;
  switch (i) {
    case 0: return pk.type;
    case 1: return (r.count0 + g) & 255;
    case 2: return ((r.sf0 + fr / (uint32_t)d.fps) & 15) << 4;
    case 3: return (uint32_t)d.stream_id;
    case 4: return pk.bits >> 8;
    case 5: return pk.bits & 255;
    default: break;
  }
  const uint32_t p = i - 6;
  if (pk.src < 8) {
    if (p == 0) return fr % (uint32_t)d.fps;
    if (p == 1) return (uint32_t)d.plp_id[pk.src];
    if (p == 2) return pk.blk == 0 ? 0x80 : 0;
    return pkt_source(d, r, pk, fc)[p - 3];
  }
  uint32_t b = pkt_source(d, r, pk, fc)[p];
  if (i + 1 == pk.T - 4 && (pk.bits & 7)) b &= (0xFFu << (8 - (pk.bits & 7))) & 0xFF;   // the pad bits are zero
  return b;
}

__global__ __launch_bounds__(256) void t2mi_out_crc(T2moDev d, T2moRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t *xp = d.tab + 256;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nw = gridDim.x * 4;
  for (uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6); g < r.G; g += nw) {
    const uint32_t fc = g / d.P;
    const T2moPkt pk = d.pkt[g - fc * d.P];
    const uint32_t Tb = pk.T - 4;
    int lo, hi;
    const uint32_t c = crc32m_wave_chunk(lane, Tb, lo, hi);   // the body: a chunk per lane, joined below
    uint32_t slo, shi;
    pkt_source_span(pk, slo, shi);
    const uint8_t *src = pkt_source(d, r, pk, fc);
    uint32_t crc = 0;
    for (uint32_t i = (uint32_t)lo; (int)i < hi;) {
      if (i >= slo && i < shi) {
        const uint32_t n = min((uint32_t)hi, shi) - i;
        crc = crc32m_run(crc, src + (i - slo), n, tab);
        i += n;
      } else {
        crc = crc32m_byte(crc, body_byte(d, r, pk, fc, g, i), tab);
        i++;
      }
    }
    crc = crc32m_wave_join(crc, lane, c, Tb, xp);
    if (lane == 0) d.crc[g] = crc;
  }
}

// ------------------------------------------------------------------------------------------ one TS packet
struct TsInfo {
  uint32_t pos;         // first T2-MI stream byte it carries
  uint32_t pusi, ptr;   // a packet starts in it; the pointer_field
  uint32_t stuff;       // adaptation-field bytes, the length byte included
  uint32_t data_c;      // the packet byte that holds stream byte pos
  uint32_t fc, j;       // the frame of the call and the packet of that frame holding stream byte pos
};

__device__ inline uint32_t pkt_start(const T2moDev &d, uint32_t g) {
  const uint32_t fc = g / d.P;
  return fc * d.B + d.pkt[g - fc * d.P].off;
}

// g: the first packet of the call that starts in TS packet q or later (r.G: none)
__device__ inline TsInfo ts_info(const T2moDev &d, const T2moRun &r, uint32_t q, uint32_t g) {
  TsInfo t;
  uint32_t n, holder;
  t.pusi = g < r.G && d.tq[g] == q;
  if (t.pusi) {
    t.ptr = d.td[g];
    t.pos = pkt_start(d, g) - t.ptr;
    n = min(183u, r.E - t.pos);
    holder = t.ptr ? g - 1 : g;   // packet 0 starts at stream byte 0 of TS packet 0
  } else {
    holder = g - 1;               // TS packet 0 has PUSI, so g >= 1 here
    t.ptr = 0;
    t.pos = pkt_start(d, holder) - d.td[holder] + 183 + 184 * (q - d.tq[holder] - 1);
    n = min(184u, r.E - t.pos);
    if (g < r.G) n = min(n, pkt_start(d, g) - t.pos);   // 183: the next start begins the next TS packet
  }
  t.stuff = 184 - n - t.pusi;
  t.data_c = 188 - n;
  t.fc = holder / d.P;
  t.j = holder - t.fc * d.P;
  return t;
}

// stream byte x >= t.pos of the TS packet -> frame fc, packet j of the frame, byte i of the packet
__device__ inline void locate(const T2moDev &d, const TsInfo &t, uint32_t x, uint32_t &fc, uint32_t &j, uint32_t &i) {
  fc = t.fc;
  j = t.j;
  uint32_t rel = x - fc * d.B;
  if (rel >= d.B) {   // a TS packet carries at most 184 bytes, a frame has more: one step
    rel -= d.B;
    fc++;
    j = 0;
  }
  while (d.pkt[j + 1].off <= rel) j++;   // pkt[P].off = B > rel
  i = rel - d.pkt[j].off;
}

__device__ inline uint32_t stream_byte(const T2moDev &d, const T2moRun &r, const TsInfo &t, uint32_t x) {
  uint32_t fc, j, i;
  locate(d, t, x, fc, j, i);
  const T2moPkt pk = d.pkt[j];
  const uint32_t g = fc * d.P + j;
  if (i >= pk.T - 4) return (d.crc[g] >> (8 * (pk.T - 1 - i))) & 255;
  return body_byte(d, r, pk, fc, g, i);
}

// byte c of TS packet q
__device__ inline uint32_t ts_byte(const T2moDev &d, const T2moRun &r, const TsInfo &t, uint32_t q, uint32_t c) {
  if (c < 4) {
    if (c == 0) return 0x47;
    if (c == 1) return (t.pusi << 6) | ((uint32_t)d.pid >> 8);
    if (c == 2) return (uint32_t)d.pid & 255;
    return ((t.stuff ? 3u : 1u) << 4) | ((r.cc0 + q) & 15);
  }
  uint32_t a = c - 4;
  if (a < t.stuff) return a == 0 ? t.stuff - 1 : a == 1 ? 0 : 0xFF;
  a -= t.stuff;
  if (t.pusi) {
    if (a == 0) return t.ptr;
    a--;
  }
  return stream_byte(d, r, t, t.pos + a);
}

// bytes c .. c + 3 (c + 4 <= 188): one or two aligned words of the source where all four are bytes of one BBFRAME or
// auxiliary payload and the words lie inside it, bytes otherwise
__device__ inline uint32_t ts_word(const T2moDev &d, const T2moRun &r, const TsInfo &t, uint32_t q, uint32_t c) {
  if (c >= t.data_c) {
    uint32_t fc, j, i, slo, shi;
    locate(d, t, t.pos + (c - t.data_c), fc, j, i);
    const T2moPkt pk = d.pkt[j];
    pkt_source_span(pk, slo, shi);
    if (i >= slo && i + 4 <= shi) {
      const uint8_t *base = pkt_source(d, r, pk, fc), *src = base + (i - slo);
      const uint32_t sh = (uint32_t)((uintptr_t)src & 3);
      const uint8_t *a = src - sh;
      if (sh == 0) return *(const uint32_t *)a;
      if (a >= base && a + 8 <= base + (shi - slo)) {
        const uint32_t lo = *(const uint32_t *)a, hi = *(const uint32_t *)(a + 4);
        return (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
      }
    }
  }
  uint32_t w = 0;
  for (uint32_t k = 0; k < 4; k++) w |= ts_byte(d, r, t, q, c + k) << (8 * k);
  return w;
}

__global__ __launch_bounds__(256) void t2mi_out_emit(T2moDev d, T2moRun r) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nruns = (r.N + EMIT_RUN - 1) / EMIT_RUN;
  // 188 = 47 x 4: every TS packet has the output pointer's phase.  head bytes up to the first aligned word, nwords
  // aligned words, tail bytes after them
  const uint32_t head = (uint32_t)((4 - ((uintptr_t)r.out & 3)) & 3), nwords = (188 - head) / 4;
  const uint32_t tail = 188 - head - 4 * nwords;
  for (uint32_t run = blockIdx.x * 4 + (threadIdx.x >> 6); run < nruns; run += gridDim.x * 4) {
    const uint32_t q0 = run * EMIT_RUN, q1 = min(r.N, q0 + EMIT_RUN);
    uint32_t g = 0, hi = r.G;   // the first g < G with tq[g] >= q0, or G
    while (g < hi) {
      const uint32_t mid = (g + hi) >> 1;
      if (d.tq[mid] < q0) g = mid + 1;
      else hi = mid;
    }
    for (uint32_t q = q0; q < q1; q++) {
      while (g < r.G && d.tq[g] < q) g++;
      const TsInfo t = ts_info(d, r, q, g);
      uint8_t *dst = r.out + (size_t)q * 188;
      if (lane < nwords) {
        *(uint32_t *)(dst + head + 4 * lane) = ts_word(d, r, t, q, head + 4 * lane);
      } else if (lane == 62) {
        for (uint32_t c = 0; c < head; c++) dst[c] = (uint8_t)ts_byte(d, r, t, q, c);
      } else if (lane == 63) {
        for (uint32_t c = 188 - tail; c < 188; c++) dst[c] = (uint8_t)ts_byte(d, r, t, q, c);
      }
    }
  }
}

}  // namespace

void t2mo_host_tables(uint32_t *tab) {
  crc32m_host_tables(tab, T2MO_MAX_T + 1);
}

void t2mo_host_walk(const T2moDev &d, const T2moPkt *pkt, std::vector<uint32_t> &tq, std::vector<uint8_t> &td,
                    T2moFrames &fr) {
  const size_t G = (size_t)d.max_frames * d.P;
  tq.assign(G + 1, 0);
  td.assign(G + 1, 0);
  fr.q0.assign(d.max_frames + 1, 0);
  fr.d0.assign(d.max_frames + 1, 0);
  fr.pusi.assign(d.max_frames + 1, 0);
  // the TS packet q that holds the current start s carries stream bytes [pos, pos + 183): it has a pointer_field
  uint64_t pos = 0, s = 0;
  uint32_t q = 0, npusi = 0;
  for (size_t g = 0;; g++) {
    const uint32_t j = (uint32_t)(g % d.P);
    tq[g] = q;
    td[g] = (uint8_t)(s - pos);
    if (j == 0) {
      const size_t f = g / d.P;
      fr.q0[f] = q;
      fr.d0[f] = td[g];
      fr.pusi[f] = npusi;   // the PUSI packets before this start's own (a call of f frames ends before it)
    }
    if (g == 0 || tq[g] != tq[g - 1]) npusi++;
    if (g == G) break;
    s += pkt[j].T;
    if (s - pos > 182) {
      // after the PUSI packet the packets carry 184 bytes each up to the one the next start lies in; a start on
      // that packet's byte 183 shortens it, and the start begins the packet after it
      const uint64_t pos1 = pos + 183, m = (s - pos1) / 184, rem = (s - pos1) % 184;
      if (rem <= 182) {
        q += 1 + (uint32_t)m;
        pos = pos1 + 184 * m;
      } else {
        q += 2 + (uint32_t)m;
        pos = s;
      }
    }
  }
}

size_t t2mo_layout(T2moDev &d, void *base) {
  LayoutTaker take{base};
  const size_t G = (size_t)d.max_frames * d.P;
  take(d.pkt, d.P + 1);
  take(d.tq, G + 1);
  take(d.td, G + 1);
  take(d.crc, G);
  take(d.tab, T2MO_TAB_WORDS);
  return take.at;
}

hipError_t t2mo_launch(const T2moDev &d, const T2moRun &r, hipStream_t st) {
  if (r.G == 0) return hipSuccess;
  hipLaunchKernelGGL(t2mi_out_crc, dim3(blocks_for(r.G, 4, CRC_MAX_BLOCKS)), dim3(256), 0, st, d, r);
  hipLaunchKernelGGL(t2mi_out_emit, dim3(blocks_for(r.N, 4 * EMIT_RUN, EMIT_MAX_BLOCKS)), dim3(256), 0, st, d, r);
  return hipGetLastError();
}

}  // namespace t2
