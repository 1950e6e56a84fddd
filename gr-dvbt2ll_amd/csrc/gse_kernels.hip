// GSE encapsulation (TS 102 606-1) on gfx950: a device buffer of PDUs and an offset table -> normal-mode BBFRAMEs.
// Semantics: include/dvbt2ll_hip.h; tests/gse_ref.py is the sequential restatement every output is compared with.
//
// A PDU is fragmented only where a BBFRAME ends, so where a packet lands depends on every PDU before it through one
// state: u, the bytes used in the open data field (0 .. D - 1; a frame with u = D is closed).  A PDU maps (u, frames
// closed) to (u', frames closed'); everything a fragmented PDU does to the frames after its first lies inside its own
// map, and such maps compose.  Passes of one run, all on the caller's stream:
//   measure    one lane per PDU: validity, Protocol Type, length
//   maps       per tile of GSE_TILE PDUs, one lane per entry state u walks the tile with the lengths in LDS and stores
//              (frames closed << 13 | exit state): a table of D words per tile
//   chain      one lane follows the tables from tile to tile, one dependent load per tile: each tile's entry
//   walk       one workgroup per tile walks it from its entry: per PDU the frame and offset of its first packet;
//              the fragmented PDUs are listed
//   crc        only fragmented PDUs carry a CRC-32: a wavefront each, lanes take contiguous chunks through the byte
//              table and the chunks are joined with x^(8 n) mod G
//   emit       one workgroup per BBFRAME: a lane finds what the frame begins with and which PDUs start in it (two
//              searches in the per-PDU frames) and builds the header; then a lane per 16 output bytes finds its
//              packet (a search in the per-PDU offsets) and gathers, storing a head up to the first 16-byte boundary,
//              then uint4s
//   count      the resume position, and the counters of the PDUs before it
// The cut (the closed frames that capacity allows, the flush frame) is arithmetic on the chain's totals: emit and
// count each work it out for themselves.
#include "gse_kernels.h"

#include <algorithm>

#include "crc32_mpeg2.h"
#include "host_util.h"

namespace t2 {

namespace {

enum : uint32_t { G_LEN = 0xFFFFu, G_SKIP_TYPE = 1u << 30, G_SKIP_LEN = 1u << 31 };
enum : int { C_T = 0, C_U = 1, C_S = 2, C_NFRAG = 3 };   // d.ctl
constexpr uint32_t ST_MASK = (1u << GSE_STATE_BITS) - 1;

uint32_t tiles_of(uint32_t n) { return std::max<uint32_t>(1, (n + GSE_TILE - 1) / GSE_TILE); }

// ------------------------------------------------------------------------------------------ measure
__global__ __launch_bounds__(256) void gse_measure(GseDev d, GseRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= r.n) return;
  const uint32_t o0 = r.off[r.i0 + i], o1 = r.off[r.i0 + i + 1];
  uint32_t n = 0, flags = 0, type = 0;
  if (o1 <= o0 || o1 > r.pdu_len || o1 - o0 > (uint32_t)GSE_MAX_PDU - d.L) flags = G_SKIP_LEN;
  else {
    if (r.type) type = r.type[r.i0 + i];
    else {
      const uint32_t nib = r.pdu[o0] >> 4;
      if (nib == 4) type = 0x0800;
      else if (nib == 6) type = 0x86DD;
      else flags = G_SKIP_TYPE;
    }
    if (!flags) n = o1 - o0;
  }
  // the start's pdu_byte counts where it names a byte 1 .. len - 1 of a valid PDU
  if (i == 0) d.ctl[C_S] = n && r.pdu_byte >= 1 && r.pdu_byte + 1 <= n ? r.pdu_byte : 0;
  d.len[i] = n | flags;
  d.typ[i] = (uint16_t)type;
}

// ------------------------------------------------------------------------------------------ the placement rule
// a fresh PDU of len bytes met with u bytes used: true when the frame is closed as it is and the PDU starts the next
__device__ inline bool gse_moves_on(uint32_t len, uint32_t u, uint32_t D, uint32_t L) {
  const uint32_t free = D - u;
  return free < 4 + L + len && free < 8 + L;
}

// an open PDU with rem bytes left at a frame's start: the PDU bytes this frame takes; end: with the CRC
__device__ inline uint32_t gse_open_piece(uint32_t rem, uint32_t D, bool &end) {
  end = rem + 7 <= D;
  if (end) return rem;
  return D - 3 < rem - 1 ? D - 3 : rem - 1;   // the end fragment keeps at least one PDU byte
}

// one PDU of len bytes (0: a skipped one) entered in state u with fr frames closed; s > 0: it is open from an
// earlier call, s bytes sent (u is 0 then)
__device__ inline void gse_step(uint32_t len, uint32_t s, uint32_t D, uint32_t L, uint32_t &u, uint32_t &fr) {
  if (!len) return;
  uint32_t rem;
  if (s) rem = len - s;
  else {
    const uint32_t p = 4 + L + len;
    if (gse_moves_on(len, u, D, L)) { fr++; u = 0; }
    const uint32_t free = D - u;
    if (free >= p) {
      u += p;
      if (u == D) { fr++; u = 0; }
      return;
    }
    rem = len - (free - 7 - L);   // the first fragment fills the frame
    fr++;
  }
  for (;;) {
    bool end;
    const uint32_t piece = gse_open_piece(rem, D, end);
    if (end) break;
    rem -= piece;
    fr++;
  }
  u = rem + 7;
  if (u == D) { fr++; u = 0; }
}

// the tile's PDU lengths into LDS
__device__ inline void gse_tile_lens(const GseDev &d, uint32_t N, uint32_t base, uint16_t *ln) {
  for (uint32_t k = threadIdx.x; k < (uint32_t)GSE_TILE; k += blockDim.x) {
    const uint32_t i = base + k;
    ln[k] = (uint16_t)(i < N ? d.len[i] & G_LEN : 0);
  }
  __syncthreads();
}

// grid: (tiles, groups of 256 entry states)
__global__ __launch_bounds__(256) void gse_maps(GseDev d, uint32_t N) {
  __shared__ uint16_t ln[GSE_TILE];
  const uint32_t base = blockIdx.x * GSE_TILE;
  gse_tile_lens(d, N, base, ln);
  const uint32_t u0 = blockIdx.y * 256 + threadIdx.x;
  if (u0 >= d.D) return;
  const uint32_t s = base == 0 ? d.ctl[C_S] : 0;
  uint32_t u = s ? 0 : u0, fr = 0;
  gse_step(ln[0], s, d.D, d.L, u, fr);
  for (int k = 1; k < GSE_TILE; k++) gse_step(ln[k], 0, d.D, d.L, u, fr);
  d.maps[(size_t)blockIdx.x * d.D + u0] = (fr << GSE_STATE_BITS) | u;
}

// one dependent load per tile
__global__ __launch_bounds__(64) void gse_chain(GseDev d, uint32_t ntiles) {
  if (threadIdx.x) return;
  uint32_t u = 0, fr = 0;
  for (uint32_t t = 0; t < ntiles; t++) {
    d.ent_u[t] = u;
    d.ent_fr[t] = fr;
    const uint32_t f = d.maps[(size_t)t * d.D + u];
    u = f & ST_MASK;
    fr += f >> GSE_STATE_BITS;
  }
  d.ctl[C_T] = fr;
  d.ctl[C_U] = u;
}

// PDU i with its first packet at offset at: does it take more than one packet?
__device__ inline bool gse_fragmented(const GseDev &d, uint32_t i, uint32_t len, uint32_t at, uint32_t s) {
  return len && ((i == 0 && s) || 4 + d.L + len > d.D - at);
}

__global__ __launch_bounds__(256) void gse_walk(GseDev d, uint32_t N) {
  __shared__ uint16_t ln[GSE_TILE];
  __shared__ uint32_t fr_s[GSE_TILE];
  __shared__ uint16_t at_s[GSE_TILE];
  const uint32_t s = d.ctl[C_S], base = blockIdx.x * GSE_TILE;
  gse_tile_lens(d, N, base, ln);
  if (threadIdx.x == 0) {
    uint32_t u = d.ent_u[blockIdx.x], fr = d.ent_fr[blockIdx.x];
    for (int k = 0; k < GSE_TILE; k++) {
      const uint32_t open = k == 0 && base == 0 ? s : 0;
      const bool on = ln[k] && !open && gse_moves_on(ln[k], u, d.D, d.L);
      fr_s[k] = on ? fr + 1 : fr;
      at_s[k] = (uint16_t)(on ? 0 : u);
      gse_step(ln[k], open, d.D, d.L, u, fr);
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < (uint32_t)GSE_TILE; k += 256) {
    const uint32_t i = base + k;
    if (i >= N) continue;
    d.frm[i] = fr_s[k];
    d.at[i] = at_s[k];
    if (gse_fragmented(d, i, ln[k], at_s[k], s)) d.frg[atomicAdd(&d.ctl[C_NFRAG], 1u)] = i;   // at most N entries
  }
}

// ------------------------------------------------------------------------------------------ CRC-32
// byte k < 4 + L of what the CRC covers before the PDU: Total Length, Protocol Type, Label
__device__ inline uint32_t gse_covered_byte(const GseDev &d, uint32_t len, uint32_t type, uint32_t k) {
  const uint32_t total = 2 + d.L + len;
  if (k == 0) return total >> 8;
  if (k == 1) return total & 255;
  if (k == 2) return type >> 8;
  if (k == 3) return type & 255;
  return d.label[k - 4];
}

// covered bytes [lo, hi)
__device__ inline uint32_t crc_span(const GseDev &d, uint32_t crc, uint32_t len, uint32_t type, const uint8_t *pdu,
                                    uint32_t lo, uint32_t hi, const uint32_t *tab) {
  const uint32_t hl = 4 + d.L;
  for (; lo < hi && lo < hl; lo++) crc = crc32m_byte(crc, gse_covered_byte(d, len, type, lo), tab);
  if (lo < hi) crc = crc32m_run(crc, pdu + (lo - hl), hi - lo, tab);
  return crc;
}

// the fragmented PDUs, as walk listed them: a wavefront each; past GSE_CRC_BLOCKS x 4 of them a wavefront takes more
// than one
__global__ __launch_bounds__(256) void gse_crc(GseDev d, GseRun r) {
  __shared__ uint32_t tab[256];
  tab[threadIdx.x] = d.tab[threadIdx.x];
  __syncthreads();
  const uint32_t *xp = d.tab + 256;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t count = d.ctl[C_NFRAG] < r.n ? d.ctl[C_NFRAG] : r.n;
  for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < count; w += gridDim.x * 4) {
    const uint32_t j = d.frg[w];
    if (j >= r.n) continue;
    const uint32_t len = d.len[j] & G_LEN, tj = d.typ[j], oj = r.off[r.i0 + j];
    if (!len) continue;
    const uint32_t T = 4 + d.L + len;
    int lo, hi;
    const uint32_t c = crc32m_wave_chunk(lane, T, lo, hi);
    uint32_t crc = 0;
    if (hi > lo) crc = crc_span(d, 0, len, tj, r.pdu + oj, (uint32_t)lo, (uint32_t)hi, tab);
    crc = crc32m_wave_join(crc, lane, c, T, xp);
    if (lane == 0) d.crc[j] = crc;
  }
}

// ------------------------------------------------------------------------------------------ the cut, positions
struct GseCut {
  uint32_t T, q, s;    // frames closed, the end state (an open frame when not 0), the start's pdu_byte as taken
  uint32_t E;          // frames emitted
  bool all;            // nothing is left
};

__device__ inline GseCut gse_cut(const GseDev &d, const GseRun &r) {
  GseCut c;
  c.T = d.ctl[C_T];
  c.q = d.ctl[C_U];
  c.s = d.ctl[C_S];
  const uint32_t det = c.T + (c.q && r.flush ? 1 : 0);   // the open frame is emitted by a flush only
  c.E = det < r.cap ? det : r.cap;
  c.all = c.E == det && (c.q == 0 || r.flush);
  return c;
}

// what frame f holds: R > 0 bytes left of PDU jc, coff of its bytes sent, at the frame's start; [jn, jend): the PDUs
// whose first packet lies in the frame; used: the bytes of its packets
struct GseRec { uint32_t jc, R, coff, jn, jend, cs, used; };

__device__ inline uint32_t gse_first_frame_at_least(const GseDev &d, uint32_t N, uint32_t f) {
  uint32_t lo = 0, hi = N;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d.frm[mid] < f) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ inline GseRec gse_locate(const GseDev &d, uint32_t N, uint32_t s, uint32_t f) {
  const uint32_t lo = gse_first_frame_at_least(d, N, f);
  GseRec q{0, 0, 0, lo, lo, 0, 0};
  uint32_t j = 0, rem = 0, m = 0;
  bool have = false;
  if (f == 0) {
    if (s && N) {   // the PDU an earlier call left open
      have = true;
      rem = (d.len[0] & G_LEN) - s;
      q.jn = 1;
    }
  } else if (lo > 0) {
    // the PDU before: only a valid one moves the frame count, and only a fragmented one runs on into f
    j = lo - 1;
    const uint32_t len = d.len[j] & G_LEN;
    if (j == 0 && s) {
      have = true;
      rem = len - s;
      m = f;
    } else if (gse_fragmented(d, j, len, d.at[j], 0)) {
      have = true;
      rem = len - (d.D - d.at[j] - 7 - d.L);
      m = f - d.frm[j] - 1;
    }
  }
  if (have) {
    for (; m && rem; m--) {   // the frames between: continuations, or the end
      bool end;
      const uint32_t piece = gse_open_piece(rem, d.D, end);
      rem -= piece;
    }
    if (rem) {
      bool end;
      const uint32_t piece = gse_open_piece(rem, d.D, end);
      q.jc = j;
      q.R = rem;
      q.coff = (d.len[j] & G_LEN) - rem;
      q.cs = (end ? 7 : 3) + piece;
    }
  }
  return q;
}

// the full record of an emitted frame: the PDUs that start in it, the bytes used
__device__ inline GseRec gse_record(const GseDev &d, uint32_t N, uint32_t s, uint32_t f) {
  GseRec q = gse_locate(d, N, s, f);
  uint32_t lo = q.jn, hi = N;   // the first PDU whose frame is past f
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d.frm[mid] <= f) lo = mid + 1;
    else hi = mid;
  }
  q.jend = lo;
  q.used = q.cs;
  if (q.jend > q.jn) {
    const uint32_t x = q.jend - 1, len = d.len[x] & G_LEN, at = d.at[x];
    // a skipped PDU stands at the state the valid ones before it left
    q.used = !len ? at : gse_fragmented(d, x, len, at, 0) ? d.D : at + 4 + d.L + len;
  }
  return q;
}

// ------------------------------------------------------------------------------------------ emit
// data-field byte b < used of the frame: the byte, or with run > 0 the first of run PDU bytes that lie at src
__device__ inline uint32_t gse_field_byte(const GseDev &d, const GseRun &r, const GseRec &q, uint32_t b,
                                          const uint8_t *&src, uint32_t &run) {
  run = 0;
  if (b < q.cs) {   // the continuation or end fragment of jc
    const bool end = q.R + 7 <= d.D;
    const uint32_t piece = q.cs - (end ? 7 : 3), glen = q.cs - 2;
    if (b == 0) return (end ? 0x40u : 0u) | 0x30u | (glen >> 8);
    if (b == 1) return glen & 255;
    if (b == 2) return (r.frag_id + q.jc) & 255;
    if (b - 3 < piece) {
      src = r.pdu + r.off[r.i0 + q.jc] + q.coff + (b - 3);
      run = piece - (b - 3);
      return *src;
    }
    return (d.crc[q.jc] >> (8 * (q.cs - 1 - b))) & 255;
  }
  uint32_t lo = q.jn, hi = q.jend;   // the last PDU that starts at or before b: a valid one, since b < used
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (d.at[mid] <= b) lo = mid;
    else hi = mid;
  }
  const uint32_t x = lo, len = d.len[x] & G_LEN, at = d.at[x], k = b - at, type = d.typ[x];
  const uint32_t free = d.D - at;
  uint32_t hl, glen, S;
  if (free >= 4 + d.L + len) { hl = 4 + d.L; glen = 2 + d.L + len; S = 0xC0; }
  else { hl = 7 + d.L; glen = free - 2; S = 0x80; }
  if (k >= hl) {
    const uint32_t body = glen + 2 - hl;   // PDU bytes in the packet
    if (k - hl >= body) return 0;          // cannot be (b < used)
    src = r.pdu + r.off[r.i0 + x] + (k - hl);
    run = body - (k - hl);
    return *src;
  }
  if (k == 0) return S | (d.lt << 4) | (glen >> 8);
  if (k == 1) return glen & 255;
  uint32_t h = k - 2;
  if (S == 0x80) {   // a first fragment: Frag ID and Total Length come first
    const uint32_t total = 2 + d.L + len;
    if (h == 0) return (r.frag_id + x) & 255;
    if (h == 1) return total >> 8;
    if (h == 2) return total & 255;
    h -= 3;
  }
  if (h == 0) return type >> 8;
  if (h == 1) return type & 255;
  return d.label[h - 2];
}

// byte o of the frame
__device__ inline uint32_t gse_out_byte(const GseDev &d, const GseRun &r, const GseRec &q, const uint8_t *hdr,
                                        uint32_t o) {
  if (o < 10) return hdr[o];
  if (o - 10 >= q.used) return 0;
  const uint8_t *src;
  uint32_t run;
  return gse_field_byte(d, r, q, o - 10, src, run);
}

// bytes o .. o + 3 of the frame (all inside it): two aligned words of the PDU buffer where all four are bytes of one
// PDU and the words lie inside the buffer, bytes otherwise
__device__ inline uint32_t gse_out_word(const GseDev &d, const GseRun &r, const GseRec &q, const uint8_t *hdr,
                                        uint32_t o) {
  if (o >= 10 && o - 10 < q.used) {
    const uint8_t *src;
    uint32_t run;
    const uint32_t b0 = gse_field_byte(d, r, q, o - 10, src, run);
    if (run >= 4) {
      const uint32_t sh = (uint32_t)((uintptr_t)src & 3);
      const uint8_t *a = src - sh;
      if (sh == 0) return *(const uint32_t *)a;
      if (a >= r.pdu && a + 8 <= r.pdu + r.pdu_len) {
        const uint32_t lo = *(const uint32_t *)a, hi = *(const uint32_t *)(a + 4);
        return (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
      }
    }
    uint32_t w = b0;
    for (uint32_t k = 1; k < 4; k++) w |= gse_out_byte(d, r, q, hdr, o + k) << (8 * k);
    return w;
  }
  uint32_t w = 0;
  for (uint32_t k = 0; k < 4; k++) w |= gse_out_byte(d, r, q, hdr, o + k) << (8 * k);
  return w;
}

// The grid covers the frames that PDUs lying side by side can become (gse_frame_estimate); where the offsets make
// valid PDUs overlap and the frames are more, a workgroup takes more than one: its second trip begins at the loop's
// second pass
__global__ __launch_bounds__(256) void gse_emit(GseDev d, GseRun r) {
  __shared__ GseRec rec;
  __shared__ uint8_t hdr[16];
  __shared__ uint32_t npk;
  const GseCut c = gse_cut(d, r);
  for (uint32_t f = blockIdx.x; f < c.E; f += gridDim.x) {
    __syncthreads();   // the trip before no longer reads rec
    if (threadIdx.x == 0) {
      const GseRec q = gse_record(d, r.n, c.s, f);
      rec = q;
      npk = q.R ? 1 : 0;
      const uint32_t dfl = 8 * q.used;
      const uint8_t h[9] = {(uint8_t)(d.matype >> 8), (uint8_t)d.matype, 0, 0, (uint8_t)(dfl >> 8), (uint8_t)dfl, 0, 0, 0};
      uint32_t crc = 0;
      for (int k = 0; k < 9; k++) {
        hdr[k] = h[k];
        crc ^= h[k];
        for (int bit = 0; bit < 8; bit++) crc = ((crc << 1) ^ ((crc & 0x80) ? 0xD5u : 0u)) & 0xFF;
      }
      hdr[9] = (uint8_t)crc;   // CRC-8 XOR MODE, MODE = 0: normal mode
      if (d.D > q.used) atomicAdd(&d.res[GSE_R_PAD], (unsigned long long)(d.D - q.used));
    }
    __syncthreads();
    const GseRec q = rec;
    uint32_t mine = 0;
    for (uint32_t x = q.jn + threadIdx.x; x < q.jend; x += 256) mine += (d.len[x] & G_LEN) ? 1 : 0;
    if (mine) atomicAdd(&npk, mine);
    // the frame's bytes [0, Lb) at dst: chunk 0 runs up to the first 16-byte boundary, the others are 16 bytes (the
    // last shorter)
    uint8_t *dst = r.out + (size_t)f * d.Lb;
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > d.Lb) head = d.Lb;
    const uint32_t nchunks = 1 + (d.Lb - head + 15) / 16;
    for (uint32_t cidx = threadIdx.x; cidx < nchunks; cidx += 256) {
      const uint32_t lo = cidx ? head + (cidx - 1) * 16 : 0;
      const uint32_t hi = cidx ? (d.Lb < lo + 16 ? d.Lb : lo + 16) : head;
      if (hi <= lo) continue;
      if (cidx && hi - lo == 16) {
        uint32_t w[4];
        for (uint32_t k = 0; k < 4; k++) w[k] = gse_out_word(d, r, q, hdr, lo + 4 * k);
        *(uint4 *)(dst + lo) = make_uint4(w[0], w[1], w[2], w[3]);
      } else {
        for (uint32_t o = lo; o < hi; o++) dst[o] = (uint8_t)gse_out_byte(d, r, q, hdr, o);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0 && npk) atomicAdd(&d.res[GSE_R_PACKETS], (unsigned long long)npk);
  }
}

// ------------------------------------------------------------------------------------------ resume, counters
__global__ __launch_bounds__(256) void gse_count(GseDev d, GseRun r) {
  __shared__ uint32_t hist[4], found;
  if (threadIdx.x < 4) hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) found = r.n;
  __syncthreads();
  const GseCut c = gse_cut(d, r);
  uint32_t jr = r.n, sb = 0;   // the resume position: the PDU (in this run's indices), its bytes sent
  if (!c.all) {
    const GseRec ps = gse_locate(d, r.n, c.s, c.E);
    if (ps.R) {
      jr = ps.jc;
      sb = ps.coff;
    } else {
      // the first valid PDU from ps.jn on: the workgroup looks at 256 at a time
      for (uint32_t base = ps.jn; base < r.n; base += 256) {
        const uint32_t x = base + threadIdx.x;
        if (x < r.n && (d.len[x] & G_LEN)) atomicMin(&found, x);
        __syncthreads();
        const uint32_t f = found;
        __syncthreads();
        if (f < r.n) break;
      }
      jr = found;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    d.res[GSE_R_PDU] = r.i0 + jr;
    d.res[GSE_R_PDU_BYTE] = sb;
    d.res[GSE_R_FRAG_ID] = (r.frag_id + jr) & 255;
    d.res[GSE_R_PDUS_IN] = jr;
    d.res[GSE_R_BBFRAMES] = c.E;
    d.res[GSE_R_FLUSHED] = r.flush && c.q && c.E == c.T + 1 ? 1 : 0;
  }
  // past GSE_COUNT_BLOCKS x 256 PDUs a lane takes more than one
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < jr; i += gridDim.x * 256) {
    const uint32_t w = d.len[i], len = w & G_LEN;
    const int k = len ? (gse_fragmented(d, i, len, d.at[i], c.s) ? 1 : 0) : (w & G_SKIP_LEN) ? 2 : 3;
    atomicAdd(&hist[k], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 4 && hist[threadIdx.x]) {
    const int at[4] = {GSE_R_COMPLETE, GSE_R_FRAGMENTED, GSE_R_SKIPPED_LEN, GSE_R_SKIPPED_TYPE};
    atomicAdd(&d.res[at[threadIdx.x]], (unsigned long long)hist[threadIdx.x]);
  }
}

}  // namespace

void gse_host_tables(uint32_t *tab) {
  crc32m_host_tables(tab, GSE_TAB_WORDS - 256);
}

size_t gse_layout(GseDev &d, void *base) {
  LayoutTaker take{base};
  const size_t n = std::max<uint32_t>(d.max_pdus, 1), nt = tiles_of(d.max_pdus);
  take(d.res, GSE_R_WORDS + 2);
  d.ctl = base ? (uint32_t *)(d.res + GSE_R_WORDS) : nullptr;
  take(d.len, n);
  take(d.typ, n);
  take(d.crc, n);
  take(d.frg, n);
  take(d.frm, n);
  take(d.at, n);
  take(d.maps, nt * d.D);
  take(d.ent_u, nt);
  take(d.ent_fr, nt);
  take(d.tab, GSE_TAB_WORDS);
  return take.at;
}

uint64_t gse_frame_estimate(const GseDev &d, uint64_t pdu_len, uint64_t n) {
  // a closed frame holds at least D - 14 - L bytes of PDUs and their 4 + L bytes each: an end fragment adds 7 and the
  // frame may then close with up to 7 + L unused; a continuation adds 3 and leaves up to 4; a first fragment adds 3
  return (pdu_len + (4 + d.L) * n) / (d.D - 14 - d.L) + 2;
}

uint64_t gse_frame_limit(const GseDev &d, uint64_t pdu_len, uint64_t n) {
  // every PDU may be the whole buffer, or the longest a packet takes
  const uint64_t one = std::min<uint64_t>(pdu_len, GSE_MAX_PDU - d.L) + 4 + d.L;
  return n * (one / (d.D - 14 - d.L) + 2) + 2;
}

hipError_t gse_launch(const GseDev &d, const GseRun &r, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, (GSE_R_WORDS + 2) * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const uint32_t nb = std::max<uint32_t>(1, (r.n + 255) / 256), nt = tiles_of(r.n);
  hipLaunchKernelGGL(gse_measure, dim3(nb), dim3(256), 0, st, d, r);
  hipLaunchKernelGGL(gse_maps, dim3(nt, (d.D + 255) / 256), dim3(256), 0, st, d, r.n);
  hipLaunchKernelGGL(gse_chain, dim3(1), dim3(64), 0, st, d, nt);
  hipLaunchKernelGGL(gse_walk, dim3(nt), dim3(256), 0, st, d, r.n);
  // a fragmented PDU ends a frame, or is the one an earlier call left open
  const uint64_t est = gse_frame_estimate(d, r.pdu_len, r.n);
  const uint32_t nfrag = (uint32_t)std::min<uint64_t>(r.n, est + 1);
  if (nfrag)
    hipLaunchKernelGGL(gse_crc, dim3(std::min<uint32_t>(GSE_CRC_BLOCKS, (nfrag + 3) / 4)), dim3(256), 0, st, d, r);
  // emit's grid is sized for PDUs that lie side by side and strides where overlapping ones make more frames
  const uint32_t ne = (uint32_t)std::min<uint64_t>(r.cap, est);
  if (ne) hipLaunchKernelGGL(gse_emit, dim3(ne), dim3(256), 0, st, d, r);
  hipLaunchKernelGGL(gse_count, dim3(std::min<uint32_t>(GSE_COUNT_BLOCKS, nb)), dim3(256), 0, st, d, r);
  return hipGetLastError();
}

}  // namespace t2
