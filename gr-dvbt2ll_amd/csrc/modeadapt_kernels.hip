// Mode adaptation with null-packet deletion (EN 302 755 5.1.4, 5.1.7) on gfx950: a device buffer of TS packets ->
// packed high-efficiency-mode BBFRAMEs.  Semantics: include/dvbt2ll_hip.h; tests/modeadapt_ref.py is the sequential
// restatement every output is compared with.
//
// The output length depends on the data, so the run is scans, a compaction and a gather.  Passes of one run, all on
// the caller's stream, sized by host-known upper bounds; what a pass needs of the data-dependent sizes it reads from
// the scans' totals on the device:
//   classify   one lane per TS packet: selected (PID against the mask staged in LDS), sync flag
//   scan M     exclusive max-scan of (selected ? index + 1 : 0): the last selected packet before each packet
//   runpos     one lane per TS packet: its position r in its run of nulls, kept (r % 256 == 255) / deleted,
//              transmitted, and a transmitted packet's DNP from the packet before it
//   scan T     exclusive sum of the transmitted flags: the unit index
//   compact    per transmitted packet: unit -> (packet index, DNP)
//   emit       one workgroup per BBFRAME: the header (CRC-8 through a table in LDS), the data field gathered from
//              unit byte -> (packet, byte) and stored as a head up to the destination's first 16-byte boundary, then
//              16-byte stores
//   count      the resume position, and the counters of the TS packets before it
// The cut (whole BBFRAMEs that input and capacity allow, the flush frame) is arithmetic on scan T's total: emit and
// count each work it out for themselves.
#include "modeadapt_kernels.h"

#include <algorithm>

#include "dev_scan.h"
#include "host_util.h"

namespace t2 {

// found by the scan templates through argument-dependent lookup
__host__ __device__ inline MaMax operator+(const MaMax &a, const MaMax &b) { return MaMax{a.v > b.v ? a.v : b.v}; }

namespace {

enum : uint32_t { MA_SEL = 1, MA_SYNC_ERR = 2 };
enum : uint32_t { MA_TX = 0x100 };
constexpr uint32_t PKT_MASK = 0xFFFFFFu;   // a run has fewer than 2^31 / 188 < 2^24 packets

// ------------------------------------------------------------------------------------------ device-wide scan
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void modeadapt_scan_reduce(const T *in, T *tile, uint32_t n,
                                                                      const uint32_t *n_dev) {
  __shared__ T lds[SCAN_THREADS];
  scan_reduce_body(in, tile, n, n_dev, lds);
}
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void modeadapt_scan_tiles(T *tile, uint32_t ntiles) {
  __shared__ T lds[2 * SCAN_THREADS];
  scan_tiles_body(tile, ntiles, lds);
}
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void modeadapt_scan_apply(T *data, const T *tile, uint32_t n,
                                                                     const uint32_t *n_dev) {
  __shared__ T lds[2 * SCAN_THREADS];
  scan_apply_body(data, tile, n, n_dev, lds);
}
template <class T>
hipError_t scan_exclusive(T *data, T *tile, uint32_t n, hipStream_t st) {
  return scan_exclusive(ScanKernels<T>{modeadapt_scan_reduce<T>, modeadapt_scan_tiles<T>, modeadapt_scan_apply<T>}, data,
                        tile, n, nullptr, st);
}

// ------------------------------------------------------------------------------------------ per-packet passes
__host__ __device__ inline bool forced_first(const MaRun &r) { return r.unit_byte > 0 || r.dnp > 0; }

// packet i of the run: flags and the max-scan's input.  mask: 256 words (LDS in the kernel)
__host__ __device__ inline void classify_one(const MaDev &d, const MaRun &r, const uint32_t *mask, uint32_t i) {
  const uint8_t *b = r.ts + (size_t)(r.i0 + i) * 188;
  uint32_t b0, b1, b2;
  if (((uintptr_t)b & 3) == 0) {   // 188 = 4 x 47: every packet of an aligned buffer starts on a word
    const uint32_t w = *(const uint32_t *)b;
    b0 = w & 255, b1 = (w >> 8) & 255, b2 = (w >> 16) & 255;
  } else {
    b0 = b[0], b1 = b[1], b2 = b[2];
  }
  const uint32_t pid = ((b1 & 0x1F) << 8) | b2;
  bool sel = true;
  if (d.npd) sel = pid != 0x1FFF && (!d.has_mask || ((mask[pid >> 5] >> (pid & 31)) & 1));
  d.flags[i] = (uint8_t)((sel ? MA_SEL : 0) | (b0 != 0x47 ? MA_SYNC_ERR : 0));
  d.mscan[i] = MaMax{sel || (i == 0 && forced_first(r)) ? i + 1 : 0};
}

// the inclusive max at packet i from the exclusive scan: index + 1 of the last selected packet at or before i
__host__ __device__ inline uint32_t last_selected(const MaDev &d, const MaRun &r, uint32_t i) {
  const bool here = (d.flags[i] & MA_SEL) || (i == 0 && forced_first(r));
  return here ? i + 1 : d.mscan[i].v;
}

__host__ __device__ inline void runpos_one(const MaDev &d, const MaRun &r, uint32_t i) {
  const uint32_t m = last_selected(d, r, i);
  // a null's position in its run is i - m; the one at 255 mod 256 is kept
  const bool tx = m == i + 1 || ((i - m) & 255) == 255;
  uint32_t dnp = 0;
  if (i == 0) dnp = r.dnp;
  else {
    const uint32_t mp = last_selected(d, r, i - 1);
    if (mp != i) dnp = (i - mp) & 255;   // the packet before is null number i - 1 - mp: deleted unless it was kept
  }
  d.info[i] = (uint16_t)(tx ? MA_TX | dnp : 0);
  d.tscan[i] = tx;
}

__host__ __device__ inline void compact_one(const MaDev &d, uint32_t i) {
  const uint32_t w = d.info[i];
  if (w & MA_TX) d.unit[d.tscan[i]] = i | ((w & 255) << 24);
}

// ------------------------------------------------------------------------------------------ the cut
struct MaCut {
  uint32_t total;      // unit-stream bytes of the call
  uint32_t whole;      // BBFRAMEs emitted with a full data field
  uint32_t rem;        // bytes of the flush frame (0: none)
  bool flushed;        // the flush was honoured: everything is consumed
};

__host__ __device__ inline MaCut cut_of(const MaDev &d, const MaRun &r, uint32_t nunits) {
  const uint32_t U = d.npd ? 188 : 187;
  MaCut c;
  c.total = nunits ? nunits * U - r.unit_byte : 0;
  const uint32_t whole = c.total / d.D, rem = c.total - whole * d.D;
  c.flushed = r.flush && whole + (rem ? 1 : 0) <= r.cap;
  c.whole = whole < r.cap ? whole : r.cap;
  c.rem = c.flushed ? rem : 0;
  return c;
}

// ------------------------------------------------------------------------------------------ emit
template <bool NPD>
__host__ __device__ inline uint32_t data_byte(const MaDev &d, const MaRun &r, uint32_t g) {
  constexpr uint32_t U = NPD ? 188 : 187;
  const uint32_t q = g / U, b = g - q * U, w = d.unit[q], pkt = w & PKT_MASK;
  if (b == 187) return w >> 24;
  if (!(d.flags[pkt] & MA_SEL)) return b == 0 ? 0x1F : b == 2 ? 0x10 : 0xFF;   // a kept null: the null packet
  return r.ts[(size_t)(r.i0 + pkt) * 188 + 1 + b];
}

// byte p of a BBFRAME whose data field holds nbytes bytes from unit-stream offset g0 (in the first unit's
// coordinates); hdr: its 10 header bytes
template <bool NPD>
__host__ __device__ inline uint32_t frame_byte(const MaDev &d, const MaRun &r, const uint8_t *hdr, uint32_t g0,
                                               uint32_t nbytes, uint32_t p) {
  if (p < 10) return hdr[p];
  if (p - 10 < nbytes) return data_byte<NPD>(d, r, g0 + (p - 10));
  return 0;
}

// bytes p .. p + 3: one or two aligned words of the source where all four lie in one selected packet and the words
// lie inside it, bytes otherwise
template <bool NPD>
__host__ __device__ inline uint32_t frame_word(const MaDev &d, const MaRun &r, const uint8_t *hdr, uint32_t g0,
                                               uint32_t nbytes, uint32_t p) {
  constexpr uint32_t U = NPD ? 188 : 187;
  if (p >= 10 && p - 10 + 4 <= nbytes) {
    const uint32_t g = g0 + (p - 10), q = g / U, b = g - q * U, pkt = d.unit[q] & PKT_MASK;
    if (b + 4 <= 187 && (d.flags[pkt] & MA_SEL)) {
      const uint8_t *base = r.ts + (size_t)(r.i0 + pkt) * 188, *src = base + 1 + b;
      const uint32_t sh = (uint32_t)((uintptr_t)src & 3);
      const uint8_t *a = src - sh;
      if (sh == 0) return *(const uint32_t *)a;
      if (a >= base && a + 8 <= base + 188) {
        const uint32_t lo = *(const uint32_t *)a, hi = *(const uint32_t *)(a + 4);
        return (lo >> (8 * sh)) | (hi << (32 - 8 * sh));
      }
    }
  }
  uint32_t w = 0;
  for (uint32_t q = 0; q < 4; q++) w |= frame_byte<NPD>(d, r, hdr, g0, nbytes, p + q) << (8 * q);
  return w;
}

// the 10 header bytes of BBFRAME k
__host__ __device__ inline void frame_header(const MaDev &d, const MaRun &r, const uint32_t *crc, uint32_t g0,
                                             uint32_t nbytes, uint8_t *hdr) {
  const uint32_t U = d.npd ? 188 : 187;
  const uint32_t ph = g0 % U, dist = ph ? U - ph : 0;
  const uint32_t syncd = dist < nbytes ? 8 * dist : 0xFFFF;   // no unit begins in the data field: 0xFFFF
  const uint32_t dfl = 8 * nbytes;
  const uint8_t h[9] = {(uint8_t)(d.matype >> 8), (uint8_t)d.matype, 0, 0, (uint8_t)(dfl >> 8), (uint8_t)dfl, 0,
                        (uint8_t)(syncd >> 8), (uint8_t)syncd};
  uint32_t c = 0;
  for (int q = 0; q < 9; q++) {
    hdr[q] = h[q];
    c = crc[c ^ h[q]];
  }
  hdr[9] = (uint8_t)(c ^ 1);   // CRC-8 XOR MODE, MODE = 1: high-efficiency mode
}

// chunk cidx of BBFRAME k at dst: chunk 0 runs up to dst's first 16-byte boundary, the others are 16 bytes (the last
// one shorter)
template <bool NPD>
__host__ __device__ inline void emit_chunk(const MaDev &d, const MaRun &r, const uint8_t *hdr, uint32_t g0,
                                           uint32_t nbytes, uint8_t *dst, uint32_t head, uint32_t cidx) {
  const uint32_t L = d.L;
  const uint32_t lo = cidx ? head + (cidx - 1) * 16 : 0;
  const uint32_t hi = cidx ? (L < lo + 16 ? L : lo + 16) : head;
  if (hi <= lo) return;
  if (hi - lo == 16 && cidx) {
    uint32_t w[4];
    for (uint32_t q = 0; q < 4; q++) w[q] = frame_word<NPD>(d, r, hdr, g0, nbytes, lo + 4 * q);
    *(uint4 *)(dst + lo) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (uint32_t p = lo; p < hi; p++) dst[p] = (uint8_t)frame_byte<NPD>(d, r, hdr, g0, nbytes, p);
  }
}

__host__ __device__ inline uint32_t head_of(const uint8_t *dst, uint32_t L) {
  const uint32_t h = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
  return h < L ? h : L;
}

// ------------------------------------------------------------------------------------------ resume, counters
// the resume position (thread 0 of the count pass writes it); returns the packets the counters cover
__host__ __device__ inline uint32_t resume_of(const MaDev &d, const MaRun &r, const MaCut &c, uint32_t nunits,
                                              uint32_t *unit_byte, uint32_t *dnp) {
  const uint32_t U = d.npd ? 188 : 187;
  *unit_byte = 0;
  *dnp = 0;
  if (c.flushed) return r.n;
  if (nunits == 0) return 0;
  const uint32_t g = c.whole * d.D + r.unit_byte, q = g / U;
  if (q >= nunits) return (d.unit[nunits - 1] & PKT_MASK) + 1;   // the emitted bytes end with the last unit
  *unit_byte = g - q * U;
  *dnp = d.unit[q] >> 24;
  return d.unit[q] & PKT_MASK;
}

// what packet i < the resume packet counts as: 0 selected, 1 deleted, 2 kept, 3 dropped at the flush
__host__ __device__ inline int count_class(const MaDev &d, const MaCut &c, uint32_t nunits, uint32_t i) {
  if (d.info[i] & MA_TX) return (d.flags[i] & MA_SEL) ? 0 : 2;
  if (c.flushed && (nunits == 0 || i > (d.unit[nunits - 1] & PKT_MASK))) return 3;
  return 1;
}

// ------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(256) void modeadapt_classify(MaDev d, MaRun r) {
  __shared__ uint32_t mask[256];
  if (d.has_mask) mask[threadIdx.x] = d.mask[threadIdx.x];
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < r.n) classify_one(d, r, mask, i);
}

__global__ __launch_bounds__(256) void modeadapt_runpos(MaDev d, MaRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < r.n) runpos_one(d, r, i);
}

__global__ __launch_bounds__(256) void modeadapt_compact(MaDev d, MaRun r) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < r.n) compact_one(d, i);
}

template <bool NPD>
__global__ __launch_bounds__(256) void modeadapt_emit(MaDev d, MaRun r, uint32_t ntiles) {
  __shared__ uint32_t crc[256];
  __shared__ uint8_t hdr[16];
  crc[threadIdx.x] = d.crc[threadIdx.x];
  const uint32_t nunits = min(d.tile_t[ntiles], r.n);   // a total past the packets cannot be: keeps the reads inside
  const MaCut c = cut_of(d, r, nunits);
  const uint32_t nframes = c.whole + (c.rem ? 1 : 0);
  for (uint32_t k = blockIdx.x; k < nframes; k += gridDim.x) {
    const uint32_t g0 = r.unit_byte + k * d.D, nbytes = k < c.whole ? d.D : c.rem;
    __syncthreads();   // the table is staged; the previous frame's header is no longer read
    if (threadIdx.x == 0) frame_header(d, r, crc, g0, nbytes, hdr);
    __syncthreads();
    uint8_t *dst = r.out + (size_t)k * d.L;
    const uint32_t head = head_of(dst, d.L);
    const uint32_t nchunks = 1 + (d.L - head + 15) / 16;
    for (uint32_t cidx = threadIdx.x; cidx < nchunks; cidx += 256) emit_chunk<NPD>(d, r, hdr, g0, nbytes, dst, head, cidx);
  }
}

__global__ __launch_bounds__(256) void modeadapt_count(MaDev d, MaRun r, uint32_t ntiles) {
  __shared__ uint32_t hist[5];
  if (threadIdx.x < 5) hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t nunits = min(d.tile_t[ntiles], r.n);
  const MaCut c = cut_of(d, r, nunits);
  uint32_t ub, dnp;
  const uint32_t iend = min(resume_of(d, r, c, nunits, &ub, &dnp), r.n);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    d.res[MA_R_TS_PACKET] = r.i0 + iend;
    d.res[MA_R_UNIT_BYTE] = ub;
    d.res[MA_R_DNP] = dnp;
    d.res[MA_R_PACKETS_IN] = iend;
    d.res[MA_R_BBFRAMES] = c.whole + (c.rem ? 1 : 0);
    d.res[MA_R_FLUSHED] = c.rem ? 1 : 0;
  }
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < iend; i += gridDim.x * 256) {
    atomicAdd(&hist[count_class(d, c, nunits, i)], 1u);
    if (d.flags[i] & MA_SYNC_ERR) atomicAdd(&hist[4], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 5 && hist[threadIdx.x]) {
    const int at[5] = {MA_R_SELECTED, MA_R_DELETED, MA_R_KEPT, MA_R_DROPPED, MA_R_SYNC};
    atomicAdd(&d.res[at[threadIdx.x]], (unsigned long long)hist[threadIdx.x]);
  }
}

}  // namespace

void modeadapt_host_table(uint32_t *tab) {
  for (uint32_t v = 0; v < 256; v++) {
    uint32_t c = v;
    for (int i = 0; i < 8; i++) c = ((c << 1) ^ ((c & 0x80) ? 0xD5u : 0u)) & 0xFF;
    tab[v] = c;
  }
}

size_t modeadapt_layout(MaDev &d, void *base) {
  LayoutTaker take{base};
  const size_t n = d.max_ts, nt = scan_tiles_of(d.max_ts) + 1;
  take(d.res, MA_R_WORDS);
  take(d.flags, n);
  take(d.info, n);
  take(d.mscan, n);
  take(d.tile_m, nt);
  take(d.tscan, n);
  take(d.tile_t, nt);
  take(d.unit, n);
  take(d.mask, 256);
  take(d.crc, 256);
  return take.at;
}

hipError_t modeadapt_launch(const MaDev &d, const MaRun &r, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d.res, 0, MA_R_WORDS * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  const uint32_t nb = std::max<uint32_t>(1, (r.n + 255) / 256), nt = scan_tiles_of(r.n);
  const uint32_t U = d.npd ? 188 : 187;
  // BBFRAMEs the call can emit at most: the whole ones of n units, the flush frame
  const uint32_t frames = (uint32_t)std::min<uint64_t>(r.cap, (uint64_t)r.n * U / d.D + 1);
  hipLaunchKernelGGL(modeadapt_classify, dim3(nb), dim3(256), 0, st, d, r);
  if ((e = scan_exclusive(d.mscan, d.tile_m, r.n, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(modeadapt_runpos, dim3(nb), dim3(256), 0, st, d, r);
  if ((e = scan_exclusive(d.tscan, d.tile_t, r.n, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(modeadapt_compact, dim3(nb), dim3(256), 0, st, d, r);
  if (d.npd) hipLaunchKernelGGL(modeadapt_emit<true>, dim3(blocks_for(frames, 1, 4096)), dim3(256), 0, st, d, r, nt);
  else hipLaunchKernelGGL(modeadapt_emit<false>, dim3(blocks_for(frames, 1, 4096)), dim3(256), 0, st, d, r, nt);
  hipLaunchKernelGGL(modeadapt_count, dim3(blocks_for(r.n, 256, 1024)), dim3(256), 0, st, d, r, nt);
  return hipGetLastError();
}

}  // namespace t2
