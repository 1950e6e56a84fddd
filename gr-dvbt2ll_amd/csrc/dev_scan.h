// Device-wide exclusive scan shared by the stream blocks (mode adapter, T2-MI, ULE, MPE, MPE-FEC): tile sums of
// SCAN_TILE entries, one workgroup over the sums, apply.  T needs operator+ and T{} (the identity).  Each block keeps
// its own three __global__ wrappers (they own the LDS and the kernel names) and hands them to scan_exclusive.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace t2 {

constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 4, SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;

inline uint32_t scan_tiles_of(uint32_t n) { return std::max<uint32_t>(1, (n + SCAN_TILE - 1) / SCAN_TILE); }

// exclusive scan of 256 per-thread values through LDS (2 x 256 entries); total = their sum
template <class T>
__device__ __forceinline__ T block_exclusive(T v, T *lds, T &total) {
  const int t = threadIdx.x;
  T *a = lds, *b = lds + SCAN_THREADS;
  a[t] = v;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {
    T x = a[t];
    if (t >= d) x = a[t - d] + x;
    b[t] = x;
    __syncthreads();
    T *s = a; a = b; b = s;
  }
  total = a[SCAN_THREADS - 1];
  T ex = t ? a[t - 1] : T{};
  __syncthreads();
  return ex;
}

// n: host-known bound; n_dev (may be null): the live count on the device, entries at or past it read as zero
__device__ __forceinline__ uint32_t scan_limit(uint32_t n, const uint32_t *n_dev) { return n_dev ? min(n, *n_dev) : n; }

// lds: SCAN_THREADS entries
template <class T>
__device__ __forceinline__ void scan_reduce_body(const T *in, T *tile, uint32_t n, const uint32_t *n_dev, T *lds) {
  const uint32_t lim = scan_limit(n, n_dev);
  const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  T s{};
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; q++) {
    T x{};
    if (i0 + q < lim) x = in[i0 + q];
    s = s + x;
  }
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int dd = SCAN_THREADS / 2; dd > 0; dd >>= 1) {
    if ((int)threadIdx.x < dd) lds[threadIdx.x] = lds[threadIdx.x] + lds[threadIdx.x + dd];
    __syncthreads();
  }
  if (threadIdx.x == 0) tile[blockIdx.x] = lds[0];
}

// one workgroup: tile sums -> exclusive tile offsets in place, the grand total to tile[ntiles].  The second round
// (tiles 256 and up) begins at the loop's second pass, with the tiles before it in carry.  lds: 2 x SCAN_THREADS
template <class T>
__device__ __forceinline__ void scan_tiles_body(T *tile, uint32_t ntiles, T *lds) {
  T carry{};
  for (uint32_t b = 0; b < ntiles; b += SCAN_THREADS) {
    const uint32_t i = b + threadIdx.x;
    T v = i < ntiles ? tile[i] : T{};
    T total;
    T ex = block_exclusive(v, lds, total);
    if (i < ntiles) tile[i] = carry + ex;
    carry = carry + total;
  }
  if (threadIdx.x == 0) tile[ntiles] = carry;
}

// lds: 2 x SCAN_THREADS
template <class T>
__device__ __forceinline__ void scan_apply_body(T *data, const T *tile, uint32_t n, const uint32_t *n_dev, T *lds) {
  const uint32_t lim = scan_limit(n, n_dev);
  if (blockIdx.x * SCAN_TILE >= lim) return;
  const uint32_t i0 = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
  T v[SCAN_ITEMS];
  T s{};
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; q++) {
    v[q] = i0 + q < lim ? data[i0 + q] : T{};
    s = s + v[q];
  }
  T total;
  T run = tile[blockIdx.x] + block_exclusive(s, lds, total);
#pragma unroll
  for (int q = 0; q < SCAN_ITEMS; q++) {
    if (i0 + q < lim) data[i0 + q] = run;
    run = run + v[q];
  }
}

// a block's three wrappers of the bodies above
template <class T>
struct ScanKernels {
  void (*reduce)(const T *, T *, uint32_t, const uint32_t *);
  void (*tiles)(T *, uint32_t);
  void (*apply)(T *, const T *, uint32_t, const uint32_t *);
};

// data[0 .. n) -> its exclusive scan in place; tile: scan_tiles_of(n) + 1 entries, the last receives the total
template <class T>
hipError_t scan_exclusive(const ScanKernels<T> &k, T *data, T *tile, uint32_t n, const uint32_t *n_dev, hipStream_t st) {
  const uint32_t ntiles = scan_tiles_of(n);
  hipLaunchKernelGGL(k.reduce, dim3(ntiles), dim3(SCAN_THREADS), 0, st, (const T *)data, tile, n, n_dev);
  hipLaunchKernelGGL(k.tiles, dim3(1), dim3(SCAN_THREADS), 0, st, tile, ntiles);
  hipLaunchKernelGGL(k.apply, dim3(ntiles), dim3(SCAN_THREADS), 0, st, data, (const T *)tile, n, n_dev);
  return hipGetLastError();
}

}  // namespace t2
