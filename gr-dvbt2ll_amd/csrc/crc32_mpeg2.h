// CRC-32/MPEG-2 (G = 0x04C11DB7, MSB first, initial value 0xFFFFFFFF, no final XOR) as the stream blocks use it: a
// byte table, and x^(8 n) mod G to join the registers of chunks that were run separately.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace t2 {

constexpr uint32_t CRC32M_POLY = 0x04C11DB7u;

// tab: the 256-entry byte table, then x^(8 n) mod G for n = 0 .. n_powers - 1
inline void crc32m_host_tables(uint32_t *tab, int n_powers) {
  for (uint32_t v = 0; v < 256; v++) {
    uint32_t c = v << 24;
    for (int i = 0; i < 8; i++) c = (c << 1) ^ ((c >> 31) ? CRC32M_POLY : 0u);
    tab[v] = c;
  }
  uint32_t p = 1;
  for (int n = 0; n < n_powers; n++) {
    tab[256 + n] = p;
    p = (p << 8) ^ tab[p >> 24];
  }
}

__device__ inline uint32_t gf_mul(uint32_t a, uint32_t b) {   // a(x) b(x) mod G, bit 31 = x^31
  uint32_t r = 0;
  for (int i = 31; i >= 0; i--) {
    r = (r << 1) ^ ((r >> 31) ? CRC32M_POLY : 0u);
    if ((b >> i) & 1) r ^= a;
  }
  return r;
}

__device__ inline uint32_t crc32m_byte(uint32_t crc, uint32_t b, const uint32_t *tab) {
  return (crc << 8) ^ tab[(crc >> 24) ^ b];
}

// n readable bytes at p: bytes up to a 4-byte boundary, aligned words, the rest
__device__ inline uint32_t crc32m_run(uint32_t crc, const uint8_t *p, uint32_t n, const uint32_t *tab) {
  while (n && ((uintptr_t)p & 3)) {
    crc = crc32m_byte(crc, *p++, tab);
    n--;
  }
  for (; n >= 4; n -= 4, p += 4) {
    const uint32_t w = *(const uint32_t *)p;
    crc = crc32m_byte(crc, w & 255, tab);
    crc = crc32m_byte(crc, (w >> 8) & 255, tab);
    crc = crc32m_byte(crc, (w >> 16) & 255, tab);
    crc = crc32m_byte(crc, w >> 24, tab);
  }
  for (; n; n--) crc = crc32m_byte(crc, *p++, tab);
  return crc;
}

// A wavefront's CRC of T bytes.  The bytes are padded in front to 64 chunks of c = (T + 63) / 64 bytes (leading zeros
// leave a zero register unchanged), and lane l ran its chunk, bytes [l c - pad, (l + 1) c - pad) cut at 0, from a zero
// register into crc.  Every chunk has the same length, so the tree multiplies the left half by x^(8 c 2^m) at level m;
// the initial 0xFFFFFFFF is added as 0xFFFFFFFF x^(8 T).  xp[n] = x^(8 n) mod G, n up to 32 c.  Every lane returns the
// whole CRC.
__device__ inline uint32_t crc32m_wave_join(uint32_t crc, uint32_t lane, uint32_t c, uint32_t T, const uint32_t *xp) {
  for (int m = 0; m < 6; m++) {
    const uint32_t other = __shfl_xor(crc, 1 << m);
    const bool right = (lane >> m) & 1;
    crc = gf_mul(right ? other : crc, xp[c << m]) ^ (right ? crc : other);
  }
  return crc ^ gf_mul(0xFFFFFFFFu, xp[T]);
}

// lane's chunk of the T bytes as [lo, hi) (empty where hi <= lo), and c for crc32m_wave_join
__device__ inline uint32_t crc32m_wave_chunk(uint32_t lane, uint32_t T, int &lo, int &hi) {
  const uint32_t c = (T + 63) >> 6, pad = 64 * c - T;
  lo = (int)(lane * c) - (int)pad;
  hi = lo + (int)c;
  if (lo < 0) lo = 0;
  return c;
}

}  // namespace t2
