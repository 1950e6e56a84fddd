// TS multiplexer on the GPU (dvbt2ll_tsmux_*, include/dvbt2ll_hip.h): device state and the launch entry.
#ifndef TSMUX_KERNELS_H
#define TSMUX_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2 {

constexpr int TSMUX_IN = 8;                 // DVBT2LL_TSMUX_INPUTS
constexpr int TSMUX_OWN = TSMUX_IN + 2;     // the inputs, the PCR generator, null
constexpr uint32_t TSMUX_PKTS = 64;         // output packets per workgroup trip
constexpr uint32_t TSMUX_MAX_BLOCKS = 2048; // the grid's cap: past TSMUX_MAX_BLOCKS x TSMUX_PKTS packets a workgroup takes more than one trip

// the device result, 64-bit words (t2_capi.cpp copies them into dvbt2ll_tsmux_result)
enum : int {
  TSMUX_R_CONSUMED = 0, TSMUX_R_DRY = TSMUX_IN, TSMUX_R_FILL_IN_FREE = 2 * TSMUX_IN, TSMUX_R_PCR, TSMUX_R_NULL,
  TSMUX_R_SYNC, TSMUX_R_WORDS
};

struct TsmuxDev {
  int n = 0, owners = 0, fill = -1, pcr_pid = -1;
  uint32_t period = 0;
  uint32_t loop = 0;                  // bit i: input i is a carousel
  uint32_t w[TSMUX_OWN] = {};         // slots per period of owner e
  unsigned long long tpp = 0;         // ticks_per_period = tpp_q x period + tpp_r: floor(t tpp / period) is then
  unsigned long long tpp_q = 0;       // t tpp_q + floor(t tpp_r / period), whose division is a 32-bit one
  uint32_t tpp_r = 0;
  const uint8_t *table = nullptr;     // period owners
  const uint32_t *pre = nullptr;      // (period + 1) x owners prefix counts, a slot's owners side by side
  unsigned long long *res = nullptr;  // TSMUX_R_WORDS
};

struct TsmuxRun {
  const uint8_t *in[TSMUX_IN] = {};
  uint32_t n_in[TSMUX_IN] = {}, next[TSMUX_IN] = {};
  uint32_t pre0[TSMUX_OWN] = {};      // pre_e[phase]
  uint32_t phase = 0, n_out = 0;
  unsigned long long pcr_ticks = 0;
  uint8_t *out = nullptr;
};

// one run on stream: the counters are zeroed, then one kernel; no host round trip
hipError_t tsmux_launch(const TsmuxDev &d, const TsmuxRun &r, hipStream_t stream);

}  // namespace t2
#endif
