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

// ---------------------------------------------------------------------------- remux (dvbt2ll_tsmux_*_remux)
constexpr int TSREMUX_SLOTS = 64;               // DVBT2LL_TSMUX_TRACK: tracked PIDs
constexpr uint32_t TSREMUX_TILE = TSMUX_PKTS;   // output packets per row of payload counts: one trip, one wave
constexpr uint32_t TSREMUX_SCAN_TILES = 256;    // tiles one workgroup of the scan's first round covers; a call of more
                                                // tiles has a non-zero base from the second round (the scan over chunks)
constexpr uint32_t TSREMUX_MAX_CHUNKS = (1u << 24) / TSREMUX_TILE / TSREMUX_SCAN_TILES;   // 1024
constexpr uint32_t TSREMUX_NO_SLOT = 0xFF;      // slot_of[pid] of a PID that is not tracked
constexpr uint32_t TSREMUX_DROP = 0x1FFF;       // a map target: the packet leaves as the null packet
constexpr uint32_t TSREMUX_ENTRY = 0x8000;      // pid_map: the value comes from a map entry

// the device result of a remux run, 64-bit words; TSREMUX_R_CC + s: the payload packets restamped on slot s, mod 256
enum : int { TSREMUX_R_REMAPPED = 0, TSREMUX_R_DROPPED, TSREMUX_R_CC_REWRITTEN, TSREMUX_R_PCR, TSREMUX_R_CC,
             TSREMUX_R_WORDS = TSREMUX_R_CC + TSREMUX_SLOTS };

struct TsremuxDev {
  const uint16_t *pid_map = nullptr;  // TSMUX_IN x 8192: TSREMUX_ENTRY | to_pid where (input, PID) has a map entry, else the PID
  const uint8_t *slot_of = nullptr;   // 8192: the tracked slot of an output PID, or TSREMUX_NO_SLOT
  uint8_t *tiles = nullptr;           // a row of TSREMUX_SLOTS bytes per tile: the payload counts, then their exclusive
                                      // prefix inside the tile's chunk (mod 256; a counter needs it mod 16)
  uint8_t *chunks = nullptr;          // a row per chunk of TSREMUX_SCAN_TILES tiles: start cc + the chunks before it
  unsigned long long *res = nullptr;  // TSREMUX_R_WORDS
  uint32_t restamp_cc = 0;            // bit i: input i's packets on tracked PIDs get new counters
  uint32_t in_period[TSMUX_IN] = {};  // 0: input i's PCRs pass unchanged
  unsigned long long in_tpp[TSMUX_IN] = {};     // in_ticks_per_period = in_q x in_period + in_r, as TsmuxDev's tpp
  unsigned long long in_q[TSMUX_IN] = {};
  uint32_t in_r[TSMUX_IN] = {};
};

struct TsremuxRun {
  unsigned long long cc[TSREMUX_SLOTS / 16] = {};   // the start counters, 4 bits each, slot s in word s / 16
  uint32_t in_phase[TSMUX_IN] = {};
  unsigned long long in_ticks[TSMUX_IN] = {};
};

// one remux run on stream: both sets of counters are zeroed, then classify, the two scan rounds and the emit kernel
// (tsmux_mux's remux instantiation); no host round trip.  d is the handle's TsmuxDev with tpp holding the mux clock.
hipError_t tsremux_launch(const TsmuxDev &d, const TsremuxDev &x, const TsmuxRun &r, const TsremuxRun &y,
                          hipStream_t stream);

}  // namespace t2
#endif
