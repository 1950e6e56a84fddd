// TS multiplexer, host side (dvbt2ll_tsmux_schedule, dvbt2ll_tsmux_ticks_per_period, dvbt2ll_psi_build of
// include/dvbt2ll_hip.h): the schedule table with its prefix counts, and the PAT / PMT carousel.  No HIP in here: the
// file also compiles alone with the host compiler (tools/tsmux_host_check.cpp).
#ifndef TSMUX_PLAN_H
#define TSMUX_PLAN_H

#include <stdint.h>
#include <vector>

#include "../../include/dvbt2ll_hip.h"

namespace t2 {

constexpr int TSMUX_OWNERS = DVBT2LL_TSMUX_INPUTS + 2;       // the inputs, the PCR generator, null
constexpr int64_t TSMUX_PCR_WRAP = ((int64_t)1 << 33) * 300; // W: the 27 MHz clock a PCR can hold

struct TsmuxPlan {
  int owners = 0;                 // n_inputs + 2
  uint32_t w[TSMUX_OWNERS] = {};  // slots per period of owner e
  std::vector<uint8_t> table;     // period owners
  std::vector<uint32_t> pre;      // (period + 1) x owners: pre[t * owners + e] = owner e's slots among table slots [0, t)
};

bool tsmux_params_ok(const dvbt2ll_tsmux_params &p);
// the table and prefix counts of valid params
void tsmux_plan(const dvbt2ll_tsmux_params &p, TsmuxPlan &plan);
// a remux configuration for a handle of valid params (dvbt2ll_tsmux_remux_check)
bool tsmux_remux_ok(const dvbt2ll_tsmux_params &p, const dvbt2ll_tsmux_remux &x);
// the mux clock of a handle of p with remux x: ticks per period
inline int64_t tsmux_remux_tpp(const dvbt2ll_tsmux_params &p, const dvbt2ll_tsmux_remux &x) {
  return p.pcr_pid >= 0 ? p.ticks_per_period : x.out_ticks_per_period;
}

}  // namespace t2
#endif
