// TS multiplexer, host side: the schedule (semantics: include/dvbt2ll_hip.h) and the PSI carousel.
#include "tsmux_plan.h"

#include <string.h>

namespace t2 {

bool tsmux_params_ok(const dvbt2ll_tsmux_params &p) {
  if (p.n_inputs < 1 || p.n_inputs > DVBT2LL_TSMUX_INPUTS) return false;
  if (p.period < 1 || p.period > DVBT2LL_TSMUX_MAX_PERIOD) return false;
  if (p.fill_input < -1 || p.fill_input >= p.n_inputs) return false;
  if (p.max_out_packets < 1 || p.max_out_packets > (1 << 24)) return false;
  int64_t sum = 0;
  for (int i = 0; i < p.n_inputs; i++) {
    if (p.loop[i] != 0 && p.loop[i] != 1) return false;
    if (p.weight[i] < 0 || p.weight[i] > p.period) return false;
    if (p.weight[i] == 0 && i != p.fill_input) return false;
    sum += p.weight[i];
  }
  if (p.fill_input >= 0 && p.loop[p.fill_input]) return false;
  if (p.pcr_pid < 0) {
    if (p.pcr_pid != -1 || p.pcr_weight != 0 || p.ticks_per_period != 0) return false;
  } else {
    if (p.pcr_pid > 0x1FFE || p.pcr_weight < 1 || p.pcr_weight > p.period) return false;
    if (p.ticks_per_period < 1 || p.ticks_per_period >= ((int64_t)1 << 36)) return false;
    sum += p.pcr_weight;
  }
  return sum <= p.period;
}

void tsmux_plan(const dvbt2ll_tsmux_params &p, TsmuxPlan &plan) {
  const int n = p.n_inputs, no = n + 2;
  const uint32_t P = (uint32_t)p.period;
  plan.owners = no;
  uint32_t sum = 0;
  for (int i = 0; i < n; i++) sum += plan.w[i] = (uint32_t)p.weight[i];
  sum += plan.w[n] = (uint32_t)p.pcr_weight;
  plan.w[n + 1] = P - sum;
  plan.table.assign(P, 0);
  plan.pre.assign((size_t)(P + 1) * no, 0);
  // a merge of the owners' due times: k[e] is owner e's next slot, due at k[e] / w[e]; the earliest goes next, the
  // lower e on a tie (k_e / w_e < k_f / w_f as k_e w_f < k_f w_e)
  uint32_t k[TSMUX_OWNERS] = {};
  for (uint32_t m = 0; m < P; m++) {
    int best = -1;
    for (int e = 0; e < no; e++) {
      if (k[e] >= plan.w[e]) continue;
      if (best < 0 || (uint64_t)k[e] * plan.w[best] < (uint64_t)k[best] * plan.w[e]) best = e;
    }
    plan.table[m] = (uint8_t)best;
    memcpy(&plan.pre[(size_t)(m + 1) * no], &plan.pre[(size_t)m * no], no * sizeof(uint32_t));
    plan.pre[(size_t)(m + 1) * no + best]++;
    k[best]++;
  }
}

bool tsmux_remux_ok(const dvbt2ll_tsmux_params &p, const dvbt2ll_tsmux_remux &x) {
  if (x.n_map < 0 || x.n_map > DVBT2LL_TSMUX_MAP || x.n_track < 0 || x.n_track > DVBT2LL_TSMUX_TRACK) return false;
  for (int a = 0; a < x.n_map; a++) {
    const dvbt2ll_tsmux_map &m = x.map[a];
    if (m.input < 0 || m.input >= p.n_inputs) return false;
    if (m.from_pid < 0 || m.from_pid > 0x1FFF || m.to_pid < 0 || m.to_pid > 0x1FFF) return false;
    if (p.pcr_pid >= 0 && m.to_pid == p.pcr_pid) return false;
    for (int b = 0; b < a; b++)
      if (x.map[b].input == m.input && x.map[b].from_pid == m.from_pid) return false;
  }
  for (int s = 0; s < x.n_track; s++) {
    if (x.track_pid[s] < 0 || x.track_pid[s] > 0x1FFE) return false;
    if (p.pcr_pid >= 0 && x.track_pid[s] == p.pcr_pid) return false;
    for (int b = 0; b < s; b++)
      if (x.track_pid[b] == x.track_pid[s]) return false;
  }
  for (int i = 0; i < DVBT2LL_TSMUX_INPUTS; i++) {
    const bool used = i < p.n_inputs;
    if (x.restamp_cc[i] != 0 && !(used && x.restamp_cc[i] == 1)) return false;
    if (x.in_ticks_per_period[i] == 0 && x.in_period[i] == 0) continue;
    if (!used || x.in_period[i] < 1 || x.in_period[i] > DVBT2LL_TSMUX_MAX_PERIOD) return false;
    if (x.in_ticks_per_period[i] < 1 || x.in_ticks_per_period[i] >= ((int64_t)1 << 36)) return false;
  }
  if (x.out_ticks_per_period < 0 || x.out_ticks_per_period >= ((int64_t)1 << 36)) return false;
  if (p.pcr_pid >= 0 && x.out_ticks_per_period != 0 && x.out_ticks_per_period != p.ticks_per_period) return false;
  return true;
}

namespace {

// CRC-32 of generator 0x04C11DB7, initial value 0xFFFFFFFF, no reflection, no final XOR (the MPE section's)
uint32_t psi_crc(const uint8_t *d, size_t n) {
  uint32_t crc = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    crc ^= (uint32_t)d[i] << 24;
    for (int b = 0; b < 8; b++) crc = (crc << 1) ^ ((crc >> 31) ? 0x04C11DB7u : 0u);
  }
  return crc;
}

void psi_finish(std::vector<uint8_t> &s) {
  const size_t len = s.size() - 3 + 4;   // the bytes behind the length field, CRC_32 included
  s[1] = (uint8_t)(0xB0 | (len >> 8));
  s[2] = (uint8_t)(len & 255);
  const uint32_t c = psi_crc(s.data(), s.size());
  for (int k = 3; k >= 0; k--) s.push_back((uint8_t)(c >> (8 * k)));
}

bool psi_params_ok(const dvbt2ll_psi_params &p) {
  if (p.transport_stream_id < 0 || p.transport_stream_id > 0xFFFF || p.version < 0 || p.version > 31) return false;
  if (p.n_programs < 1 || p.n_programs > DVBT2LL_PSI_PROGRAMS) return false;
  for (int a = 0; a < p.n_programs; a++) {
    const dvbt2ll_psi_program &g = p.programs[a];
    if (g.program_number < 1 || g.program_number > 0xFFFF) return false;
    if (g.pmt_pid < 0x10 || g.pmt_pid > 0x1FFE || g.pcr_pid < 0 || g.pcr_pid > 0x1FFF) return false;
    if (g.n_streams < 0 || g.n_streams > DVBT2LL_PSI_STREAMS) return false;
    for (int b = 0; b < a; b++)
      if (p.programs[b].pmt_pid == g.pmt_pid) return false;
    for (int s = 0; s < g.n_streams; s++) {
      const dvbt2ll_psi_stream &e = g.streams[s];
      if (e.stream_type < 0 || e.stream_type > 255 || e.pid < 0 || e.pid > 0x1FFF) return false;
      if (e.descriptor_len < 0 || e.descriptor_len > DVBT2LL_PSI_DESCRIPTOR_BYTES) return false;
    }
  }
  return true;
}

}  // namespace
}  // namespace t2

using namespace t2;

extern "C" int dvbt2ll_tsmux_schedule(const dvbt2ll_tsmux_params *p, uint8_t *owner) {
  if (!p || !owner || !tsmux_params_ok(*p)) return DVBT2LL_EINVAL;
  TsmuxPlan plan;
  tsmux_plan(*p, plan);
  memcpy(owner, plan.table.data(), plan.table.size());
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_tsmux_remux_check(const dvbt2ll_tsmux_params *p, const dvbt2ll_tsmux_remux *x) {
  return p && x && tsmux_params_ok(*p) && tsmux_remux_ok(*p, *x) ? DVBT2LL_OK : DVBT2LL_EINVAL;
}

extern "C" int64_t dvbt2ll_tsmux_ticks_per_period(int period, int64_t ts_bits_per_second) {
  if (period < 1 || period > DVBT2LL_TSMUX_MAX_PERIOD || ts_bits_per_second < 1) return -1;
  // below 2^52: 65536 x 1504 x 27e6
  const uint64_t num = (uint64_t)period * 1504u * 27000000u, rate = (uint64_t)ts_bits_per_second;
  return (int64_t)(num / rate + (num % rate >= rate - rate / 2 ? 1 : 0));
}

extern "C" int64_t dvbt2ll_psi_build(const dvbt2ll_psi_params *p, uint8_t *out, int64_t cap_packets) {
  if (!p || !psi_params_ok(*p)) return DVBT2LL_EINVAL;
  // the sections: the PAT, then each programme's PMT, with the PID each goes out on
  std::vector<std::vector<uint8_t>> sec;
  std::vector<int> pid;
  const uint8_t ver = (uint8_t)(0xC1 | (p->version << 1));
  std::vector<uint8_t> s = {0x00, 0, 0, (uint8_t)(p->transport_stream_id >> 8), (uint8_t)(p->transport_stream_id & 255),
                            ver, 0x00, 0x00};
  for (int a = 0; a < p->n_programs; a++) {
    const dvbt2ll_psi_program &g = p->programs[a];
    s.insert(s.end(), {(uint8_t)(g.program_number >> 8), (uint8_t)(g.program_number & 255),
                       (uint8_t)(0xE0 | (g.pmt_pid >> 8)), (uint8_t)(g.pmt_pid & 255)});
  }
  psi_finish(s);
  sec.push_back(s);
  pid.push_back(0);
  for (int a = 0; a < p->n_programs; a++) {
    const dvbt2ll_psi_program &g = p->programs[a];
    s = {0x02, 0, 0, (uint8_t)(g.program_number >> 8), (uint8_t)(g.program_number & 255), ver, 0x00, 0x00,
         (uint8_t)(0xE0 | (g.pcr_pid >> 8)), (uint8_t)(g.pcr_pid & 255), 0xF0, 0x00};
    for (int k = 0; k < g.n_streams; k++) {
      const dvbt2ll_psi_stream &e = g.streams[k];
      s.insert(s.end(), {(uint8_t)e.stream_type, (uint8_t)(0xE0 | (e.pid >> 8)), (uint8_t)(e.pid & 255),
                         (uint8_t)(0xF0 | (e.descriptor_len >> 8)), (uint8_t)(e.descriptor_len & 255)});
      s.insert(s.end(), e.descriptors, e.descriptors + e.descriptor_len);
    }
    psi_finish(s);
    sec.push_back(s);
    pid.push_back(g.pmt_pid);
  }
  int64_t round = 0;
  std::vector<int64_t> pk(sec.size());
  for (size_t a = 0; a < sec.size(); a++) round += pk[a] = (int64_t)(1 + sec[a].size() + 183) / 184;   // pointer_field first
  const int64_t total = DVBT2LL_PSI_ROUNDS * round;
  if (!out) return total;
  if (cap_packets < total) return DVBT2LL_EINVAL;
  uint8_t *q = out;
  for (int r = 0; r < DVBT2LL_PSI_ROUNDS; r++)
    for (size_t a = 0; a < sec.size(); a++) {
      size_t at = 0;
      for (int64_t j = 0; j < pk[a]; j++, q += 188) {
        memset(q, 0xFF, 188);
        q[0] = 0x47;
        q[1] = (uint8_t)((j == 0 ? 0x40 : 0) | (pid[a] >> 8));
        q[2] = (uint8_t)(pid[a] & 255);
        q[3] = (uint8_t)(0x10 | ((r * pk[a] + j) & 15));
        size_t room = 184, o = 4;
        if (j == 0) { q[4] = 0x00; room = 183; o = 5; }
        const size_t take = sec[a].size() - at < room ? sec[a].size() - at : room;
        memcpy(q + o, sec[a].data() + at, take);
        at += take;
      }
    }
  return total;
}
