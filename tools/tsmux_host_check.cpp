// Host-side robustness check of the TS multiplexer's planner and the PSI builder (gr-dvbt2ll_amd/csrc/tsmux_plan.cpp):
// a stand-alone program for an AddressSanitizer + UBSan build on the host compiler, no GPU and no Python
// (make -C gr-dvbt2ll_amd/csrc tsmux-host-check).  It runs dvbt2ll_tsmux_schedule over the shapes of
// tests/tsmux_cases.py and the largest allowed parameters into exactly-sized heap buffers, checks every table against
// a direct evaluation of the rule (each slot's pair is the least (due, owner) not yet taken), and runs
// dvbt2ll_psi_build from the smallest to the largest parameter set into exactly-sized buffers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/dvbt2ll_hip.h"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static dvbt2ll_tsmux_params mux(int period, std::vector<int> w, int fill, int pcr_weight) {
  dvbt2ll_tsmux_params p;
  std::memset(&p, 0, sizeof p);
  p.n_inputs = (int)w.size();
  p.period = period;
  for (size_t i = 0; i < w.size(); i++) p.weight[i] = w[i];
  p.fill_input = fill;
  p.pcr_pid = pcr_weight ? 0x1FF : -1;
  p.pcr_weight = pcr_weight;
  p.ticks_per_period = pcr_weight ? ((int64_t)1 << 36) - 1 : 0;
  p.max_out_packets = 1 << 24;
  return p;
}

static void check_schedule(const dvbt2ll_tsmux_params &p) {
  std::vector<uint8_t> owner((size_t)p.period);   // exactly period bytes: a write past them is reported
  EXPECT(dvbt2ll_tsmux_schedule(&p, owner.data()) == DVBT2LL_OK);
  const int no = p.n_inputs + 2;
  std::vector<uint64_t> w(no), k(no, 0);
  uint64_t sum = 0;
  for (int i = 0; i < p.n_inputs; i++) sum += w[i] = (uint64_t)p.weight[i];
  sum += w[p.n_inputs] = (uint64_t)p.pcr_weight;
  w[no - 1] = (uint64_t)p.period - sum;
  for (int m = 0; m < p.period; m++) {
    const int e = owner[m];
    EXPECT(e < no && k[e] < w[e]);
    if (e >= no || k[e] >= w[e]) return;
    // no other owner's next pair sorts before this one
    for (int f = 0; f < no; f++) {
      if (f == e || k[f] >= w[f]) continue;
      const uint64_t a = k[e] * w[f], b = k[f] * w[e];   // k_e / w_e against k_f / w_f
      EXPECT(a < b || (a == b && e < f));
    }
    k[e]++;
  }
  for (int e = 0; e < no; e++) EXPECT(k[e] == w[e]);
}

static dvbt2ll_psi_params psi(int programs, int streams, int desc) {
  dvbt2ll_psi_params p;
  std::memset(&p, 0, sizeof p);
  p.transport_stream_id = 0xFFFF;
  p.version = 31;
  p.n_programs = programs;
  for (int a = 0; a < programs; a++) {
    dvbt2ll_psi_program &g = p.programs[a];
    g.program_number = 65535 - a;
    g.pmt_pid = 0x1FFE - a;
    g.pcr_pid = 0x1FFF;
    g.n_streams = streams;
    for (int s = 0; s < streams; s++) {
      g.streams[s].stream_type = 255;
      g.streams[s].pid = 0x1FFF;
      g.streams[s].descriptor_len = desc;
      std::memset(g.streams[s].descriptors, 0xA0 + s, sizeof g.streams[s].descriptors);
    }
  }
  return p;
}

static void check_psi(const dvbt2ll_psi_params &p) {
  const int64_t n = dvbt2ll_psi_build(&p, nullptr, 0);
  EXPECT(n > 0 && n % DVBT2LL_PSI_ROUNDS == 0);
  if (n <= 0) return;
  std::vector<uint8_t> out((size_t)n * 188);      // exactly n packets
  EXPECT(dvbt2ll_psi_build(&p, out.data(), n) == n);
  EXPECT(dvbt2ll_psi_build(&p, out.data(), n - 1) == DVBT2LL_EINVAL);
  int cc[0x2000];
  std::memset(cc, 0, sizeof cc);
  for (int64_t k = 0; k < n; k++) {
    const uint8_t *q = &out[(size_t)k * 188];
    const int pid = ((q[1] & 0x1F) << 8) | q[2];
    EXPECT(q[0] == 0x47 && (q[3] >> 4) == 1 && (q[3] & 15) == cc[pid]);
    cc[pid] = (cc[pid] + 1) & 15;
  }
  for (int pid = 0; pid < 0x2000; pid++) EXPECT(cc[pid] == 0);   // every PID sent a multiple of 16 packets
}

int main() {
  // the shapes of tests/tsmux_cases.py
  check_schedule(mux(1, {1}, -1, 0));
  check_schedule(mux(7, {3, 2}, -1, 1));
  check_schedule(mux(12, {3, 3, 3}, -1, 3));
  check_schedule(mux(12, {2, 4, 6}, -1, 0));
  check_schedule(mux(10, {5, 3}, -1, 2));
  check_schedule(mux(65536, {1, 65534}, -1, 0));
  check_schedule(mux(65536, {0, 4097}, 0, 1));
  // the largest: 8 inputs, the longest period, with and without a null owner
  check_schedule(mux(65536, {8192, 8191, 8190, 8189, 8188, 8187, 8186, 8185}, 7, 28));
  check_schedule(mux(65536, {1, 2, 3, 4, 5, 6, 7, 60000}, -1, 5508));
  check_schedule(mux(65536, {65536}, -1, 0));
  check_schedule(mux(65536, {0, 1, 1, 1, 1, 1, 1, 1}, 0, 65529));
  // refusals write nothing
  dvbt2ll_tsmux_params bad = mux(7, {3, 5}, -1, 0);
  uint8_t none = 0xEE;
  EXPECT(dvbt2ll_tsmux_schedule(&bad, &none) == DVBT2LL_EINVAL && none == 0xEE);
  EXPECT(dvbt2ll_tsmux_schedule(nullptr, &none) == DVBT2LL_EINVAL);
  EXPECT(dvbt2ll_tsmux_ticks_per_period(65536, 1) == (int64_t)65536 * 1504 * 27000000);
  EXPECT(dvbt2ll_tsmux_ticks_per_period(10, 4000000) == 101520);
  EXPECT(dvbt2ll_tsmux_ticks_per_period(1, INT64_MAX) == 0);
  EXPECT(dvbt2ll_tsmux_ticks_per_period(0, 1) == -1);
  check_psi(psi(1, 0, 0));
  check_psi(psi(1, 1, 0));
  check_psi(psi(2, 8, 64));
  check_psi(psi(8, 8, 64));
  check_psi(psi(8, 8, 63));
  dvbt2ll_psi_params over = psi(8, 8, 64);
  over.programs[7].streams[7].descriptor_len = 65;
  EXPECT(dvbt2ll_psi_build(&over, nullptr, 0) == DVBT2LL_EINVAL);
  over = psi(8, 8, 64);
  over.programs[7].pmt_pid = over.programs[0].pmt_pid;
  EXPECT(dvbt2ll_psi_build(&over, nullptr, 0) == DVBT2LL_EINVAL);
  if (fails) { std::fprintf(stderr, "tsmux_host_check: %d failures\n", fails); return 1; }
  std::printf("tsmux_host_check ok\n");
  return 0;
}
