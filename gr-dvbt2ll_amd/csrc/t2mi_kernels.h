// T2-MI de-encapsulation on the GPU (dvbt2ll_t2mi_*, include/dvbt2ll_hip.h): device state and the launch entry.
#ifndef T2MI_KERNELS_H
#define T2MI_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2 {

constexpr int T2MI_MAX_PLP = 8;
constexpr int T2MI_MAX_T = 10 + 8192;   // longest T2-MI packet: payload_len 0xFFFF bits

// the device result, 64-bit words (t2_capi.cpp copies them into dvbt2ll_t2mi_result)
enum : int {
  T2MI_R_OFFSET = 0, T2MI_R_SKIP, T2MI_R_PACKETS,
  T2MI_R_TS = 3,      // contributing, foreign, null, tei, scrambled, bad_sync, no_payload, discontinuities, bad_pointers
  T2MI_R_PKT = 12,    // broken, crc_errors, filtered, len_errors, other_plp, accepted
  T2MI_R_BLOCKS = 18, T2MI_R_TYPE = 26, T2MI_R_WORDS = 26 + 256
};

struct T2miV8 { uint32_t v[T2MI_MAX_PLP]; };

// one table record: dvbt2ll_t2mi_packet
struct T2miRec {
  uint32_t ts_index, ts_byte;
  uint8_t type, count, sf_idx, stream_id;
  uint16_t payload_len;
  uint8_t flags, ifs, frame_idx, plp_id;
  int8_t out;
  uint8_t why;        // scratch between the passes (1: unmapped plp_id, 2: wrong length); 0 in the emitted table
  int32_t block;
};
static_assert(sizeof(T2miRec) == 24, "dvbt2ll_t2mi_packet layout");

struct T2miDev {
  int pid = 0, stream_id = -1, nplp = 0;
  int plp_id[T2MI_MAX_PLP] = {}, L[T2MI_MAX_PLP] = {};
  uint32_t max_ts = 0;        // TS packets per run
  uint32_t max_packets = 0;   // T2-MI packets per run
  // scratch, carved by t2mi_layout
  uint32_t *cls = nullptr;                 // per TS packet: class, pusi, cc, payload offset, pointer_field
  unsigned long long *scan_a = nullptr;    // per TS packet: stream offset << 32 | index among the contributing
  unsigned long long *tile_a = nullptr;
  uint32_t *c_base = nullptr, *c_off = nullptr, *c_ts = nullptr;   // per contributing packet (+ 1 for c_base)
  uint8_t *c_disc = nullptr;
  uint32_t *nst = nullptr, *tile_b = nullptr;                      // starts per contributing packet, scanned
  uint32_t *pk_s = nullptr, *pk_k = nullptr, *pk_T = nullptr;      // per T2-MI packet (+ 1)
  T2miV8 *cand = nullptr, *tile_c = nullptr;                       // per T2-MI packet: its output, scanned to ranks
  T2miRec *table = nullptr;
  unsigned long long *res = nullptr;       // T2MI_R_WORDS
  uint32_t *ctl = nullptr;                 // T2MI_CTL_*
  T2miV8 *tot_c = nullptr;
  uint32_t *tab = nullptr;                 // 256 CRC table entries, then x^(8 n) mod G for n <= T2MI_MAX_T
};

struct T2miRun {
  const uint8_t *ts = nullptr;
  uint32_t i0 = 0, n = 0;     // TS packets [i0, i0 + n) of ts
  uint32_t skip = 0;
  uint8_t *out[T2MI_MAX_PLP] = {};
  uint32_t cap[T2MI_MAX_PLP] = {};
};

constexpr int T2MI_TAB_WORDS = 256 + T2MI_MAX_T + 1;
// fills tab (host): the CRC-32/MPEG-2 byte table and the powers of x^8
void t2mi_host_tables(uint32_t *tab);
// assigns d's scratch pointers inside base (nullptr: sizing only); returns the bytes needed
size_t t2mi_layout(T2miDev &d, void *base);
// every pass of one run on stream; no host round trip
hipError_t t2mi_launch(const T2miDev &d, const T2miRun &r, hipStream_t stream);

}  // namespace t2
#endif
