// Mode adaptation with null-packet deletion on the GPU (dvbt2ll_modeadapt_*, include/dvbt2ll_hip.h): device state and
// the launch entry.
#ifndef MODEADAPT_KERNELS_H
#define MODEADAPT_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2 {

// the device result, 64-bit words (t2_capi.cpp copies them into dvbt2ll_modeadapt_result)
enum : int {
  MA_R_TS_PACKET = 0, MA_R_UNIT_BYTE, MA_R_DNP,
  MA_R_PACKETS_IN, MA_R_SELECTED, MA_R_DELETED, MA_R_KEPT, MA_R_DROPPED, MA_R_SYNC, MA_R_BBFRAMES, MA_R_FLUSHED,
  MA_R_WORDS = 16
};

struct MaMax { uint32_t v; };   // the scan's monoid of "index + 1 of the last selected packet": + is max, {} is none

struct MaDev {
  int npd = 0, has_mask = 0;
  uint32_t D = 0, L = 0;      // data-field and BBFRAME bytes
  uint32_t matype = 0;        // MATYPE-1 << 8 | MATYPE-2
  uint32_t max_ts = 0;        // TS packets per run
  // scratch, carved by modeadapt_layout
  unsigned long long *res = nullptr;                   // MA_R_WORDS
  uint8_t *flags = nullptr;                            // per TS packet: MA_SEL, MA_SYNC_ERR
  uint16_t *info = nullptr;                            // per TS packet: DNP | transmitted << 8
  MaMax *mscan = nullptr, *tile_m = nullptr;           // exclusive max-scan of (selected ? index + 1 : 0)
  uint32_t *tscan = nullptr, *tile_t = nullptr;        // exclusive sum of the transmitted flags: the unit index
  uint32_t *unit = nullptr;                            // per unit: packet index | DNP << 24
  uint32_t *mask = nullptr;                            // 256 words: the PID selection, bit pid & 31 of word pid >> 5
  uint32_t *crc = nullptr;                             // 256 entries: the CRC-8 byte table
};

struct MaRun {
  const uint8_t *ts = nullptr;
  uint32_t i0 = 0, n = 0;          // TS packets [i0, i0 + n) of ts
  uint32_t unit_byte = 0, dnp = 0; // of packet i0's unit, from the previous call's resume position
  uint8_t *out = nullptr;
  uint32_t cap = 0;                // BBFRAMEs
  int flush = 0;
};

// fills tab (host): the CRC-8 byte table of generator 0xD5
void modeadapt_host_table(uint32_t *tab);
// assigns d's scratch pointers inside base (nullptr: sizing only); returns the bytes needed
size_t modeadapt_layout(MaDev &d, void *base);
// every pass of one run on stream; no host round trip
hipError_t modeadapt_launch(const MaDev &d, const MaRun &r, hipStream_t stream);

}  // namespace t2
#endif
