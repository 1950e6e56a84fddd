// MPE encapsulation on the GPU (dvbt2ll_mpe_*, include/dvbt2ll_hip.h): device state and the launch entry.
#ifndef MPE_KERNELS_H
#define MPE_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2 {

// the device result, 64-bit words (t2_capi.cpp copies them into dvbt2ll_mpe_result)
enum : int {
  MPE_R_PDU = 0, MPE_R_SECTION_BYTE, MPE_R_CC,
  MPE_R_PDUS_IN, MPE_R_SECTIONS, MPE_R_SKIPPED_LEN, MPE_R_SKIPPED_TYPE, MPE_R_MAPPED, MPE_R_TS_PACKETS, MPE_R_PUSI,
  MPE_R_PAD, MPE_R_FLUSHED,
  MPE_R_WORDS = 16
};

constexpr int MPE_HEADER = 12;                         // section bytes before the datagram
constexpr int MPE_MAX_PDU = 4080;                      // the longest datagram: a section has at most 4096 bytes
constexpr int MPE_MAX_SECTION = MPE_HEADER + MPE_MAX_PDU + 4;
constexpr int MPE_TAB_WORDS = 256 + MPE_MAX_SECTION + 1;   // the CRC-32 byte table, then x^(8 n) mod G, n = 0 .. 4096
constexpr int MPE_MAP_STATES = 184;                    // entries of a tile's transition map (the state is 0 or 2 .. 183)
constexpr int MPE_TILE = 512;                          // PDUs per tile of the state scan

struct MpeDev {
  int pid = 0, mac_mode = 0, packing = 1;
  uint8_t mac[6] = {};
  uint32_t max_pdus = 0;
  // scratch, carved by mpe_layout
  unsigned long long *res = nullptr;   // MPE_R_WORDS, then the control words (32-bit) in two more
  uint32_t *ctl = nullptr;             // packets completed, the end state, the start's section_byte as taken, long ones
  uint32_t *len = nullptr;             // per PDU: the section's length n (0: skipped) | the skip reason | MAC mapped
  uint32_t *hdr = nullptr;             // per PDU: the section's 12 header bytes as three little-endian words
  uint32_t *crc = nullptr;             // per PDU: the section's CRC_32
  uint32_t *lng = nullptr;             // the PDUs whose section the CRC pass gives a wavefront, in no order
  uint32_t *pkt = nullptr;             // per PDU: the packet its section's first byte of this call lies in
  uint8_t *at = nullptr;               // per PDU: that byte's payload offset (0: it continues an earlier call's section)
  uint32_t *tile = nullptr;            // packing 0: the sum scan's tile offsets and total
  uint32_t *maps = nullptr;            // packing 1: per tile, per entry state: packets completed << 8 | exit state
  uint32_t *ent_q = nullptr, *ent_pk = nullptr;   // packing 1: per tile, the state and packet count it is entered with
  uint32_t *tab = nullptr;             // MPE_TAB_WORDS
};

struct MpeRun {
  const uint8_t *pdu = nullptr;
  uint32_t pdu_len = 0;
  const uint32_t *off = nullptr;       // n_pdus + 1 offsets
  uint32_t i0 = 0, n = 0;              // PDUs [i0, i0 + n)
  uint32_t section_byte = 0, cc = 0;   // of PDU i0's section, from the previous call's resume position
  uint8_t *out = nullptr;
  uint32_t cap = 0;                    // TS packets
  int flush = 0;
};

// fills tab (host): the CRC-32 byte table of generator 0x04C11DB7 and the powers of x^8
void mpe_host_tables(uint32_t *tab);
// assigns d's scratch pointers inside base (nullptr: sizing only); returns the bytes needed
size_t mpe_layout(MpeDev &d, void *base);
// the most TS packets that n PDUs lying side by side in pdu_len bytes can become (overlapping ones can become more)
uint64_t mpe_packet_estimate(const MpeDev &d, uint64_t pdu_len, uint64_t n);
// the most TS packets that n PDUs inside pdu_len bytes can become, wherever the offsets put them
uint64_t mpe_packet_limit(const MpeDev &d, uint64_t pdu_len, uint64_t n);
// every pass of one run on stream; no host round trip
hipError_t mpe_launch(const MpeDev &d, const MpeRun &r, hipStream_t stream);

}  // namespace t2
#endif
