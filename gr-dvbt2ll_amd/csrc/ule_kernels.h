// ULE encapsulation on the GPU (dvbt2ll_ule_*, include/dvbt2ll_hip.h): device state and the launch entry.
#ifndef ULE_KERNELS_H
#define ULE_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2 {

// the device result, 64-bit words (t2_capi.cpp copies them into dvbt2ll_ule_result)
enum : int {
  ULE_R_PDU = 0, ULE_R_SNDU_BYTE, ULE_R_CC,
  ULE_R_PDUS_IN, ULE_R_SNDUS, ULE_R_SKIPPED_LEN, ULE_R_SKIPPED_TYPE, ULE_R_TS_PACKETS, ULE_R_PUSI, ULE_R_PAD,
  ULE_R_FLUSHED,
  ULE_R_WORDS = 16
};

constexpr int ULE_MAX_SNDU = 4 + 32767;              // the longest SNDU
constexpr int ULE_TAB_WORDS = 256 + ULE_MAX_SNDU + 1;  // the CRC-32 byte table, then x^(8 n) mod G for n = 0 .. ULE_MAX_SNDU
constexpr int ULE_MAP_STATES = 184;                  // entries of a tile's transition map (the state is 0 or 2 .. 182)
constexpr int ULE_TILE = 512;                        // PDUs per tile of the state scan

struct UleDev {
  int pid = 0, d_bit = 0, packing = 1;
  uint8_t dest[6] = {};
  uint32_t max_pdus = 0;
  // scratch, carved by ule_layout
  unsigned long long *res = nullptr;   // ULE_R_WORDS, then the control words (32-bit) in two more
  uint32_t *ctl = nullptr;             // packets completed, the end state, the start's sndu_byte as taken, long SNDUs
  uint32_t *len = nullptr;             // per PDU: the SNDU's length n (0: skipped) | the skip reason
  uint16_t *typ = nullptr;             // per PDU: the Type field
  uint32_t *crc = nullptr;             // per PDU: the SNDU's CRC-32
  uint32_t *lng = nullptr;             // the PDUs whose SNDU the CRC pass gives a wavefront, in no order
  uint32_t *pkt = nullptr;             // per PDU: the packet its SNDU's first byte of this call lies in
  uint8_t *at = nullptr;               // per PDU: that byte's payload offset (0: it continues an earlier call's SNDU)
  uint32_t *tile = nullptr;            // packing 0: the sum scan's tile offsets and total
  uint32_t *maps = nullptr;            // packing 1: per tile, per entry state: packets completed << 8 | exit state
  uint32_t *ent_q = nullptr, *ent_pk = nullptr;   // packing 1: per tile, the state and packet count it is entered with
  uint32_t *tab = nullptr;             // ULE_TAB_WORDS
};

struct UleRun {
  const uint8_t *pdu = nullptr;
  uint32_t pdu_len = 0;
  const uint32_t *off = nullptr;       // n_pdus + 1 offsets
  const uint16_t *type = nullptr;      // n_pdus type fields, or nullptr
  uint32_t i0 = 0, n = 0;              // PDUs [i0, i0 + n)
  uint32_t sndu_byte = 0, cc = 0;      // of PDU i0's SNDU, from the previous call's resume position
  uint8_t *out = nullptr;
  uint32_t cap = 0;                    // TS packets
  int flush = 0;
};

// fills tab (host): the CRC-32 byte table of generator 0x04C11DB7 and the powers of x^8
void ule_host_tables(uint32_t *tab);
// assigns d's scratch pointers inside base (nullptr: sizing only); returns the bytes needed
size_t ule_layout(UleDev &d, void *base);
// the most TS packets that n PDUs lying side by side in pdu_len bytes can become (overlapping ones can become more)
uint64_t ule_packet_estimate(const UleDev &d, uint64_t pdu_len, uint64_t n);
// the most TS packets that n PDUs inside pdu_len bytes can become, wherever the offsets put them
uint64_t ule_packet_limit(const UleDev &d, uint64_t pdu_len, uint64_t n);
// every pass of one run on stream; no host round trip
hipError_t ule_launch(const UleDev &d, const UleRun &r, hipStream_t stream);

}  // namespace t2
#endif
