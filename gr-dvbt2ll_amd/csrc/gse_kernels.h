// GSE encapsulation on the GPU (dvbt2ll_gse_*, include/dvbt2ll_hip.h): device state and the launch entry.
#ifndef GSE_KERNELS_H
#define GSE_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2 {

// the device result, 64-bit words (t2_capi.cpp copies them into dvbt2ll_gse_result)
enum : int {
  GSE_R_PDU = 0, GSE_R_PDU_BYTE, GSE_R_FRAG_ID,
  GSE_R_PDUS_IN, GSE_R_COMPLETE, GSE_R_FRAGMENTED, GSE_R_PACKETS, GSE_R_SKIPPED_LEN, GSE_R_SKIPPED_TYPE,
  GSE_R_BBFRAMES, GSE_R_PAD, GSE_R_FLUSHED,
  GSE_R_WORDS = 16
};

constexpr int GSE_MAX_PDU = 4090;                    // the longest PDU (without a label): GSE Length 4095 - 5
constexpr int GSE_TAB_WORDS = 256 + 4096 + 1;        // the CRC-32 byte table, then x^(8 n) mod G for n = 0 .. 4096
constexpr int GSE_TILE = 256;                        // PDUs per tile of the position tables
constexpr int GSE_STATE_BITS = 13;                   // a table entry: frames closed << 13 | the exit state u < 8192
constexpr int GSE_CRC_BLOCKS = 64;                   // the CRC pass's grid cap: 4 fragmented PDUs a workgroup a trip
constexpr int GSE_COUNT_BLOCKS = 64;                 // the count pass strides over the PDUs past 64 x 256

struct GseDev {
  uint32_t D = 0, Lb = 0;              // data-field bytes, BBFRAME bytes (kbch / 8 = D + 10)
  uint32_t L = 0, lt = 0;              // label bytes (6, 3, 0) and the Label Type that says so
  uint8_t label[6] = {};
  uint32_t matype = 0;                 // MATYPE-1 << 8 | MATYPE-2
  uint32_t max_pdus = 0;
  // scratch, carved by gse_layout
  unsigned long long *res = nullptr;   // GSE_R_WORDS, then the control words (32-bit) in two more
  uint32_t *ctl = nullptr;             // frames closed, the end state, the start's pdu_byte as taken, fragmented PDUs
  uint32_t *len = nullptr;             // per PDU: its length (0: skipped) | the skip reason
  uint16_t *typ = nullptr;             // per PDU: the Protocol Type
  uint32_t *crc = nullptr;             // per fragmented PDU: its CRC-32
  uint32_t *frg = nullptr;             // the fragmented PDUs, in no order
  uint32_t *frm = nullptr;             // per PDU: the frame its first packet of this call lies in
  uint16_t *at = nullptr;              // per PDU: that packet's offset in the data field
  uint32_t *maps = nullptr;            // per tile, per entry state u: frames closed << 13 | exit state
  uint32_t *ent_u = nullptr, *ent_fr = nullptr;   // per tile: the state and the frame count it is entered with
  uint32_t *tab = nullptr;             // GSE_TAB_WORDS
};

struct GseRun {
  const uint8_t *pdu = nullptr;
  uint32_t pdu_len = 0;
  const uint32_t *off = nullptr;       // n_pdus + 1 offsets
  const uint16_t *type = nullptr;      // n_pdus protocol types, or nullptr
  uint32_t i0 = 0, n = 0;              // PDUs [i0, i0 + n)
  uint32_t pdu_byte = 0, frag_id = 0;  // of PDU i0, from the previous call's resume position
  uint8_t *out = nullptr;
  uint32_t cap = 0;                    // BBFRAMEs
  int flush = 0;
};

// fills tab (host): the CRC-32 byte table of generator 0x04C11DB7 and the powers of x^8
void gse_host_tables(uint32_t *tab);
// assigns d's scratch pointers inside base (nullptr: sizing only); returns the bytes needed:
// about 22 bytes per PDU of max_pdus, and 4 D + 8 bytes per tile of GSE_TILE PDUs
size_t gse_layout(GseDev &d, void *base);
// the most BBFRAMEs that n PDUs lying side by side in pdu_len bytes can become (overlapping ones can become more)
uint64_t gse_frame_estimate(const GseDev &d, uint64_t pdu_len, uint64_t n);
// the most BBFRAMEs that n PDUs inside pdu_len bytes can become, wherever the offsets put them
uint64_t gse_frame_limit(const GseDev &d, uint64_t pdu_len, uint64_t n);
// every pass of one run on stream; no host round trip
hipError_t gse_launch(const GseDev &d, const GseRun &r, hipStream_t stream);

}  // namespace t2
#endif
