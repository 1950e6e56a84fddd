// MPE-FEC encapsulation on the GPU (dvbt2ll_mpefec_*, include/dvbt2ll_hip.h): device state and the launch entry.
#ifndef MPEFEC_KERNELS_H
#define MPEFEC_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace t2 {

// the device result, 64-bit words (t2_capi.cpp copies them into dvbt2ll_mpefec_result)
enum : int {
  MF_R_PDU = 0, MF_R_SECTION, MF_R_SECTION_BYTE, MF_R_CC, MF_R_FRAME,
  MF_R_PDUS_IN, MF_R_SECTIONS, MF_R_FEC_SECTIONS, MF_R_FRAMES, MF_R_SKIPPED_LEN, MF_R_SKIPPED_TYPE, MF_R_MAPPED,
  MF_R_TS_PACKETS, MF_R_PUSI, MF_R_PAD, MF_R_FLUSHED,
  MF_R_WORDS = 16,
  MF_CTL_WORDS = 16                                    // 32-bit control words behind the result
};

constexpr int MF_HEADER = 12;                          // section bytes before the datagram / the RS column
constexpr int MF_MAX_PDU = 4080;
constexpr int MF_MAX_SECTION = MF_HEADER + MF_MAX_PDU + 4;
constexpr int MF_TAB_WORDS = 256 + MF_MAX_SECTION + 1; // the CRC-32 byte table, then x^(8 n) mod G, n = 0 .. 4096
constexpr int MF_RS_WORDS = 256 * 16;                  // per feedback symbol: its 64 parity bytes as 16 words
constexpr int MF_MAP_STATES = 184;
constexpr int MF_TILE = 512;                           // sections per tile of the state scan
constexpr int MF_DATA_COLS = 191, MF_RS_COLS = 64;

struct MfDev {
  int pid = 0, mac_mode = 0, packing = 1;
  uint8_t mac[6] = {};
  uint32_t rows = 256, D = 191, K = 64;
  uint32_t max_pdus = 0, max_frames = 0, max_items = 0;
  // scratch, carved by mf_layout
  unsigned long long *res = nullptr;   // MF_R_WORDS, then the control words
  uint32_t *ctl = nullptr;
  uint32_t *len = nullptr;             // per PDU: the datagram's length p (0: skipped) | the skip reason | MAC mapped
  uint32_t *macw = nullptr;            // per PDU: MAC_address_6 | MAC_address_5 << 8
  unsigned long long *pre = nullptr;   // n + 1: before PDU i, the valid lengths' sum << 25 | the valid PDUs' count
  unsigned long long *tile = nullptr;  // the sum scan's tile offsets and total
  uint32_t *end = nullptr;             // per PDU: a frame that begins here ends before this index | closed << 31
  uint32_t *fs = nullptr;              // max_frames + 3: the first index of the call's frames, then of what follows
  uint32_t *ilen = nullptr;            // per section (item): its length | FEC section << 31
  uint32_t *isrc = nullptr;            // per section: the PDU, or frame x K + column
  uint32_t *ihdr = nullptr;            // per section: the 12 header bytes as three little-endian words
  uint32_t *icrc = nullptr;            // per section: CRC_32
  uint32_t *lng = nullptr;             // the sections the CRC pass gives a wavefront, in no order
  uint32_t *pkt = nullptr;             // per section: the packet its first byte of this call lies in
  uint8_t *at = nullptr;               // per section: that byte's payload offset (0: it continues an earlier call's)
  uint32_t *maps = nullptr, *ent_q = nullptr, *ent_pk = nullptr;   // the state scan, as the MPE handle's
  uint32_t *tab = nullptr;             // MF_TAB_WORDS
  uint32_t *rstab = nullptr;           // MF_RS_WORDS
  uint8_t *tbl = nullptr;              // (max_frames + 1) x D x rows: the application data tables' first D columns
  uint8_t *par = nullptr;              // (max_frames + 1) x K x rows: the RS columns sent
};

struct MfRun {
  const uint8_t *pdu = nullptr;
  uint32_t pdu_len = 0;
  const uint32_t *off = nullptr;       // n_pdus + 1 offsets
  uint32_t i0 = 0, n = 0;              // PDUs [i0, i0 + n)
  uint32_t section = 0, section_byte = 0, cc = 0, frame = 0;   // the start position
  uint8_t *out = nullptr;
  uint32_t cap = 0;                    // TS packets
  int flush = 0;
};

// fills tab (MF_TAB_WORDS: CRC-32) and rstab (MF_RS_WORDS: v x g_63 .. v x g_0 for every symbol v) on the host
void mf_host_tables(uint32_t *tab, uint32_t *rstab);
// assigns d's scratch pointers inside base (nullptr: sizing only); returns the bytes needed
size_t mf_layout(MfDev &d, void *base);
// the most TS packets that n PDUs lying side by side in pdu_len bytes can become, FEC sections included
uint64_t mf_packet_estimate(const MfDev &d, uint64_t pdu_len, uint64_t n);
// the most TS packets that n PDUs inside pdu_len bytes can become, wherever the offsets put them
uint64_t mf_packet_limit(const MfDev &d, uint64_t pdu_len, uint64_t n);
// every pass of one run on stream; no host round trip
hipError_t mf_launch(const MfDev &d, const MfRun &r, hipStream_t stream);

}  // namespace t2
#endif
