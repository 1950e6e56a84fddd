// T2-MI output on the GPU (dvbt2ll_t2mi_out_*, include/dvbt2ll_hip.h): device state, the create-time position walk
// and the launch entry.
#ifndef T2MI_OUT_KERNELS_H
#define T2MI_OUT_KERNELS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace t2 {

constexpr int T2MO_MAX_PLP = 8;
constexpr int T2MO_MAX_AUX = 4;
constexpr int T2MO_MAX_T = 10 + 8192;   // longest T2-MI packet: payload_len 0xFFFF bits
constexpr int T2MO_TAB_WORDS = 256 + T2MO_MAX_T + 1;

// one packet of a T2 frame: the same for every frame of the handle
struct T2moPkt {
  uint32_t off;      // first byte, relative to the frame's first byte in the T2-MI stream
  uint32_t T;        // 6 + payload bytes + 4
  uint32_t blk;      // a BBFRAME packet: its block within the PLP's F blocks of the frame
  uint16_t bits;     // payload_len
  uint8_t type;
  uint8_t src;       // 0 .. 7: PLP k; 8 + a: aux slot a
};
static_assert(sizeof(T2moPkt) == 16, "packet descriptor layout");

struct T2moDev {
  int pid = 0, stream_id = 0, nplp = 0, fps = 1;
  int plp_id[T2MO_MAX_PLP] = {};
  uint32_t Lb[T2MO_MAX_PLP] = {}, F[T2MO_MAX_PLP] = {};
  uint32_t P = 0;            // packets per T2 frame
  uint32_t B = 0;            // T2-MI stream bytes per T2 frame
  uint32_t max_frames = 0;
  // scratch, carved by t2mo_layout
  T2moPkt *pkt = nullptr;    // P + 1 (the last: off = B)
  uint32_t *tq = nullptr;    // per packet of a call (max_frames P + 1): the TS packet its first byte lies in
  uint8_t *td = nullptr;     // ... and that byte's offset in that TS packet's stream bytes, 0 .. 182
  uint32_t *crc = nullptr;   // per packet of a call
  uint32_t *tab = nullptr;   // 256 CRC table entries, then x^(8 n) mod G for n <= T2MO_MAX_T
};

struct T2moRun {
  const uint8_t *bb[T2MO_MAX_PLP] = {};
  const uint8_t *aux = nullptr;
  size_t aux_stride = 0;
  uint32_t aux_off[T2MO_MAX_AUX] = {};
  uint32_t fi0 = 0, sf0 = 0;   // start.frame % fps, (start.frame / fps) & 15
  uint32_t count0 = 0, cc0 = 0;
  uint32_t nframes = 0;
  uint32_t G = 0;              // T2-MI packets of the call: nframes P
  uint32_t E = 0;              // T2-MI stream bytes of the call: nframes B
  uint32_t N = 0;              // TS packets of the call
  uint8_t *out = nullptr;
};

// per T2 frame boundary f = 0 .. max_frames, host side: the TS packet frame f's first byte lies in, its offset there,
// and the PUSI packets among the TS packets that hold a packet start of the frames before f
struct T2moFrames {
  std::vector<uint32_t> q0, pusi;
  std::vector<uint8_t> d0;
  // TS packets a call of n frames writes
  uint32_t ts_packets(uint32_t n) const { return q0[n] + (d0[n] ? 1u : 0u); }
};

// fills tab (host): the CRC-32/MPEG-2 byte table and the powers of x^8
void t2mo_host_tables(uint32_t *tab);
// the sequential walk over max_frames P + 1 packet starts: every call begins on a TS packet boundary, so the
// positions of a call's packets depend on nothing but their index.  pkt: the P + 1 descriptors.
void t2mo_host_walk(const T2moDev &d, const T2moPkt *pkt, std::vector<uint32_t> &tq, std::vector<uint8_t> &td,
                    T2moFrames &fr);
// assigns d's scratch pointers inside base (nullptr: sizing only); returns the bytes needed
size_t t2mo_layout(T2moDev &d, void *base);
// the CRC pass and the emit pass of one run on stream; no host round trip
hipError_t t2mo_launch(const T2moDev &d, const T2moRun &r, hipStream_t stream);

}  // namespace t2
#endif
