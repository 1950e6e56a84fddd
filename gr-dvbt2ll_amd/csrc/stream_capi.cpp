// stream_capi.cpp -- C ABI (include/dvbt2ll_hip.h): the stream handles beside the chain.
//
// The T2-MI deframer, the mode adapter, the ULE / MPE / MPE-FEC / GSE encapsulators, the TS multiplexer and the T2-MI
// framer.  Each handle has its scratch (sized at create) and no stream state: all passes of a run go to the caller's
// stream, and the result stays on the device until get_result.  What they share is here once: the run ordering
// (StreamHandle), and for the four PDU-batch encapsulators the argument prologue (pdu_run_args) and the host run's
// device copies (PduStage).  The *_params_from_chain functions read a chain and are beside it in t2_capi.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "capi_common.h"
#include "t2_kernels.h"
#include "modeadapt_kernels.h"
#include "ule_kernels.h"
#include "mpe_kernels.h"
#include "mpefec_kernels.h"
#include "tsmux_kernels.h"
#include "tsmux_plan.h"
#include "gse_kernels.h"
#include "t2mi_kernels.h"
#include "t2mi_out_kernels.h"

using namespace t2;

namespace {

// The ordering of a handle's runs.  The runs share the handle's scratch and result words, so a run on another stream
// than the last one's first waits for the last run's event, and whoever reads or regrows what a run uses waits for it
// on the host.
//
// Destruction order: the wait on `done` first, then the handle's device buffers, then the stream.  A handle holds its
// StreamHandle as the FIRST member, so the stream goes last, and keeps a one-line destructor `{ s.drain(); }`, so the
// wait comes before the members behind it are freed (a base class or a member alone cannot do both: either's own
// destructor runs after the buffers are gone).
struct StreamHandle {
  DeviceCtx ctx;
  hipEvent_t done = nullptr;     // the last run
  hipStream_t last = nullptr;
  bool ran = false;

  int init(int device) {
    int r = ctx.init(device);
    if (r) return r;
    HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    return 0;
  }
  // before a run's launches: *st is the caller's stream, or the handle's own for null
  int begin(void *stream, hipStream_t *st) {
    HIP_TRY(hipSetDevice(ctx.device));
    *st = stream ? (hipStream_t)stream : ctx.stream;
    if (ran && last != *st) HIP_TRY(hipStreamWaitEvent(*st, done, 0));
    return 0;
  }
  // after them
  int end(hipStream_t st) {
    HIP_TRY(hipEventRecord(done, st));
    last = st;
    ran = true;
    return 0;
  }
  // the last run is complete
  int wait() {
    HIP_TRY(hipSetDevice(ctx.device));
    if (ran) HIP_TRY(hipEventSynchronize(done));
    return 0;
  }
  // the last run's N result words
  template <size_t N>
  int read(const void *res_dev, uint64_t (&w)[N]) {
    int e = wait();
    if (e) return e;
    HIP_TRY(hipMemcpy(w, res_dev, sizeof w, hipMemcpyDeviceToHost));
    return 0;
  }
  void drain() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
    done = nullptr;
  }
  ~StreamHandle() { drain(); }
};

// the head of every *_create: the handle with its device, stream and event
template <class H>
int new_handle(int device, std::unique_ptr<H> &h) {
  h.reset(new (std::nothrow) H());
  if (!h) return DVBT2LL_ENOMEM;
  return h->s.init(device);
}

// a handle's scratch: sized by the block's layout function, which then points the Dev's arrays into it
template <class Dev>
int lay_out(DevBuf &scratch, Dev &d, size_t (*layout)(Dev &, void *)) {
  if (scratch.ensure(layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)layout(d, scratch.p);
  return 0;
}

// What the run arguments of the four PDU-batch encapsulators have in common: the checks of the pointers, of the sizes
// against the handle's and of the position's PDU, and the Run fields they fill.  A block checks the rest of its
// position after this, before anything is launched.
template <class H, class Pos, class Run>
int pdu_run_args(const H *h, const void *pdu, int64_t pdu_len, const uint32_t *off, int64_t n_pdus, const Pos *start,
                 void *out, int64_t cap, Run &r) {
  if (!h || !pdu || !off || !start || !out) return DVBT2LL_EINVAL;
  if (pdu_len < 0 || pdu_len > h->p.max_pdu_bytes || n_pdus < 0 || n_pdus > h->p.max_pdus || cap < 0)
    return DVBT2LL_EINVAL;
  if (start->pdu < 0 || start->pdu > n_pdus) return DVBT2LL_EINVAL;
  r.pdu = (const uint8_t *)pdu;
  r.pdu_len = (uint32_t)pdu_len;
  r.off = off;
  r.i0 = (uint32_t)start->pdu;
  r.n = (uint32_t)(n_pdus - start->pdu);
  r.out = (uint8_t *)out;
  r.cap = (uint32_t)std::min<int64_t>(cap, (int64_t)1 << 30);
  return DVBT2LL_OK;
}

// The device copies of a PDU-batch encapsulator's host run: the PDU bytes, the n + 1 offsets, the types where the
// block has them and the caller gave them, and room for the output.
struct PduStage {
  DevBuf pdu, off, type, out;
  // Grows the buffers and queues the uploads on st.  out_bytes is the capacity the run is given times the output
  // unit.  The caller has clamped that capacity by its block's limit function: no more units than the PDUs can become
  // wherever the offsets put them, whatever the caller's capacity says, so this buffer holds all the run may write.
  int stage(hipStream_t st, const void *pdu_h, int64_t pdu_len, const uint32_t *off_h, const uint16_t *type_h,
            int64_t n_pdus, size_t out_bytes) {
    if (pdu.ensure((size_t)std::max<int64_t>(pdu_len, 1))) return DVBT2LL_ENOMEM;
    if (off.ensure((size_t)(n_pdus + 1) * 4)) return DVBT2LL_ENOMEM;
    if (type_h && type.ensure((size_t)std::max<int64_t>(n_pdus, 1) * 2)) return DVBT2LL_ENOMEM;
    if (out.ensure(out_bytes + 16)) return DVBT2LL_ENOMEM;
    if (pdu_len) HIP_TRY(hipMemcpyAsync(pdu.p, pdu_h, (size_t)pdu_len, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(off.p, off_h, (size_t)(n_pdus + 1) * 4, hipMemcpyHostToDevice, st));
    if (type_h && n_pdus) HIP_TRY(hipMemcpyAsync(type.p, type_h, (size_t)n_pdus * 2, hipMemcpyHostToDevice, st));
    return 0;
  }
  const uint16_t *types(const uint16_t *type_h) const { return type_h ? type.as<uint16_t>() : nullptr; }
  // the output's first bytes, once get_result has synchronised
  int fetch(void *dst, int64_t bytes) {
    if (bytes > 0) HIP_TRY(hipMemcpy(dst, out.p, (size_t)bytes, hipMemcpyDeviceToHost));
    return DVBT2LL_OK;
  }
};

bool t2mi_valid_len(int L) {
  static const int kbch[14] = {32208, 38688, 43040, 48408, 51648, 53840, 7032, 9552, 10632, 11712, 12432, 13152,
                               5232, 6312};   // the codes of build_fec (t2_plan.cpp fec_numbers)
  for (int k : kbch)
    if (L == k / 8) return true;
  return false;
}

// Kbch of (framesize, rate) as build_fec has them (t2_plan.cpp fec_numbers); 0: not a code
int modeadapt_kbch_of(int framesize, int rate) {
  static const int normal[6] = {32208, 38688, 43040, 48408, 51648, 53840};
  static const int shortf[8] = {7032, 9552, 10632, 11712, 12432, 13152, 5232, 6312};
  if (framesize == 1) return rate >= 0 && rate < 6 ? normal[rate] : 0;
  if (framesize == 0) return rate >= 0 && rate < 8 ? shortf[rate] : 0;
  return 0;
}

}  // namespace

// ============================================================================ T2-MI input
// Scratch sized at create from max_ts_bytes and max_packets; the passes are in t2mi_kernels.hip.
struct dvbt2ll_t2mi {
  StreamHandle s;
  dvbt2ll_t2mi_params p{};
  T2miDev dev;
  DevBuf scratch, ts_tmp, out_tmp[DVBT2LL_MAX_PLP];
  ~dvbt2ll_t2mi() { s.drain(); }
};

static bool t2mi_params_ok(const dvbt2ll_t2mi_params &p) {
  if (p.pid < 0 || p.pid > 0x1FFE || p.stream_id < -1 || p.stream_id > 7) return false;
  if (p.nplp < 1 || p.nplp > DVBT2LL_MAX_PLP) return false;
  if (p.max_ts_bytes < 188 || p.max_ts_bytes % 188 || p.max_ts_bytes >= ((int64_t)1 << 31)) return false;
  if (p.max_packets < 1 || p.max_packets > (1 << 28)) return false;
  for (int k = 0; k < p.nplp; k++) {
    if (p.plp_id[k] < 0 || p.plp_id[k] > 255 || !t2mi_valid_len(p.bbframe_bytes[k])) return false;
    for (int j = 0; j < k; j++)
      if (p.plp_id[j] == p.plp_id[k]) return false;
  }
  return true;
}

extern "C" int dvbt2ll_t2mi_create(const dvbt2ll_t2mi_params *p, int device, dvbt2ll_t2mi **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (!t2mi_params_ok(*p)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_t2mi> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  T2miDev &d = h->dev;
  d.pid = p->pid;
  d.stream_id = p->stream_id;
  d.nplp = p->nplp;
  for (int k = 0; k < p->nplp; k++) { d.plp_id[k] = p->plp_id[k]; d.L[k] = p->bbframe_bytes[k]; }
  d.max_ts = (uint32_t)(p->max_ts_bytes / 188);
  d.max_packets = (uint32_t)p->max_packets;
  if ((r = lay_out(h->scratch, d, t2mi_layout))) return r;
  std::vector<uint32_t> tab(T2MI_TAB_WORDS);
  t2mi_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, T2MI_R_WORDS * 8));
  *out = h.release();
  return DVBT2LL_OK;
}

static int t2mi_run_args(const dvbt2ll_t2mi *h, const void *ts, int64_t ts_len, const dvbt2ll_t2mi_pos *start,
                         void *const *out, const int64_t *cap, T2miRun &r) {
  if (!h || !ts || !start || !out || !cap) return DVBT2LL_EINVAL;
  if (ts_len < 0 || ts_len % 188 || ts_len > h->p.max_ts_bytes) return DVBT2LL_EINVAL;
  if (start->ts_offset < 0 || start->ts_offset % 188 || start->ts_offset > ts_len || start->skip < 0)
    return DVBT2LL_EINVAL;
  for (int k = 0; k < h->p.nplp; k++)
    if (!out[k] || cap[k] < 0) return DVBT2LL_EINVAL;
  r.ts = (const uint8_t *)ts;
  r.i0 = (uint32_t)(start->ts_offset / 188);
  r.n = (uint32_t)(ts_len / 188) - r.i0;
  r.skip = (uint32_t)start->skip;
  for (int k = 0; k < h->p.nplp; k++) {
    r.out[k] = (uint8_t *)out[k];
    r.cap[k] = (uint32_t)std::min<int64_t>(cap[k], (int64_t)1 << 30);
  }
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_run_device(dvbt2ll_t2mi *h, const void *ts_dev, int64_t ts_len,
                                       const dvbt2ll_t2mi_pos *start, void *const *out_dev,
                                       const int64_t *out_cap_blocks, void *stream) {
  T2miRun r;
  hipStream_t st;
  int e = t2mi_run_args(h, ts_dev, ts_len, start, out_dev, out_cap_blocks, r);
  if (e || (e = h->s.begin(stream, &st))) return e;
  HIP_TRY(t2mi_launch(h->dev, r, st));
  return h->s.end(st);
}

extern "C" int dvbt2ll_t2mi_get_result(dvbt2ll_t2mi *h, dvbt2ll_t2mi_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  uint64_t w[T2MI_R_WORDS];
  int e = h->s.read(h->dev.res, w);
  if (e) return e;
  memset(res, 0, sizeof *res);
  res->resume.ts_offset = (int64_t)w[T2MI_R_OFFSET];
  res->resume.skip = (int)w[T2MI_R_SKIP];
  res->packets = (int64_t)w[T2MI_R_PACKETS];
  int64_t *ts = &res->ts_contributing, *pk = &res->broken;
  for (int k = 0; k < 9; k++) ts[k] = (int64_t)w[T2MI_R_TS + k];
  for (int k = 0; k < 6; k++) pk[k] = (int64_t)w[T2MI_R_PKT + k];
  for (int k = 0; k < DVBT2LL_MAX_PLP; k++) res->blocks[k] = (int64_t)w[T2MI_R_BLOCKS + k];
  for (int k = 0; k < 256; k++) res->by_type[k] = (int64_t)w[T2MI_R_TYPE + k];
  return DVBT2LL_OK;
}

extern "C" int64_t dvbt2ll_t2mi_get_packets(dvbt2ll_t2mi *h, dvbt2ll_t2mi_packet *out, int64_t max_records) {
  static_assert(sizeof(dvbt2ll_t2mi_packet) == sizeof(T2miRec), "table record layout");
  if (!h || !out || max_records < 0) return DVBT2LL_EINVAL;
  int e = h->s.wait();
  if (e) return e;
  uint64_t n = 0;
  HIP_TRY(hipMemcpy(&n, h->dev.res + T2MI_R_PACKETS, 8, hipMemcpyDeviceToHost));
  const int64_t m = std::min<int64_t>((int64_t)n, max_records);
  if (m > 0) HIP_TRY(hipMemcpy(out, h->dev.table, (size_t)m * sizeof(T2miRec), hipMemcpyDeviceToHost));
  return m;
}

extern "C" int dvbt2ll_t2mi_run_host(dvbt2ll_t2mi *h, const void *ts, int64_t ts_len, const dvbt2ll_t2mi_pos *start,
                                     void *const *out, const int64_t *out_cap_blocks, dvbt2ll_t2mi_result *res) {
  T2miRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = t2mi_run_args(h, ts, ts_len, start, out, out_cap_blocks, r);
  if (e || (e = h->s.wait())) return e;
  hipStream_t st = h->s.ctx.stream;
  if (h->ts_tmp.ensure((size_t)std::max<int64_t>(ts_len, 1))) return DVBT2LL_ENOMEM;
  void *od[DVBT2LL_MAX_PLP] = {};
  for (int k = 0; k < h->p.nplp; k++) {
    if (h->out_tmp[k].ensure((size_t)r.cap[k] * h->p.bbframe_bytes[k] + 16)) return DVBT2LL_ENOMEM;
    od[k] = h->out_tmp[k].p;
  }
  if (ts_len) HIP_TRY(hipMemcpyAsync(h->ts_tmp.p, ts, (size_t)ts_len, hipMemcpyHostToDevice, st));
  if ((e = dvbt2ll_t2mi_run_device(h, h->ts_tmp.p, ts_len, start, od, out_cap_blocks, st))) return e;
  if ((e = dvbt2ll_t2mi_get_result(h, res))) return e;
  for (int k = 0; k < h->p.nplp; k++)
    if (res->blocks[k] > 0)
      HIP_TRY(hipMemcpy(out[k], od[k], (size_t)res->blocks[k] * h->p.bbframe_bytes[k], hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_t2mi_destroy(dvbt2ll_t2mi *h) { delete h; }

// ============================================================================ mode adapter
// Scratch sized at create from max_ts_bytes; the passes are in modeadapt_kernels.hip.
struct dvbt2ll_modeadapt {
  StreamHandle s;
  dvbt2ll_modeadapt_params p{};
  MaDev dev;
  DevBuf scratch, ts_tmp, out_tmp;
  ~dvbt2ll_modeadapt() { s.drain(); }
};

// the resolved Kbch of the parameters, or 0 when they are refused
static int modeadapt_params_kbch(const dvbt2ll_modeadapt_params &p) {
  const int kbch = p.kbch ? p.kbch : modeadapt_kbch_of(p.framesize, p.rate);
  if (kbch != 3072 && (kbch <= 0 || kbch % 8 || !t2mi_valid_len(kbch / 8))) return 0;
  if ((p.sis_mis != 0 && p.sis_mis != 1) || p.isi < 0 || p.isi > 255) return 0;
  if ((p.npd != 0 && p.npd != 1) || (p.pid_mask && !p.npd)) return 0;
  if (p.max_ts_bytes < 188 || p.max_ts_bytes % 188 || p.max_ts_bytes >= ((int64_t)1 << 31)) return 0;
  return kbch;
}

extern "C" int dvbt2ll_modeadapt_create(const dvbt2ll_modeadapt_params *p, int device, dvbt2ll_modeadapt **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  const int kbch = modeadapt_params_kbch(*p);
  if (!kbch) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_modeadapt> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  h->p.kbch = kbch;
  h->p.pid_mask = nullptr;   // copied to the device below: the caller's array is not kept
  MaDev &d = h->dev;
  d.npd = p->npd;
  d.has_mask = p->pid_mask != nullptr;
  d.L = (uint32_t)kbch / 8;
  d.D = d.L - 10;
  // MATYPE-1: TS_GS 11, SIS/MIS, CCM 1, ISSYI 0, NPD, EXT 00 (the chain's MATYPE_SIS / MATYPE_MIS with the NPD bit)
  d.matype = (uint32_t)(p->sis_mis ? MATYPE_SIS : MATYPE_MIS | p->isi) | (p->npd ? 0x0400u : 0u);
  d.max_ts = (uint32_t)(p->max_ts_bytes / 188);
  if ((r = lay_out(h->scratch, d, modeadapt_layout))) return r;
  uint32_t tab[256];
  modeadapt_host_table(tab);
  HIP_TRY(hipMemcpy(d.crc, tab, sizeof tab, hipMemcpyHostToDevice));
  if (p->pid_mask) HIP_TRY(hipMemcpy(d.mask, p->pid_mask, 1024, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, MA_R_WORDS * 8));
  *out = h.release();
  return DVBT2LL_OK;
}

static int modeadapt_run_args(const dvbt2ll_modeadapt *h, const void *ts, int64_t ts_len,
                              const dvbt2ll_modeadapt_pos *start, void *out, int64_t cap, MaRun &r) {
  if (!h || !ts || !start || !out) return DVBT2LL_EINVAL;
  if (ts_len < 0 || ts_len % 188 || ts_len > h->p.max_ts_bytes || cap < 0) return DVBT2LL_EINVAL;
  const int64_t n = ts_len / 188;
  const int U = h->p.npd ? 188 : 187;
  if (start->ts_packet < 0 || start->ts_packet > n || start->unit_byte < 0 || start->unit_byte >= U ||
      start->dnp < 0 || start->dnp > 255 || (start->dnp && !h->p.npd))
    return DVBT2LL_EINVAL;
  if ((start->unit_byte || start->dnp) && start->ts_packet == n) return DVBT2LL_EINVAL;
  r.ts = (const uint8_t *)ts;
  r.i0 = (uint32_t)start->ts_packet;
  r.n = (uint32_t)(n - start->ts_packet);
  r.unit_byte = (uint32_t)start->unit_byte;
  r.dnp = (uint32_t)start->dnp;
  r.out = (uint8_t *)out;
  r.cap = (uint32_t)std::min<int64_t>(cap, (int64_t)1 << 30);
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_modeadapt_run_device(dvbt2ll_modeadapt *h, const void *ts_dev, int64_t ts_len,
                                            const dvbt2ll_modeadapt_pos *start, void *out_dev, int64_t out_cap_blocks,
                                            int flush, void *stream) {
  MaRun r;
  hipStream_t st;
  int e = modeadapt_run_args(h, ts_dev, ts_len, start, out_dev, out_cap_blocks, r);
  if (e || (e = h->s.begin(stream, &st))) return e;
  r.flush = flush != 0;
  HIP_TRY(modeadapt_launch(h->dev, r, st));
  return h->s.end(st);
}

extern "C" int dvbt2ll_modeadapt_get_result(dvbt2ll_modeadapt *h, dvbt2ll_modeadapt_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  uint64_t w[MA_R_WORDS];
  int e = h->s.read(h->dev.res, w);
  if (e) return e;
  memset(res, 0, sizeof *res);
  res->resume.ts_packet = (int64_t)w[MA_R_TS_PACKET];
  res->resume.unit_byte = (int)w[MA_R_UNIT_BYTE];
  res->resume.dnp = (int)w[MA_R_DNP];
  int64_t *c = &res->packets_in;
  for (int k = 0; k < 8; k++) c[k] = (int64_t)w[MA_R_PACKETS_IN + k];
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_modeadapt_run_host(dvbt2ll_modeadapt *h, const void *ts, int64_t ts_len,
                                          const dvbt2ll_modeadapt_pos *start, void *out, int64_t out_cap_blocks,
                                          int flush, dvbt2ll_modeadapt_result *res) {
  MaRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = modeadapt_run_args(h, ts, ts_len, start, out, out_cap_blocks, r);
  if (e || (e = h->s.wait())) return e;
  hipStream_t st = h->s.ctx.stream;
  // no more BBFRAMEs than the buffer's packets can fill, whatever the capacity says
  const int64_t cap = std::min<int64_t>(r.cap, (int64_t)r.n * 188 / h->dev.D + 1);
  if (h->ts_tmp.ensure((size_t)std::max<int64_t>(ts_len, 1))) return DVBT2LL_ENOMEM;
  if (h->out_tmp.ensure((size_t)cap * h->dev.L + 16)) return DVBT2LL_ENOMEM;
  if (ts_len) HIP_TRY(hipMemcpyAsync(h->ts_tmp.p, ts, (size_t)ts_len, hipMemcpyHostToDevice, st));
  if ((e = dvbt2ll_modeadapt_run_device(h, h->ts_tmp.p, ts_len, start, h->out_tmp.p, out_cap_blocks, flush, st)))
    return e;
  if ((e = dvbt2ll_modeadapt_get_result(h, res))) return e;
  if (res->bbframes > 0)
    HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)res->bbframes * h->dev.L, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_modeadapt_destroy(dvbt2ll_modeadapt *h) { delete h; }

// ============================================================================ ULE encapsulator
// Scratch sized at create from max_pdus; the passes are in ule_kernels.hip.
struct dvbt2ll_ule {
  StreamHandle s;
  dvbt2ll_ule_params p{};
  UleDev dev;
  DevBuf scratch;
  PduStage tmp;
  ~dvbt2ll_ule() { s.drain(); }
};

static bool ule_params_ok(const dvbt2ll_ule_params &p) {
  if (p.pid < 0 || p.pid > 0x1FFE) return false;
  if ((p.d_bit != 0 && p.d_bit != 1) || (p.packing != 0 && p.packing != 1)) return false;
  if (p.max_pdu_bytes < 1 || p.max_pdu_bytes >= ((int64_t)1 << 31)) return false;
  return p.max_pdus >= 1 && p.max_pdus <= (1 << 24);   // 2^24 SNDUs of 180 packets: below 2^32 packets
}

extern "C" int dvbt2ll_ule_create(const dvbt2ll_ule_params *p, int device, dvbt2ll_ule **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (!ule_params_ok(*p)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_ule> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  UleDev &d = h->dev;
  d.pid = p->pid;
  d.d_bit = p->d_bit;
  d.packing = p->packing;
  memcpy(d.dest, p->dest, 6);
  d.max_pdus = (uint32_t)p->max_pdus;
  if ((r = lay_out(h->scratch, d, ule_layout))) return r;
  std::vector<uint32_t> tab(ULE_TAB_WORDS);
  ule_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (ULE_R_WORDS + 2) * 8));
  *out = h.release();
  return DVBT2LL_OK;
}

static int ule_run_args(const dvbt2ll_ule *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                        const uint16_t *type, int64_t n_pdus, const dvbt2ll_ule_pos *start, void *out, int64_t cap,
                        UleRun &r) {
  int e = pdu_run_args(h, pdu, pdu_len, off, n_pdus, start, out, cap, r);
  if (e) return e;
  if (start->sndu_byte < 0 || start->sndu_byte >= ULE_MAX_SNDU || start->cc < 0 || start->cc > 15 ||
      (start->sndu_byte && start->pdu == n_pdus))
    return DVBT2LL_EINVAL;
  r.type = type;
  r.sndu_byte = (uint32_t)start->sndu_byte;
  r.cc = (uint32_t)start->cc;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_ule_run_device(dvbt2ll_ule *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                                      const uint16_t *type_dev, int64_t n_pdus, const dvbt2ll_ule_pos *start,
                                      void *out_dev, int64_t out_cap_packets, int flush, void *stream) {
  UleRun r;
  hipStream_t st;
  int e = ule_run_args(h, pdu_dev, pdu_len, off_dev, type_dev, n_pdus, start, out_dev, out_cap_packets, r);
  if (e || (e = h->s.begin(stream, &st))) return e;
  r.flush = flush != 0;
  HIP_TRY(ule_launch(h->dev, r, st));
  return h->s.end(st);
}

extern "C" int dvbt2ll_ule_get_result(dvbt2ll_ule *h, dvbt2ll_ule_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  uint64_t w[ULE_R_WORDS];
  int e = h->s.read(h->dev.res, w);
  if (e) return e;
  memset(res, 0, sizeof *res);
  res->resume.pdu = (int64_t)w[ULE_R_PDU];
  res->resume.sndu_byte = (int)w[ULE_R_SNDU_BYTE];
  res->resume.cc = (int)w[ULE_R_CC];
  int64_t *c = &res->pdus_in;
  for (int k = 0; k < 8; k++) c[k] = (int64_t)w[ULE_R_PDUS_IN + k];
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_ule_run_host(dvbt2ll_ule *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                                    const uint16_t *type, int64_t n_pdus, const dvbt2ll_ule_pos *start, void *out,
                                    int64_t out_cap_packets, int flush, dvbt2ll_ule_result *res) {
  UleRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = ule_run_args(h, pdu, pdu_len, off, type, n_pdus, start, out, out_cap_packets, r);
  if (e || (e = h->s.wait())) return e;
  PduStage &t = h->tmp;
  hipStream_t st = h->s.ctx.stream;
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, ule_packet_limit(h->dev, r.pdu_len, r.n));
  if ((e = t.stage(st, pdu, pdu_len, off, type, n_pdus, (size_t)cap * 188))) return e;
  if ((e = dvbt2ll_ule_run_device(h, t.pdu.p, pdu_len, t.off.as<uint32_t>(), t.types(type), n_pdus, start, t.out.p,
                                  cap, flush, st)))
    return e;
  if ((e = dvbt2ll_ule_get_result(h, res))) return e;
  return t.fetch(out, res->ts_packets * 188);
}

extern "C" void dvbt2ll_ule_destroy(dvbt2ll_ule *h) { delete h; }

// ============================================================================ MPE encapsulator
// Scratch sized at create from max_pdus; the passes are in mpe_kernels.hip.
struct dvbt2ll_mpe {
  StreamHandle s;
  dvbt2ll_mpe_params p{};
  MpeDev dev;
  DevBuf scratch;
  PduStage tmp;
  ~dvbt2ll_mpe() { s.drain(); }
};

static bool mpe_params_ok(const dvbt2ll_mpe_params &p) {
  if (p.pid < 0 || p.pid > 0x1FFE) return false;
  if ((p.mac_mode != 0 && p.mac_mode != 1) || (p.packing != 0 && p.packing != 1)) return false;
  if (p.max_pdu_bytes < 1 || p.max_pdu_bytes >= ((int64_t)1 << 31)) return false;
  return p.max_pdus >= 1 && p.max_pdus <= (1 << 24);   // 2^24 sections of 23 packets: below 2^32 packets
}

extern "C" int dvbt2ll_mpe_create(const dvbt2ll_mpe_params *p, int device, dvbt2ll_mpe **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (!mpe_params_ok(*p)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_mpe> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  MpeDev &d = h->dev;
  d.pid = p->pid;
  d.mac_mode = p->mac_mode;
  d.packing = p->packing;
  memcpy(d.mac, p->mac, 6);
  d.max_pdus = (uint32_t)p->max_pdus;
  if ((r = lay_out(h->scratch, d, mpe_layout))) return r;
  std::vector<uint32_t> tab(MPE_TAB_WORDS);
  mpe_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (MPE_R_WORDS + 2) * 8));
  *out = h.release();
  return DVBT2LL_OK;
}

static int mpe_run_args(const dvbt2ll_mpe *h, const void *pdu, int64_t pdu_len, const uint32_t *off, int64_t n_pdus,
                        const dvbt2ll_mpe_pos *start, void *out, int64_t cap, MpeRun &r) {
  int e = pdu_run_args(h, pdu, pdu_len, off, n_pdus, start, out, cap, r);
  if (e) return e;
  if (start->section_byte < 0 || start->section_byte >= MPE_MAX_SECTION || start->cc < 0 || start->cc > 15 ||
      (start->section_byte && start->pdu == n_pdus))
    return DVBT2LL_EINVAL;
  r.section_byte = (uint32_t)start->section_byte;
  r.cc = (uint32_t)start->cc;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpe_run_device(dvbt2ll_mpe *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                                      int64_t n_pdus, const dvbt2ll_mpe_pos *start, void *out_dev,
                                      int64_t out_cap_packets, int flush, void *stream) {
  MpeRun r;
  hipStream_t st;
  int e = mpe_run_args(h, pdu_dev, pdu_len, off_dev, n_pdus, start, out_dev, out_cap_packets, r);
  if (e || (e = h->s.begin(stream, &st))) return e;
  r.flush = flush != 0;
  HIP_TRY(mpe_launch(h->dev, r, st));
  return h->s.end(st);
}

extern "C" int dvbt2ll_mpe_get_result(dvbt2ll_mpe *h, dvbt2ll_mpe_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  uint64_t w[MPE_R_WORDS];
  int e = h->s.read(h->dev.res, w);
  if (e) return e;
  memset(res, 0, sizeof *res);
  res->resume.pdu = (int64_t)w[MPE_R_PDU];
  res->resume.section_byte = (int)w[MPE_R_SECTION_BYTE];
  res->resume.cc = (int)w[MPE_R_CC];
  int64_t *c = &res->pdus_in;
  for (int k = 0; k < 9; k++) c[k] = (int64_t)w[MPE_R_PDUS_IN + k];
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpe_run_host(dvbt2ll_mpe *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                                    int64_t n_pdus, const dvbt2ll_mpe_pos *start, void *out, int64_t out_cap_packets,
                                    int flush, dvbt2ll_mpe_result *res) {
  MpeRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = mpe_run_args(h, pdu, pdu_len, off, n_pdus, start, out, out_cap_packets, r);
  if (e || (e = h->s.wait())) return e;
  PduStage &t = h->tmp;
  hipStream_t st = h->s.ctx.stream;
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, mpe_packet_limit(h->dev, r.pdu_len, r.n));
  if ((e = t.stage(st, pdu, pdu_len, off, nullptr, n_pdus, (size_t)cap * 188))) return e;
  if ((e = dvbt2ll_mpe_run_device(h, t.pdu.p, pdu_len, t.off.as<uint32_t>(), n_pdus, start, t.out.p, cap, flush, st)))
    return e;
  if ((e = dvbt2ll_mpe_get_result(h, res))) return e;
  return t.fetch(out, res->ts_packets * 188);
}

extern "C" void dvbt2ll_mpe_destroy(dvbt2ll_mpe *h) { delete h; }

// ============================================================================ MPE-FEC encapsulator
// Scratch sized at create from max_pdus and max_frames (the frames' tables and RS columns); the passes are in
// mpefec_kernels.hip.
struct dvbt2ll_mpefec {
  StreamHandle s;
  dvbt2ll_mpefec_params p{};
  MfDev dev;
  DevBuf scratch;
  PduStage tmp;
  ~dvbt2ll_mpefec() { s.drain(); }
};

static bool mpefec_params_ok(const dvbt2ll_mpefec_params &p) {
  if (p.pid < 0 || p.pid > 0x1FFE) return false;
  if ((p.mac_mode != 0 && p.mac_mode != 1) || (p.packing != 0 && p.packing != 1)) return false;
  if (p.max_pdu_bytes < 1 || p.max_pdu_bytes >= ((int64_t)1 << 31)) return false;
  if (p.max_pdus < 1 || p.max_pdus > (1 << 24)) return false;
  if (p.rows != 256 && p.rows != 512 && p.rows != 768 && p.rows != 1024) return false;
  if (p.data_columns < 1 || p.data_columns > MF_DATA_COLS || p.rs_columns < 1 || p.rs_columns > MF_RS_COLS) return false;
  return p.max_frames >= 1 && p.max_frames <= (1 << 16);
}

extern "C" int dvbt2ll_mpefec_create(const dvbt2ll_mpefec_params *p, int device, dvbt2ll_mpefec **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (!mpefec_params_ok(*p)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_mpefec> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  MfDev &d = h->dev;
  d.pid = p->pid;
  d.mac_mode = p->mac_mode;
  d.packing = p->packing;
  memcpy(d.mac, p->mac, 6);
  d.rows = (uint32_t)p->rows;
  d.D = (uint32_t)p->data_columns;
  d.K = (uint32_t)p->rs_columns;
  d.max_pdus = (uint32_t)p->max_pdus;
  d.max_frames = (uint32_t)p->max_frames;
  // a frame holds a datagram or more: no more frames than PDUs; one frame past max_frames is computed as well
  d.max_items = d.max_pdus + std::min(d.max_frames + 1, d.max_pdus) * d.K;
  if ((r = lay_out(h->scratch, d, mf_layout))) return r;
  std::vector<uint32_t> tab(MF_TAB_WORDS), rstab(MF_RS_WORDS);
  mf_host_tables(tab.data(), rstab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.rstab, rstab.data(), rstab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (MF_R_WORDS + MF_CTL_WORDS / 2) * 8));
  *out = h.release();
  return DVBT2LL_OK;
}

static int mpefec_run_args(const dvbt2ll_mpefec *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                           int64_t n_pdus, const dvbt2ll_mpefec_pos *start, void *out, int64_t cap, MfRun &r) {
  int e = pdu_run_args(h, pdu, pdu_len, off, n_pdus, start, out, cap, r);
  if (e) return e;
  // a frame holds at most D x rows datagrams (of one byte each) and K RS columns: no frame has a section past that
  const int64_t sections = (int64_t)h->p.data_columns * h->p.rows + h->p.rs_columns;
  if (start->section < 0 || start->section >= sections || start->section_byte < 0 ||
      start->section_byte >= MF_MAX_SECTION || start->cc < 0 || start->cc > 15 || start->frame < 0 ||
      start->frame > 0xFFF || ((start->section || start->section_byte) && start->pdu == n_pdus))
    return DVBT2LL_EINVAL;
  r.section = (uint32_t)start->section;
  r.section_byte = (uint32_t)start->section_byte;
  r.cc = (uint32_t)start->cc;
  r.frame = (uint32_t)start->frame;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpefec_run_device(dvbt2ll_mpefec *h, const void *pdu_dev, int64_t pdu_len,
                                         const uint32_t *off_dev, int64_t n_pdus, const dvbt2ll_mpefec_pos *start,
                                         void *out_dev, int64_t out_cap_packets, int flush, void *stream) {
  MfRun r;
  hipStream_t st;
  int e = mpefec_run_args(h, pdu_dev, pdu_len, off_dev, n_pdus, start, out_dev, out_cap_packets, r);
  if (e || (e = h->s.begin(stream, &st))) return e;
  r.flush = flush != 0;
  HIP_TRY(mf_launch(h->dev, r, st));
  return h->s.end(st);
}

extern "C" int dvbt2ll_mpefec_get_result(dvbt2ll_mpefec *h, dvbt2ll_mpefec_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  uint64_t w[MF_R_WORDS];
  int e = h->s.read(h->dev.res, w);
  if (e) return e;
  memset(res, 0, sizeof *res);
  res->resume.pdu = (int64_t)w[MF_R_PDU];
  res->resume.section = (int)w[MF_R_SECTION];
  res->resume.section_byte = (int)w[MF_R_SECTION_BYTE];
  res->resume.cc = (int)w[MF_R_CC];
  res->resume.frame = (int)w[MF_R_FRAME];
  res->pdus_in = (int64_t)w[MF_R_PDUS_IN];
  res->sections = (int64_t)w[MF_R_SECTIONS];
  res->fec_sections = (int64_t)w[MF_R_FEC_SECTIONS];
  res->frames = (int64_t)w[MF_R_FRAMES];
  res->skipped_len = (int64_t)w[MF_R_SKIPPED_LEN];
  res->skipped_type = (int64_t)w[MF_R_SKIPPED_TYPE];
  res->mapped_macs = (int64_t)w[MF_R_MAPPED];
  res->ts_packets = (int64_t)w[MF_R_TS_PACKETS];
  res->pusi_packets = (int64_t)w[MF_R_PUSI];
  res->pad_bytes = (int64_t)w[MF_R_PAD];
  res->flushed = (int64_t)w[MF_R_FLUSHED];
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpefec_run_host(dvbt2ll_mpefec *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                                       int64_t n_pdus, const dvbt2ll_mpefec_pos *start, void *out,
                                       int64_t out_cap_packets, int flush, dvbt2ll_mpefec_result *res) {
  MfRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = mpefec_run_args(h, pdu, pdu_len, off, n_pdus, start, out, out_cap_packets, r);
  if (e || (e = h->s.wait())) return e;
  PduStage &t = h->tmp;
  hipStream_t st = h->s.ctx.stream;
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, mf_packet_limit(h->dev, r.pdu_len, r.n));
  if ((e = t.stage(st, pdu, pdu_len, off, nullptr, n_pdus, (size_t)cap * 188))) return e;
  if ((e = dvbt2ll_mpefec_run_device(h, t.pdu.p, pdu_len, t.off.as<uint32_t>(), n_pdus, start, t.out.p, cap, flush,
                                     st)))
    return e;
  if ((e = dvbt2ll_mpefec_get_result(h, res))) return e;
  return t.fetch(out, res->ts_packets * 188);
}

extern "C" void dvbt2ll_mpefec_destroy(dvbt2ll_mpefec *h) { delete h; }

// ============================================================================ TS multiplexer
// The schedule tables are made at create (tsmux_plan.cpp) and stay on the device; a run is one kernel on the caller's
// stream (tsmux_kernels.hip) whose counters stay on the device until get_result, which adds the resume position: that
// is arithmetic on the start position and the counters.
struct dvbt2ll_tsmux {
  StreamHandle s;
  dvbt2ll_tsmux_params p{};
  TsmuxPlan plan;
  TsmuxDev dev;
  DevBuf table, pre, res, out_tmp;
  DevBuf in_tmp[TSMUX_IN];
  dvbt2ll_tsmux_pos start{};     // of the last run
  int64_t n_in[TSMUX_IN] = {}, n_out = 0;
  // the remux (dvbt2ll_tsmux_set_remux): its tables and scan scratch, the last run's start position
  bool remux = false;
  dvbt2ll_tsmux_remux x{};
  TsremuxDev xdev;
  DevBuf pid_map, slot_of, tiles, chunks, xres;
  dvbt2ll_tsmux_remux_pos rstart{};
  int64_t tpp = 0;               // the mux clock: p.ticks_per_period, or the remux's out_ticks_per_period
  ~dvbt2ll_tsmux() { s.drain(); }
};

extern "C" int dvbt2ll_tsmux_create(const dvbt2ll_tsmux_params *p, int device, dvbt2ll_tsmux **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (!tsmux_params_ok(*p)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_tsmux> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  h->tpp = p->ticks_per_period;
  tsmux_plan(*p, h->plan);
  if ((r = upload(h->table, h->plan.table)) || (r = upload(h->pre, h->plan.pre))) return r;
  if (h->res.ensure(TSMUX_R_WORDS * 8)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemset(h->res.p, 0, TSMUX_R_WORDS * 8));
  TsmuxDev &d = h->dev;
  d.n = p->n_inputs;
  d.owners = h->plan.owners;
  d.fill = p->fill_input;
  d.pcr_pid = p->pcr_pid;
  d.period = (uint32_t)p->period;
  for (int i = 0; i < p->n_inputs; i++) d.loop |= (uint32_t)p->loop[i] << i;
  for (int e = 0; e < TSMUX_OWN; e++) d.w[e] = h->plan.w[e];
  d.tpp = (unsigned long long)p->ticks_per_period;
  d.tpp_q = d.tpp / d.period;
  d.tpp_r = (uint32_t)(d.tpp % d.period);
  d.table = h->table.as<uint8_t>();
  d.pre = h->pre.as<uint32_t>();
  d.res = h->res.as<unsigned long long>();
  *out = h.release();
  return DVBT2LL_OK;
}

static int tsmux_run_args(const dvbt2ll_tsmux *h, const void *const *in, const int64_t *n_in,
                          const dvbt2ll_tsmux_pos *start, void *out, int64_t n_out, TsmuxRun &r) {
  if (!h || !in || !n_in || !start || !out) return DVBT2LL_EINVAL;
  if (n_out < 0 || n_out > h->p.max_out_packets) return DVBT2LL_EINVAL;
  if (start->phase < 0 || start->phase >= h->p.period || start->pcr_ticks < 0 || start->pcr_ticks >= TSMUX_PCR_WRAP)
    return DVBT2LL_EINVAL;
  for (int i = 0; i < h->p.n_inputs; i++) {
    if (n_in[i] < 0 || n_in[i] > 0x7FFFFFFF || (n_in[i] > 0 && !in[i])) return DVBT2LL_EINVAL;
    if (start->next[i] < 0 || start->next[i] > n_in[i]) return DVBT2LL_EINVAL;
    r.in[i] = (const uint8_t *)in[i];
    r.n_in[i] = (uint32_t)n_in[i];
    r.next[i] = (uint32_t)start->next[i];
  }
  const uint32_t *row = &h->plan.pre[(size_t)start->phase * h->plan.owners];
  for (int e = 0; e < h->plan.owners; e++) r.pre0[e] = row[e];
  r.phase = (uint32_t)start->phase;
  r.n_out = (uint32_t)n_out;
  r.pcr_ticks = (unsigned long long)start->pcr_ticks;
  r.out = (uint8_t *)out;
  return DVBT2LL_OK;
}

// rstart: the remux position of a handle with a remux, null on one without (each run call refuses the other kind)
static int tsmux_run(dvbt2ll_tsmux *h, const void *const *in_dev, const int64_t *n_in, const dvbt2ll_tsmux_pos *start,
                     const dvbt2ll_tsmux_remux_pos *rstart, void *out_dev, int64_t n_out, void *stream) {
  TsmuxRun r;
  TsremuxRun y;
  int e = tsmux_run_args(h, in_dev, n_in, start, out_dev, n_out, r);
  if (e) return e;
  if (h->remux != (rstart != nullptr)) return DVBT2LL_EINVAL;
  if (rstart) {
    for (int s = 0; s < DVBT2LL_TSMUX_TRACK; s++) {
      if (rstart->cc[s] < 0 || rstart->cc[s] > (s < h->x.n_track ? 15 : 0)) return DVBT2LL_EINVAL;
      y.cc[s / 16] |= (unsigned long long)rstart->cc[s] << (4 * (s % 16));
    }
    for (int i = 0; i < TSMUX_IN; i++) {
      const int64_t per = h->x.in_period[i], tpp = h->x.in_ticks_per_period[i];
      if (rstart->in_phase[i] < 0 || rstart->in_phase[i] > std::max<int64_t>(per, 1) - 1) return DVBT2LL_EINVAL;
      if (rstart->in_ticks[i] < 0 || rstart->in_ticks[i] >= (per ? TSMUX_PCR_WRAP : 1)) return DVBT2LL_EINVAL;
      // the input's clock stays inside 64 bits: (n_in / in_period + 1) x in_ticks_per_period <= 2^62, without the product
      if (per && n_in[i] / per + 1 > ((int64_t)1 << 62) / tpp) return DVBT2LL_EINVAL;
      y.in_phase[i] = (uint32_t)rstart->in_phase[i];
      y.in_ticks[i] = (unsigned long long)rstart->in_ticks[i];
    }
  }
  hipStream_t st;
  if ((e = h->s.begin(stream, &st))) return e;
  if (rstart) {
    HIP_TRY(tsremux_launch(h->dev, h->xdev, r, y, st));
    h->rstart = *rstart;
  } else HIP_TRY(tsmux_launch(h->dev, r, st));
  if ((e = h->s.end(st))) return e;
  h->start = *start;
  h->n_out = n_out;
  for (int i = 0; i < TSMUX_IN; i++) h->n_in[i] = i < h->p.n_inputs ? n_in[i] : 0;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_tsmux_run_device(dvbt2ll_tsmux *h, const void *const *in_dev, const int64_t *n_in,
                                        const dvbt2ll_tsmux_pos *start, void *out_dev, int64_t n_out, void *stream) {
  return tsmux_run(h, in_dev, n_in, start, nullptr, out_dev, n_out, stream);
}

extern "C" int dvbt2ll_tsmux_run_device_remux(dvbt2ll_tsmux *h, const void *const *in_dev, const int64_t *n_in,
                                              const dvbt2ll_tsmux_pos *start, const dvbt2ll_tsmux_remux_pos *rstart,
                                              void *out_dev, int64_t n_out, void *stream) {
  if (!rstart) return DVBT2LL_EINVAL;
  return tsmux_run(h, in_dev, n_in, start, rstart, out_dev, n_out, stream);
}

extern "C" int dvbt2ll_tsmux_set_remux(dvbt2ll_tsmux *h, const dvbt2ll_tsmux_remux *x) {
  if (!h || !x || h->s.ran || h->remux || !tsmux_remux_ok(h->p, *x)) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->s.ctx.device));
  const int n = h->p.n_inputs;
  std::vector<uint16_t> pid_map((size_t)TSMUX_IN * 8192);
  for (size_t k = 0; k < pid_map.size(); k++) pid_map[k] = (uint16_t)(k & 8191);
  for (int a = 0; a < x->n_map; a++)
    pid_map[(size_t)x->map[a].input * 8192 + x->map[a].from_pid] = (uint16_t)(TSREMUX_ENTRY | x->map[a].to_pid);
  std::vector<uint8_t> slot_of(8192, (uint8_t)TSREMUX_NO_SLOT);
  for (int s = 0; s < x->n_track; s++) slot_of[x->track_pid[s]] = (uint8_t)s;
  int r;
  if ((r = upload(h->pid_map, pid_map)) || (r = upload(h->slot_of, slot_of))) return r;
  const size_t ntiles = ((size_t)h->p.max_out_packets + TSREMUX_TILE - 1) / TSREMUX_TILE;
  const size_t nchunks = (ntiles + TSREMUX_SCAN_TILES - 1) / TSREMUX_SCAN_TILES;
  if (h->tiles.ensure(ntiles * TSREMUX_SLOTS) || h->chunks.ensure(nchunks * TSREMUX_SLOTS) ||
      h->xres.ensure(TSREMUX_R_WORDS * 8))
    return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemset(h->xres.p, 0, TSREMUX_R_WORDS * 8));
  TsremuxDev &d = h->xdev;
  d.pid_map = h->pid_map.as<uint16_t>();
  d.slot_of = h->slot_of.as<uint8_t>();
  d.tiles = h->tiles.as<uint8_t>();
  d.chunks = h->chunks.as<uint8_t>();
  d.res = h->xres.as<unsigned long long>();
  for (int i = 0; i < n; i++) {
    d.restamp_cc |= (uint32_t)x->restamp_cc[i] << i;
    if (!x->in_period[i]) continue;
    d.in_period[i] = (uint32_t)x->in_period[i];
    d.in_tpp[i] = (unsigned long long)x->in_ticks_per_period[i];
    d.in_q[i] = d.in_tpp[i] / d.in_period[i];
    d.in_r[i] = (uint32_t)(d.in_tpp[i] % d.in_period[i]);
  }
  // the slot clock of a handle without a PCR PID, which no kernel of a plain handle reads
  h->tpp = tsmux_remux_tpp(h->p, *x);
  h->dev.tpp = (unsigned long long)h->tpp;
  h->dev.tpp_q = h->dev.tpp / h->dev.period;
  h->dev.tpp_r = (uint32_t)(h->dev.tpp % h->dev.period);
  h->x = *x;
  h->remux = true;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_tsmux_get_remux_result(dvbt2ll_tsmux *h, dvbt2ll_tsmux_remux_result *res) {
  if (!h || !res || !h->remux) return DVBT2LL_EINVAL;
  dvbt2ll_tsmux_result plain;
  int e = dvbt2ll_tsmux_get_result(h, &plain);   // synchronises
  if (e) return e;
  uint64_t w[TSREMUX_R_WORDS];
  HIP_TRY(hipMemcpy(w, h->xdev.res, sizeof w, hipMemcpyDeviceToHost));
  memset(res, 0, sizeof *res);
  res->remapped = (int64_t)w[TSREMUX_R_REMAPPED];
  res->dropped = (int64_t)w[TSREMUX_R_DROPPED];
  res->cc_rewritten = (int64_t)w[TSREMUX_R_CC_REWRITTEN];
  res->pcr_restamped = (int64_t)w[TSREMUX_R_PCR];
  for (int s = 0; s < h->x.n_track; s++) res->resume.cc[s] = (int)((h->rstart.cc[s] + w[TSREMUX_R_CC + s]) & 15);
  for (int i = 0; i < h->p.n_inputs; i++) {
    const int64_t per = h->x.in_period[i];
    if (!per) continue;
    const int64_t at = h->rstart.in_phase[i] + plain.consumed[i];
    res->resume.in_phase[i] = (int)(at % per);
    // at most 2^31 periods of less than 2^36 ticks, checked against 2^62 at the run
    res->resume.in_ticks[i] = (h->rstart.in_ticks[i] + (at / per) * h->x.in_ticks_per_period[i]) % TSMUX_PCR_WRAP;
  }
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_tsmux_get_result(dvbt2ll_tsmux *h, dvbt2ll_tsmux_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  uint64_t w[TSMUX_R_WORDS];
  int e = h->s.read(h->dev.res, w);
  if (e) return e;
  memset(res, 0, sizeof *res);
  for (int i = 0; i < TSMUX_IN; i++) {
    res->consumed[i] = (int64_t)w[TSMUX_R_CONSUMED + i];
    res->dry_slots[i] = (int64_t)w[TSMUX_R_DRY + i];
    const int64_t nx = h->start.next[i] + res->consumed[i];
    res->resume.next[i] = i < h->p.n_inputs && h->p.loop[i] ? (h->n_in[i] ? nx % h->n_in[i] : 0) : nx;
  }
  res->fill_in_free = (int64_t)w[TSMUX_R_FILL_IN_FREE];
  res->pcr_packets = (int64_t)w[TSMUX_R_PCR];
  res->null_packets = (int64_t)w[TSMUX_R_NULL];
  res->sync_errors = (int64_t)w[TSMUX_R_SYNC];
  const int64_t at = h->start.phase + h->n_out;
  res->resume.phase = (int)(at % h->p.period);
  // the periods passed are at most 2^24 + 1 and ticks_per_period is below 2^36
  res->resume.pcr_ticks = (h->start.pcr_ticks + (at / h->p.period) * h->tpp) % TSMUX_PCR_WRAP;
  return DVBT2LL_OK;
}

static int tsmux_run_host(dvbt2ll_tsmux *h, const void *const *in, const int64_t *n_in, const dvbt2ll_tsmux_pos *start,
                          const dvbt2ll_tsmux_remux_pos *rstart, void *out, int64_t n_out, dvbt2ll_tsmux_result *res,
                          dvbt2ll_tsmux_remux_result *rres) {
  TsmuxRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = tsmux_run_args(h, in, n_in, start, out, n_out, r);
  if (e) return e;
  if (h->remux != (rstart != nullptr)) return DVBT2LL_EINVAL;
  if ((e = h->s.wait())) return e;
  hipStream_t st = h->s.ctx.stream;
  const void *dev_in[TSMUX_IN] = {};
  for (int i = 0; i < h->p.n_inputs; i++) {
    if (!n_in[i]) continue;
    if (h->in_tmp[i].ensure((size_t)n_in[i] * 188)) return DVBT2LL_ENOMEM;
    HIP_TRY(hipMemcpyAsync(h->in_tmp[i].p, in[i], (size_t)n_in[i] * 188, hipMemcpyHostToDevice, st));
    dev_in[i] = h->in_tmp[i].p;
  }
  if (h->out_tmp.ensure((size_t)std::max<int64_t>(n_out, 1) * 188)) return DVBT2LL_ENOMEM;
  if ((e = tsmux_run(h, dev_in, n_in, start, rstart, h->out_tmp.p, n_out, st))) return e;
  if ((e = dvbt2ll_tsmux_get_result(h, res))) return e;
  if (rstart && (e = dvbt2ll_tsmux_get_remux_result(h, rres))) return e;
  if (n_out > 0) HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)n_out * 188, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_tsmux_run_host(dvbt2ll_tsmux *h, const void *const *in, const int64_t *n_in,
                                      const dvbt2ll_tsmux_pos *start, void *out, int64_t n_out,
                                      dvbt2ll_tsmux_result *res) {
  return tsmux_run_host(h, in, n_in, start, nullptr, out, n_out, res, nullptr);
}

extern "C" int dvbt2ll_tsmux_run_host_remux(dvbt2ll_tsmux *h, const void *const *in, const int64_t *n_in,
                                            const dvbt2ll_tsmux_pos *start, const dvbt2ll_tsmux_remux_pos *rstart,
                                            void *out, int64_t n_out, dvbt2ll_tsmux_result *res,
                                            dvbt2ll_tsmux_remux_result *rres) {
  if (!rstart || !rres) return DVBT2LL_EINVAL;
  return tsmux_run_host(h, in, n_in, start, rstart, out, n_out, res, rres);
}

extern "C" void dvbt2ll_tsmux_destroy(dvbt2ll_tsmux *h) { delete h; }

// ============================================================================ GSE encapsulator
// Scratch sized at create from max_pdus and Kbch; the passes are in gse_kernels.hip.
struct dvbt2ll_gse {
  StreamHandle s;
  dvbt2ll_gse_params p{};
  GseDev dev;
  DevBuf scratch;
  PduStage tmp;
  ~dvbt2ll_gse() { s.drain(); }
};

// the resolved Kbch of the parameters, or 0 when they are refused
static int gse_params_kbch(const dvbt2ll_gse_params &p) {
  const int kbch = p.kbch ? p.kbch : modeadapt_kbch_of(p.framesize, p.rate);
  // 58192 (D = 7264) is the DVB family's largest Kbch; no T2 code has it, the chain takes no such frame.  It is
  // accepted so that the position tables are pinned at the largest state count the entry format is sized for
  if (kbch != 3072 && kbch != 58192 && (kbch <= 0 || kbch % 8 || !t2mi_valid_len(kbch / 8))) return 0;
  if ((p.sis_mis != 0 && p.sis_mis != 1) || p.isi < 0 || p.isi > 255) return 0;
  if (p.label_len != 0 && p.label_len != 3 && p.label_len != 6) return 0;
  if (p.max_pdu_bytes < 1 || p.max_pdu_bytes >= ((int64_t)1 << 31)) return 0;
  if (p.max_pdus < 1 || p.max_pdus > (1 << 24)) return 0;   // 2^24 PDUs of 13 frames: below 2^32 frames
  return kbch;
}

extern "C" int dvbt2ll_gse_create(const dvbt2ll_gse_params *p, int device, dvbt2ll_gse **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  const int kbch = gse_params_kbch(*p);
  if (!kbch) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_gse> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  h->p.kbch = kbch;
  GseDev &d = h->dev;
  d.Lb = (uint32_t)kbch / 8;
  d.D = d.Lb - 10;
  d.L = (uint32_t)p->label_len;
  d.lt = d.L == 6 ? 0 : d.L == 3 ? 1 : 2;
  memcpy(d.label, p->label, 6);
  // MATYPE-1: TS_GS 10, SIS/MIS, CCM 1, ISSYI 0, NPD 0, EXT 00
  d.matype = p->sis_mis ? 0xB000u : 0x9000u | (uint32_t)p->isi;
  d.max_pdus = (uint32_t)p->max_pdus;
  if ((r = lay_out(h->scratch, d, gse_layout))) return r;
  std::vector<uint32_t> tab(GSE_TAB_WORDS);
  gse_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (GSE_R_WORDS + 2) * 8));
  *out = h.release();
  return DVBT2LL_OK;
}

static int gse_run_args(const dvbt2ll_gse *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                        const uint16_t *type, int64_t n_pdus, const dvbt2ll_gse_pos *start, void *out, int64_t cap,
                        GseRun &r) {
  int e = pdu_run_args(h, pdu, pdu_len, off, n_pdus, start, out, cap, r);
  if (e) return e;
  if (start->pdu_byte < 0 || start->frag_id < 0 || start->frag_id > 255) return DVBT2LL_EINVAL;
  r.type = type;
  r.pdu_byte = (uint32_t)start->pdu_byte;
  r.frag_id = (uint32_t)start->frag_id;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_gse_run_device(dvbt2ll_gse *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                                      const uint16_t *type_dev, int64_t n_pdus, const dvbt2ll_gse_pos *start,
                                      void *out_dev, int64_t out_cap_blocks, int flush, void *stream) {
  GseRun r;
  hipStream_t st;
  int e = gse_run_args(h, pdu_dev, pdu_len, off_dev, type_dev, n_pdus, start, out_dev, out_cap_blocks, r);
  if (e || (e = h->s.begin(stream, &st))) return e;
  r.flush = flush != 0;
  HIP_TRY(gse_launch(h->dev, r, st));
  return h->s.end(st);
}

extern "C" int dvbt2ll_gse_get_result(dvbt2ll_gse *h, dvbt2ll_gse_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  uint64_t w[GSE_R_WORDS];
  int e = h->s.read(h->dev.res, w);
  if (e) return e;
  memset(res, 0, sizeof *res);
  res->resume.pdu = (int64_t)w[GSE_R_PDU];
  res->resume.pdu_byte = (int)w[GSE_R_PDU_BYTE];
  res->resume.frag_id = (int)w[GSE_R_FRAG_ID];
  int64_t *c = &res->pdus_in;
  for (int k = 0; k < 9; k++) c[k] = (int64_t)w[GSE_R_PDUS_IN + k];
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_gse_run_host(dvbt2ll_gse *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                                    const uint16_t *type, int64_t n_pdus, const dvbt2ll_gse_pos *start, void *out,
                                    int64_t out_cap_blocks, int flush, dvbt2ll_gse_result *res) {
  GseRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = gse_run_args(h, pdu, pdu_len, off, type, n_pdus, start, out, out_cap_blocks, r);
  if (e || (e = h->s.wait())) return e;
  PduStage &t = h->tmp;
  hipStream_t st = h->s.ctx.stream;
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, gse_frame_limit(h->dev, r.pdu_len, r.n));
  if ((e = t.stage(st, pdu, pdu_len, off, type, n_pdus, (size_t)cap * h->dev.Lb))) return e;
  if ((e = dvbt2ll_gse_run_device(h, t.pdu.p, pdu_len, t.off.as<uint32_t>(), t.types(type), n_pdus, start, t.out.p,
                                  cap, flush, st)))
    return e;
  if ((e = dvbt2ll_gse_get_result(h, res))) return e;
  return t.fetch(out, res->bbframes * h->dev.Lb);
}

extern "C" void dvbt2ll_gse_destroy(dvbt2ll_gse *h) { delete h; }

// ============================================================================ T2-MI output
// Every packet length is a constant of the handle and every call starts on a TS packet boundary, so the positions of a
// call's packets are walked once at create (t2mo_host_walk) and a call's counters are arithmetic on the host:
// run_device launches the CRC and emit passes on the caller's stream (t2mi_out_kernels.hip) and keeps the result for
// get_result.
struct dvbt2ll_t2mi_out {
  StreamHandle s;
  dvbt2ll_t2mi_out_params p{};
  T2moDev dev;
  T2moFrames frames;
  std::vector<T2moPkt> pkt;        // P + 1
  uint32_t aux_bytes[DVBT2LL_T2MI_OUT_MAX_AUX] = {};
  dvbt2ll_t2mi_out_result res{};   // the last run's
  DevBuf scratch, bb_tmp[DVBT2LL_MAX_PLP], aux_tmp, out_tmp;
  ~dvbt2ll_t2mi_out() { s.drain(); }
};

// the packets of one T2 frame, or nothing when the parameters are refused
static std::vector<T2moPkt> t2mo_frame_packets(const dvbt2ll_t2mi_out_params &p) {
  std::vector<T2moPkt> out;
  if (p.pid < 0 || p.pid > 0x1FFE || p.t2mi_stream_id < 0 || p.t2mi_stream_id > 7) return out;
  if (p.nplp < 1 || p.nplp > DVBT2LL_MAX_PLP || p.naux < 0 || p.naux > DVBT2LL_T2MI_OUT_MAX_AUX) return out;
  if (p.frames_per_superframe < 1 || p.frames_per_superframe > 256 || p.max_frames < 1) return out;
  for (int k = 0; k < p.nplp; k++) {
    if (p.plp_id[k] < 0 || p.plp_id[k] > 255 || !t2mi_valid_len(p.bbframe_bytes[k])) return out;
    if (p.blocks_per_frame[k] < 1 || p.blocks_per_frame[k] > 1023) return out;
    for (int j = 0; j < k; j++)
      if (p.plp_id[j] == p.plp_id[k]) return out;
  }
  for (int a = 0; a < p.naux; a++) {
    const dvbt2ll_t2mi_out_slot &s = p.aux[a];
    if (s.packet_type < 0 || s.packet_type > 255 || s.payload_bits < 1 || s.payload_bits > 65535) return out;
    if (s.after != 0 && s.after != 1) return out;
  }
  uint64_t off = 0;
  auto add_aux = [&](int after) {
    for (int a = 0; a < p.naux; a++) {
      if (p.aux[a].after != after) continue;
      const uint32_t bits = (uint32_t)p.aux[a].payload_bits;
      out.push_back({(uint32_t)off, 10 + (bits + 7) / 8, 0, (uint16_t)bits, (uint8_t)p.aux[a].packet_type, (uint8_t)(8 + a)});
      off += out.back().T;
    }
  };
  add_aux(0);
  for (int k = 0; k < p.nplp; k++)
    for (int b = 0; b < p.blocks_per_frame[k]; b++) {
      const uint32_t L = (uint32_t)p.bbframe_bytes[k];
      out.push_back({(uint32_t)off, 13 + L, (uint32_t)b, (uint16_t)(24 + 8 * L), 0, (uint8_t)k});
      off += out.back().T;
    }
  add_aux(1);
  if (off * (uint64_t)p.max_frames >= ((uint64_t)1 << 31) - ((uint64_t)1 << 24)) return {};
  out.push_back({(uint32_t)off, 0, 0, 0, 0, 0});   // the frame's end
  return out;
}

extern "C" int dvbt2ll_t2mi_out_create(const dvbt2ll_t2mi_out_params *p, int device, dvbt2ll_t2mi_out **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  std::vector<T2moPkt> pkt = t2mo_frame_packets(*p);
  if (pkt.empty()) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_t2mi_out> h;
  int r = new_handle(device, h);
  if (r) return r;
  h->p = *p;
  T2moDev &d = h->dev;
  d.pid = p->pid;
  d.stream_id = p->t2mi_stream_id;
  d.nplp = p->nplp;
  d.fps = p->frames_per_superframe;
  for (int k = 0; k < p->nplp; k++) {
    d.plp_id[k] = p->plp_id[k];
    d.Lb[k] = (uint32_t)p->bbframe_bytes[k];
    d.F[k] = (uint32_t)p->blocks_per_frame[k];
  }
  for (int a = 0; a < p->naux; a++) h->aux_bytes[a] = ((uint32_t)p->aux[a].payload_bits + 7) / 8;
  d.P = (uint32_t)pkt.size() - 1;
  d.B = pkt.back().off;
  d.max_frames = (uint32_t)p->max_frames;
  std::vector<uint32_t> tq;
  std::vector<uint8_t> td;
  t2mo_host_walk(d, pkt.data(), tq, td, h->frames);
  if ((r = lay_out(h->scratch, d, t2mo_layout))) return r;
  std::vector<uint32_t> tab(T2MO_TAB_WORDS);
  t2mo_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.pkt, pkt.data(), pkt.size() * sizeof(T2moPkt), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.tq, tq.data(), tq.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.td, td.data(), td.size(), hipMemcpyHostToDevice));
  h->pkt = std::move(pkt);
  *out = h.release();
  return DVBT2LL_OK;
}

extern "C" int64_t dvbt2ll_t2mi_out_ts_packets(const dvbt2ll_t2mi_out *h, int nframes) {
  if (!h || nframes < 0 || nframes > h->p.max_frames) return DVBT2LL_EINVAL;
  return (int64_t)h->frames.ts_packets((uint32_t)nframes);
}

static int t2mo_run_args(const dvbt2ll_t2mi_out *h, const void *const *bb, const void *aux, int64_t aux_stride,
                         const int64_t *aux_off, const dvbt2ll_t2mi_out_pos *start, int nframes, void *out,
                         int64_t cap, T2moRun &r) {
  if (!h || !bb || !start || !out) return DVBT2LL_EINVAL;
  if (nframes < 0 || nframes > h->p.max_frames) return DVBT2LL_EINVAL;
  if (start->frame < 0 || start->packet_count < 0 || start->packet_count > 255 || start->cc < 0 || start->cc > 15)
    return DVBT2LL_EINVAL;
  for (int k = 0; k < h->p.nplp; k++)
    if (!bb[k]) return DVBT2LL_EINVAL;
  if (h->p.naux) {
    if (!aux || !aux_off || aux_stride < 0) return DVBT2LL_EINVAL;
    for (int a = 0; a < h->p.naux; a++)
      if (aux_off[a] < 0 || aux_off[a] > 0x7FFFFFFF) return DVBT2LL_EINVAL;
  }
  const uint32_t n = (uint32_t)nframes;
  r.N = h->frames.ts_packets(n);
  if (cap < (int64_t)r.N) return DVBT2LL_EINVAL;
  for (int k = 0; k < h->p.nplp; k++) r.bb[k] = (const uint8_t *)bb[k];
  r.aux = (const uint8_t *)aux;
  r.aux_stride = h->p.naux ? (size_t)aux_stride : 0;
  for (int a = 0; a < h->p.naux; a++) r.aux_off[a] = (uint32_t)aux_off[a];
  const int64_t fps = h->p.frames_per_superframe;
  r.fi0 = (uint32_t)(start->frame % fps);
  r.sf0 = (uint32_t)((start->frame / fps) & 15);
  r.count0 = (uint32_t)start->packet_count;
  r.cc0 = (uint32_t)start->cc;
  r.nframes = n;
  r.G = n * h->dev.P;
  r.E = n * h->dev.B;
  r.out = (uint8_t *)out;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_out_run_device(dvbt2ll_t2mi_out *h, const void *const *bb_dev, const void *aux_dev,
                                           int64_t aux_stride, const int64_t *aux_off,
                                           const dvbt2ll_t2mi_out_pos *start, int nframes, void *out_dev,
                                           int64_t out_cap_packets, void *stream) {
  T2moRun r;
  hipStream_t st;
  int e = t2mo_run_args(h, bb_dev, aux_dev, aux_stride, aux_off, start, nframes, out_dev, out_cap_packets, r);
  if (e || (e = h->s.begin(stream, &st))) return e;
  HIP_TRY(t2mo_launch(h->dev, r, st));
  if ((e = h->s.end(st))) return e;
  // the result is arithmetic on the handle's constants
  dvbt2ll_t2mi_out_result &res = h->res;
  memset(&res, 0, sizeof res);
  res.next.frame = start->frame + nframes;
  res.next.packet_count = (int)((r.count0 + r.G) & 255);
  res.next.cc = (int)((r.cc0 + r.N) & 15);
  res.frames = nframes;
  res.t2mi_packets = r.G;
  res.ts_packets = r.N;
  res.pusi_packets = h->frames.pusi[r.nframes];
  res.stuffing_bytes = (int64_t)r.N * 184 - (int64_t)r.E - res.pusi_packets;
  for (uint32_t j = 0; j < h->dev.P; j++) res.by_type[h->pkt[j].type] += nframes;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_out_get_result(dvbt2ll_t2mi_out *h, dvbt2ll_t2mi_out_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  int e = h->s.wait();
  if (e) return e;
  *res = h->res;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_out_run_host(dvbt2ll_t2mi_out *h, const void *const *bb, const void *aux,
                                         int64_t aux_stride, const int64_t *aux_off, const dvbt2ll_t2mi_out_pos *start,
                                         int nframes, void *out, int64_t out_cap_packets, dvbt2ll_t2mi_out_result *res) {
  T2moRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = t2mo_run_args(h, bb, aux, aux_stride, aux_off, start, nframes, out, out_cap_packets, r);
  if (e || (e = h->s.wait())) return e;
  hipStream_t st = h->s.ctx.stream;
  const void *bd[DVBT2LL_MAX_PLP] = {};
  for (int k = 0; k < h->p.nplp; k++) {
    const size_t bytes = (size_t)nframes * h->dev.F[k] * h->dev.Lb[k];
    if (h->bb_tmp[k].ensure(std::max<size_t>(bytes, 1))) return DVBT2LL_ENOMEM;
    if (bytes) HIP_TRY(hipMemcpyAsync(h->bb_tmp[k].p, bb[k], bytes, hipMemcpyHostToDevice, st));
    bd[k] = h->bb_tmp[k].p;
  }
  size_t aux_len = 0;   // up to the end of the last frame's last payload
  if (nframes)
    for (int a = 0; a < h->p.naux; a++)
      aux_len = std::max(aux_len, (size_t)(nframes - 1) * r.aux_stride + r.aux_off[a] + h->aux_bytes[a]);
  if (h->aux_tmp.ensure(std::max<size_t>(aux_len, 1))) return DVBT2LL_ENOMEM;
  if (aux_len) HIP_TRY(hipMemcpyAsync(h->aux_tmp.p, aux, aux_len, hipMemcpyHostToDevice, st));
  if (h->out_tmp.ensure(std::max<size_t>((size_t)r.N * 188, 1))) return DVBT2LL_ENOMEM;
  if ((e = dvbt2ll_t2mi_out_run_device(h, bd, h->aux_tmp.p, aux_stride, aux_off, start, nframes, h->out_tmp.p, r.N,
                                       st)))
    return e;
  if ((e = dvbt2ll_t2mi_out_get_result(h, res))) return e;
  if (r.N) HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)r.N * 188, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_t2mi_out_destroy(dvbt2ll_t2mi_out *h) { delete h; }
