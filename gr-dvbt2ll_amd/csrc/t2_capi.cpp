// t2_capi.cpp -- C ABI (include/dvbt2ll_hip.h): handles, device tables, launches.
//
// Each handle mirrors one reference gr::block: the constructor work happens in
// *_create (host planning in t2_plan.cpp + one upload of the device tables), and
// *_general_work runs the block's kernels synchronously on the handle's HIP stream
// with the caller's host buffers (GNU Radio's circular buffers).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/dvbt2ll_hip.h"
#include "t2_kernels.h"
#include "t2_plan.h"
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

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e_ = (expr);                             \
    if (e_ != hipSuccess) {                             \
      last_hip_error() = e_;                            \
      return e_ == hipErrorOutOfMemory ? DVBT2LL_ENOMEM : DVBT2LL_EDEVICE; \
    }                                                   \
  } while (0)

hipError_t &last_hip_error() {
  static thread_local hipError_t e = hipSuccess;
  return e;
}

// device buffer with grow-on-demand
struct DevBuf {
  void *p = nullptr;
  size_t n = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  int ensure(size_t bytes) {
    if (bytes <= n) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    if (hipMalloc(&p, bytes) != hipSuccess) return DVBT2LL_ENOMEM;
    n = bytes;
    return 0;
  }
  template <class T> T *as() const { return (T *)p; }
};

template <class T>
int upload(DevBuf &b, const std::vector<T> &v) {
  if (v.empty()) return 0;
  if (b.ensure(v.size() * sizeof(T))) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}
int upload_raw(DevBuf &b, const void *src, size_t bytes) {
  if (b.ensure(bytes)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

struct DeviceCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  int init(int dev) {
    device = dev;
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return 0;
  }
  ~DeviceCtx() {
    if (stream) { (void)hipSetDevice(device); (void)hipStreamDestroy(stream); }
  }
};

// ---------------------------------------------------------------- FEC tables on device
struct FecTables {
  FecPlan plan;
  DevBuf hcrc, tab, ctab, rowptr, ent, prbs, crc8, crcsh, bmf;
  FecDev dev{};
  // the fused chain's BCH pass on the matrix cores: the generator matrix as fp4 B fragments
  int init_chain() {
    if (build_bch_mfma(plan)) return DVBT2LL_EINVAL;
    int r = upload(bmf, plan.bch_mfma);
    if (r) return r;
    dev.bch_mfma = bmf.as<uint4>();
    dev.bch_nq = plan.bch_nq;
    dev.bch_nt = plan.bch_nt;
    return 0;
  }
  int init(int framesize, int rate, int constellation, int mode, int inband, int fecblocks, int tsrate) {
    if (build_fec(framesize, rate, constellation, plan)) return DVBT2LL_EINVAL;
    int r;
    if ((r = upload(tab, plan.bch_tab)) || (r = upload(ctab, plan.bch_ctab)) ||
        (r = upload(rowptr, plan.ldpc_rowptr)) || (r = upload(ent, plan.ldpc_ent)) ||
        (r = upload(prbs, plan.prbs_bytes)) || (r = upload(crc8, plan.crc8_tab)) || (r = upload(crcsh, plan.crc8_shift)) ||
        (r = upload(hcrc, plan.hcrc_bits)))
      return r;
    dev.bch_tab = tab.as<uint64_t>();
    dev.bch_ctab = ctab.as<uint64_t>();
    dev.ldpc_rowptr = rowptr.as<uint16_t>();
    dev.ldpc_ent = ent.as<uint32_t>();
    dev.prbs = prbs.as<uint8_t>();
    dev.crc8_tab = crc8.as<uint8_t>();
    dev.crc8_shift = crcsh.as<uint8_t>();
    dev.hcrc_bits = hcrc.as<uint8_t>();
    dev.kbch = plan.kbch; dev.nbch = plan.nbch; dev.P = plan.nparity; dev.nldpc = plan.nldpc;
    dev.q = plan.q; dev.nent = (int)plan.ldpc_ent.size(); dev.chunk = plan.bch_chunk;
    dev.parity_il = plan.parity_interleave ? 1 : 0;
    dev.hem = mode ? 1 : 0;
    dev.inband = inband ? 1 : 0;
    dev.fec_blocks = fecblocks > 0 ? fecblocks : 1;
    dev.ts_rate = tsrate;
    dev.matype = MATYPE_SIS;
    return 0;
  }
};

struct MapTables {
  MapPlan plan;
  DevBuf lut, colbuf;
  MapDev dev{};
  int init(int framesize, int rate, int constellation, int rotation, const FecPlan &fec) {
    if (build_map(framesize, rate, constellation, rotation, plan)) return DVBT2LL_EINVAL;
    int r = upload_raw(lut, plan.lut, sizeof(plan.lut));
    if (r) return r;
    dev.lut = lut.as<float2>();
    dev.mode = plan.mode; dev.mod = plan.mod; dev.W = plan.W; dev.R = plan.R; dev.cs = plan.cs;
    dev.nldpc = plan.nldpc; dev.nbch = fec.nbch; dev.q = fec.q; dev.rotation = plan.rotation;
    dev.parity_il = fec.parity_interleave ? 1 : 0;
    dev.F = 1;
    // column feeding bit b of the demuxed row word (b = W - 1 - mux[e]): its start bit and twist
    std::vector<int2> col(16, int2{-1, 0});
    for (int e = 0; e < plan.W && plan.mode != 0; e++) col[plan.W - 1 - plan.mux[e]] = int2{e * plan.R, plan.twist[e]};
    if ((r = upload(colbuf, col))) return r;
    dev.col = colbuf.as<int2>();
    return 0;
  }
};

// ---------------------------------------------------------------- L1-post tables on device
struct L1Tables {
  DevBuf tmpl, crc_c, scr, sig_pos, bch_r, ldpc_ptr, ldpc_addr, sel, lut;
  L1Dev dev{};
  int init(const FramePlan &fp) {
    const L1PostPlan &l = fp.l1;
    int r;
    if ((r = upload(tmpl, l.tmpl)) || (r = upload(crc_c, l.crc_c)) || (r = upload(scr, l.scr)) ||
        (r = upload(sig_pos, l.sig_pos)) || (r = upload(bch_r, l.bch_r)) || (r = upload(ldpc_ptr, l.ldpc_ptr)) ||
        (r = upload(ldpc_addr, l.ldpc_addr)) || (r = upload(sel, l.sel)) || (r = upload_raw(lut, l.lut, sizeof(l.lut))))
      return r;
    dev.tmpl = tmpl.as<uint32_t>();
    dev.crc_c = crc_c.as<uint32_t>();
    dev.scr = l.scr.empty() ? nullptr : scr.as<uint32_t>();
    dev.sig_pos = sig_pos.as<uint16_t>();
    dev.bch_r = bch_r.as<uint32_t>();
    dev.ldpc_ptr = ldpc_ptr.as<uint16_t>();
    dev.ldpc_addr = ldpc_addr.as<uint16_t>();
    dev.sel = sel.as<uint16_t>();
    dev.lut = lut.as<float2>();
    dev.crc_k = l.crc_k;
    dev.nsig = l.nsig; dev.fidx_pos = l.fidx_pos; dev.npost = l.npost; dev.lp = l.lp; dev.mode = l.mode;
    dev.ncols = l.ncols; dev.rows = l.rows; dev.q = l.q; dev.pbits = l.pbits; dev.t2frames = fp.t2frames;
    dev.ncls = l.ncls;
    memcpy(dev.mux, l.mux, sizeof(dev.mux));
    return 0;
  }
};

}  // namespace

// ============================================================================ common
extern "C" const char *dvbt2ll_strerror(int status) {
  switch (status) {
    case DVBT2LL_OK: return "ok";
    case DVBT2LL_EINVAL: return "invalid parameter combination";
    case DVBT2LL_ENOMEM: return "out of memory";
    case DVBT2LL_EDEVICE: return hipGetErrorString(last_hip_error());
    case DVBT2LL_ESHORT: return "not enough input items";
    default: return "unknown status";
  }
}
extern "C" const char *dvbt2ll_version(void) { return "dvbt2ll-mi355x 0.1 (gfx950)"; }
extern "C" int dvbt2ll_abi_version(void) { return DVBT2LL_ABI_VERSION; }
extern "C" int dvbt2ll_abi_check(int abi_version, size_t sizeof_chain_params, size_t sizeof_chain_info,
                                 size_t sizeof_plp_params, size_t sizeof_mplp_params, size_t sizeof_mplp_chain_params) {
  return abi_version == DVBT2LL_ABI_VERSION && sizeof_chain_params == sizeof(dvbt2ll_chain_params) &&
                 sizeof_chain_info == sizeof(dvbt2ll_chain_info) && sizeof_plp_params == sizeof(dvbt2ll_plp_params) &&
                 sizeof_mplp_params == sizeof(dvbt2ll_mplp_params) &&
                 sizeof_mplp_chain_params == sizeof(dvbt2ll_mplp_chain_params)
             ? DVBT2LL_OK
             : DVBT2LL_EINVAL;
}
extern "C" int dvbt2ll_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// ============================================================================ bbheaderbch
struct dvbt2ll_bbheaderbch {
  DeviceCtx ctx;
  FecTables fec;
  dvbt2ll_bbheaderbch_params p{};
  int64_t blocks_done = 0;       // fec_block state = blocks_done % fecblocks
  int64_t consumed_total = 0;    // absolute TS offset of the next input byte
  std::vector<uint8_t> history;  // last <= 376 consumed TS bytes (previous packet for CRC-8)
  DevBuf din, dout;
  std::vector<uint8_t> hbuf;
  DevBuf sync_err;               // device counter: TS sync bytes != 0x47 consumed so far
  uint32_t sync_err_host = 0;
};

extern "C" int dvbt2ll_bbheaderbch_create(const dvbt2ll_bbheaderbch_params *p, int device, dvbt2ll_bbheaderbch **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  std::unique_ptr<dvbt2ll_bbheaderbch> h(new (std::nothrow) dvbt2ll_bbheaderbch());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  if (p->inband && p->fecblocks < 1) return DVBT2LL_EINVAL;
  int r = h->ctx.init(device);
  if (r) return r;
  if ((r = h->fec.init(p->framesize, p->rate, 3, p->mode, p->inband, p->fecblocks, p->tsrate))) return r;
  if (h->sync_err.ensure(4)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemset(h->sync_err.p, 0, 4));
  *out = h.release();
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_bbheaderbch_output_multiple(const dvbt2ll_bbheaderbch *h) { return h ? h->fec.plan.nbch : 0; }
extern "C" int dvbt2ll_bbheaderbch_forecast(const dvbt2ll_bbheaderbch *h, int nout, int *nin) {
  if (!h || !nin) return DVBT2LL_EINVAL;
  const FecPlan &f = h->fec.plan;
  int n = (nout - 80 - (f.nbch - f.kbch)) / 8;       // bbheader:207-216
  if (h->p.mode) n += (((f.kbch - 80) / 8) / 187) + 1;
  *nin = n;
  return DVBT2LL_OK;
}

// input bytes consumed by nblocks FEC blocks starting at absolute block b0 / stream offset
static int64_t bb_consumed(const FecDev &d, int64_t b0, int64_t nblocks) {
  auto J = [&](int64_t B) {
    int64_t pay = (d.kbch - 80) / 8;
    int64_t npad = d.inband ? (B + d.fec_blocks - 1) / d.fec_blocks : 0;
    return B * pay - 13 * npad;
  };
  auto pos_after = [&](int64_t B) -> int64_t {   // stream offset after block B-1
    int64_t j = J(B);
    if (!d.hem || j == 0) return j;
    int64_t last = j - 1;
    return 188 * (last / 187) + 1 + (last % 187) + 1;
  };
  return pos_after(b0 + nblocks) - pos_after(b0);
}

extern "C" int dvbt2ll_bbheaderbch_general_work(dvbt2ll_bbheaderbch *h, int nout, int nin, const void *in, void *out,
                                                int *consumed) {
  if (!h || nout < 0 || (nout && (!in || !out))) return DVBT2LL_EINVAL;
  const FecDev &d = h->fec.dev;
  int nb = nout / d.nbch;
  if (consumed) *consumed = 0;
  if (nb == 0) return 0;
  int64_t need = bb_consumed(d, h->blocks_done, nb);
  if (need > nin) return DVBT2LL_ESHORT;
  // device buffer: [history | new input]; ts_base = absolute offset of history start
  int64_t hist = (int64_t)h->history.size();
  h->hbuf.resize(hist + need);
  if (hist) memcpy(h->hbuf.data(), h->history.data(), hist);
  memcpy(h->hbuf.data() + hist, in, need);
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->din.ensure(h->hbuf.size() + 16) || h->dout.ensure((size_t)nb * d.nbch)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpyAsync(h->din.p, h->hbuf.data(), h->hbuf.size(), hipMemcpyHostToDevice, h->ctx.stream));
  FecIO io{};
  io.in = h->din.as<uint8_t>();
  io.ts_base = h->consumed_total - hist;
  io.ts_len = (int64_t)h->hbuf.size();
  io.first_block = h->blocks_done;
  io.out = h->dout.as<uint8_t>();
  io.nblocks = nb;
  io.sync_err = h->sync_err.as<uint32_t>();
  HIP_TRY(launch_fec(FEC_TS_TO_BITS, d, io, h->ctx.stream));
  HIP_TRY(hipMemcpyAsync(out, h->dout.p, (size_t)nb * d.nbch, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipMemcpyAsync(&h->sync_err_host, h->sync_err.p, 4, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  h->blocks_done += nb;
  h->consumed_total += need;
  size_t keep = std::min<size_t>(376, h->hbuf.size());
  h->history.assign(h->hbuf.end() - keep, h->hbuf.end());
  if (consumed) *consumed = (int)need;
  return nb * d.nbch;
}
extern "C" int64_t dvbt2ll_bbheaderbch_sync_errors(const dvbt2ll_bbheaderbch *h) {
  return h ? (int64_t)h->sync_err_host : 0;
}
extern "C" int dvbt2ll_bbheaderbch_set_isi(dvbt2ll_bbheaderbch *h, int isi) {
  if (!h || isi < 0 || isi > 255) return DVBT2LL_EINVAL;
  h->fec.dev.matype = MATYPE_MIS | isi;   // bbheader:288-298
  return DVBT2LL_OK;
}
extern "C" void dvbt2ll_bbheaderbch_destroy(dvbt2ll_bbheaderbch *h) { delete h; }

// ============================================================================ ldpc
struct dvbt2ll_ldpc {
  DeviceCtx ctx;
  FecTables fec;
  DevBuf din, dout;
};
extern "C" int dvbt2ll_ldpc_create(const dvbt2ll_ldpc_params *p, int device, dvbt2ll_ldpc **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  std::unique_ptr<dvbt2ll_ldpc> h(new (std::nothrow) dvbt2ll_ldpc());
  if (!h) return DVBT2LL_ENOMEM;
  int r = h->ctx.init(device);
  if (r) return r;
  if ((r = h->fec.init(p->framesize, p->rate, 3, 0, 0, 1, 0))) return r;
  *out = h.release();
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_ldpc_output_multiple(const dvbt2ll_ldpc *h) { return h ? h->fec.plan.nldpc : 0; }
extern "C" int dvbt2ll_ldpc_forecast(const dvbt2ll_ldpc *h, int nout, int *nin) {
  if (!h || !nin) return DVBT2LL_EINVAL;
  *nin = (nout / h->fec.plan.nldpc) * h->fec.plan.nbch;
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_ldpc_general_work(dvbt2ll_ldpc *h, int nout, int nin, const void *in, void *out, int *consumed) {
  if (!h || nout < 0 || (nout && (!in || !out))) return DVBT2LL_EINVAL;
  const FecDev &d = h->fec.dev;
  int nb = nout / d.nldpc;
  if (consumed) *consumed = 0;
  if (nb == 0) return 0;
  if ((int64_t)nb * d.nbch > nin) return DVBT2LL_ESHORT;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->din.ensure((size_t)nb * d.nbch) || h->dout.ensure((size_t)nb * d.nldpc)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpyAsync(h->din.p, in, (size_t)nb * d.nbch, hipMemcpyHostToDevice, h->ctx.stream));
  FecIO io{};
  io.in = h->din.as<uint8_t>();
  io.out = h->dout.as<uint8_t>();
  io.nblocks = nb;
  HIP_TRY(launch_fec(FEC_BITS_TO_BITS, d, io, h->ctx.stream));
  HIP_TRY(hipMemcpyAsync(out, h->dout.p, (size_t)nb * d.nldpc, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  if (consumed) *consumed = nb * d.nbch;
  return nb * d.nldpc;
}
extern "C" void dvbt2ll_ldpc_destroy(dvbt2ll_ldpc *h) { delete h; }

// ============================================================================ interleavermod
struct dvbt2ll_interleavermod {
  DeviceCtx ctx;
  FecPlan fec;
  MapTables map;
  DevBuf din, dout;
};
extern "C" int dvbt2ll_interleavermod_create(const dvbt2ll_interleavermod_params *p, int device,
                                             dvbt2ll_interleavermod **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  std::unique_ptr<dvbt2ll_interleavermod> h(new (std::nothrow) dvbt2ll_interleavermod());
  if (!h) return DVBT2LL_ENOMEM;
  if (build_fec(p->framesize, p->rate, p->constellation, h->fec)) return DVBT2LL_EINVAL;
  int r = h->ctx.init(device);
  if (r) return r;
  if ((r = h->map.init(p->framesize, p->rate, p->constellation, p->rotation, h->fec))) return r;
  *out = h.release();
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_interleavermod_output_multiple(const dvbt2ll_interleavermod *h) { return h ? h->map.plan.cs : 0; }
extern "C" int dvbt2ll_interleavermod_forecast(const dvbt2ll_interleavermod *h, int nout, int *nin) {
  if (!h || !nin) return DVBT2LL_EINVAL;
  *nin = (nout / h->map.plan.cs) * h->map.plan.nldpc;   // interleavermod:264-268
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_interleavermod_general_work(dvbt2ll_interleavermod *h, int nout, int nin, const void *in,
                                                   void *out, int *consumed) {
  if (!h || nout < 0 || (nout && (!in || !out))) return DVBT2LL_EINVAL;
  const MapDev &d = h->map.dev;
  int nb = nout / d.cs;
  if (consumed) *consumed = 0;
  if (nb == 0) return 0;
  if ((int64_t)nb * d.nldpc > nin) return DVBT2LL_ESHORT;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->din.ensure((size_t)nb * d.nldpc) || h->dout.ensure((size_t)nb * d.cs * 8)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpyAsync(h->din.p, in, (size_t)nb * d.nldpc, hipMemcpyHostToDevice, h->ctx.stream));
  MapIO io{};
  io.in = h->din.as<uint8_t>();
  io.out = h->dout.as<float2>();
  io.nblocks = nb;
  HIP_TRY(launch_map(d, io, h->ctx.stream));
  HIP_TRY(hipMemcpyAsync(out, h->dout.p, (size_t)nb * d.cs * 8, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  if (consumed) *consumed = nb * d.nldpc;
  return nb * d.cs;
}
extern "C" void dvbt2ll_interleavermod_destroy(dvbt2ll_interleavermod *h) { delete h; }

// ============================================================================ framemapperfint
static FmParams to_fm(const dvbt2ll_framemapperfint_params &p) {
  return FmParams{p.framesize, p.rate, p.constellation, p.rotation, p.fecblocks, p.tiblocks, p.carriermode,
                  p.fftsize, p.guardinterval, p.l1constellation, p.pilotpattern, p.t2frames, p.numdatasyms,
                  p.paprmode, p.version, p.preamble, p.inputmode, p.reservedbiasbits, p.l1scrambled, p.inband};
}

struct dvbt2ll_framemapperfint {
  DeviceCtx ctx;
  FramePlan plan;
  L1Tables l1;
  DevBuf map, aux, din, dout;   // aux: one row; its L1-post cells are rewritten per call on the GPU
  int t2_frame_num = 0;
};
extern "C" int dvbt2ll_framemapperfint_create(const dvbt2ll_framemapperfint_params *p, int device,
                                              dvbt2ll_framemapperfint **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  std::unique_ptr<dvbt2ll_framemapperfint> h(new (std::nothrow) dvbt2ll_framemapperfint());
  if (!h) return DVBT2LL_ENOMEM;
  if (build_frame(to_fm(*p), h->plan)) return DVBT2LL_EINVAL;
  int r = h->ctx.init(device);
  if (r) return r;
  if ((r = upload(h->map, h->plan.gather_in)) || (r = upload(h->aux, h->plan.aux)) || (r = h->l1.init(h->plan)))
    return r;
  *out = h.release();
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_framemapperfint_output_multiple(const dvbt2ll_framemapperfint *h) { return h ? h->plan.M : 0; }
extern "C" int dvbt2ll_framemapperfint_stream_items(const dvbt2ll_framemapperfint *h) { return h ? h->plan.S : 0; }
extern "C" int dvbt2ll_framemapperfint_forecast(const dvbt2ll_framemapperfint *h, int nout, int *nin) {
  if (!h || !nin) return DVBT2LL_EINVAL;
  *nin = h->plan.S * (nout / h->plan.M);   // framemapper:1942-1946
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_framemapperfint_general_work(dvbt2ll_framemapperfint *h, int nout, int nin, const void *in,
                                                    void *out, int *consumed) {
  if (!h || nout < 0 || (nout && (!in || !out))) return DVBT2LL_EINVAL;
  const FramePlan &f = h->plan;
  if (consumed) *consumed = 0;
  if (nout < f.M) return 0;
  if (nin < f.S) return DVBT2LL_ESHORT;
  // one T2 frame per call (the reference consumes exactly one frame, framemapper:2147)
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->din.ensure((size_t)f.S * 8) || h->dout.ensure((size_t)f.M * 8)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpyAsync(h->din.p, in, (size_t)f.S * 8, hipMemcpyHostToDevice, h->ctx.stream));
  // this frame's L1-post cells (FRAME_IDX = t2_frame_num) into the aux row, then the gather
  L1IO lio{};
  lio.out = h->aux.as<float2>() + AUX_L1PRE + 1840;
  lio.first_frame = h->t2_frame_num;
  lio.nframes = 1;
  HIP_TRY(launch_l1post(h->l1.dev, lio, h->ctx.stream));
  GatherIO io{};
  io.in = h->din.as<float2>();
  io.out = h->dout.as<float2>();
  io.map = h->map.as<int32_t>();
  io.aux = h->aux.as<float2>();
  io.M = f.M;
  HIP_TRY(launch_gather(io, h->ctx.stream));
  HIP_TRY(hipMemcpyAsync(out, h->dout.p, (size_t)f.M * 8, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  h->t2_frame_num = (h->t2_frame_num + 1) % f.t2frames;
  if (consumed) *consumed = f.S;
  return f.M;
}
extern "C" void dvbt2ll_framemapperfint_destroy(dvbt2ll_framemapperfint *h) { delete h; }

// ============================================================================ framemapper, multi-PLP
static bool mplp_to_plan(const dvbt2ll_mplp_params &m, FmParams &fm, std::vector<PlpParams> &plps,
                         std::vector<int> &tsrate, int *nss) {
  if (m.nplp < 1 || m.nplp > DVBT2LL_MAX_PLP) return false;
  const dvbt2ll_plp_params &q0 = m.plp[0];
  fm = FmParams{q0.framesize, q0.rate, q0.constellation, q0.rotation, q0.fecblocks, q0.tiblocks, m.carriermode,
                m.fftsize, m.guardinterval, m.l1constellation, m.pilotpattern, m.t2frames, m.numdatasyms, m.paprmode,
                m.version, m.preamble, q0.inputmode, m.reservedbiasbits, m.l1scrambled, q0.inband};
  plps.clear();
  tsrate.clear();
  for (int k = 0; k < m.nplp; k++) {
    const dvbt2ll_plp_params &q = m.plp[k];
    plps.push_back(PlpParams{q.framesize, q.rate, q.constellation, q.rotation, q.fecblocks, q.tiblocks, q.inputmode,
                             q.inband, q.plp_type, q.ti_type, q.ti_frames, q.frame_interval, q.first_frame_idx});
    tsrate.push_back(q.tsrate);
  }
  *nss = m.num_subslices;
  return true;
}

struct dvbt2ll_framemapper_mplp {
  DeviceCtx ctx;
  FramePlan plan;
  L1Tables l1;
  // din: the current interleaving frame of every PLP (PLP k's S_if cells at in_off); map: one gather row per
  // frame phase (frame mod unit)
  DevBuf map, aux, din, dout;
  int t2_frame_num = 0;
  int64_t frame = 0;            // T2 frames produced (the phase of the next one is frame mod unit)
  // cells port k consumes at the T2 frame frame + i: a whole interleaving frame on its first T2 frame
  int need(int k, int64_t i) const {
    const PlpPlan &pl = plan.plp[k];
    return (frame + i) % pl.cycle() == pl.FF ? pl.S_if : 0;
  }
};
extern "C" int dvbt2ll_framemapper_mplp_create(const dvbt2ll_mplp_params *p, int device, dvbt2ll_framemapper_mplp **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  FmParams fm;
  std::vector<PlpParams> plps;
  std::vector<int> tsrate;
  int nss = 1;
  if (!mplp_to_plan(*p, fm, plps, tsrate, &nss)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_framemapper_mplp> h(new (std::nothrow) dvbt2ll_framemapper_mplp());
  if (!h) return DVBT2LL_ENOMEM;
  if (build_frame_mplp(fm, plps, h->plan, false, nss)) return DVBT2LL_EINVAL;
  int r = h->ctx.init(device);
  if (r) return r;
  if ((r = upload(h->map, h->plan.gather_in)) || (r = upload(h->aux, h->plan.aux)) || (r = h->l1.init(h->plan)))
    return r;
  *out = h.release();
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_framemapper_mplp_output_multiple(const dvbt2ll_framemapper_mplp *h) { return h ? h->plan.M : 0; }
extern "C" int dvbt2ll_framemapper_mplp_stream_items(const dvbt2ll_framemapper_mplp *h, int plp) {
  return h && plp >= 0 && plp < h->plan.nplp ? h->plan.plp[plp].S : 0;
}
extern "C" int dvbt2ll_framemapper_mplp_forecast(const dvbt2ll_framemapper_mplp *h, int nout, int *nin) {
  if (!h || !nin) return DVBT2LL_EINVAL;
  // framemapper:1942-1946: the cells of nout / M frames; a TIME_IL_TYPE 1 PLP's interleaving frame is
  // consumed whole on its first T2 frame
  for (int k = 0; k < h->plan.nplp; k++) {
    int64_t n = 0;
    for (int i = 0; i < nout / h->plan.M; i++) n += h->need(k, i);
    nin[k] = (int)std::min<int64_t>(n, INT32_MAX);
  }
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_framemapper_mplp_general_work(dvbt2ll_framemapper_mplp *h, int nout, const int *nin,
                                                     const void *const *in, void *out, int *consumed) {
  if (!h || nout < 0 || (nout && (!in || !out || !nin))) return DVBT2LL_EINVAL;
  const FramePlan &f = h->plan;
  if (consumed)
    for (int k = 0; k < f.nplp; k++) consumed[k] = 0;
  if (nout < f.M) return 0;
  for (int k = 0; k < f.nplp; k++)
    if (h->need(k, 0) && (!in[k] || nin[k] < h->need(k, 0))) return DVBT2LL_ESHORT;
  // one T2 frame per call, one frame of every port (framemapper:2147); a port whose PLP starts an interleaving
  // frame here delivers all of it
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->din.ensure((size_t)f.S_in * 8) || h->dout.ensure((size_t)f.M * 8)) return DVBT2LL_ENOMEM;
  for (int k = 0; k < f.nplp; k++)
    if (h->need(k, 0))
      HIP_TRY(hipMemcpyAsync(h->din.as<float2>() + f.plp[k].in_off, in[k], (size_t)f.plp[k].S_if * 8,
                             hipMemcpyHostToDevice, h->ctx.stream));
  L1IO lio{};
  lio.out = h->aux.as<float2>() + AUX_L1PRE + 1840;
  lio.first_frame = h->t2_frame_num;
  lio.nframes = 1;
  HIP_TRY(launch_l1post(h->l1.dev, lio, h->ctx.stream));
  GatherIO io{};
  io.in = h->din.as<float2>();
  io.out = h->dout.as<float2>();
  io.map = h->map.as<int32_t>() + (size_t)(h->frame % f.unit) * f.M;
  io.aux = h->aux.as<float2>();
  io.M = f.M;
  HIP_TRY(launch_gather(io, h->ctx.stream));
  HIP_TRY(hipMemcpyAsync(out, h->dout.p, (size_t)f.M * 8, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  if (consumed)
    for (int k = 0; k < f.nplp; k++) consumed[k] = h->need(k, 0);
  h->t2_frame_num = (h->t2_frame_num + 1) % f.t2frames;
  h->frame++;
  return f.M;
}
extern "C" void dvbt2ll_framemapper_mplp_destroy(dvbt2ll_framemapper_mplp *h) { delete h; }

// ============================================================================ pilotgenp1insert
static PgParams to_pg(const dvbt2ll_pilotgenp1insert_params &p) {
  return PgParams{p.carriermode, p.fftsize, p.pilotpattern, p.guardinterval, p.numdatasyms, p.paprmode, p.version,
                  p.preamble, p.misogroup, p.equalization, p.bandwidth, p.vlength};
}

struct OfdmTables {
  DevBuf map, tw, tw1k, isinc, p1;
  OfdmDev dev{};
  // stored_map: per-symbol rows in the kernel's read order (the chain: ofdm_stored_rows; the pilotgen
  // block's gather mode: natural order)
  int init(const PilotPlan &pp, const std::vector<int32_t> &stored_map, int aux_len, int t2frames) {
    int r;
    if ((r = upload(map, stored_map))) return r;
    if ((r = upload(tw, pp.twiddle)) || (r = upload(tw1k, pp.twiddle1k)) || (r = upload(p1, pp.p1))) return r;
    if (pp.eq && (r = upload(isinc, pp.isinc))) return r;
    dev.bin_map = map.as<int32_t>();
    dev.twiddle = tw.as<float2>();
    dev.twiddle1k = tw1k.as<float2>();
    dev.isinc = pp.eq ? isinc.as<float>() : nullptr;
    dev.p1 = p1.as<float2>();
    dev.N = pp.N; dev.G = pp.G; dev.Nsym = pp.Nsym; dev.aux_len = aux_len; dev.t2frames = t2frames;
    dev.norm = pp.normalization;
    dev.miso = pp.miso_proc;
    dev.gain = 1.f;
    dev.fmt = DVBT2LL_IQ_CF32;
    return 0;
  }
};

struct dvbt2ll_pilotgenp1insert {
  DeviceCtx ctx;
  PilotPlan plan;
  OfdmTables ofdm;
  DevBuf din, dout;    // din = [aux (pilot values) | one frame of mapped cells]
  int out_items = 0;
};
constexpr int PG_AUX_PAD = 16;
extern "C" int dvbt2ll_pilotgenp1insert_create(const dvbt2ll_pilotgenp1insert_params *p, int device,
                                               dvbt2ll_pilotgenp1insert **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  std::unique_ptr<dvbt2ll_pilotgenp1insert> h(new (std::nothrow) dvbt2ll_pilotgenp1insert());
  if (!h) return DVBT2LL_ENOMEM;
  if (build_pilot(to_pg(*p), h->plan)) return DVBT2LL_EINVAL;
  int r = h->ctx.init(device);
  if (r) return r;
  std::vector<cf32> aux(PG_AUX_PAD, cf32{0.f, 0.f});
  for (int i = 0; i < 12; i++) aux[AUX_PILOT0 + i] = h->plan.pilot_values[i];
  if ((r = h->ofdm.init(h->plan, h->plan.bin_map, PG_AUX_PAD, 1))) return r;   // gather rows: natural order
  if (h->din.ensure((size_t)(PG_AUX_PAD + h->plan.active) * 8)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpy(h->din.p, aux.data(), PG_AUX_PAD * 8, hipMemcpyHostToDevice));
  h->out_items = h->plan.Nsym * (h->plan.N + h->plan.G) + 2048;
  *out = h.release();
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_pilotgenp1insert_output_multiple(const dvbt2ll_pilotgenp1insert *h) { return h ? h->out_items : 0; }
extern "C" int dvbt2ll_pilotgenp1insert_active_items(const dvbt2ll_pilotgenp1insert *h) { return h ? h->plan.active : 0; }
extern "C" int dvbt2ll_pilotgenp1insert_forecast(const dvbt2ll_pilotgenp1insert *h, int nout, int *nin) {
  if (!h || !nin) return DVBT2LL_EINVAL;
  *nin = h->plan.active * (nout / h->out_items);   // pilotgen:1240-1243
  return DVBT2LL_OK;
}
static int pg_run(dvbt2ll_pilotgenp1insert *h, const void *in, void *out, int carriers_only) {
  const PilotPlan &pp = h->plan;
  size_t out_n = carriers_only ? (size_t)pp.Nsym * pp.N : (size_t)h->out_items;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->dout.ensure(out_n * 8)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpyAsync(h->din.as<float2>() + PG_AUX_PAD, in, (size_t)pp.active * 8, hipMemcpyHostToDevice,
                         h->ctx.stream));
  OfdmIO io{};
  io.data = h->din.as<float2>();
  io.aux_off = 0;
  io.cell_off = PG_AUX_PAD;
  io.cell_stride = (uint32_t)pp.active;
  io.out = h->dout.as<float2>();
  io.out_stride = (int64_t)out_n;
  io.first_frame = 0;
  io.nframes = 1;
  io.carriers_only = carriers_only;
  HIP_TRY(launch_ofdm(h->ofdm.dev, io, h->ctx.stream));
  HIP_TRY(hipMemcpyAsync(out, h->dout.p, out_n * 8, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  return 0;
}
extern "C" int dvbt2ll_pilotgenp1insert_general_work(dvbt2ll_pilotgenp1insert *h, int nout, int nin, const void *in,
                                                     void *out, int *consumed) {
  if (!h || nout < 0 || (nout && (!in || !out))) return DVBT2LL_EINVAL;
  if (consumed) *consumed = 0;
  if (nout < h->out_items) return 0;
  if (nin < h->plan.active) return DVBT2LL_ESHORT;
  int r = pg_run(h, in, out, 0);   // one T2 frame per call (pilotgen:2903)
  if (r) return r;
  if (consumed) *consumed = h->plan.active;
  return h->out_items;
}
extern "C" int dvbt2ll_pilotgenp1insert_debug_carriers(dvbt2ll_pilotgenp1insert *h, const void *in, void *carriers) {
  if (!h || !in || !carriers) return DVBT2LL_EINVAL;
  return pg_run(h, in, carriers, 1);
}
extern "C" void dvbt2ll_pilotgenp1insert_destroy(dvbt2ll_pilotgenp1insert *h) { delete h; }

// ============================================================================ chain
// One PLP of the fused chain: its FEC and map tables, the cell-interleaver / time-interleaver store
// tables, and per buffer slot its packed codewords and BCH parities.  A single-PLP chain (the
// reference's frame) has one.
struct ChainPlp {
  FecTables fec;
  MapTables map;
  DevBuf part, pbase, poff, pnq;
  DevBuf cw[DVBT2LL_CHAIN_MAX_SLOTS], bpart[DVBT2LL_CHAIN_MAX_SLOTS];
  int64_t cw_stride = 0;
  int64_t ts_per_frame = 0;   // payload bytes per interleaving frame (NM positions; HEM: before sync-byte removal)
  int pay = 0, F = 0, inputmode = 0, inband = 0;
  int P = 1;                  // T2 frames per interleaving frame (TIME_IL_TYPE 1: P_I); F, ts_per_frame are per
                              // interleaving frame
  int cyc = 1;                // T2 frames from one interleaving frame to the next (P_I x FRAME_INTERVAL)
  int64_t blocks(int64_t frames) const { return (frames + cyc - 1) / cyc * F; }   // FEC blocks of `frames` T2 frames
  // what the run calls' input holds (dvbt2ll_chain_set_input): the TS, or packed BBFRAMEs of bbf_len() bytes,
  // interleaving frame m consuming stream bytes [m F bbf_len(), (m + 1) F bbf_len())
  int input = DVBT2LL_INPUT_TS;
  int64_t bbf_len() const { return fec.plan.kbch / 8; }
  // the unit the run calls' ts_base must be a multiple of
  int64_t base_unit() const { return input == DVBT2LL_INPUT_BBFRAME ? bbf_len() : 188; }
};

// instantiated hipGraphs of the chain's kernels (per PLP: bbch_kernel, BBFRAMEs + matrix-core BCH; per PLP: LDPC +
// map (PLP 0's launch also generates the L1-post); OFDM) for one (nframes, IQ format, slot),
// captured once from the ordinary launch path into a ring of instantiations.  A call takes the next
// ring entry, waits for it only if it is still in flight, rewrites its kernel nodes' arguments
// (hipGraphExecKernelNodeSetParams) and launches it.
struct ChainGraph {
  int nframes = 0, fmt = -1, slot = -1;
  hipGraph_t graph = nullptr;
  std::vector<hipGraphNode_t> node;            // kernel nodes in launch order
  std::vector<hipKernelNodeParams> base;
  hipGraphExec_t exec[DVBT2LL_CHAIN_GRAPH_RING] = {};
  hipEvent_t done[DVBT2LL_CHAIN_GRAPH_RING] = {};
  bool used[DVBT2LL_CHAIN_GRAPH_RING] = {};
  // the argument bytes each instantiation's kernel nodes hold: a call whose arguments match skips
  // hipGraphExecKernelNodeSetParams (one per node, the bulk of a graph call's host time)
  std::vector<std::vector<uint8_t>> held[DVBT2LL_CHAIN_GRAPH_RING];
  int next = 0;
  ~ChainGraph() {
    for (auto &e : exec)
      if (e) (void)hipGraphExecDestroy(e);
    for (auto &e : done)
      if (e) (void)hipEventDestroy(e);
    if (graph) (void)hipGraphDestroy(graph);
  }
};

// the asynchronous host path (dvbt2ll_chain_host_submit): a ring of submissions, each with its own device TS
// and IQ buffers and three events; the TS copy-in, the kernels and the IQ copy-out of a submission run on
// three streams ordered by those events, so consecutive submissions overlap (copy-in of k + 1 and copy-out
// of k - 1 beside the kernels of k)
struct HostRing {
  hipStream_t in = nullptr, comp = nullptr, out = nullptr;
  struct Entry {
    DevBuf ts, iq;
    hipEvent_t h2d = nullptr, kern = nullptr, d2h = nullptr;
    int64_t ticket = -1;   // the submission holding the entry (-1: never used)
  } e[DVBT2LL_HOST_RING];
  int64_t next_ticket = 0;
  int init(int device) {
    if (in) return 0;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&in, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&comp, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&out, hipStreamNonBlocking));
    for (auto &x : e) {
      HIP_TRY(hipEventCreateWithFlags(&x.h2d, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&x.kern, hipEventDisableTiming));
      HIP_TRY(hipEventCreateWithFlags(&x.d2h, hipEventDisableTiming));
    }
    return 0;
  }
  hipError_t synchronize() const {
    for (hipStream_t st : {in, comp, out})
      if (st) {
        hipError_t r = hipStreamSynchronize(st);
        if (r != hipSuccess) return r;
      }
    return hipSuccess;
  }
  ~HostRing() {
    (void)synchronize();   // no copy or kernel of a submission may outlive the entries' buffers
    for (auto &x : e)
      for (hipEvent_t ev : {x.h2d, x.kern, x.d2h})
        if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t st : {in, comp, out})
      if (st) (void)hipStreamDestroy(st);
  }
};

struct dvbt2ll_chain {
  DeviceCtx ctx;
  HostRing host;
  dvbt2ll_chain_params p{};   // single-PLP create parameters (PLP 0's for a multi-PLP chain)
  int nplp = 1;
  std::vector<std::unique_ptr<ChainPlp>> plps;
  FramePlan frame;
  PilotPlan pilot;
  OfdmTables ofdm;
  DevBuf aux, inv, sym_d0, sym_n, sym_n0, ts_tmp, iq_tmp;
  DevBuf ts_plp_tmp[DVBT2LL_MAX_PLP];   // run_plps_host: each PLP's TS on the device
  DevBuf abin, aval, aind, agrp, azr;   // non-data bins as compact lists (t2_plan.h AuxLists)
  DevBuf plp_bnd, plp_qbase, qam_all;   // multi-PLP frames: slot ranges per PLP, the PLPs' constellations
  DevBuf cls_inv;                       // per frame class: its data slots' bins at inv + cls_inv[c]
  // MISO pair chain (dvbt2ll_chain_create_miso_pair): both transmitter groups from one FEC + map pass.  pilot /
  // ofdm are group 1's (MISO_TX1); group 2's (MISO_TX2_PROCESSED) OFDM launch reads the same index pairs and L1-post
  // cells through tables of its own over group 1's slot order (t2_plan.h build_pair_layout): its bins, aux lists
  // and, at 32K, the cross lists.  The symbol runs, PLP boundaries, class offsets and constellations are shared.
  bool pair = false;
  PilotPlan pilot2;
  OfdmTables ofdm2;
  DevBuf inv2, abin2, aval2, aind2, agrp2, azr2, xent, xgrp;
  std::vector<int32_t> plp_bnd_host;
  std::vector<int> qbase_host;
  DevBuf sync_err;                      // TS sync bytes != 0x47 consumed by run calls (bbheader:675, 703)
  DevBuf bbh_err;                       // BBFRAME input: BBFRAMEs consumed whose header CRC-8 does not match
  // intermediate buffer slots (index pairs, L1-post cells; the PLPs' codewords): run calls take them
  // round-robin, so calls issued on different streams overlap; a slot reused on another stream first
  // waits for its previous run (slot_done) -- see dvbt2ll_chain_set_slots
  DevBuf pairs[DVBT2LL_CHAIN_MAX_SLOTS];
  // per-frame L1-post cells of a run (l1post_kernel -> the OFDM kernel's indirect aux entries)
  L1Tables l1;
  DevBuf l1buf[DVBT2LL_CHAIN_MAX_SLOTS];
  uint32_t l1_stride = 0;
  hipEvent_t slot_done[DVBT2LL_CHAIN_MAX_SLOTS] = {};
  hipStream_t slot_stream[DVBT2LL_CHAIN_MAX_SLOTS] = {};
  // test hook (dvbt2ll_chain_debug_keep_codewords): runs also store the codewords; per slot, whether its
  // last run did
  bool keep_cw = false;
  bool cw_kept[DVBT2LL_CHAIN_MAX_SLOTS] = {};
  bool slot_used[DVBT2LL_CHAIN_MAX_SLOTS] = {};
  // a run on the slot failed after its FEC pass may have run: its BCH partial parities are not known to be zero
  bool bpart_dirty[DVBT2LL_CHAIN_MAX_SLOTS] = {};
  int nslots = 1, next_slot = 0, last_slot = 0;
  // hipGraph mode (dvbt2ll_chain_set_graph)
  bool use_graph = false;
  hipStream_t cap_stream = nullptr;
  std::vector<std::unique_ptr<ChainGraph>> graphs;
  int max_frames = 0;
  int64_t pair_stride = 0;   // pairs buffer: frame k's slots at k * pair_stride (multiple of 8)
  int64_t iq_per_frame = 0;
  // stage timing: 4 events per run (start, after fec, after map + L1-post, after ofdm) recorded
  // on the launch stream without host synchronisation; folded into ms[] by get_timing()
  // (stages 0 fec, 1 map, 2 ofdm; stage 3 is reserved and stays 0)
  static constexpr int NEV = 4;
  bool timing = false;
  std::vector<hipEvent_t> evpool;
  size_t evused = 0;
  double ms[4] = {0, 0, 0, 0};
  int64_t launches[4] = {0, 0, 0, 0};
  hipEvent_t next_event() {
    if (evused == evpool.size()) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return nullptr;
      evpool.push_back(e);
    }
    return evpool[evused++];
  }
  // every run's end event is waited on (runs may sit on several streams, so the last recorded
  // event does not imply the earlier ones); the pool is emptied even when a query fails
  int fold_timing() {
    if (!evused) return 0;
    int st = 0;
    static const int stage_of[NEV - 1] = {0, 1, 2};   // event interval k -> stage
    for (size_t b = 0; b + NEV - 1 < evused && !st; b += NEV) {
      hipError_t e = hipEventSynchronize(evpool[b + NEV - 1]);
      for (int k = 0; k < NEV - 1 && e == hipSuccess; k++) {
        float t = 0;
        e = hipEventElapsedTime(&t, evpool[b + k], evpool[b + k + 1]);
        if (e == hipSuccess) {
          ms[stage_of[k]] += t;
          launches[stage_of[k]] += 1;
        }
      }
      if (e != hipSuccess) {
        last_hip_error() = e;
        st = DVBT2LL_EDEVICE;
      }
    }
    evused = 0;
    return st;
  }
  // the chain's kernels on stream s: every PLP's BB + matrix-core BCH kernel, every PLP's LDPC + map
  // (PLP 0's launch has the extra workgroups that generate the frames' L1-post cells), OFDM.  ev1, ev2
  // (timing): recorded after the BB + BCH kernels and after the LDPC + map kernels.  A pair handle: oio2 is group
  // 2's OFDM launch over the same pairs and L1-post cells; a group whose output pointer is null is skipped
  hipError_t launch_chain(const L1IO &lio, const FecIO *fio, const MapIO *mio, const OfdmIO &oio, hipStream_t s,
                          hipEvent_t ev1, hipEvent_t ev2, const OfdmIO *oio2 = nullptr) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < nplp && e == hipSuccess; k++) e = launch_fec(FEC_TS_TO_BBFRAME, plps[k]->fec.dev, fio[k], s);
    if (e == hipSuccess && ev1) e = hipEventRecord(ev1, s);
    for (int k = 0; k < nplp && e == hipSuccess; k++)
      e = k == 0 ? launch_ldpc_map(plps[k]->fec.dev, fio[k], plps[k]->map.dev, mio[k], s, &l1.dev, &lio)
                 : launch_ldpc_map(plps[k]->fec.dev, fio[k], plps[k]->map.dev, mio[k], s);
    if (e == hipSuccess && ev2) e = hipEventRecord(ev2, s);
    if (e == hipSuccess && (!pair || oio.out)) e = launch_ofdm(ofdm.dev, oio, s);
    if (e == hipSuccess && pair && oio2 && oio2->out) e = launch_ofdm(ofdm2.dev, *oio2, s);
    return e;
  }
  // kernel nodes per run: the fused BB + BCH pass and the LDPC + map kernel per PLP, one OFDM
  int graph_nodes() const { return 2 * nplp + 1; }
  int graph_launch(const L1IO &lio, const FecIO *fio, const MapIO *mio, const OfdmIO &oio, int nframes, int slot,
                   hipStream_t s) {
    const int nk = graph_nodes();
    ChainGraph *g = nullptr;
    for (auto &c : graphs)
      if (c->nframes == nframes && c->fmt == ofdm.dev.fmt && c->slot == slot) g = c.get();
    if (!g) {
      if (!cap_stream) HIP_TRY(hipStreamCreateWithFlags(&cap_stream, hipStreamNonBlocking));
      std::unique_ptr<ChainGraph> c(new (std::nothrow) ChainGraph());
      if (!c) return DVBT2LL_ENOMEM;
      c->nframes = nframes;
      c->fmt = ofdm.dev.fmt;
      c->slot = slot;
      HIP_TRY(hipStreamBeginCapture(cap_stream, hipStreamCaptureModeThreadLocal));
      hipError_t e1 = launch_chain(lio, fio, mio, oio, cap_stream, nullptr, nullptr);
      hipError_t ec = hipStreamEndCapture(cap_stream, &c->graph);
      HIP_TRY(e1);
      HIP_TRY(ec);
      // the kernel nodes in dependency order: a linear chain of nk
      size_t n = 0;
      HIP_TRY(hipGraphGetNodes(c->graph, nullptr, &n));
      std::vector<hipGraphNode_t> nodes(n);
      HIP_TRY(hipGraphGetNodes(c->graph, nodes.data(), &n));
      std::vector<hipGraphNode_t> kn;
      for (auto nd : nodes) {
        hipGraphNodeType t;
        HIP_TRY(hipGraphNodeGetType(nd, &t));
        if (t == hipGraphNodeTypeKernel) kn.push_back(nd);
      }
      if ((int)kn.size() != nk) return DVBT2LL_EDEVICE;
      c->node.assign(nk, nullptr);
      c->base.assign(nk, hipKernelNodeParams{});
      // order: the root (no dependencies), then the node depending on it, and so on
      hipGraphNode_t prev = nullptr;
      for (int k = 0; k < nk; k++) {
        for (auto nd : kn) {
          size_t nd_n = 0;
          HIP_TRY(hipGraphNodeGetDependencies(nd, nullptr, &nd_n));
          bool ok = false;
          if (k == 0) {
            ok = nd_n == 0;
          } else if (nd_n == 1) {
            hipGraphNode_t dep = nullptr;
            size_t one = 1;
            HIP_TRY(hipGraphNodeGetDependencies(nd, &dep, &one));
            ok = dep == prev;
          }
          if (ok) { c->node[k] = nd; break; }
        }
        if (!c->node[k]) return DVBT2LL_EDEVICE;
        prev = c->node[k];
        HIP_TRY(hipGraphKernelNodeGetParams(c->node[k], &c->base[k]));
      }
      for (int r = 0; r < DVBT2LL_CHAIN_GRAPH_RING; r++) {
        HIP_TRY(hipGraphInstantiate(&c->exec[r], c->graph, nullptr, nullptr, 0));
        HIP_TRY(hipEventCreateWithFlags(&c->done[r], hipEventDisableTiming));
      }
      g = c.get();
      graphs.push_back(std::move(c));
    }
    // the ring's next instantiation; the host waits only if it is still in flight (every entry of
    // the ring is), so consecutive calls never wait for each other below that depth
    const int r = g->next;
    g->next = (r + 1) % DVBT2LL_CHAIN_GRAPH_RING;
    if (g->used[r]) HIP_TRY(hipEventSynchronize(g->done[r]));
    L1Dev ld = l1.dev, ld0{};   // PLP 0's map launch generates the L1-post, the others carry none
    L1IO li = lio, li0{};
    OfdmDev od = ofdm.dev;
    OfdmIO oi = oio;
    std::vector<FecDev> fd(nplp);
    std::vector<FecIO> fi(fio, fio + nplp);
    std::vector<MapDev> md(nplp);
    std::vector<MapIO> mi(mio, mio + nplp);
    std::vector<std::vector<void *>> args;
    for (int k = 0; k < nplp; k++) {
      fd[k] = plps[k]->fec.dev;
      md[k] = plps[k]->map.dev;
    }
    for (int k = 0; k < nplp; k++) args.push_back({&fd[k], &fi[k]});
    for (int k = 0; k < nplp; k++) args.push_back({&fd[k], &fi[k], &md[k], &mi[k], k ? &ld0 : &ld, k ? &li0 : &li});
    args.push_back({&od, &oi});
    std::vector<std::vector<size_t>> sizes;
    for (int k = 0; k < nplp; k++) sizes.push_back({sizeof(FecDev), sizeof(FecIO)});
    for (int k = 0; k < nplp; k++)
      sizes.push_back({sizeof(FecDev), sizeof(FecIO), sizeof(MapDev), sizeof(MapIO), sizeof(L1Dev), sizeof(L1IO)});
    sizes.push_back({sizeof(OfdmDev), sizeof(OfdmIO)});
    if (g->held[r].size() != (size_t)nk) g->held[r].assign(nk, {});
    for (int k = 0; k < nk; k++) {
      std::vector<uint8_t> bytes;
      for (size_t a = 0; a < args[k].size(); a++) {
        const uint8_t *b = (const uint8_t *)args[k][a];
        bytes.insert(bytes.end(), b, b + sizes[k][a]);
      }
      if (bytes == g->held[r][k]) continue;
      hipKernelNodeParams p = g->base[k];
      p.kernelParams = args[k].data();
      p.extra = nullptr;
      g->held[r][k].clear();   // unknown until the update succeeds
      HIP_TRY(hipGraphExecKernelNodeSetParams(g->exec[r], g->node[k], &p));
      g->held[r][k] = std::move(bytes);
    }
    HIP_TRY(hipGraphLaunch(g->exec[r], s));
    HIP_TRY(hipEventRecord(g->done[r], s));
    g->used[r] = true;
    return 0;
  }
  int alloc_slot(int k) {
    for (auto &pl : plps) {
      // one spare row past the largest launch: the fused FEC pass stores its dead lanes' pieces there
      if (pl->cw[k].ensure((size_t)(pl->blocks(max_frames) + 1) * pl->cw_stride) ||
          pl->bpart[k].ensure((size_t)pl->blocks(max_frames) * BCH_PART_WORDS * sizeof(uint32_t)))
        return DVBT2LL_ENOMEM;
      // the BCH partial parities start at zero (bbch_kernel XORs into them, ldpc_map_kernel zeroes what it reads)
      HIP_TRY(hipMemset(pl->bpart[k].p, 0, pl->bpart[k].n));
    }
    bpart_dirty[k] = false;
    if (pairs[k].ensure((size_t)pair_stride * max_frames * 2) || l1buf[k].ensure((size_t)l1_stride * max_frames * 8))
      return DVBT2LL_ENOMEM;
    if (!slot_done[k]) HIP_TRY(hipEventCreateWithFlags(&slot_done[k], hipEventDisableTiming));
    return 0;
  }
  ~dvbt2ll_chain() {
    // every run still in flight (the ring's streams, the slots' last runs on caller streams) ends before
    // the slot buffers and ring entries are freed
    (void)host.synchronize();
    for (int k = 0; k < DVBT2LL_CHAIN_MAX_SLOTS; k++)
      if (slot_used[k] && slot_done[k]) (void)hipEventSynchronize(slot_done[k]);
    graphs.clear();
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    for (auto &e : evpool)
      if (e) (void)hipEventDestroy(e);
    for (auto &e : slot_done)
      if (e) (void)hipEventDestroy(e);
  }
};

// One transmitter group's scatter tables as the OFDM kernels read them, from its layouts (one per frame class) over
// the aux row auxv: the data slots' bins as padded LDS slots within their half (the kernel writes them as they
// are), the classes' tables back to back, each class's bins from an 8-slot boundary (the kernel reads aligned quads
// / octets; cls_inv: each class's offset); the classes' aux lists back to back (a class's dummy cells differ) with
// the group offsets rebased, their bins and zero runs as padded slots, and the tail padding the kernels' last loads
// want.  cross (a pair handle's group 2, else null): the classes' cross-listed slots get one of the kernel's dummy
// LDS slots, the ones after the half's padded bins (t2_kernels.hip), as their bin.
struct GroupTables {
  std::vector<uint16_t> inv_pad;
  std::vector<int32_t> cls_inv, zr;
  AuxLists al;
};
static int group_tables(const FramePlan &fp, const PilotPlan &pp, const std::vector<ChainLayout> &layouts,
                        const std::vector<CrossLists> *cross, const std::vector<cf32> &auxv, GroupTables &t) {
  const int nsub_h = ofdm_split(pp.N) ? pp.N / 2 : pp.N;
  const uint32_t dummy0 = ofdm_padded_bin(pp.N, (uint32_t)nsub_h);
  // (MISO-processed frames: the selector stays in the padded bin's top bit)
  const uint16_t selbit = pp.miso_proc ? (uint16_t)(1u << MISO_INV_SEL_BIT) : (uint16_t)0;
  AuxLists &al = t.al;
  for (size_t c = 0; c < layouts.size(); c++) {
    const ChainLayout &lc = layouts[c];
    t.cls_inv.push_back((int32_t)t.inv_pad.size());
    for (size_t si = 0; si < lc.inv.size(); si++)
      t.inv_pad.push_back(cross && (*cross)[c].skip[si]
                              ? (uint16_t)(dummy0 + (si & 63))
                              : (uint16_t)(ofdm_padded_bin(pp.N, (lc.inv[si] & ~selbit) % nsub_h) | (lc.inv[si] & selbit)));
    t.inv_pad.resize(((t.inv_pad.size() + 7) & ~(size_t)7) + 8, 0);
    AuxLists ac;
    if (build_aux_lists(lc, pp.N, pp.Nsym, auxv, fp.aux_len, 1, ac, AUX_L1PRE + 1840, fp.Lp)) return DVBT2LL_EINVAL;
    if (ac.dbin.size() % 4) return DVBT2LL_EINVAL;   // groups of direct quads stay aligned
    for (size_t g = 0; g + 3 < ac.grp.size(); g += 4) {
      ac.grp[g] += (int32_t)al.dbin.size();
      ac.grp[g + 2] += (int32_t)al.ind.size();
    }
    al.dbin.insert(al.dbin.end(), ac.dbin.begin(), ac.dbin.end());
    al.dval.insert(al.dval.end(), ac.dval.begin(), ac.dval.end());
    al.ind.insert(al.ind.end(), ac.ind.begin(), ac.ind.end());
    al.grp.insert(al.grp.end(), ac.grp.begin(), ac.grp.end());
    al.zrun.insert(al.zrun.end(), ac.zrun.begin(), ac.zrun.end());
  }
  for (auto &b : al.dbin)
    if (b != 0xFFFF) b = (uint16_t)ofdm_padded_bin(pp.N, b);
  for (auto &e : al.ind) e = ofdm_padded_bin(pp.N, e & 0x7FFFu) | (e & ~0x7FFFu);   // (code and selector bits kept)
  t.zr.assign(al.zrun.size(), 0);   // zero runs as padded slot ranges
  for (size_t g = 0; g + 1 < al.zrun.size(); g += 2) {
    const int z0 = al.zrun[g], z1 = al.zrun[g + 1];
    t.zr[g] = z1 > z0 ? (int32_t)ofdm_padded_bin(pp.N, (uint32_t)z0) : 0;
    t.zr[g + 1] = z1 > z0 ? (int32_t)ofdm_padded_bin(pp.N, (uint32_t)(z1 - 1)) + 1 : 0;
  }
  al.ind.push_back(0);   // never empty (device pointer)
  al.dbin.resize(al.dbin.size() + 4, 0xFFFF);
  al.dval.resize(al.dval.size() + 4, cf32{0.f, 0.f});
  return 0;
}

// A pair handle's group 2 (MISO_TX2_PROCESSED) after group 1's tables are built: its pilot plan, and per frame
// class its layout over group 1's slot order (layouts: group 1's; cls_inv: their offsets in the bin table), as
// device tables.  pg1: group 1's pilot parameters; auxrow: the frame's aux row.
static_assert(MISO_CROSS_MAX == OFDM_CROSS_MAX, "the planner's cross-list capacity is the 32K kernel's");
static int chain_build_group2(dvbt2ll_chain *h, const PgParams &pg1, const std::vector<ChainLayout> &layouts,
                              const std::vector<int32_t> &cls_inv, const std::vector<cf32> &auxrow) {
  const FramePlan &fp = h->frame;
  PgParams pg = pg1;
  pg.misogroup = MISO_TX2_PROCESSED;
  if (build_pilot(pg, h->pilot2) || h->pilot2.active != fp.M) return DVBT2LL_EINVAL;
  const PilotPlan &pp = h->pilot2;
  const bool split = ofdm_split(pp.N);
  const int nsub_h = split ? pp.N / 2 : pp.N;
  std::vector<cf32> auxv = auxrow;
  for (int i = 0; i < 12; i++) auxv[AUX_PILOT0 + i] = pp.pilot_values[i];
  std::vector<ChainLayout> lay2(fp.ncls);
  std::vector<CrossLists> cross(fp.ncls);
  std::vector<uint32_t> xent;
  std::vector<int32_t> xgrp;
  for (int c = 0; c < fp.ncls; c++) {
    const CrossLists &xl = cross[c];
    if (build_pair_layout(fp, h->pilot, layouts[c], pp, lay2[c], cross[c], c) || xl.max_len > OFDM_CROSS_MAX)
      return DVBT2LL_EINVAL;
    for (size_t g = 0; g + 1 < xl.grp.size(); g += 2) {
      xgrp.push_back(xl.grp[g] + (int32_t)(xent.size() / 2));
      xgrp.push_back(xl.grp[g + 1]);
    }
    for (const CrossEntry &e : xl.ent) {
      const int qb = h->qbase_host[e.plp];
      if (e.bin >= nsub_h || qb < 0 || qb > 0xFFFF || e.slot < 0 || e.slot >= h->pair_stride) return DVBT2LL_EINVAL;
      xent.push_back((uint32_t)e.slot);
      xent.push_back(ofdm_padded_bin(pp.N, e.bin) | (uint32_t)(e.sel & 1) << 15 | (uint32_t)qb << 16);
    }
  }
  xent.resize(xent.size() + 2, 0);   // never empty (device pointer)
  GroupTables t;
  int r;
  if ((r = group_tables(fp, pp, lay2, &cross, auxv, t))) return r;
  if (t.cls_inv != cls_inv) return DVBT2LL_EINVAL;   // the classes' offsets are group 1's
  const std::vector<int32_t> &cmap0 = lay2[0].cmap;
  const AuxLists &al = t.al;
  if ((r = h->ofdm2.init(pp, cmap0, fp.aux_len, 1))) return r;
  if ((r = upload(h->inv2, t.inv_pad)) || (r = upload(h->abin2, al.dbin)) || (r = upload(h->aval2, al.dval)) ||
      (r = upload(h->aind2, al.ind)) || (r = upload(h->agrp2, al.grp)) || (r = upload(h->azr2, t.zr)) ||
      (r = upload(h->xent, xent)) || (r = upload(h->xgrp, xgrp)))
    return r;
  // the symbol runs, PLP boundaries, class offsets and constellations are group 1's
  const OfdmDev &o1 = h->ofdm.dev;
  OfdmDev &od = h->ofdm2.dev;
  od.inv = h->inv2.as<uint16_t>();
  od.abin = h->abin2.as<uint16_t>();
  od.aval = h->aval2.as<float2>();
  od.aind = h->aind2.as<uint32_t>();
  od.agrp = h->agrp2.as<int4>();
  od.azr = h->azr2.as<int2>();
  od.sym_d0 = o1.sym_d0;
  od.sym_n = o1.sym_n;
  od.sym_n0 = o1.sym_n0;
  od.ncls = o1.ncls;
  od.cls_inv = o1.cls_inv;
  od.nplp = o1.nplp;
  od.qam = o1.qam;
  od.nq = o1.nq;
  od.plp_bnd = o1.plp_bnd;
  od.plp_qbase = o1.plp_qbase;
  if (split) {   // 32K: the cross lists select the pair kernel
    od.xent = h->xent.as<uint2>();
    od.xgrp = h->xgrp.as<int2>();
  }
  return 0;
}

// the common construction of single- and multi-PLP chains: fm's common fields with plps' PLPs
static int chain_build(dvbt2ll_chain *h, const FmParams &fm, const std::vector<PlpParams> &plps,
                       const std::vector<int> &tsrate, int misogroup, int equalization, int bandwidth, int device,
                       int nss = 1) {
  PgParams pg{fm.carriermode, fm.fftsize, fm.pilotpattern, fm.guardinterval, fm.numdatasyms, fm.paprmode, fm.version,
              fm.preamble, misogroup, equalization, bandwidth, fft_points(fm.fftsize)};
  if (build_frame_mplp(fm, plps, h->frame, false, nss) || build_pilot(pg, h->pilot)) return DVBT2LL_EINVAL;
  if (h->pilot.active != h->frame.M) return DVBT2LL_EINVAL;
  const FramePlan &fp = h->frame;
  if (h->max_frames < fp.unit) return DVBT2LL_EINVAL;   // runs cover whole interleaving frames
  h->nplp = fp.nplp;
  h->pair_stride = ((int64_t)fp.S + 7) / 8 * 8;
  int r = h->ctx.init(device);
  if (r) return r;
  // OFDM side: aux bins from cmap, data cells streamed per symbol and scattered through inv
  // one layout per frame class (FRAME_INTERVAL > 1: the T2 frames carry different PLPs); class 0's is `layout`
  std::vector<ChainLayout> layouts(fp.ncls);
  for (int c = 0; c < fp.ncls; c++)
    if (build_chain_layout(fp, h->pilot, layouts[c], c)) return DVBT2LL_EINVAL;
  const ChainLayout &layout = layouts[0];
  int nq = 0;   // the PLPs' constellation tables back to back (multi-PLP); 256 entries for one PLP
  std::vector<cf32> qall;
  for (int k = 0; k < h->nplp; k++) {
    const PlpParams &q = plps[k];
    std::unique_ptr<ChainPlp> pl(new (std::nothrow) ChainPlp());
    if (!pl) return DVBT2LL_ENOMEM;
    const PlpPlan &pp = fp.plp[k];
    if ((r = pl->fec.init(q.framesize, q.rate, q.constellation, q.inputmode, q.inband, q.fecblocks, tsrate[k])))
      return r;
    // one PLP of several: multiple input streams, ISI = the PLP_ID (bbheader:288-298)
    if (h->nplp > 1) pl->fec.dev.matype = MATYPE_MIS | k;
    if ((r = pl->fec.init_chain())) return r;
    if ((r = pl->map.init(q.framesize, q.rate, q.constellation, q.rotation, pl->fec.plan))) return r;
    MapDev &md = pl->map.dev;
    // the LDPC + map kernel's cell interleaver + TI store as a quad table over one launch unit (t2_plan.h QuadTable)
    QuadTable qt;
    if (build_quad_table(fp, layouts, k, h->pair_stride, qt)) return DVBT2LL_EINVAL;
    md.F = qt.rows;
    if ((r = upload(pl->part, qt.qsrc)) || (r = upload(pl->pbase, qt.qb)) || (r = upload(pl->poff, qt.qoff)) ||
        (r = upload(pl->pnq, qt.qn)))
      return r;
    md.slot_quad = pl->part.as<uint2>();
    md.slot_qoff = pl->poff.as<uint16_t>();
    md.slot_qbase = pl->pbase.as<int32_t>();
    md.slot_nq = pl->pnq.as<int32_t>();
    md.slot_stride = qt.stride;
    pl->F = pp.F;
    pl->P = pp.P;
    pl->cyc = pp.cycle();
    pl->inputmode = q.inputmode;
    pl->inband = q.inband;
    pl->cw_stride = ((pl->fec.plan.nldpc / 8) + 255) / 256 * 256;
    pl->pay = (pl->fec.plan.kbch - 80) / 8;
    // payload bytes per interleaving frame: in-band type B takes 13 bytes of its first BBFRAME
    // (bbheader:327-355, fec_block == 0)
    pl->ts_per_frame = (int64_t)pp.F * pl->pay - (q.inband ? 13 : 0);
    // PLPs with the same constellation and rotation share one table (their LUTs are equal)
    int qb0 = -1;
    for (int k2 = 0; k2 < k && qb0 < 0; k2++)
      if (plps[k2].constellation == q.constellation && plps[k2].rotation == q.rotation) qb0 = h->qbase_host[k2];
    if (qb0 < 0) {
      qb0 = nq;
      const int entries = 1 << pl->map.plan.mod;
      for (int i = 0; i < entries; i++) qall.push_back(pl->map.plan.lut[i]);
      nq += entries;
    }
    h->qbase_host.push_back(qb0);
    h->plps.push_back(std::move(pl));
  }
  const PilotPlan &pp = h->pilot;
  // one aux row (pilot values, L1-pre, dummy cells): the L1-post cells come per frame from the GPU
  std::vector<cf32> auxv = fp.aux;
  for (int i = 0; i < 12; i++) auxv[AUX_PILOT0 + i] = pp.pilot_values[i];
  // the data slots' padded bins and the aux lists of every frame class (group_tables), and the classes' symbol runs
  GroupTables t;
  if ((r = group_tables(fp, pp, layouts, nullptr, auxv, t))) return r;
  const std::vector<int32_t> &cls_inv = t.cls_inv;
  const AuxLists &al = t.al;
  std::vector<int32_t> sd0, sdn, sdn0, bnd_all;
  for (const ChainLayout &lc : layouts) {
    sd0.insert(sd0.end(), lc.sym_d0.begin(), lc.sym_d0.end());
    sdn.insert(sdn.end(), lc.sym_n.begin(), lc.sym_n.end());
    sdn0.insert(sdn0.end(), lc.sym_n0.begin(), lc.sym_n0.end());
    bnd_all.insert(bnd_all.end(), lc.plp_bnd.begin(), lc.plp_bnd.end());
  }
  if ((r = upload(h->inv, t.inv_pad)) || (r = upload(h->sym_d0, sd0)) || (r = upload(h->sym_n, sdn)) ||
      (r = upload(h->sym_n0, sdn0)) || (r = upload(h->cls_inv, cls_inv)))
    return r;
  if ((r = h->ofdm.init(pp, layout.cmap, fp.aux_len, 1))) return r;
  if ((r = h->l1.init(fp))) return r;
  h->l1_stride = (uint32_t)((fp.Lp + 3) & ~3);
  if ((r = upload(h->abin, al.dbin)) || (r = upload(h->aval, al.dval)) || (r = upload(h->aind, al.ind)) ||
      (r = upload(h->agrp, al.grp)) || (r = upload(h->azr, t.zr)))
    return r;
  OfdmDev &od = h->ofdm.dev;
  od.abin = h->abin.as<uint16_t>();
  od.aval = h->aval.as<float2>();
  od.aind = h->aind.as<uint32_t>();
  od.agrp = h->agrp.as<int4>();
  od.azr = h->azr.as<int2>();
  od.inv = h->inv.as<uint16_t>();
  od.sym_d0 = h->sym_d0.as<int32_t>();
  od.sym_n = h->sym_n.as<int32_t>();
  od.sym_n0 = h->sym_n0.as<int32_t>();
  od.ncls = fp.ncls;
  od.cls_inv = h->cls_inv.as<int32_t>();
  od.nplp = h->nplp;
  if (h->nplp == 1) {
    od.qam = h->plps[0]->map.dev.lut;   // the 256-entry table (entries past the constellation are zero)
    od.nq = 256;
  } else {
    if (nq > OFDM_MAX_QAM) return DVBT2LL_EINVAL;
    h->plp_bnd_host = layout.plp_bnd;   // class 0's (the debug hook's frame 0)
    std::vector<int32_t> qb(h->qbase_host.begin(), h->qbase_host.end());
    if ((r = upload(h->qam_all, qall)) || (r = upload(h->plp_bnd, bnd_all)) || (r = upload(h->plp_qbase, qb)))
      return r;
    od.qam = h->qam_all.as<float2>();
    od.nq = nq;
    od.plp_bnd = h->plp_bnd.as<int32_t>();
    od.plp_qbase = h->plp_qbase.as<int32_t>();
  }
  if (h->pair && (r = chain_build_group2(h, pg, layouts, cls_inv, auxv))) return r;
  h->iq_per_frame = (int64_t)pp.Nsym * (pp.N + pp.G) + 2048;
  // the OFDM kernel addresses index pairs and aux cells with 32-bit byte offsets
  if ((uint64_t)h->pair_stride * h->max_frames * 2 >= (1ull << 32) || auxv.size() * 8 >= (1ull << 32) ||
      (uint64_t)h->l1_stride * h->max_frames * 8 >= (1ull << 32))
    return DVBT2LL_EINVAL;
  if ((r = h->alloc_slot(0))) return r;
  if ((r = upload(h->aux, auxv))) return r;
  if (h->sync_err.ensure(4) || h->bbh_err.ensure(4)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemset(h->sync_err.p, 0, 4));
  HIP_TRY(hipMemset(h->bbh_err.p, 0, 4));
  return 0;
}

// pair: a MISO pair handle (both transmitter groups): misogroup MISO_TX1 and a MISO preamble (dvbt2_preamble_t
// T2_MISO = 1, T2_LITE_MISO = 4; the planner's own test, t2_plan.cpp build_pilot), checked before anything is built
static bool pair_params_ok(int misogroup, int preamble) { return misogroup == 0 && (preamble == 1 || preamble == 4); }
static int chain_create(const dvbt2ll_chain_params *p, int device, dvbt2ll_chain **out, bool pair) {
  if (!p || !out || p->max_frames < 1) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (pair && !pair_params_ok(p->misogroup, p->fm.preamble)) return DVBT2LL_EINVAL;
  const dvbt2ll_framemapperfint_params &f = p->fm;
  std::unique_ptr<dvbt2ll_chain> h(new (std::nothrow) dvbt2ll_chain());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  h->pair = pair;
  h->max_frames = p->max_frames;
  const PlpParams one{f.framesize, f.rate, f.constellation, f.rotation, f.fecblocks, f.tiblocks, f.inputmode, f.inband};
  int r = chain_build(h.get(), to_fm(f), {one}, {p->tsrate}, p->misogroup, p->equalization, p->bandwidth, device);
  if (r) return r;
  *out = h.release();
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_create(const dvbt2ll_chain_params *p, int device, dvbt2ll_chain **out) {
  return chain_create(p, device, out, false);
}
extern "C" int dvbt2ll_chain_create_miso_pair(const dvbt2ll_chain_params *p, int device, dvbt2ll_chain **out) {
  return chain_create(p, device, out, true);
}

static int chain_create_mplp(const dvbt2ll_mplp_chain_params *p, int device, dvbt2ll_chain **out, bool pair) {
  if (!p || !out || p->max_frames < 1) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (pair && !pair_params_ok(p->misogroup, p->fm.preamble)) return DVBT2LL_EINVAL;
  FmParams fm;
  std::vector<PlpParams> plps;
  std::vector<int> tsrate;
  int nss = 1;
  if (!mplp_to_plan(p->fm, fm, plps, tsrate, &nss)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_chain> h(new (std::nothrow) dvbt2ll_chain());
  if (!h) return DVBT2LL_ENOMEM;
  h->pair = pair;
  h->max_frames = p->max_frames;
  const dvbt2ll_plp_params &q0 = p->fm.plp[0];
  h->p.fm = dvbt2ll_framemapperfint_params{q0.framesize, q0.rate, q0.constellation, q0.rotation, q0.fecblocks,
                                           q0.tiblocks, fm.carriermode, fm.fftsize, fm.guardinterval,
                                           fm.l1constellation, fm.pilotpattern, fm.t2frames, fm.numdatasyms,
                                           fm.paprmode, fm.version, fm.preamble, q0.inputmode, fm.reservedbiasbits,
                                           fm.l1scrambled, q0.inband};
  h->p.misogroup = p->misogroup;
  h->p.equalization = p->equalization;
  h->p.bandwidth = p->bandwidth;
  h->p.max_frames = p->max_frames;
  h->p.tsrate = q0.tsrate;
  int r = chain_build(h.get(), fm, plps, tsrate, p->misogroup, p->equalization, p->bandwidth, device, nss);
  if (r) return r;
  *out = h.release();
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_create_mplp(const dvbt2ll_mplp_chain_params *p, int device, dvbt2ll_chain **out) {
  return chain_create_mplp(p, device, out, false);
}
extern "C" int dvbt2ll_chain_create_mplp_miso_pair(const dvbt2ll_mplp_chain_params *p, int device,
                                                   dvbt2ll_chain **out) {
  return chain_create_mplp(p, device, out, true);
}
extern "C" int dvbt2ll_chain_num_groups(const dvbt2ll_chain *h) { return h ? (h->pair ? 2 : 1) : 0; }

extern "C" int dvbt2ll_chain_unit_frames(const dvbt2ll_chain *h) { return h ? h->frame.unit : 0; }

extern "C" int dvbt2ll_chain_num_plps(const dvbt2ll_chain *h) { return h ? h->nplp : 0; }

extern "C" int dvbt2ll_chain_get_plp_info(const dvbt2ll_chain *h, int plp, dvbt2ll_chain_info *info) {
  if (!h || !info || plp < 0 || plp >= h->nplp) return DVBT2LL_EINVAL;
  const ChainPlp &pl = *h->plps[plp];
  info->fec_blocks_per_frame = pl.F;
  info->payload_bytes_per_block = pl.pay;
  info->ts_bytes_per_frame = pl.inputmode ? (pl.ts_per_frame * 188 + 186) / 187 : pl.ts_per_frame;
  if (pl.input == DVBT2LL_INPUT_BBFRAME) {   // whole BBFRAMEs, header included
    info->payload_bytes_per_block = (int)pl.bbf_len();
    info->ts_bytes_per_frame = pl.F * pl.bbf_len();
  }
  info->iq_samples_per_frame = h->iq_per_frame;
  info->cell_size = h->frame.plp[plp].cs;
  info->stream_items = h->frame.plp[plp].S;
  info->mapped_items = h->frame.M;
  info->num_symbols = h->pilot.Nsym;
  info->fft_size = h->pilot.N;
  info->guard_interval = h->pilot.G;
  info->cw_stride_bytes = pl.cw_stride;
  info->frames_per_if = pl.cyc;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_get_info(const dvbt2ll_chain *h, dvbt2ll_chain_info *info) {
  int r = dvbt2ll_chain_get_plp_info(h, 0, info);
  if (r) return r;
  info->stream_items = h->frame.S;   // the frame's data cells (every PLP)
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_run_device(dvbt2ll_chain *h, const void *ts_dev, int64_t ts_base, int64_t ts_len,
                                        int64_t first_frame, int nframes, void *iq_dev, void *stream) {
  return dvbt2ll_chain_run_streams(h, ts_dev, 0, 1, ts_base, ts_len, first_frame, nframes, iq_dev, stream);
}

// stream bytes [lo, end) that frames [first, first + n) of PLP pl consume: their payload plus the packet before
// the first one touched (its CRC-8 replaces the next sync byte, bbheader:701-713).  BBFRAME input: exactly the
// frames' BBFRAMEs, no byte before them
static void ts_span(const ChainPlp &pl, int64_t first, int64_t n, int64_t *lo, int64_t *end) {
  if (pl.input == DVBT2LL_INPUT_BBFRAME) {
    *lo = first / pl.cyc * pl.F * pl.bbf_len();
    *end = (first + n) / pl.cyc * pl.F * pl.bbf_len();
    return;
  }
  int64_t start = first / pl.cyc * pl.ts_per_frame, e = (first + n) / pl.cyc * pl.ts_per_frame;
  if (pl.inputmode) {
    start = 188 * (start / 187) + (start % 187);
    e = 188 * (e / 187) + (e % 187) + 1;
  }
  *lo = start >= 188 ? (start / 188) * 188 - 188 : 0;
  *end = e;
}

// BBFRAME input from host memory: the span [lo, end) of the frames' BBFRAMEs (the host paths copy exactly those
// bytes), nonzero when the caller's [base, base + len) does not hold it or base is no BBFRAME boundary
static int bbf_host_span(const ChainPlp &pl, int64_t base, int64_t len, int64_t first, int64_t n, int64_t *lo,
                         int64_t *end) {
  if (first < 0 || n < 1 || base < 0 || len < 0 || base % pl.base_unit()) return DVBT2LL_EINVAL;
  ts_span(pl, first, n, lo, end);
  return base > *lo || base + len < *end ? DVBT2LL_EINVAL : 0;
}

// one run over nstreams independent single-PLP streams (nplp == 1) or over one frame sequence of
// every PLP (nstreams == 1): ts[k], base[k], len[k] per PLP (stream s of a batch at ts[0] + s * ts_stride)
// A pair handle (groups: the *_groups calls) writes group 1's IQ to iq_dev and group 2's to iq2_dev, either of which
// may be null; an ordinary handle takes iq_dev alone.
static int chain_run(dvbt2ll_chain *h, const void *const *ts, const int64_t *base, const int64_t *len,
                     int64_t ts_stride, int nstreams, int64_t first_frame, int nframes, void *iq_dev, void *stream,
                     bool groups = false, void *iq2_dev = nullptr) {
  if (!h || !ts || h->pair != groups || (!iq_dev && !iq2_dev) || (!groups && !iq_dev) || nframes < 1 || nstreams < 1 ||
      (int64_t)nframes * nstreams > h->max_frames || first_frame < 0 ||
      (nstreams > 1 && (h->nplp > 1 || ts_stride < len[0])) || (groups && h->use_graph))
    return DVBT2LL_EINVAL;
  // iq_dev is aligned to one output sample (the IQ stores are whole samples, or pairs where the address allows)
  const unsigned iq_align = h->ofdm.dev.fmt == DVBT2LL_IQ_SC16 ? 4u : 8u;
  if ((uintptr_t)iq_dev % iq_align || (uintptr_t)iq2_dev % iq_align) return DVBT2LL_EINVAL;
  // whole interleaving frames of every PLP (TIME_IL_TYPE 1: P_I T2 frames each)
  if (first_frame % h->frame.unit || nframes % h->frame.unit) return DVBT2LL_EINVAL;
  const int nf = nframes * nstreams;   // frames of the launch, stream-major
  hipStream_t s = stream ? (hipStream_t)stream : h->ctx.stream;
  for (int k = 0; k < h->nplp; k++) {
    const ChainPlp &pl = *h->plps[k];
    if (!ts[k] || base[k] < 0 || base[k] % pl.base_unit() != 0) return DVBT2LL_EINVAL;
    // the TS slice must cover every byte the frames consume plus the packet before the first one touched (BBFRAME
    // input: the frames' BBFRAMEs)
    int64_t lo, end;
    ts_span(pl, first_frame, nframes, &lo, &end);
    if (base[k] > lo || base[k] + len[k] < end) return DVBT2LL_EINVAL;
  }
  HIP_TRY(hipSetDevice(h->ctx.device));
  const int slot = h->next_slot;
  if (h->slot_used[slot] && h->slot_stream[slot] != s) HIP_TRY(hipStreamWaitEvent(s, h->slot_done[slot], 0));
  DevBuf &pairs = h->pairs[slot];
  if (h->bpart_dirty[slot]) {
    for (auto &pl : h->plps) HIP_TRY(hipMemsetAsync(pl->bpart[slot].p, 0, pl->bpart[slot].n, s));
    h->bpart_dirty[slot] = false;
  }
  hipEvent_t ev[dvbt2ll_chain::NEV] = {};
  if (h->timing && !h->use_graph) {   // per-stage events only on the direct launch path
    if (h->evused + dvbt2ll_chain::NEV > 4096 && h->fold_timing()) return DVBT2LL_EDEVICE;
    for (auto &e : ev)
      if (!(e = h->next_event())) return DVBT2LL_EDEVICE;
    HIP_TRY(hipEventRecord(ev[0], s));
  }
  L1IO lio{};
  FecIO fio[DVBT2LL_MAX_PLP] = {};
  MapIO mio[DVBT2LL_MAX_PLP] = {};
  OfdmIO oio{};
  lio.out = h->l1buf[slot].as<float2>();
  lio.out_stride = h->l1_stride;
  lio.first_frame = first_frame;
  lio.nframes = nf;
  lio.frames_per_stream = nstreams > 1 ? nframes : 0;
  for (int k = 0; k < h->nplp; k++) {
    ChainPlp &pl = *h->plps[k];
    DevBuf &cw = pl.cw[slot];
    fio[k].in = (const uint8_t *)ts[k];
    fio[k].ts_base = base[k];
    fio[k].ts_len = len[k];
    // launch block b: FEC block b mod F of interleaving frame b / F, which fills T2 frames P (b / F) ..
    // P (b / F) + P - 1 of the launch (pairs at P pair_stride per interleaving frame)
    fio[k].first_block = first_frame / pl.cyc * pl.F;
    fio[k].out = cw.as<uint8_t>();
    fio[k].cw_stride = pl.cw_stride;
    fio[k].nblocks = (int)pl.blocks(nf);
    fio[k].sync_err = h->sync_err.as<uint32_t>();
    fio[k].bbh_err = h->bbh_err.as<uint32_t>();
    fio[k].blocks_per_stream = nstreams > 1 ? (int)pl.blocks(nframes) : 0;
    fio[k].ts_stride = nstreams > 1 ? ts_stride : 0;
    fio[k].bch_part = pl.bpart[slot].as<uint32_t>();
    fio[k].bch_part_blocks = pl.blocks(h->max_frames);
    fio[k].keep_cw = h->keep_cw;
    mio[k].out_pairs = pairs.as<uint16_t>();
    mio[k].frame_stride = h->pair_stride * h->frame.unit;
    mio[k].nblocks = (int)pl.blocks(nf);
  }
  oio.data = h->aux.as<float2>();
  oio.aux_off = 0;
  oio.cell_off = 0;
  oio.cell_stride = (uint32_t)h->pair_stride;
  oio.pairs = pairs.as<uint16_t>();
  oio.out = (float2 *)iq_dev;
  oio.out_stride = h->iq_per_frame;
  oio.first_frame = first_frame;
  oio.nframes = nf;
  oio.frames_per_stream = nstreams > 1 ? nframes : 0;
  oio.l1 = h->l1buf[slot].as<float2>();
  oio.l1_stride = h->l1_stride;
  OfdmIO oio2 = oio;   // a pair handle's group 2: the same pairs and L1-post cells into its own IQ buffer
  oio2.out = (float2 *)iq2_dev;
  if (h->use_graph) {
    int r = h->graph_launch(lio, fio, mio, oio, nf, slot, s);
    if (r) {
      h->bpart_dirty[slot] = true;
      return r;
    }
  } else {
    const hipError_t e = h->launch_chain(lio, fio, mio, oio, s, ev[1], ev[2], groups ? &oio2 : nullptr);
    if (e != hipSuccess) {
      h->bpart_dirty[slot] = true;
      HIP_TRY(e);
    }
    if (h->timing) HIP_TRY(hipEventRecord(ev[3], s));
  }
  HIP_TRY(hipEventRecord(h->slot_done[slot], s));
  h->slot_used[slot] = true;
  h->slot_stream[slot] = s;
  h->cw_kept[slot] = h->keep_cw;
  h->last_slot = slot;
  h->next_slot = (slot + 1) % h->nslots;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_run_streams(dvbt2ll_chain *h, const void *ts_dev, int64_t ts_stride, int nstreams,
                                         int64_t ts_base, int64_t ts_len, int64_t first_frame, int nframes,
                                         void *iq_dev, void *stream) {
  if (!h || h->nplp != 1) return DVBT2LL_EINVAL;
  const void *ts[1] = {ts_dev};
  return chain_run(h, ts, &ts_base, &ts_len, ts_stride, nstreams, first_frame, nframes, iq_dev, stream);
}

extern "C" int dvbt2ll_chain_run_plps(dvbt2ll_chain *h, const void *const *ts_dev, const int64_t *ts_base,
                                      const int64_t *ts_len, int64_t first_frame, int nframes, void *iq_dev,
                                      void *stream) {
  if (!h || !ts_dev || !ts_base || !ts_len) return DVBT2LL_EINVAL;
  return chain_run(h, ts_dev, ts_base, ts_len, 0, 1, first_frame, nframes, iq_dev, stream);
}

extern "C" int dvbt2ll_chain_run_groups(dvbt2ll_chain *h, const void *ts_dev, int64_t ts_stride, int nstreams,
                                        int64_t ts_base, int64_t ts_len, int64_t first_frame, int nframes,
                                        void *const iq_dev[2], void *stream) {
  if (!h || h->nplp != 1 || !iq_dev) return DVBT2LL_EINVAL;
  const void *ts[1] = {ts_dev};
  return chain_run(h, ts, &ts_base, &ts_len, ts_stride, nstreams, first_frame, nframes, iq_dev[0], stream, true,
                   iq_dev[1]);
}

extern "C" int dvbt2ll_chain_run_plps_groups(dvbt2ll_chain *h, const void *const *ts_dev, const int64_t *ts_base,
                                             const int64_t *ts_len, int64_t first_frame, int nframes,
                                             void *const iq_dev[2], void *stream) {
  if (!h || !ts_dev || !ts_base || !ts_len || !iq_dev) return DVBT2LL_EINVAL;
  return chain_run(h, ts_dev, ts_base, ts_len, 0, 1, first_frame, nframes, iq_dev[0], stream, true, iq_dev[1]);
}

extern "C" int dvbt2ll_chain_set_graph(dvbt2ll_chain *h, int enable) {
  if (!h || (h->pair && enable)) return DVBT2LL_EINVAL;   // graph mode: not for pair handles
  h->use_graph = enable != 0;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_set_slots(dvbt2ll_chain *h, int nslots) {
  if (!h || nslots < 1 || nslots > DVBT2LL_CHAIN_MAX_SLOTS) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HIP_TRY(hipDeviceSynchronize());   // no run in flight while slots change
  for (int k = 0; k < nslots; k++) {
    int r = h->alloc_slot(k);
    if (r) return r;
  }
  for (int k = nslots; k < DVBT2LL_CHAIN_MAX_SLOTS; k++) {
    for (auto &pl : h->plps) {
      pl->cw[k].release();
      pl->bpart[k].release();
    }
    h->pairs[k].release();
    h->l1buf[k].release();
    h->slot_used[k] = false;
  }
  h->nslots = nslots;
  h->next_slot = 0;
  if (h->last_slot >= nslots) h->last_slot = 0;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_run_host(dvbt2ll_chain *h, const void *ts, int64_t ts_base, int64_t ts_len,
                                      int64_t first_frame, int nframes, void *iq) {
  if (!h || !ts || !iq || nframes < 1 || nframes > h->max_frames || h->nplp != 1 || h->pair) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  size_t iq_bytes = (size_t)nframes * h->iq_per_frame * (h->ofdm.dev.fmt == DVBT2LL_IQ_SC16 ? 4 : 8);
  if (h->plps[0]->input == DVBT2LL_INPUT_BBFRAME) {   // exactly the frames' BBFRAMEs go to the device
    int64_t lo, end;
    if (bbf_host_span(*h->plps[0], ts_base, ts_len, first_frame, nframes, &lo, &end)) return DVBT2LL_EINVAL;
    ts = (const uint8_t *)ts + (lo - ts_base);
    ts_base = lo;
    ts_len = end - lo;
  }
  if (h->ts_tmp.ensure((size_t)ts_len + 16) || h->iq_tmp.ensure(iq_bytes)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpyAsync(h->ts_tmp.p, ts, (size_t)ts_len, hipMemcpyHostToDevice, h->ctx.stream));
  int r = dvbt2ll_chain_run_device(h, h->ts_tmp.p, ts_base, ts_len, first_frame, nframes, h->iq_tmp.p, nullptr);
  if (r) return r;
  HIP_TRY(hipMemcpyAsync(iq, h->iq_tmp.p, iq_bytes, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_run_plps_host(dvbt2ll_chain *h, const void *const *ts, const int64_t *ts_base,
                                           const int64_t *ts_len, int64_t first_frame, int nframes, void *iq) {
  if (!h || !ts || !ts_base || !ts_len || !iq || nframes < 1 || nframes > h->max_frames || h->pair)
    return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  const void *dev[DVBT2LL_MAX_PLP];
  int64_t base[DVBT2LL_MAX_PLP], len[DVBT2LL_MAX_PLP];
  for (int k = 0; k < h->nplp; k++) {
    if (!ts[k] || ts_len[k] < 0) return DVBT2LL_EINVAL;
    const uint8_t *src = (const uint8_t *)ts[k];
    base[k] = ts_base[k];
    len[k] = ts_len[k];
    if (h->plps[k]->input == DVBT2LL_INPUT_BBFRAME) {   // exactly the frames' BBFRAMEs go to the device
      int64_t lo, end;
      if (bbf_host_span(*h->plps[k], ts_base[k], ts_len[k], first_frame, nframes, &lo, &end)) return DVBT2LL_EINVAL;
      src += lo - ts_base[k];
      base[k] = lo;
      len[k] = end - lo;
    }
    if (h->ts_plp_tmp[k].ensure((size_t)len[k] + 16)) return DVBT2LL_ENOMEM;
    HIP_TRY(hipMemcpyAsync(h->ts_plp_tmp[k].p, src, (size_t)len[k], hipMemcpyHostToDevice, h->ctx.stream));
    dev[k] = h->ts_plp_tmp[k].p;
  }
  const size_t iq_bytes = (size_t)nframes * h->iq_per_frame * (h->ofdm.dev.fmt == DVBT2LL_IQ_SC16 ? 4 : 8);
  if (h->iq_tmp.ensure(iq_bytes)) return DVBT2LL_ENOMEM;
  int r = dvbt2ll_chain_run_plps(h, dev, base, len, first_frame, nframes, h->iq_tmp.p, nullptr);
  if (r) return r;
  HIP_TRY(hipMemcpyAsync(iq, h->iq_tmp.p, iq_bytes, hipMemcpyDeviceToHost, h->ctx.stream));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_host_submit(dvbt2ll_chain *h, const void *ts, int64_t ts_base, int64_t ts_len,
                                         int64_t first_frame, int nframes, void *iq, int64_t *ticket) {
  // every argument check precedes the first asynchronous operation, so a refused submission leaves no copy
  // of the caller's buffers in flight (the unit check is repeated by chain_run, after the copy-in is queued)
  if (!h || !ts || !iq || !ticket || h->nplp != 1 || h->pair || nframes < 1 || nframes > h->max_frames || first_frame < 0 ||
      ts_base < 0 || ts_base % h->plps[0]->base_unit() || first_frame % h->frame.unit || nframes % h->frame.unit)
    return DVBT2LL_EINVAL;
  const ChainPlp &pl = *h->plps[0];
  int64_t lo, end;
  ts_span(pl, first_frame, nframes, &lo, &end);
  if (ts_base > lo || ts_base + ts_len < end) return DVBT2LL_EINVAL;
  int r = h->host.init(h->ctx.device);
  if (r) return r;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HostRing &R = h->host;
  const int64_t t = R.next_ticket;
  HostRing::Entry &x = R.e[t % DVBT2LL_HOST_RING];
  // the entry's previous submission must have left its buffers: its copy-out is the last thing it does
  if (x.ticket >= 0) HIP_TRY(hipEventSynchronize(x.d2h));
  const size_t iq_bytes = (size_t)nframes * h->iq_per_frame * (h->ofdm.dev.fmt == DVBT2LL_IQ_SC16 ? 4 : 8);
  if (x.ts.ensure((size_t)(end - lo) + 16) || x.iq.ensure(iq_bytes)) return DVBT2LL_ENOMEM;
  HIP_TRY(hipMemcpyAsync(x.ts.p, (const uint8_t *)ts + (lo - ts_base), (size_t)(end - lo), hipMemcpyHostToDevice,
                         R.in));
  HIP_TRY(hipEventRecord(x.h2d, R.in));
  HIP_TRY(hipStreamWaitEvent(R.comp, x.h2d, 0));
  if ((r = dvbt2ll_chain_run_device(h, x.ts.p, lo, end - lo, first_frame, nframes, x.iq.p, R.comp))) {
    // unreachable after the checks above unless the device fails; the copy-in must still end before the
    // caller may reuse ts
    (void)hipStreamSynchronize(R.in);
    return r;
  }
  HIP_TRY(hipEventRecord(x.kern, R.comp));
  HIP_TRY(hipStreamWaitEvent(R.out, x.kern, 0));
  HIP_TRY(hipMemcpyAsync(iq, x.iq.p, iq_bytes, hipMemcpyDeviceToHost, R.out));
  HIP_TRY(hipEventRecord(x.d2h, R.out));
  x.ticket = t;
  R.next_ticket = t + 1;
  *ticket = t;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_host_wait(dvbt2ll_chain *h, int64_t ticket) {
  if (!h || ticket < 0 || ticket >= h->host.next_ticket) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  const HostRing::Entry &x = h->host.e[ticket % DVBT2LL_HOST_RING];
  // an entry reused by a later submission was waited for at that submission
  if (x.ticket == ticket) HIP_TRY(hipEventSynchronize(x.d2h));
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_run_host_pipelined(dvbt2ll_chain *h, const void *ts, int64_t ts_base, int64_t ts_len,
                                                int64_t first_frame, int nframes, void *iq, int chunk_frames) {
  if (!h || !ts || !iq || nframes < 1 || chunk_frames < 0 || h->nplp != 1 || h->pair) return DVBT2LL_EINVAL;
  const int U = h->frame.unit;
  // chunks of whole launch units; every chunk is checked before the first one is submitted
  int c = chunk_frames ? std::min(chunk_frames, h->max_frames) : h->max_frames;
  c -= c % U;
  if (c < U || first_frame < 0 || first_frame % U || nframes % U || ts_base < 0 || ts_base % h->plps[0]->base_unit())
    return DVBT2LL_EINVAL;
  {
    int64_t lo, end;
    ts_span(*h->plps[0], first_frame, nframes, &lo, &end);   // the union of the chunks' spans
    if (ts_base > lo || ts_base + ts_len < end) return DVBT2LL_EINVAL;
  }
  const size_t per = (size_t)h->iq_per_frame * (h->ofdm.dev.fmt == DVBT2LL_IQ_SC16 ? 4 : 8);
  int64_t t = -1;
  for (int f = 0; f < nframes; f += c) {
    const int n = std::min(c, nframes - f);
    int r = dvbt2ll_chain_host_submit(h, ts, ts_base, ts_len, first_frame + f, n, (char *)iq + (size_t)f * per, &t);
    if (r) {
      // the chunks already submitted still copy into iq: drain them before the caller sees the error
      if (t >= 0) (void)dvbt2ll_chain_host_wait(h, t);
      return r;
    }
  }
  return dvbt2ll_chain_host_wait(h, t);
}

// page-aligned heap memory, page-locked by hipHostRegister (the copies then run at the PCIe rate, as from
// hipHostMalloc memory; the buffer stays ordinary heap memory, which the host sanitizer build tracks)
extern "C" void *dvbt2ll_host_alloc(size_t bytes) {
  const size_t n = ((bytes ? bytes : 1) + 4095) & ~(size_t)4095;
  void *p = nullptr;
  if (posix_memalign(&p, 4096, n)) return nullptr;
  if (hipHostRegister(p, n, hipHostRegisterDefault) != hipSuccess) {
    std::free(p);
    return nullptr;
  }
  return p;
}
extern "C" void dvbt2ll_host_free(void *p) {
  if (!p) return;
  (void)hipHostUnregister(p);
  std::free(p);
}

extern "C" int dvbt2ll_chain_set_output(dvbt2ll_chain *h, float gain, int format) {
  if (!h || !(gain == gain) || (format != DVBT2LL_IQ_CF32 && format != DVBT2LL_IQ_SC16)) return DVBT2LL_EINVAL;
  h->ofdm.dev.gain = gain;
  h->ofdm.dev.fmt = format;
  h->ofdm2.dev.gain = gain;   // (a pair handle's group 2)
  h->ofdm2.dev.fmt = format;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_set_input(dvbt2ll_chain *h, int plp, int format) {
  if (!h || plp < -1 || plp >= h->nplp || (format != DVBT2LL_INPUT_TS && format != DVBT2LL_INPUT_BBFRAME))
    return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HIP_TRY(hipDeviceSynchronize());   // no run in flight while the format changes
  for (int k = 0; k < h->nplp; k++) {
    if (plp >= 0 && k != plp) continue;
    h->plps[k]->input = format;
    h->plps[k]->fec.dev.input = format == DVBT2LL_INPUT_BBFRAME ? FEC_INPUT_BBFRAME : FEC_INPUT_TS;
  }
  // the instantiated graphs hold the other format's kernel in their first nodes: the next graph run captures anew
  h->graphs.clear();
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_get_input(const dvbt2ll_chain *h, int plp) {
  if (!h || plp < 0 || plp >= h->nplp) return DVBT2LL_EINVAL;
  return h->plps[plp]->input;
}
extern "C" int dvbt2ll_chain_bbheader_errors(dvbt2ll_chain *h, int64_t *count) {
  if (!h || !count) return DVBT2LL_EINVAL;
  uint32_t v = 0;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&v, h->bbh_err.p, 4, hipMemcpyDeviceToHost));
  *count = (int64_t)v;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_chain_set_timing(dvbt2ll_chain *h, int enable) {
  if (!h) return DVBT2LL_EINVAL;
  if (h->fold_timing()) return DVBT2LL_EDEVICE;
  h->timing = enable != 0;
  for (int k = 0; k < 4; k++) { h->ms[k] = 0; h->launches[k] = 0; }
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_get_timing(dvbt2ll_chain *h, double *ms, int64_t *launches, int nstages) {
  if (!h || !ms || nstages < 1) return DVBT2LL_EINVAL;
  if (h->fold_timing()) return DVBT2LL_EDEVICE;
  for (int k = 0; k < nstages && k < 4; k++) {
    ms[k] = h->ms[k];
    if (launches) launches[k] = h->launches[k];
  }
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_debug_plp_codewords(dvbt2ll_chain *h, int plp, void *out, int64_t bytes) {
  if (!h || !out || bytes < 0 || plp < 0 || plp >= h->nplp) return DVBT2LL_EINVAL;
  const DevBuf &cw = h->plps[plp]->cw[h->last_slot];
  if ((size_t)bytes > cw.n || !h->cw_kept[h->last_slot]) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, cw.p, (size_t)bytes, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_debug_keep_codewords(dvbt2ll_chain *h, int enable) {
  if (!h) return DVBT2LL_EINVAL;
  h->keep_cw = enable != 0;
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_debug_codewords(dvbt2ll_chain *h, void *out, int64_t bytes) {
  return dvbt2ll_chain_debug_plp_codewords(h, 0, out, bytes);
}
extern "C" int dvbt2ll_chain_debug_cell_pairs(dvbt2ll_chain *h, void *out, int64_t cells) {
  if (!h || !out || cells < 0 || (size_t)cells * 2 > h->pairs[h->last_slot].n) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, h->pairs[h->last_slot].p, (size_t)cells * 2, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_debug_cells(dvbt2ll_chain *h, void *out, int64_t cells) {
  // frame 0's data cells: index pairs expanded through the constellation exactly as the OFDM
  // kernel does, (lut[lo].re, lut[hi].im) with the table of the slot's PLP
  if (!h || !out || cells < 0 || (size_t)cells * 2 > h->pairs[h->last_slot].n) return DVBT2LL_EINVAL;
  std::vector<uint16_t> pr((size_t)cells);
  int r = dvbt2ll_chain_debug_cell_pairs(h, pr.data(), cells);
  if (r) return r;
  cf32 *o = (cf32 *)out;
  std::vector<int> plp_of((size_t)cells, 0);
  if (h->nplp > 1) {
    const int P = h->nplp;
    for (size_t g = 0; g + 1 <= h->plp_bnd_host.size() / (P + 1); g++)
      for (int k = 0; k < P; k++)
        for (int32_t s = h->plp_bnd_host[g * (P + 1) + k]; s < h->plp_bnd_host[g * (P + 1) + k + 1]; s++)
          if (s < cells) plp_of[s] = k;
  }
  for (int64_t i = 0; i < cells; i++) {
    const cf32 *lut = h->plps[plp_of[i]]->map.plan.lut;
    o[i] = cf32{lut[pr[i] & 0xFF].re, lut[pr[i] >> 8].im};
  }
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_sync_errors(dvbt2ll_chain *h, int64_t *count) {
  if (!h || !count) return DVBT2LL_EINVAL;
  uint32_t v = 0;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(&v, h->sync_err.p, 4, hipMemcpyDeviceToHost));
  *count = (int64_t)v;
  return DVBT2LL_OK;
}
extern "C" int dvbt2ll_chain_synchronize(dvbt2ll_chain *h) {
  if (!h) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  HIP_TRY(hipStreamSynchronize(h->ctx.stream));
  // the streaming host path's three streams (dvbt2ll_chain_host_submit) and the slots' last runs on
  // caller streams
  HIP_TRY(h->host.synchronize());
  for (int k = 0; k < DVBT2LL_CHAIN_MAX_SLOTS; k++)
    if (h->slot_used[k] && h->slot_done[k]) HIP_TRY(hipEventSynchronize(h->slot_done[k]));
  return DVBT2LL_OK;
}
extern "C" void dvbt2ll_chain_destroy(dvbt2ll_chain *h) { delete h; }

// ============================================================================ T2-MI input
// A handle beside the chain: its scratch (sized at create from max_ts_bytes and max_packets), no stream state.  All
// passes of a run go to the caller's stream (t2mi_kernels.hip); the result stays on the device until get_result.
struct dvbt2ll_t2mi {
  DeviceCtx ctx;
  dvbt2ll_t2mi_params p{};
  T2miDev dev;
  DevBuf scratch, ts_tmp, out_tmp[DVBT2LL_MAX_PLP];
  hipEvent_t done = nullptr;     // the last run; a run on another stream waits for it (the scratch is shared)
  hipStream_t last = nullptr;
  bool ran = false;
  ~dvbt2ll_t2mi() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
};

static bool t2mi_valid_len(int L) {
  static const int kbch[14] = {32208, 38688, 43040, 48408, 51648, 53840, 7032, 9552, 10632, 11712, 12432, 13152,
                               5232, 6312};   // the codes of build_fec (t2_plan.cpp fec_numbers)
  for (int k : kbch)
    if (L == k / 8) return true;
  return false;
}

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
  std::unique_ptr<dvbt2ll_t2mi> h(new (std::nothrow) dvbt2ll_t2mi());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  int r = h->ctx.init(device);
  if (r) return r;
  T2miDev &d = h->dev;
  d.pid = p->pid;
  d.stream_id = p->stream_id;
  d.nplp = p->nplp;
  for (int k = 0; k < p->nplp; k++) { d.plp_id[k] = p->plp_id[k]; d.L[k] = p->bbframe_bytes[k]; }
  d.max_ts = (uint32_t)(p->max_ts_bytes / 188);
  d.max_packets = (uint32_t)p->max_packets;
  if (h->scratch.ensure(t2mi_layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)t2mi_layout(d, h->scratch.p);
  std::vector<uint32_t> tab(T2MI_TAB_WORDS);
  t2mi_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, T2MI_R_WORDS * 8));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_params_from_chain(const dvbt2ll_chain *chain, const int *plp_ids, dvbt2ll_t2mi_params *p) {
  if (!chain || !p || chain->nplp < 1 || chain->nplp > DVBT2LL_MAX_PLP) return DVBT2LL_EINVAL;
  p->nplp = chain->nplp;
  for (int k = 0; k < chain->nplp; k++) {
    p->plp_id[k] = plp_ids ? plp_ids[k] : k;
    p->bbframe_bytes[k] = (int)chain->plps[k]->bbf_len();
  }
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
  int e = t2mi_run_args(h, ts_dev, ts_len, start, out_dev, out_cap_blocks, r);
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  HIP_TRY(t2mi_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->last = st;
  h->ran = true;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_get_result(dvbt2ll_t2mi *h, dvbt2ll_t2mi_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  std::vector<uint64_t> w(T2MI_R_WORDS);
  HIP_TRY(hipMemcpy(w.data(), h->dev.res, w.size() * 8, hipMemcpyDeviceToHost));
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
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
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
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  if (h->ts_tmp.ensure((size_t)std::max<int64_t>(ts_len, 1))) return DVBT2LL_ENOMEM;
  void *od[DVBT2LL_MAX_PLP] = {};
  for (int k = 0; k < h->p.nplp; k++) {
    if (h->out_tmp[k].ensure((size_t)r.cap[k] * h->p.bbframe_bytes[k] + 16)) return DVBT2LL_ENOMEM;
    od[k] = h->out_tmp[k].p;
  }
  if (ts_len) HIP_TRY(hipMemcpyAsync(h->ts_tmp.p, ts, (size_t)ts_len, hipMemcpyHostToDevice, h->ctx.stream));
  if ((e = dvbt2ll_t2mi_run_device(h, h->ts_tmp.p, ts_len, start, od, out_cap_blocks, h->ctx.stream))) return e;
  if ((e = dvbt2ll_t2mi_get_result(h, res))) return e;
  for (int k = 0; k < h->p.nplp; k++)
    if (res->blocks[k] > 0)
      HIP_TRY(hipMemcpy(out[k], od[k], (size_t)res->blocks[k] * h->p.bbframe_bytes[k], hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_t2mi_destroy(dvbt2ll_t2mi *h) { delete h; }

// ============================================================================ mode adapter
// A handle beside the chain, built like the T2-MI one: scratch sized at create from max_ts_bytes, no stream state, all
// passes of a run on the caller's stream (modeadapt_kernels.hip), the result on the device until get_result.
struct dvbt2ll_modeadapt {
  DeviceCtx ctx;
  dvbt2ll_modeadapt_params p{};
  MaDev dev;
  DevBuf scratch, ts_tmp, out_tmp;
  hipEvent_t done = nullptr;     // the last run; a run on another stream waits for it (the scratch is shared)
  hipStream_t last = nullptr;
  bool ran = false;
  ~dvbt2ll_modeadapt() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
};

// Kbch of (framesize, rate) as build_fec has them (t2_plan.cpp fec_numbers); 0: not a code
static int modeadapt_kbch_of(int framesize, int rate) {
  static const int normal[6] = {32208, 38688, 43040, 48408, 51648, 53840};
  static const int shortf[8] = {7032, 9552, 10632, 11712, 12432, 13152, 5232, 6312};
  if (framesize == 1) return rate >= 0 && rate < 6 ? normal[rate] : 0;
  if (framesize == 0) return rate >= 0 && rate < 8 ? shortf[rate] : 0;
  return 0;
}

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
  std::unique_ptr<dvbt2ll_modeadapt> h(new (std::nothrow) dvbt2ll_modeadapt());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  h->p.kbch = kbch;
  h->p.pid_mask = nullptr;   // copied to the device below: the caller's array is not kept
  int r = h->ctx.init(device);
  if (r) return r;
  MaDev &d = h->dev;
  d.npd = p->npd;
  d.has_mask = p->pid_mask != nullptr;
  d.L = (uint32_t)kbch / 8;
  d.D = d.L - 10;
  // MATYPE-1: TS_GS 11, SIS/MIS, CCM 1, ISSYI 0, NPD, EXT 00 (the chain's MATYPE_SIS / MATYPE_MIS with the NPD bit)
  d.matype = (uint32_t)(p->sis_mis ? MATYPE_SIS : MATYPE_MIS | p->isi) | (p->npd ? 0x0400u : 0u);
  d.max_ts = (uint32_t)(p->max_ts_bytes / 188);
  if (h->scratch.ensure(modeadapt_layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)modeadapt_layout(d, h->scratch.p);
  uint32_t tab[256];
  modeadapt_host_table(tab);
  HIP_TRY(hipMemcpy(d.crc, tab, sizeof tab, hipMemcpyHostToDevice));
  if (p->pid_mask) HIP_TRY(hipMemcpy(d.mask, p->pid_mask, 1024, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, MA_R_WORDS * 8));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_modeadapt_params_from_chain(const dvbt2ll_chain *chain, int plp, dvbt2ll_modeadapt_params *p) {
  if (!chain || !p || plp < 0 || plp >= chain->nplp) return DVBT2LL_EINVAL;
  const auto &pl = *chain->plps[plp];
  p->kbch = pl.fec.plan.kbch;
  p->sis_mis = (pl.fec.dev.matype & 0x2000) ? 1 : 0;
  p->isi = p->sis_mis ? 0 : (pl.fec.dev.matype & 255);
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
  int e = modeadapt_run_args(h, ts_dev, ts_len, start, out_dev, out_cap_blocks, r);
  if (e) return e;
  r.flush = flush != 0;
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  HIP_TRY(modeadapt_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->last = st;
  h->ran = true;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_modeadapt_get_result(dvbt2ll_modeadapt *h, dvbt2ll_modeadapt_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  uint64_t w[MA_R_WORDS];
  HIP_TRY(hipMemcpy(w, h->dev.res, sizeof w, hipMemcpyDeviceToHost));
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
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  // no more BBFRAMEs than the buffer's packets can fill, whatever the capacity says
  const int64_t cap = std::min<int64_t>(r.cap, (int64_t)r.n * 188 / h->dev.D + 1);
  if (h->ts_tmp.ensure((size_t)std::max<int64_t>(ts_len, 1))) return DVBT2LL_ENOMEM;
  if (h->out_tmp.ensure((size_t)cap * h->dev.L + 16)) return DVBT2LL_ENOMEM;
  if (ts_len) HIP_TRY(hipMemcpyAsync(h->ts_tmp.p, ts, (size_t)ts_len, hipMemcpyHostToDevice, h->ctx.stream));
  if ((e = dvbt2ll_modeadapt_run_device(h, h->ts_tmp.p, ts_len, start, h->out_tmp.p, out_cap_blocks, flush,
                                        h->ctx.stream)))
    return e;
  if ((e = dvbt2ll_modeadapt_get_result(h, res))) return e;
  if (res->bbframes > 0)
    HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)res->bbframes * h->dev.L, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_modeadapt_destroy(dvbt2ll_modeadapt *h) { delete h; }

// ============================================================================ ULE encapsulator
// A handle beside the chain, built like the mode adapter's: scratch sized at create from max_pdus, no stream state,
// all passes of a run on the caller's stream (ule_kernels.hip), the result on the device until get_result.
struct dvbt2ll_ule {
  DeviceCtx ctx;
  dvbt2ll_ule_params p{};
  UleDev dev;
  DevBuf scratch, pdu_tmp, off_tmp, type_tmp, out_tmp;
  hipEvent_t done = nullptr;     // the last run; a run on another stream waits for it (the scratch is shared)
  hipStream_t last = nullptr;
  bool ran = false;
  ~dvbt2ll_ule() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
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
  std::unique_ptr<dvbt2ll_ule> h(new (std::nothrow) dvbt2ll_ule());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  int r = h->ctx.init(device);
  if (r) return r;
  UleDev &d = h->dev;
  d.pid = p->pid;
  d.d_bit = p->d_bit;
  d.packing = p->packing;
  memcpy(d.dest, p->dest, 6);
  d.max_pdus = (uint32_t)p->max_pdus;
  if (h->scratch.ensure(ule_layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)ule_layout(d, h->scratch.p);
  std::vector<uint32_t> tab(ULE_TAB_WORDS);
  ule_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (ULE_R_WORDS + 2) * 8));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
  return DVBT2LL_OK;
}

static int ule_run_args(const dvbt2ll_ule *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                        const uint16_t *type, int64_t n_pdus, const dvbt2ll_ule_pos *start, void *out, int64_t cap,
                        UleRun &r) {
  if (!h || !pdu || !off || !start || !out) return DVBT2LL_EINVAL;
  if (pdu_len < 0 || pdu_len > h->p.max_pdu_bytes || n_pdus < 0 || n_pdus > h->p.max_pdus || cap < 0)
    return DVBT2LL_EINVAL;
  if (start->pdu < 0 || start->pdu > n_pdus || start->sndu_byte < 0 || start->sndu_byte >= ULE_MAX_SNDU ||
      start->cc < 0 || start->cc > 15 || (start->sndu_byte && start->pdu == n_pdus))
    return DVBT2LL_EINVAL;
  r.pdu = (const uint8_t *)pdu;
  r.pdu_len = (uint32_t)pdu_len;
  r.off = off;
  r.type = type;
  r.i0 = (uint32_t)start->pdu;
  r.n = (uint32_t)(n_pdus - start->pdu);
  r.sndu_byte = (uint32_t)start->sndu_byte;
  r.cc = (uint32_t)start->cc;
  r.out = (uint8_t *)out;
  r.cap = (uint32_t)std::min<int64_t>(cap, (int64_t)1 << 30);
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_ule_run_device(dvbt2ll_ule *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                                      const uint16_t *type_dev, int64_t n_pdus, const dvbt2ll_ule_pos *start,
                                      void *out_dev, int64_t out_cap_packets, int flush, void *stream) {
  UleRun r;
  int e = ule_run_args(h, pdu_dev, pdu_len, off_dev, type_dev, n_pdus, start, out_dev, out_cap_packets, r);
  if (e) return e;
  r.flush = flush != 0;
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  HIP_TRY(ule_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->last = st;
  h->ran = true;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_ule_get_result(dvbt2ll_ule *h, dvbt2ll_ule_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  uint64_t w[ULE_R_WORDS];
  HIP_TRY(hipMemcpy(w, h->dev.res, sizeof w, hipMemcpyDeviceToHost));
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
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  // no more packets than the PDUs can become wherever the offsets put them, whatever the capacity says: the
  // device buffer holds this capacity, and this capacity is what the run is given
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, ule_packet_limit(h->dev, r.pdu_len, r.n));
  if (h->pdu_tmp.ensure((size_t)std::max<int64_t>(pdu_len, 1))) return DVBT2LL_ENOMEM;
  if (h->off_tmp.ensure((size_t)(n_pdus + 1) * 4)) return DVBT2LL_ENOMEM;
  if (type && h->type_tmp.ensure((size_t)std::max<int64_t>(n_pdus, 1) * 2)) return DVBT2LL_ENOMEM;
  if (h->out_tmp.ensure((size_t)cap * 188 + 16)) return DVBT2LL_ENOMEM;
  hipStream_t st = h->ctx.stream;
  if (pdu_len) HIP_TRY(hipMemcpyAsync(h->pdu_tmp.p, pdu, (size_t)pdu_len, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(h->off_tmp.p, off, (size_t)(n_pdus + 1) * 4, hipMemcpyHostToDevice, st));
  if (type && n_pdus) HIP_TRY(hipMemcpyAsync(h->type_tmp.p, type, (size_t)n_pdus * 2, hipMemcpyHostToDevice, st));
  if ((e = dvbt2ll_ule_run_device(h, h->pdu_tmp.p, pdu_len, (const uint32_t *)h->off_tmp.p,
                                  type ? (const uint16_t *)h->type_tmp.p : nullptr, n_pdus, start, h->out_tmp.p,
                                  cap, flush, st)))
    return e;
  if ((e = dvbt2ll_ule_get_result(h, res))) return e;
  if (res->ts_packets > 0)
    HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)res->ts_packets * 188, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_ule_destroy(dvbt2ll_ule *h) { delete h; }

// ============================================================================ MPE encapsulator
// A handle beside the chain, built like the ULE one: scratch sized at create from max_pdus, no stream state, all passes
// of a run on the caller's stream (mpe_kernels.hip), the result on the device until get_result.
struct dvbt2ll_mpe {
  DeviceCtx ctx;
  dvbt2ll_mpe_params p{};
  MpeDev dev;
  DevBuf scratch, pdu_tmp, off_tmp, out_tmp;
  hipEvent_t done = nullptr;     // the last run; a run on another stream waits for it (the scratch is shared)
  hipStream_t last = nullptr;
  bool ran = false;
  ~dvbt2ll_mpe() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
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
  std::unique_ptr<dvbt2ll_mpe> h(new (std::nothrow) dvbt2ll_mpe());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  int r = h->ctx.init(device);
  if (r) return r;
  MpeDev &d = h->dev;
  d.pid = p->pid;
  d.mac_mode = p->mac_mode;
  d.packing = p->packing;
  memcpy(d.mac, p->mac, 6);
  d.max_pdus = (uint32_t)p->max_pdus;
  if (h->scratch.ensure(mpe_layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)mpe_layout(d, h->scratch.p);
  std::vector<uint32_t> tab(MPE_TAB_WORDS);
  mpe_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (MPE_R_WORDS + 2) * 8));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
  return DVBT2LL_OK;
}

static int mpe_run_args(const dvbt2ll_mpe *h, const void *pdu, int64_t pdu_len, const uint32_t *off, int64_t n_pdus,
                        const dvbt2ll_mpe_pos *start, void *out, int64_t cap, MpeRun &r) {
  if (!h || !pdu || !off || !start || !out) return DVBT2LL_EINVAL;
  if (pdu_len < 0 || pdu_len > h->p.max_pdu_bytes || n_pdus < 0 || n_pdus > h->p.max_pdus || cap < 0)
    return DVBT2LL_EINVAL;
  if (start->pdu < 0 || start->pdu > n_pdus || start->section_byte < 0 || start->section_byte >= MPE_MAX_SECTION ||
      start->cc < 0 || start->cc > 15 || (start->section_byte && start->pdu == n_pdus))
    return DVBT2LL_EINVAL;
  r.pdu = (const uint8_t *)pdu;
  r.pdu_len = (uint32_t)pdu_len;
  r.off = off;
  r.i0 = (uint32_t)start->pdu;
  r.n = (uint32_t)(n_pdus - start->pdu);
  r.section_byte = (uint32_t)start->section_byte;
  r.cc = (uint32_t)start->cc;
  r.out = (uint8_t *)out;
  r.cap = (uint32_t)std::min<int64_t>(cap, (int64_t)1 << 30);
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpe_run_device(dvbt2ll_mpe *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                                      int64_t n_pdus, const dvbt2ll_mpe_pos *start, void *out_dev,
                                      int64_t out_cap_packets, int flush, void *stream) {
  MpeRun r;
  int e = mpe_run_args(h, pdu_dev, pdu_len, off_dev, n_pdus, start, out_dev, out_cap_packets, r);
  if (e) return e;
  r.flush = flush != 0;
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  HIP_TRY(mpe_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->last = st;
  h->ran = true;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpe_get_result(dvbt2ll_mpe *h, dvbt2ll_mpe_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  uint64_t w[MPE_R_WORDS];
  HIP_TRY(hipMemcpy(w, h->dev.res, sizeof w, hipMemcpyDeviceToHost));
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
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  // no more packets than the PDUs can become wherever the offsets put them, whatever the capacity says: the
  // device buffer holds this capacity, and this capacity is what the run is given
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, mpe_packet_limit(h->dev, r.pdu_len, r.n));
  if (h->pdu_tmp.ensure((size_t)std::max<int64_t>(pdu_len, 1))) return DVBT2LL_ENOMEM;
  if (h->off_tmp.ensure((size_t)(n_pdus + 1) * 4)) return DVBT2LL_ENOMEM;
  if (h->out_tmp.ensure((size_t)cap * 188 + 16)) return DVBT2LL_ENOMEM;
  hipStream_t st = h->ctx.stream;
  if (pdu_len) HIP_TRY(hipMemcpyAsync(h->pdu_tmp.p, pdu, (size_t)pdu_len, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(h->off_tmp.p, off, (size_t)(n_pdus + 1) * 4, hipMemcpyHostToDevice, st));
  if ((e = dvbt2ll_mpe_run_device(h, h->pdu_tmp.p, pdu_len, (const uint32_t *)h->off_tmp.p, n_pdus, start,
                                  h->out_tmp.p, cap, flush, st)))
    return e;
  if ((e = dvbt2ll_mpe_get_result(h, res))) return e;
  if (res->ts_packets > 0)
    HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)res->ts_packets * 188, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_mpe_destroy(dvbt2ll_mpe *h) { delete h; }

// ============================================================================ MPE-FEC encapsulator
// A handle beside the chain, built like the MPE one: scratch sized at create from max_pdus and max_frames (the frames'
// tables and RS columns), no stream state, all passes of a run on the caller's stream (mpefec_kernels.hip).
struct dvbt2ll_mpefec {
  DeviceCtx ctx;
  dvbt2ll_mpefec_params p{};
  MfDev dev;
  DevBuf scratch, pdu_tmp, off_tmp, out_tmp;
  hipEvent_t done = nullptr;     // the last run; a run on another stream waits for it (the scratch is shared)
  hipStream_t last = nullptr;
  bool ran = false;
  ~dvbt2ll_mpefec() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
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
  std::unique_ptr<dvbt2ll_mpefec> h(new (std::nothrow) dvbt2ll_mpefec());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  int r = h->ctx.init(device);
  if (r) return r;
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
  if (h->scratch.ensure(mf_layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)mf_layout(d, h->scratch.p);
  std::vector<uint32_t> tab(MF_TAB_WORDS), rstab(MF_RS_WORDS);
  mf_host_tables(tab.data(), rstab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.rstab, rstab.data(), rstab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (MF_R_WORDS + MF_CTL_WORDS / 2) * 8));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
  return DVBT2LL_OK;
}

static int mpefec_run_args(const dvbt2ll_mpefec *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                           int64_t n_pdus, const dvbt2ll_mpefec_pos *start, void *out, int64_t cap, MfRun &r) {
  if (!h || !pdu || !off || !start || !out) return DVBT2LL_EINVAL;
  if (pdu_len < 0 || pdu_len > h->p.max_pdu_bytes || n_pdus < 0 || n_pdus > h->p.max_pdus || cap < 0)
    return DVBT2LL_EINVAL;
  // a frame holds at most D x rows datagrams (of one byte each) and K RS columns: no frame has a section past that
  const int64_t sections = (int64_t)h->p.data_columns * h->p.rows + h->p.rs_columns;
  if (start->pdu < 0 || start->pdu > n_pdus || start->section < 0 || start->section >= sections ||
      start->section_byte < 0 || start->section_byte >= MF_MAX_SECTION || start->cc < 0 || start->cc > 15 ||
      start->frame < 0 || start->frame > 0xFFF || ((start->section || start->section_byte) && start->pdu == n_pdus))
    return DVBT2LL_EINVAL;
  r.pdu = (const uint8_t *)pdu;
  r.pdu_len = (uint32_t)pdu_len;
  r.off = off;
  r.i0 = (uint32_t)start->pdu;
  r.n = (uint32_t)(n_pdus - start->pdu);
  r.section = (uint32_t)start->section;
  r.section_byte = (uint32_t)start->section_byte;
  r.cc = (uint32_t)start->cc;
  r.frame = (uint32_t)start->frame;
  r.out = (uint8_t *)out;
  r.cap = (uint32_t)std::min<int64_t>(cap, (int64_t)1 << 30);
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpefec_run_device(dvbt2ll_mpefec *h, const void *pdu_dev, int64_t pdu_len,
                                         const uint32_t *off_dev, int64_t n_pdus, const dvbt2ll_mpefec_pos *start,
                                         void *out_dev, int64_t out_cap_packets, int flush, void *stream) {
  MfRun r;
  int e = mpefec_run_args(h, pdu_dev, pdu_len, off_dev, n_pdus, start, out_dev, out_cap_packets, r);
  if (e) return e;
  r.flush = flush != 0;
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  HIP_TRY(mf_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->last = st;
  h->ran = true;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_mpefec_get_result(dvbt2ll_mpefec *h, dvbt2ll_mpefec_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  uint64_t w[MF_R_WORDS];
  HIP_TRY(hipMemcpy(w, h->dev.res, sizeof w, hipMemcpyDeviceToHost));
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
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  // no more packets than the PDUs can become wherever the offsets put them, whatever the capacity says
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, mf_packet_limit(h->dev, r.pdu_len, r.n));
  if (h->pdu_tmp.ensure((size_t)std::max<int64_t>(pdu_len, 1))) return DVBT2LL_ENOMEM;
  if (h->off_tmp.ensure((size_t)(n_pdus + 1) * 4)) return DVBT2LL_ENOMEM;
  if (h->out_tmp.ensure((size_t)cap * 188 + 16)) return DVBT2LL_ENOMEM;
  hipStream_t st = h->ctx.stream;
  if (pdu_len) HIP_TRY(hipMemcpyAsync(h->pdu_tmp.p, pdu, (size_t)pdu_len, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(h->off_tmp.p, off, (size_t)(n_pdus + 1) * 4, hipMemcpyHostToDevice, st));
  if ((e = dvbt2ll_mpefec_run_device(h, h->pdu_tmp.p, pdu_len, (const uint32_t *)h->off_tmp.p, n_pdus, start,
                                     h->out_tmp.p, cap, flush, st)))
    return e;
  if ((e = dvbt2ll_mpefec_get_result(h, res))) return e;
  if (res->ts_packets > 0)
    HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)res->ts_packets * 188, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_mpefec_destroy(dvbt2ll_mpefec *h) { delete h; }

// ============================================================================ TS multiplexer
// A handle beside the chain, built like the MPE one: the schedule tables are made at create (tsmux_plan.cpp) and stay
// on the device; a run is one kernel on the caller's stream (tsmux_kernels.hip) whose counters stay on the device
// until get_result, which adds the resume position: that is arithmetic on the start position and the counters.
struct dvbt2ll_tsmux {
  DeviceCtx ctx;
  dvbt2ll_tsmux_params p{};
  TsmuxPlan plan;
  TsmuxDev dev;
  DevBuf table, pre, res, out_tmp;
  DevBuf in_tmp[TSMUX_IN];
  dvbt2ll_tsmux_pos start{};     // of the last run
  int64_t n_in[TSMUX_IN] = {}, n_out = 0;
  hipEvent_t done = nullptr;     // the last run; a run on another stream waits for it (the counters are shared)
  hipStream_t last = nullptr;
  bool ran = false;
  // the remux (dvbt2ll_tsmux_set_remux): its tables and scan scratch, the last run's start position
  bool remux = false;
  dvbt2ll_tsmux_remux x{};
  TsremuxDev xdev;
  DevBuf pid_map, slot_of, tiles, chunks, xres;
  dvbt2ll_tsmux_remux_pos rstart{};
  int64_t tpp = 0;               // the mux clock: p.ticks_per_period, or the remux's out_ticks_per_period
  ~dvbt2ll_tsmux() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
};

extern "C" int dvbt2ll_tsmux_create(const dvbt2ll_tsmux_params *p, int device, dvbt2ll_tsmux **out) {
  if (!p || !out) return DVBT2LL_EINVAL;
  *out = nullptr;
  if (!tsmux_params_ok(*p)) return DVBT2LL_EINVAL;
  std::unique_ptr<dvbt2ll_tsmux> h(new (std::nothrow) dvbt2ll_tsmux());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  h->tpp = p->ticks_per_period;
  int r = h->ctx.init(device);
  if (r) return r;
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
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
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
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  if (rstart) {
    HIP_TRY(tsremux_launch(h->dev, h->xdev, r, y, st));
    h->rstart = *rstart;
  } else HIP_TRY(tsmux_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->start = *start;
  h->n_out = n_out;
  for (int i = 0; i < TSMUX_IN; i++) h->n_in[i] = i < h->p.n_inputs ? n_in[i] : 0;
  h->last = st;
  h->ran = true;
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
  if (!h || !x || h->ran || h->remux || !tsmux_remux_ok(h->p, *x)) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
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
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  uint64_t w[TSMUX_R_WORDS];
  HIP_TRY(hipMemcpy(w, h->dev.res, sizeof w, hipMemcpyDeviceToHost));
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
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  hipStream_t st = h->ctx.stream;
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
// A handle beside the chain, built like the ULE one: scratch sized at create from max_pdus and Kbch, no stream state,
// all passes of a run on the caller's stream (gse_kernels.hip), the result on the device until get_result.
struct dvbt2ll_gse {
  DeviceCtx ctx;
  dvbt2ll_gse_params p{};
  GseDev dev;
  DevBuf scratch, pdu_tmp, off_tmp, type_tmp, out_tmp;
  hipEvent_t done = nullptr;     // the last run; a run on another stream waits for it (the scratch is shared)
  hipStream_t last = nullptr;
  bool ran = false;
  ~dvbt2ll_gse() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
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
  std::unique_ptr<dvbt2ll_gse> h(new (std::nothrow) dvbt2ll_gse());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  h->p.kbch = kbch;
  int r = h->ctx.init(device);
  if (r) return r;
  GseDev &d = h->dev;
  d.Lb = (uint32_t)kbch / 8;
  d.D = d.Lb - 10;
  d.L = (uint32_t)p->label_len;
  d.lt = d.L == 6 ? 0 : d.L == 3 ? 1 : 2;
  memcpy(d.label, p->label, 6);
  // MATYPE-1: TS_GS 10, SIS/MIS, CCM 1, ISSYI 0, NPD 0, EXT 00
  d.matype = p->sis_mis ? 0xB000u : 0x9000u | (uint32_t)p->isi;
  d.max_pdus = (uint32_t)p->max_pdus;
  if (h->scratch.ensure(gse_layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)gse_layout(d, h->scratch.p);
  std::vector<uint32_t> tab(GSE_TAB_WORDS);
  gse_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(d.res, 0, (GSE_R_WORDS + 2) * 8));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  *out = h.release();
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_gse_params_from_chain(const dvbt2ll_chain *chain, int plp, dvbt2ll_gse_params *p) {
  if (!chain || !p || plp < 0 || plp >= chain->nplp) return DVBT2LL_EINVAL;
  const auto &pl = *chain->plps[plp];
  p->kbch = pl.fec.plan.kbch;
  p->sis_mis = (pl.fec.dev.matype & 0x2000) ? 1 : 0;
  p->isi = p->sis_mis ? 0 : (pl.fec.dev.matype & 255);
  return DVBT2LL_OK;
}

static int gse_run_args(const dvbt2ll_gse *h, const void *pdu, int64_t pdu_len, const uint32_t *off,
                        const uint16_t *type, int64_t n_pdus, const dvbt2ll_gse_pos *start, void *out, int64_t cap,
                        GseRun &r) {
  if (!h || !pdu || !off || !start || !out) return DVBT2LL_EINVAL;
  if (pdu_len < 0 || pdu_len > h->p.max_pdu_bytes || n_pdus < 0 || n_pdus > h->p.max_pdus || cap < 0)
    return DVBT2LL_EINVAL;
  if (start->pdu < 0 || start->pdu > n_pdus || start->pdu_byte < 0 || start->frag_id < 0 ||
      start->frag_id > 255)
    return DVBT2LL_EINVAL;
  r.pdu = (const uint8_t *)pdu;
  r.pdu_len = (uint32_t)pdu_len;
  r.off = off;
  r.type = type;
  r.i0 = (uint32_t)start->pdu;
  r.n = (uint32_t)(n_pdus - start->pdu);
  r.pdu_byte = (uint32_t)start->pdu_byte;
  r.frag_id = (uint32_t)start->frag_id;
  r.out = (uint8_t *)out;
  r.cap = (uint32_t)std::min<int64_t>(cap, (int64_t)1 << 30);
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_gse_run_device(dvbt2ll_gse *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                                      const uint16_t *type_dev, int64_t n_pdus, const dvbt2ll_gse_pos *start,
                                      void *out_dev, int64_t out_cap_blocks, int flush, void *stream) {
  GseRun r;
  int e = gse_run_args(h, pdu_dev, pdu_len, off_dev, type_dev, n_pdus, start, out_dev, out_cap_blocks, r);
  if (e) return e;
  r.flush = flush != 0;
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  HIP_TRY(gse_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->last = st;
  h->ran = true;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_gse_get_result(dvbt2ll_gse *h, dvbt2ll_gse_result *res) {
  if (!h || !res) return DVBT2LL_EINVAL;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  uint64_t w[GSE_R_WORDS];
  HIP_TRY(hipMemcpy(w, h->dev.res, sizeof w, hipMemcpyDeviceToHost));
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
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  // no more frames than the PDUs can become wherever the offsets put them, whatever the capacity says: the device
  // buffer holds this capacity, and this capacity is what the run is given
  const int64_t cap = (int64_t)std::min<uint64_t>(r.cap, gse_frame_limit(h->dev, r.pdu_len, r.n));
  if (h->pdu_tmp.ensure((size_t)std::max<int64_t>(pdu_len, 1))) return DVBT2LL_ENOMEM;
  if (h->off_tmp.ensure((size_t)(n_pdus + 1) * 4)) return DVBT2LL_ENOMEM;
  if (type && h->type_tmp.ensure((size_t)std::max<int64_t>(n_pdus, 1) * 2)) return DVBT2LL_ENOMEM;
  if (h->out_tmp.ensure((size_t)cap * h->dev.Lb + 16)) return DVBT2LL_ENOMEM;
  hipStream_t st = h->ctx.stream;
  if (pdu_len) HIP_TRY(hipMemcpyAsync(h->pdu_tmp.p, pdu, (size_t)pdu_len, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(h->off_tmp.p, off, (size_t)(n_pdus + 1) * 4, hipMemcpyHostToDevice, st));
  if (type && n_pdus) HIP_TRY(hipMemcpyAsync(h->type_tmp.p, type, (size_t)n_pdus * 2, hipMemcpyHostToDevice, st));
  if ((e = dvbt2ll_gse_run_device(h, h->pdu_tmp.p, pdu_len, (const uint32_t *)h->off_tmp.p,
                                  type ? (const uint16_t *)h->type_tmp.p : nullptr, n_pdus, start, h->out_tmp.p,
                                  cap, flush, st)))
    return e;
  if ((e = dvbt2ll_gse_get_result(h, res))) return e;
  if (res->bbframes > 0)
    HIP_TRY(hipMemcpy(out, h->out_tmp.p, (size_t)res->bbframes * h->dev.Lb, hipMemcpyDeviceToHost));
  return DVBT2LL_OK;
}

extern "C" void dvbt2ll_gse_destroy(dvbt2ll_gse *h) { delete h; }

// ============================================================================ T2-MI output
// A handle beside the chain, built like the T2-MI input one.  Every packet length is a constant of the handle and every
// call starts on a TS packet boundary, so the positions of a call's packets are walked once at create
// (t2mo_host_walk) and a call's counters are arithmetic on the host: run_device launches the CRC and emit passes on the
// caller's stream (t2mi_out_kernels.hip) and keeps the result for get_result.
struct dvbt2ll_t2mi_out {
  DeviceCtx ctx;
  dvbt2ll_t2mi_out_params p{};
  T2moDev dev;
  T2moFrames frames;
  std::vector<T2moPkt> pkt;        // P + 1
  uint32_t aux_bytes[DVBT2LL_T2MI_OUT_MAX_AUX] = {};
  dvbt2ll_t2mi_out_result res{};   // the last run's
  DevBuf scratch, bb_tmp[DVBT2LL_MAX_PLP], aux_tmp, out_tmp;
  hipEvent_t done = nullptr;       // the last run; a run on another stream waits for it (the scratch is shared)
  hipStream_t last = nullptr;
  bool ran = false;
  ~dvbt2ll_t2mi_out() {
    if (done) { (void)hipSetDevice(ctx.device); (void)hipEventSynchronize(done); (void)hipEventDestroy(done); }
  }
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
  std::unique_ptr<dvbt2ll_t2mi_out> h(new (std::nothrow) dvbt2ll_t2mi_out());
  if (!h) return DVBT2LL_ENOMEM;
  h->p = *p;
  int r = h->ctx.init(device);
  if (r) return r;
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
  if (h->scratch.ensure(t2mo_layout(d, nullptr))) return DVBT2LL_ENOMEM;
  (void)t2mo_layout(d, h->scratch.p);
  std::vector<uint32_t> tab(T2MO_TAB_WORDS);
  t2mo_host_tables(tab.data());
  HIP_TRY(hipMemcpy(d.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.pkt, pkt.data(), pkt.size() * sizeof(T2moPkt), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.tq, tq.data(), tq.size() * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d.td, td.data(), td.size(), hipMemcpyHostToDevice));
  HIP_TRY(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
  h->pkt = std::move(pkt);
  *out = h.release();
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_out_params_from_chain(const dvbt2ll_chain *chain, const int *plp_ids,
                                                  dvbt2ll_t2mi_out_params *p) {
  if (!chain || !p || chain->nplp < 1 || chain->nplp > DVBT2LL_MAX_PLP) return DVBT2LL_EINVAL;
  for (int k = 0; k < chain->nplp; k++)
    if (chain->plps[k]->cyc != 1 || chain->plps[k]->P != 1) return DVBT2LL_EINVAL;   // P_I x I_JUMP > 1: not built
  p->nplp = chain->nplp;
  for (int k = 0; k < chain->nplp; k++) {
    p->plp_id[k] = plp_ids ? plp_ids[k] : k;
    p->bbframe_bytes[k] = (int)chain->plps[k]->bbf_len();
    p->blocks_per_frame[k] = chain->plps[k]->F;
  }
  p->frames_per_superframe = std::max(1, chain->frame.t2frames);
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
  int e = t2mo_run_args(h, bb_dev, aux_dev, aux_stride, aux_off, start, nframes, out_dev, out_cap_packets, r);
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  hipStream_t st = stream ? (hipStream_t)stream : h->ctx.stream;
  if (h->ran && h->last != st) HIP_TRY(hipStreamWaitEvent(st, h->done, 0));
  HIP_TRY(t2mo_launch(h->dev, r, st));
  HIP_TRY(hipEventRecord(h->done, st));
  h->last = st;
  h->ran = true;
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
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  *res = h->res;
  return DVBT2LL_OK;
}

extern "C" int dvbt2ll_t2mi_out_run_host(dvbt2ll_t2mi_out *h, const void *const *bb, const void *aux,
                                         int64_t aux_stride, const int64_t *aux_off, const dvbt2ll_t2mi_out_pos *start,
                                         int nframes, void *out, int64_t out_cap_packets, dvbt2ll_t2mi_out_result *res) {
  T2moRun r;
  if (!res) return DVBT2LL_EINVAL;
  int e = t2mo_run_args(h, bb, aux, aux_stride, aux_off, start, nframes, out, out_cap_packets, r);
  if (e) return e;
  HIP_TRY(hipSetDevice(h->ctx.device));
  if (h->ran) HIP_TRY(hipEventSynchronize(h->done));
  hipStream_t st = h->ctx.stream;
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
