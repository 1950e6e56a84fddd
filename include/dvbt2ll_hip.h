/*
 * dvbt2ll_hip.h -- C ABI of the MI355X-native DVB-T2 transmit chain.
 *
 * Drop-in boundary for the four gr-dvbt2ll blocks (plus the gr-dtv LDPC block the
 * shipped flowgraph places between bbheaderbch and interleavermod).  Each block is an
 * opaque handle that reproduces the reference gr::block contract:
 *
 *   make()            -> dvbt2ll_<blk>_create()      (reference include/dvbt2ll/<blk>.h:49)
 *   set_output_multiple -> dvbt2ll_<blk>_output_multiple()
 *   forecast()        -> dvbt2ll_<blk>_forecast()
 *   general_work()    -> dvbt2ll_<blk>_general_work() (+ consume_each via *consumed)
 *
 * Buffers passed to general_work are HOST buffers owned by the caller (GNU Radio
 * circular buffers); the call is synchronous and retains no pointer.  Handles own
 * their device memory and one HIP stream.  Instances are independent; one instance
 * must not be called from two threads at once (GNU Radio never does).
 *
 * The fused chain (dvbt2ll_chain_*) runs TS bytes -> IQ for whole T2 frames with
 * device-resident buffers; it is what bench.py measures.
 *
 * Enum arguments use the reference's numeric values (include/dvbt2ll/dvbt2ll_config.h:60-202).
 * Errors: the reference throws std::bad_alloc from constructors and silently accepts
 * invalid parameter combinations; this ABI returns negative status codes instead.
 */
#ifndef DVBT2LL_HIP_H
#define DVBT2LL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVBT2LL_OK 0
#define DVBT2LL_EINVAL (-1)   /* invalid parameter combination                       */
#define DVBT2LL_ENOMEM (-2)   /* device/host allocation failed (reference: bad_alloc) */
#define DVBT2LL_EDEVICE (-3)  /* HIP runtime / kernel launch error                     */
#define DVBT2LL_ESHORT (-4)   /* fewer input items than forecast() requires            */

const char *dvbt2ll_strerror(int status);
const char *dvbt2ll_version(void);
/* number of visible HIP devices (0 when no GPU) -- never initialises a context */
int dvbt2ll_device_count(void);

/* ---------------------------------------------------------------------------
 * bbheaderbch_bb: TS bytes -> BBFRAME + BCH, one unpacked bit per output byte.
 * Replaces gr::dvbt2ll::bbheaderbch_bb::make(framesize, rate, mode, inband, fecblocks,
 * tsrate) (include/dvbt2ll/bbheaderbch_bb.h:49; lib/bbheaderbch_bb_impl.cc:32-37).
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_bbheaderbch dvbt2ll_bbheaderbch;
typedef struct {
  int framesize, rate, mode, inband, fecblocks, tsrate;
} dvbt2ll_bbheaderbch_params;
int dvbt2ll_bbheaderbch_create(const dvbt2ll_bbheaderbch_params *p, int device, dvbt2ll_bbheaderbch **out);
int dvbt2ll_bbheaderbch_output_multiple(const dvbt2ll_bbheaderbch *h);             /* nbch (impl.cc:195) */
int dvbt2ll_bbheaderbch_forecast(const dvbt2ll_bbheaderbch *h, int noutput_items, int *ninput_items_required);
int dvbt2ll_bbheaderbch_general_work(dvbt2ll_bbheaderbch *h, int noutput_items, int ninput_items,
                                     const void *in, void *out, int *consumed);
/* TS sync bytes != 0x47 consumed so far (the reference logs "Transport Stream sync error!" for each,
 * lib/bbheaderbch_bb_impl.cc:675-677, 703-705; the output is unaffected in both input modes) */
int64_t dvbt2ll_bbheaderbch_sync_errors(const dvbt2ll_bbheaderbch *h);
void dvbt2ll_bbheaderbch_destroy(dvbt2ll_bbheaderbch *h);

/* ---------------------------------------------------------------------------
 * ldpc_bb: nbch unpacked bits -> nldpc unpacked bits (natural parity order).
 * Replaces gr-dtv dvb_ldpc_bb(standard=DVBT2, framesize, rate, MOD_OTHER) as wired in
 * apps/vv009-4kshort.grc:386-460; arithmetic = lib/bbheaderbch_bb_impl.cc:533-646.
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_ldpc dvbt2ll_ldpc;
typedef struct {
  int framesize, rate;
} dvbt2ll_ldpc_params;
int dvbt2ll_ldpc_create(const dvbt2ll_ldpc_params *p, int device, dvbt2ll_ldpc **out);
int dvbt2ll_ldpc_output_multiple(const dvbt2ll_ldpc *h);                           /* nldpc */
int dvbt2ll_ldpc_forecast(const dvbt2ll_ldpc *h, int noutput_items, int *ninput_items_required);
int dvbt2ll_ldpc_general_work(dvbt2ll_ldpc *h, int noutput_items, int ninput_items, const void *in,
                              void *out, int *consumed);
void dvbt2ll_ldpc_destroy(dvbt2ll_ldpc *h);

/* ---------------------------------------------------------------------------
 * interleavermod_bc: nldpc unpacked bits -> cell_size complex64 cells per FEC block.
 * Replaces gr::dvbt2ll::interleavermod_bc::make(framesize, rate, constellation, rotation)
 * (include/dvbt2ll/interleavermod_bc.h:49; lib/interleavermod_bc_impl.cc:32-37).
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_interleavermod dvbt2ll_interleavermod;
typedef struct {
  int framesize, rate, constellation, rotation;
} dvbt2ll_interleavermod_params;
int dvbt2ll_interleavermod_create(const dvbt2ll_interleavermod_params *p, int device,
                                  dvbt2ll_interleavermod **out);
int dvbt2ll_interleavermod_output_multiple(const dvbt2ll_interleavermod *h);       /* cell_size (:254) */
int dvbt2ll_interleavermod_forecast(const dvbt2ll_interleavermod *h, int noutput_items, int *ninput_items_required);
int dvbt2ll_interleavermod_general_work(dvbt2ll_interleavermod *h, int noutput_items, int ninput_items,
                                        const void *in, void *out, int *consumed);
void dvbt2ll_interleavermod_destroy(dvbt2ll_interleavermod *h);

/* ---------------------------------------------------------------------------
 * framemapperfint_cc: one T2 frame of stream cells -> mapped (frequency-interleaved)
 * cells.  Replaces gr::dvbt2ll::framemapperfint_cc::make(...20 parameters...)
 * (include/dvbt2ll/framemapperfint_cc.h:49; lib/framemapperfint_cc_impl.cc:31-36).
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_framemapperfint dvbt2ll_framemapperfint;
typedef struct {
  int framesize, rate, constellation, rotation, fecblocks, tiblocks, carriermode, fftsize,
      guardinterval, l1constellation, pilotpattern, t2frames, numdatasyms, paprmode, version,
      preamble, inputmode, reservedbiasbits, l1scrambled, inband;
} dvbt2ll_framemapperfint_params;
int dvbt2ll_framemapperfint_create(const dvbt2ll_framemapperfint_params *p, int device,
                                   dvbt2ll_framemapperfint **out);
int dvbt2ll_framemapperfint_output_multiple(const dvbt2ll_framemapperfint *h);     /* mapped_items */
int dvbt2ll_framemapperfint_stream_items(const dvbt2ll_framemapperfint *h);
int dvbt2ll_framemapperfint_forecast(const dvbt2ll_framemapperfint *h, int noutput_items, int *ninput_items_required);
int dvbt2ll_framemapperfint_general_work(dvbt2ll_framemapperfint *h, int noutput_items, int ninput_items,
                                         const void *in, void *out, int *consumed);
void dvbt2ll_framemapperfint_destroy(dvbt2ll_framemapperfint *h);

/* ---------------------------------------------------------------------------
 * pilotgenp1insert_cc: one T2 frame of mapped cells -> P1 + OFDM symbols with GI.
 * Replaces gr::dvbt2ll::pilotgenp1insert_cc::make(carriermode, fftsize, pilotpattern,
 * guardinterval, numdatasyms, paprmode, version, preamble, misogroup, equalization,
 * bandwidth, vlength) (include/dvbt2ll/pilotgenp1insert_cc.h:49; impl.cc:33-38).
 * ------------------------------------------------------------------------- */
/* misogroup (here, in dvbt2ll_chain_params and in dvbt2ll_mplp_chain_params) takes gr-dvbt2ll's
 * dvbt2_misogroup_t values, MISO_TX1 = 0 and MISO_TX2 = 1, which differ in the pilots only (group 2's inverted
 * scattered / continual / edge pilots and MISO P2 pilots; the payload cells go out unchanged, as in the
 * reference), and one value beyond the reference:
 *   DVBT2LL_MISO_TX2_PROCESSED: group 2's pilots plus the MISO processing of EN 302 755 clause 9.1 on the
 *   payload cells.  With a_p, p < n, the payload cells of an OFDM symbol (every symbol but P1) in carrier
 *   order -- all the frame mapper emits for it: L1-pre / L1-post, data, dummy and thinning cells, n = C_P2,
 *   C_DATA or N_FC, always even -- group 2 sends e_2i = -conj(a_2i+1) and e_2i+1 = conj(a_2i) on the carriers
 *   of a_2i and a_2i+1.  Pilots, reserved tones and unused carriers are untouched; the inverse-sinc
 *   equalisation applies after it.  Group 1 of the same service is a second handle with MISO_TX1.
 * DVBT2LL_MISO_TX2_PROCESSED needs a MISO preamble (T2_MISO, T2_LITE_MISO); with a SISO preamble, and for any
 * misogroup outside 0..2, create returns DVBT2LL_EINVAL.  The reference has no MISO processing block, so the
 * processed output has no reference parity; it is pinned to the 9.1 rule applied to the reference's cells. */
#define DVBT2LL_MISO_TX2_PROCESSED 2
typedef struct dvbt2ll_pilotgenp1insert dvbt2ll_pilotgenp1insert;
typedef struct {
  int carriermode, fftsize, pilotpattern, guardinterval, numdatasyms, paprmode, version, preamble,
      misogroup, equalization, bandwidth, vlength;
} dvbt2ll_pilotgenp1insert_params;
int dvbt2ll_pilotgenp1insert_create(const dvbt2ll_pilotgenp1insert_params *p, int device,
                                    dvbt2ll_pilotgenp1insert **out);
int dvbt2ll_pilotgenp1insert_output_multiple(const dvbt2ll_pilotgenp1insert *h);   /* Nsym*(N+GI)+2048 */
int dvbt2ll_pilotgenp1insert_active_items(const dvbt2ll_pilotgenp1insert *h);
int dvbt2ll_pilotgenp1insert_forecast(const dvbt2ll_pilotgenp1insert *h, int noutput_items, int *ninput_items_required);
int dvbt2ll_pilotgenp1insert_general_work(dvbt2ll_pilotgenp1insert *h, int noutput_items, int ninput_items,
                                          const void *in, void *out, int *consumed);
/* test hook: the frequency-domain symbols (after EQ, before fftshift/IFFT) of one frame,
 * num_symbols * vlength complex64 written to carriers (host). */
int dvbt2ll_pilotgenp1insert_debug_carriers(dvbt2ll_pilotgenp1insert *h, const void *in, void *carriers);
void dvbt2ll_pilotgenp1insert_destroy(dvbt2ll_pilotgenp1insert *h);

/* ---------------------------------------------------------------------------
 * Fused chain: TS bytes -> IQ for whole T2 frames (BB+BCH+LDPC -> bit interleave +
 * QAM + cell interleave -> frame/time/frequency interleave + pilots + IFFT + GI + P1).
 * Equivalent to the five blocks above connected in the shipped flowgraph, each frame
 * k encoded with the state the reference would hold at that point of the stream
 * (TS offset, SYNCD count, CRC-8 of the previous packet, t2_frame_num = k % t2frames).
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_chain dvbt2ll_chain;
typedef struct {
  dvbt2ll_framemapperfint_params fm;   /* framesize ... inband */
  int misogroup, equalization, bandwidth;
  int max_frames;                      /* largest nframes per run call */
  int tsrate;                          /* bbheaderbch tsrate: the in-band type B TS rate field */
} dvbt2ll_chain_params;
typedef struct {
  int fec_blocks_per_frame;   /* F */
  int payload_bytes_per_block; /* TS bytes consumed per FEC block (NM) */
  int64_t ts_bytes_per_frame;
  int64_t iq_samples_per_frame;
  int cell_size, stream_items, mapped_items, num_symbols, fft_size, guard_interval;
  int64_t cw_stride_bytes;     /* packed codeword stride in the internal buffer */
  /* T2 frames from one interleaving frame of the PLP to the next: 1 for the reference's PLP, P_I x
   * FRAME_INTERVAL in general (dvbt2ll_plp_params); fec_blocks_per_frame and ts_bytes_per_frame then count
   * one interleaving frame; stream_items stays the cells per T2 frame carrying the PLP */
  int frames_per_if;
} dvbt2ll_chain_info;
int dvbt2ll_chain_create(const dvbt2ll_chain_params *p, int device, dvbt2ll_chain **out);
int dvbt2ll_chain_get_info(const dvbt2ll_chain *h, dvbt2ll_chain_info *info);
/* ts_dev: device pointer to TS bytes whose first byte is absolute stream offset ts_base
 * (a multiple of 188, else DVBT2LL_EINVAL; at least one packet before the first byte the frames consume so
 * the CRC-8 of the preceding packet can be formed); ts_len bytes valid.  iq_dev receives
 * nframes * iq_samples_per_frame samples (complex64, or int16 I/Q pairs after
 * dvbt2ll_chain_set_output(.., DVBT2LL_IQ_SC16)).  iq_dev must be aligned to one output sample:
 * 8 bytes for DVBT2LL_IQ_CF32, 4 bytes for DVBT2LL_IQ_SC16 (else DVBT2LL_EINVAL, nothing is launched).
 * Any such address is valid, e.g. an odd sample offset into a larger buffer (the kernels store sample
 * pairs where the address allows and single samples elsewhere, the same bits either way).  stream:
 * hipStream_t (NULL = the handle's own stream).  Asynchronous on that stream. */
int dvbt2ll_chain_run_device(dvbt2ll_chain *h, const void *ts_dev, int64_t ts_base, int64_t ts_len,
                             int64_t first_frame, int nframes, void *iq_dev, void *stream);
/* multi-stream batch (BASELINE cfg4 "4 independent PLP streams", cfg5 "8-stream batch"): nstreams
 * independent single-PLP T2 signals (the reference carries one PLP per instance,
 * lib/framemapperfint_cc_impl.cc:153, so each stream is its own five-block chain) encoded in one launch of
 * the three kernels.  Stream s's TS bytes are at ts_dev + s * ts_stride, every stream laid out as
 * run_device's ts_dev (the same ts_base and ts_len; ts_stride >= ts_len); all streams encode frames
 * [first_frame, first_frame + nframes).  IQ: stream s, frame first_frame + j at sample
 * (s * nframes + j) * iq_samples_per_frame of iq_dev (aligned to one output sample, as run_device's).
 * nstreams * nframes <= max_frames.
 * run_device(...) == run_streams(h, ts, 0, 1, ...).  Asynchronous on stream. */
int dvbt2ll_chain_run_streams(dvbt2ll_chain *h, const void *ts_dev, int64_t ts_stride, int nstreams,
                              int64_t ts_base, int64_t ts_len, int64_t first_frame, int nframes,
                              void *iq_dev, void *stream);
/* intermediate buffer slots (packed codewords + cell index pairs, ~310 MB per slot for 64 cfg3
 * frames): run calls take the slots round-robin, so calls issued on different streams run
 * concurrently on the GPU (one call's kernels fill the CUs the other call's kernel tails leave
 * idle).  A slot reused on a different stream than its previous run first waits for that run
 * (hipStreamWaitEvent), so any call order is safe.  1 <= nslots <= DVBT2LL_CHAIN_MAX_SLOTS;
 * synchronises the device.  Default 1.  Not part of the reference (GNU Radio runs one
 * general_work per block at a time): the pipelined form of the same calls. */
#define DVBT2LL_CHAIN_MAX_SLOTS 4
int dvbt2ll_chain_set_slots(dvbt2ll_chain *h, int nslots);
/* hipGraph launch mode: run calls issue the chain's kernels as one instantiated hipGraph, captured
 * on first use for each (nframes, IQ format, buffer slot) into a ring of DVBT2LL_CHAIN_GRAPH_RING
 * instantiations; a call re-arms the next idle instantiation of the ring (its kernel nodes'
 * arguments, hipGraphExecKernelNodeSetParams) and launches it, so back-to-back calls on one slot do
 * not wait for each other on the host (the host only waits when every instantiation of the ring is
 * still in flight).  For small per-call batches (one T2 frame per call, as GNU Radio's scheduler
 * calls a block); output identical to the direct launches.  Per-stage timing events are skipped in
 * this mode.  Default off. */
#define DVBT2LL_CHAIN_GRAPH_RING 4
int dvbt2ll_chain_set_graph(dvbt2ll_chain *h, int enable);
/* host buffers, synchronous */
int dvbt2ll_chain_run_host(dvbt2ll_chain *h, const void *ts, int64_t ts_base, int64_t ts_len,
                           int64_t first_frame, int nframes, void *iq);
/* Streaming host path (the reference's output is host memory feeding a sink,
 * lib/pilotgenp1insert_cc_impl.cc:2785-2906 -> apps/vv009-4kshort.grc:801-1623).  A submission copies the
 * TS bytes its frames need from host ts (laid out as run_device's: absolute stream offset ts_base, ts_len
 * bytes) to the device, encodes the frames and copies their IQ (the current dvbt2ll_chain_set_output format)
 * to host iq, on three HIP streams of the handle ordered by events, into the next entry of a ring of
 * DVBT2LL_HOST_RING device buffer sets: submission k + 1's copy-in and k - 1's copy-out run beside k's
 * kernels.  Returns at once with a ticket (the host blocks only when the ring entry's previous submission
 * is still in flight); ts and iq must stay valid, and iq unread, until dvbt2ll_chain_host_wait(ticket)
 * returns.  Page-locked host buffers (dvbt2ll_host_alloc, or hipHostRegister) move at the PCIe rate;
 * pageable ones work, but the runtime stages their copies and the submit call waits for them.
 * Single-PLP chains; nframes <= max_frames; submissions complete in order. */
#define DVBT2LL_HOST_RING 3
int dvbt2ll_chain_host_submit(dvbt2ll_chain *h, const void *ts, int64_t ts_base, int64_t ts_len,
                              int64_t first_frame, int nframes, void *iq, int64_t *ticket);
int dvbt2ll_chain_host_wait(dvbt2ll_chain *h, int64_t ticket);
/* frames [first_frame, first_frame + nframes) through the ring in chunks of chunk_frames (0: max_frames),
 * frame f's IQ at iq + (f - first_frame) * iq_samples_per_frame samples; synchronous */
int dvbt2ll_chain_run_host_pipelined(dvbt2ll_chain *h, const void *ts, int64_t ts_base, int64_t ts_len,
                                     int64_t first_frame, int nframes, void *iq, int chunk_frames);
/* page-locked host memory for the streaming path (page-aligned heap memory, hipHostRegister'ed); NULL on
 * failure.  Free with dvbt2ll_host_free. */
void *dvbt2ll_host_alloc(size_t bytes);
void dvbt2ll_host_free(void *p);
/* IQ output of the chain (default: gain 1, DVBT2LL_IQ_CF32 = pilotgenp1insert_cc's own complex64
 * output).  gain multiplies every normalised sample, as the blocks_multiply_const_xx that follows
 * pilotgen in apps/vv009-4kshort.grc:335-385 (const 0.2) does.  DVBT2LL_IQ_SC16 stores each sample
 * as interleaved int16 I, Q = saturate(round-half-even(x * 32767)), the sc16 wire format of the
 * flowgraph's SDR sink (apps/vv009-4kshort.grc:802-1623): 4 bytes per sample instead of 8.
 * Applies to later run calls. */
#define DVBT2LL_IQ_CF32 0
#define DVBT2LL_IQ_SC16 1
int dvbt2ll_chain_set_output(dvbt2ll_chain *h, float gain, int format);
/* Input format of a PLP (plp = -1: every PLP; default DVBT2LL_INPUT_TS, the transport stream described above).
 * DVBT2LL_INPUT_BBFRAME: the run calls' ts_dev / ts point to BBFRAMEs the caller built (EN 302 755 5.1: any input
 * type, NPD, ISSY, either in-band type; e.g. what dvbt2ll_t2mi_run_device wrote from a T2-MI stream), and the chain
 * starts after the mode adaptation: it scrambles each BBFRAME with the BB PRBS, appends the BCH parity and continues
 * as for a TS.  With L = kbch / 8:
 *   layout   packed, unscrambled BBFRAMEs of L bytes each (80 header bits, then the data field: kbch bits, MSB
 *            first), back to back; the chain writes or alters no header, padding or in-band field
 *   ts_base  the absolute byte offset of the buffer's byte 0 in that BBFRAME stream, a multiple of L
 *   frames   interleaving frame m of the PLP (T2 frame m for the reference's PLP) consumes FEC blocks
 *            [m F, (m + 1) F), stream bytes [m F L, (m + 1) F L): nothing before them, no state from frame to frame
 *   bounds   a run whose BBFRAMEs are not all inside [ts_base, ts_base + ts_len) is DVBT2LL_EINVAL, nothing
 *            launched; no byte outside the buffer is read.  Stream batches use ts_stride as for a TS; the host
 *            paths copy exactly the frames' BBFRAMEs
 * tsrate is unused; inputmode and inband only set the L1-post fields they set for a TS (the caller declares
 * there what its BBFRAMEs carry).  sync_errors counts nothing for such a PLP.  get_info / get_plp_info report
 * ts_bytes_per_frame = F L and payload_bytes_per_block = L while the PLP is in this format.
 * Applies to later run calls, of every form (device, streams, plps, groups, host, the streaming ring), and on
 * ordinary, multi-PLP (the format is per PLP) and MISO pair handles; synchronises the device, and in graph mode
 * drops the instantiated graphs.  An unknown format or PLP index is DVBT2LL_EINVAL.  get_input returns the
 * PLP's format or DVBT2LL_EINVAL. */
#define DVBT2LL_INPUT_TS 0
#define DVBT2LL_INPUT_BBFRAME 1
int dvbt2ll_chain_set_input(dvbt2ll_chain *h, int plp, int format);
int dvbt2ll_chain_get_input(const dvbt2ll_chain *h, int plp);
/* BBFRAME input: the BBFRAMEs consumed by all run calls so far whose header byte 9 is neither the CRC-8 (DVB-S2,
 * generator 0xD5) of bytes 0 .. 8 nor that value XOR 1 (the HEM mode bit, EN 302 755 5.1.7); each BBFRAME is
 * counted once per run, and the output does not depend on it.  DFL and MATYPE are not validated.  Synchronises
 * the device */
int dvbt2ll_chain_bbheader_errors(dvbt2ll_chain *h, int64_t *count);
/* per-stage kernel timing with HIP events on the launch stream: enable, then read the
 * accumulated milliseconds and launch counts of stages {0: fec, 1: map, 2: ofdm, 3: reserved (0)};
 * nstages <= 4.  The frames' L1-post signalling is generated on the GPU every run by extra
 * workgroups of the map launch (counted in stage 1). */
int dvbt2ll_chain_set_timing(dvbt2ll_chain *h, int enable);
int dvbt2ll_chain_get_timing(dvbt2ll_chain *h, double *ms, int64_t *launches, int nstages);
/* test hooks (host outputs, synchronous), last run's frame 0: packed codewords (tempu
 * order; only when that run stored them, see dvbt2ll_chain_debug_keep_codewords, else
 * DVBT2LL_EINVAL); the frame data region in the slot order the OFDM kernel reads, as stored
 * (uint16 constellation index pairs: lo = the cell's index, hi = the index whose Q part
 * it carries, i.e. the previous cell's under rotation) and as complex64 cells */
int dvbt2ll_chain_debug_codewords(dvbt2ll_chain *h, void *out, int64_t bytes);
/* test hook: enable != 0 -> the following runs also store every FEC block's packed codeword in the
 * chain's codeword buffer (the LDPC + map kernel otherwise keeps it on chip) */
int dvbt2ll_chain_debug_keep_codewords(dvbt2ll_chain *h, int enable);
int dvbt2ll_chain_debug_cell_pairs(dvbt2ll_chain *h, void *out, int64_t cells);
int dvbt2ll_chain_debug_cells(dvbt2ll_chain *h, void *out, int64_t cells);
/* TS sync bytes != 0x47 consumed by all run calls so far (bbheaderbch_bb_impl.cc:675, 703);
 * synchronises the device */
int dvbt2ll_chain_sync_errors(dvbt2ll_chain *h, int64_t *count);
int dvbt2ll_chain_synchronize(dvbt2ll_chain *h);
void dvbt2ll_chain_destroy(dvbt2ll_chain *h);

/* ---------------------------------------------------------------------------
 * Multi-PLP frames (EN 302 755 8.3.6.3): nplp Type-1 data PLPs in one T2
 * frame, PLP_ID = index, each with its own TS stream, FEC, constellation, cell interleaver and time
 * interleaver (TIME_IL_TYPE 0, FRAME_INTERVAL 1, so T2 frames stay independent), its cells placed
 * back to back after the L1 signalling in PLP_ID order (PLP_START = the cells before it); the
 * L1-post carries the PLP loops.  The reference carries exactly one PLP
 * (lib/framemapperfint_cc_impl.cc:152-250: num_plp = 1; L1-post serialised at :1553-1691): nplp = 1
 * is its frame bit for bit, nplp > 1 is not pinned by it (PARITY UNPINNED).
 * The OFDM kernels hold one constellation table per distinct (constellation, rotation) pair of the
 * frame's PLPs (PLPs that agree share it): at most 2 x (4 + 16 + 64 + 256) = 680 entries, so every
 * combination of up to DVBT2LL_MAX_PLP PLPs fits the kernels' 1024-entry table area.
 * ------------------------------------------------------------------------- */
#define DVBT2LL_MAX_PLP 8
typedef struct {
  int framesize, rate, constellation, rotation, fecblocks, tiblocks, inputmode, inband, tsrate;
  /* EN 302 755 beyond the reference's PLP (which is plp_type 1, ti_type 0, ti_frames 1,
   * lib/framemapperfint_cc_impl.cc:159, 198-200; PARITY UNPINNED otherwise):
   *   plp_type  1: Type-1 data PLP, one run of cells at its PLP_START (0 is read as 1);
   *             2: Type-2 data PLP, cut into num_subslices sub-slices (8.3.6.3);
   *   ti_type   TIME_IL_TYPE (6.5): 0 = one interleaving frame of fecblocks FEC blocks in tiblocks TI
   *             blocks per T2 frame (the reference's); 1 = one TI block (tiblocks must be 1) of fecblocks
   *             FEC blocks per interleaving frame, spread over ti_frames = P_I consecutive T2 frames
   *             (TIME_IL_LENGTH = P_I, FRAME_INTERVAL 1): T2 frame i of interleaving frame m (frames
   *             m P_I + i) carries TI output cells [i D, (i + 1) D), D = fecblocks x cell size / P_I;
   *   ti_frames P_I (0 is read as 1; must be 1 for ti_type 0; fecblocks x cell size divisible by it);
   *   frame_interval  FRAME_INTERVAL = I_JUMP (7.2.3.1; 0 is read as 1): the PLP occurs only in the T2 frames f
   *             with f mod I_JUMP = first_frame_idx (FIRST_FRAME_IDX < I_JUMP), its interleaving frame spanning
   *             P_I of them; t2frames must be a multiple of P_I x I_JUMP.  A T2 frame carries only its PLPs
   *             (the others' L1-post PLP_START and PLP_NUM_BLOCKS are 0), dummy cells fill the rest.
   * fecblocks is then PLP_NUM_BLOCKS: the FEC blocks of one interleaving frame. */
  int plp_type, ti_type, ti_frames, frame_interval, first_frame_idx;
} dvbt2ll_plp_params;
typedef struct {
  /* the common (frame, L1, OFDM) fields of framemapperfint_cc::make */
  int carriermode, fftsize, guardinterval, l1constellation, pilotpattern, t2frames, numdatasyms, paprmode,
      version, preamble, reservedbiasbits, l1scrambled;
  int nplp;                                  /* 1 .. DVBT2LL_MAX_PLP */
  dvbt2ll_plp_params plp[DVBT2LL_MAX_PLP];   /* plp[k]: PLP_ID k */
  /* SUB_SLICES_PER_FRAME of the Type-2 PLPs (0 is read as 1; must be 1 without Type-2 PLPs): the frame's
   * data cells are the Type-1 PLPs back to back in PLP_ID order, then sub-slice 0 of every Type-2 PLP
   * (PLP_ID order), sub-slice 1 of every Type-2 PLP, ...; each Type-2 PLP's cells per T2 frame divisible
   * by it.  A chain whose PLPs have interleaving frames of several T2 frames or FRAME_INTERVAL > 1 runs whole
   * launch units: first_frame and nframes multiples of the least common multiple of the PLPs' P_I x I_JUMP
   * (dvbt2ll_chain_unit_frames). */
  int num_subslices;
} dvbt2ll_mplp_params;

/* one PLP of a multi-PLP frame: the BBHEADER of every later BBFRAME says MATYPE SIS/MIS = multiple
 * input streams and MATYPE-2 (ISI) = isi (the PLP_ID), the MIS branch of the reference's add_bbheader
 * (lib/bbheaderbch_bb_impl.cc:288-298) that its ctor never selects (:168) */
int dvbt2ll_bbheaderbch_set_isi(dvbt2ll_bbheaderbch *h, int isi);

/* framemapperfint_cc with one input port per PLP (the per-PLP bbheaderbch -> ldpc -> interleavermod
 * chains feed port k with PLP k's cells): one T2 frame per general_work call, consuming
 * stream_items(k) cells from every port (framemapper:1942-1946, 2147 per port); a TIME_IL_TYPE 1 PLP's port
 * instead delivers its whole interleaving frame (fecblocks x cell size cells) on the interleaving frame's
 * first T2 frame and nothing on the other P_I - 1 (forecast and consumed say so per port) */
typedef struct dvbt2ll_framemapper_mplp dvbt2ll_framemapper_mplp;
int dvbt2ll_framemapper_mplp_create(const dvbt2ll_mplp_params *p, int device, dvbt2ll_framemapper_mplp **out);
int dvbt2ll_framemapper_mplp_output_multiple(const dvbt2ll_framemapper_mplp *h);     /* mapped_items */
int dvbt2ll_framemapper_mplp_stream_items(const dvbt2ll_framemapper_mplp *h, int plp);
/* nin_required[k] for each of the nplp ports */
int dvbt2ll_framemapper_mplp_forecast(const dvbt2ll_framemapper_mplp *h, int noutput_items, int *ninput_items_required);
/* in[k], ninput_items[k]: port k's cells (host complex64); consumed[k] per port */
int dvbt2ll_framemapper_mplp_general_work(dvbt2ll_framemapper_mplp *h, int noutput_items, const int *ninput_items,
                                          const void *const *in, void *out, int *consumed);
void dvbt2ll_framemapper_mplp_destroy(dvbt2ll_framemapper_mplp *h);

/* fused chain of a multi-PLP frame: every PLP's TS -> BBFRAME/BCH/LDPC -> map, one frame's OFDM */
typedef struct {
  dvbt2ll_mplp_params fm;
  int misogroup, equalization, bandwidth;
  int max_frames;
} dvbt2ll_mplp_chain_params;
int dvbt2ll_chain_create_mplp(const dvbt2ll_mplp_chain_params *p, int device, dvbt2ll_chain **out);
int dvbt2ll_chain_num_plps(const dvbt2ll_chain *h);
/* T2 frames of the chain's launch unit: the least common multiple of its PLPs' P_I x FRAME_INTERVAL
 * (1 for the reference's PLPs).  Every run's first_frame and nframes are multiples of it (else
 * DVBT2LL_EINVAL); create fails when max_frames is smaller. */
int dvbt2ll_chain_unit_frames(const dvbt2ll_chain *h);
/* PLP plp's FEC blocks, payload and TS bytes per frame, cell size, cells per frame (stream_items) and
 * codeword stride; the frame-wide fields as dvbt2ll_chain_get_info (which reports PLP 0's) */
int dvbt2ll_chain_get_plp_info(const dvbt2ll_chain *h, int plp, dvbt2ll_chain_info *info);
/* ts_dev[k], ts_base[k], ts_len[k]: PLP k's TS, laid out as run_device's (host arrays of nplp entries);
 * frames [first_frame, first_frame + nframes) into iq_dev (aligned to one output sample, as
 * run_device's: 8 bytes for DVBT2LL_IQ_CF32, 4 for DVBT2LL_IQ_SC16).  Asynchronous on stream.  run_device on a
 * one-PLP chain == run_plps with one entry. */
int dvbt2ll_chain_run_plps(dvbt2ll_chain *h, const void *const *ts_dev, const int64_t *ts_base,
                           const int64_t *ts_len, int64_t first_frame, int nframes, void *iq_dev, void *stream);
/* run_plps with host buffers (each PLP's TS copied to the device, IQ copied back), synchronous */
int dvbt2ll_chain_run_plps_host(dvbt2ll_chain *h, const void *const *ts, const int64_t *ts_base, const int64_t *ts_len,
                                int64_t first_frame, int nframes, void *iq);
/* test hook: PLP plp's packed codewords of the last run's frame 0 (as dvbt2ll_chain_debug_codewords) */
int dvbt2ll_chain_debug_plp_codewords(dvbt2ll_chain *h, int plp, void *out, int64_t bytes);

/* ---------------------------------------------------------------------------
 * MISO pair chain: both transmitter groups of one MISO service from one FEC + map pass.  A pair handle encodes
 * each frame once (one BB + BCH launch and one LDPC + map launch per PLP, with the L1-post workgroups) and runs
 * two OFDM launches over the same index-pair buffer and L1-post cells: group 1's output is bit-identical to a
 * MISO_TX1 handle's, group 2's to a DVBT2LL_MISO_TX2_PROCESSED handle's.  The pair buffer is in group 1's slot
 * order; group 2's launch reads it through tables of its own and is not bank-balanced for its own bins.
 * p->misogroup must be MISO_TX1 (0) and the preamble a MISO one, else DVBT2LL_EINVAL.
 * On a pair handle set_output, set_slots, set_timing (stage 2 accumulates both OFDM launches), sync_errors (each
 * packet counted once), get_info and the debug hooks (dvbt2ll_chain_debug_cell_pairs / _cells: group 1's slot
 * order) work as on any chain; a buffer slot reused on another stream waits for both OFDM launches of its
 * previous run.  Not supported on a pair handle, DVBT2LL_EINVAL with nothing launched: the single-output run
 * calls (run_device, run_streams, run_plps, the host and streaming-host calls) and set_graph(1): graph mode and
 * the streaming host ring are out of scope for pair handles.
 * ------------------------------------------------------------------------- */
int dvbt2ll_chain_create_miso_pair(const dvbt2ll_chain_params *p, int device, dvbt2ll_chain **out);
int dvbt2ll_chain_create_mplp_miso_pair(const dvbt2ll_mplp_chain_params *p, int device, dvbt2ll_chain **out);
int dvbt2ll_chain_num_groups(const dvbt2ll_chain *h);   /* 2 for a pair handle, else 1 */
/* as dvbt2ll_chain_run_streams (single-PLP) / dvbt2ll_chain_run_plps (multi-PLP), with one IQ buffer per group:
 * iq_dev[0] = group 1 (a MISO_TX1 handle's output), iq_dev[1] = group 2 (a MISO_TX2_PROCESSED handle's), each
 * laid out and aligned as run_streams' iq_dev.  One of the two may be NULL: that group's OFDM launch is skipped.
 * DVBT2LL_EINVAL with nothing launched: an ordinary handle, both pointers NULL, a misaligned pointer. */
int dvbt2ll_chain_run_groups(dvbt2ll_chain *h, const void *ts_dev, int64_t ts_stride, int nstreams, int64_t ts_base,
                             int64_t ts_len, int64_t first_frame, int nframes, void *const iq_dev[2], void *stream);
int dvbt2ll_chain_run_plps_groups(dvbt2ll_chain *h, const void *const *ts_dev, const int64_t *ts_base,
                                  const int64_t *ts_len, int64_t first_frame, int nframes, void *const iq_dev[2],
                                  void *stream);

/* ---------------------------------------------------------------------------
 * T2-MI input (ETSI TS 102 773 over DVB data piping): a device buffer of 188-byte TS packets -> per-PLP packed
 * BBFRAME streams in the layout DVBT2LL_INPUT_BBFRAME reads (L = kbch / 8 bytes per block, back to back), a packet
 * table and counters.  A handle of its own beside the chain: it holds scratch, no stream state, and composes with
 * every run form.  The reference has no T2-MI code: PARITY UNPINNED, pinned by tests/t2mi_ref.py's sequential
 * restatement and known answers.
 *
 * TS layer   packets of PID pid with a payload (AFC 01: bytes 4 .. 187; AFC 11: bytes 5 + a .. 187, a = byte 4),
 *            TEI = 0 and scrambling = 0 contribute; with PUSI the first payload byte is the pointer_field p, which
 *            is removed.  The remaining payloads, concatenated, are the T2-MI byte stream.  A contributing packet
 *            whose continuity counter is not its predecessor's + 1 mod 16 is a discontinuity at its first stream
 *            byte (the first contributing packet of a call has no predecessor).
 * packets    6 header bytes (packet_type 8, packet_count 8, superframe_idx 4, rfu 9, t2mi_stream_id 3,
 *            payload_len 16 in bits), ceil(payload_len / 8) payload bytes, CRC-32/MPEG-2 of all of it: T = 10 +
 *            ceil(payload_len / 8) bytes.  Type 0x00: frame_idx 8, plp_id 8, intl_frame_start 1, rfu 7, BBFRAME.
 * starts     p bytes into a contributing PUSI packet's stripped payload (p past its end: counted in bad_pointers,
 *            no start); and, where the packet at a start ends inside the same TS packet's payload, the next byte.
 * a packet   at start s is complete when s + T <= the stream length; consistent when no other start lies in
 *            (s, s + T) and no discontinuity in (s, s + T) (one exactly at s is a packet that begins a TS packet
 *            after a loss: intact, and a call that resumes there could not see it); accepted when complete,
 *            consistent, the CRC matches and (stream_id < 0 or t2mi_stream_id == stream_id).
 * output     an accepted type-0 packet of mapped plp_id[o] with payload_len == 24 + 8 bbframe_bytes[o] is block n
 *            of out_dev[o], n = its rank among such packets of the call; otherwise len_errors / other_plp.
 * prefix     the call emits (table, outputs, counters) the longest prefix of packets in stream order in which
 *            every packet is complete, no output's capacity and not max_packets is exceeded.  The resume position
 *            is the byte offset of the TS packet holding the first packet not emitted and the number of starts in
 *            that TS packet already emitted; (ts_len, 0) when nothing is left (a call whose start is at ts_len
 *            returns its start).  The TS-level counters count the TS packets before the resume position, so every
 *            counter adds up over chained calls -- except a discontinuity at a call's first contributing packet.
 * bounds     nothing outside [ts_dev, ts_dev + ts_len) is read, nothing outside out_cap_blocks[o] blocks of
 *            out_dev[o] is written, whatever the stream's length fields say.
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_t2mi dvbt2ll_t2mi;
typedef struct {
  int pid;                               /* 0 .. 0x1FFE */
  int stream_id;                         /* -1: any; 0 .. 7: accept only this t2mi_stream_id */
  int nplp;                              /* 1 .. DVBT2LL_MAX_PLP outputs */
  int plp_id[DVBT2LL_MAX_PLP];           /* 0 .. 255, distinct */
  int bbframe_bytes[DVBT2LL_MAX_PLP];    /* L = kbch / 8 of one of the standard's 14 codes */
  int64_t max_ts_bytes;                  /* largest ts_len of a run, a multiple of 188 below 2^31 */
  int max_packets;                       /* table capacity: T2-MI packets emitted per run */
} dvbt2ll_t2mi_params;
typedef struct {
  int64_t ts_offset;                     /* a multiple of 188 in [0, ts_len] */
  int skip;                              /* starts of that TS packet already emitted */
} dvbt2ll_t2mi_pos;
/* one table record, 24 bytes, little-endian; ts_index / ts_byte are in ts_dev's coordinates */
#define DVBT2LL_T2MI_COMPLETE 1
#define DVBT2LL_T2MI_CONSISTENT 2
#define DVBT2LL_T2MI_CRC_OK 4
#define DVBT2LL_T2MI_ACCEPTED 8
typedef struct {
  uint32_t ts_index;                     /* TS packet holding the T2-MI packet's first byte */
  uint32_t ts_byte;                      /* byte offset of that first byte in the TS buffer */
  uint8_t packet_type, packet_count, superframe_idx, t2mi_stream_id;
  uint16_t payload_len;                  /* bits */
  uint8_t flags;                         /* DVBT2LL_T2MI_* */
  uint8_t intl_frame_start;              /* type 0x00 with payload_len >= 24 (else 0, as the next two) */
  uint8_t frame_idx, plp_id;
  int8_t out_index;                      /* output written, or -1 */
  uint8_t reserved;
  int32_t block;                         /* block rank in that output, or -1 */
} dvbt2ll_t2mi_packet;
typedef struct {
  dvbt2ll_t2mi_pos resume;
  int64_t packets;                       /* table records of the call */
  int64_t ts_contributing, ts_foreign, ts_null, ts_tei, ts_scrambled, ts_bad_sync, ts_no_payload, discontinuities,
      bad_pointers;
  int64_t broken, crc_errors, filtered, len_errors, other_plp, accepted;
  int64_t blocks[DVBT2LL_MAX_PLP];       /* blocks written per output */
  int64_t by_type[256];                  /* table records per packet_type */
} dvbt2ll_t2mi_result;
int dvbt2ll_t2mi_create(const dvbt2ll_t2mi_params *p, int device, dvbt2ll_t2mi **out);
/* fills nplp, plp_id[k] = plp_ids[k] (NULL: k) and bbframe_bytes[k] from the chain's PLP k; the other fields stay */
int dvbt2ll_t2mi_params_from_chain(const dvbt2ll_chain *chain, const int *plp_ids, dvbt2ll_t2mi_params *p);
/* ts_dev: ts_len bytes (a multiple of 188, <= max_ts_bytes) on the device; start: (0, 0) or a previous call's resume
 * position for this buffer; out_dev[o]: room for out_cap_blocks[o] blocks of bbframe_bytes[o].  Asynchronous on
 * stream (NULL: the handle's own); no host round trip.  One run of a handle at a time: the next run call on another
 * stream first waits for the previous one.  DVBT2LL_EINVAL, nothing launched: ts_len not a multiple of 188 or above
 * max_ts_bytes, start outside the buffer or off a packet boundary, skip < 0, a negative capacity, a null pointer. */
int dvbt2ll_t2mi_run_device(dvbt2ll_t2mi *h, const void *ts_dev, int64_t ts_len, const dvbt2ll_t2mi_pos *start,
                            void *const *out_dev, const int64_t *out_cap_blocks, void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_t2mi_get_result(dvbt2ll_t2mi *h, dvbt2ll_t2mi_result *res);
/* the last run's table: up to max_records records to host memory; returns the number copied, or a negative status */
int64_t dvbt2ll_t2mi_get_packets(dvbt2ll_t2mi *h, dvbt2ll_t2mi_packet *out, int64_t max_records);
/* host buffers, synchronous: the TS is copied in, each output's written blocks are copied out */
int dvbt2ll_t2mi_run_host(dvbt2ll_t2mi *h, const void *ts, int64_t ts_len, const dvbt2ll_t2mi_pos *start,
                          void *const *out, const int64_t *out_cap_blocks, dvbt2ll_t2mi_result *res);
void dvbt2ll_t2mi_destroy(dvbt2ll_t2mi *h);

/* ---------------------------------------------------------------------------
 * Mode adapter (EN 302 755 5.1.4, 5.1.7): a device buffer of 188-byte TS packets -> one PLP's packed BBFRAMEs in
 * high-efficiency mode, with null-packet deletion and an optional PID selection, in the layout
 * DVBT2LL_INPUT_BBFRAME reads (L = kbch / 8 bytes per BBFRAME, back to back).  A handle of its own beside the chain:
 * it holds scratch, no stream state, and composes with every run form.  Scope: high-efficiency mode only (no sync
 * byte, no CRC-8 in the stream; UPL = SYNC = 0).  Not built: null-packet deletion in normal mode, ISSY (ISCR / BUFS
 * / TTO), in-band type A, the common PLP (GSE: dvbt2ll_gse_* below).  With npd = 0 the output is the reference's HEM BBFRAME stream of the
 * same TS byte for byte (in-band off); the reference sets NPD = 0 (lib/bbheaderbch_bb_impl.cc:272-325), so npd = 1 is
 * PARITY UNPINNED, pinned by tests/modeadapt_ref.py's sequential restatement and its receiver.
 *
 * input      whole 188-byte packets; a length that is not a multiple of 188 is refused before any launch.
 * classes    npd = 1: a packet is selected when its PID is in pid_mask (NULL: every PID) and is not 0x1FFF; every
 *            other packet is null.  npd = 0: every packet is selected (a mask is refused: without deletion the
 *            unselected packets have nowhere to go).  A first byte other than 0x47 is counted in sync_errors and the
 *            packet is otherwise treated normally (bbheaderbch_bb_impl.cc:675).
 * DNP        (npd = 1) the nulls of a maximal run are numbered r = 0, 1, ...; the null with r % 256 == 255 is kept:
 *            it is transmitted as a user packet holding the null packet (47 1F FF 10, 184 x FF, whatever the packet
 *            held: another PLP's bytes never leak), and the count restarts after it.  Every other null is deleted.
 *            A transmitted packet's DNP byte is the number of nulls deleted since the previous transmitted packet:
 *            255 for a kept null, n % 256 for a selected packet after a run of n nulls.
 * units      each transmitted packet contributes its bytes 1 .. 187 (the sync byte is dropped), then with npd = 1
 *            its DNP byte: units of U = 188 (npd = 1) or 187 (npd = 0) bytes, back to back.
 * BBFRAMEs   D = (kbch - 80) / 8 data-field bytes each; BBFRAME k's data field is unit-stream bytes [k D, (k + 1) D).
 *            Header: MATYPE-1 = TS_GS 11, SIS/MIS, CCM 1, ISSYI 0, NPD = npd, EXT 00; MATYPE-2 = the ISI (MIS) or 0;
 *            UPL 0; DFL 8 D; SYNC 0; SYNCD = 8 x the bytes from the data field's start to the first unit that begins
 *            in it (0 when one begins at byte 0, 0xFFFF when none does); CRC-8 XOR 1 (MODE = high efficiency), the
 *            byte the chain's own HEM header has: dvbt2ll_chain_bbheader_errors counts none.
 * capacity   a call emits the largest number of whole BBFRAMEs that the input and out_cap_blocks allow, and returns
 *            resume = {ts_packet, unit_byte, dnp}: the index, in this call's buffer, of the transmitted packet whose
 *            unit holds the first unit-stream byte not emitted, how many of that unit's bytes were emitted, and that
 *            unit's DNP.  If the emitted bytes end exactly with the call's last unit, resume is the packet after the
 *            last transmitted one (the call's start packet when none was) with unit_byte = dnp = 0: trailing nulls
 *            are seen again, as the start of a run.  The next call passes resume as start, with a buffer that begins
 *            at or before that packet (start.ts_packet = its index there).  A start with unit_byte > 0 or dnp > 0
 *            makes that packet transmitted unconditionally with that DNP (it may be a kept null) and must name a
 *            packet of the buffer.  Chained calls at any split produce the single call's bytes, and their counters
 *            add up.
 * flush      flush = 1 is honoured when the whole BBFRAMEs and the flush frame fit out_cap_blocks: one more BBFRAME
 *            carries the remaining bytes (DFL = 8 x their count, SYNCD by the rule above, the rest of the data field
 *            zero; none when nothing remains), the nulls after the last transmitted packet are dropped and counted
 *            in nulls_dropped_at_flush (not in nulls_deleted), and resume is {packets of the buffer, 0, 0}.
 * counters   cover exactly the packets from start.ts_packet to before resume.ts_packet; bbframes includes the flush
 *            frame, flushed is 1 when one was written.
 * bounds     nothing outside [ts_dev, ts_dev + ts_len) is read, nothing outside out_cap_blocks BBFRAMEs of out_dev
 *            is written.
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_modeadapt dvbt2ll_modeadapt;
typedef struct {
  int kbch;                              /* a T2 code's Kbch: one of the chain's 14, or 3072 (short 1/4, which the
                                            chain does not encode); 0: taken from framesize / rate */
  int framesize, rate;                   /* FECFRAME_* / C*: used when kbch == 0 */
  int sis_mis;                           /* 1: single input stream; 0: multiple, MATYPE-2 = isi (0 .. 255) */
  int isi;
  int npd;                               /* 0 / 1 */
  const uint8_t *pid_mask;               /* NULL, or 1024 bytes: PID p is bit p & 7 of byte p >> 3 (copied at create) */
  int64_t max_ts_bytes;                  /* largest ts_len of a run, a multiple of 188 below 2^31 */
} dvbt2ll_modeadapt_params;
typedef struct {
  int64_t ts_packet;                     /* a packet index in [0, ts_len / 188] */
  int unit_byte;                         /* 0 .. U - 1 bytes of that packet's unit already emitted */
  int dnp;                               /* 0 .. 255: that unit's DNP (0 with npd = 0) */
} dvbt2ll_modeadapt_pos;
typedef struct {
  dvbt2ll_modeadapt_pos resume;
  int64_t packets_in, selected, nulls_deleted, nulls_kept, nulls_dropped_at_flush, sync_errors, bbframes, flushed;
} dvbt2ll_modeadapt_result;
int dvbt2ll_modeadapt_create(const dvbt2ll_modeadapt_params *p, int device, dvbt2ll_modeadapt **out);
/* fills kbch, sis_mis and isi from the chain's PLP plp (a multi-PLP chain's headers say MIS with ISI = the PLP's
 * index); the other fields stay */
int dvbt2ll_modeadapt_params_from_chain(const dvbt2ll_chain *chain, int plp, dvbt2ll_modeadapt_params *p);
/* ts_dev: ts_len bytes (a multiple of 188, <= max_ts_bytes) on the device; start: {0, 0, 0} or a previous call's
 * resume position in this buffer's packet indices; out_dev: room for out_cap_blocks BBFRAMEs of kbch / 8 bytes.
 * Asynchronous on stream (NULL: the handle's own); no host round trip.  One run of a handle at a time: the next run
 * call on another stream first waits for the previous one.  DVBT2LL_EINVAL, nothing launched: ts_len not a multiple
 * of 188 or above max_ts_bytes, start outside the buffer, unit_byte outside 0 .. U - 1, dnp outside 0 .. 255 (or not 0
 * with npd = 0), unit_byte > 0 or dnp > 0 at the buffer's end, a negative capacity, a null pointer. */
int dvbt2ll_modeadapt_run_device(dvbt2ll_modeadapt *h, const void *ts_dev, int64_t ts_len,
                                 const dvbt2ll_modeadapt_pos *start, void *out_dev, int64_t out_cap_blocks, int flush,
                                 void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_modeadapt_get_result(dvbt2ll_modeadapt *h, dvbt2ll_modeadapt_result *res);
/* host buffers, synchronous: the TS is copied in, the written BBFRAMEs are copied out */
int dvbt2ll_modeadapt_run_host(dvbt2ll_modeadapt *h, const void *ts, int64_t ts_len, const dvbt2ll_modeadapt_pos *start,
                               void *out, int64_t out_cap_blocks, int flush, dvbt2ll_modeadapt_result *res);
void dvbt2ll_modeadapt_destroy(dvbt2ll_modeadapt *h);

/* ---------------------------------------------------------------------------
 * ULE encapsulator (RFC 4326): a device buffer of PDUs (IP datagrams) and a device offset table -> 188-byte TS
 * packets that the chain's TS input, the mode adapter and dvbt2ll_tx take as they are: the data path of the
 * reference flowgraph's source block (gr-ule's ule_source in apps/vv009-4kshort.grc).  A handle of its own beside the
 * chain: it holds scratch, no stream state.  Not built: ULE extension headers and bridged frames (Type is an opaque
 * 16-bit field), per-PDU destination addresses, adaptation-field stuffing, the TAP interface, PSI / SI (GSE:
 * dvbt2ll_gse_* below).
 * gr-ule is not part of the reference tree, so all of this is PARITY UNPINNED, pinned by tests/ule_ref.py's
 * sequential restatement and its RFC 4326 section 7 receiver.
 *
 * input      pdu_dev holds pdu_len bytes (below 2^31); off_dev holds n_pdus + 1 uint32_t offsets: PDU i is bytes
 *            [off[i], off[i + 1]).  type_dev is optional: n_pdus uint16_t Type fields.  With type_dev == NULL the
 *            Type comes from the PDU's first nibble: 4 -> 0x0800, 6 -> 0x86DD; any other nibble: the PDU is skipped
 *            and counted in skipped_type.  A PDU is skipped and counted in skipped_len when off[i + 1] <= off[i],
 *            or off[i + 1] > pdu_len, or the SNDU Length would exceed 32767 (the length is judged first: such a PDU
 *            is never counted in skipped_type).  A skipped PDU contributes nothing; every rule below speaks of the
 *            remaining (valid) PDUs only.  Nothing outside [pdu_dev, pdu_dev + pdu_len) and the two tables is read,
 *            whatever the offsets say.  The offsets need not ascend: valid PDUs may overlap or repeat, each is
 *            encapsulated as it stands, and the packets may then be more than the buffer's bytes suggest.
 * SNDU       (RFC 4326 section 4) in order: the D bit (d_bit); Length, 15 bits: the bytes after the Type field up to
 *            and including the CRC = (d_bit ? 0 : 6) + pdu_bytes + 4; Type, 16 bits; the 6-byte destination address
 *            dest when d_bit == 0; the PDU; CRC-32 (polynomial 0x04C11DB7, initial value 0xFFFFFFFF, no reflection,
 *            no final XOR: the CRC the T2-MI deframer checks) over every SNDU byte before it, big-endian.  The SNDU
 *            has n = 4 + Length bytes; the smallest has 9.
 * TS packets sync 47, TEI 0, PUSI, priority 0, pid, scrambling 00, adaptation field control 01; the continuity
 *            counter is start.cc, plus one mod 16 per emitted packet; 184 payload bytes.  With PUSI = 1 the first
 *            payload byte is the Payload Pointer PP: the payload bytes between it and the first SNDU that starts in
 *            the packet.
 * packing=1  when a packet begins, R is the number of bytes of the current SNDU not yet sent (0: the packet begins
 *            with a new SNDU); "next": another valid SNDU follows in this call.
 *              R >= 184: PUSI 0, 184 SNDU bytes.   R = 183: PUSI 0, 183 bytes, FF.   R = 182: PUSI 0, 182 bytes,
 *              FF FF (the End Indicator).
 *              R <= 181 and next: PUSI 1, PP = R, the R bytes, then SNDUs back to back: a new SNDU starts while at
 *              least 2 payload bytes are free and next exists (one that does not fit runs on into the following
 *              packets, to which this list applies again); an SNDU ending with exactly 1 byte free is followed by FF
 *              and the packet is closed; one ending on the last byte closes the packet.
 *              0 < R <= 181, no next, flush = 1: PUSI 0, R bytes, the rest FF.   R = 0, no next: no packet.
 *              A PUSI packet left with free bytes and no next: with flush = 1 it is filled with FF (the first two are
 *              the End Indicator); without flush it is not emitted.
 * packing=0  one SNDU per packet start.  R = 0: PUSI 1, PP 0, up to 183 SNDU bytes, the rest FF.  R > 0: PUSI 0,
 *            min(R, 184) bytes, the rest FF.  Every packet is determined by its own SNDU; flush changes nothing
 *            except flushed.
 * capacity   a call emits the longest prefix of determined packets that fits out_cap_packets and returns resume =
 *            {pdu, sndu_byte, cc}: the index of the PDU whose SNDU holds the first SNDU byte not emitted, how many of
 *            that SNDU's bytes were emitted, the counter of the next packet; {n_pdus, 0, cc} when nothing is left.
 *            The next call passes resume as start, with a PDU list that begins at or before that PDU.  A start with
 *            sndu_byte > 0 begins with R = n - sndu_byte of that SNDU, whose CRC is computed again (a sndu_byte that
 *            is not below n, or at a skipped PDU, is taken as 0).  Chained calls at any split produce the single
 *            call's bytes.
 * counters   pdus_in, sndus, skipped_len, skipped_type cover the PDUs from start.pdu to before resume.pdu, so they
 *            add up over chained calls; ts_packets, pusi_packets and pad_bytes (the FF bytes; a PP is none) cover the
 *            packets emitted; flushed is 1 when flush was set and nothing is left.
 * bounds     nothing outside out_cap_packets x 188 bytes of out_dev is written.
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_ule dvbt2ll_ule;
typedef struct {
  int pid;                               /* 0 .. 0x1FFE */
  int d_bit;                             /* 0: every SNDU carries dest; 1: none does */
  uint8_t dest[6];                       /* the destination address (the flowgraph's 02:00:48:55:4c:4b) */
  int packing;                           /* 0 / 1 */
  int64_t max_pdu_bytes;                 /* largest pdu_len of a run, 1 .. 2^31 - 1 */
  int max_pdus;                          /* largest n_pdus of a run, 1 .. 2^24 */
} dvbt2ll_ule_params;
typedef struct {
  int64_t pdu;                           /* a PDU index in [0, n_pdus] */
  int sndu_byte;                         /* bytes of that PDU's SNDU already emitted */
  int cc;                                /* 0 .. 15: the next packet's continuity counter */
} dvbt2ll_ule_pos;
typedef struct {
  dvbt2ll_ule_pos resume;
  int64_t pdus_in, sndus, skipped_len, skipped_type, ts_packets, pusi_packets, pad_bytes, flushed;
} dvbt2ll_ule_result;
/* DVBT2LL_EINVAL: a null pointer, pid / d_bit / packing / the maxima out of range; DVBT2LL_EDEVICE without a GPU */
int dvbt2ll_ule_create(const dvbt2ll_ule_params *p, int device, dvbt2ll_ule **out);
/* pdu_dev, off_dev, type_dev (or NULL) on the device; start: {0, 0, cc} or a previous call's resume position in this
 * list's PDU indices; out_dev: room for out_cap_packets x 188 bytes.  Asynchronous on stream (NULL: the handle's
 * own); no host round trip.  One run of a handle at a time: the next run call on another stream first waits for the
 * previous one.  DVBT2LL_EINVAL, nothing launched: a null pointer (type_dev may be), pdu_len or n_pdus negative or
 * above the create-time maxima, a negative capacity, start.pdu outside [0, n_pdus], sndu_byte negative or > 0 at
 * n_pdus, cc outside 0 .. 15. */
int dvbt2ll_ule_run_device(dvbt2ll_ule *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                           const uint16_t *type_dev, int64_t n_pdus, const dvbt2ll_ule_pos *start, void *out_dev,
                           int64_t out_cap_packets, int flush, void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_ule_get_result(dvbt2ll_ule *h, dvbt2ll_ule_result *res);
/* host buffers, synchronous: the PDUs and tables are copied in, the written packets are copied out.  The device
 * output buffer holds out_cap_packets, or what n_pdus PDUs inside pdu_len bytes can become at the most if that is
 * less. */
int dvbt2ll_ule_run_host(dvbt2ll_ule *h, const void *pdu, int64_t pdu_len, const uint32_t *off, const uint16_t *type,
                         int64_t n_pdus, const dvbt2ll_ule_pos *start, void *out, int64_t out_cap_packets, int flush,
                         dvbt2ll_ule_result *res);
void dvbt2ll_ule_destroy(dvbt2ll_ule *h);

/* ---------------------------------------------------------------------------
 * MPE encapsulator (Multi-Protocol Encapsulation, EN 301 192 clause 7): a device buffer of IP datagrams and a device
 * offset table -> DSM-CC datagram_sections in 188-byte TS packets that the chain's TS input, the mode adapter and
 * dvbt2ll_tx take as they are: the encapsulation DVB itself specifies for IP over a transport stream, the one deployed
 * IP-over-DVB receivers and TS analysers read.  A handle of its own beside the chain: it holds scratch, no stream
 * state.  Not built: LLC/SNAP, section_number > 0 (a datagram split over several sections), the checksum form
 * (section_syntax_indicator 0), scrambling, time slicing, INT / PSI tables, adaptation-field stuffing (MPE-FEC: the
 * dvbt2ll_mpefec handle below).
 * The reference has no MPE code, so all of this is PARITY UNPINNED, pinned by tests/mpe_ref.py's sequential
 * restatement and its ISO/IEC 13818-1 section receiver.
 *
 * input      as the ULE handle's: pdu_dev holds pdu_len bytes (below 2^31); off_dev holds n_pdus + 1 uint32_t
 *            offsets: PDU i is bytes [off[i], off[i + 1]), p bytes.  A PDU is skipped and counted in skipped_len when
 *            off[i + 1] <= off[i], or off[i + 1] > pdu_len, or p > 4080 (a whole section is at most 4096 bytes); the
 *            length is judged first.  It is skipped and counted in skipped_type when its first nibble is neither 4 nor
 *            6: MPE without LLC/SNAP carries IP only, and there is no type table.  A skipped PDU contributes nothing;
 *            every rule below speaks of the remaining (valid) PDUs only.  Nothing outside [pdu_dev, pdu_dev + pdu_len)
 *            and the offset table is read, whatever the offsets say.  The offsets need not ascend: valid PDUs may
 *            overlap or repeat, each is encapsulated as it stands, and the packets may then be more than the buffer's
 *            bytes suggest.
 * section    n = 12 + p + 4 bytes, section_length = n - 3; the smallest has 17 bytes.
 *              byte 0        3E (table_id)
 *              byte 1        B0 | (section_length >> 8): section_syntax_indicator 1, private_indicator 0, reserved 11,
 *                            the length's high 4 bits
 *              byte 2        section_length & FF
 *              byte 3, 4     MAC_address_6, MAC_address_5: the address's last byte, then the one before it
 *              byte 5        C1: reserved 11, payload_scrambling_control 00, address_scrambling_control 00,
 *                            LLC_SNAP_flag 0, current_next_indicator 1
 *              byte 6, 7     section_number 0, last_section_number 0
 *              byte 8 .. 11  MAC_address_4, _3, _2, _1: byte 11 is the address's first byte
 *              byte 12 ..    the datagram
 *              last 4        CRC_32, big-endian, over every section byte before it (polynomial 0x04C11DB7, initial
 *                            value 0xFFFFFFFF, no reflection, no final XOR: the CRC the ULE encapsulator writes and
 *                            the T2-MI deframer checks)
 * MAC        mac_mode 0: every section carries mac.  mac_mode 1: an IPv4 datagram (first nibble 4) of at least 20
 *            bytes whose byte 16 is in 224 .. 239 carries 01:00:5e:(b17 & 7f):b18:b19; an IPv6 datagram (first nibble
 *            6) of at least 40 bytes whose byte 24 is ff carries 33:33:b36:b37:b38:b39; any other carries mac.
 * TS packets sync 47, TEI 0, PUSI, priority 0, pid, scrambling 00, adaptation_field_control 01; the continuity
 *            counter is start.cc, plus one mod 16 per emitted packet; 184 payload bytes.  With PUSI = 1 the first
 *            payload byte is the pointer_field: the payload bytes between it and the first section that starts in the
 *            packet.
 * packing=1  when a packet begins, R is the number of bytes of the current section not yet sent (0: the packet begins
 *            with a new section); "next": another valid section follows in this call.
 *              R >= 184: PUSI 0, 184 section bytes.   R = 183: PUSI 0, 183 bytes, FF (no pointer_field can point
 *              inside the packet).
 *              R <= 182 and next: PUSI 1, pointer_field R, the R bytes, then sections back to back: a new section
 *              starts while at least one payload byte is free and next exists (its header may straddle into the
 *              following packets, to which this list applies again); a section ending on the packet's last byte
 *              closes the packet.
 *              0 < R <= 183, no next, flush = 1: PUSI 0, R bytes, the rest FF.   R = 0, no next: no packet.
 *              A PUSI packet left with free bytes and no next: with flush = 1 it is filled with FF; without flush it
 *              is not emitted (its content depends on whether a section follows).
 * packing=0  every section starts a packet behind pointer_field 0, with up to 183 bytes and the rest FF; later
 *            packets of the same section have PUSI 0, min(R, 184) bytes and the rest FF.  A section takes
 *            ceil((n + 1) / 184) packets.  Flush changes nothing except flushed.
 * capacity   a call emits the longest prefix of determined packets that fits out_cap_packets and returns resume =
 *            {pdu, section_byte, cc}: the index of the PDU whose section holds the first section byte not emitted,
 *            how many of that section's bytes were emitted, the counter of the next packet; {n_pdus, 0, cc} when
 *            nothing is left.  The next call passes resume as start, with a PDU list that begins at or before that
 *            PDU.  A start with section_byte > 0 begins with R = n - section_byte of that section, whose CRC is
 *            computed again (a section_byte that is not below n, or at a skipped PDU, is taken as 0).  Chained calls
 *            at any split produce the single call's bytes.
 * counters   pdus_in, sections, skipped_len, skipped_type, mapped_macs (the sections whose MAC came from the
 *            datagram) cover the PDUs from start.pdu to before resume.pdu, so they add up over chained calls;
 *            ts_packets, pusi_packets and pad_bytes (the FF bytes; a pointer_field is none) cover the packets emitted;
 *            flushed is 1 when flush was set and nothing is left.
 * bounds     nothing outside out_cap_packets x 188 bytes of out_dev is written.
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_mpe dvbt2ll_mpe;
typedef struct {
  int pid;                               /* 0 .. 0x1FFE */
  uint8_t mac[6];                        /* the MAC address, first byte first */
  int mac_mode;                          /* 0: every section carries mac; 1: multicast datagrams carry their group's */
  int packing;                           /* 0 / 1 */
  int64_t max_pdu_bytes;                 /* largest pdu_len of a run, 1 .. 2^31 - 1 */
  int max_pdus;                          /* largest n_pdus of a run, 1 .. 2^24 */
} dvbt2ll_mpe_params;
typedef struct {
  int64_t pdu;                           /* a PDU index in [0, n_pdus] */
  int section_byte;                      /* bytes of that PDU's section already emitted */
  int cc;                                /* 0 .. 15: the next packet's continuity counter */
} dvbt2ll_mpe_pos;
typedef struct {
  dvbt2ll_mpe_pos resume;
  int64_t pdus_in, sections, skipped_len, skipped_type, mapped_macs, ts_packets, pusi_packets, pad_bytes, flushed;
} dvbt2ll_mpe_result;
/* DVBT2LL_EINVAL: a null pointer, pid / mac_mode / packing / the maxima out of range; DVBT2LL_EDEVICE without a GPU */
int dvbt2ll_mpe_create(const dvbt2ll_mpe_params *p, int device, dvbt2ll_mpe **out);
/* pdu_dev, off_dev on the device; start: {0, 0, cc} or a previous call's resume position in this list's PDU indices;
 * out_dev: room for out_cap_packets x 188 bytes.  Asynchronous on stream (NULL: the handle's own); no host round trip.
 * One run of a handle at a time: the next run call on another stream first waits for the previous one.
 * DVBT2LL_EINVAL, nothing launched: a null pointer, pdu_len or n_pdus negative or above the create-time maxima, a
 * negative capacity, start.pdu outside [0, n_pdus], section_byte negative or > 0 at n_pdus, cc outside 0 .. 15. */
int dvbt2ll_mpe_run_device(dvbt2ll_mpe *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                           int64_t n_pdus, const dvbt2ll_mpe_pos *start, void *out_dev, int64_t out_cap_packets,
                           int flush, void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_mpe_get_result(dvbt2ll_mpe *h, dvbt2ll_mpe_result *res);
/* host buffers, synchronous: the PDUs and the table are copied in, the written packets are copied out.  The device
 * output buffer holds out_cap_packets, or what n_pdus PDUs inside pdu_len bytes can become at the most if that is
 * less. */
int dvbt2ll_mpe_run_host(dvbt2ll_mpe *h, const void *pdu, int64_t pdu_len, const uint32_t *off, int64_t n_pdus,
                         const dvbt2ll_mpe_pos *start, void *out, int64_t out_cap_packets, int flush,
                         dvbt2ll_mpe_result *res);
void dvbt2ll_mpe_destroy(dvbt2ll_mpe *h);

/* ---------------------------------------------------------------------------
 * MPE-FEC encapsulator: the MPE encapsulator's input -> per MPE-FEC frame its MPE sections (with real-time
 * parameters), then Reed-Solomon columns in MPE-FEC sections, in 188-byte TS packets, so that a receiver can rebuild
 * datagrams lost to TS packet errors; a receiver that knows nothing of MPE-FEC still reads every datagram.  A handle of
 * its own beside the chain: it holds scratch, no stream state.  The rules are this project's reading of EN 301 192
 * clause 9, written without the standard at hand; the reference has no MPE-FEC code, so all of this is PARITY
 * UNPINNED, pinned by tests/mpefec_ref.py's sequential restatement and its independent receiver.
 * Not built: time slicing (delta_t as a time, burst scheduling with null packets, the time_slice_fec_identifier
 * descriptor with INT / PSI tables), datagrams split over frames or sections, LLC/SNAP, per-frame data_columns or
 * rs_columns, interleaved MPE and MPE-FEC sections, GNU Radio adapters and distributed variants.
 *
 * input      the MPE handle's (pdu_dev, off_dev, the skip rules and skipped_len / skipped_type), and a PDU is also
 *            skipped into skipped_len when p > min(4080, D x rows).  With rows, D = data_columns, K = rs_columns:
 *            C = D x rows.
 * frames     the frames partition the call's PDU index range from start.pdu.  A frame takes successive valid PDUs
 *            while the sum of their lengths stays <= C; it ends just behind its last datagram, and a later frame
 *            begins there: skipped PDUs in front of a frame's first datagram belong to that frame and contribute
 *            nothing.  A frame is closed when a further valid PDU of the call does not fit, or when flush = 1 and the
 *            list ends with at least one datagram in it.  An open frame emits nothing, not even its MPE sections, so
 *            where a call's list ends never changes the partition.
 * table      the application data table A has 191 x rows bytes: the frame's m datagrams back to back from address 0,
 *            U bytes in all, then zeros.  Address a is column a / rows, row a mod rows.
 * RS         GF(2^8) with x^8 + x^4 + x^3 + x^2 + 1 (0x11D), lambda = 02, g(x) = prod (x + lambda^i), i = 0 .. 63.
 *            Row r's data symbols are d_c = A[c x rows + r], c = 0 .. 190; par_0 .. par_63 are the coefficients of
 *            (sum d_c x^(254 - c)) mod g(x), par_k that of x^(63 - k); RS column k, row r, is par_k: the 255-symbol
 *            row vanishes at lambda^0 .. lambda^63.  Only RS columns 0 .. K - 1 are sent (K < 64: puncturing).
 *            d_190 = 01 alone gives g_63 .. g_0 = c1 0a ff 3a .. e4 f2 f5; d_0 = 01 alone gives 8f 2f 0f 0e .. 96 8b.
 * sections   a closed frame sends its m MPE sections, then K MPE-FEC sections.  RT (bytes 8 .. 11, big-endian) =
 *            delta_t << 20 | table_boundary << 19 | frame_boundary << 18 | address; delta_t is the frame's cyclic
 *            index, (start.frame + the frames closed before it in the call) & 0xFFF: time slicing is not used.
 *              MPE section j: the MPE handle's 12 + p + 4 bytes, but bytes 8 .. 11 hold RT with table_boundary =
 *              (j == m - 1), frame_boundary 0, address = the datagram's first byte in A.  Bytes 3, 4 carry MAC bytes
 *              6, 5 by mac_mode, and mapped_macs counts as before.
 *              MPE-FEC section k, rows + 16 bytes: 78; B0 | L >> 8, L & FF with L = rows + 13; padding_columns =
 *              191 - ceil(U / rows); FF; FF (reserved 1s, current_next_indicator 1); section_number k;
 *              last_section_number K - 1; RT with table_boundary = frame_boundary = (k == K - 1), address = k x rows;
 *              RS column k, row 0 first; CRC_32 as the MPE section's.
 * TS packets the MPE handle's rules for either packing value, over the whole section sequence; the sections of
 *            successive frames pack back to back.  "next": another section of a closed frame follows in this call.
 * capacity   a call emits the longest prefix of determined packets that fits out_cap_packets, of the first
 *            max_frames closed frames.  Where a closed frame follows them, no packet that begins behind the last byte
 *            of frame max_frames is emitted: the packet that frame ends in holds the next frame's first bytes (the
 *            handle computes that frame as well, to know them, so its scratch holds max_frames + 1 frames), and the
 *            flush does not apply.  resume = {pdu, section, section_byte, cc,
 *            frame}: the first PDU index of the frame that holds the first section byte not emitted, which of that
 *            frame's sections (0 .. m + K - 1) holds it, how many of that section's bytes were emitted, the next
 *            packet's counter, that frame's index; with every closed frame sent, {the open frame's first index, or
 *            n_pdus when no datagram is left; 0; 0; cc; the next frame's index}.  A start inside a frame recomputes
 *            that frame from its first PDU, parity included.  Where the frame the start names is not closed in this
 *            call, nothing is emitted and resume = start.  A start.section that is not below m + K is taken as
 *            section 0, byte 0; a section_byte that is not below that section's length as 0.  Chained calls at any
 *            list split, any capacity and any max_frames produce the single call's bytes.
 * counters   pdus_in, sections (MPE), fec_sections, frames, skipped_len, skipped_type, mapped_macs cover the frames
 *            wholly sent: the PDUs from start.pdu to before resume.pdu, so they add up over chained calls; ts_packets,
 *            pusi_packets, pad_bytes cover the packets emitted; flushed is 1 when flush was set and resume.pdu is
 *            n_pdus.
 * bounds     nothing outside out_cap_packets x 188 bytes of out_dev is written.
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_mpefec dvbt2ll_mpefec;
typedef struct {
  int pid;                               /* 0 .. 0x1FFE */
  uint8_t mac[6];                        /* the MAC address, first byte first */
  int mac_mode;                          /* 0: every section carries mac; 1: multicast datagrams carry their group's */
  int packing;                           /* 0 / 1 */
  int64_t max_pdu_bytes;                 /* largest pdu_len of a run, 1 .. 2^31 - 1 */
  int max_pdus;                          /* largest n_pdus of a run, 1 .. 2^24 */
  int rows;                              /* 256, 512, 768 or 1024 */
  int data_columns;                      /* D, 1 .. 191: the application data columns a frame may fill */
  int rs_columns;                        /* K, 1 .. 64: the RS columns sent */
  int max_frames;                        /* 1 .. 2^16: the most frames one call closes.  The scratch holds (max_frames + 1)
                                          * x (D + K) x rows bytes of tables and RS columns (16 MiB at 64, rows 1024, D 191,
                                          * K 64; about 17 GB at 2^16): create returns DVBT2LL_ENOMEM where that is too much */
} dvbt2ll_mpefec_params;
typedef struct {
  int64_t pdu;                           /* a frame's first PDU index, in [0, n_pdus] */
  int section;                           /* a section of that frame */
  int section_byte;                      /* bytes of that section already emitted */
  int cc;                                /* 0 .. 15: the next packet's continuity counter */
  int frame;                             /* 0 .. 4095: that frame's index */
} dvbt2ll_mpefec_pos;
typedef struct {
  dvbt2ll_mpefec_pos resume;
  int64_t pdus_in, sections, fec_sections, frames, skipped_len, skipped_type, mapped_macs, ts_packets, pusi_packets,
      pad_bytes, flushed;
} dvbt2ll_mpefec_result;
/* DVBT2LL_EINVAL: a null pointer or a parameter out of range; DVBT2LL_EDEVICE without a GPU */
int dvbt2ll_mpefec_create(const dvbt2ll_mpefec_params *p, int device, dvbt2ll_mpefec **out);
/* as dvbt2ll_mpe_run_device.  DVBT2LL_EINVAL, nothing launched: a null pointer, pdu_len or n_pdus negative or above the
 * create-time maxima, a negative capacity, start.pdu outside [0, n_pdus], section outside 0 .. D x rows + K - 1 (a
 * frame of one-byte datagrams has D x rows MPE sections; every resume position lies inside), section_byte outside
 * 0 .. 4095, section or section_byte > 0 at n_pdus, cc outside 0 .. 15, frame outside 0 .. 4095. */
int dvbt2ll_mpefec_run_device(dvbt2ll_mpefec *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                              int64_t n_pdus, const dvbt2ll_mpefec_pos *start, void *out_dev, int64_t out_cap_packets,
                              int flush, void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_mpefec_get_result(dvbt2ll_mpefec *h, dvbt2ll_mpefec_result *res);
/* host buffers, synchronous, as dvbt2ll_mpe_run_host */
int dvbt2ll_mpefec_run_host(dvbt2ll_mpefec *h, const void *pdu, int64_t pdu_len, const uint32_t *off, int64_t n_pdus,
                            const dvbt2ll_mpefec_pos *start, void *out, int64_t out_cap_packets, int flush,
                            dvbt2ll_mpefec_result *res);
void dvbt2ll_mpefec_destroy(dvbt2ll_mpefec *h);

/* ---------------------------------------------------------------------------
 * TS multiplexer: up to 8 device buffers of 188-byte TS packets -> one constant-bit-rate TS on the device, with null
 * packets where nothing is due and, if asked for, PCR packets: what turns the single-PID streams of the ULE / MPE /
 * MPE-FEC handles and a PSI carousel (dvbt2ll_psi_build below) into a stream a deployed receiver or TS analyser can
 * find its way in, and what the mode adapter then splits over the PLPs by PID.  A handle of its own beside the chain:
 * it holds the schedule tables and the last run's counters, no stream state.  Which input a slot belongs to is a fixed
 * periodic schedule, so every output packet is resolved on its own: no scan.  An input packet's bytes are never
 * altered unless the handle has a remux (the next block: per-PID remapping, continuity and PCR restamping).  Not
 * built: SDT / NIT / INT, section versions changing inside a carousel, GNU Radio adapters and distributed variants.
 * The reference has no multiplexer, so all of this is PARITY UNPINNED, pinned by tests/tsmux_ref.py's sequential
 * restatement and its TS checker.
 *
 * schedule   the owners are the inputs 0 .. n - 1, the PCR generator (owner n, weight pcr_weight) and "null" (owner
 *            n + 1, weight period - the sum of the others).  Owner e's k-th slot, k = 0 .. w_e - 1, is due at k / w_e
 *            of the period.  All period (due, e) pairs are sorted by due time ascending (compared exactly: k w_f
 *            against k' w_e), ties to the lower e; the m-th pair takes table slot m.  pre_e[t] is the number of
 *            owner e's slots among table slots [0, t).  dvbt2ll_tsmux_schedule returns the table without a GPU.
 * position   {phase, pcr_ticks, next[8]}: the table slot of the call's first output packet (0 .. period - 1); the
 *            27 MHz clock at the start of the period that holds that slot, modulo W = 2^33 x 300; next[i], the index
 *            of input i's next packet in the buffer passed (0 .. n_in[i]).
 * a run      writes exactly n_out packets, whatever the inputs hold.  For output index m: dc = (phase + m) / period,
 *            t = (phase + m) mod period, the owner e = table[t], and r_e(m) = dc w_e + pre_e[t] - pre_e[phase] is the
 *            number of e's slots in this call before m.  avail_i = n_in[i] - next[i].
 *              a non-loop input i (not the fill input): packet next[i] + r_i(m) when r_i(m) < avail_i, else the slot is
 *                free and counted in dry_slots[i]
 *              a loop input i: packet (next[i] + r_i(m)) mod n_in[i]; with n_in[i] = 0 the slot is free and counted in
 *                dry_slots[i]
 *              null: a free slot
 *              PCR: 47, pcr_pid >> 8, pcr_pid & FF, 20 (adaptation field only, continuity counter 0: it does not
 *                count on such packets); B7 (adaptation_field_length 183), 10 (PCR_flag); six bytes holding the
 *                33-bit base, six 1 bits and the 9-bit extension; 176 x FF.  The clock is T = (pcr_ticks + dc
 *                ticks_per_period + floor(t ticks_per_period / period)) mod W, base = T / 300, extension = T mod 300.
 *              a free slot without a fill input: the null packet 47 1F FF 10, 184 x FF
 *              with fill input f (loop[f] = 0): f's claims are its own slots and every free slot of the others, in
 *                slot order.  The claim of rank c(m) = r_f(m) + r_null(m) + the sum over the non-loop inputs i != f
 *                of max(0, r_i(m) - avail_i) + the sum over the empty loop inputs of r_i(m) carries packet next[f] +
 *                c(m) when c(m) < avail_f; any other claim is a null packet (f's own slot is then counted in
 *                dry_slots[f])
 *            An input packet whose first byte is not 47 is consumed, counted in sync_errors and sent as a null
 *            packet.
 * result     resume: phase advanced by n_out mod period; pcr_ticks advanced by ((phase + n_out) / period)
 *            ticks_per_period, mod W; next[i] advanced by consumed[i] (mod n_in[i] for a loop input).  consumed[i]:
 *            the packets taken from input i, bad-sync ones included; dry_slots[i] as above; fill_in_free: the fill
 *            input's packets carried in slots it does not own; pcr_packets; null_packets: every null packet written,
 *            those replacing a bad-sync packet included; sync_errors.  Chained calls at any split of n_out, given the
 *            same buffers and each call's resume position, produce the single call's bytes and summed counters.
 * bounds     nothing outside n_out x 188 bytes of out_dev is written, nothing outside an input's n_in[i] x 188 bytes
 *            is read.  Inputs and output may have any byte alignment.
 * ------------------------------------------------------------------------- */
#define DVBT2LL_TSMUX_INPUTS 8
#define DVBT2LL_TSMUX_MAX_PERIOD 65536
typedef struct dvbt2ll_tsmux dvbt2ll_tsmux;
typedef struct {
  int n_inputs;                          /* 1 .. 8 */
  int period;                            /* slots of the schedule's period, 1 .. 65536 */
  int weight[DVBT2LL_TSMUX_INPUTS];      /* slots per period of input i; 0 only for the fill input */
  int loop[DVBT2LL_TSMUX_INPUTS];        /* 0 / 1: the input's buffer is a carousel, read round and round */
  int fill_input;                        /* -1, or the index of an input with loop 0 that also takes the free slots */
  int pcr_pid;                           /* -1: no PCR packets; else 0 .. 0x1FFE */
  int pcr_weight;                        /* PCR packets per period: >= 1 with a PCR PID, else 0 */
  int64_t ticks_per_period;              /* 27 MHz ticks that period slots last, 1 .. 2^36 - 1 (0 without a PCR PID) */
  int max_out_packets;                   /* largest n_out of a run, 1 .. 2^24 */
} dvbt2ll_tsmux_params;
typedef struct {
  int phase;                             /* 0 .. period - 1 */
  int64_t pcr_ticks;                     /* 0 .. 2^33 x 300 - 1 */
  int64_t next[DVBT2LL_TSMUX_INPUTS];    /* 0 .. n_in[i] */
} dvbt2ll_tsmux_pos;
typedef struct {
  dvbt2ll_tsmux_pos resume;
  int64_t consumed[DVBT2LL_TSMUX_INPUTS], dry_slots[DVBT2LL_TSMUX_INPUTS];
  int64_t fill_in_free, pcr_packets, null_packets, sync_errors;
} dvbt2ll_tsmux_result;
/* host only: the schedule table of p, period owner indices (input i, n_inputs: PCR, n_inputs + 1: null).
 * DVBT2LL_EINVAL: a null pointer, a value out of range, the weights and pcr_weight above period, a weight of 0 on an
 * input that is not the fill input, a fill input that loops, pcr_weight / ticks_per_period that do not go with pcr_pid */
int dvbt2ll_tsmux_schedule(const dvbt2ll_tsmux_params *p, uint8_t *owner);
/* host only: round(period x 1504 x 27e6 / ts_bits_per_second), the ticks_per_period of a TS of that rate; -1 when
 * period is outside 1 .. 65536 or the rate is not positive */
int64_t dvbt2ll_tsmux_ticks_per_period(int period, int64_t ts_bits_per_second);
/* DVBT2LL_EINVAL as dvbt2ll_tsmux_schedule; DVBT2LL_EDEVICE without a GPU */
int dvbt2ll_tsmux_create(const dvbt2ll_tsmux_params *p, int device, dvbt2ll_tsmux **out);
/* in_dev[i]: input i's n_in[i] packets on the device (entries from n_inputs on are ignored); out_dev: room for n_out x
 * 188 bytes.  Asynchronous on stream (NULL: the handle's own); no host round trip.  One run of a handle at a time: the
 * next run call on another stream first waits for the previous one.  DVBT2LL_EINVAL, nothing launched: a null handle,
 * start or out_dev, a null in_dev[i] where n_in[i] > 0, n_in[i] negative or above 2^31 - 1, n_out negative or above
 * max_out_packets, next[i] outside [0, n_in[i]], phase outside [0, period), pcr_ticks outside [0, 2^33 x 300) */
int dvbt2ll_tsmux_run_device(dvbt2ll_tsmux *h, const void *const *in_dev, const int64_t *n_in,
                             const dvbt2ll_tsmux_pos *start, void *out_dev, int64_t n_out, void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_tsmux_get_result(dvbt2ll_tsmux *h, dvbt2ll_tsmux_result *res);
/* host buffers, synchronous: the inputs are copied in, the n_out packets are copied out */
int dvbt2ll_tsmux_run_host(dvbt2ll_tsmux *h, const void *const *in, const int64_t *n_in,
                           const dvbt2ll_tsmux_pos *start, void *out, int64_t n_out, dvbt2ll_tsmux_result *res);
void dvbt2ll_tsmux_destroy(dvbt2ll_tsmux *h);

/* ---------------------------------------------------------------------------
 * TS multiplexer, remux: per-PID remapping, continuity restamping and PCR restamping, what lets the multiplexer take
 * inputs it did not make: a recorded programme with its own PCR, a clip or carousel whose packet count per PID is no
 * multiple of 16, an input that runs dry and goes on later, two inputs on one PID.  A configuration set once on a
 * handle (dvbt2ll_tsmux_set_remux); the handle is then run with the *_remux calls, which take and return a second
 * position beside dvbt2ll_tsmux_pos, and the plain run calls refuse it (DVBT2LL_EINVAL), so that nobody loses the
 * continuity state by accident.  A handle on which set_remux was never called launches the plain kernel and writes
 * the plain bytes.  Schedule, position, run, result and bounds of the block above hold unchanged; this block adds
 * what happens to an input packet after it is resolved.  PARITY UNPINNED as the multiplexer is: pinned by
 * tests/tsremux_ref.py's sequential restatement and its independent checker.
 *
 * order      per output packet: resolved as above.  A bad-sync packet becomes a null packet and nothing below applies
 *            to it.  Then the remap, then the continuity restamp, then the PCR restamp.  Generated PCR packets and
 *            null packets are not touched.
 * remap      n_map entries {input, from_pid, to_pid}: a packet of that input with PID from_pid leaves with to_pid
 *            (the other 3 bits of its byte 1 stay) and is counted in remapped.  to_pid 0x1FFF drops it: the packet is
 *            consumed, counted in dropped (not in remapped) and in null_packets, and sent as the null packet 47 1F FF
 *            10, 184 x FF, as a bad-sync packet is; nothing below applies to it.  Packets without an entry keep their
 *            PID.  A pair (input, from_pid) may appear once.  No to_pid may be the handle's pcr_pid: that PID carries
 *            nothing else.
 * continuity n_track distinct output PIDs track_pid[s], none of them 0x1FFF or the handle's pcr_pid; s is the PID's
 *            slot.  A packet is restamped on slot s when its input has restamp_cc set and its PID after the remap is
 *            track_pid[s].  k(m) is the number of output packets before m in this call that were restamped on s and
 *            carry a payload (adaptation_field_control & 1).  A restamped packet with a payload takes the counter
 *            (cc[s] + k(m)) & 15, one without takes (cc[s] + k(m) - 1) & 15, the last payload packet's (13818-1
 *            2.4.3.3).  Packets of an input with restamp_cc 0 are left alone and not counted, whatever their PID.
 *            cc_rewritten counts the packets whose counter left different from how it came.
 * PCR        for a packet of an input i with in_ticks_per_period[i] > 0 whose adaptation field is present
 *            (adaptation_field_control & 2), at least 7 bytes long (byte 4 >= 7) and has PCR_flag (byte 5 & 0x10):
 *            input i's in_period[i] packets last in_ticks_per_period[i] ticks, the formulation of period and
 *            ticks_per_period.  j is the packet's rank among its input's packets in this call: r_i(m), or the claim
 *            rank c(m) for the fill input; it is not reduced mod n_in[i] for a loop input.  in_phase[i] + j = dq
 *            in_period[i] + r with 0 <= r < in_period[i]; T_in = in_ticks[i] + dq in_ticks_per_period[i] + floor(r
 *            in_ticks_per_period[i] / in_period[i]); T_out is the slot's clock T of the block above, from the handle's
 *            ticks_per_period or, on a handle without a PCR PID, from out_ticks_per_period; PCR_in = 300 base +
 *            extension as found in bytes 6 .. 11; PCR_out = (PCR_in + T_out - T_in) mod W, written back as base, six 1
 *            bits and extension, and the packet is counted in pcr_restamped.  OPCR, PTS and DTS are untouched.
 *            Precondition: the correction keeps a programme clock right only if the caller gives the input slots at
 *            its own long-term rate; pacing an input by its own clock is not built.  All arithmetic is 64-bit, as the
 *            generator's: a run with (n_in[i] / in_period[i] + 1) x in_ticks_per_period[i] above 2^62 is refused.
 * position   {cc[64], in_phase[8], in_ticks[8]}: cc[s], 0 .. 15, the counter the next payload packet restamped on
 *            slot s takes (0 from n_track on); in_phase[i], 0 .. in_period[i] - 1, of input i's next packet; in_ticks[i],
 *            0 .. W - 1, input i's clock at the start of the input period holding that packet.  Both are 0 for an input
 *            whose in_ticks_per_period is 0.
 * result     resume: cc[s] advanced by k(n_out), mod 16; in_phase[i] advanced by consumed[i] mod in_period[i];
 *            in_ticks[i] advanced by ((in_phase[i] + consumed[i]) / in_period[i]) in_ticks_per_period[i], mod W.  The
 *            multiplexer's own resume position is dvbt2ll_tsmux_result's; on a handle without a PCR PID its pcr_ticks
 *            advances by out_ticks_per_period per period.  Chained calls at any split of n_out, each started from the
 *            previous call's two resume positions, give the single call's bytes and summed counters.
 * Not built: recognising duplicate packets (13818-1 allows one repeat of a packet; a repeat counts as a new packet
 * here), setting discontinuity_indicator (it is left as it came), pacing an input by its own clock, more than 64 map
 * entries or tracked PIDs, a PID shared with the PCR generator, SDT / NIT / INT, GNU Radio adapters and distributed
 * variants.
 * ------------------------------------------------------------------------- */
#define DVBT2LL_TSMUX_MAP 64
#define DVBT2LL_TSMUX_TRACK 64
typedef struct {
  int input;                             /* 0 .. n_inputs - 1 */
  int from_pid, to_pid;                  /* 0 .. 0x1FFF; to_pid 0x1FFF: dropped */
} dvbt2ll_tsmux_map;
typedef struct {
  int n_map;                             /* 0 .. 64 */
  dvbt2ll_tsmux_map map[DVBT2LL_TSMUX_MAP];
  int n_track;                           /* 0 .. 64 */
  int track_pid[DVBT2LL_TSMUX_TRACK];    /* distinct, 0 .. 0x1FFE, not the handle's pcr_pid */
  int restamp_cc[DVBT2LL_TSMUX_INPUTS];  /* 0 / 1 */
  int in_period[DVBT2LL_TSMUX_INPUTS];   /* 1 .. 65536; 0 with in_ticks_per_period 0 */
  int64_t in_ticks_per_period[DVBT2LL_TSMUX_INPUTS];   /* 1 .. 2^36 - 1; 0 (with in_period 0): the PCRs pass unchanged */
  int64_t out_ticks_per_period;          /* the mux clock of a handle without a PCR PID, 0 .. 2^36 - 1; with one: 0 or
                                            the handle's ticks_per_period */
} dvbt2ll_tsmux_remux;
typedef struct {
  int cc[DVBT2LL_TSMUX_TRACK];           /* 0 .. 15 */
  int in_phase[DVBT2LL_TSMUX_INPUTS];    /* 0 .. in_period[i] - 1 */
  int64_t in_ticks[DVBT2LL_TSMUX_INPUTS];/* 0 .. 2^33 x 300 - 1 */
} dvbt2ll_tsmux_remux_pos;
typedef struct {
  dvbt2ll_tsmux_remux_pos resume;
  int64_t remapped, dropped, cc_rewritten, pcr_restamped;
} dvbt2ll_tsmux_remux_result;
/* host only, no GPU: 0, or DVBT2LL_EINVAL for a null pointer, params dvbt2ll_tsmux_schedule refuses, n_map or n_track
 * outside 0 .. 64, an entry's input outside 0 .. n_inputs - 1 or a PID outside its range, a pair (input, from_pid)
 * that appears twice, a tracked PID that repeats, a to_pid or tracked PID equal to pcr_pid, restamp_cc other than 0 / 1,
 * in_period / in_ticks_per_period out of range or only one of them 0, out_ticks_per_period out of range or, on a handle
 * with a PCR PID, neither 0 nor its ticks_per_period.  Entries of inputs from n_inputs on must be 0. */
int dvbt2ll_tsmux_remux_check(const dvbt2ll_tsmux_params *p, const dvbt2ll_tsmux_remux *x);
/* once per handle, before its first run: DVBT2LL_EINVAL as dvbt2ll_tsmux_remux_check, after a run, or a second time */
int dvbt2ll_tsmux_set_remux(dvbt2ll_tsmux *h, const dvbt2ll_tsmux_remux *x);
/* as dvbt2ll_tsmux_run_device, with the remux position.  DVBT2LL_EINVAL, nothing launched: as there, a handle without
 * a remux, a null rstart, cc[s] outside 0 .. 15 (or not 0 from n_track on), in_phase[i] outside 0 .. in_period[i] - 1
 * or in_ticks[i] outside [0, 2^33 x 300) (or not 0 where in_ticks_per_period[i] is 0), (n_in[i] / in_period[i] + 1) x
 * in_ticks_per_period[i] above 2^62 */
int dvbt2ll_tsmux_run_device_remux(dvbt2ll_tsmux *h, const void *const *in_dev, const int64_t *n_in,
                                   const dvbt2ll_tsmux_pos *start, const dvbt2ll_tsmux_remux_pos *rstart,
                                   void *out_dev, int64_t n_out, void *stream);
/* synchronises with the last run and returns its remux result (dvbt2ll_tsmux_get_result returns the other) */
int dvbt2ll_tsmux_get_remux_result(dvbt2ll_tsmux *h, dvbt2ll_tsmux_remux_result *res);
/* host buffers, synchronous, as dvbt2ll_tsmux_run_host */
int dvbt2ll_tsmux_run_host_remux(dvbt2ll_tsmux *h, const void *const *in, const int64_t *n_in,
                                 const dvbt2ll_tsmux_pos *start, const dvbt2ll_tsmux_remux_pos *rstart, void *out,
                                 int64_t n_out, dvbt2ll_tsmux_result *res, dvbt2ll_tsmux_remux_result *rres);

/* ---------------------------------------------------------------------------
 * PSI builder (host only): a PAT and one PMT per programme (ISO/IEC 13818-1 2.4.4) as a carousel of TS packets for a
 * loop input of the multiplexer.  The stream types and descriptors are the caller's, carried as they are.
 *
 * rounds     the buffer holds 16 rounds.  A round is the PAT (PID 0) in one packet, then each programme's PMT on its
 *            pmt_pid in as many packets as it needs.  A section's first packet has PUSI 1 and pointer_field 00, later
 *            ones carry 184 section bytes; the bytes behind the section's end are FF.  Every PID's continuity counter
 *            runs on across the rounds, and after 16 rounds every PID has sent a multiple of 16 packets: the buffer
 *            read round and round is a seamless stream, which is why the multiplexer needs no continuity logic.
 * PAT        00, B0 | len >> 8, len & FF; transport_stream_id (2 bytes); C1 | version << 1; 00 00; per programme:
 *            program_number (2 bytes), E0 | pmt_pid >> 8, pmt_pid & FF; CRC_32 (the MPE section's).  len counts the
 *            bytes behind the length field, CRC_32 included.
 * PMT        02, B0 | len >> 8, len & FF; program_number (2 bytes); C1 | version << 1; 00 00; E0 | pcr_pid >> 8,
 *            pcr_pid & FF; F0 00 (no programme descriptors); per stream: stream_type, E0 | pid >> 8, pid & FF,
 *            F0 | n >> 8, n & FF, the n descriptor bytes; CRC_32.
 * ------------------------------------------------------------------------- */
#define DVBT2LL_PSI_PROGRAMS 8
#define DVBT2LL_PSI_STREAMS 8
#define DVBT2LL_PSI_DESCRIPTOR_BYTES 64
#define DVBT2LL_PSI_ROUNDS 16
typedef struct {
  int stream_type;                       /* 0 .. 255 */
  int pid;                               /* 0 .. 0x1FFF */
  int descriptor_len;                    /* 0 .. 64 */
  uint8_t descriptors[DVBT2LL_PSI_DESCRIPTOR_BYTES];
} dvbt2ll_psi_stream;
typedef struct {
  int program_number;                    /* 1 .. 65535 */
  int pmt_pid;                           /* 0x10 .. 0x1FFE, distinct across the programmes */
  int pcr_pid;                           /* 0 .. 0x1FFF; 0x1FFF: the programme has no PCR */
  int n_streams;                         /* 0 .. 8 */
  dvbt2ll_psi_stream streams[DVBT2LL_PSI_STREAMS];
} dvbt2ll_psi_program;
typedef struct {
  int transport_stream_id;               /* 0 .. 65535 */
  int version;                           /* 0 .. 31 */
  int n_programs;                        /* 1 .. 8 */
  dvbt2ll_psi_program programs[DVBT2LL_PSI_PROGRAMS];
} dvbt2ll_psi_params;
/* writes the carousel's packets to out (room for cap_packets x 188 bytes) and returns their number; with out NULL it
 * returns the number only.  DVBT2LL_EINVAL: a null p, a value out of range, PMT PIDs that repeat, too small a capacity */
int64_t dvbt2ll_psi_build(const dvbt2ll_psi_params *p, uint8_t *out, int64_t cap_packets);

/* ---------------------------------------------------------------------------
 * GSE encapsulator (Generic Stream Encapsulation, ETSI TS 102 606-1; EN 302 755 5.1.7): a device buffer of PDUs (IP
 * datagrams) and a device offset table -> one PLP's normal-mode BBFRAMEs with TS/GS = 10, in the layout
 * DVBT2LL_INPUT_BBFRAME reads (kbch / 8 bytes per BBFRAME, back to back): IP reaches IQ with no TS layer.  A handle
 * of its own beside the chain: it holds scratch, no stream state.  Not built: extension headers, label reuse (LT 11
 * on complete packets) and per-PDU labels, PDUs above 4090 - L bytes, several PDUs open at once (QoS interleaving),
 * HEM / ISSY headers, GSE-Lite signalling.  The reference has no GSE code, so all of this is PARITY UNPINNED, pinned
 * by tests/gse_ref.py's sequential restatement and its receiver.  The rules are this project's
 * reading of the two standards.  D = (kbch - 80) / 8 is the data field in bytes, L = label_len (6, 3 or 0), LT = 00 /
 * 01 / 10 for these.
 *
 * input      as the ULE handle's: pdu_dev holds pdu_len bytes (below 2^31); off_dev holds n_pdus + 1 uint32_t
 *            offsets: PDU i is bytes [off[i], off[i + 1]), len of them.  type_dev is optional: n_pdus uint16_t
 *            Protocol Types.  With type_dev == NULL the type comes from the PDU's first nibble: 4 -> 0x0800, 6 ->
 *            0x86DD; any other nibble: the PDU is skipped and counted in skipped_type.  A PDU is skipped and counted
 *            in skipped_len when off[i + 1] <= off[i], or off[i + 1] > pdu_len, or len > 4090 - L (the length is
 *            judged first).  The bound keeps every packet's 12-bit GSE Length <= 4095, so no PDU needs two packets in
 *            one frame.  A skipped PDU contributes nothing (it still takes its place in the Frag ID count); every
 *            rule below speaks of the valid PDUs.  Nothing outside [pdu_dev, pdu_dev + pdu_len) and the two tables is
 *            read.  Valid PDUs may overlap or repeat; the frames may then be more than the buffer's bytes suggest.
 * packets    every GSE packet starts with S, E, LT (2 bits) and GSE Length (12 bits) = the bytes that follow:
 *              complete        S 1, E 1, the handle's LT: Protocol Type (2), Label (L), the PDU: 4 + L + len bytes
 *              first fragment  S 1, E 0, the handle's LT: Frag ID (1), Total Length (2) = 2 + L + len, Protocol Type,
 *                              Label, a piece of the PDU: 7 + L + piece bytes
 *              continuation    S 0, E 0, LT 11: Frag ID, piece: 3 + piece bytes
 *              end fragment    S 0, E 1, LT 11: Frag ID, piece, CRC-32: 7 + piece bytes
 *            The CRC-32 (generator 0x04C11DB7, initial value 0xFFFFFFFF, MSB first, no final XOR, big-endian: the CRC
 *            ULE uses) covers Total Length, Protocol Type, Label and the whole PDU.  The Frag ID of PDU i is
 *            (start.frag_id + i - start.pdu) mod 256.  Only one PDU is ever open.
 * placement  sequential over the PDUs; u is the bytes used in the open data field (0 at a frame's start); a packet
 *            never crosses a BBFRAME; a frame with u = D is closed.  A fresh PDU with free = D - u:
 *              free >= 4 + L + len: a complete packet;
 *              else free >= 8 + L: a first fragment with piece = free - 7 - L, which fills the frame;
 *              else the frame is closed as it is and the PDU is fresh at u = 0 of the next one.
 *            An open PDU with rem bytes left (always at u = 0):
 *              rem + 7 <= D: an end fragment with piece = rem;
 *              else a continuation with piece = min(D - 3, rem - 1), so that the end fragment always carries a PDU
 *              byte, and the frame is closed: at most 4 of its bytes stay unused.
 * BBFRAMEs   normal-mode header: MATYPE-1 = TS/GS 10, SIS/MIS, CCM 1, ISSYI 0, NPD 0, EXT 00 (B0 for SIS); MATYPE-2 =
 *            the ISI (MIS) or 0; UPL 0; DFL = 8 x the bytes of the frame's packets; SYNC 0; SYNCD 0 (a packet always
 *            starts at byte 0); CRC-8 with MODE = 0: dvbt2ll_chain_bbheader_errors counts none.  The unused rest of
 *            the data field is zero and counted in pad_bytes.
 * capacity   a call emits the closed frames that out_cap_blocks allows and returns resume = {pdu, pdu_byte, frag_id},
 *            the state at the start of the first frame not emitted: the first valid PDU that continues or starts
 *            there, the number of its bytes already sent (0: it is fresh), its Frag ID.  A frame still open when the
 *            input ends is emitted only with flush = 1, and only if it fits the capacity (DFL = 8 u; none when u =
 *            0); then resume = {n_pdus, 0, the Frag ID n_pdus would have}.  Without flush the open frame's PDUs are
 *            presented again by the next call, which passes resume as start with a PDU list that begins at or before
 *            that PDU.  A start whose pdu_byte is not in 1 .. len - 1 of a valid PDU is taken as 0.  Chained calls at
 *            any split, and after any capacity cut, produce the single call's bytes.
 * counters   pdus_in, complete, fragmented (PDUs), skipped_len, skipped_type cover the PDUs from start.pdu to before
 *            resume.pdu, so they add up over chained calls (a PDU an earlier call left open counts as fragmented
 *            where it ends); gse_packets, bbframes and pad_bytes cover the frames emitted; flushed is 1 when the
 *            flush frame was written.
 * bounds     nothing outside out_cap_blocks x kbch / 8 bytes of out_dev is written.
 * scratch    about 22 bytes per PDU of max_pdus, and a position table of 4 D bytes per 256 PDUs.
 * ------------------------------------------------------------------------- */
typedef struct dvbt2ll_gse dvbt2ll_gse;
typedef struct {
  int kbch;                              /* one of the chain's 14 Kbch, or 3072; 0: taken from framesize / rate.
                                            58192 (D = 7264, the DVB family's largest; no T2 code has it and the
                                            chain takes no such frame) is accepted too: the tests pin the tables there */
  int framesize, rate;                   /* FECFRAME_* / C*: used when kbch == 0 */
  int sis_mis;                           /* 1: single input stream; 0: multiple, MATYPE-2 = isi (0 .. 255) */
  int isi;
  int label_len;                         /* 6, 3 or 0 (broadcast) */
  uint8_t label[6];                      /* the first label_len bytes are sent */
  int64_t max_pdu_bytes;                 /* largest pdu_len of a run, 1 .. 2^31 - 1 */
  int max_pdus;                          /* largest n_pdus of a run, 1 .. 2^24 */
} dvbt2ll_gse_params;
typedef struct {
  int64_t pdu;                           /* a PDU index in [0, n_pdus] */
  int pdu_byte;                          /* bytes of that PDU already sent */
  int frag_id;                           /* 0 .. 255: that PDU's Frag ID */
} dvbt2ll_gse_pos;
typedef struct {
  dvbt2ll_gse_pos resume;
  int64_t pdus_in, complete, fragmented, gse_packets, skipped_len, skipped_type, bbframes, pad_bytes, flushed;
} dvbt2ll_gse_result;
/* DVBT2LL_EINVAL: a null pointer, a Kbch that is neither one of the chain's 14 nor 3072 (nor 58192), sis_mis / isi / the maxima
 * out of range, a label_len other than 0, 3 or 6; DVBT2LL_EDEVICE without a GPU */
int dvbt2ll_gse_create(const dvbt2ll_gse_params *p, int device, dvbt2ll_gse **out);
/* fills kbch, sis_mis and isi from the chain's PLP plp; the other fields stay */
int dvbt2ll_gse_params_from_chain(const dvbt2ll_chain *chain, int plp, dvbt2ll_gse_params *p);
/* pdu_dev, off_dev, type_dev (or NULL) on the device; start: {0, 0, frag_id} or a previous call's resume position in
 * this list's PDU indices; out_dev: room for out_cap_blocks BBFRAMEs of kbch / 8 bytes.  Asynchronous on stream (NULL:
 * the handle's own); no host round trip.  One run of a handle at a time: the next run call on another stream first
 * waits for the previous one.  DVBT2LL_EINVAL, nothing launched: a null pointer (type_dev may be), pdu_len or n_pdus
 * negative or above the create-time maxima, a negative capacity, start.pdu outside [0, n_pdus], a negative pdu_byte,
 * frag_id outside 0 .. 255. */
int dvbt2ll_gse_run_device(dvbt2ll_gse *h, const void *pdu_dev, int64_t pdu_len, const uint32_t *off_dev,
                           const uint16_t *type_dev, int64_t n_pdus, const dvbt2ll_gse_pos *start, void *out_dev,
                           int64_t out_cap_blocks, int flush, void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_gse_get_result(dvbt2ll_gse *h, dvbt2ll_gse_result *res);
/* host buffers, synchronous: the PDUs and tables are copied in, the written BBFRAMEs are copied out.  The device
 * output buffer holds out_cap_blocks, or what n_pdus PDUs inside pdu_len bytes can become at the most if that is
 * less. */
int dvbt2ll_gse_run_host(dvbt2ll_gse *h, const void *pdu, int64_t pdu_len, const uint32_t *off, const uint16_t *type,
                         int64_t n_pdus, const dvbt2ll_gse_pos *start, void *out, int64_t out_cap_blocks, int flush,
                         dvbt2ll_gse_result *res);
void dvbt2ll_gse_destroy(dvbt2ll_gse *h);

/* ---------------------------------------------------------------------------
 * T2-MI output (ETSI TS 102 773 over DVB data piping): per-PLP packed BBFRAMEs on the device -> the 188-byte TS
 * packets a T2 gateway distributes to its modulators: the inverse of dvbt2ll_t2mi_* above.  A handle of its own beside
 * the chain: it holds tables and scratch sized at create, no stream state.  The BBFRAMEs are in the layout
 * DVBT2LL_INPUT_BBFRAME reads and the mode adapter, the GSE encapsulator and the T2-MI deframer write, so one GPU can
 * adapt or encapsulate, ship the result as T2-MI and encode the same buffers to IQ.  The reference has no T2-MI code:
 * PARITY UNPINNED, pinned by tests/t2mi_out_ref.py (a sequential framer composed from tests/t2mi_ref.py's t2mi_packet
 * and ts_mux), by t2mi_ref.parse as an independent receiver and by the deframer on the device.
 * Not built: PLPs whose interleaving frame spans several T2 frames or that skip frames (P_I x I_JUMP > 1;
 * params_from_chain refuses such a chain); a PLP_NUM_BLOCKS that varies from frame to frame; authoring L1-current or
 * timestamp payloads from the chain's configuration (they are carried as opaque slots); raw T2-MI without a TS layer;
 * a PCR or other adaptation-field content; carrying a partial TS packet across calls; FEF, auxiliary-stream I/Q and
 * addressing packets beyond what an opaque slot carries.
 *
 * input      per PLP k a device pointer to packed BBFRAMEs of bbframe_bytes[k] = kbch / 8 bytes, back to back,
 *            blocks_per_frame[k] = F_k of them per T2 frame: frame f of the call (0 .. nframes - 1) reads blocks
 *            [f F_k, (f + 1) F_k).  Up to 4 auxiliary packet slots per T2 frame, fixed at create: {packet_type,
 *            payload_bits, after}.  The payload of slot a in frame f of the call is ceil(payload_bits / 8) bytes at
 *            aux_dev + f aux_stride + aux_off[a]; it is copied as given, except that the pad bits of the last byte
 *            (its 8 ceil(payload_bits / 8) - payload_bits low bits) are forced to zero.  This is how a caller carries
 *            timestamp (0x20) and L1-current (0x10) packets: the handle neither interprets nor authors them.
 * a call     frames nframes whole T2 frames, numbered start.frame, start.frame + 1, ...
 * frame      the packets of one T2 frame in order: the slots with after = 0 in slot order; PLP 0's F_0 BBFRAME
 *            packets, then PLP 1's, and so on; the slots with after = 1 in slot order.
 * packets    as dvbt2ll_t2mi_* reads them: 6 header bytes (packet_type 8, packet_count 8, superframe_idx 4, rfu 9 = 0,
 *            t2mi_stream_id 3, payload_len 16 in bits), ceil(payload_len / 8) payload bytes, CRC-32/MPEG-2 (generator
 *            0x04C11DB7, initial value 0xFFFFFFFF, MSB first, no final XOR) of all bytes before it, big-endian.
 *            packet_count = (start.packet_count + the packet's index in the call) mod 256; superframe_idx =
 *            (frame / frames_per_superframe) & 15; t2mi_stream_id from the parameters.  Type 0x00 (a BBFRAME):
 *            payload_len = 24 + kbch; payload = frame_idx = frame % frames_per_superframe, plp_id[k],
 *            intl_frame_start in bit 7 of the third byte (rfu 7 = 0), the BBFRAME.  intl_frame_start = 1 on the first
 *            BBFRAME of each PLP in each T2 frame.
 * TS layer   the call's packets, concatenated, are its T2-MI byte stream; the output is byte for byte
 *            tests/t2mi_ref.py ts_mux(packets, pid, cc0 = start.cc).  Every TS packet: sync 47, TEI 0, PUSI, priority
 *            0, pid, scrambling 00, AFC, continuity counter = (start.cc + its index in the call) mod 16.  A TS packet
 *            that begins at stream position pos, with s the first packet start at or after pos:
 *              s - pos in 0 .. 182: PUSI 1, pointer_field = s - pos, then 183 stream bytes;
 *              s - pos = 183:       PUSI 0, 183 stream bytes (shortened, so that the next TS packet begins on s);
 *              otherwise:           PUSI 0, 184 stream bytes.
 *            The call's last TS packet carries what is left.  A body (pointer_field and stream bytes) shorter than 184
 *            bytes is preceded by an adaptation field of stuff = 184 - body bytes: AFC 11, the length byte a = stuff -
 *            1, and when a > 0 a flags byte 00 and a - 1 bytes FF; a full body has AFC 01.  Every call starts on a TS
 *            packet boundary with pointer_field 0 and ends with a stuffed packet (or, when the stream ends on a
 *            packet's last byte, a full one): a partial TS packet is not carried from call to call, which costs fewer
 *            than 184 bytes per call and keeps the handle without state.
 * result     next = {start.frame + nframes, the next packet_count, the next continuity counter}: passed as the next
 *            call's start, the concatenated outputs are one stream a receiver reads without a discontinuity.
 *            Counters: frames; t2mi_packets and by_type[packet_type]; ts_packets; pusi_packets; stuffing_bytes (the
 *            adaptation-field bytes, length bytes included).
 * capacity   every packet length is a constant of the handle, so the TS packets a call of nframes frames writes are
 *            known before it is launched: dvbt2ll_t2mi_out_ts_packets.  A call whose out_cap_packets is smaller is
 *            refused with DVBT2LL_EINVAL and launches nothing.
 * bounds     nothing but the BBFRAMEs and auxiliary payloads stated above is read; nothing outside the first
 *            dvbt2ll_t2mi_out_ts_packets(h, nframes) x 188 bytes of out_dev is written.  Source and destination
 *            pointers of any alignment are accepted.
 * scratch    9 bytes per T2-MI packet of max_frames frames.
 * ------------------------------------------------------------------------- */
#define DVBT2LL_T2MI_OUT_MAX_AUX 4
typedef struct dvbt2ll_t2mi_out dvbt2ll_t2mi_out;
typedef struct {
  int packet_type;                       /* 0 .. 255 */
  int payload_bits;                      /* 1 .. 65535 */
  int after;                             /* 0: before the frame's BBFRAME packets; 1: after them */
} dvbt2ll_t2mi_out_slot;
typedef struct {
  int pid;                               /* 0 .. 0x1FFE */
  int t2mi_stream_id;                    /* 0 .. 7 */
  int nplp;                              /* 1 .. DVBT2LL_MAX_PLP */
  int plp_id[DVBT2LL_MAX_PLP];           /* 0 .. 255, distinct */
  int bbframe_bytes[DVBT2LL_MAX_PLP];    /* kbch / 8 of one of the standard's 14 codes */
  int blocks_per_frame[DVBT2LL_MAX_PLP]; /* F_k: 1 .. 1023 BBFRAMEs per T2 frame */
  int frames_per_superframe;             /* 1 .. 256 (frame_idx has 8 bits) */
  int naux;                              /* 0 .. DVBT2LL_T2MI_OUT_MAX_AUX */
  dvbt2ll_t2mi_out_slot aux[DVBT2LL_T2MI_OUT_MAX_AUX];
  int max_frames;                        /* the most T2 frames of a call, >= 1; max_frames frames must stay below
                                            2^31 - 2^24 stream bytes */
} dvbt2ll_t2mi_out_params;
typedef struct {
  int64_t frame;                         /* >= 0: the T2 frame number of the call's first frame */
  int packet_count;                      /* 0 .. 255: the first packet's packet_count */
  int cc;                                /* 0 .. 15: the first TS packet's continuity counter */
} dvbt2ll_t2mi_out_pos;
typedef struct {
  dvbt2ll_t2mi_out_pos next;
  int64_t frames, t2mi_packets, ts_packets, pusi_packets, stuffing_bytes;
  int64_t by_type[256];                  /* T2-MI packets per packet_type */
} dvbt2ll_t2mi_out_result;
/* DVBT2LL_EINVAL: a null pointer, a field outside the range stated above, more than 4 slots; DVBT2LL_EDEVICE without
 * a GPU */
int dvbt2ll_t2mi_out_create(const dvbt2ll_t2mi_out_params *p, int device, dvbt2ll_t2mi_out **out);
/* fills nplp, plp_id[k] = plp_ids[k] (NULL: k), bbframe_bytes[k], blocks_per_frame[k] and frames_per_superframe
 * (the chain's t2frames) from a chain; the other fields stay.  DVBT2LL_EINVAL for a chain with a PLP whose
 * interleaving frame spans more than one T2 frame or that skips frames */
int dvbt2ll_t2mi_out_params_from_chain(const dvbt2ll_chain *chain, const int *plp_ids, dvbt2ll_t2mi_out_params *p);
/* the TS packets a call of nframes frames writes (0 .. max_frames), or a negative status */
int64_t dvbt2ll_t2mi_out_ts_packets(const dvbt2ll_t2mi_out *h, int nframes);
/* bb_dev[k]: PLP k's nframes x F_k BBFRAMEs on the device; aux_dev (NULL with naux = 0), aux_stride >= 0 and
 * aux_off[a] >= 0 (NULL with naux = 0): the auxiliary payloads; out_dev: room for out_cap_packets x 188 bytes.
 * Asynchronous on stream (NULL: the handle's own); no host round trip.  One run of a handle at a time: the next run
 * call on another stream first waits for the previous one.  DVBT2LL_EINVAL, nothing launched: a null pointer, nframes
 * outside 0 .. max_frames, start.frame < 0, packet_count outside 0 .. 255, cc outside 0 .. 15, a negative stride or
 * offset, out_cap_packets below dvbt2ll_t2mi_out_ts_packets(h, nframes). */
int dvbt2ll_t2mi_out_run_device(dvbt2ll_t2mi_out *h, const void *const *bb_dev, const void *aux_dev,
                                int64_t aux_stride, const int64_t *aux_off, const dvbt2ll_t2mi_out_pos *start,
                                int nframes, void *out_dev, int64_t out_cap_packets, void *stream);
/* synchronises with the last run and returns its result */
int dvbt2ll_t2mi_out_get_result(dvbt2ll_t2mi_out *h, dvbt2ll_t2mi_out_result *res);
/* host buffers, synchronous: the BBFRAMEs and the auxiliary bytes from aux up to the end of the last frame's last
 * payload are copied in, the written packets are copied out */
int dvbt2ll_t2mi_out_run_host(dvbt2ll_t2mi_out *h, const void *const *bb, const void *aux, int64_t aux_stride,
                              const int64_t *aux_off, const dvbt2ll_t2mi_out_pos *start, int nframes, void *out,
                              int64_t out_cap_packets, dvbt2ll_t2mi_out_result *res);
void dvbt2ll_t2mi_out_destroy(dvbt2ll_t2mi_out *h);

/* ---------------------------------------------------------------------------
 * ABI version.  The parameter and info structs are passed by pointer with no size field, so a caller
 * compiled against another layout would be read or written past its struct.  Version history:
 *   1  rounds 1-4: dvbt2ll_plp_params = the first nine ints, no num_subslices, no frames_per_if;
 *   2  round 5: dvbt2ll_plp_params + plp_type .. first_frame_idx (which moves every field of
 *      dvbt2ll_mplp_params / dvbt2ll_mplp_chain_params after plp[0]), dvbt2ll_mplp_params.num_subslices,
 *      dvbt2ll_chain_info.frames_per_if.
 * dvbt2ll_abi_check(DVBT2LL_ABI_VERSION, sizeof ...) (or the DVBT2LL_ABI_CHECK() macro) returns DVBT2LL_OK when the
 * caller's header is this library's, DVBT2LL_EINVAL otherwise; the adapters and the Python mirror call it
 * before their first create.
 * ------------------------------------------------------------------------- */
#define DVBT2LL_ABI_VERSION 2
int dvbt2ll_abi_version(void);
int dvbt2ll_abi_check(int abi_version, size_t sizeof_chain_params, size_t sizeof_chain_info,
                      size_t sizeof_plp_params, size_t sizeof_mplp_params, size_t sizeof_mplp_chain_params);
#define DVBT2LL_ABI_CHECK()                                                                                      \
  dvbt2ll_abi_check(DVBT2LL_ABI_VERSION, sizeof(dvbt2ll_chain_params), sizeof(dvbt2ll_chain_info),               \
                    sizeof(dvbt2ll_plp_params), sizeof(dvbt2ll_mplp_params), sizeof(dvbt2ll_mplp_chain_params))

#ifdef __cplusplus
}
#endif
#endif /* DVBT2LL_HIP_H */
