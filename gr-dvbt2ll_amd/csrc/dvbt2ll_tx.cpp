// dvbt2ll_tx -- native command-line DVB-T2 transmitter over the C ABI (include/dvbt2ll_hip.h):
// MPEG-TS file in, baseband IQ file out, whole T2 frames per GPU call.  It is the file-sink
// form of the shipped flowgraph apps/vv009-4kshort.grc (TS source -> the five blocks ->
// multiply_const -> sink): TS bytes -> the chain's streaming host path (dvbt2ll_chain_host_submit /
// _host_wait: a ring of DVBT2LL_HOST_RING batches in flight, page-locked buffers, so reading batch k + 1,
// encoding batch k and writing batch k - 2 overlap) -> complex64 or sc16 samples.
//
//   dvbt2ll_tx --preset cfg3 --in stream.ts --out iq.sc16 --format sc16 --gain 0.2
//   dvbt2ll_tx --mplp mix_4k --in plp0.ts --in plp1.ts --in plp2.ts --out iq.cf32
//   dvbt2ll_tx --preset cfg3 --input bbframe --in frames.bbf --out iq.cf32
//   dvbt2ll_tx --mplp mplp3_4k --input t2mi --pid 4096 --in gateway.ts --out iq.cf32
//
// --input bbframe reads a file of packed, unscrambled BBFRAMEs (kbch / 8 bytes each, back to back: what a T2
// gateway built) in place of a TS (dvbt2ll_chain_set_input).
//
// --input t2mi reads a transport stream carrying T2-MI (ETSI TS 102 773, DVB data piping) on --pid: the file is
// de-encapsulated on the GPU in chunks (dvbt2ll_t2mi_run_host, continued from each call's resume position), every
// PLP's BBFRAMEs are collected, and whole frames are encoded as they complete.  It works with single-PLP presets
// and with --mplp presets (one --in file for all PLPs; --plp-id per PLP, default 0, 1, ...).  Every interleaving
// frame must carry the preset's number of FEC blocks: dynamic PLP_NUM_BLOCKS is not supported and is refused.
//
// --input ts-npd reads an ordinary (multi-programme) TS and builds the BBFRAMEs itself on the GPU, in high-efficiency
// mode with null-packet deletion (dvbt2ll_modeadapt_run_host in chunks, continued from each call's resume position,
// flushed at the end of the file): --pids a,b,... selects the PLP's PIDs (default: every PID but 0x1FFF).  With
// --mplp presets the one --in file feeds every PLP, each through an adapter of its own: repeat --pids per PLP.
//
// --input ule reads IP datagrams (records of a 16-bit big-endian length and that many PDU bytes) and wraps them on the
// GPU in ULE SNDUs packed into TS packets of --pid (RFC 4326; dvbt2ll_ule_run_host in chunks, continued from each
// call's resume position, flushed at the end of the file): the reference flowgraph's ule_source.  --mac sets the
// destination address (default 02:00:48:55:4c:4b), --no-dest sends none (D = 1), --packing 0 starts a packet per
// SNDU.  The TS then goes through the chain's TS input exactly as a TS file does.
//
// --input mpe reads the same records and wraps them on the GPU in DSM-CC datagram_sections packed into TS packets of
// --pid (Multi-Protocol Encapsulation, EN 301 192 clause 7; dvbt2ll_mpe_run_host in chunks, continued from each call's
// resume position, flushed at the end of the file).  --mac sets the MAC address, --mac-from-dest gives datagrams to a
// multicast group the group's MAC, --packing 0 starts a packet per section.  The TS then goes through the chain's TS
// input exactly as a TS file does.
//
// --input mpe-fec reads the same records and groups them on the GPU into MPE-FEC frames of --rows rows, up to
// --data-columns application data columns and --rs-columns Reed-Solomon columns: MPE sections with real-time
// parameters, then MPE-FEC sections (dvbt2ll_mpefec_run_host in chunks, continued from each call's resume position,
// flushed at the end of the file).  --mac, --mac-from-dest and --packing as for --input mpe.
//
// --input gse reads the same records and wraps them on the GPU in GSE packets laid into normal-mode BBFRAMEs (TS 102
// 606-1; dvbt2ll_gse_run_host in chunks, continued from each call's resume position, flushed at the end of the file).
// --label / --label3 / --no-label choose the 6-byte, 3-byte or no label.  The BBFRAMEs then go through the chain's
// BBFRAME input exactly as a BBFRAME file does.
//
// --mux period=P,weight=W,psi-weight=V[,pcr-pid=N,pcr-weight=K,ts-rate=R] (with --input ule, mpe or mpe-fec) sends the
// encapsulated TS through the TS multiplexer before the chain reads it (dvbt2ll_tsmux_run_host, in calls of whole
// periods: at least 8192 slots, each continuing from the previous one's resume position, until the encapsulated TS is
// used up).  Input 0 is the encapsulated TS with W slots of P, and it is the fill input; input 1 is a one-programme
// PAT / PMT carousel (dvbt2ll_psi_build: transport_stream_id 1, version 0) with V slots, looped.  --program,
// --pmt-pid and --stream-type choose the PMT's values; its one stream is --pid, without descriptors.  pcr-pid adds K PCR
// packets per period (default 1) from a clock that starts at 0 and runs at ts-rate bits per second, and becomes the
// PMT's PCR_PID.  remap=FROM:TO (repeatable) sends input 0's packets of PID FROM out on PID TO (0x1FFF drops them); a
// remap of --pid also changes the PID the PMT names.  restamp-cc gives input 0's output PID and the carousel's PIDs new
// continuity counters, carried from call to call (dvbt2ll_tsmux_set_remux, dvbt2ll_tsmux_run_host_remux).
//
// --t2mi-out FILE --t2mi-pid N [--t2mi-stream-id S] writes, next to the IQ, the T2-MI transport stream of exactly the
// frames encoded (dvbt2ll_t2mi_out_run_host per batch, each batch continuing from the previous one's next position;
// no auxiliary slots): what a gateway would send to remote modulators, which produce the same IQ from it with
// --input t2mi.  It needs an input that yields BBFRAMEs: bbframe, ts-npd, gse or t2mi.
//
// --mplp runs a multi-PLP frame preset (one TS file per PLP, dvbt2ll_chain_create_mplp / _run_plps_host;
// batches are whole launch units, dvbt2ll_chain_unit_frames).
//
// The TS is consumed as one continuous stream (absolute offsets from the start of the file);
// frame k is encoded with the stream state the reference blocks would hold at that point.
// Trailing bytes that do not complete a T2 frame are left unused.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "dvbt2ll_hip.h"

namespace {

struct Preset {
  const char *name;
  int framesize, rate, constellation, rotation, fecblocks, tiblocks, carriermode, fftsize, guardinterval,
      l1constellation, pilotpattern, t2frames, numdatasyms;
};
// SURVEY.md section 6 configurations (enum values of include/dvbt2ll/dvbt2ll_config.h:60-202);
// cfg1 is the shipped flowgraph (apps/vv009-4kshort.grc:524-709)
const Preset kPresets[] = {
    {"cfg1", 0, 4, 3, 1, 8, 3, 0, 2, 0, 3, 6, 2, 3},
    {"cfg2", 1, 2, 2, 0, 148, 3, 0, 5, 4, 3, 6, 2, 59},
    {"cfg3", 1, 1, 3, 1, 195, 3, 1, 5, 1, 3, 3, 2, 59},
    {"cfg4", 1, 0, 1, 0, 24, 3, 0, 1, 0, 3, 6, 2, 59},
    {"cfg5", 1, 5, 3, 0, 197, 3, 0, 5, 4, 3, 6, 2, 59},
    {"cfg1q", 0, 0, 0, 1, 2, 3, 0, 2, 0, 3, 6, 2, 3},   // BASELINE config 1 as worded: QPSK 1/2
};

// multi-PLP presets (gr-dvbt2ll_amd/dvbt2ll/configs.py MPLP_CONFIGS / IF_CONFIGS of the same names): the
// common fields of dvbt2ll_mplp_params, then per PLP {framesize, rate, constellation, rotation, fecblocks,
// tiblocks, inputmode, inband, tsrate, plp_type, ti_type, ti_frames, frame_interval, first_frame_idx}
struct MplpPreset {
  const char *name;
  int common[12];
  int nplp;
  dvbt2ll_plp_params plp[3];
  int num_subslices;
};
const MplpPreset kMplpPresets[] = {
    // the GRC's 4K short frame as three Type-1 PLPs (256-QAM 4/5 rotated, QPSK 1/2, 16-QAM 3/5 HEM)
    {"mplp3_4k", {0, 2, 0, 3, 6, 2, 3, 0, 0, 0, 0, 0}, 3,
     {{0, 4, 3, 1, 2, 1, 0, 0, 4000000, 1, 0, 1, 1, 0}, {0, 0, 0, 0, 1, 0, 0, 0, 4000000, 1, 0, 1, 1, 0},
      {0, 1, 1, 1, 1, 2, 1, 0, 4000000, 1, 0, 1, 1, 0}}, 1},
    // the same frame with a Type-2 TIME_IL_TYPE 1 PLP (P_I = 2), a Type-1 PLP and a Type-2 HEM PLP, 6 sub-slices
    {"mix_4k", {0, 2, 0, 3, 6, 2, 3, 0, 0, 0, 0, 0}, 3,
     {{0, 4, 3, 1, 4, 1, 0, 0, 4000000, 2, 1, 2, 1, 0}, {0, 0, 0, 0, 1, 1, 0, 0, 4000000, 1, 0, 1, 1, 0},
      {0, 1, 1, 1, 1, 1, 1, 0, 4000000, 2, 0, 1, 1, 0}}, 6},
};

void usage(FILE *f) {
  std::fprintf(f,
               "usage: dvbt2ll_tx --in TS_FILE --out IQ_FILE [options]\n"
               "  --preset cfg1..cfg5|cfg1q parameter preset (default cfg1, the shipped flowgraph)\n"
               "  --mplp mplp3_4k|mix_4k    multi-PLP frame preset: give one --in per PLP\n"
               "  --set NAME=VALUE        override one chain parameter (framemapperfint_cc names:\n"
               "                          framesize rate constellation rotation fecblocks tiblocks\n"
               "                          carriermode fftsize guardinterval l1constellation\n"
               "                          pilotpattern t2frames numdatasyms paprmode version preamble\n"
               "                          inputmode reservedbiasbits l1scrambled inband; pilotgen:\n"
               "                          misogroup equalization bandwidth; bbheaderbch: tsrate)\n"
               "                          misogroup: 0 TX1, 1 TX2 (pilots only), 2 TX2 with MISO processing\n"
               "  --input ts|bbframe|t2mi|ts-npd|ule|mpe|mpe-fec|gse what --in holds: an MPEG-TS (default), packed unscrambled BBFRAMEs\n"
               "                          of kbch / 8 bytes each (single-PLP presets), or a TS carrying T2-MI\n"
               "                          (one file; single-PLP and --mplp presets)\n"
               "                          ts-npd: a TS adapted on the GPU to HEM BBFRAMEs with null-packet deletion\n"
               "                          ule: records of a 16-bit big-endian length and an IP datagram, wrapped on\n"
               "                          the GPU in ULE SNDUs (RFC 4326) on --pid (single-PLP presets)\n"
               "                          mpe: the same records, wrapped on the GPU in MPE datagram_sections (EN 301 192)\n"
               "                          on --pid (single-PLP presets)\n"
               "                          mpe-fec: the same records in MPE-FEC frames: MPE sections, then RS(255,191)\n"
               "                          columns in MPE-FEC sections, on --pid (single-PLP presets)\n"
               "                          gse: the same records, wrapped on the GPU in GSE packets (TS 102 606-1) in\n"
               "                          normal-mode BBFRAMEs (single-PLP presets)\n"
               "  --label aa:bb:cc:dd:ee:ff | --label3 aa:bb:cc | --no-label\n"
               "                          --input gse: the 6-byte label (default 02:00:48:55:4c:4b), a 3-byte one, none\n"
               "  --mac aa:bb:cc:dd:ee:ff --input ule / mpe: the destination / MAC address (default 02:00:48:55:4c:4b)\n"
               "  --mac-from-dest         --input mpe: a datagram to a multicast group carries the group's MAC\n"
               "  --rows R                --input mpe-fec: rows of a frame's tables, 256 / 512 / 768 / 1024 (default 1024)\n"
               "  --data-columns D        --input mpe-fec: the application data columns a frame may fill, 1 .. 191 (default 191)\n"
               "  --rs-columns K          --input mpe-fec: the RS columns sent, 1 .. 64 (default 64)\n"
               "  --no-dest               --input ule: SNDUs without a destination address (D = 1)\n"
               "  --packing 0|1           --input ule / mpe: pack SNDUs / sections back to back (default 1) or one per packet start\n"
               "  --mux period=P,weight=W,psi-weight=V[,pcr-pid=N,pcr-weight=K,ts-rate=R][,remap=FROM:TO]...[,restamp-cc]\n"
               "                          --input ule / mpe / mpe-fec: multiplex the encapsulated TS (W slots of P, and the\n"
               "                          free ones) with a PAT / PMT carousel (V slots), null packets and, with pcr-pid,\n"
               "                          K PCR packets per period of a TS of R bit/s; remap=FROM:TO moves a PID of the\n"
               "                          encapsulated TS (0x1FFF drops it), restamp-cc renumbers the continuity counters\n"
               "  --program N             --mux: the PMT's program_number (default 1)\n"
               "  --pmt-pid N             --mux: the PMT's PID (default 0x20)\n"
               "  --stream-type N         --mux: the stream_type of --pid in the PMT (default 0x0D)\n"
               "  --pids A,B,...          --input ts-npd: the PIDs of the next PLP of the preset (repeat per PLP;\n"
               "                          default: every PID but 0x1FFF)\n"
               "  --pid N                 --input t2mi / ule / mpe: the PID of the T2-MI stream / SNDUs / sections (default 4096)\n"
               "  --plp-id K              --input t2mi: the PLP_ID feeding the next PLP of the preset (repeat per\n"
               "                          PLP; default 0, 1, ...)\n"
               "  --t2mi-out FILE         also write the T2-MI TS of the frames encoded (--input bbframe, ts-npd, gse, t2mi)\n"
               "  --t2mi-pid N            its PID (default 4096); --t2mi-stream-id S: its t2mi_stream_id (default 0)\n"
               "  --format cf32|sc16      IQ sample format (default cf32, pilotgen's complex64)\n"
               "  --gain G                output gain (the flowgraph's multiply_const; default 1)\n"
               "  --frames N              T2 frames to encode (default: as many as the input holds)\n"
               "  --batch B               T2 frames per GPU call (default 16)\n"
               "  --device D              GPU index (default 0)\n"
               "  --print-params          print the resolved parameters and exit (no GPU)\n");
}

struct Field { const char *n; int *v; };
std::vector<Field> fields(dvbt2ll_chain_params &p) {
  dvbt2ll_framemapperfint_params &f = p.fm;
  return {
      {"framesize", &f.framesize}, {"rate", &f.rate}, {"constellation", &f.constellation},
      {"rotation", &f.rotation}, {"fecblocks", &f.fecblocks}, {"tiblocks", &f.tiblocks},
      {"carriermode", &f.carriermode}, {"fftsize", &f.fftsize}, {"guardinterval", &f.guardinterval},
      {"l1constellation", &f.l1constellation}, {"pilotpattern", &f.pilotpattern}, {"t2frames", &f.t2frames},
      {"numdatasyms", &f.numdatasyms}, {"paprmode", &f.paprmode}, {"version", &f.version},
      {"preamble", &f.preamble}, {"inputmode", &f.inputmode}, {"reservedbiasbits", &f.reservedbiasbits},
      {"l1scrambled", &f.l1scrambled}, {"inband", &f.inband}, {"misogroup", &p.misogroup},
      {"equalization", &p.equalization}, {"bandwidth", &p.bandwidth}, {"tsrate", &p.tsrate}};
}
int *field(dvbt2ll_chain_params &p, const std::string &n) {
  for (auto &e : fields(p))
    if (n == e.n) return e.v;
  return nullptr;
}

// stream position of payload byte J (HEM drops each packet's sync byte)
int64_t payload_pos(int64_t J, bool hem) { return hem ? 188 * (J / 187) + 1 + J % 187 : J; }

// one TS input: the stream window [base, base + buf.size()) of a file read as the frames need it
struct TsIn {
  FILE *f = nullptr;
  std::vector<uint8_t> buf;
  int64_t base = 0;
  bool eof = false;
  // make [lo, end) available (dropping bytes before lo); false if the file ends first
  bool span(int64_t lo, int64_t end) {
    if (lo > base) {
      const size_t drop = (size_t)std::min<int64_t>(lo - base, (int64_t)buf.size());
      buf.erase(buf.begin(), buf.begin() + drop);
      base = lo;
    }
    while (!eof && base + (int64_t)buf.size() < end) {
      size_t old = buf.size();
      buf.resize(old + (1 << 20));
      size_t got = std::fread(buf.data() + old, 1, buf.size() - old, f);
      buf.resize(old + got);
      if (got == 0) eof = true;
    }
    return base + (int64_t)buf.size() >= end;
  }
};

// --t2mi-out: the gateway's view of the frames encoded.  One framer call per batch; a batch's last TS packet is stuffed.
struct T2miOut {
  std::string path;
  int pid = 4096, stream_id = 0;
  dvbt2ll_t2mi_out *fr = nullptr;
  FILE *f = nullptr;
  dvbt2ll_t2mi_out_pos pos = {0, 0, 0};
  dvbt2ll_t2mi_out_result tot;
  std::vector<uint8_t> ts;
  int open(const dvbt2ll_chain *chain, const std::vector<int> &plp_ids, int batch, int device) {
    std::memset(&tot, 0, sizeof(tot));
    dvbt2ll_t2mi_out_params op;
    std::memset(&op, 0, sizeof(op));
    if (!plp_ids.empty() && (int)plp_ids.size() != dvbt2ll_chain_num_plps(chain)) return DVBT2LL_EINVAL;
    int st = dvbt2ll_t2mi_out_params_from_chain(chain, plp_ids.empty() ? nullptr : plp_ids.data(), &op);
    if (st) {
      std::fprintf(stderr, "dvbt2ll_tx: --t2mi-out: a PLP's interleaving frame spans several T2 frames or skips frames: not supported\n");
      return st;
    }
    op.pid = pid;
    op.t2mi_stream_id = stream_id;
    op.max_frames = batch;
    if ((st = dvbt2ll_t2mi_out_create(&op, device, &fr))) {
      std::fprintf(stderr, "dvbt2ll_tx: --t2mi-out: %s\n", dvbt2ll_strerror(st));
      return st;
    }
    ts.resize((size_t)dvbt2ll_t2mi_out_ts_packets(fr, batch) * 188);
    f = std::fopen(path.c_str(), "wb");
    if (!f) { std::fprintf(stderr, "dvbt2ll_tx: cannot open %s: %s\n", path.c_str(), std::strerror(errno)); return -1; }
    return 0;
  }
  // bb[k]: PLP k's BBFRAMEs of the n frames just encoded
  int write(const void *const *bb, int n) {
    dvbt2ll_t2mi_out_result res;
    int st = dvbt2ll_t2mi_out_run_host(fr, bb, nullptr, 0, nullptr, &pos, n, ts.data(), (int64_t)(ts.size() / 188), &res);
    if (st) { std::fprintf(stderr, "dvbt2ll_tx: --t2mi-out: %s\n", dvbt2ll_strerror(st)); return st; }
    if (std::fwrite(ts.data(), 188, (size_t)res.ts_packets, f) != (size_t)res.ts_packets) return -1;
    pos = res.next;
    int64_t *a = &tot.frames, *b = &res.frames;
    for (int i = 0; i < 5; i++) a[i] += b[i];
    return 0;
  }
  void close() {
    if (fr)
      std::fprintf(stderr, "dvbt2ll_tx: t2mi-out: %lld T2 frames, t2mi_packets %lld, ts_packets %lld, pusi_packets %lld, "
                   "stuffing_bytes %lld\n", (long long)tot.frames, (long long)tot.t2mi_packets, (long long)tot.ts_packets,
                   (long long)tot.pusi_packets, (long long)tot.stuffing_bytes);
    if (f) std::fclose(f);
    dvbt2ll_t2mi_out_destroy(fr);
    fr = nullptr;
    f = nullptr;
  }
};

constexpr int kInputT2mi = 2;   // --input t2mi (the chain itself runs in DVBT2LL_INPUT_BBFRAME)

// --input t2mi: the file's TS -> T2-MI deframer in chunks -> per-PLP BBFRAME queues -> whole launch units through
// dvbt2ll_chain_run_plps_host.  h: a chain of any preset, already in BBFRAME input with its output set.
int run_t2mi(dvbt2ll_chain *h, const std::string &in_path, const std::string &out_path, int fmt, int pid,
             const std::vector<int> &plp_ids, int64_t frames, int batch, int device, T2miOut *gw) {
  const int nplp = dvbt2ll_chain_num_plps(h), unit = dvbt2ll_chain_unit_frames(h);
  if (!plp_ids.empty() && (int)plp_ids.size() != nplp) {
    std::fprintf(stderr, "dvbt2ll_tx: --plp-id: give one per PLP (%d)\n", nplp);
    return 2;
  }
  if (batch % unit) { std::fprintf(stderr, "dvbt2ll_tx: --batch must be a multiple of the launch unit %d\n", unit); return 2; }
  dvbt2ll_chain_info pi[DVBT2LL_MAX_PLP];
  int st = 0;
  for (int k = 0; k < nplp && !st; k++) st = dvbt2ll_chain_get_plp_info(h, k, &pi[k]);
  dvbt2ll_t2mi_params tp;
  std::memset(&tp, 0, sizeof(tp));
  tp.pid = pid;
  tp.stream_id = -1;
  const int64_t chunk = 188 * 22310;   // about 4 MiB of TS per deframer call
  tp.max_ts_bytes = chunk;
  tp.max_packets = 65536;
  dvbt2ll_t2mi *de = nullptr;
  if (!st) st = dvbt2ll_t2mi_params_from_chain(h, plp_ids.empty() ? nullptr : plp_ids.data(), &tp);
  if (!st) st = dvbt2ll_t2mi_create(&tp, device, &de);
  if (st) { std::fprintf(stderr, "dvbt2ll_tx: t2mi: %s\n", dvbt2ll_strerror(st)); return 1; }
  FILE *fin = in_path == "-" ? stdin : std::fopen(in_path.c_str(), "rb");
  FILE *fout = out_path == "-" ? stdout : std::fopen(out_path.c_str(), "wb");
  if (!fin || !fout) {
    std::fprintf(stderr, "dvbt2ll_tx: cannot open %s: %s\n", !fin ? in_path.c_str() : out_path.c_str(), std::strerror(errno));
    dvbt2ll_t2mi_destroy(de);
    return 1;
  }
  const size_t sb = fmt == DVBT2LL_IQ_SC16 ? 4 : 8;
  std::vector<uint8_t> win, iq((size_t)batch * pi[0].iq_samples_per_frame * sb);
  std::vector<uint8_t> tmp[DVBT2LL_MAX_PLP], q[DVBT2LL_MAX_PLP];   // a call's blocks; the queue of validated blocks
  int64_t q_base[DVBT2LL_MAX_PLP] = {}, cap[DVBT2LL_MAX_PLP] = {}, whole[DVBT2LL_MAX_PLP] = {};
  int64_t in_frame[DVBT2LL_MAX_PLP] = {}, leading[DVBT2LL_MAX_PLP] = {};
  bool started[DVBT2LL_MAX_PLP] = {};
  void *optr[DVBT2LL_MAX_PLP] = {};
  for (int k = 0; k < nplp; k++) {
    cap[k] = chunk / tp.bbframe_bytes[k] + 1;
    tmp[k].resize((size_t)cap[k] * tp.bbframe_bytes[k]);
    optr[k] = tmp[k].data();
  }
  std::vector<dvbt2ll_t2mi_packet> recs;
  dvbt2ll_t2mi_result tot;
  std::memset(&tot, 0, sizeof(tot));
  dvbt2ll_t2mi_pos pos = {0, 0};
  bool eof = false, refused = false;
  int64_t done = 0;
  while (!st && !refused && (frames < 0 || done < frames)) {
    while (!eof && (int64_t)win.size() < chunk) {
      const size_t old = win.size();
      win.resize((size_t)chunk);
      const size_t got = std::fread(win.data() + old, 1, win.size() - old, fin);
      win.resize(old + got);
      if (got == 0) eof = true;
    }
    const int64_t len = (int64_t)win.size() / 188 * 188;
    dvbt2ll_t2mi_result res;
    if ((st = dvbt2ll_t2mi_run_host(de, win.data(), len, &pos, optr, cap, &res))) break;
    recs.resize((size_t)res.packets);
    if (res.packets && dvbt2ll_t2mi_get_packets(de, recs.data(), res.packets) != res.packets) { st = DVBT2LL_EDEVICE; break; }
    int64_t *a = &tot.ts_contributing, *b = &res.ts_contributing;
    for (int i = 0; i < 15; i++) a[i] += b[i];   // ts_contributing .. accepted
    tot.packets += res.packets;
    for (int i = 0; i < 256; i++) tot.by_type[i] += res.by_type[i];
    // the blocks in stream order: interleaving frames must hold exactly F blocks
    for (const dvbt2ll_t2mi_packet &r : recs) {
      if (r.out_index < 0 || r.block < 0) continue;
      const int k = r.out_index, F = pi[k].fec_blocks_per_frame, L = tp.bbframe_bytes[k];
      if (r.intl_frame_start) {
        if (started[k] && in_frame[k] != 0) {
          std::fprintf(stderr, "dvbt2ll_tx: PLP_ID %d: an interleaving frame of %lld FEC blocks, the preset has %d: "
                       "dynamic PLP_NUM_BLOCKS is not supported\n", tp.plp_id[k], (long long)in_frame[k], F);
          refused = true;
          break;
        }
        started[k] = true;
      } else if (!started[k]) {
        leading[k]++;   // the tail of an interleaving frame that began before the file
        continue;
      } else if (in_frame[k] == 0) {
        std::fprintf(stderr, "dvbt2ll_tx: PLP_ID %d: an interleaving frame of more than %d FEC blocks: dynamic "
                     "PLP_NUM_BLOCKS is not supported\n", tp.plp_id[k], F);
        refused = true;
        break;
      }
      tot.blocks[k]++;
      q[k].insert(q[k].end(), tmp[k].begin() + (size_t)r.block * L, tmp[k].begin() + (size_t)(r.block + 1) * L);
      if (++in_frame[k] == F) { in_frame[k] = 0; whole[k]++; }
    }
    if (refused) break;
    // encode the launch units every PLP has whole interleaving frames for
    for (;;) {
      int64_t n = frames >= 0 ? std::min<int64_t>(batch, frames - done) : batch;
      for (int k = 0; k < nplp; k++) n = std::min<int64_t>(n, whole[k] * pi[k].frames_per_if - done);
      n = n / unit * unit;
      if (n <= 0) break;
      const void *ptr[DVBT2LL_MAX_PLP];
      int64_t base[DVBT2LL_MAX_PLP], ql[DVBT2LL_MAX_PLP];
      for (int k = 0; k < nplp; k++) { ptr[k] = q[k].data(); base[k] = q_base[k]; ql[k] = (int64_t)q[k].size(); }
      if ((st = dvbt2ll_chain_run_plps_host(h, ptr, base, ql, done, (int)n, iq.data()))) break;
      const size_t bytes = (size_t)n * pi[0].iq_samples_per_frame * sb;
      if (std::fwrite(iq.data(), 1, bytes, fout) != bytes) { st = -1; break; }
      if (gw) {   // frames_per_if = 1 (T2miOut::open): frame `done` begins ts_bytes_per_frame x done into the stream
        const void *bb[DVBT2LL_MAX_PLP];
        for (int k = 0; k < nplp; k++) bb[k] = q[k].data() + (size_t)(done * pi[k].ts_bytes_per_frame - q_base[k]);
        if ((st = gw->write(bb, (int)n))) break;
      }
      done += n;
      for (int k = 0; k < nplp; k++) {   // drop the interleaving frames no later T2 frame needs
        const int64_t nb = done / pi[k].frames_per_if * pi[k].ts_bytes_per_frame;
        q[k].erase(q[k].begin(), q[k].begin() + (size_t)(nb - q_base[k]));
        q_base[k] = nb;
      }
    }
    // continue from the resume position: drop the TS before it
    const bool progress = res.resume.ts_offset > 0 || res.packets > 0;
    win.erase(win.begin(), win.begin() + (size_t)res.resume.ts_offset);
    pos.ts_offset = 0;
    pos.skip = res.resume.skip;
    if (eof && (!progress || win.size() < 188)) break;
    if (!progress && (int64_t)win.size() >= chunk) {
      std::fprintf(stderr, "dvbt2ll_tx: a T2-MI packet does not complete within %lld bytes of TS\n", (long long)chunk);
      st = -1;
    }
  }
  if (st) std::fprintf(stderr, "dvbt2ll_tx: t2mi run failed: %s\n", dvbt2ll_strerror(st));
  std::fprintf(stderr, "dvbt2ll_tx: t2mi: %lld T2 frames; %lld T2-MI packets, accepted %lld, broken %lld, crc_errors %lld, "
               "filtered %lld, len_errors %lld, other_plp %lld; TS packets: contributing %lld, foreign %lld, null %lld, "
               "tei %lld, scrambled %lld, bad_sync %lld, no_payload %lld, discontinuities %lld, bad_pointers %lld; blocks",
               (long long)done, (long long)tot.packets, (long long)tot.accepted, (long long)tot.broken,
               (long long)tot.crc_errors, (long long)tot.filtered, (long long)tot.len_errors, (long long)tot.other_plp,
               (long long)tot.ts_contributing, (long long)tot.ts_foreign, (long long)tot.ts_null, (long long)tot.ts_tei,
               (long long)tot.ts_scrambled, (long long)tot.ts_bad_sync, (long long)tot.ts_no_payload,
               (long long)tot.discontinuities, (long long)tot.bad_pointers);
  for (int k = 0; k < nplp; k++)
    std::fprintf(stderr, " %d:%lld(+%lld before the first frame start)", tp.plp_id[k], (long long)tot.blocks[k],
                 (long long)leading[k]);
  std::fprintf(stderr, "\n");
  if (fin != stdin) std::fclose(fin);
  if (fout != stdout) std::fclose(fout);
  dvbt2ll_t2mi_destroy(de);
  return refused ? 3 : st ? 1 : 0;
}

constexpr int kInputTsNpd = 3;   // --input ts-npd (the chain itself runs in DVBT2LL_INPUT_BBFRAME)

// --input ts-npd: the file's TS -> one mode adapter per PLP in chunks -> per-PLP BBFRAME queues -> whole launch units
// through dvbt2ll_chain_run_plps_host.  h: a chain of any preset, already in BBFRAME input with its output set.
int run_tsnpd(dvbt2ll_chain *h, const std::string &in_path, const std::string &out_path, int fmt,
              const std::vector<std::vector<int>> &pids, int64_t frames, int batch, int device, T2miOut *gw) {
  const int nplp = dvbt2ll_chain_num_plps(h), unit = dvbt2ll_chain_unit_frames(h);
  if (!pids.empty() && (int)pids.size() != nplp) {
    std::fprintf(stderr, "dvbt2ll_tx: --pids: give one list per PLP (%d)\n", nplp);
    return 2;
  }
  if (batch % unit) { std::fprintf(stderr, "dvbt2ll_tx: --batch must be a multiple of the launch unit %d\n", unit); return 2; }
  const int64_t chunk = 188 * 22310;   // about 4 MiB of TS per adapter call
  struct Plp {
    dvbt2ll_modeadapt *ad = nullptr;
    FILE *f = nullptr;
    dvbt2ll_chain_info info;
    std::vector<uint8_t> win, tmp, q;   // the TS window, one call's BBFRAMEs, the queue
    dvbt2ll_modeadapt_pos pos = {0, 0, 0};
    dvbt2ll_modeadapt_result tot;
    int64_t q_base = 0, L = 0;
    bool eof = false, done = false;
  };
  std::vector<Plp> pl(nplp);
  int st = 0;
  for (int k = 0; k < nplp && !st; k++) {
    Plp &p = pl[k];
    std::memset(&p.tot, 0, sizeof(p.tot));
    dvbt2ll_modeadapt_params mp;
    std::memset(&mp, 0, sizeof(mp));
    uint8_t mask[1024] = {};
    if (!pids.empty()) {
      for (int pid : pids[k])
        if (pid >= 0 && pid < 0x1FFF) mask[pid >> 3] |= (uint8_t)(1 << (pid & 7));
      mp.pid_mask = mask;
    }
    mp.npd = 1;
    mp.max_ts_bytes = chunk;
    if ((st = dvbt2ll_chain_get_plp_info(h, k, &p.info)) || (st = dvbt2ll_modeadapt_params_from_chain(h, k, &mp)) ||
        (st = dvbt2ll_modeadapt_create(&mp, device, &p.ad)))
      break;
    p.L = mp.kbch / 8;
    p.tmp.resize((size_t)(chunk / (p.L - 10) + 2) * p.L);
    p.f = std::fopen(in_path.c_str(), "rb");
    if (!p.f) { std::fprintf(stderr, "dvbt2ll_tx: cannot open %s: %s\n", in_path.c_str(), std::strerror(errno)); st = -1; }
  }
  FILE *fout = st ? nullptr : (out_path == "-" ? stdout : std::fopen(out_path.c_str(), "wb"));
  if (!st && !fout) { std::fprintf(stderr, "dvbt2ll_tx: cannot open %s\n", out_path.c_str()); st = -1; }
  const size_t sb = fmt == DVBT2LL_IQ_SC16 ? 4 : 8;
  std::vector<uint8_t> iq;
  if (!st) iq.resize((size_t)batch * pl[0].info.iq_samples_per_frame * sb);
  int64_t done = 0;
  while (!st && (frames < 0 || done < frames)) {
    const int64_t want = frames >= 0 ? std::min<int64_t>(batch, frames - done) : batch;
    // adapt until every PLP's queue covers the batch, or its file is used up
    for (int k = 0; k < nplp && !st; k++) {
      Plp &p = pl[k];
      const int64_t if_bytes = p.info.ts_bytes_per_frame;   // BBFRAME bytes of one interleaving frame
      while (!st && !p.done && (p.q_base + (int64_t)p.q.size()) / if_bytes * p.info.frames_per_if < done + want) {
        while (!p.eof && (int64_t)p.win.size() < chunk) {
          const size_t old = p.win.size();
          p.win.resize((size_t)chunk);
          const size_t got = std::fread(p.win.data() + old, 1, p.win.size() - old, p.f);
          p.win.resize(old + got);
          if (got == 0) p.eof = true;
        }
        const int64_t len = (int64_t)p.win.size() / 188 * 188;
        dvbt2ll_modeadapt_result res;
        if ((st = dvbt2ll_modeadapt_run_host(p.ad, p.win.data(), len, &p.pos, p.tmp.data(),
                                             (int64_t)(p.tmp.size() / p.L), p.eof, &res)))
          break;
        int64_t *a = &p.tot.packets_in, *b = &res.packets_in;
        for (int i = 0; i < 8; i++) a[i] += b[i];
        p.q.insert(p.q.end(), p.tmp.begin(), p.tmp.begin() + (size_t)(res.bbframes * p.L));
        p.win.erase(p.win.begin(), p.win.begin() + (size_t)(res.resume.ts_packet * 188));
        p.pos = {0, res.resume.unit_byte, res.resume.dnp};
        if (p.eof) p.done = true;   // flushed: nothing is left
        else if (res.resume.ts_packet == 0 && res.bbframes == 0 && (int64_t)p.win.size() >= chunk) {
          std::fprintf(stderr, "dvbt2ll_tx: PLP %d: no BBFRAME completes within %lld bytes of TS\n", k, (long long)chunk);
          st = -1;
        }
      }
    }
    if (st) break;
    int64_t n = want;
    for (int k = 0; k < nplp; k++)
      n = std::min<int64_t>(n, (pl[k].q_base + (int64_t)pl[k].q.size()) / pl[k].info.ts_bytes_per_frame *
                                   pl[k].info.frames_per_if - done);
    n = n / unit * unit;
    if (n <= 0) break;
    const void *ptr[DVBT2LL_MAX_PLP];
    int64_t base[DVBT2LL_MAX_PLP], ql[DVBT2LL_MAX_PLP];
    for (int k = 0; k < nplp; k++) { ptr[k] = pl[k].q.data(); base[k] = pl[k].q_base; ql[k] = (int64_t)pl[k].q.size(); }
    if ((st = dvbt2ll_chain_run_plps_host(h, ptr, base, ql, done, (int)n, iq.data()))) break;
    const size_t bytes = (size_t)n * pl[0].info.iq_samples_per_frame * sb;
    if (std::fwrite(iq.data(), 1, bytes, fout) != bytes) { st = -1; break; }
    if (gw) {
      const void *bb[DVBT2LL_MAX_PLP];
      for (int k = 0; k < nplp; k++) bb[k] = pl[k].q.data() + (size_t)(done * pl[k].info.ts_bytes_per_frame - pl[k].q_base);
      if ((st = gw->write(bb, (int)n))) break;
    }
    done += n;
    for (int k = 0; k < nplp; k++) {   // drop the interleaving frames no later T2 frame needs
      const int64_t nb = done / pl[k].info.frames_per_if * pl[k].info.ts_bytes_per_frame;
      pl[k].q.erase(pl[k].q.begin(), pl[k].q.begin() + (size_t)(nb - pl[k].q_base));
      pl[k].q_base = nb;
    }
  }
  if (st) std::fprintf(stderr, "dvbt2ll_tx: ts-npd run failed: %s\n", dvbt2ll_strerror(st));
  std::fprintf(stderr, "dvbt2ll_tx: ts-npd: %lld T2 frames\n", (long long)done);
  for (int k = 0; k < nplp; k++) {
    const dvbt2ll_modeadapt_result &t = pl[k].tot;
    std::fprintf(stderr, "dvbt2ll_tx: ts-npd: PLP %d: packets_in %lld, selected %lld, nulls_deleted %lld, nulls_kept %lld, "
                 "nulls_dropped_at_flush %lld, sync_errors %lld, bbframes %lld, flushed %lld\n", k,
                 (long long)t.packets_in, (long long)t.selected, (long long)t.nulls_deleted, (long long)t.nulls_kept,
                 (long long)t.nulls_dropped_at_flush, (long long)t.sync_errors, (long long)t.bbframes,
                 (long long)t.flushed);
    if (pl[k].f) std::fclose(pl[k].f);
    dvbt2ll_modeadapt_destroy(pl[k].ad);
  }
  if (fout && fout != stdout) std::fclose(fout);
  return st ? 1 : 0;
}

constexpr int kInputUle = 4;   // --input ule (the chain itself runs in DVBT2LL_INPUT_TS)

constexpr size_t kEncapChunk = 4 << 20, kEncapMaxPdus = 65536;   // PDU bytes and PDUs per encapsulator call

// What one of --input ule, mpe, mpe-fec and gse gives encap_file: its names in the stderr lines, its output unit, and
// its calls.  The callables hold the handle, the position carried from call to call and the counter totals.
struct Encap {
  const char *name, *unit;   // "ule", "packet"
  size_t unit_bytes;         // of an output unit: a TS packet, a BBFRAME
  bool more_at_eof;          // a flushed call can stop short of the last PDU (MPE-FEC's max_frames) and is continued
  // the capacity in units that holds n records of `bytes` bytes lying side by side
  std::function<int64_t(int64_t bytes, int64_t n)> bound;
  // one run_host call from the carried position: adds its counters to the totals, carries the position on, says how
  // many units it wrote and which PDU it resumes at
  std::function<int(const uint8_t *pdu, int64_t bytes, const uint32_t *off, int64_t n, uint8_t *out, int64_t cap,
                    bool flush, int64_t *units, int64_t *resume_pdu)> run;
  std::function<void()> report;   // the line of counter totals
};

// The file's length-prefixed PDUs -> an encapsulator in chunks, each call continuing from the previous one's resume
// position, flushed at the end of the file -> a temporary file of its output units, which the caller reads as it reads
// a TS or BBFRAME file.  Returns the file rewound, or nullptr.
FILE *encap_file(const Encap &b, const std::string &in_path) {
  FILE *fin = in_path == "-" ? stdin : std::fopen(in_path.c_str(), "rb");
  FILE *tmp = std::tmpfile();
  if (!fin || !tmp) {
    std::fprintf(stderr, "dvbt2ll_tx: cannot open %s: %s\n", !fin ? in_path.c_str() : "a temporary file", std::strerror(errno));
    return nullptr;
  }
  std::vector<uint8_t> pdus, out;
  std::vector<uint32_t> off(1, 0);
  bool eof = false;
  int st = 0;
  while (!st) {
    while (!eof && pdus.size() < kEncapChunk && off.size() <= kEncapMaxPdus) {
      uint8_t lb[2];
      if (std::fread(lb, 1, 2, fin) != 2) { eof = true; break; }
      const size_t len = ((size_t)lb[0] << 8) | lb[1], old = pdus.size();
      pdus.resize(old + len);
      if (len && std::fread(pdus.data() + old, 1, len, fin) != len) { pdus.resize(old); eof = true; break; }   // a cut record
      off.push_back((uint32_t)pdus.size());
    }
    const int64_t n = (int64_t)off.size() - 1;
    const int64_t cap = b.bound((int64_t)pdus.size(), n);
    out.resize((size_t)cap * b.unit_bytes);
    const uint8_t none = 0;
    int64_t units = 0, resume_pdu = 0;
    if ((st = b.run(pdus.empty() ? &none : pdus.data(), (int64_t)pdus.size(), off.data(), n, out.data(), cap, eof, &units,
                    &resume_pdu)))
      break;
    if (units && std::fwrite(out.data(), b.unit_bytes, (size_t)units, tmp) != (size_t)units) { st = -1; break; }
    // continue from the resume position: drop the PDUs before it
    const uint32_t cut = off[(size_t)resume_pdu];
    pdus.erase(pdus.begin(), pdus.begin() + cut);
    off.erase(off.begin(), off.begin() + (size_t)resume_pdu);
    for (uint32_t &o : off) o -= cut;
    const bool stuck = resume_pdu == 0 && units == 0;
    if (eof && (!b.more_at_eof || off.size() == 1 || stuck)) break;
    // nothing consumed and no room to read on (a short datagram with max_pdus skipped records behind it holds its
    // open packet or frame back for ever): give up, not loop
    if (stuck && (pdus.size() >= kEncapChunk || off.size() > kEncapMaxPdus)) {
      std::fprintf(stderr, "dvbt2ll_tx: %s: no %s completes within %zu bytes / %zu records\n", b.name, b.unit, pdus.size(),
                   off.size() - 1);
      st = -1;
      break;
    }
  }
  if (st) std::fprintf(stderr, "dvbt2ll_tx: %s run failed: %s\n", b.name, dvbt2ll_strerror(st));
  b.report();
  if (fin != stdin) std::fclose(fin);
  if (st) { std::fclose(tmp); return nullptr; }
  std::rewind(tmp);
  return tmp;
}

// --input ule: the ULE encapsulator's TS packets (encap_file)
FILE *run_ule(const std::string &in_path, int pid, int d_bit, const uint8_t *dest, int packing, int device) {
  dvbt2ll_ule_params up;
  std::memset(&up, 0, sizeof(up));
  up.pid = pid;
  up.d_bit = d_bit;
  std::memcpy(up.dest, dest, 6);
  up.packing = packing;
  up.max_pdu_bytes = (int64_t)kEncapChunk + 65536;
  up.max_pdus = (int)kEncapMaxPdus;
  dvbt2ll_ule *enc = nullptr;
  int st = dvbt2ll_ule_create(&up, device, &enc);
  if (st) { std::fprintf(stderr, "dvbt2ll_tx: ule: %s\n", dvbt2ll_strerror(st)); return nullptr; }
  dvbt2ll_ule_pos pos = {0, 0, 0};
  dvbt2ll_ule_result tot;
  std::memset(&tot, 0, sizeof(tot));
  Encap b = {"ule", "packet", 188, false, nullptr, nullptr, nullptr};
  b.bound = [&](int64_t bytes, int64_t n) {
    return packing ? (bytes + 14 * n) / 182 + 2 : (bytes + 14 * n) / 184 + n + 1;
  };
  b.run = [&](const uint8_t *pdu, int64_t bytes, const uint32_t *off, int64_t n, uint8_t *out, int64_t cap, bool flush,
              int64_t *units, int64_t *resume_pdu) {
    dvbt2ll_ule_result res;
    const int e = dvbt2ll_ule_run_host(enc, pdu, bytes, off, nullptr, n, &pos, out, cap, flush, &res);
    if (e) return e;
    int64_t *a = &tot.pdus_in, *c = &res.pdus_in;
    for (int i = 0; i < 8; i++) a[i] += c[i];
    pos = {0, res.resume.sndu_byte, res.resume.cc};
    *units = res.ts_packets;
    *resume_pdu = res.resume.pdu;
    return 0;
  };
  b.report = [&] {
    std::fprintf(stderr, "dvbt2ll_tx: ule: pdus_in %lld, sndus %lld, skipped_len %lld, skipped_type %lld, ts_packets %lld, "
                 "pusi_packets %lld, pad_bytes %lld, flushed %lld\n", (long long)tot.pdus_in, (long long)tot.sndus,
                 (long long)tot.skipped_len, (long long)tot.skipped_type, (long long)tot.ts_packets,
                 (long long)tot.pusi_packets, (long long)tot.pad_bytes, (long long)tot.flushed);
  };
  FILE *ts = encap_file(b, in_path);
  dvbt2ll_ule_destroy(enc);
  return ts;
}

constexpr int kInputMpe = 6;   // --input mpe (the chain itself runs in DVBT2LL_INPUT_TS)

// --input mpe: the MPE encapsulator's TS packets (encap_file)
FILE *run_mpe(const std::string &in_path, int pid, const uint8_t *mac, int mac_mode, int packing, int device) {
  dvbt2ll_mpe_params up;
  std::memset(&up, 0, sizeof(up));
  up.pid = pid;
  std::memcpy(up.mac, mac, 6);
  up.mac_mode = mac_mode;
  up.packing = packing;
  up.max_pdu_bytes = (int64_t)kEncapChunk + 65536;
  up.max_pdus = (int)kEncapMaxPdus;
  dvbt2ll_mpe *enc = nullptr;
  int st = dvbt2ll_mpe_create(&up, device, &enc);
  if (st) { std::fprintf(stderr, "dvbt2ll_tx: mpe: %s\n", dvbt2ll_strerror(st)); return nullptr; }
  dvbt2ll_mpe_pos pos = {0, 0, 0};
  dvbt2ll_mpe_result tot;
  std::memset(&tot, 0, sizeof(tot));
  Encap b = {"mpe", "packet", 188, false, nullptr, nullptr, nullptr};
  b.bound = [&](int64_t bytes, int64_t n) {
    return packing ? (bytes + 16 * n) / 183 + 2 : (bytes + 16 * n) / 184 + n + 1;
  };
  b.run = [&](const uint8_t *pdu, int64_t bytes, const uint32_t *off, int64_t n, uint8_t *out, int64_t cap, bool flush,
              int64_t *units, int64_t *resume_pdu) {
    dvbt2ll_mpe_result res;
    const int e = dvbt2ll_mpe_run_host(enc, pdu, bytes, off, n, &pos, out, cap, flush, &res);
    if (e) return e;
    int64_t *a = &tot.pdus_in, *c = &res.pdus_in;
    for (int i = 0; i < 9; i++) a[i] += c[i];
    pos = {0, res.resume.section_byte, res.resume.cc};
    *units = res.ts_packets;
    *resume_pdu = res.resume.pdu;
    return 0;
  };
  b.report = [&] {
    std::fprintf(stderr, "dvbt2ll_tx: mpe: pdus_in %lld, sections %lld, skipped_len %lld, skipped_type %lld, mapped_macs %lld, "
                 "ts_packets %lld, pusi_packets %lld, pad_bytes %lld, flushed %lld\n", (long long)tot.pdus_in,
                 (long long)tot.sections, (long long)tot.skipped_len, (long long)tot.skipped_type,
                 (long long)tot.mapped_macs, (long long)tot.ts_packets, (long long)tot.pusi_packets,
                 (long long)tot.pad_bytes, (long long)tot.flushed);
  };
  FILE *ts = encap_file(b, in_path);
  dvbt2ll_mpe_destroy(enc);
  return ts;
}

constexpr int kInputMpeFec = 7;   // --input mpe-fec (the chain itself runs in DVBT2LL_INPUT_TS)

// --input mpe-fec: the MPE-FEC encapsulator's TS packets (encap_file)
FILE *run_mpefec(const std::string &in_path, int pid, const uint8_t *mac, int mac_mode, int packing, int rows, int dcols,
                 int kcols, int device) {
  dvbt2ll_mpefec_params up;
  std::memset(&up, 0, sizeof(up));
  up.pid = pid;
  std::memcpy(up.mac, mac, 6);
  up.mac_mode = mac_mode;
  up.packing = packing;
  up.max_pdu_bytes = (int64_t)kEncapChunk + 65536;
  up.max_pdus = (int)kEncapMaxPdus;
  up.rows = rows;
  up.data_columns = dcols;
  up.rs_columns = kcols;
  up.max_frames = 256;
  dvbt2ll_mpefec *enc = nullptr;
  int st = dvbt2ll_mpefec_create(&up, device, &enc);
  if (st) { std::fprintf(stderr, "dvbt2ll_tx: mpe-fec: %s\n", dvbt2ll_strerror(st)); return nullptr; }
  dvbt2ll_mpefec_pos pos = {0, 0, 0, 0, 0};
  dvbt2ll_mpefec_result tot;
  std::memset(&tot, 0, sizeof(tot));
  Encap b = {"mpe-fec", "packet", 188, true, nullptr, nullptr, nullptr};
  // two successive frames hold more than a table's bytes, which bounds the frames, and so this many packets hold all
  // the sections
  b.bound = [&](int64_t bytes, int64_t n) {
    const int64_t fr = std::min<int64_t>(std::min<int64_t>(up.max_frames, n), 2 * bytes / ((int64_t)dcols * rows + 1) + 2);
    const int64_t all = bytes + 16 * n + fr * kcols * (rows + 16);
    return packing ? all / 183 + 2 : all / 184 + n + fr * kcols + 1;
  };
  b.run = [&](const uint8_t *pdu, int64_t bytes, const uint32_t *off, int64_t n, uint8_t *out, int64_t cap, bool flush,
              int64_t *units, int64_t *resume_pdu) {
    dvbt2ll_mpefec_result res;
    const int e = dvbt2ll_mpefec_run_host(enc, pdu, bytes, off, n, &pos, out, cap, flush, &res);
    if (e) return e;
    tot.pdus_in += res.pdus_in;
    tot.sections += res.sections;
    tot.fec_sections += res.fec_sections;
    tot.frames += res.frames;
    tot.skipped_len += res.skipped_len;
    tot.skipped_type += res.skipped_type;
    tot.mapped_macs += res.mapped_macs;
    tot.ts_packets += res.ts_packets;
    tot.pusi_packets += res.pusi_packets;
    tot.pad_bytes += res.pad_bytes;
    tot.flushed = res.flushed;   // the last call's
    pos = res.resume;
    pos.pdu = 0;
    *units = res.ts_packets;
    *resume_pdu = res.resume.pdu;
    return 0;
  };
  b.report = [&] {
    std::fprintf(stderr, "dvbt2ll_tx: mpe-fec: pdus_in %lld, sections %lld, fec_sections %lld, frames %lld, skipped_len %lld, "
                 "skipped_type %lld, mapped_macs %lld, ts_packets %lld, pusi_packets %lld, pad_bytes %lld, flushed %lld\n",
                 (long long)tot.pdus_in, (long long)tot.sections, (long long)tot.fec_sections, (long long)tot.frames,
                 (long long)tot.skipped_len, (long long)tot.skipped_type, (long long)tot.mapped_macs,
                 (long long)tot.ts_packets, (long long)tot.pusi_packets, (long long)tot.pad_bytes, (long long)tot.flushed);
  };
  FILE *ts = encap_file(b, in_path);
  dvbt2ll_mpefec_destroy(enc);
  return ts;
}

// --mux: the encapsulated TS (a temporary file) -> the TS multiplexer with a PSI carousel -> another temporary file,
// which the caller reads in its place.  Closes ts; returns the new file rewound, or nullptr.
struct MuxOpt {
  bool on = false;
  int period = 0, weight = 0, psi_weight = 0, pcr_pid = -1, pcr_weight = 1;
  long long ts_rate = 0;
  int program = 1, pmt_pid = 0x20, stream_type = 0x0D;
  std::vector<std::pair<int, int>> remap;   // remap=FROM:TO, input 0's PIDs
  bool restamp_cc = false;                  // new continuity counters for input 0 and the carousel
};

bool parse_mux(const char *arg, MuxOpt &m) {
  m.on = true;
  for (const char *c = arg; *c;) {
    const char *eq = std::strchr(c, '='), *end = std::strchr(c, ',');
    if (!end) end = c + std::strlen(c);
    if (std::string(c, end - c) == "restamp-cc") {
      m.restamp_cc = true;
      c = *end ? end + 1 : end;
      continue;
    }
    if (!eq || eq > end) return false;
    const std::string key(c, eq - c);
    if (key == "remap") {
      char *colon = nullptr;
      const long from = std::strtol(eq + 1, &colon, 0);
      if (!colon || *colon != ':' || colon > end) return false;
      m.remap.emplace_back((int)from, (int)std::strtol(colon + 1, nullptr, 0));
      c = *end ? end + 1 : end;
      continue;
    }
    const long long v = std::strtoll(eq + 1, nullptr, 0);
    if (key == "period") m.period = (int)v;
    else if (key == "weight") m.weight = (int)v;
    else if (key == "psi-weight") m.psi_weight = (int)v;
    else if (key == "pcr-pid") m.pcr_pid = (int)v;
    else if (key == "pcr-weight") m.pcr_weight = (int)v;
    else if (key == "ts-rate") m.ts_rate = v;
    else return false;
    c = *end ? end + 1 : end;
  }
  return true;
}

FILE *run_mux(FILE *ts, const MuxOpt &m, int pid, int device) {
  std::vector<uint8_t> in;
  uint8_t buf[188 * 256];
  for (size_t got; (got = std::fread(buf, 1, sizeof buf, ts)) > 0;) in.insert(in.end(), buf, buf + got);
  std::fclose(ts);
  dvbt2ll_psi_params pp;
  std::memset(&pp, 0, sizeof(pp));
  pp.transport_stream_id = 1;
  pp.n_programs = 1;
  pp.programs[0].program_number = m.program;
  pp.programs[0].pmt_pid = m.pmt_pid;
  pp.programs[0].pcr_pid = m.pcr_pid >= 0 ? m.pcr_pid : 0x1FFF;
  pp.programs[0].n_streams = 1;
  pp.programs[0].streams[0].stream_type = m.stream_type;
  int out_pid = pid;   // the PID the encapsulated stream leaves with, which is the one the PMT names
  for (const auto &e : m.remap)
    if (e.first == pid) out_pid = e.second;
  pp.programs[0].streams[0].pid = out_pid;
  const int64_t npsi = dvbt2ll_psi_build(&pp, nullptr, 0);
  if (npsi < 0 || m.pmt_pid == out_pid || m.pcr_pid == m.pmt_pid) { std::fprintf(stderr, "dvbt2ll_tx: mux: bad --program / --pmt-pid / --stream-type / --pid\n"); return nullptr; }
  std::vector<uint8_t> psi((size_t)npsi * 188);
  (void)dvbt2ll_psi_build(&pp, psi.data(), npsi);
  dvbt2ll_tsmux_params up;
  std::memset(&up, 0, sizeof(up));
  up.n_inputs = 2;
  up.period = m.period;
  up.weight[0] = m.weight;
  up.weight[1] = m.psi_weight;
  up.loop[1] = 1;
  up.fill_input = 0;
  up.pcr_pid = m.pcr_pid >= 0 ? m.pcr_pid : -1;
  up.pcr_weight = m.pcr_pid >= 0 ? m.pcr_weight : 0;
  up.ticks_per_period = m.pcr_pid >= 0 ? dvbt2ll_tsmux_ticks_per_period(m.period, m.ts_rate) : 0;
  const int64_t per_call = m.period > 0 ? (int64_t)m.period * std::max(1, 8192 / m.period) : 1;   // whole periods
  up.max_out_packets = (int)per_call;
  dvbt2ll_tsmux *mux = nullptr;
  int st = dvbt2ll_tsmux_create(&up, device, &mux);
  if (st) { std::fprintf(stderr, "dvbt2ll_tx: mux: %s\n", dvbt2ll_strerror(st)); return nullptr; }
  const bool remux = !m.remap.empty() || m.restamp_cc;
  if (remux) {
    dvbt2ll_tsmux_remux rx;
    std::memset(&rx, 0, sizeof(rx));
    if (m.remap.size() > DVBT2LL_TSMUX_MAP) st = DVBT2LL_EINVAL;
    for (size_t k = 0; !st && k < m.remap.size(); k++) {
      rx.map[k].input = 0;
      rx.map[k].from_pid = m.remap[k].first;
      rx.map[k].to_pid = m.remap[k].second;
      rx.n_map = (int)k + 1;
    }
    if (m.restamp_cc) {   // input 0's output PID, then the carousel's
      rx.track_pid[0] = out_pid;
      rx.track_pid[1] = 0;
      rx.track_pid[2] = m.pmt_pid;
      rx.n_track = 3;
      rx.restamp_cc[0] = rx.restamp_cc[1] = 1;
    }
    if (!st) st = dvbt2ll_tsmux_set_remux(mux, &rx);
    if (st) { std::fprintf(stderr, "dvbt2ll_tx: mux: bad remap= / restamp-cc\n"); dvbt2ll_tsmux_destroy(mux); return nullptr; }
  }
  FILE *out_f = std::tmpfile();
  if (!out_f) { std::fprintf(stderr, "dvbt2ll_tx: cannot open a temporary file: %s\n", std::strerror(errno)); dvbt2ll_tsmux_destroy(mux); return nullptr; }
  std::vector<uint8_t> out((size_t)per_call * 188);
  dvbt2ll_tsmux_pos pos;
  std::memset(&pos, 0, sizeof(pos));
  const int64_t total = (int64_t)(in.size() / 188);
  int64_t used = 0, slots = 0, psi_packets = 0, in_free = 0, pcr = 0, nulls = 0, sync = 0;
  dvbt2ll_tsmux_remux_pos rpos;
  std::memset(&rpos, 0, sizeof(rpos));
  int64_t remapped = 0, dropped = 0, cc_rewritten = 0, pcr_restamped = 0;
  while (!st && used < total) {
    // a call of per_call slots takes at most per_call packets, so it is given that window of the encapsulated TS
    const void *ptr[DVBT2LL_TSMUX_INPUTS] = {in.data() + (size_t)used * 188, psi.data()};
    const int64_t n_in[DVBT2LL_TSMUX_INPUTS] = {std::min(per_call, total - used), npsi};
    pos.next[0] = 0;
    dvbt2ll_tsmux_result res;
    dvbt2ll_tsmux_remux_result rres;
    std::memset(&rres, 0, sizeof(rres));
    if (remux) st = dvbt2ll_tsmux_run_host_remux(mux, ptr, n_in, &pos, &rpos, out.data(), per_call, &res, &rres);
    else st = dvbt2ll_tsmux_run_host(mux, ptr, n_in, &pos, out.data(), per_call, &res);
    if (st) break;
    rpos = rres.resume;
    remapped += rres.remapped;
    dropped += rres.dropped;
    cc_rewritten += rres.cc_rewritten;
    pcr_restamped += rres.pcr_restamped;
    if (std::fwrite(out.data(), 188, (size_t)per_call, out_f) != (size_t)per_call) { st = -1; break; }
    pos = res.resume;
    used += res.consumed[0];
    slots += per_call;
    psi_packets += res.consumed[1];
    in_free += res.fill_in_free;
    pcr += res.pcr_packets;
    nulls += res.null_packets;
    sync += res.sync_errors;
    if (res.consumed[0] == 0) { std::fprintf(stderr, "dvbt2ll_tx: mux: the schedule gives the input no slot\n"); st = -1; }
  }
  if (st) std::fprintf(stderr, "dvbt2ll_tx: mux run failed: %s\n", dvbt2ll_strerror(st));
  std::fprintf(stderr, "dvbt2ll_tx: mux: slots %lld, consumed %lld, psi_packets %lld, fill_in_free %lld, pcr_packets %lld, "
               "null_packets %lld, sync_errors %lld\n", (long long)slots, (long long)used, (long long)psi_packets,
               (long long)in_free, (long long)pcr, (long long)nulls, (long long)sync);
  if (remux)
    std::fprintf(stderr, "dvbt2ll_tx: remux: remapped %lld, dropped %lld, cc_rewritten %lld, pcr_restamped %lld\n",
                 (long long)remapped, (long long)dropped, (long long)cc_rewritten, (long long)pcr_restamped);
  dvbt2ll_tsmux_destroy(mux);
  if (st) { std::fclose(out_f); return nullptr; }
  std::rewind(out_f);
  return out_f;
}

constexpr int kInputGse = 5;   // --input gse (the chain itself runs in DVBT2LL_INPUT_BBFRAME)

// --input gse: the GSE encapsulator's BBFRAMEs (encap_file)
FILE *run_gse(const dvbt2ll_chain *chain, const std::string &in_path, int label_len, const uint8_t *label, int device) {
  dvbt2ll_gse_params gp;
  std::memset(&gp, 0, sizeof(gp));
  int st = dvbt2ll_gse_params_from_chain(chain, 0, &gp);
  gp.label_len = label_len;
  std::memcpy(gp.label, label, 6);
  gp.max_pdu_bytes = (int64_t)kEncapChunk + 65536;
  gp.max_pdus = (int)kEncapMaxPdus;
  dvbt2ll_gse *enc = nullptr;
  if (!st) st = dvbt2ll_gse_create(&gp, device, &enc);
  if (st) { std::fprintf(stderr, "dvbt2ll_tx: gse: %s\n", dvbt2ll_strerror(st)); return nullptr; }
  const int64_t Lb = gp.kbch / 8, D = Lb - 10;
  dvbt2ll_gse_pos pos = {0, 0, 0};
  dvbt2ll_gse_result tot;
  std::memset(&tot, 0, sizeof(tot));
  Encap b = {"gse", "frame", (size_t)Lb, false, nullptr, nullptr, nullptr};
  b.bound = [&](int64_t bytes, int64_t n) { return (bytes + (4 + label_len) * n) / (D - 14 - label_len) + 2; };
  b.run = [&](const uint8_t *pdu, int64_t bytes, const uint32_t *off, int64_t n, uint8_t *out, int64_t cap, bool flush,
              int64_t *units, int64_t *resume_pdu) {
    dvbt2ll_gse_result res;
    const int e = dvbt2ll_gse_run_host(enc, pdu, bytes, off, nullptr, n, &pos, out, cap, flush, &res);
    if (e) return e;
    int64_t *a = &tot.pdus_in, *c = &res.pdus_in;
    for (int i = 0; i < 9; i++) a[i] += c[i];
    pos = {0, res.resume.pdu_byte, res.resume.frag_id};
    *units = res.bbframes;
    *resume_pdu = res.resume.pdu;
    return 0;
  };
  b.report = [&] {
    std::fprintf(stderr, "dvbt2ll_tx: gse: pdus_in %lld, complete %lld, fragmented %lld, gse_packets %lld, skipped_len %lld, "
                 "skipped_type %lld, bbframes %lld, pad_bytes %lld, flushed %lld\n", (long long)tot.pdus_in,
                 (long long)tot.complete, (long long)tot.fragmented, (long long)tot.gse_packets, (long long)tot.skipped_len,
                 (long long)tot.skipped_type, (long long)tot.bbframes, (long long)tot.pad_bytes, (long long)tot.flushed);
  };
  FILE *bb = encap_file(b, in_path);
  dvbt2ll_gse_destroy(enc);
  return bb;
}

// the multi-PLP transmitter: whole launch units per batch, each PLP's TS span from its own file
int run_mplp(const MplpPreset &ps, const std::vector<std::string> &ins, const std::string &out_path, int fmt,
             float gain, int64_t frames, int batch, int device, bool print_params, int input = DVBT2LL_INPUT_TS,
             int pid = 0, const std::vector<int> &plp_ids = {}, const std::vector<std::vector<int>> &pids = {},
             T2miOut *gw = nullptr) {
  dvbt2ll_mplp_chain_params p;
  std::memset(&p, 0, sizeof(p));
  dvbt2ll_mplp_params &m = p.fm;
  int *c[12] = {&m.carriermode, &m.fftsize, &m.guardinterval, &m.l1constellation, &m.pilotpattern, &m.t2frames,
                &m.numdatasyms, &m.paprmode, &m.version, &m.preamble, &m.reservedbiasbits, &m.l1scrambled};
  for (int i = 0; i < 12; i++) *c[i] = ps.common[i];
  m.nplp = ps.nplp;
  for (int k = 0; k < ps.nplp; k++) m.plp[k] = ps.plp[k];
  m.num_subslices = ps.num_subslices;
  p.bandwidth = 4;   // BANDWIDTH_8_0_MHZ
  if (print_params) {   // the dvbt2ll_mplp_params ints (configs.MplpConfig.mplp_array layout)
    for (int i = 0; i < 12; i++) std::printf("%d ", *c[i]);
    std::printf("%d", m.nplp);
    for (int k = 0; k < DVBT2LL_MAX_PLP; k++) {
      const dvbt2ll_plp_params &q = m.plp[k];
      const int v[14] = {q.framesize, q.rate, q.constellation, q.rotation, q.fecblocks, q.tiblocks, q.inputmode,
                         q.inband, q.tsrate, q.plp_type, q.ti_type, q.ti_frames, q.frame_interval,
                         q.first_frame_idx};
      for (int x : v) std::printf(" %d", x);
    }
    std::printf(" %d\n", m.num_subslices);
    return 0;
  }
  const bool tsnpd = input == kInputTsNpd;
  const bool t2mi = input == kInputT2mi || tsnpd;   // one file for all PLPs, the chain in BBFRAME input
  if ((int)ins.size() != (t2mi ? 1 : ps.nplp) || out_path.empty()) {
    std::fprintf(stderr, "dvbt2ll_tx: --mplp %s needs %d --in file(s) and --out\n", ps.name, t2mi ? 1 : ps.nplp);
    return 2;
  }
  dvbt2ll_chain *h = nullptr;
  p.max_frames = batch;
  int st = dvbt2ll_chain_create_mplp(&p, device, &h);
  const int unit = st ? 1 : dvbt2ll_chain_unit_frames(h);
  if (!st && batch % unit) st = DVBT2LL_EINVAL;   // batches of whole launch units
  if (!st) st = dvbt2ll_chain_set_output(h, gain, fmt);
  if (!st && t2mi) st = dvbt2ll_chain_set_input(h, -1, DVBT2LL_INPUT_BBFRAME);
  if (st) {
    std::fprintf(stderr, "dvbt2ll_tx: chain: %s (batch must be a multiple of the launch unit)\n", dvbt2ll_strerror(st));
    dvbt2ll_chain_destroy(h);
    return 1;
  }
  if (t2mi) {
    int rc = gw && gw->open(h, plp_ids, batch, device) ? 1 : 0;
    if (!rc)
      rc = tsnpd ? run_tsnpd(h, ins[0], out_path, fmt, pids, frames, batch, device, gw)
                 : run_t2mi(h, ins[0], out_path, fmt, pid, plp_ids, frames, batch, device, gw);
    if (gw) gw->close();
    dvbt2ll_chain_destroy(h);
    return rc;
  }
  dvbt2ll_chain_info pi[DVBT2LL_MAX_PLP];
  std::vector<TsIn> ts(ps.nplp);
  for (int k = 0; k < ps.nplp && !st; k++) {
    st = dvbt2ll_chain_get_plp_info(h, k, &pi[k]);
    ts[k].f = std::fopen(ins[k].c_str(), "rb");
    if (!ts[k].f) { std::fprintf(stderr, "dvbt2ll_tx: cannot open %s\n", ins[k].c_str()); st = -1; }
  }
  FILE *fout = st ? nullptr : (out_path == "-" ? stdout : std::fopen(out_path.c_str(), "wb"));
  if (!st && !fout) { std::fprintf(stderr, "dvbt2ll_tx: cannot open %s\n", out_path.c_str()); st = -1; }
  const size_t sb = fmt == DVBT2LL_IQ_SC16 ? 4 : 8;
  std::vector<uint8_t> iq;
  if (!st) iq.resize((size_t)batch * pi[0].iq_samples_per_frame * sb);
  int64_t done = 0;
  while (!st && (frames < 0 || done < frames)) {
    int n = batch;
    if (frames >= 0 && frames - done < n) n = (int)((frames - done) / unit * unit);
    const void *ptr[DVBT2LL_MAX_PLP];
    int64_t base[DVBT2LL_MAX_PLP], len[DVBT2LL_MAX_PLP];
    for (; n > 0; n -= unit) {   // the most whole units every PLP's input still covers
      bool ok = true;
      for (int k = 0; k < ps.nplp && ok; k++) {
        const dvbt2ll_plp_params &q = ps.plp[k];
        const int P = pi[k].frames_per_if;
        const bool hem = q.inputmode != 0;
        const int64_t pay = (int64_t)pi[k].fec_blocks_per_frame * pi[k].payload_bytes_per_block - (q.inband ? 13 : 0);
        const int64_t start = payload_pos(done / P * pay, hem), end = payload_pos((done + n) / P * pay, hem) + 1;
        const int64_t lo = start >= 188 ? (start / 188) * 188 - 188 : 0;
        ok = ts[k].span(lo, end);
        ptr[k] = ts[k].buf.data();
        base[k] = ts[k].base;
        len[k] = (int64_t)ts[k].buf.size();
      }
      if (ok) break;
    }
    if (n <= 0) break;
    st = dvbt2ll_chain_run_plps_host(h, ptr, base, len, done, n, iq.data());
    if (st) { std::fprintf(stderr, "dvbt2ll_tx: run: %s\n", dvbt2ll_strerror(st)); break; }
    const size_t bytes = (size_t)n * pi[0].iq_samples_per_frame * sb;
    if (std::fwrite(iq.data(), 1, bytes, fout) != bytes) { st = -1; break; }
    done += n;
  }
  std::fprintf(stderr, "dvbt2ll_tx: %s: %lld T2 frames\n", ps.name, (long long)done);
  for (auto &t : ts)
    if (t.f) std::fclose(t.f);
  if (fout && fout != stdout) std::fclose(fout);
  dvbt2ll_chain_destroy(h);
  return st ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv) {
  std::string in_path, out_path, preset = "cfg1", mplp;
  std::vector<std::string> sets, ins;
  int fmt = DVBT2LL_IQ_CF32, input = DVBT2LL_INPUT_TS, batch = 16, device = 0, pid = 4096;
  std::vector<int> plp_ids;
  std::vector<std::vector<int>> pids;
  uint8_t mac[6] = {0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B};   // the flowgraph's ule_source
  int ule_d_bit = 0, ule_packing = 1, mpe_mac_mode = 0;
  int fec_rows = 1024, fec_dcols = 191, fec_kcols = 64;
  uint8_t gse_label[6] = {0x02, 0x00, 0x48, 0x55, 0x4C, 0x4B};
  int gse_label_len = 6;
  T2miOut gw;
  MuxOpt mux;
  bool print_params = false;
  int64_t frames = -1;
  float gain = 1.f;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto next = [&]() -> const char * {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "dvbt2ll_tx: %s needs a value\n", a.c_str());
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "-h" || a == "--help") { usage(stdout); return 0; }
    else if (a == "--in") ins.push_back(in_path = next());
    else if (a == "--mplp") mplp = next();
    else if (a == "--out") out_path = next();
    else if (a == "--preset") preset = next();
    else if (a == "--set") sets.push_back(next());
    else if (a == "--format") {
      std::string v = next();
      if (v == "cf32") fmt = DVBT2LL_IQ_CF32;
      else if (v == "sc16") fmt = DVBT2LL_IQ_SC16;
      else { std::fprintf(stderr, "dvbt2ll_tx: unknown format %s\n", v.c_str()); return 2; }
    } else if (a == "--input") {
      std::string v = next();
      if (v == "ts") input = DVBT2LL_INPUT_TS;
      else if (v == "bbframe") input = DVBT2LL_INPUT_BBFRAME;
      else if (v == "t2mi") input = kInputT2mi;
      else if (v == "ts-npd") input = kInputTsNpd;
      else if (v == "ule") input = kInputUle;
      else if (v == "mpe") input = kInputMpe;
      else if (v == "mpe-fec") input = kInputMpeFec;
      else if (v == "gse") input = kInputGse;
      else { std::fprintf(stderr, "dvbt2ll_tx: unknown input %s\n", v.c_str()); return 2; }
    } else if (a == "--pid") pid = (int)std::strtol(next(), nullptr, 0);
    else if (a == "--pids") {
      std::vector<int> one;
      for (const char *c = next(); *c;) {
        char *end;
        one.push_back((int)std::strtol(c, &end, 0));
        if (end == c) { std::fprintf(stderr, "dvbt2ll_tx: bad --pids list\n"); return 2; }
        c = *end == ',' ? end + 1 : end;
      }
      pids.push_back(one);
    } else if (a == "--mac") {
      unsigned m[6];
      if (std::sscanf(next(), "%2x:%2x:%2x:%2x:%2x:%2x", &m[0], &m[1], &m[2], &m[3], &m[4], &m[5]) != 6) {
        std::fprintf(stderr, "dvbt2ll_tx: bad --mac\n");
        return 2;
      }
      for (int k = 0; k < 6; k++) mac[k] = (uint8_t)m[k];
    } else if (a == "--label" || a == "--label3") {
      unsigned m[6] = {};
      const int want = a == "--label" ? 6 : 3;
      if (std::sscanf(next(), "%2x:%2x:%2x:%2x:%2x:%2x", &m[0], &m[1], &m[2], &m[3], &m[4], &m[5]) != want) {
        std::fprintf(stderr, "dvbt2ll_tx: bad %s\n", a.c_str());
        return 2;
      }
      for (int k = 0; k < 6; k++) gse_label[k] = (uint8_t)m[k];
      gse_label_len = want;
    } else if (a == "--no-label") gse_label_len = 0;
    else if (a == "--no-dest") ule_d_bit = 1;
    else if (a == "--mac-from-dest") mpe_mac_mode = 1;
    else if (a == "--packing") ule_packing = std::atoi(next());
    else if (a == "--rows") fec_rows = std::atoi(next());
    else if (a == "--data-columns") fec_dcols = std::atoi(next());
    else if (a == "--rs-columns") fec_kcols = std::atoi(next());
    else if (a == "--mux") {
      if (!parse_mux(next(), mux)) { std::fprintf(stderr, "dvbt2ll_tx: bad --mux\n"); return 2; }
    } else if (a == "--program") mux.program = (int)std::strtol(next(), nullptr, 0);
    else if (a == "--pmt-pid") mux.pmt_pid = (int)std::strtol(next(), nullptr, 0);
    else if (a == "--stream-type") mux.stream_type = (int)std::strtol(next(), nullptr, 0);
    else if (a == "--plp-id") plp_ids.push_back((int)std::strtol(next(), nullptr, 0));
    else if (a == "--t2mi-out") gw.path = next();
    else if (a == "--t2mi-pid") gw.pid = (int)std::strtol(next(), nullptr, 0);
    else if (a == "--t2mi-stream-id") gw.stream_id = (int)std::strtol(next(), nullptr, 0);
    else if (a == "--gain") gain = std::strtof(next(), nullptr);
    else if (a == "--frames") frames = std::strtoll(next(), nullptr, 10);
    else if (a == "--batch") batch = std::atoi(next());
    else if (a == "--device") device = std::atoi(next());
    else if (a == "--print-params") print_params = true;
    else { std::fprintf(stderr, "dvbt2ll_tx: unknown option %s\n", a.c_str()); usage(stderr); return 2; }
  }

  T2miOut *gwp = gw.path.empty() ? nullptr : &gw;
  if (gwp && !print_params && (input == DVBT2LL_INPUT_TS || input == kInputUle || input == kInputMpe || input == kInputMpeFec)) {
    std::fprintf(stderr, "dvbt2ll_tx: --t2mi-out needs an input that yields BBFRAMEs: --input bbframe, ts-npd, gse or t2mi\n");
    return 2;
  }
  if (mux.on && input != kInputUle && input != kInputMpe && input != kInputMpeFec) {
    std::fprintf(stderr, "dvbt2ll_tx: --mux needs --input ule, mpe or mpe-fec\n");
    return 2;
  }
  if (!mplp.empty()) {
    if (input == DVBT2LL_INPUT_BBFRAME || input == kInputUle || input == kInputMpe || input == kInputMpeFec || input == kInputGse) {
      std::fprintf(stderr, "dvbt2ll_tx: --input bbframe / ule / mpe / mpe-fec / gse takes a single-PLP preset\n");
      return 2;
    }
    for (auto &q : kMplpPresets)
      if (mplp == q.name)
        return run_mplp(q, ins, out_path, fmt, gain, frames, batch, device, print_params, input, pid, plp_ids, pids, gwp);
    std::fprintf(stderr, "dvbt2ll_tx: unknown multi-PLP preset %s\n", mplp.c_str());
    return 2;
  }
  dvbt2ll_chain_params p;
  std::memset(&p, 0, sizeof(p));
  const Preset *ps = nullptr;
  for (auto &q : kPresets)
    if (preset == q.name) ps = &q;
  if (!ps) { std::fprintf(stderr, "dvbt2ll_tx: unknown preset %s\n", preset.c_str()); return 2; }
  dvbt2ll_framemapperfint_params &f = p.fm;
  f.framesize = ps->framesize; f.rate = ps->rate; f.constellation = ps->constellation; f.rotation = ps->rotation;
  f.fecblocks = ps->fecblocks; f.tiblocks = ps->tiblocks; f.carriermode = ps->carriermode; f.fftsize = ps->fftsize;
  f.guardinterval = ps->guardinterval; f.l1constellation = ps->l1constellation; f.pilotpattern = ps->pilotpattern;
  f.t2frames = ps->t2frames; f.numdatasyms = ps->numdatasyms;
  p.tsrate = 4000000;
  p.bandwidth = 4;   // BANDWIDTH_8_0_MHZ
  for (auto &s : sets) {
    size_t eq = s.find('=');
    int *v = eq == std::string::npos ? nullptr : field(p, s.substr(0, eq));
    if (!v) { std::fprintf(stderr, "dvbt2ll_tx: bad --set %s\n", s.c_str()); return 2; }
    *v = std::atoi(s.c_str() + eq + 1);
  }
  p.max_frames = batch;
  if (print_params) {
    for (auto &e : fields(p)) std::printf("%s=%d\n", e.n, *e.v);
    return 0;
  }
  if (in_path.empty() || out_path.empty() || batch < 1) { usage(stderr); return 2; }

  dvbt2ll_chain *h = nullptr;
  int st = dvbt2ll_chain_create(&p, device, &h);
  if (st) { std::fprintf(stderr, "dvbt2ll_tx: chain create: %s\n", dvbt2ll_strerror(st)); return 1; }
  dvbt2ll_chain_info info;
  // (the info after set_input: it then counts whole BBFRAMEs)
  const bool tsnpd = input == kInputTsNpd, ule = input == kInputUle, mpe = input == kInputMpe, gse = input == kInputGse;
  const bool mpefec = input == kInputMpeFec;
  const bool t2mi = input == kInputT2mi || tsnpd;
  if (ule || mpe || mpefec) input = DVBT2LL_INPUT_TS;   // the encapsulator's TS is read as a TS file is
  if (gse) input = DVBT2LL_INPUT_BBFRAME;   // the encapsulator's BBFRAMEs are read as a BBFRAME file is
  if ((st = dvbt2ll_chain_set_input(h, -1, t2mi ? DVBT2LL_INPUT_BBFRAME : input)) || (st = dvbt2ll_chain_get_info(h, &info)) ||
      (st = dvbt2ll_chain_set_output(h, gain, fmt))) {
    std::fprintf(stderr, "dvbt2ll_tx: %s\n", dvbt2ll_strerror(st));
    dvbt2ll_chain_destroy(h);
    return 1;
  }
  if (gwp && gwp->open(h, plp_ids, batch, device)) {
    gwp->close();
    dvbt2ll_chain_destroy(h);
    return 1;
  }
  if (t2mi) {
    const int rc = tsnpd ? run_tsnpd(h, in_path, out_path, fmt, pids, frames, batch, device, gwp)
                         : run_t2mi(h, in_path, out_path, fmt, pid, plp_ids, frames, batch, device, gwp);
    if (gwp) gwp->close();
    dvbt2ll_chain_destroy(h);
    return rc;
  }
  FILE *fin = ule ? run_ule(in_path, pid, ule_d_bit, mac, ule_packing, device)
                  : mpe ? run_mpe(in_path, pid, mac, mpe_mac_mode, ule_packing, device)
                  : mpefec ? run_mpefec(in_path, pid, mac, mpe_mac_mode, ule_packing, fec_rows, fec_dcols, fec_kcols, device)
                  : gse ? run_gse(h, in_path, gse_label_len, gse_label, device)
                  : in_path == "-" ? stdin : std::fopen(in_path.c_str(), "rb");
  if (mux.on && fin) fin = run_mux(fin, mux, pid, device);
  if ((ule || mpe || mpefec || gse) && !fin) {
    if (gwp) gwp->close();
    dvbt2ll_chain_destroy(h);
    return 1;
  }
  FILE *fout = out_path == "-" ? stdout : std::fopen(out_path.c_str(), "wb");
  if (!fin || !fout) {
    std::fprintf(stderr, "dvbt2ll_tx: cannot open %s: %s\n", !fin ? in_path.c_str() : out_path.c_str(),
                 std::strerror(errno));
    dvbt2ll_chain_destroy(h);
    return 1;
  }
  const bool hem = f.inputmode != 0;
  // payload bytes per frame: F BBFRAME payloads less the in-band type B field of the first
  const int64_t pay_frame = (int64_t)info.fec_blocks_per_frame * info.payload_bytes_per_block - (f.inband ? 13 : 0);
  const size_t sample_bytes = fmt == DVBT2LL_IQ_SC16 ? 4 : 8;
  std::vector<uint8_t> ts;                 // stream bytes [ts_base, ts_base + ts.size())
  int64_t ts_base = 0;
  bool eof = false;
  // the ring: batch k's TS span and IQ in page-locked buffers of slot k % R until it is written out
  constexpr int R = DVBT2LL_HOST_RING;
  const size_t iq_slot = (size_t)batch * info.iq_samples_per_frame * sample_bytes;
  const bool bbf = input == DVBT2LL_INPUT_BBFRAME;
  // stream bytes [lo, end) the frames [first, first + n) consume: a TS span has the packet before the first one
  // touched (its CRC-8 replaces the next sync byte); BBFRAME input: the frames' BBFRAMEs and nothing else
  auto span_of = [&](int64_t first, int64_t n, int64_t *lo, int64_t *end) {
    if (bbf) {
      *lo = first * info.ts_bytes_per_frame;
      *end = (first + n) * info.ts_bytes_per_frame;
      return;
    }
    const int64_t start = payload_pos(first * pay_frame, hem);
    *end = payload_pos((first + n) * pay_frame, hem) + 1;
    *lo = start >= 188 ? (start / 188) * 188 - 188 : 0;
  };
  const size_t ts_slot = bbf ? (size_t)((int64_t)batch * info.ts_bytes_per_frame)
                             : (size_t)(payload_pos((int64_t)batch * pay_frame, hem) + 4 * 188);
  void *ts_pin[R] = {}, *iq_pin[R] = {};
  int64_t ticket[R] = {}, slot_frames[R] = {};
  for (int k = 0; k < R; k++)
    if (!(ts_pin[k] = dvbt2ll_host_alloc(ts_slot)) || !(iq_pin[k] = dvbt2ll_host_alloc(iq_slot))) {
      std::fprintf(stderr, "dvbt2ll_tx: page-locked host buffers: out of memory\n");
      st = DVBT2LL_ENOMEM;
    }
  int64_t done = 0, written = 0, submitted = 0;
  // write out the oldest batch in flight (waits for its copy-out)
  auto drain_one = [&]() -> bool {
    const int sl = (int)(written % R);
    int e = dvbt2ll_chain_host_wait(h, ticket[sl]);
    if (e) { std::fprintf(stderr, "dvbt2ll_tx: run: %s\n", dvbt2ll_strerror(e)); st = e; return false; }
    const size_t bytes = (size_t)slot_frames[sl] * info.iq_samples_per_frame * sample_bytes;
    if (std::fwrite(iq_pin[sl], 1, bytes, fout) != bytes) {
      std::fprintf(stderr, "dvbt2ll_tx: write failed: %s\n", std::strerror(errno));
      st = -1;
      return false;
    }
    written++;
    return true;
  };
  const auto t0 = std::chrono::steady_clock::now();
  while (!st && (frames < 0 || done < frames)) {
    int n = batch;
    if (frames >= 0 && frames - done < n) n = (int)(frames - done);
    int64_t lo, end;
    span_of(done, n, &lo, &end);
    if (lo > ts_base) {                    // drop bytes no later frame needs
      ts.erase(ts.begin(), ts.begin() + (lo - ts_base));
      ts_base = lo;
    }
    while (!eof && ts_base + (int64_t)ts.size() < end) {
      size_t old = ts.size();
      ts.resize(old + (1 << 20));
      size_t got = std::fread(ts.data() + old, 1, ts.size() - old, fin);
      ts.resize(old + got);
      if (got == 0) eof = true;
    }
    while (n > 0 && ts_base + (int64_t)ts.size() < end) {   // short input: fewer frames
      n--;
      span_of(done, n, &lo, &end);
    }
    if (n == 0) break;
    if (submitted - written == R && !drain_one()) break;   // the slot's previous batch goes out first
    const int sl = (int)(submitted % R);
    const int64_t span = end - lo;
    if ((size_t)span > ts_slot) { st = DVBT2LL_EINVAL; break; }
    std::memcpy(ts_pin[sl], ts.data() + (lo - ts_base), (size_t)span);
    st = dvbt2ll_chain_host_submit(h, ts_pin[sl], lo, span, done, n, iq_pin[sl], &ticket[sl]);
    if (st) { std::fprintf(stderr, "dvbt2ll_tx: run: %s\n", dvbt2ll_strerror(st)); break; }
    if (gwp) {   // BBFRAME input: the span is exactly the n frames' BBFRAMEs
      const void *bb[1] = {ts_pin[sl]};
      if ((st = gwp->write(bb, n))) break;
    }
    slot_frames[sl] = n;
    submitted++;
    done += n;
  }
  while (!st && written < submitted && drain_one()) {
  }
  const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::fprintf(stderr, "dvbt2ll_tx: %lld T2 frames, %lld samples (%s, gain %g) in %.3f s: %.1f Msamples/s\n",
               (long long)done, (long long)(done * info.iq_samples_per_frame), fmt ? "sc16" : "cf32", gain, dt,
               dt > 0 ? done * info.iq_samples_per_frame / dt / 1e6 : 0.0);
  if (fin != stdin) std::fclose(fin);
  if (fout != stdout) std::fclose(fout);
  if (gwp) gwp->close();
  (void)dvbt2ll_chain_synchronize(h);
  for (int k = 0; k < R; k++) {
    if (submitted > written) (void)dvbt2ll_chain_host_wait(h, ticket[k]);   // nothing in flight on the buffers
    dvbt2ll_host_free(ts_pin[k]);
    dvbt2ll_host_free(iq_pin[k]);
  }
  dvbt2ll_chain_destroy(h);
  return st ? 1 : 0;
}
