"""ctypes loader for the in-tree HIP library libdvbt2ll_hip.so (built by __graft_entry__.build()).

There is no CPU fallback: if the shared library is missing this module raises, so a GPU
test can never pass on a silent host path.
"""
import ctypes
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "libdvbt2ll_hip.so"

_lib = None


class DVBT2Error(RuntimeError):
    pass


class _FmParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "framesize", "rate", "constellation", "rotation", "fecblocks", "tiblocks", "carriermode",
        "fftsize", "guardinterval", "l1constellation", "pilotpattern", "t2frames", "numdatasyms",
        "paprmode", "version", "preamble", "inputmode", "reservedbiasbits", "l1scrambled", "inband")]


class _BbParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("framesize", "rate", "mode", "inband", "fecblocks", "tsrate")]


class _LdpcParams(ctypes.Structure):
    _fields_ = [("framesize", ctypes.c_int), ("rate", ctypes.c_int)]


class _ImParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("framesize", "rate", "constellation", "rotation")]


class _PgParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "carriermode", "fftsize", "pilotpattern", "guardinterval", "numdatasyms", "paprmode", "version",
        "preamble", "misogroup", "equalization", "bandwidth", "vlength")]


class _ChainParams(ctypes.Structure):
    _fields_ = [("fm", _FmParams), ("misogroup", ctypes.c_int), ("equalization", ctypes.c_int),
                ("bandwidth", ctypes.c_int), ("max_frames", ctypes.c_int), ("tsrate", ctypes.c_int)]


MAX_PLP = 8   # DVBT2LL_MAX_PLP
ABI_VERSION = 2   # DVBT2LL_ABI_VERSION


class _PlpParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "framesize", "rate", "constellation", "rotation", "fecblocks", "tiblocks", "inputmode", "inband", "tsrate",
        "plp_type", "ti_type", "ti_frames", "frame_interval", "first_frame_idx")]


PLP_INTS = len(_PlpParams._fields_)


class _MplpParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in (
        "carriermode", "fftsize", "guardinterval", "l1constellation", "pilotpattern", "t2frames", "numdatasyms",
        "paprmode", "version", "preamble", "reservedbiasbits", "l1scrambled", "nplp")] + [
        ("plp", _PlpParams * MAX_PLP), ("num_subslices", ctypes.c_int)]

    @classmethod
    def from_config(cls, mcfg):
        """dvbt2ll_mplp_params of a dvbt2ll.configs.MplpConfig"""
        a = mcfg.mplp_array()
        p = cls(*a[:13])
        for k in range(MAX_PLP):
            p.plp[k] = _PlpParams(*a[13 + PLP_INTS * k:13 + PLP_INTS * (k + 1)])
        p.num_subslices = a[13 + PLP_INTS * MAX_PLP]
        return p


class _MplpChainParams(ctypes.Structure):
    _fields_ = [("fm", _MplpParams), ("misogroup", ctypes.c_int), ("equalization", ctypes.c_int),
                ("bandwidth", ctypes.c_int), ("max_frames", ctypes.c_int)]


class _ChainInfo(ctypes.Structure):
    _fields_ = [("fec_blocks_per_frame", ctypes.c_int), ("payload_bytes_per_block", ctypes.c_int),
                ("ts_bytes_per_frame", ctypes.c_int64), ("iq_samples_per_frame", ctypes.c_int64),
                ("cell_size", ctypes.c_int), ("stream_items", ctypes.c_int), ("mapped_items", ctypes.c_int),
                ("num_symbols", ctypes.c_int), ("fft_size", ctypes.c_int), ("guard_interval", ctypes.c_int),
                ("cw_stride_bytes", ctypes.c_int64), ("frames_per_if", ctypes.c_int)]


class _T2miParams(ctypes.Structure):
    _fields_ = [("pid", ctypes.c_int), ("stream_id", ctypes.c_int), ("nplp", ctypes.c_int),
                ("plp_id", ctypes.c_int * MAX_PLP), ("bbframe_bytes", ctypes.c_int * MAX_PLP),
                ("max_ts_bytes", ctypes.c_int64), ("max_packets", ctypes.c_int)]


class _T2miPos(ctypes.Structure):
    _fields_ = [("ts_offset", ctypes.c_int64), ("skip", ctypes.c_int)]


class _T2miResult(ctypes.Structure):
    _fields_ = [("resume", _T2miPos), ("packets", ctypes.c_int64)] + [(n, ctypes.c_int64) for n in (
        "ts_contributing", "ts_foreign", "ts_null", "ts_tei", "ts_scrambled", "ts_bad_sync", "ts_no_payload",
        "discontinuities", "bad_pointers", "broken", "crc_errors", "filtered", "len_errors", "other_plp",
        "accepted")] + [("blocks", ctypes.c_int64 * MAX_PLP), ("by_type", ctypes.c_int64 * 256)]


class _ModeAdaptParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("kbch", "framesize", "rate", "sis_mis", "isi", "npd")] + [
        ("pid_mask", ctypes.c_void_p), ("max_ts_bytes", ctypes.c_int64)]


class _ModeAdaptPos(ctypes.Structure):
    _fields_ = [("ts_packet", ctypes.c_int64), ("unit_byte", ctypes.c_int), ("dnp", ctypes.c_int)]


class _ModeAdaptResult(ctypes.Structure):
    _fields_ = [("resume", _ModeAdaptPos)] + [(n, ctypes.c_int64) for n in (
        "packets_in", "selected", "nulls_deleted", "nulls_kept", "nulls_dropped_at_flush", "sync_errors", "bbframes",
        "flushed")]


class _UleParams(ctypes.Structure):
    _fields_ = [("pid", ctypes.c_int), ("d_bit", ctypes.c_int), ("dest", ctypes.c_uint8 * 6),
                ("packing", ctypes.c_int), ("max_pdu_bytes", ctypes.c_int64), ("max_pdus", ctypes.c_int)]


class _UlePos(ctypes.Structure):
    _fields_ = [("pdu", ctypes.c_int64), ("sndu_byte", ctypes.c_int), ("cc", ctypes.c_int)]


class _UleResult(ctypes.Structure):
    _fields_ = [("resume", _UlePos)] + [(n, ctypes.c_int64) for n in (
        "pdus_in", "sndus", "skipped_len", "skipped_type", "ts_packets", "pusi_packets", "pad_bytes", "flushed")]


class _MpeParams(ctypes.Structure):
    _fields_ = [("pid", ctypes.c_int), ("mac", ctypes.c_uint8 * 6), ("mac_mode", ctypes.c_int),
                ("packing", ctypes.c_int), ("max_pdu_bytes", ctypes.c_int64), ("max_pdus", ctypes.c_int)]


class _MpePos(ctypes.Structure):
    _fields_ = [("pdu", ctypes.c_int64), ("section_byte", ctypes.c_int), ("cc", ctypes.c_int)]


class _MpeResult(ctypes.Structure):
    _fields_ = [("resume", _MpePos)] + [(n, ctypes.c_int64) for n in (
        "pdus_in", "sections", "skipped_len", "skipped_type", "mapped_macs", "ts_packets", "pusi_packets", "pad_bytes",
        "flushed")]


class _MpeFecParams(ctypes.Structure):
    _fields_ = [("pid", ctypes.c_int), ("mac", ctypes.c_uint8 * 6), ("mac_mode", ctypes.c_int),
                ("packing", ctypes.c_int), ("max_pdu_bytes", ctypes.c_int64), ("max_pdus", ctypes.c_int),
                ("rows", ctypes.c_int), ("data_columns", ctypes.c_int), ("rs_columns", ctypes.c_int),
                ("max_frames", ctypes.c_int)]


class _MpeFecPos(ctypes.Structure):
    _fields_ = [("pdu", ctypes.c_int64), ("section", ctypes.c_int), ("section_byte", ctypes.c_int),
                ("cc", ctypes.c_int), ("frame", ctypes.c_int)]


class _MpeFecResult(ctypes.Structure):
    _fields_ = [("resume", _MpeFecPos)] + [(n, ctypes.c_int64) for n in (
        "pdus_in", "sections", "fec_sections", "frames", "skipped_len", "skipped_type", "mapped_macs", "ts_packets",
        "pusi_packets", "pad_bytes", "flushed")]


TSMUX_INPUTS = 8      # DVBT2LL_TSMUX_INPUTS
PSI_PROGRAMS, PSI_STREAMS, PSI_DESCRIPTOR_BYTES, PSI_ROUNDS = 8, 8, 64, 16   # DVBT2LL_PSI_*


class _TsMuxParams(ctypes.Structure):
    _fields_ = [("n_inputs", ctypes.c_int), ("period", ctypes.c_int), ("weight", ctypes.c_int * TSMUX_INPUTS),
                ("loop", ctypes.c_int * TSMUX_INPUTS), ("fill_input", ctypes.c_int), ("pcr_pid", ctypes.c_int),
                ("pcr_weight", ctypes.c_int), ("ticks_per_period", ctypes.c_int64), ("max_out_packets", ctypes.c_int)]


class _TsMuxPos(ctypes.Structure):
    _fields_ = [("phase", ctypes.c_int), ("pcr_ticks", ctypes.c_int64), ("next", ctypes.c_int64 * TSMUX_INPUTS)]


class _TsMuxResult(ctypes.Structure):
    _fields_ = [("resume", _TsMuxPos), ("consumed", ctypes.c_int64 * TSMUX_INPUTS),
                ("dry_slots", ctypes.c_int64 * TSMUX_INPUTS)] + [(n, ctypes.c_int64) for n in (
                    "fill_in_free", "pcr_packets", "null_packets", "sync_errors")]


TSMUX_MAP, TSMUX_TRACK = 64, 64      # DVBT2LL_TSMUX_MAP, DVBT2LL_TSMUX_TRACK


class _TsMuxMap(ctypes.Structure):
    _fields_ = [("input", ctypes.c_int), ("from_pid", ctypes.c_int), ("to_pid", ctypes.c_int)]


class _TsMuxRemux(ctypes.Structure):
    _fields_ = [("n_map", ctypes.c_int), ("map", _TsMuxMap * TSMUX_MAP), ("n_track", ctypes.c_int),
                ("track_pid", ctypes.c_int * TSMUX_TRACK), ("restamp_cc", ctypes.c_int * TSMUX_INPUTS),
                ("in_period", ctypes.c_int * TSMUX_INPUTS), ("in_ticks_per_period", ctypes.c_int64 * TSMUX_INPUTS),
                ("out_ticks_per_period", ctypes.c_int64)]


class _TsMuxRemuxPos(ctypes.Structure):
    _fields_ = [("cc", ctypes.c_int * TSMUX_TRACK), ("in_phase", ctypes.c_int * TSMUX_INPUTS),
                ("in_ticks", ctypes.c_int64 * TSMUX_INPUTS)]


class _TsMuxRemuxResult(ctypes.Structure):
    _fields_ = [("resume", _TsMuxRemuxPos)] + [(n, ctypes.c_int64) for n in (
        "remapped", "dropped", "cc_rewritten", "pcr_restamped")]


class _PsiStream(ctypes.Structure):
    _fields_ = [("stream_type", ctypes.c_int), ("pid", ctypes.c_int), ("descriptor_len", ctypes.c_int),
                ("descriptors", ctypes.c_uint8 * PSI_DESCRIPTOR_BYTES)]


class _PsiProgram(ctypes.Structure):
    _fields_ = [("program_number", ctypes.c_int), ("pmt_pid", ctypes.c_int), ("pcr_pid", ctypes.c_int),
                ("n_streams", ctypes.c_int), ("streams", _PsiStream * PSI_STREAMS)]


class _PsiParams(ctypes.Structure):
    _fields_ = [("transport_stream_id", ctypes.c_int), ("version", ctypes.c_int), ("n_programs", ctypes.c_int),
                ("programs", _PsiProgram * PSI_PROGRAMS)]


class _GseParams(ctypes.Structure):
    _fields_ = [("kbch", ctypes.c_int), ("framesize", ctypes.c_int), ("rate", ctypes.c_int),
                ("sis_mis", ctypes.c_int), ("isi", ctypes.c_int), ("label_len", ctypes.c_int),
                ("label", ctypes.c_uint8 * 6), ("max_pdu_bytes", ctypes.c_int64), ("max_pdus", ctypes.c_int)]


class _GsePos(ctypes.Structure):
    _fields_ = [("pdu", ctypes.c_int64), ("pdu_byte", ctypes.c_int), ("frag_id", ctypes.c_int)]


class _GseResult(ctypes.Structure):
    _fields_ = [("resume", _GsePos)] + [(n, ctypes.c_int64) for n in (
        "pdus_in", "complete", "fragmented", "gse_packets", "skipped_len", "skipped_type", "bbframes", "pad_bytes",
        "flushed")]


T2MI_OUT_MAX_AUX = 4   # DVBT2LL_T2MI_OUT_MAX_AUX


class _T2miOutSlot(ctypes.Structure):
    _fields_ = [("packet_type", ctypes.c_int), ("payload_bits", ctypes.c_int), ("after", ctypes.c_int)]


class _T2miOutParams(ctypes.Structure):
    _fields_ = [("pid", ctypes.c_int), ("t2mi_stream_id", ctypes.c_int), ("nplp", ctypes.c_int),
                ("plp_id", ctypes.c_int * MAX_PLP), ("bbframe_bytes", ctypes.c_int * MAX_PLP),
                ("blocks_per_frame", ctypes.c_int * MAX_PLP), ("frames_per_superframe", ctypes.c_int),
                ("naux", ctypes.c_int), ("aux", _T2miOutSlot * T2MI_OUT_MAX_AUX), ("max_frames", ctypes.c_int)]


class _T2miOutPos(ctypes.Structure):
    _fields_ = [("frame", ctypes.c_int64), ("packet_count", ctypes.c_int), ("cc", ctypes.c_int)]


class _T2miOutResult(ctypes.Structure):
    _fields_ = [("next", _T2miOutPos)] + [(n, ctypes.c_int64) for n in (
        "frames", "t2mi_packets", "ts_packets", "pusi_packets", "stuffing_bytes")] + [
        ("by_type", ctypes.c_int64 * 256)]


BLOCKS = ("bbheaderbch", "ldpc", "interleavermod", "framemapperfint", "pilotgenp1insert")
PARAMS = {"bbheaderbch": _BbParams, "ldpc": _LdpcParams, "interleavermod": _ImParams,
          "framemapperfint": _FmParams, "pilotgenp1insert": _PgParams}
PDU_BLOCKS = {"ule": (_UleParams, _UlePos, _UleResult, True), "mpe": (_MpeParams, _MpePos, _MpeResult, False),
              "mpefec": (_MpeFecParams, _MpeFecPos, _MpeFecResult, False),
              "gse": (_GseParams, _GsePos, _GseResult, True)}

# every symbol include/dvbt2ll_hip.h declares (checked by the CPU test suite)
EXPORTS = ["dvbt2ll_strerror", "dvbt2ll_version", "dvbt2ll_device_count", "dvbt2ll_abi_version", "dvbt2ll_abi_check"]
for _b in BLOCKS:
    EXPORTS += ["dvbt2ll_%s_%s" % (_b, f) for f in
                ("create", "output_multiple", "forecast", "general_work", "destroy")]
EXPORTS += ["dvbt2ll_framemapperfint_stream_items", "dvbt2ll_pilotgenp1insert_active_items",
            "dvbt2ll_pilotgenp1insert_debug_carriers", "dvbt2ll_bbheaderbch_sync_errors"]
EXPORTS += ["dvbt2ll_bbheaderbch_set_isi"]
EXPORTS += ["dvbt2ll_framemapper_mplp_" + f for f in ("create", "output_multiple", "stream_items", "forecast",
                                                      "general_work", "destroy")]
EXPORTS += ["dvbt2ll_gse_" + f for f in ("create", "params_from_chain", "run_device", "get_result", "run_host",
                                         "destroy")]
EXPORTS += ["dvbt2ll_t2mi_out_" + f for f in ("create", "params_from_chain", "ts_packets", "run_device", "get_result",
                                              "run_host", "destroy")]
EXPORTS += ["dvbt2ll_chain_" + f for f in ("host_submit", "host_wait", "run_host_pipelined", "run_plps_host")]
EXPORTS += ["dvbt2ll_host_alloc", "dvbt2ll_host_free"]
EXPORTS += ["dvbt2ll_chain_" + f for f in ("create_mplp", "num_plps", "unit_frames", "get_plp_info", "run_plps",
                                           "debug_plp_codewords", "debug_keep_codewords")]
EXPORTS += ["dvbt2ll_chain_" + f for f in ("create_miso_pair", "create_mplp_miso_pair", "num_groups", "run_groups",
                                           "run_plps_groups")]
EXPORTS += ["dvbt2ll_chain_" + f for f in ("set_input", "get_input", "bbheader_errors")]
EXPORTS += ["dvbt2ll_t2mi_" + f for f in ("create", "params_from_chain", "run_device", "get_result", "get_packets",
                                          "run_host", "destroy")]
EXPORTS += ["dvbt2ll_modeadapt_" + f for f in ("create", "params_from_chain", "run_device", "get_result", "run_host",
                                               "destroy")]
EXPORTS += ["dvbt2ll_ule_" + f for f in ("create", "run_device", "get_result", "run_host", "destroy")]
EXPORTS += ["dvbt2ll_mpe_" + f for f in ("create", "run_device", "get_result", "run_host", "destroy")]
EXPORTS += ["dvbt2ll_mpefec_" + f for f in ("create", "run_device", "get_result", "run_host", "destroy")]
EXPORTS += ["dvbt2ll_tsmux_" + f for f in ("schedule", "ticks_per_period", "create", "run_device", "get_result",
                                           "run_host", "destroy", "remux_check", "set_remux", "run_device_remux",
                                           "get_remux_result", "run_host_remux")]
EXPORTS += ["dvbt2ll_psi_build"]
EXPORTS += ["dvbt2ll_chain_" + f for f in ("create", "get_info", "run_device", "run_streams", "run_host", "set_output", "set_slots", "set_graph", "set_timing",
                                           "get_timing", "debug_codewords", "debug_cell_pairs", "debug_cells",
                                           "synchronize", "sync_errors",
                                           "destroy")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise DVBT2Error("%s is missing: run __graft_entry__.build() (no CPU fallback exists)" % LIB_PATH)
    L = ctypes.CDLL(str(LIB_PATH))
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.dvbt2ll_strerror.restype = ctypes.c_char_p
    L.dvbt2ll_strerror.argtypes = [ci]
    L.dvbt2ll_version.restype = ctypes.c_char_p
    L.dvbt2ll_device_count.restype = ci
    L.dvbt2ll_abi_version.restype = ci
    L.dvbt2ll_abi_check.argtypes = [ci] + [ctypes.c_size_t] * 5
    # this mirror's struct layouts must be the library's (include/dvbt2ll_hip.h DVBT2LL_ABI_VERSION)
    if L.dvbt2ll_abi_check(ABI_VERSION, ctypes.sizeof(_ChainParams), ctypes.sizeof(_ChainInfo),
                           ctypes.sizeof(_PlpParams), ctypes.sizeof(_MplpParams), ctypes.sizeof(_MplpChainParams)):
        raise DVBT2Error("%s: ABI version %d with other struct layouts than this mirror's (ABI %d)"
                         % (LIB_PATH, L.dvbt2ll_abi_version(), ABI_VERSION))
    for b in BLOCKS:
        getattr(L, "dvbt2ll_%s_create" % b).argtypes = [ctypes.POINTER(PARAMS[b]), ci, ctypes.POINTER(vp)]
        getattr(L, "dvbt2ll_%s_output_multiple" % b).argtypes = [vp]
        getattr(L, "dvbt2ll_%s_forecast" % b).argtypes = [vp, ci, ctypes.POINTER(ci)]
        getattr(L, "dvbt2ll_%s_general_work" % b).argtypes = [vp, ci, ci, vp, vp, ctypes.POINTER(ci)]
        getattr(L, "dvbt2ll_%s_destroy" % b).argtypes = [vp]
        getattr(L, "dvbt2ll_%s_destroy" % b).restype = None
    L.dvbt2ll_framemapperfint_stream_items.argtypes = [vp]
    L.dvbt2ll_pilotgenp1insert_active_items.argtypes = [vp]
    L.dvbt2ll_pilotgenp1insert_debug_carriers.argtypes = [vp, vp, vp]
    L.dvbt2ll_chain_create.argtypes = [ctypes.POINTER(_ChainParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_chain_get_info.argtypes = [vp, ctypes.POINTER(_ChainInfo)]
    L.dvbt2ll_chain_run_device.argtypes = [vp, vp, i64, i64, i64, ci, vp, vp]
    L.dvbt2ll_chain_run_streams.argtypes = [vp, vp, i64, ci, i64, i64, i64, ci, vp, vp]
    L.dvbt2ll_chain_run_host.argtypes = [vp, vp, i64, i64, i64, ci, vp]
    L.dvbt2ll_chain_set_output.argtypes = [vp, ctypes.c_float, ci]
    L.dvbt2ll_chain_host_submit.argtypes = [vp, vp, i64, i64, i64, ci, vp, ctypes.POINTER(i64)]
    L.dvbt2ll_chain_host_wait.argtypes = [vp, i64]
    L.dvbt2ll_chain_run_plps_host.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64), i64,
                                              ci, vp]
    L.dvbt2ll_chain_run_host_pipelined.argtypes = [vp, vp, i64, i64, i64, ci, vp, ci]
    L.dvbt2ll_host_alloc.restype = vp
    L.dvbt2ll_host_alloc.argtypes = [ctypes.c_size_t]
    L.dvbt2ll_host_free.argtypes = [vp]
    L.dvbt2ll_host_free.restype = None
    L.dvbt2ll_chain_set_slots.argtypes = [vp, ci]
    L.dvbt2ll_chain_set_graph.argtypes = [vp, ci]
    L.dvbt2ll_chain_set_timing.argtypes = [vp, ci]
    L.dvbt2ll_chain_get_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64), ci]
    L.dvbt2ll_chain_debug_codewords.argtypes = [vp, vp, i64]
    L.dvbt2ll_chain_debug_keep_codewords.argtypes = [vp, ci]
    L.dvbt2ll_chain_debug_cell_pairs.argtypes = [vp, vp, i64]
    L.dvbt2ll_chain_debug_cells.argtypes = [vp, vp, i64]
    L.dvbt2ll_chain_synchronize.argtypes = [vp]
    L.dvbt2ll_chain_sync_errors.argtypes = [vp, ctypes.POINTER(i64)]
    L.dvbt2ll_bbheaderbch_sync_errors.argtypes = [vp]
    L.dvbt2ll_bbheaderbch_sync_errors.restype = i64
    L.dvbt2ll_bbheaderbch_set_isi.argtypes = [vp, ci]
    L.dvbt2ll_framemapper_mplp_create.argtypes = [ctypes.POINTER(_MplpParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_framemapper_mplp_output_multiple.argtypes = [vp]
    L.dvbt2ll_framemapper_mplp_stream_items.argtypes = [vp, ci]
    L.dvbt2ll_framemapper_mplp_forecast.argtypes = [vp, ci, ctypes.POINTER(ci)]
    L.dvbt2ll_framemapper_mplp_general_work.argtypes = [vp, ci, ctypes.POINTER(ci), ctypes.POINTER(vp), vp,
                                                        ctypes.POINTER(ci)]
    L.dvbt2ll_framemapper_mplp_destroy.argtypes = [vp]
    L.dvbt2ll_framemapper_mplp_destroy.restype = None
    L.dvbt2ll_chain_create_mplp.argtypes = [ctypes.POINTER(_MplpChainParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_chain_num_plps.argtypes = [vp]
    L.dvbt2ll_chain_unit_frames.argtypes = [vp]
    L.dvbt2ll_chain_get_plp_info.argtypes = [vp, ci, ctypes.POINTER(_ChainInfo)]
    L.dvbt2ll_chain_run_plps.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64), i64, ci,
                                         vp, vp]
    L.dvbt2ll_chain_debug_plp_codewords.argtypes = [vp, ci, vp, i64]
    L.dvbt2ll_chain_create_miso_pair.argtypes = [ctypes.POINTER(_ChainParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_chain_create_mplp_miso_pair.argtypes = [ctypes.POINTER(_MplpChainParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_chain_num_groups.argtypes = [vp]
    L.dvbt2ll_chain_run_groups.argtypes = [vp, vp, i64, ci, i64, i64, i64, ci, ctypes.POINTER(vp), vp]
    L.dvbt2ll_chain_run_plps_groups.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64), i64,
                                                ci, ctypes.POINTER(vp), vp]
    L.dvbt2ll_chain_set_input.argtypes = [vp, ci, ci]
    L.dvbt2ll_chain_get_input.argtypes = [vp, ci]
    L.dvbt2ll_chain_bbheader_errors.argtypes = [vp, ctypes.POINTER(i64)]
    L.dvbt2ll_t2mi_create.argtypes = [ctypes.POINTER(_T2miParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_t2mi_params_from_chain.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(_T2miParams)]
    L.dvbt2ll_t2mi_run_device.argtypes = [vp, vp, i64, ctypes.POINTER(_T2miPos), ctypes.POINTER(vp),
                                          ctypes.POINTER(i64), vp]
    L.dvbt2ll_t2mi_get_result.argtypes = [vp, ctypes.POINTER(_T2miResult)]
    L.dvbt2ll_t2mi_get_packets.argtypes = [vp, vp, i64]
    L.dvbt2ll_t2mi_get_packets.restype = i64
    L.dvbt2ll_t2mi_run_host.argtypes = [vp, vp, i64, ctypes.POINTER(_T2miPos), ctypes.POINTER(vp),
                                        ctypes.POINTER(i64), ctypes.POINTER(_T2miResult)]
    L.dvbt2ll_t2mi_destroy.argtypes = [vp]
    L.dvbt2ll_t2mi_destroy.restype = None
    L.dvbt2ll_modeadapt_create.argtypes = [ctypes.POINTER(_ModeAdaptParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_modeadapt_params_from_chain.argtypes = [vp, ci, ctypes.POINTER(_ModeAdaptParams)]
    L.dvbt2ll_modeadapt_run_device.argtypes = [vp, vp, i64, ctypes.POINTER(_ModeAdaptPos), vp, i64, ci, vp]
    L.dvbt2ll_modeadapt_get_result.argtypes = [vp, ctypes.POINTER(_ModeAdaptResult)]
    L.dvbt2ll_modeadapt_run_host.argtypes = [vp, vp, i64, ctypes.POINTER(_ModeAdaptPos), vp, i64, ci,
                                             ctypes.POINTER(_ModeAdaptResult)]
    L.dvbt2ll_modeadapt_destroy.argtypes = [vp]
    L.dvbt2ll_modeadapt_destroy.restype = None
    # the four PDU-batch encapsulators: (params, pos, result, whether the run calls take a type array)
    for b, (par, pos, res, types) in PDU_BLOCKS.items():
        head = [vp, vp, i64, vp] + ([vp] if types else []) + [i64, ctypes.POINTER(pos), vp, i64, ci]
        getattr(L, "dvbt2ll_%s_create" % b).argtypes = [ctypes.POINTER(par), ci, ctypes.POINTER(vp)]
        getattr(L, "dvbt2ll_%s_run_device" % b).argtypes = head + [vp]
        getattr(L, "dvbt2ll_%s_get_result" % b).argtypes = [vp, ctypes.POINTER(res)]
        getattr(L, "dvbt2ll_%s_run_host" % b).argtypes = head + [ctypes.POINTER(res)]
        getattr(L, "dvbt2ll_%s_destroy" % b).argtypes = [vp]
        getattr(L, "dvbt2ll_%s_destroy" % b).restype = None
    L.dvbt2ll_tsmux_schedule.argtypes = [ctypes.POINTER(_TsMuxParams), vp]
    L.dvbt2ll_tsmux_ticks_per_period.argtypes = [ci, i64]
    L.dvbt2ll_tsmux_ticks_per_period.restype = i64
    L.dvbt2ll_tsmux_create.argtypes = [ctypes.POINTER(_TsMuxParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_tsmux_run_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(_TsMuxPos), vp,
                                           i64, vp]
    L.dvbt2ll_tsmux_get_result.argtypes = [vp, ctypes.POINTER(_TsMuxResult)]
    L.dvbt2ll_tsmux_run_host.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(_TsMuxPos), vp,
                                         i64, ctypes.POINTER(_TsMuxResult)]
    L.dvbt2ll_tsmux_destroy.argtypes = [vp]
    L.dvbt2ll_tsmux_remux_check.argtypes = [ctypes.POINTER(_TsMuxParams), ctypes.POINTER(_TsMuxRemux)]
    L.dvbt2ll_tsmux_set_remux.argtypes = [vp, ctypes.POINTER(_TsMuxRemux)]
    L.dvbt2ll_tsmux_run_device_remux.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(_TsMuxPos),
                                                 ctypes.POINTER(_TsMuxRemuxPos), vp, i64, vp]
    L.dvbt2ll_tsmux_get_remux_result.argtypes = [vp, ctypes.POINTER(_TsMuxRemuxResult)]
    L.dvbt2ll_tsmux_run_host_remux.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(_TsMuxPos),
                                               ctypes.POINTER(_TsMuxRemuxPos), vp, i64, ctypes.POINTER(_TsMuxResult),
                                               ctypes.POINTER(_TsMuxRemuxResult)]
    L.dvbt2ll_tsmux_destroy.restype = None
    L.dvbt2ll_psi_build.argtypes = [ctypes.POINTER(_PsiParams), vp, i64]
    L.dvbt2ll_psi_build.restype = i64
    L.dvbt2ll_gse_params_from_chain.argtypes = [vp, ci, ctypes.POINTER(_GseParams)]
    L.dvbt2ll_t2mi_out_create.argtypes = [ctypes.POINTER(_T2miOutParams), ci, ctypes.POINTER(vp)]
    L.dvbt2ll_t2mi_out_params_from_chain.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(_T2miOutParams)]
    L.dvbt2ll_t2mi_out_ts_packets.argtypes = [vp, ci]
    L.dvbt2ll_t2mi_out_ts_packets.restype = i64
    L.dvbt2ll_t2mi_out_run_device.argtypes = [vp, ctypes.POINTER(vp), vp, i64, ctypes.POINTER(i64),
                                              ctypes.POINTER(_T2miOutPos), ci, vp, i64, vp]
    L.dvbt2ll_t2mi_out_get_result.argtypes = [vp, ctypes.POINTER(_T2miOutResult)]
    L.dvbt2ll_t2mi_out_run_host.argtypes = [vp, ctypes.POINTER(vp), vp, i64, ctypes.POINTER(i64),
                                            ctypes.POINTER(_T2miOutPos), ci, vp, i64, ctypes.POINTER(_T2miOutResult)]
    L.dvbt2ll_t2mi_out_destroy.argtypes = [vp]
    L.dvbt2ll_t2mi_out_destroy.restype = None
    L.dvbt2ll_chain_destroy.argtypes = [vp]
    L.dvbt2ll_chain_destroy.restype = None
    _lib = L
    return L


def check(status, what):
    if status < 0:
        msg = lib().dvbt2ll_strerror(status).decode()
        if status == -2:
            raise MemoryError("%s: %s" % (what, msg))     # reference: std::bad_alloc
        raise DVBT2Error("%s failed (%d): %s" % (what, status, msg))
    return status
