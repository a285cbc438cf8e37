"""ctypes binding of libcrnsense's C ABI (include/crn_sense.h).

Plumbing for tests/, bench.py and __graft_entry__.py only: the product is the C-ABI shared
library and the C++ engine in cognitive_engines/CE_Predictive_Node_GPU/; nothing here computes.  There is no CPU fallback: loading
fails loudly when libcrnsense.so has not been built, and crn_sense_create fails when no GPU is
visible.
"""
import ctypes as C
import os
import weakref

HERE = os.path.dirname(os.path.abspath(__file__))
# env overrides: CRN_SENSE_LIB = another build of the library (libcrnsense_sc16.so: the optional wire-format kernels, make SC16=1;
# libcrnsense_plain.so: no assembly filter, a test artefact); CRN_SENSE_AB=1 = libcrnsense_ab.so, the build that also carries the
# measurement variants (tools/, the A/B test) — the engine and bench.py's default run use the shipped library
LIB_PATH = os.environ.get("CRN_SENSE_LIB") or os.path.join(HERE, "libcrnsense_ab.so" if os.environ.get("CRN_SENSE_AB") == "1" else "libcrnsense.so")
SC16_LIB_PATH = os.path.join(HERE, "libcrnsense_sc16.so")
PLAIN_LIB_PATH = os.path.join(HERE, "libcrnsense_plain.so")
LIQUID_SHIM_PATH = os.path.join(HERE, "libcrnliquidfft.so")  # include/crn_liquid_fft.h

CRN_ABI_VERSION = 4
CRN_ERR_ARG = -1
CRN_ERR_BUSY = -5
CRN_MAX_BANDS = 80
CRN_MAX_SEGS = 160

MODE_REF_MAG, MODE_ENERGY = 0, 1
DECIDE_ANN, DECIDE_THRESHOLD, DECIDE_NONE = 0, 1, 2
WINDOW_RECT, WINDOW_HANN, WINDOW_BLACKMAN_HARRIS = 0, 1, 2

# the optional wire-format entry points (include/crn_sense_sc16.h): only in a library built with make SC16=1
SC16_EXPORTS = ["crn_sense_run_device_sc16", "crn_pack_sc16_device", "crn_sense_set_wire_full_scale", "crn_ingest_create_sc16", "crn_ingest_push_sc16"]

# every symbol include/crn_sense.h declares unconditionally (tests check the library exports them all)
EXPORTS = [
    "crn_cfg_reference", "crn_cfg_energy_scaled", "crn_cfg_welch", "crn_cfg_reference_scaled", "crn_cfg_welch_scaled",
    "crn_cfg_save_ann", "crn_cfg_load_ann", "crn_sense_set_ann", "crn_sense_set_bands", "crn_noise_floor_host", "crn_sense_synchronize",
    "crn_sense_create", "crn_sense_destroy", "crn_sense_run_device", "crn_sense_run_host",
    "crn_synth_fill_device", "crn_synth_fill_device_ex", "crn_ann_train_device", "crn_fft_forward_device",
    "crn_sense_kernel_info", "crn_sense_set_variant", "crn_sense_dealt_launches",
    "crn_ingest_create", "crn_ingest_push", "crn_ingest_flush", "crn_ingest_poll", "crn_ingest_drain",
    "crn_ingest_destroy", "crn_ingest_set_packet_len", "crn_ingest_wait", "crn_ingest_dropped", "crn_ingest_packets_per_epoch",
    "crn_noise_floor_device", "crn_sense_set_thresholds", "crn_sense_reserve_noise_floor", "crn_sense_calibrate_thresholds",
    "crn_ingest_calibrate", "crn_ingest_noise_floor",
    "crn_sense_reserve_host", "crn_sense_set_timing", "crn_sense_get_stats", "crn_ingest_get_stats",
    "crn_monitor_rows_device",
    "crn_sense_set_cfar", "crn_sense_get_cfar", "crn_sense_run_device_cfar", "crn_cfar_alpha",
    "crn_sense_set_cfar_ex", "crn_sense_get_cfar_ex", "crn_cfar_alpha_ex",
    "crn_segments_device", "crn_tracks_workspace_bytes", "crn_tracks_device",
    "crn_tracks_carry_bytes", "crn_tracks_carry_workspace_bytes", "crn_tracks_carry_device",
    "crn_channels_workspace_bytes", "crn_channels_device", "crn_channel_forecast",
    "crn_fuse_device", "crn_fuse_member_pfa",
    "crn_holes_workspace_bytes", "crn_holes_device",
    "crn_lad_device", "crn_lad_factor",
    "crn_tcfar_hist_bytes", "crn_tcfar_device",
    "crn_measure_device",
    "crn_occmap_workspace_bytes", "crn_occmap_device",
    "crn_cyclo_device", "crn_cyclo_zmin",
    "crn_hops_bytes", "crn_hops_workspace_bytes", "crn_hops_device", "crn_hop_forecast",
    "crn_extract_device",
    "crn_resample_state_bytes", "crn_resample_device",
    "crn_comm_unique_id", "crn_comm_create", "crn_comm_local", "crn_comm_allgather", "crn_comm_gathered",
    "crn_comm_finish", "crn_comm_destroy", "crn_comm_local_addr", "crn_comm_wait", "crn_comm_info",
    "crn_last_error", "crn_abi_version", "crn_build_info",
]


class BandSeg(C.Structure):
    _fields_ = [("lo", C.c_int32), ("hi", C.c_int32), ("band", C.c_int32)]


class Cfg(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("fft_len", C.c_int32), ("frames_per_epoch", C.c_int32),
        ("hop", C.c_int32), ("mode", C.c_int32), ("decide", C.c_int32), ("window", C.c_int32),
        ("n_bands", C.c_int32), ("n_segs", C.c_int32), ("ref_band", C.c_int32),
        ("device", C.c_int32), ("reserved0", C.c_int32),
        ("segs", BandSeg * CRN_MAX_SEGS),
        ("thresh", C.c_float * CRN_MAX_BANDS),
        ("ann_w_ih", (C.c_double * 6) * 5),
        ("ann_w_ho", (C.c_double * 4) * 6),
        ("ann_threshold", C.c_double),
        ("tx_freq_for_decision", C.c_double * 4),
    ]


class Out(C.Structure):
    _fields_ = [("features", C.c_void_p), ("ann_out", C.c_void_p), ("decision", C.c_void_p),
                ("occupancy", C.c_void_p), ("spectrum", C.c_void_p)]


class CfarParams(C.Structure):
    """crn_cfar_params: per-bin CA-CFAR (crn_sense_set_cfar)."""
    _fields_ = [("guard", C.c_int32), ("train", C.c_int32), ("min_bins", C.c_int32), ("reserved", C.c_int32), ("alpha", C.c_float)]


class CfarParamsEx(C.Structure):
    """crn_cfar_params_ex: per-bin CFAR of any method (crn_sense_set_cfar_ex)."""
    _fields_ = [("method", C.c_int32), ("guard", C.c_int32), ("train", C.c_int32), ("min_bins", C.c_int32), ("rank", C.c_int32),
                ("reserved", C.c_int32), ("alpha", C.c_float)]


CFAR_CA, CFAR_GO, CFAR_SO, CFAR_OS = 0, 1, 2, 3    # crn_cfar_method


class SegmentParams(C.Structure):
    """crn_segment_params (crn_segments_device)."""
    _fields_ = [("merge_gap", C.c_int32), ("min_width", C.c_int32), ("max_segments", C.c_int32), ("reserved", C.c_int32)]


class Segment(C.Structure):
    """crn_segment: one stored segment, 32 bytes."""
    _fields_ = [("lo", C.c_int32), ("width", C.c_int32), ("peak_bin", C.c_int32), ("n_detected", C.c_int32),
                ("power", C.c_float), ("peak_power", C.c_float), ("centroid", C.c_float), ("reserved", C.c_float)]


class SegmentEpoch(C.Structure):
    """crn_segment_epoch: one epoch's header, 16 bytes."""
    _fields_ = [("n_found", C.c_int32), ("n_stored", C.c_int32), ("noise_bins", C.c_int32), ("noise_mean", C.c_float)]


# numpy views of the two arrays crn_segments_device writes: np.frombuffer(bytes, SEGMENT_EPOCH_DTYPE), (.., SEGMENT_DTYPE).reshape(E, max_segments)
SEGMENT_DTYPE = [("lo", "<i4"), ("width", "<i4"), ("peak_bin", "<i4"), ("n_detected", "<i4"),
                 ("power", "<f4"), ("peak_power", "<f4"), ("centroid", "<f4"), ("reserved", "<f4")]
SEGMENT_EPOCH_DTYPE = [("n_found", "<i4"), ("n_stored", "<i4"), ("noise_bins", "<i4"), ("noise_mean", "<f4")]


class TrackParams(C.Structure):
    """crn_track_params (crn_tracks_device), 32 bytes."""
    _fields_ = [("max_segments", C.c_int32), ("epochs_per_stream", C.c_int32), ("slack_bins", C.c_int32), ("max_miss", C.c_int32),
                ("min_epochs", C.c_int32), ("max_tracks", C.c_int32), ("reserved", C.c_int32 * 2)]


# numpy views of the two arrays crn_tracks_device writes: (.., TRACK_STREAM_DTYPE) [n_streams], (.., TRACK_DTYPE).reshape(n_streams, max_tracks)
TRACK_DTYPE = [("first_t", "<i4"), ("last_t", "<i4"), ("first_slot", "<i4"), ("last_slot", "<i4"), ("n_epochs_hit", "<i4"), ("n_segments", "<i4"),
               ("lo_off", "<i4"), ("hi_off", "<i4"), ("width_sum", "<i8"), ("power_sum", "<f4"), ("peak_power", "<f4"), ("centre", "<f4"),
               ("flags", "<i4"), ("reserved", "<i4", (2,))]
TRACK_STREAM_DTYPE = [("n_found", "<i4"), ("n_stored", "<i4"), ("n_nodes", "<i4"), ("reserved", "<i4")]
TRACK_BEGAN_BEFORE, TRACK_GOES_ON = 1, 2      # crn_track.flags
TRACK_HITS_UPPER_BOUND = 4                    # crn_track.flags from crn_tracks_carry_device: two carried tracks merged, n_epochs_hit is an upper bound
# the per-stream header crn_tracks_carry_device writes: (.., TRACK_CARRY_STREAM_DTYPE) [n_streams]
TRACK_CARRY_STREAM_DTYPE = [("n_found", "<i4"), ("n_stored", "<i4"), ("n_nodes", "<i4"), ("n_open", "<i4"), ("n_open_found", "<i4"),
                            ("n_open_stored", "<i4"), ("status", "<i4"), ("reserved", "<i4")]
CRN_MAX_CHANNELS = 64


class ChannelSpan(C.Structure):
    """crn_channel_span: bins (lo + i) mod fft_len, 0 <= i < width."""
    _fields_ = [("lo", C.c_int32), ("width", C.c_int32)]


class ChannelParams(C.Structure):
    """crn_channel_params (crn_channels_device), 544 bytes."""
    _fields_ = [("n_channels", C.c_int32), ("epochs_per_stream", C.c_int32), ("min_bins", C.c_int32), ("first", C.c_int32),
                ("reserved", C.c_int32 * 4), ("span", ChannelSpan * CRN_MAX_CHANNELS)]


class ChannelStats(C.Structure):
    """crn_channel_stats: one stream's record of one channel, 192 bytes."""
    _fields_ = [("n_epochs", C.c_int64), ("n_busy", C.c_int64), ("n_trans", (C.c_int64 * 2) * 2), ("n_runs", C.c_int64 * 2),
                ("run_sum", C.c_int64 * 2), ("run_max", C.c_int64 * 2), ("run", C.c_int64), ("state", C.c_int32), ("reserved", C.c_int32),
                ("power", C.c_double * 2), ("idle_hist", C.c_int32 * 16)]


# numpy view of the records crn_channels_device keeps: np.frombuffer(bytes, CHANNEL_STATS_DTYPE).reshape(n_streams, n_channels)
CHANNEL_STATS_DTYPE = [("n_epochs", "<i8"), ("n_busy", "<i8"), ("n_trans", "<i8", (2, 2)), ("n_runs", "<i8", (2,)), ("run_sum", "<i8", (2,)),
                       ("run_max", "<i8", (2,)), ("run", "<i8"), ("state", "<i4"), ("reserved", "<i4"), ("power", "<f8", (2,)),
                       ("idle_hist", "<i4", (16,))]
CRN_MAX_FUSE_MEMBERS = 32
FUSE_VOTE, FUSE_SOFT = 0, 1                   # crn_fuse_rule


class FuseParams(C.Structure):
    """crn_fuse_params (crn_fuse_device), 168 bytes."""
    _fields_ = [("rule", C.c_int32), ("group_size", C.c_int32), ("epochs_per_stream", C.c_int32), ("votes", C.c_int32), ("guard", C.c_int32),
                ("train", C.c_int32), ("reserved", C.c_int32 * 3), ("alpha", C.c_float), ("weight", C.c_float * CRN_MAX_FUSE_MEMBERS)]


class FuseRow(C.Structure):
    """crn_fuse_row: one fused row's header, 16 bytes."""
    _fields_ = [("n_detected", C.c_int32), ("n_any", C.c_int32), ("n_all", C.c_int32), ("n_active", C.c_int32)]


# numpy view of the headers crn_fuse_device writes: np.frombuffer(bytes, FUSE_ROW_DTYPE), one per fused row
FUSE_ROW_DTYPE = [("n_detected", "<i4"), ("n_any", "<i4"), ("n_all", "<i4"), ("n_active", "<i4")]


class HoleParams(C.Structure):
    """crn_hole_params (crn_holes_device), 32 bytes."""
    _fields_ = [("epochs_per_stream", C.c_int32), ("first", C.c_int32), ("guard", C.c_int32), ("min_age", C.c_int32), ("min_width", C.c_int32),
                ("max_holes", C.c_int32), ("avg_epochs", C.c_int32), ("reserved", C.c_int32)]


class Hole(C.Structure):
    """crn_hole: one stored hole, bins (lo + i) mod fft_len, 0 <= i < width; 32 bytes."""
    _fields_ = [("lo", C.c_int32), ("width", C.c_int32), ("age", C.c_int32), ("age_max", C.c_int32), ("peak_bin", C.c_int32),
                ("reserved", C.c_int32), ("power", C.c_float), ("peak_power", C.c_float)]


class HoleStream(C.Structure):
    """crn_hole_stream: one stream's header, 32 bytes."""
    _fields_ = [("n_found", C.c_int32), ("n_stored", C.c_int32), ("free_bins", C.c_int32), ("widest_lo", C.c_int32), ("widest_width", C.c_int32),
                ("widest_age", C.c_int32), ("floor_mean", C.c_float), ("reserved", C.c_int32)]


# numpy views of what crn_holes_device writes: (.., HOLE_STREAM_DTYPE) [n_streams] and (.., HOLE_DTYPE) [n_streams][max_holes]
HOLE_DTYPE = [("lo", "<i4"), ("width", "<i4"), ("age", "<i4"), ("age_max", "<i4"), ("peak_bin", "<i4"), ("reserved", "<i4"), ("power", "<f4"),
              ("peak_power", "<f4")]
HOLE_STREAM_DTYPE = [("n_found", "<i4"), ("n_stored", "<i4"), ("free_bins", "<i4"), ("widest_lo", "<i4"), ("widest_width", "<i4"),
                     ("widest_age", "<i4"), ("floor_mean", "<f4"), ("reserved", "<i4")]


class LadParams(C.Structure):
    """crn_lad_params (crn_lad_device), 32 bytes."""
    _fields_ = [("n_blocks", C.c_int32), ("init_percent", C.c_int32), ("t_cme", C.c_float), ("t_lower", C.c_float), ("t_upper", C.c_float),
                ("reserved", C.c_int32 * 3)]


# numpy view of the headers crn_lad_device writes: np.frombuffer(bytes, LAD_ROW_DTYPE), one per epoch
LAD_ROW_DTYPE = [("n_lower", "<i4"), ("n_upper", "<i4"), ("n_detected", "<i4"), ("n_clusters", "<i4"), ("n_rejected", "<i4"), ("n_clean", "<i4"),
                 ("floor_min", "<f4"), ("floor_max", "<f4")]


class TcfarParams(C.Structure):
    """crn_tcfar_params (crn_tcfar_device), 32 bytes."""
    _fields_ = [("epochs_per_stream", C.c_int32), ("first", C.c_int32), ("cells", C.c_int32), ("guard_epochs", C.c_int32), ("rank", C.c_int32),
                ("alpha", C.c_float), ("reserved", C.c_int32 * 2)]


class TcfarRow(C.Structure):
    """crn_tcfar_row: one epoch's header, 16 bytes."""
    _fields_ = [("n_detected", C.c_int32), ("n_new", C.c_int32), ("n_cells", C.c_int32), ("reserved", C.c_int32)]


# numpy view of the headers crn_tcfar_device writes: np.frombuffer(bytes, TCFAR_ROW_DTYPE), one per epoch
TCFAR_ROW_DTYPE = [("n_detected", "<i4"), ("n_new", "<i4"), ("n_cells", "<i4"), ("reserved", "<i4")]


class MeasureParams(C.Structure):
    """crn_measure_params (crn_measure_device), 32 bytes."""
    _fields_ = [("max_segments", C.c_int32), ("tail_ppm", C.c_int32), ("xdb_ratio", C.c_float), ("subtract_noise", C.c_int32),
                ("reserved", C.c_int32 * 4)]


# numpy view of the records crn_measure_device writes: np.frombuffer(bytes, MEASURE_DTYPE).reshape(n_epochs, max_segments), slot by slot
# next to SEGMENT_DTYPE's; offsets count from the segment's own lo
MEASURE_DTYPE = [("obw_lo", "<i4"), ("obw_width", "<i4"), ("xdb_lo", "<i4"), ("xdb_width", "<i4"), ("n_above", "<i4"), ("net_power", "<f4"),
                 ("crest", "<f4"), ("reserved", "<f4")]


class OccmapParams(C.Structure):
    """crn_occmap_params (crn_occmap_device), 32 bytes."""
    _fields_ = [("epochs_per_stream", C.c_int32), ("first", C.c_int32), ("duty_ppm", C.c_int32), ("reserved", C.c_int32 * 5)]


# numpy views of what crn_occmap_device keeps and writes: (.., OCCMAP_BIN_DTYPE).reshape(n_streams, fft_len), one 64-byte record per
# stream and bin, its own carry; (.., OCCMAP_STREAM_DTYPE) [n_streams], the headers
OCCMAP_BIN_DTYPE = [("n_epochs", "<i4"), ("n_busy", "<i4"), ("n_rise", "<i4"), ("n_fall", "<i4"), ("run", "<i4"), ("state", "<i4"),
                    ("run_max", "<i4", (2,)), ("max_hold", "<f4"), ("min_hold", "<f4"), ("reserved", "<i4", (2,)), ("power", "<f8", (2,))]
OCCMAP_STREAM_DTYPE = [("busy_sum", "<i8"), ("n_epochs", "<i4"), ("usual_bins", "<i4"), ("clear_bins", "<i4"), ("busy_now", "<i4"),
                       ("reserved", "<i4", (2,))]


class CycloParams(C.Structure):
    """crn_cyclo_params (crn_cyclo_device), 36 bytes."""
    _fields_ = [("max_segments", C.c_int32), ("frames", C.c_int32), ("a_lo", C.c_int32), ("n_a", C.c_int32), ("max_width", C.c_int32),
                ("min_pairs", C.c_int32), ("reserved", C.c_int32 * 2), ("z_min", C.c_float)]


class Cyclo(C.Structure):
    """crn_cyclo: one slot's record, 32 bytes."""
    _fields_ = [("a", C.c_int32), ("q", C.c_int32), ("n_pairs", C.c_int32), ("n_over", C.c_int32), ("stat", C.c_float), ("stat_lo", C.c_float),
                ("stat_hi", C.c_float), ("z", C.c_float)]


# numpy view of the records crn_cyclo_device writes: np.frombuffer(bytes, CYCLO_DTYPE).reshape(n_epochs, max_segments), slot by slot next
# to SEGMENT_DTYPE's
CYCLO_DTYPE = [("a", "<i4"), ("q", "<i4"), ("n_pairs", "<i4"), ("n_over", "<i4"), ("stat", "<f4"), ("stat_lo", "<f4"), ("stat_hi", "<f4"),
               ("z", "<f4")]


class HopParams(C.Structure):
    """crn_hop_params (crn_hops_device), 64 bytes."""
    _fields_ = [("n_channels", C.c_int32), ("epochs_per_stream", C.c_int32), ("n_lags", C.c_int32), ("first", C.c_int32), ("lag", C.c_int32 * 8),
                ("reserved", C.c_int32 * 4)]


# numpy view of ONE record crn_hops_device keeps, for n_lags lags: np.frombuffer(bytes, hop_dtype(n_lags)); hop_record does it
CRN_HOP_IDLE = 63                             # the virtual channel "nothing busy"


def hop_dtype(n_lags):
    import numpy as np
    return np.dtype([("n_epochs", "<i8"), ("n_channels", "<i4"), ("n_lags", "<i4"), ("lag", "<i4", (8,)), ("reserved", "<i4", (4,)),
                     ("hist", "<u8", (64,)), ("hop", "<i4", (64, 64)),
                     ("lags", [("from", "<i4", (64,)), ("to", "<i4", (64,)), ("pair", "<i4", (64, 64))], (int(n_lags),))])


class ExtractParams(C.Structure):
    """crn_extract_params (crn_extract_device), 32 bytes."""
    _fields_ = [("out_len", C.c_int32), ("frames_per_stream", C.c_int32), ("t0", C.c_int32), ("reserved", C.c_int32 * 5)]


class ExtractChannel(C.Structure):
    """crn_extract_channel: one channel of crn_extract_device, 16 bytes."""
    _fields_ = [("stream", C.c_int32), ("centre", C.c_int32), ("reserved", C.c_int32 * 2)]


# numpy view of the channel records crn_extract_device reads: np.zeros(n_chan, EXTRACT_CHANNEL_DTYPE); extract_channels fills one
EXTRACT_CHANNEL_DTYPE = [("stream", "<i4"), ("centre", "<i4"), ("reserved", "<i4", (2,))]
EXTRACT_OUT_LENS = (16, 32, 64, 128, 256)


class ResampleParams(C.Structure):
    """crn_resample_params (crn_resample_device), 32 bytes."""
    _fields_ = [("in_len", C.c_int32), ("out_cap", C.c_int32), ("taps", C.c_int32), ("phases", C.c_int32), ("first", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class ResampleRow(C.Structure):
    """crn_resample_row: ratio and offset of one row of crn_resample_device, 16 bytes."""
    _fields_ = [("step", C.c_uint64), ("dphi", C.c_int32), ("reserved", C.c_int32)]


# numpy views of the row records crn_resample_device reads (resample_rows fills them) and of the states it carries, 320 bytes a row
RESAMPLE_ROW_DTYPE = [("step", "<u8"), ("dphi", "<i4"), ("reserved", "<i4")]
RESAMPLE_STATE_DTYPE = [("pos", "<u8"), ("phase", "<u4"), ("taps", "<i4"), ("n_in", "<i8"), ("n_out", "<i8"), ("n_dropped", "<i8"),
                        ("last_n_out", "<i4"), ("reserved", "<i4", (5,)), ("hist", "<c8", (32,))]
RESAMPLE_TAPS = (8, 16, 32)
RESAMPLE_PHASES = (32, 64, 128, 256)


CFAR_METHODS = {"ca": CFAR_CA, "go": CFAR_GO, "so": CFAR_SO, "os": CFAR_OS}


class EpochResult(C.Structure):
    _fields_ = [("stream", C.c_int32), ("decision", C.c_int32), ("epoch_seq", C.c_int64),
                ("ann_out", C.c_double * 3), ("features", C.c_float * CRN_MAX_BANDS),
                ("occupancy", C.c_uint8 * CRN_MAX_BANDS), ("flags", C.c_int32), ("noise_floor", C.c_float)]


EPOCH_CALIBRATION = 1


MONITOR_GNURADIO, MONITOR_PSD = 0, 1
PU_UNIFORM, PU_MARKOV_AS_WRITTEN, PU_MARKOV_INTENDED, PU_SWEEP = 0, 1, 2, 3
SIG_TONES, SIG_CW, SIG_BAND_NOISE, SIG_RRC_QPSK, SIG_GMSK, SIG_OFDM = 0, 1, 2, 3, 4, 5


class SenseStats(C.Structure):
    _fields_ = [("launches", C.c_int64), ("epochs", C.c_int64), ("samples", C.c_int64), ("timed_launches", C.c_int64),
                ("kernel_ms", C.c_double), ("kernel_ms_last", C.c_double), ("kernel_ms_min", C.c_double), ("kernel_ms_max", C.c_double)]


class IngestStats(C.Structure):
    _fields_ = [("packets", C.c_int64), ("dropped", C.c_int64), ("batches", C.c_int64), ("batches_failed", C.c_int64),
                ("epochs_launched", C.c_int64), ("epochs_ready", C.c_int64), ("epochs_polled", C.c_int64),
                ("latency_us_sum", C.c_double), ("latency_us_max", C.c_double)]


class CommInfo(C.Structure):
    _fields_ = [("nranks", C.c_int32), ("rank", C.c_int32), ("rccl_device", C.c_int32), ("rccl_version", C.c_int32),
                ("device", C.c_int32), ("depth", C.c_int32), ("bytes_per_rank", C.c_int64), ("gathers", C.c_int64),
                ("library", C.c_char * 128), ("pci_bus_id", C.c_char * 32)]


class SynthCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("noise_power", C.c_float), ("signal_rms", C.c_float),
                ("tones_per_band", C.c_int32), ("pu_model", C.c_int32), ("signal_kind", C.c_int32),
                ("n_streams", C.c_int32), ("adc_bits", C.c_int32)]


class TrainCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("iterations", C.c_int32), ("restarts", C.c_int32), ("eta", C.c_float),
                ("alpha", C.c_float), ("normalise", C.c_int32), ("reserved", C.c_int32)]


class CrnError(RuntimeError):
    pass


_lib = None


def lib():
    """Load libcrnsense.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CrnError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
        # A process that uses both PyTorch and this library must load PyTorch first: the wheel bundles its own ROCm runtime, and when
        # /opt/rocm's copy (which libcrnsense links) is loaded before it the two HSA runtimes collide — the library then reports
        # "no ROCm-capable device is detected".  Tests and bench.py use torch for device memory, so pin the order here.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        if L.crn_abi_version() != CRN_ABI_VERSION:   # the ctypes structures below mirror ONE version of include/crn_sense.h
            raise CrnError(f"{LIB_PATH} speaks ABI version {L.crn_abi_version()}, crnsense.py mirrors version {CRN_ABI_VERSION}: rebuild the library")
        L.crn_last_error.restype = C.c_char_p
        L.crn_build_info.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.crn_cfg_reference.argtypes = [C.POINTER(Cfg)]
        L.crn_cfg_energy_scaled.argtypes = [C.POINTER(Cfg), C.c_int32, C.c_float]
        L.crn_cfg_welch.argtypes = [C.POINTER(Cfg), C.c_int32, C.c_int32, C.c_int32]
        L.crn_cfg_reference_scaled.argtypes = [C.POINTER(Cfg), C.c_int32]
        L.crn_cfg_welch_scaled.argtypes = [C.POINTER(Cfg), C.c_int32, C.c_int32, C.c_float]
        L.crn_cfg_save_ann.argtypes = [C.POINTER(Cfg), C.c_char_p]
        L.crn_cfg_load_ann.argtypes = [C.POINTER(Cfg), C.c_char_p]
        L.crn_sense_set_ann.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        L.crn_sense_set_bands.argtypes = [C.c_void_p, C.POINTER(BandSeg), C.c_int32, C.c_int32, C.POINTER(C.c_float)]
        L.crn_sense_synchronize.argtypes = [C.c_void_p, C.c_void_p]
        L.crn_noise_floor_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float)]
        L.crn_sense_create.argtypes = [C.POINTER(Cfg), C.POINTER(C.c_void_p)]
        L.crn_sense_destroy.argtypes = [C.c_void_p]
        L.crn_sense_run_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                           C.POINTER(Out), C.c_void_p]
        if hasattr(L, "crn_sense_run_device_sc16"):   # a library built with make SC16=1
            L.crn_sense_run_device_sc16.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                                    C.POINTER(Out), C.c_void_p]
            L.crn_sense_set_wire_full_scale.argtypes = [C.c_void_p, C.c_double]
            L.crn_pack_sc16_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.crn_ingest_create_sc16.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
            L.crn_ingest_push_sc16.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.crn_sense_run_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                         C.POINTER(Out)]
        L.crn_synth_fill_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64,
                                            C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
        L.crn_synth_fill_device_ex.argtypes = [C.c_void_p, C.POINTER(SynthCfg), C.c_void_p, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_void_p]
        L.crn_ann_train_device.argtypes = [C.c_void_p, C.POINTER(TrainCfg), C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
        L.crn_fft_forward_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p,
                                             C.c_void_p]
        L.crn_sense_kernel_info.argtypes = [C.c_void_p, C.c_char_p, C.c_int32, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.crn_sense_set_variant.argtypes = [C.c_void_p, C.c_int32]
        L.crn_sense_set_cfar.argtypes = [C.c_void_p, C.POINTER(CfarParams)]
        L.crn_sense_get_cfar.argtypes = [C.c_void_p, C.POINTER(CfarParams), C.POINTER(C.c_int32)]
        L.crn_sense_run_device_cfar.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.POINTER(Out),
                                                C.c_void_p, C.c_void_p, C.c_void_p]
        L.crn_cfar_alpha.argtypes = [C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        L.crn_sense_set_cfar_ex.argtypes = [C.c_void_p, C.POINTER(CfarParamsEx)]
        L.crn_sense_get_cfar_ex.argtypes = [C.c_void_p, C.POINTER(CfarParamsEx), C.POINTER(C.c_int32)]
        L.crn_cfar_alpha_ex.argtypes = [C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        L.crn_segments_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(SegmentParams), C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        L.crn_tracks_workspace_bytes.argtypes = [C.c_int64, C.POINTER(TrackParams)]
        L.crn_tracks_workspace_bytes.restype = C.c_int64
        L.crn_tracks_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(TrackParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p]
        for f in (L.crn_tracks_carry_bytes, L.crn_tracks_carry_workspace_bytes):
            f.argtypes, f.restype = [C.c_int64, C.POINTER(TrackParams)], C.c_int64
        L.crn_tracks_carry_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(TrackParams), C.c_int64, C.c_int32, C.c_void_p,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.crn_channels_workspace_bytes.argtypes, L.crn_channels_workspace_bytes.restype = [C.c_int64, C.POINTER(ChannelParams)], C.c_int64
        L.crn_channels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ChannelParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_void_p]
        L.crn_channel_forecast.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.crn_fuse_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(FuseParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        L.crn_fuse_member_pfa.argtypes = [C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        L.crn_holes_workspace_bytes.argtypes, L.crn_holes_workspace_bytes.restype = [C.c_int64, C.POINTER(HoleParams)], C.c_int64
        L.crn_holes_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(HoleParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.crn_lad_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(LadParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.crn_lad_factor.argtypes = [C.c_double, C.c_int32, C.c_double, C.POINTER(C.c_double)]
        L.crn_tcfar_hist_bytes.argtypes, L.crn_tcfar_hist_bytes.restype = [C.c_int64, C.c_int32, C.POINTER(TcfarParams)], C.c_int64
        L.crn_tcfar_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(TcfarParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p]
        L.crn_measure_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(MeasureParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.crn_occmap_workspace_bytes.argtypes, L.crn_occmap_workspace_bytes.restype = [C.c_int64, C.POINTER(OccmapParams)], C.c_int64
        L.crn_occmap_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(OccmapParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p]
        L.crn_cyclo_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(CycloParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
        L.crn_cyclo_zmin.argtypes = [C.c_double, C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        for f in (L.crn_hops_bytes, L.crn_hops_workspace_bytes):
            f.argtypes, f.restype = [C.c_int64, C.POINTER(HopParams)], C.c_int64
        L.crn_hops_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(HopParams), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.crn_hop_forecast.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_double, C.POINTER(C.c_double)]
        L.crn_extract_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ExtractParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
        L.crn_resample_state_bytes.argtypes, L.crn_resample_state_bytes.restype = [C.c_int64], C.c_int64
        L.crn_resample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ResampleParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        L.crn_ingest_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.crn_ingest_push.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.crn_ingest_flush.argtypes = [C.c_void_p]
        L.crn_ingest_poll.argtypes = [C.c_void_p, C.POINTER(EpochResult), C.c_int32, C.POINTER(C.c_int32)]
        L.crn_ingest_drain.argtypes = [C.c_void_p]
        L.crn_ingest_destroy.argtypes = [C.c_void_p]
        L.crn_ingest_set_packet_len.argtypes = [C.c_void_p, C.c_int32]
        L.crn_ingest_wait.argtypes = [C.c_void_p]
        L.crn_ingest_dropped.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.crn_ingest_packets_per_epoch.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.crn_sense_reserve_host.argtypes = [C.c_void_p, C.c_int64, C.c_int32]
        L.crn_noise_floor_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_void_p]
        L.crn_sense_set_thresholds.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_void_p]
        L.crn_sense_reserve_noise_floor.argtypes = [C.c_void_p]
        L.crn_sense_calibrate_thresholds.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.POINTER(C.c_float), C.c_void_p]
        L.crn_ingest_calibrate.argtypes = [C.c_void_p, C.c_int32, C.c_float]
        L.crn_ingest_noise_floor.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        L.crn_sense_set_timing.argtypes = [C.c_void_p, C.c_int32]
        L.crn_sense_dealt_launches.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.crn_sense_get_stats.argtypes = [C.c_void_p, C.POINTER(SenseStats)]
        L.crn_ingest_get_stats.argtypes = [C.c_void_p, C.POINTER(IngestStats)]
        L.crn_monitor_rows_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_int32,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.crn_comm_unique_id.argtypes = [C.c_void_p]
        L.crn_comm_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                      C.POINTER(C.c_void_p)]
        L.crn_comm_local.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]
        L.crn_comm_allgather.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.crn_comm_local_addr.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.crn_comm_wait.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        L.crn_comm_gathered.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.crn_comm_finish.argtypes = [C.c_void_p, C.c_void_p]
        L.crn_comm_destroy.argtypes = [C.c_void_p]
        L.crn_comm_info.argtypes = [C.c_void_p, C.POINTER(CommInfo)]
        _lib = L
    return _lib


def has_sc16():
    """Does the loaded library carry the optional wire-format kernels and entry points (a `make SC16=1` build)?  (False, not an error,
    while the library has not been built yet: test modules ask at import time, before the fixture that builds it has run.)"""
    if _lib is None and not os.path.exists(LIB_PATH):
        return False
    return hasattr(lib(), "crn_sense_run_device_sc16")


def _need_sc16(what):
    if not has_sc16():
        raise CrnError(f"{what}: {LIB_PATH} was built without the optional wire-format kernels "
                       "(make -C csrc SC16=1 builds libcrnsense_sc16.so; select it with $CRN_SENSE_LIB)")


def build_info():
    """(built_hip, runtime_hip, compatible): HIP_VERSION the library was compiled with, the runtime's, and crn_build_info's verdict."""
    b, r = C.c_int32(), C.c_int32()
    rc = lib().crn_build_info(C.byref(b), C.byref(r))
    return b.value, r.value, rc == 0


def check(rc, what):
    if rc != 0:
        raise CrnError(f"{what} failed ({rc}): {lib().crn_last_error().decode()}")


def cfg_reference():
    c = Cfg()
    check(lib().crn_cfg_reference(C.byref(c)), "crn_cfg_reference")
    return c


def cfg_energy_scaled(fft_len, lam=4.0):
    c = Cfg()
    check(lib().crn_cfg_energy_scaled(C.byref(c), fft_len, lam), "crn_cfg_energy_scaled")
    return c


def cfg_reference_scaled(fft_len):
    c = Cfg()
    check(lib().crn_cfg_reference_scaled(C.byref(c), fft_len), "crn_cfg_reference_scaled")
    return c


def cfg_welch_scaled(fft_len, frames_per_epoch=8, lam=4.0):
    c = Cfg()
    check(lib().crn_cfg_welch_scaled(C.byref(c), fft_len, frames_per_epoch, lam), "crn_cfg_welch_scaled")
    return c


def _cfar_method(method):
    if method not in CFAR_METHODS:
        raise ValueError(f"CFAR method must be one of {sorted(CFAR_METHODS)}, not {method!r}")
    return CFAR_METHODS[method]


def cfar_os_rank(train):
    """The default OS-CFAR rank: 3/4 of the 2 W training cells."""
    return 3 * 2 * int(train) // 4


def cfar_alpha(pfa, K, train, method="ca", rank=None):
    """CFAR scale alpha for a per-bin false-alarm probability pfa at K frames per epoch and `train` training cells per side
    (white complex Gaussian noise, rectangular window, disjoint frames: include/crn_sense.h, crn_cfar_alpha / crn_cfar_alpha_ex).
    method: "ca", "go", "so" or "os"; rank (OS only) defaults to cfar_os_rank(train)."""
    a = C.c_double()
    if method == "ca" and rank is None:
        check(lib().crn_cfar_alpha(float(pfa), int(K), int(train), C.byref(a)), "crn_cfar_alpha")
        return a.value
    m = _cfar_method(method)
    if rank is None:
        rank = cfar_os_rank(train) if m == CFAR_OS else 0
    check(lib().crn_cfar_alpha_ex(m, float(pfa), int(K), int(train), int(rank), C.byref(a)), "crn_cfar_alpha_ex")
    return a.value


def segment_hz(lo, width, centroid, fft_len, fs, fc):
    """(centre frequency, bandwidth) in Hz of a segment from crn_segments_device: the centre is the power centroid, at bin
    lo + centroid; bin k lies at fc + k fs / N for k < N / 2 and at fc + (k - N) fs / N above, so a segment that crosses the wrap
    (lo + width > N) comes out as one emitter around fc.  The bandwidth is width bins."""
    k = (float(lo) + float(centroid)) % fft_len
    if k >= fft_len / 2:
        k -= fft_len
    return fc + k * fs / fft_len, width * fs / fft_len


def track_params(max_segments=16, epochs_per_stream=1, slack_bins=1, max_miss=0, min_epochs=1, max_tracks=64):
    q = TrackParams(max_segments=int(max_segments), epochs_per_stream=int(epochs_per_stream), slack_bins=int(slack_bins), max_miss=int(max_miss),
                    min_epochs=int(min_epochs), max_tracks=int(max_tracks))
    q.reserved[0] = q.reserved[1] = 0
    return q


def tracks_workspace_bytes(n_epochs, max_segments=16, epochs_per_stream=None, max_miss=0, min_epochs=1, max_tracks=64):
    """Bytes of device scratch Sensor.tracks_device needs (crn_tracks_workspace_bytes): no handle, no device."""
    q = track_params(max_segments, n_epochs if epochs_per_stream is None else epochs_per_stream, 0, max_miss, min_epochs, max_tracks)
    nb = lib().crn_tracks_workspace_bytes(int(n_epochs), C.byref(q))
    if nb <= 0:
        raise CrnError(f"crn_tracks_workspace_bytes: arguments out of range ({nb})")
    return nb


def tracks_carry_bytes(n_streams, max_segments=16, max_miss=0):
    """Bytes of the per-stream carry Sensor.tracks_carry_device reads and rewrites (crn_tracks_carry_bytes): no handle, no device."""
    q = track_params(max_segments, 1, 0, max_miss, 1, 1)
    nb = lib().crn_tracks_carry_bytes(int(n_streams), C.byref(q))
    if nb <= 0:
        raise CrnError(f"crn_tracks_carry_bytes: arguments out of range ({nb})")
    return nb


def tracks_carry_workspace_bytes(n_epochs, max_segments=16, epochs_per_stream=None, max_miss=0):
    """Bytes of device scratch Sensor.tracks_carry_device needs (crn_tracks_carry_workspace_bytes): no handle, no device."""
    q = track_params(max_segments, n_epochs if epochs_per_stream is None else epochs_per_stream, 0, max_miss, 1, 1)
    nb = lib().crn_tracks_carry_workspace_bytes(int(n_epochs), C.byref(q))
    if nb <= 0:
        raise CrnError(f"crn_tracks_carry_workspace_bytes: arguments out of range ({nb})")
    return nb


def track_hz(centre, width_sum, n_segments, fft_len, fs, fc):
    """(centre frequency, mean bandwidth) in Hz of a track from crn_tracks_device: `centre` is already an absolute bin (the power-weighted
    mean position of the members), the bandwidth is the members' mean width, width_sum / n_segments bins; the mapping of bins to hertz
    is segment_hz's."""
    return segment_hz(0, float(width_sum) / max(int(n_segments), 1), centre, fft_len, fs, fc)


def channel_params(spans, epochs_per_stream, min_bins=1, first=False):
    """crn_channel_params from a list of (lo, width) pairs or ChannelSpan."""
    spans = [(sp.lo, sp.width) if isinstance(sp, ChannelSpan) else (int(sp[0]), int(sp[1])) for sp in spans]
    if len(spans) > CRN_MAX_CHANNELS:
        raise ValueError(f"at most {CRN_MAX_CHANNELS} channels, not {len(spans)}")
    q = ChannelParams(n_channels=len(spans), epochs_per_stream=int(epochs_per_stream), min_bins=int(min_bins), first=int(bool(first)))
    for c, (lo, width) in enumerate(spans):
        q.span[c].lo, q.span[c].width = lo, width
    return q


def channels_workspace_bytes(n_epochs, spans, epochs_per_stream=None, min_bins=1):
    """Bytes of device scratch Sensor.channels_device needs (crn_channels_workspace_bytes): no handle, no device."""
    q = channel_params(spans, n_epochs if epochs_per_stream is None else epochs_per_stream, min_bins)
    nb = lib().crn_channels_workspace_bytes(int(n_epochs), C.byref(q))
    if nb <= 0:
        raise CrnError(f"crn_channels_workspace_bytes: arguments out of range ({nb})")
    return nb


def fuse_params(rule, group_size, epochs_per_stream, votes=0, guard=0, train=0, alpha=0.0, weights=None):
    """crn_fuse_params: rule FUSE_VOTE (votes = k of the active members) or FUSE_SOFT (guard, train, alpha: CA-CFAR on the fused row, alpha
    from cfar_alpha(pfa, n_active * K, train)); weights one per member, 0 = the member is left out, None = equal gain, 1 / group_size."""
    m = int(group_size)
    if weights is None:
        weights = [1.0 / m] * m if 1 <= m <= CRN_MAX_FUSE_MEMBERS else []
    if len(weights) > CRN_MAX_FUSE_MEMBERS:
        raise ValueError(f"at most {CRN_MAX_FUSE_MEMBERS} members, not {len(weights)}")
    q = FuseParams(rule=int(rule), group_size=m, epochs_per_stream=int(epochs_per_stream), votes=int(votes), guard=int(guard), train=int(train),
                   alpha=float(alpha))
    for i, w in enumerate(weights):
        q.weight[i] = float(w)
    return q


def fuse_member_pfa(pfa, n, k):
    """The per-sensor false-alarm probability at which k-of-n voting of independent sensors gives `pfa` (crn_fuse_member_pfa); it goes into
    cfar_alpha(p, K, train)."""
    p = C.c_double()
    check(lib().crn_fuse_member_pfa(float(pfa), int(n), int(k), C.byref(p)), "crn_fuse_member_pfa")
    return p.value


def hole_params(epochs_per_stream, guard=0, min_age=1, min_width=1, max_holes=16, avg_epochs=1, first=False):
    """crn_hole_params."""
    return HoleParams(epochs_per_stream=int(epochs_per_stream), first=int(bool(first)), guard=int(guard), min_age=int(min_age),
                      min_width=int(min_width), max_holes=int(max_holes), avg_epochs=int(avg_epochs), reserved=0)


def holes_workspace_bytes(n_epochs, epochs_per_stream=None, guard=0, min_age=1, min_width=1, max_holes=16, avg_epochs=1):
    """Bytes of device scratch Sensor.holes_device needs (crn_holes_workspace_bytes): no handle, no device."""
    q = hole_params(n_epochs if epochs_per_stream is None else epochs_per_stream, guard, min_age, min_width, max_holes, avg_epochs)
    nb = lib().crn_holes_workspace_bytes(int(n_epochs), C.byref(q))
    if nb <= 0:
        raise CrnError(f"crn_holes_workspace_bytes: arguments out of range ({nb})")
    return nb


def lad_params(n_blocks=1, init_percent=10, t_cme=0.0, t_lower=0.0, t_upper=0.0):
    """crn_lad_params: the factors come from lad_factor, t_cme = lad_factor(pfa_cme, K) and t_lower, t_upper = lad_factor(pfa, K, t_cme)."""
    return LadParams(n_blocks=int(n_blocks), init_percent=int(init_percent), t_cme=float(t_cme), t_lower=float(t_lower), t_upper=float(t_upper))


def lad_factor(pfa, K, t_cme=0.0):
    """The threshold factor over the excised floor at which a noise bin (the mean of K frames) exceeds it with probability pfa
    (crn_lad_factor): t_cme = 0 gives the plain Gamma(K) quantile, which is the FCME factor itself; with t_cme > 0 the quantile is divided
    by the mean the excision converges to in noise."""
    f = C.c_double()
    check(lib().crn_lad_factor(float(pfa), int(K), float(t_cme), C.byref(f)), "crn_lad_factor")
    return f.value


def tcfar_params(epochs_per_stream, cells, rank, alpha, guard_epochs=1, first=False):
    """crn_tcfar_params: alpha from tcfar_alpha(pfa, K, cells, rank)."""
    return TcfarParams(epochs_per_stream=int(epochs_per_stream), first=int(bool(first)), cells=int(cells), guard_epochs=int(guard_epochs),
                       rank=int(rank), alpha=float(alpha))


def tcfar_alpha(pfa, K, cells, rank):
    """alpha of crn_tcfar_device for a per-bin false-alarm probability pfa at K frames per epoch: the ordered-statistic CFAR's, whose
    training cells are the bin's own `cells` earlier epochs (cfar_alpha(..., method="os") with train = cells // 2)."""
    return cfar_alpha(pfa, K, int(cells) // 2, method="os", rank=int(rank))


def tcfar_hist_bytes(n_streams, fft_len, params):
    """Bytes of the history Sensor.tcfar_device carries for n_streams streams (crn_tcfar_hist_bytes): no handle, no device."""
    nb = lib().crn_tcfar_hist_bytes(int(n_streams), int(fft_len), C.byref(params))
    if nb <= 0:
        raise CrnError(f"crn_tcfar_hist_bytes: arguments out of range ({nb})")
    return nb


def xdb_ratio(db):
    """The linear power ratio of an x-dB rule, 10^(-db / 10), for crn_measure_params.xdb_ratio: 26 dB gives 10^-2.6."""
    return 10.0 ** (-float(db) / 10.0)


def measure_params(max_segments=16, obw_percent=99.0, xdb=26.0, subtract_noise=True):
    """crn_measure_params: max_segments as given to the segment stage; obw_percent the share of the net power inside the occupied
    bandwidth, split evenly between the two tails (99 % leaves 5000 ppm on each side); xdb the depth of the x-dB rule in dB."""
    return MeasureParams(max_segments=int(max_segments), tail_ppm=int(round((100.0 - float(obw_percent)) * 5000.0)), xdb_ratio=xdb_ratio(xdb),
                         subtract_noise=int(bool(subtract_noise)))


def measure_hz(lo, obw_lo, obw_width, xdb_lo, xdb_width, fft_len, fs, fc):
    """((centre frequency, occupied bandwidth), (centre frequency, x-dB bandwidth)) in Hz of a record from crn_measure_device and the lo
    of its segment: each centre is the middle of its span, at bin lo + offset + (width - 1) / 2, and the mapping of bins to hertz is
    segment_hz's, so a span that crosses the wrap comes out around fc.  A width of 0 (not measured, or no bin above the line) gives
    a bandwidth of 0 at the segment's first bin."""
    def span(off, width):
        return segment_hz(lo, width, float(off) + max(float(width) - 1.0, 0.0) / 2.0, fft_len, fs, fc)
    return span(obw_lo, obw_width), span(xdb_lo, xdb_width)


def occmap_params(epochs_per_stream, duty=0.5, first=False):
    """crn_occmap_params: `duty` is the busy fraction from which a bin enters the usual mask, kept in parts per million."""
    return OccmapParams(epochs_per_stream=int(epochs_per_stream), first=int(bool(first)), duty_ppm=int(round(float(duty) * 1e6)))


def occmap_workspace_bytes(n_epochs, epochs_per_stream=None, duty=0.5):
    """Bytes of device scratch Sensor.occmap_device needs (crn_occmap_workspace_bytes): no handle, no device."""
    q = occmap_params(n_epochs if epochs_per_stream is None else epochs_per_stream, duty)
    nb = lib().crn_occmap_workspace_bytes(int(n_epochs), C.byref(q))
    if nb < 0:
        raise CrnError(f"crn_occmap_workspace_bytes: arguments out of range ({nb})")
    return nb


def occupancy_map(records):
    """What the records of crn_occmap_device (OCCMAP_BIN_DTYPE, any shape) say per bin, as a dict of arrays of that shape: `duty` =
    n_busy / n_epochs (the frequency channel occupancy), `rise_rate` = n_rise / n_epochs (idle -> busy transitions per epoch),
    `mean_idle` = power[0] / (n_epochs - n_busy) (the noise floor's shape) and `mean_busy` = power[1] / n_busy, each 0 where its count
    is 0; `max_hold` and `min_hold` as they are."""
    import numpy as np
    r = np.asarray(records)
    n, nb = r["n_epochs"].astype(np.float64), r["n_busy"].astype(np.float64)

    def over(num, den):
        return np.divide(num, den, out=np.zeros(r.shape, np.float64), where=den > 0)
    return {"duty": over(nb, n), "rise_rate": over(r["n_rise"].astype(np.float64), n), "mean_idle": over(r["power"][..., 0], n - nb),
            "mean_busy": over(r["power"][..., 1], nb), "max_hold": r["max_hold"].copy(), "min_hold": r["min_hold"].copy()}


def floor_db(records, fallback=None):
    """The noise floor per bin in dB, 10 log10 of occupancy_map's mean_idle.  A bin never seen idle, or whose idle mean is not positive,
    has no floor of its own: it takes `fallback` (dB), NaN when that is None."""
    import numpy as np
    m = occupancy_map(records)["mean_idle"]
    out = np.full(m.shape, np.nan if fallback is None else float(fallback), np.float64)
    np.log10(m, out=out, where=m > 0)
    return np.where(m > 0, 10.0 * out, out)


def cyclo_zmin(pfa, frames, n_pairs):
    """z_min of crn_cyclo_params at which a tested cell of n_pairs pairs exceeds it in noise with probability pfa (crn_cyclo_zmin; a
    Gamma approximation).  Pass the smallest n_pairs in use, min_pairs: the conservative choice."""
    z = C.c_double()
    check(lib().crn_cyclo_zmin(float(pfa), int(frames), int(n_pairs), C.byref(z)), "crn_cyclo_zmin")
    return z.value


def cyclo_params(max_segments=16, frames=32, a_lo=8, n_a=64, max_width=256, min_pairs=16, z_min=None, pfa=1e-6):
    """crn_cyclo_params: max_segments as given to the segment stage, frames the frames of an epoch in the array of spectra; separations
    a_lo .. a_lo + n_a - 1 bins over the central max_width bins of a segment, a cell tested from min_pairs pairs on; z_min as given or
    cyclo_zmin(pfa, frames, min_pairs)."""
    z = cyclo_zmin(pfa, frames, min_pairs) if z_min is None else z_min
    return CycloParams(max_segments=int(max_segments), frames=int(frames), a_lo=int(a_lo), n_a=int(n_a), max_width=int(max_width),
                       min_pairs=int(min_pairs), z_min=float(z))


def cyclo_bins(rec, frames):
    """The symbol rate in bins from a record of crn_cyclo_device (a CYCLO_DTYPE element, a Cyclo, or anything with those fields by name
    or key): the peak in a is interpolated over its two neighbours, a^ = a + (stat_hi - stat_lo) / (stat_lo + stat + stat_hi), and the
    value congruent to q / frames modulo one bin that lies nearest a^ is returned.  0.0 for a record with no tested cell."""
    get = (lambda k: getattr(rec, k)) if hasattr(rec, "stat") else (lambda k: rec[k])
    a, q, s0, s1, s2 = int(get("a")), int(get("q")), float(get("stat_lo")), float(get("stat")), float(get("stat_hi"))
    if int(get("n_pairs")) <= 0:
        return 0.0
    total = s0 + s1 + s2
    a_hat = a + ((s2 - s0) / total if total > 0.0 else 0.0)
    frac = q / float(frames)
    return float(round(a_hat - frac)) + frac


def cyclo_hz(rec, frames, fft_len, fs):
    """The symbol rate in Hz: cyclo_bins x fs / fft_len."""
    return cyclo_bins(rec, frames) * float(fs) / float(fft_len)


def extract_params(out_len, frames_per_stream, t0=0):
    """crn_extract_params: out_len = M samples of a block, of which M / 2 are kept per frame; frames_per_stream = F; t0 = the frames of
    each stream that earlier calls were given."""
    return ExtractParams(out_len=int(out_len), frames_per_stream=int(frames_per_stream), t0=int(t0))


def extract_taper(out_len, flat):
    """The taper H of crn_extract_device as float32 [out_len], entry j for offset i = j - M / 2: 1 for |i| <= flat, a raised-cosine
    roll-off 0.5 (1 + cos(pi (|i| - flat) / (M / 2 - flat))) beyond, which reaches 0 at i = -M / 2.  Computed in float64 and rounded once."""
    import numpy as np
    m, flat = int(out_len), int(flat)
    if m not in EXTRACT_OUT_LENS or not 0 <= flat < m // 2:
        raise ValueError(f"extract_taper: out_len must be one of {EXTRACT_OUT_LENS} and 0 <= flat < out_len / 2, not {out_len}, {flat}")
    i = np.abs(np.arange(m, dtype=np.float64) - m // 2)
    h = np.where(i <= flat, 1.0, 0.5 * (1.0 + np.cos(np.pi * (i - flat) / (m // 2 - flat))))
    h[0] = 0.0
    return h.astype(np.float32)


def extract_channels(records, stream=0, fft_len=None):
    """Channel records (EXTRACT_CHANNEL_DTYPE) for the emitters of ONE stream: `records` are that stream's track records (TRACK_DTYPE: the
    rounded `centre`), or segment records of one of its epochs (SEGMENT_DTYPE: lo + the rounded `centroid`), or plain bin numbers;
    `stream` is carried into every record.  With fft_len the centres are taken into 0 .. fft_len - 1 (the stage does so itself)."""
    import numpy as np
    r = np.asarray(records)
    names = r.dtype.names or ()
    if "centre" in names:
        centre = np.rint(r["centre"].astype(np.float64))
    elif "centroid" in names:
        centre = r["lo"].astype(np.float64) + np.rint(r["centroid"].astype(np.float64))
    else:
        centre = np.rint(r.astype(np.float64))
    centre = centre.reshape(-1).astype(np.int64)
    if fft_len is not None:
        centre %= int(fft_len)
    out = np.zeros(centre.size, np.dtype(EXTRACT_CHANNEL_DTYPE))
    out["stream"], out["centre"] = int(stream), centre
    return out


def extract_rate(fs, fft_len, out_len):
    """Sample rate of the streams crn_extract_device writes: fs out_len / fft_len."""
    return float(fs) * int(out_len) / int(fft_len)


def resample_params(in_len, out_cap, taps=16, phases=128, first=False):
    """crn_resample_params: in_len samples of every input row, out_cap of every output row (resample_out_cap), T = taps, P = phases;
    first: the states' contents mean nothing."""
    return ResampleParams(in_len=int(in_len), out_cap=int(out_cap), taps=int(taps), phases=int(phases), first=int(bool(first)))


def resample_rows(ratio, offset=0.0):
    """Row records (RESAMPLE_ROW_DTYPE) of crn_resample_device, one per entry of `ratio`: step = rint(ratio 2^32), ratio in input
    samples per output sample (resample_ratio); dphi = rint(offset 2^32) wrapped to int32, `offset` in cycles per OUTPUT sample, the
    frequency the mixer adds.  Either may be a scalar.  A ratio outside 1/4 .. 4 makes a row that the stage answers with zeros; ValueError
    for a ratio or an offset that is not finite."""
    import numpy as np
    ratio, offset = np.broadcast_arrays(np.atleast_1d(np.asarray(ratio, np.float64)), np.asarray(offset, np.float64))
    out = np.zeros(ratio.size, np.dtype(RESAMPLE_ROW_DTYPE))
    if not (np.isfinite(ratio).all() and np.isfinite(offset).all()):
        raise ValueError(f"resample_rows: ratio and offset must be finite, not {ratio.tolist()}, {offset.tolist()}")
    for i, (rho, off) in enumerate(zip(ratio.reshape(-1), offset.reshape(-1))):
        step = int(np.rint(rho * 2.0 ** 32)) if 0 <= rho < 2.0 ** 31 else 0
        dphi = (int(np.rint(off * 2.0 ** 32)) + 2 ** 31) % 2 ** 32 - 2 ** 31
        out[i] = (step, dphi, 0)
    return out


def resample_out_cap(in_len, min_ratio):
    """The most outputs a call of in_len input samples can give a row whose ratio is at least min_ratio: step 1's n at pos = 0."""
    import numpy as np
    step = int(np.rint(float(min_ratio) * 2.0 ** 32))
    if int(in_len) < 1 or not 2 ** 30 <= step <= 2 ** 34:
        raise ValueError(f"resample_out_cap: in_len >= 1 and min_ratio in 1/4 .. 4, not {in_len}, {min_ratio}")
    return ((int(in_len) << 32) - 1) // step + 1


def resample_state_bytes(n_rows):
    """Bytes of the states of n_rows rows (320 each)."""
    nb = lib().crn_resample_state_bytes(int(n_rows))
    if nb < 0:
        raise ValueError(f"resample_state_bytes: n_rows must be in 0..65536, not {n_rows}")
    return nb


def resample_ratio(out_len, symbol_bins, sps):
    """Input samples per output sample that bring a stream of crn_extract_device (out_len = M) to sps samples per symbol, for a symbol
    rate of symbol_bins bins (cyclo_bins): out_len / symbol_bins / sps.  ValueError for a rate of 0 (nothing was found)."""
    if not symbol_bins > 0 or not sps > 0:
        raise ValueError(f"resample_ratio: symbol rate and samples per symbol must be positive, not {symbol_bins}, {sps}")
    return float(out_len) / float(symbol_bins) / float(sps)


def resample_delay(taps):
    """Input samples by which the output of crn_resample_device lags its position, for a table of resample_taps: T / 2."""
    return int(taps) // 2


def resample_taps(taps, phases, cutoff, beta):
    """The polyphase table h of crn_resample_device as float32 [phases + 1][taps]: h[phi][k] = g(k - T / 2 + phi / P), g(t) = 2 fc
    sinc(2 fc t) I0(beta sqrt(1 - (2 t / T)^2)) / I0(beta) for |t| < T / 2 and 0 beyond, fc = cutoff in cycles per input sample; scaled
    once so that the entries of rows 0 .. P - 1 sum to P.  Computed in float64 and rounded once."""
    import numpy as np
    T, P = int(taps), int(phases)
    if T not in RESAMPLE_TAPS or P not in RESAMPLE_PHASES or not 0 < cutoff <= 0.5 or not beta >= 0:
        raise ValueError(f"resample_taps: taps in {RESAMPLE_TAPS}, phases in {RESAMPLE_PHASES}, 0 < cutoff <= 0.5, beta >= 0, not {taps}, {phases}, {cutoff}, {beta}")
    t = np.arange(T, dtype=np.float64)[None, :] - T // 2 + np.arange(P + 1, dtype=np.float64)[:, None] / P
    inside = np.abs(t) < T / 2
    g = np.where(inside, 2 * cutoff * np.sinc(2 * cutoff * t) * np.i0(beta * np.sqrt(np.where(inside, 1 - (2 * t / T) ** 2, 0.0))) / np.i0(beta), 0.0)
    return (g * (P / g[:P].sum())).astype(np.float32)


def hop_params(n_channels, epochs_per_stream, lags=(1,), first=False):
    """crn_hop_params: `lags` strictly ascending, each in 1..64, at most 8 of them."""
    lags = [int(d) for d in lags]
    if len(lags) > 8:
        raise ValueError(f"at most 8 lags, not {len(lags)}")
    q = HopParams(n_channels=int(n_channels), epochs_per_stream=int(epochs_per_stream), n_lags=len(lags), first=int(bool(first)))
    for m, d in enumerate(lags):
        q.lag[m] = d
    return q


def hops_bytes(n_streams, n_channels, lags=(1,)):
    """Bytes of n_streams records of Sensor.hops_device (crn_hops_bytes): no handle, no device."""
    q = hop_params(n_channels, 1, lags)
    nb = lib().crn_hops_bytes(int(n_streams), C.byref(q))
    if nb < 0:
        raise CrnError(f"crn_hops_bytes: arguments out of range ({nb})")
    return nb


def hops_workspace_bytes(n_epochs, n_channels, epochs_per_stream=None, lags=(1,)):
    """Bytes of device scratch Sensor.hops_device needs (crn_hops_workspace_bytes): no handle, no device."""
    q = hop_params(n_channels, n_epochs if epochs_per_stream is None else epochs_per_stream, lags)
    nb = lib().crn_hops_workspace_bytes(int(n_epochs), C.byref(q))
    if nb <= 0:
        raise CrnError(f"crn_hops_workspace_bytes: arguments out of range ({nb})")
    return nb


def hop_record(buf, n_lags):
    """One record of crn_hops_device as numpy views of `buf` (bytes, or a uint8 array, of exactly one record of n_lags lags): a dict
    with n_epochs, n_channels, n_lags, lag [8], hist [64] uint64, hop [64][64], and from [n_lags][64], to [n_lags][64], pair
    [n_lags][64][64]; "raw" is the record itself, what hop_forecast hands to the library."""
    import numpy as np
    dt = hop_dtype(n_lags)
    raw = np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if raw.size != dt.itemsize:
        raise ValueError(f"hop_record takes ONE record of {dt.itemsize} bytes for {n_lags} lags, not {raw.size}")
    r = raw.view(dt)[0]
    return {"raw": raw, "n_epochs": r["n_epochs"], "n_channels": r["n_channels"], "n_lags": r["n_lags"], "lag": r["lag"], "hist": r["hist"],
            "hop": r["hop"], "from": r["lags"]["from"], "to": r["lags"]["to"], "pair": r["lags"]["pair"]}


def hop_forecast(rec, m, word, prior=1.0):
    """p [64] of crn_hop_forecast: how likely channel j is busy lag[m] epochs after an epoch whose busy word is `word` (p[63]: nothing
    busy), on one record as hop_record returns it (or its bytes)."""
    import numpy as np
    raw = rec["raw"] if isinstance(rec, dict) else np.frombuffer(rec, np.uint8)
    raw = np.ascontiguousarray(raw)
    p = (C.c_double * 64)()
    check(lib().crn_hop_forecast(raw.ctypes.data_as(C.c_void_p), int(m), int(word) & (2 ** 64 - 1), float(prior), p), "crn_hop_forecast")
    return np.array(p[:], np.float64)


def hop_table(rec, prior=0.0):
    """The jump chain of one record: [C + 1][C + 1], row i = hop[i][j] / sum_j hop[i][j] over the channels 0 .. C - 1 and, last, the idle
    state (`prior` added to every off-diagonal cell; a row never left is all zero).  With a primary user that dwells many epochs on a
    channel this is its transition table without the diagonal, rows renormalised."""
    import numpy as np
    nch = int(rec["n_channels"])
    idx = list(range(nch)) + [CRN_HOP_IDLE]
    h = np.maximum(np.asarray(rec["hop"], np.float64)[np.ix_(idx, idx)], 0.0) + float(prior) * (1.0 - np.eye(nch + 1))
    tot = h.sum(axis=1, keepdims=True)
    return np.divide(h, tot, out=np.zeros_like(h), where=tot > 0)


def next_channel(rec, word, horizon, prior=1.0):
    """The channel j < C least likely to be hit in the next `horizon` epochs given the busy word of the epoch at hand: the largest
    prod over d = 1 .. horizon of (1 - p_d[j]), p_d = hop_forecast at lag d; ties go to the lowest j.  ValueError unless the lags
    1 .. horizon are all in the record."""
    import numpy as np
    lags = [int(d) for d in rec["lag"][:int(rec["n_lags"])]]
    if horizon < 1 or any(d not in lags for d in range(1, horizon + 1)):
        raise ValueError(f"next_channel: the record keeps the lags {lags}, not all of 1 .. {horizon}")
    free = np.ones(64)
    for d in range(1, horizon + 1):
        free *= 1.0 - hop_forecast(rec, lags.index(d), word, prior)
    return int(np.argmax(free[:int(rec["n_channels"])]))


def hole_hz(lo, width, fft_len, fs, fc):
    """(centre frequency, bandwidth) in Hz of a hole from crn_holes_device: the centre is the geometric one, at bin lo + (width - 1) / 2,
    and the mapping of bins to hertz is segment_hz's, so a hole that crosses the wrap (lo + width > N) comes out around fc."""
    return segment_hz(lo, width, (float(width) - 1.0) / 2.0, fft_len, fs, fc)


def pick_hole(holes, need_bins):
    """The index of the stored hole to transmit in: among the holes of one stream (records of HOLE_DTYPE; slots with width 0 are empty) with
    width >= need_bins, the one idle longest (the largest `age`); ties go to the lower power per bin, then to the lower lo.  None when
    none fits."""
    best = None
    for i, h in enumerate(holes):
        w = int(h["width"])
        if w < 1 or w < need_bins:
            continue
        key = (-int(h["age"]), float(h["power"]) / w, int(h["lo"]), i)
        if best is None or key < best:
            best = key
    return None if best is None else best[3]


def channel_spans_from_bands(cfg):
    """[ChannelSpan] per band of a plan whose bands are single circular intervals (crn_cfg_welch's are): one segment, or two that meet
    at the wrap (one ends at fft_len, the other begins at 0).  ValueError for any other plan."""
    spans = []
    for b in range(cfg.n_bands):
        segs = sorted((cfg.segs[i].lo, cfg.segs[i].hi) for i in range(cfg.n_segs) if cfg.segs[i].band == b and cfg.segs[i].hi > cfg.segs[i].lo)
        if len(segs) == 1:
            lo, width = segs[0][0], segs[0][1] - segs[0][0]
        elif len(segs) == 2 and segs[0][0] == 0 and segs[1][1] == cfg.fft_len and segs[0][1] <= segs[1][0]:
            lo, width = segs[1][0], segs[1][1] - segs[1][0] + segs[0][1]
        else:
            raise ValueError(f"band {b} is not one circular interval: {segs}")
        spans.append(ChannelSpan(lo=lo % cfg.fft_len, width=width))
    return spans


def _channel_stats(row):
    """A ChannelStats from one numpy record of CHANNEL_STATS_DTYPE (or a ChannelStats)."""
    if isinstance(row, ChannelStats):
        return row
    import numpy as np
    raw = np.asarray(row, dtype=np.dtype(CHANNEL_STATS_DTYPE)).tobytes()
    if len(raw) != C.sizeof(ChannelStats):
        raise ValueError("channel_forecast takes ONE record of CHANNEL_STATS_DTYPE")
    return ChannelStats.from_buffer_copy(raw)


def channel_forecast(stats_row, horizon, prior=1.0):
    """(p01, p10, p_idle) of one record (crn_channel_forecast): the two-state chain's transition probabilities with `prior` added to
    every count, and the probability that the next `horizon` epochs are all idle."""
    st = _channel_stats(stats_row)
    p01, p10, pi = C.c_double(), C.c_double(), C.c_double()
    check(lib().crn_channel_forecast(C.byref(st), int(horizon), float(prior), C.byref(p01), C.byref(p10), C.byref(pi)), "crn_channel_forecast")
    return p01.value, p10.value, pi.value


def best_channel(stats_of_stream, horizon, prior=1.0, widths=None):
    """The channel of one stream's records most likely to stay idle for `horizon` epochs: the argmax of p_idle.  Ties go to the lower mean
    idle power per bin (power[0] over the idle epochs, over widths[c] when given; a channel never seen idle counts as the loudest), then to
    the lower index."""
    best = None
    for c, row in enumerate(stats_of_stream):
        st = _channel_stats(row)
        idle = st.n_epochs - st.n_busy
        quiet = st.power[0] / idle / (widths[c] if widths is not None else 1) if idle > 0 else float("inf")
        key = (-channel_forecast(st, horizon, prior)[2], quiet, c)
        if best is None or key < best:
            best = key
    if best is None:
        raise ValueError("best_channel: no records")
    return best[2]


def save_ann(cfg, path):
    check(lib().crn_cfg_save_ann(C.byref(cfg), os.fsencode(path)), "crn_cfg_save_ann")


def load_ann(cfg, path):
    check(lib().crn_cfg_load_ann(C.byref(cfg), os.fsencode(path)), "crn_cfg_load_ann")
    return cfg


def cfg_welch(fft_len, frames_per_epoch, n_bands):
    c = Cfg()
    check(lib().crn_cfg_welch(C.byref(c), fft_len, frames_per_epoch, n_bands), "crn_cfg_welch")
    return c


def samples_per_epoch(cfg, L=None):
    """Dense epoch length in samples (the default epoch_stride)."""
    L = cfg.fft_len if L is None else L
    return cfg.frames_per_epoch * (L if cfg.hop == cfg.fft_len else cfg.hop)


def samples_needed(cfg, n_epochs, L=None):
    """Samples a dense buffer must hold for n_epochs (overlap adds a tail)."""
    L = cfg.fft_len if L is None else L
    tail = 0 if cfg.hop == cfg.fft_len else cfg.fft_len - cfg.hop
    return n_epochs * samples_per_epoch(cfg, L) + tail


class Sensor:
    """Owns one crn_handle."""

    def __init__(self, cfg):
        self.cfg = cfg
        self._h = C.c_void_p()
        # Ingest objects attached to this handle: closed before it (crn_sense_destroy refuses otherwise).  Weak references: a ring keeps
        # its sensor alive, not the other way round, so a dropped Ingest is destroyed by its refcount (launcher thread, pinned buffers)
        self._rings = weakref.WeakSet()
        check(lib().crn_sense_create(C.byref(cfg), C.byref(self._h)), "crn_sense_create")

    def close(self):
        if self._h:
            for ring in list(self._rings):
                ring.close()
            check(lib().crn_sense_destroy(self._h), "crn_sense_destroy")
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve_host(self, max_epochs, want_spectrum=False):
        check(lib().crn_sense_reserve_host(self._h, max_epochs, int(want_spectrum)), "crn_sense_reserve_host")

    def set_variant(self, v):
        check(lib().crn_sense_set_variant(self._h, v), "crn_sense_set_variant")

    def noise_floor(self, features_ptr, n_epochs, stream=0):
        """Median over epochs of each epoch's median band energy (features [n_epochs][n_bands] on the device)."""
        nf = C.c_float()
        check(lib().crn_noise_floor_device(self._h, features_ptr, n_epochs, C.byref(nf), stream), "crn_noise_floor_device")
        return nf.value

    def set_thresholds(self, thresh, stream=0):
        """Replace the per-band thresholds (ordered on `stream`); also updates self.cfg so that a checker sees the same values."""
        arr = (C.c_float * len(thresh))(*[float(t) for t in thresh])
        check(lib().crn_sense_set_thresholds(self._h, arr, len(thresh), stream), "crn_sense_set_thresholds")
        for b, t in enumerate(arr):
            self.cfg.thresh[b] = t

    def set_ann(self, w_ih, w_ho, threshold=0.8, stream=0):
        """Replace the network of a DECIDE_ANN handle (ordered on `stream`); also updates self.cfg."""
        import numpy as np
        a, b = np.ascontiguousarray(w_ih, np.float64), np.ascontiguousarray(w_ho, np.float64)
        assert a.shape == (5, 6) and b.shape == (6, 4)
        check(lib().crn_sense_set_ann(self._h, a.ctypes.data, b.ctypes.data, threshold, C.c_void_p(stream or None)), "crn_sense_set_ann")
        set_ann_weights(self.cfg, a, b, threshold)

    def set_bands(self, segs, n_bands, thresh=None):
        """Replace the band plan of the live handle: segs = [(lo, hi, band), ..]; thresh = n_bands floats or None (keep)."""
        arr = (BandSeg * len(segs))(*[BandSeg(int(lo), int(hi), int(b)) for lo, hi, b in segs])
        th = None if thresh is None else (C.c_float * n_bands)(*[float(t) for t in thresh])
        check(lib().crn_sense_set_bands(self._h, arr, len(segs), n_bands, th), "crn_sense_set_bands")
        self.cfg.n_segs, self.cfg.n_bands = len(segs), n_bands
        for i, sg in enumerate(arr):
            self.cfg.segs[i] = sg
        if th is not None:
            for b in range(n_bands):
                self.cfg.thresh[b] = th[b]

    def reserve_noise_floor(self):
        check(lib().crn_sense_reserve_noise_floor(self._h), "crn_sense_reserve_noise_floor")

    def calibrate_thresholds(self, features, lam, stream=0):
        """Upload a numpy [n_epochs][n_bands] float32 matrix, estimate the noise floor, set every threshold to lam x it; returns the
        estimate and updates self.cfg."""
        import numpy as np
        f = np.ascontiguousarray(features, np.float32)
        nf = C.c_float()
        check(lib().crn_sense_calibrate_thresholds(self._h, f.ctypes.data, f.shape[0], lam, C.byref(nf), C.c_void_p(stream or None)),
              "crn_sense_calibrate_thresholds")
        for b in range(self.cfg.n_bands):
            self.cfg.thresh[b] = float(np.float32(lam) * np.float32(nf.value))
        return nf.value

    def noise_floor_host(self, features):
        """crn_noise_floor_host on a numpy [n_epochs][n_bands] float32 matrix."""
        import numpy as np
        f = np.ascontiguousarray(features, np.float32)
        nf = C.c_float()
        check(lib().crn_noise_floor_host(self._h, f.ctypes.data, f.shape[0], C.byref(nf)), "crn_noise_floor_host")
        return nf.value

    def set_timing(self, on=True):
        check(lib().crn_sense_set_timing(self._h, 1 if on else 0), "crn_sense_set_timing")

    def stats(self):
        st = SenseStats()
        check(lib().crn_sense_get_stats(self._h, C.byref(st)), "crn_sense_get_stats")
        return {k: getattr(st, k) for k, _ in SenseStats._fields_}

    def dealt_launches(self):
        """Launches of this handle that ran the dealt-frame form of the kernel (small launches at 512 / 1024 points)."""
        n = C.c_int64()
        check(lib().crn_sense_dealt_launches(self._h, C.byref(n)), "crn_sense_dealt_launches")
        return n.value

    def kernel_info(self):
        name = C.create_string_buffer(256)
        thr, lds, epb = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().crn_sense_kernel_info(self._h, name, 256, C.byref(thr), C.byref(lds), C.byref(epb)),
              "crn_sense_kernel_info")
        return {"name": name.value.decode(), "threads_per_block": thr.value, "lds_bytes": lds.value,
                "epochs_per_block": epb.value}

    def run_device(self, iq_ptr, n_epochs, L, out_ptrs, stream=0, epoch_stride=0, sc16=False):
        """iq_ptr / out_ptrs: raw device addresses (ints); out_ptrs keys are Out fields.  sc16: iq_ptr holds the radio's wire
        format (int16 pairs, 4 bytes per complex sample)."""
        o = Out(**{k: (v or None) for k, v in out_ptrs.items()})
        if sc16:
            _need_sc16("run_device(sc16=True)")
        fn = lib().crn_sense_run_device_sc16 if sc16 else lib().crn_sense_run_device
        check(fn(self._h, iq_ptr, n_epochs, L, epoch_stride, C.byref(o), C.c_void_p(stream or None)),
              "crn_sense_run_device_sc16" if sc16 else "crn_sense_run_device")

    def set_cfar(self, guard, train=16, alpha=None, min_bins=1, *, method="ca", rank=None):
        """Per-bin CFAR on (guard, train, alpha, min_bins), or off with set_cfar(None).  method: "ca" (cell averaging), "go" (greatest
        of), "so" (smallest of) or "os" (ordered statistic, the rank-th smallest of the 2 W cells; rank defaults to cfar_os_rank(train)).
        alpha defaults to cfar_alpha(1e-3, K, train, method, rank)."""
        if guard is None:
            check(lib().crn_sense_set_cfar(self._h, None), "crn_sense_set_cfar")
            return
        m = _cfar_method(method)
        if rank is None:
            rank = cfar_os_rank(train) if m == CFAR_OS else 0
        if alpha is None:
            alpha = cfar_alpha(1e-3, self.cfg.frames_per_epoch, train, method, rank)
        if m == CFAR_CA and rank == 0:
            q = CfarParams(guard=int(guard), train=int(train), min_bins=int(min_bins), reserved=0, alpha=float(alpha))
            check(lib().crn_sense_set_cfar(self._h, C.byref(q)), "crn_sense_set_cfar")
            return
        q = CfarParamsEx(method=m, guard=int(guard), train=int(train), min_bins=int(min_bins), rank=int(rank), reserved=0,
                         alpha=float(alpha))
        check(lib().crn_sense_set_cfar_ex(self._h, C.byref(q)), "crn_sense_set_cfar_ex")

    def get_cfar(self):
        """None while CFAR is off, else {"guard", "train", "alpha", "min_bins"}, plus "method" and "rank" for a method other than CA."""
        q, on = CfarParamsEx(), C.c_int32()
        check(lib().crn_sense_get_cfar_ex(self._h, C.byref(q), C.byref(on)), "crn_sense_get_cfar_ex")
        if not on.value:
            return None
        d = {"guard": q.guard, "train": q.train, "alpha": q.alpha, "min_bins": q.min_bins}
        if q.method != CFAR_CA:
            d.update(method={v: k for k, v in CFAR_METHODS.items()}[q.method], rank=q.rank)
        return d

    def run_device_cfar(self, iq_ptr, n_epochs, L, out_ptrs, mask_ptr=0, band_bins_ptr=0, stream=0, epoch_stride=0):
        """run_device plus the CFAR outputs: mask_ptr [n_epochs][fft_len / 32] uint32, band_bins_ptr [n_epochs][n_bands] int32 (device
        addresses, 0 = not wanted)."""
        o = Out(**{k: (v or None) for k, v in out_ptrs.items()})
        check(lib().crn_sense_run_device_cfar(self._h, iq_ptr, n_epochs, L, epoch_stride, C.byref(o), C.c_void_p(mask_ptr or None),
                                              C.c_void_p(band_bins_ptr or None), C.c_void_p(stream or None)), "crn_sense_run_device_cfar")

    def segments_device(self, mask_ptr, spectrum_ptr, n_epochs, epochs_ptr, segments_ptr=0, merge_gap=0, min_width=1, max_segments=16, stream=0):
        """Segments of n_epochs rows of a CFAR bin mask and the matching `spectrum` rows (device pointers): epochs_ptr [n_epochs]
        SEGMENT_EPOCH_DTYPE, segments_ptr [n_epochs][max_segments] SEGMENT_DTYPE or 0 for the headers alone.  Only enqueues."""
        q = SegmentParams(merge_gap=int(merge_gap), min_width=int(min_width), max_segments=int(max_segments), reserved=0)
        check(lib().crn_segments_device(self._h, C.c_void_p(mask_ptr or None), C.c_void_p(spectrum_ptr or None), n_epochs, C.byref(q),
                                        C.c_void_p(epochs_ptr or None), C.c_void_p(segments_ptr or None), C.c_void_p(stream or None)),
              "crn_segments_device")

    def tracks_device(self, epochs_ptr, segments_ptr, n_epochs, streams_ptr, tracks_ptr, workspace_ptr, workspace_bytes, track_of_ptr=0,
                      max_segments=16, epochs_per_stream=None, slack_bins=1, max_miss=0, min_epochs=1, max_tracks=64, stream=0):
        """Tracks from the two arrays segments_device wrote (device pointers): streams_ptr [n_streams] TRACK_STREAM_DTYPE, tracks_ptr
        [n_streams][max_tracks] TRACK_DTYPE, track_of_ptr [n_epochs][max_segments] int32 or 0, workspace_ptr at least
        tracks_workspace_bytes(...) of scratch; n_streams = n_epochs / epochs_per_stream (one stream when None).  Only enqueues."""
        q = track_params(max_segments, n_epochs if epochs_per_stream is None else epochs_per_stream, slack_bins, max_miss, min_epochs, max_tracks)
        check(lib().crn_tracks_device(self._h, C.c_void_p(epochs_ptr or None), C.c_void_p(segments_ptr or None), n_epochs, C.byref(q),
                                      C.c_void_p(streams_ptr or None), C.c_void_p(tracks_ptr or None), C.c_void_p(track_of_ptr or None),
                                      C.c_void_p(workspace_ptr or None), int(workspace_bytes), C.c_void_p(stream or None)),
              "crn_tracks_device")

    def tracks_carry_device(self, epochs_ptr, segments_ptr, n_epochs, t_start, carry_ptr, carry_bytes, streams_ptr, tracks_ptr, workspace_ptr,
                            workspace_bytes, open_ptr=0, flush=False, max_segments=16, epochs_per_stream=None, slack_bins=1, max_miss=0,
                            min_epochs=1, max_tracks=64, stream=0):
        """One call of a sequence that carries tracks across batches (device pointers): the epochs t_start .. t_start + epochs_per_stream - 1
        of every stream; t_start = 0 starts afresh.  carry_ptr: at least tracks_carry_bytes(n_streams, ...) that the caller keeps between
        calls; streams_ptr [n_streams] TRACK_CARRY_STREAM_DTYPE; tracks_ptr [n_streams][max_tracks] TRACK_DTYPE, the records this call
        closed; open_ptr the same shape or 0, the tracks still open; workspace_ptr at least tracks_carry_workspace_bytes(...) of scratch;
        flush closes everything.  Only enqueues."""
        q = track_params(max_segments, n_epochs if epochs_per_stream is None else epochs_per_stream, slack_bins, max_miss, min_epochs, max_tracks)
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_tracks_carry_device(self._h, v(epochs_ptr), v(segments_ptr), n_epochs, C.byref(q), int(t_start), int(bool(flush)),
                                            v(carry_ptr), carry_bytes, v(streams_ptr), v(tracks_ptr), v(open_ptr), v(workspace_ptr),
                                            workspace_bytes, v(stream)),
              "crn_tracks_carry_device")

    def channels_device(self, mask_ptr, spectrum_ptr, n_epochs, stats_ptr, workspace_ptr, workspace_bytes, spans, epochs_per_stream=None,
                        min_bins=1, first=False, busy_ptr=0, power_ptr=0, stream=0):
        """Per-channel occupancy records from n_epochs rows of a CFAR bin mask and, unless spectrum_ptr is 0, the matching `spectrum` rows
        (device pointers): stats_ptr [n_streams][len(spans)] CHANNEL_STATS_DTYPE, read (unless `first`) and rewritten; busy_ptr [n_epochs]
        uint64 or 0; power_ptr [n_epochs][len(spans)] float32 or 0; workspace_ptr at least channels_workspace_bytes(...) of scratch;
        n_streams = n_epochs / epochs_per_stream (one stream when None).  Only enqueues."""
        q = channel_params(spans, n_epochs if epochs_per_stream is None else epochs_per_stream, min_bins, first)
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_channels_device(self._h, v(mask_ptr), v(spectrum_ptr), n_epochs, C.byref(q), v(stats_ptr), v(busy_ptr), v(power_ptr),
                                        v(workspace_ptr), int(workspace_bytes), v(stream)), "crn_channels_device")

    def holes_device(self, mask_ptr, spectrum_ptr, n_epochs, age_ptr, streams_ptr, workspace_ptr, workspace_bytes, params, holes_ptr=0,
                     free_mask_ptr=0, stream=0):
        """Spectrum holes with idle age from n_epochs rows of a CFAR bin mask and, unless spectrum_ptr is 0, the matching `spectrum` rows
        (device pointers; params from hole_params): age_ptr [n_streams][fft_len] int32, the carry, read (unless params.first) and
        rewritten; streams_ptr [n_streams] HOLE_STREAM_DTYPE; holes_ptr [n_streams][params.max_holes] HOLE_DTYPE or 0; free_mask_ptr
        [n_streams][fft_len / 32] uint32 or 0; workspace_ptr at least holes_workspace_bytes(...) of scratch;
        n_streams = n_epochs / params.epochs_per_stream.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_holes_device(self._h, v(mask_ptr), v(spectrum_ptr), n_epochs, C.byref(params), v(age_ptr), v(streams_ptr), v(holes_ptr),
                                     v(free_mask_ptr), v(workspace_ptr), int(workspace_bytes), v(stream)), "crn_holes_device")

    def lad_device(self, spectrum_ptr, n_epochs, params, mask_ptr=0, rows_ptr=0, floor_ptr=0, or_mask_ptr=0, stream=None):
        """Wideband detection against an excised noise floor on n_epochs `spectrum` rows (device pointers; params from lad_params):
        mask_ptr [n_epochs][fft_len / 32] uint32, the CFAR mask's layout; rows_ptr [n_epochs] LAD_ROW_DTYPE; floor_ptr
        [n_epochs][params.n_blocks] float32; each or 0, not all three.  or_mask_ptr: a mask of the same layout OR-ed into the output (the
        CFAR mask of the same launch; it may be mask_ptr itself), or 0.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_lad_device(self._h, v(spectrum_ptr), n_epochs, C.byref(params), v(or_mask_ptr), v(mask_ptr), v(rows_ptr), v(floor_ptr),
                                   v(stream)), "crn_lad_device")

    def tcfar_device(self, spectrum_ptr, n_epochs, params, hist_ptr, seen_ptr, mask_ptr=0, rows_ptr=0, or_mask_ptr=0, stream=None):
        """Ordered-statistic CFAR along time on n_epochs `spectrum` rows (device pointers; params from tcfar_params): hist_ptr
        tcfar_hist_bytes(...) of float32 and seen_ptr [n_streams] int64, the carry, read (unless params.first) and rewritten; mask_ptr
        [n_epochs][fft_len / 32] uint32, the CFAR mask's layout, or 0; rows_ptr [n_epochs] TCFAR_ROW_DTYPE or 0 (both 0: the call only
        feeds the history); or_mask_ptr: a mask of the same layout OR-ed into the output (the CFAR or LAD mask of the same rows; it may be
        mask_ptr itself), or 0.  n_streams = n_epochs / params.epochs_per_stream.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_tcfar_device(self._h, v(spectrum_ptr), n_epochs, C.byref(params), v(or_mask_ptr), v(mask_ptr), v(rows_ptr), v(hist_ptr),
                                     v(seen_ptr), v(stream)), "crn_tcfar_device")

    def measure_device(self, spectrum_ptr, n_epochs, params, epochs_ptr, segments_ptr, measures_ptr, stream=None):
        """Occupied bandwidth, x-dB bandwidth and shape of every stored segment of n_epochs rows (device pointers; params from
        measure_params): spectrum_ptr [n_epochs][fft_len] float32, epochs_ptr and segments_ptr what segments_device wrote with the same
        max_segments, measures_ptr [n_epochs][max_segments] MEASURE_DTYPE, every slot written.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_measure_device(self._h, v(spectrum_ptr), n_epochs, C.byref(params), v(epochs_ptr), v(segments_ptr), v(measures_ptr),
                                       v(stream)), "crn_measure_device")

    def occmap_device(self, mask_ptr, spectrum_ptr, n_epochs, bins_ptr, streams_ptr, workspace_ptr, workspace_bytes, epochs_per_stream=None,
                      duty=0.5, first=False, usual_mask_ptr=0, stream=None):
        """The occupancy map of n_epochs rows of a CFAR bin mask and, unless spectrum_ptr is 0, the matching `spectrum` rows (device
        pointers): bins_ptr [n_streams][fft_len] OCCMAP_BIN_DTYPE, read unless first and then rewritten; streams_ptr [n_streams]
        OCCMAP_STREAM_DTYPE; usual_mask_ptr [n_streams][fft_len / 32] uint32 or 0, the bins busy in at least `duty` of their epochs;
        workspace_ptr at least occmap_workspace_bytes(...) of scratch.  One stream unless epochs_per_stream is given.  Only enqueues."""
        q = occmap_params(n_epochs if epochs_per_stream is None else epochs_per_stream, duty, first)
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_occmap_device(self._h, v(mask_ptr), v(spectrum_ptr), n_epochs, C.byref(q), v(bins_ptr), v(streams_ptr), v(usual_mask_ptr),
                                      v(workspace_ptr), int(workspace_bytes), v(stream)), "crn_occmap_device")

    def hops_device(self, busy_ptr, n_epochs, params, records_ptr, record_bytes, workspace_ptr, workspace_bytes, stream=None):
        """Channel-to-channel transition counts from n_epochs busy words (device pointers; params from hop_params): busy_ptr [n_epochs]
        uint64 as channels_device writes them; records_ptr hops_bytes(...) of records, one per stream (hop_record), read unless
        params.first and then rewritten; workspace_ptr at least hops_workspace_bytes(...) of scratch.  n_streams = n_epochs /
        params.epochs_per_stream.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_hops_device(self._h, v(busy_ptr), n_epochs, C.byref(params), v(records_ptr), int(record_bytes), v(workspace_ptr),
                                    int(workspace_bytes), v(stream)), "crn_hops_device")

    def extract_device(self, spectra_ptr, n_frames, params, channels_ptr, n_chan, taper_ptr, out_ptr, stream=0):
        """Baseband sample streams of n_chan channels (device pointers; params from extract_params): spectra_ptr [n_frames][fft_len]
        complex float32, what fft_forward_device writes with frame_stride = fft_len / 2; channels_ptr [n_chan] EXTRACT_CHANNEL_DTYPE;
        taper_ptr [out_len] float32 (extract_taper); out_ptr [n_chan][frames_per_stream out_len / 2] complex float32, every sample
        written, at extract_rate(fs, fft_len, out_len).  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_extract_device(self._h, v(spectra_ptr), n_frames, C.byref(params), v(channels_ptr), int(n_chan), v(taper_ptr), v(out_ptr),
                                       v(stream)), "crn_extract_device")

    def resample_device(self, in_ptr, n_rows, params, rows_ptr, taps_ptr, state_ptr, out_ptr, stream=0):
        """n_rows sample streams resampled and mixed (device pointers; params from resample_params): in_ptr [n_rows][in_len] complex
        float32, the rows extract_device writes as they are; rows_ptr [n_rows] RESAMPLE_ROW_DTYPE (resample_rows); taps_ptr
        [phases + 1][taps] float32 (resample_taps); state_ptr resample_state_bytes(n_rows) of RESAMPLE_STATE_DTYPE, read unless
        params.first and then rewritten; out_ptr [n_rows][out_cap] complex float32, every sample written, of which the state's
        last_n_out are outputs.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_resample_device(self._h, v(in_ptr), int(n_rows), C.byref(params), v(rows_ptr), v(taps_ptr), v(state_ptr), v(out_ptr),
                                        v(stream)), "crn_resample_device")

    def cyclo_device(self, frames_ptr, n_epochs, params, epochs_ptr, segments_ptr, cyclo_ptr, profile_ptr=0, stream=0):
        """The strongest cyclic feature of every stored segment of n_epochs epochs (device pointers; params from cyclo_params): frames_ptr
        [n_epochs][params.frames][fft_len] complex float32, what fft_forward_device writes for the epochs' frames; epochs_ptr and
        segments_ptr what segments_device wrote with the same max_segments; cyclo_ptr [n_epochs][max_segments] CYCLO_DTYPE, every slot
        written; profile_ptr [n_epochs][max_segments][n_a][frames] float32 or 0.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_cyclo_device(self._h, v(frames_ptr), n_epochs, C.byref(params), v(epochs_ptr), v(segments_ptr), v(cyclo_ptr),
                                     v(profile_ptr), v(stream)), "crn_cyclo_device")

    def fuse_device(self, mask_ptr, spectrum_ptr, n_epochs, params, fused_mask_ptr=0, fused_spectrum_ptr=0, rows_ptr=0, stream=0):
        """Fuses groups of params.group_size streams (fuse_params; device pointers): mask_ptr [n_epochs][fft_len / 32] uint32 and
        spectrum_ptr [n_epochs][fft_len] float32, either 0 where the rule does not need it; fused_mask_ptr and fused_spectrum_ptr the same
        shapes with n_epochs / group_size rows, rows_ptr [n_epochs / group_size] FUSE_ROW_DTYPE, each or 0.  Only enqueues."""
        v = lambda ptr: C.c_void_p(ptr or None)      # noqa: E731
        check(lib().crn_fuse_device(self._h, v(mask_ptr), v(spectrum_ptr), n_epochs, C.byref(params), v(fused_mask_ptr), v(fused_spectrum_ptr),
                                    v(rows_ptr), v(stream)), "crn_fuse_device")

    def set_wire_full_scale(self, full_scale):
        _need_sc16("set_wire_full_scale")
        check(lib().crn_sense_set_wire_full_scale(self._h, float(full_scale)), "crn_sense_set_wire_full_scale")

    def pack_sc16_device(self, iq_ptr, n_samples, out_ptr, stream=0):
        """complex floats -> int16 pairs on the device (n_samples complex samples)."""
        _need_sc16("pack_sc16_device")
        check(lib().crn_pack_sc16_device(self._h, iq_ptr, n_samples, out_ptr, C.c_void_p(stream or None)), "crn_pack_sc16_device")

    def run_host(self, iq, n_epochs, L=None, want_spectrum=False, epoch_stride=0):
        """iq: numpy float32 array of interleaved samples. Returns dict of numpy outputs."""
        import numpy as np
        cfg = self.cfg
        L = cfg.fft_len if L is None else L
        iq = np.ascontiguousarray(iq, dtype=np.float32)
        res = {
            "features": np.zeros((n_epochs, cfg.n_bands), np.float32),
            "ann_out": np.zeros((n_epochs, 3), np.float64),
            "decision": np.zeros((n_epochs,), np.int32),
            "occupancy": np.zeros((n_epochs, cfg.n_bands), np.uint8),
        }
        if want_spectrum:
            res["spectrum"] = np.zeros((n_epochs, cfg.fft_len), np.float32)
        o = Out(**{k: v.ctypes.data for k, v in res.items()})
        check(lib().crn_sense_run_host(self._h, iq.ctypes.data, n_epochs, L, epoch_stride, C.byref(o)),
              "crn_sense_run_host")
        return res

    def synth_fill_device(self, iq_ptr, n_epochs, spe, seed, noise_power=1e-6, signal_rms=0.02,
                          tones=8, truth_ptr=0, stream=0):
        check(lib().crn_synth_fill_device(self._h, iq_ptr, n_epochs, spe, seed, noise_power, signal_rms,
                                          tones, C.c_void_p(truth_ptr or None), C.c_void_p(stream or None)),
              "crn_synth_fill_device")

    def synth_fill_device_ex(self, iq_ptr, n_epochs, spe, sc, truth_ptr=0, stream=0):
        """sc: SynthCfg (traffic model, signal kind, streams)."""
        check(lib().crn_synth_fill_device_ex(self._h, C.byref(sc), iq_ptr, n_epochs, spe,
                                             C.c_void_p(truth_ptr or None), C.c_void_p(stream or None)),
              "crn_synth_fill_device_ex")

    def fft_forward_device(self, in_ptr, n_frames, L, out_ptr, frame_stride=0, stream=0):
        """Unnormalised forward DFT of n_frames frames (device pointers)."""
        check(lib().crn_fft_forward_device(self._h, in_ptr, n_frames, L, frame_stride, out_ptr,
                                           C.c_void_p(stream or None)), "crn_fft_forward_device")

    def monitor_rows_device(self, spec_ptr, n_rows, kind, alpha, first, state_ptr, waterfall_ptr=0, average_ptr=0, stream=0):
        """fftshifted dB rows + IIR-averaged trace from rows of the `spectrum` output (device pointers)."""
        check(lib().crn_monitor_rows_device(self._h, spec_ptr, n_rows, kind, alpha, int(first), state_ptr,
                                            C.c_void_p(waterfall_ptr or None), C.c_void_p(average_ptr or None),
                                            C.c_void_p(stream or None)), "crn_monitor_rows_device")

    def ann_train_device(self, tc, feat_ptr, label_ptr, n, stream=0):
        """Fit the 4-5-3 network to device-resident features/labels; returns (w_ih, w_ho, loss)."""
        import numpy as np
        wih, who = np.zeros((5, 6), np.float64), np.zeros((6, 4), np.float64)
        loss = C.c_double()
        check(lib().crn_ann_train_device(self._h, C.byref(tc), feat_ptr, label_ptr, n, wih.ctypes.data,
                                         who.ctypes.data, C.byref(loss), C.c_void_p(stream or None)),
              "crn_ann_train_device")
        return wih, who, loss.value


def set_ann_weights(cfg, w_ih, w_ho, threshold=0.8):
    """Put trained weights into a crn_cfg and select the ANN + cascade decision."""
    for i in range(5):
        for j in range(6):
            cfg.ann_w_ih[i][j] = float(w_ih[i][j])
    for j in range(6):
        for k in range(4):
            cfg.ann_w_ho[j][k] = float(w_ho[j][k])
    cfg.ann_threshold = threshold
    cfg.decide = DECIDE_ANN
    return cfg


COMM_ID_BYTES = 128

_hip = None


def device_to_host(ptr, nbytes):
    """Blocking copy of device memory at raw address `ptr` into a bytes object (plumbing for checks)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    buf = (C.c_uint8 * nbytes)()
    rc = _hip.hipMemcpy(buf, C.c_void_p(ptr), nbytes, 2)  # hipMemcpyDeviceToHost
    if rc != 0:
        raise CrnError(f"hipMemcpy D2H failed ({rc})")
    return bytes(buf)


def comm_unique_id():
    """bytes(128): call on rank 0, hand to the other ranks out of band."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    check(lib().crn_comm_unique_id(buf), "crn_comm_unique_id")
    return bytes(buf)


class Comm:
    """The occupancy exchange over RCCL (crn_comm_* in include/crn_sense.h): `depth` slots of
    bytes_per_rank on `device`, all-gathers queued on a side stream."""

    def __init__(self, device, rank, world, unique_id, bytes_per_rank, depth=2):
        self.rank, self.world, self.bytes, self.depth = rank, world, bytes_per_rank, depth
        self._c = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        check(lib().crn_comm_create(device, rank, world, buf, bytes_per_rank, depth, C.byref(self._c)), "crn_comm_create")

    def local(self, step, stream=0):
        p = C.c_void_p()
        check(lib().crn_comm_local(self._c, step, C.c_void_p(stream or None), C.byref(p)), "crn_comm_local")
        return p.value

    def local_addr(self, step):
        """The slot's address, without making any stream wait or releasing the slot."""
        p = C.c_void_p()
        check(lib().crn_comm_local_addr(self._c, step, C.byref(p)), "crn_comm_local_addr")
        return p.value

    def wait(self, step, stream=0):
        """Make `stream` wait for step's gather only; the slot stays in flight for local() / finish()."""
        check(lib().crn_comm_wait(self._c, step, C.c_void_p(stream or None)), "crn_comm_wait")

    def allgather(self, step, stream=0):
        check(lib().crn_comm_allgather(self._c, step, C.c_void_p(stream or None)), "crn_comm_allgather")

    def gathered(self, step):
        p = C.c_void_p()
        check(lib().crn_comm_gathered(self._c, step, C.byref(p)), "crn_comm_gathered")
        return p.value

    def finish(self, stream=0):
        check(lib().crn_comm_finish(self._c, C.c_void_p(stream or None)), "crn_comm_finish")

    def info(self):
        """What RCCL says the communicator is (ncclCommCount / UserRank / CuDevice / GetVersion), as a dict."""
        ci = CommInfo()
        check(lib().crn_comm_info(self._c, C.byref(ci)), "crn_comm_info")
        return {"nranks": ci.nranks, "rank": ci.rank, "rccl_device": ci.rccl_device, "rccl_version": ci.rccl_version,
                "device": ci.device, "depth": ci.depth, "bytes_per_rank": ci.bytes_per_rank, "gathers": ci.gathers,
                "library": ci.library.decode(errors="replace"), "pci_bus_id": ci.pci_bus_id.decode(errors="replace")}

    def close(self):
        if self._c:
            lib().crn_comm_destroy(self._c)
            self._c = C.c_void_p()


class Ingest:
    """Packet ingest ring over a Sensor (crn_ingest_* in include/crn_sense.h)."""

    def __init__(self, sensor, n_streams, samples_per_packet, epochs_per_batch, sc16=False):
        """sc16: packets are int16 pairs (the radio's wire format) instead of complex floats."""
        self.sensor = sensor
        self._g = C.c_void_p()
        if sc16:
            _need_sc16("Ingest(sc16=True)")
        self._push = lib().crn_ingest_push_sc16 if sc16 else lib().crn_ingest_push
        create = lib().crn_ingest_create_sc16 if sc16 else lib().crn_ingest_create
        check(create(sensor._h, n_streams, samples_per_packet, epochs_per_batch, C.byref(self._g)), "crn_ingest_create")
        sensor._rings.add(self)

    def calibrate(self, n_epochs, lam):
        """Post a noise-floor calibration over the next n_epochs epochs (carried out by the ring's launcher thread)."""
        check(lib().crn_ingest_calibrate(self._g, n_epochs, lam), "crn_ingest_calibrate")

    def noise_floor(self):
        """(estimate in force, calibration collecting?)"""
        nf, busy = C.c_float(), C.c_int32()
        check(lib().crn_ingest_noise_floor(self._g, C.byref(nf), C.byref(busy)), "crn_ingest_noise_floor")
        return nf.value, bool(busy.value)

    def push(self, stream, packet, block=True):
        """block=True: on CRN_ERR_BUSY wait for a free buffer and push again (tests, tools);
        block=False: returns False when the packet was refused (what an engine's execute() does)."""
        rc = self._push(self._g, stream, packet.ctypes.data)
        while rc == CRN_ERR_BUSY and block:
            check(lib().crn_ingest_wait(self._g), "crn_ingest_wait")
            rc = self._push(self._g, stream, packet.ctypes.data)
        if rc == CRN_ERR_BUSY:
            return False
        check(rc, "crn_ingest_push")
        return True

    def set_packet_len(self, L):
        check(lib().crn_ingest_set_packet_len(self._g, L), "crn_ingest_set_packet_len")

    def stats(self):
        st = IngestStats()
        check(lib().crn_ingest_get_stats(self._g, C.byref(st)), "crn_ingest_get_stats")
        return {k: getattr(st, k) for k, _ in IngestStats._fields_}

    def packets_per_epoch(self):
        n = C.c_int32()
        check(lib().crn_ingest_packets_per_epoch(self._g, C.byref(n)), "crn_ingest_packets_per_epoch")
        return n.value

    def dropped(self):
        n = C.c_int64()
        check(lib().crn_ingest_dropped(self._g, C.byref(n)), "crn_ingest_dropped")
        return n.value

    def flush(self):
        check(lib().crn_ingest_flush(self._g), "crn_ingest_flush")

    def drain(self):
        check(lib().crn_ingest_drain(self._g), "crn_ingest_drain")

    def poll(self, max_results=64):
        arr = (EpochResult * max_results)()
        n = C.c_int32()
        check(lib().crn_ingest_poll(self._g, arr, max_results, C.byref(n)), "crn_ingest_poll")
        return [arr[i] for i in range(n.value)]

    def close(self):
        if self._g:
            lib().crn_ingest_destroy(self._g)
            self._g = C.c_void_p()
            self.sensor._rings.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
