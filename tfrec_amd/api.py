"""ctypes binding of the C ABI in include/tfrec_amd.h.

The product is the HIP library ``libtfrec_amd.so``; this module only loads it, marshals arguments and
exposes the events as numpy records.  There is NO CPU fallback: if the library is missing or no GPU is
present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from fractions import Fraction

import numpy as np

from . import _build
from .burst import BURST_DTYPE  # tfrec_amd_burst
from .capture import RUN_DTYPE  # tfrec_amd_run
from .clock import CLOCK_DTYPE  # tfrec_amd_clock
from .crc import CRC_DTYPE  # tfrec_amd_burst_crc
from .envelope import ENVELOPE_DTYPE  # tfrec_amd_envelope
from .levels import LEVEL_DTYPE  # tfrec_amd_level
from .occupancy import OCC_DTYPE  # tfrec_amd_occupancy
from .sync import SYNC_DTYPE  # tfrec_amd_burst_sync
from .track import TRACK_DTYPE  # tfrec_amd_track

BLOCK_BYTES = 65536
BLOCK_DEC = 8192
NSLOTS = 5
FIFO_DEPTH = 4  # TFREC_AMD_FIFO_DEPTH
SLOT_NAMES = ("TFA_1", "TFA_2", "TFA_3", "TX22", "WHB")

F_ALL_FLUSHES = 1
F_TIMING = 2
F_SERIAL_CHAINS = 4
F_INPUT_10X = 8
F_BITS = 16
F_LEVELS = 32
STATUS_BITS = 0x80

E_OK, E_INVAL, E_NOMEM, E_HIP, E_OVERFLOW, E_STATE = 0, -1, -2, -3, -4, -5


class TfrecAmdError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("tfrec_amd error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("n_streams", C.c_int32),
        ("types_mask", C.c_int32),
        ("thresh", C.c_int32),
        ("filter_type", C.c_int32),
        ("device", C.c_int32),
        ("max_blocks", C.c_int32),
        ("max_events", C.c_int32),
        ("flags", C.c_uint32),
    ]


class Timings(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("frontend_ms", "chains_ms", "total_ms", "windows_ms", "spec_biquad_ms",
                                         "repair_biquad_ms", "fix_biquad_ms", "slicer_ms", "coop_slicer_ms", "decode_ms",
                                         "commit_ms", "whb_biquad_ms", "whb_demod_ms", "whb_decode_ms", "whb_commit_ms",
                                         "tfa1_slicer_ms", "tfa1_coop_slicer_ms", "tfa1_decode_commit_ms", "fmdev_ms",
                                         "whb_verify_ms")]


class Stats(C.Structure):
    _fields_ = [("biquad_segments", C.c_uint64), ("biquad_unconverged", C.c_uint64), ("biquad_serial", C.c_uint64),
                ("tfa2_resliced", C.c_uint64), ("tfa1_recomputed", C.c_uint64), ("biquad_repair_slots", C.c_uint64),
                ("whb_respeculated", C.c_uint64), ("tfa1_scalar_groups", C.c_uint64), ("tfa2_scalar_groups", C.c_uint64),
                ("tfa1_vector_groups", C.c_uint64), ("tfa2_vector_groups", C.c_uint64)]


class StreamConfig(C.Structure):
    """tfrec_amd_stream_config: one stream's -T, -t and -W (tfrec_amd_configure_streams)."""
    _fields_ = [("types_mask", C.c_int32), ("thresh", C.c_int32), ("filter_type", C.c_int32), ("reserved", C.c_int32)]


class FmStats(C.Structure):
    _fields_ = [("resolved", C.c_uint64), ("host_verified", C.c_uint64), ("host_mismatch", C.c_uint64),
                ("undecidable", C.c_uint64), ("reserved", C.c_uint64 * 4)]


EVENT_DTYPE = np.dtype(
    [
        ("stream", "<u4"),
        ("slot", "u1"),
        ("status", "u1"),
        ("byte_cnt", "<u2"),
        ("offset", "<i4"),
        ("seq", "<u4"),
        ("end_sample", "<i8"),
        ("rssi_raw", "<i8"),
        ("rdata", "u1", (64,)),
    ]
)
assert EVENT_DTYPE.itemsize == 96

# every symbol include/tfrec_amd.h declares
EXPORTS = (
    "tfrec_amd_version", "tfrec_amd_strerror", "tfrec_amd_last_error", "tfrec_amd_create", "tfrec_amd_destroy",
    "tfrec_amd_submit_device", "tfrec_amd_submit_host", "tfrec_amd_sync", "tfrec_amd_drain_events",
    "tfrec_amd_pending_events", "tfrec_amd_rssi_db", "tfrec_amd_read_decimated", "tfrec_amd_atan_uncertain",
    "tfrec_amd_get_timings", "tfrec_amd_read_thresh", "tfrec_amd_get_stats", "tfrec_amd_get_layout", "tfrec_amd_host_alloc",
    "tfrec_amd_host_free", "tfrec_amd_read_stage0", "tfrec_amd_get_fm_stats", "tfrec_amd_fm_dev_probe",
    "tfrec_amd_fifo_depth", "tfrec_amd_get_memory", "tfrec_amd_iir_probe", "tfrec_amd_reset_streams",
    "tfrec_amd_configure_streams", "tfrec_amd_get_stream_config", "tfrec_amd_tune_streams", "tfrec_amd_get_stream_tune",
    "tfrec_amd_map_streams", "tfrec_amd_get_stream_input", "tfrec_amd_tune_streams_wide", "tfrec_amd_get_stream_tune_wide",
    "tfrec_amd_create_rate", "tfrec_amd_get_input_rate", "tfrec_amd_input_bytes", "tfrec_amd_resample_taps",
    "tfrec_amd_tune_streams_input", "tfrec_amd_get_stream_tune_input", "tfrec_amd_create_format", "tfrec_amd_get_input_format",
    "tfrec_amd_read_levels", "tfrec_amd_enable_capture", "tfrec_amd_read_captures", "tfrec_amd_enable_spectrum",
    "tfrec_amd_read_spectrum", "tfrec_amd_enable_occupancy", "tfrec_amd_read_occupancy", "tfrec_amd_create_dc", "tfrec_amd_get_dc",
    "tfrec_amd_read_dc", "tfrec_amd_reset_dc_rows", "tfrec_amd_create_iq", "tfrec_amd_get_iq", "tfrec_amd_read_iq", "tfrec_amd_reset_iq_rows", "tfrec_amd_create_decimated", "tfrec_amd_enable_capture_pre",
    "tfrec_amd_read_capture_pre", "tfrec_amd_enable_runs_input", "tfrec_amd_submit_runs", "tfrec_amd_read_biquad_row",
    "tfrec_amd_enable_burst_meter", "tfrec_amd_read_bursts", "tfrec_amd_stream_state_bytes", "tfrec_amd_save_streams",
    "tfrec_amd_load_streams", "tfrec_amd_enable_burst_envelope", "tfrec_amd_read_burst_envelopes",
    "tfrec_amd_enable_burst_clock", "tfrec_amd_read_burst_clocks",
    "tfrec_amd_enable_burst_track", "tfrec_amd_set_burst_track_centre", "tfrec_amd_read_burst_tracks",
    "tfrec_amd_enable_burst_track_amplitude", "tfrec_amd_set_burst_track_level",
    "tfrec_amd_enable_burst_track_auto", "tfrec_amd_read_burst_track_centres", "tfrec_amd_enable_burst_track_phase",
    "tfrec_amd_enable_burst_sync", "tfrec_amd_read_burst_syncs",
    "tfrec_amd_enable_burst_code", "tfrec_amd_read_burst_codes",
    "tfrec_amd_enable_burst_crc", "tfrec_amd_read_burst_crcs",
)

_libs = {}


def library_path(experiments: bool = False, short_segments: bool = False) -> str:
    return _build.VARIANTS[_build.variant_name(experiments, short_segments)][0]


def load_library(build: bool = True, experiments: bool = False, short_segments: bool = False):
    """Load libtfrec_amd.so -- or, experiments=True, libtfrec_amd_exp.so: the same sources with the environment knobs and
    test hooks compiled in (csrc/knobs.h); or, short_segments=True, libtfrec_amd_seg.so: that build with biquad segments of
    _build.SEG_SLOTS slots -- building it in-tree first when hipcc is available.  Raises if absent."""
    key = _build.variant_name(experiments, short_segments)
    if key in _libs:
        return _libs[key]
    if build:
        try:
            _build.build_device_lib(experiments=bool(experiments), short_segments=bool(short_segments))
        except (OSError, FileNotFoundError):
            pass  # no hipcc on this box: use the prebuilt library that travelled with the tree
    lib_so = library_path(experiments, short_segments)
    if key == "experiments":
        lib_so = os.environ.get("TFREC_AMD_LIB", lib_so)  # (A/B sessions: an alternative experiments build)
    if not os.path.exists(lib_so):
        raise RuntimeError("HIP extension %s is missing: run __graft_entry__.build()" % lib_so)
    # One HIP runtime per process: PyTorch bundles its own libamdhip64.so.7; importing torch first makes our
    # library bind to that same copy (same SONAME) instead of loading /opt/rocm's next to it, which would
    # leave whichever runtime comes second without a GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(lib_so)
    L.tfrec_amd_version.restype = C.c_char_p
    L.tfrec_amd_strerror.restype = C.c_char_p
    L.tfrec_amd_strerror.argtypes = [C.c_int]
    L.tfrec_amd_last_error.restype = C.c_char_p
    L.tfrec_amd_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.tfrec_amd_destroy.argtypes = [C.c_void_p]
    L.tfrec_amd_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.tfrec_amd_submit_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.tfrec_amd_sync.argtypes = [C.c_void_p]
    L.tfrec_amd_drain_events.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.tfrec_amd_pending_events.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.tfrec_amd_rssi_db.argtypes = [C.c_int, C.c_int64]
    L.tfrec_amd_rssi_db.restype = C.c_int
    L.tfrec_amd_read_decimated.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.tfrec_amd_read_stage0.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.tfrec_amd_read_biquad_row.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.tfrec_amd_atan_uncertain.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.tfrec_amd_get_timings.argtypes = [C.c_void_p, C.POINTER(Timings)]
    L.tfrec_amd_read_thresh.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.tfrec_amd_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.tfrec_amd_get_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.tfrec_amd_get_memory.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.tfrec_amd_get_fm_stats.argtypes = [C.c_void_p, C.POINTER(FmStats)]
    L.tfrec_amd_fm_dev_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(FmStats)]
    L.tfrec_amd_iir_probe.argtypes = [C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.tfrec_amd_reset_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_configure_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_get_stream_config.argtypes = [C.c_void_p, C.c_int, C.POINTER(StreamConfig)]
    L.tfrec_amd_tune_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_get_stream_tune.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.tfrec_amd_map_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_get_stream_input.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.tfrec_amd_tune_streams_wide.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_get_stream_tune_wide.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.tfrec_amd_tune_streams_input.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_get_stream_tune_input.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]
    L.tfrec_amd_create_rate.argtypes = [C.POINTER(Config), C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.tfrec_amd_get_input_rate.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.tfrec_amd_input_bytes.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    L.tfrec_amd_resample_taps.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.tfrec_amd_create_format.argtypes = [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.tfrec_amd_get_input_format.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.tfrec_amd_read_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    L.tfrec_amd_enable_capture.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.tfrec_amd_read_captures.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t,
                                          C.POINTER(C.c_uint64)]
    L.tfrec_amd_enable_spectrum.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    L.tfrec_amd_read_spectrum.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_int)]
    L.tfrec_amd_enable_occupancy.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.tfrec_amd_read_occupancy.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    L.tfrec_amd_create_dc.argtypes = [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.tfrec_amd_get_dc.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.tfrec_amd_read_dc.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    L.tfrec_amd_reset_dc_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_create_iq.argtypes = [C.POINTER(Config), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.tfrec_amd_get_iq.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.tfrec_amd_read_iq.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
    L.tfrec_amd_reset_iq_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_create_decimated.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.tfrec_amd_enable_capture_pre.argtypes = [C.c_void_p]
    L.tfrec_amd_read_capture_pre.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.tfrec_amd_enable_runs_input.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.tfrec_amd_submit_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int]
    L.tfrec_amd_enable_burst_meter.argtypes = [C.c_void_p]
    L.tfrec_amd_read_bursts.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.tfrec_amd_enable_burst_envelope.argtypes = [C.c_void_p]
    L.tfrec_amd_read_burst_envelopes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.tfrec_amd_enable_burst_clock.argtypes = [C.c_void_p]
    L.tfrec_amd_read_burst_clocks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.tfrec_amd_enable_burst_track.argtypes = [C.c_void_p, C.c_int32]
    L.tfrec_amd_set_burst_track_centre.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_enable_burst_track_amplitude.argtypes = [C.c_void_p, C.c_int32]
    L.tfrec_amd_set_burst_track_level.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.tfrec_amd_enable_burst_track_auto.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.tfrec_amd_read_burst_track_centres.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]
    L.tfrec_amd_enable_burst_track_phase.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    L.tfrec_amd_read_burst_tracks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t,
                                              C.POINTER(C.c_uint64)]
    L.tfrec_amd_enable_burst_sync.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_uint32]
    L.tfrec_amd_read_burst_syncs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t,
                                             C.POINTER(C.c_uint64)]
    L.tfrec_amd_enable_burst_code.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32]
    L.tfrec_amd_read_burst_codes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t,
                                             C.POINTER(C.c_uint64)]
    L.tfrec_amd_enable_burst_crc.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32]
    L.tfrec_amd_read_burst_crcs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t,
                                            C.POINTER(C.c_uint64)]
    L.tfrec_amd_stream_state_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.tfrec_amd_save_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.tfrec_amd_load_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.tfrec_amd_fifo_depth.restype = C.c_int
    if L.tfrec_amd_fifo_depth() != FIFO_DEPTH:
        raise RuntimeError("libtfrec_amd.so was built with FIFO depth %d, this binding expects %d" % (
            L.tfrec_amd_fifo_depth(), FIFO_DEPTH))
    _libs[key] = L
    return L


def _check(L, rc: int, ok=(E_OK,)):
    if rc not in ok:
        detail = L.tfrec_amd_last_error().decode() if rc == E_HIP or rc == E_INVAL or rc == E_NOMEM else ""
        raise TfrecAmdError(rc, L.tfrec_amd_strerror(rc).decode() + (" (" + detail + ")" if detail else ""))
    return rc


def resample_taps(p: int, q: int) -> np.ndarray:
    """The library's tap table of the input rate 1536000 P / Q (tfrec_amd_resample_taps) as int32 [Q, T]; TfrecAmdError(E_INVAL) for
    a rate outside the rules or refused by them.  Needs no GPU.  (tfrec_amd/resample.py: taps is the independent restatement.)"""
    L = load_library()
    if not all(-2 ** 31 <= int(v) < 2 ** 31 for v in (p, q)):
        raise TfrecAmdError(E_INVAL, "rate outside int32")
    t = C.c_int(0)
    _check(L, L.tfrec_amd_resample_taps(int(p), int(q), None, 0, C.byref(t)))
    out = np.empty((int(q), t.value), dtype=np.int32)
    _check(L, L.tfrec_amd_resample_taps(int(p), int(q), out.ctypes.data, out.size, C.byref(t)))
    return out


def rssi_db(slot: int, rssi_raw: int) -> int:
    return int(load_library().tfrec_amd_rssi_db(int(slot), int(rssi_raw)))


class Receiver:
    """A batch of ``n_streams`` independent receivers on one GPU (one C-ABI context).

    ``submit`` replaces, for every stream, the reference's per-block
    ``process_iq`` + ``fsk_demod::process`` (engine.cpp:85-86); ``drain`` returns the decoder flush events.
    """

    def __init__(self, n_streams: int, types_mask: int = 0x2F, thresh: int = 500, filter_type: int = 0,
                 device: int = 0, max_blocks: int = 48, max_events: int | None = None, all_flushes: bool = False,
                 timing: bool = False, serial_chains: bool = False, input_10x: bool = False, bits: bool = False,
                 experiments: bool = False, input_rate=None, input_format=None, levels: bool = False, dc_windows=None,
                 dc_rows=None, decimated: bool = False, short_segments: bool = False, iq_windows=None, burst_meter: bool = False):
        # experiments=True: the build that reads the TFREC_AMD_* knobs / test hooks from the environment (csrc/knobs.h);
        # the default is the product library, which has none.  short_segments=True: the experiments build with biquad
        # segments of _build.SEG_SLOTS slots (libtfrec_amd_seg.so)
        self.L = load_library(experiments=experiments, short_segments=short_segments)
        if max_events is None:
            max_events = max(4096, n_streams * max_blocks * 4 * (8 if all_flushes else 2))
        flags = ((F_ALL_FLUSHES if all_flushes else 0) | (F_TIMING if timing else 0)
                 | (F_SERIAL_CHAINS if serial_chains else 0) | (F_INPUT_10X if input_10x else 0) | (F_BITS if bits else 0)
                 | (F_LEVELS if levels else 0))  # levels: the level meter (read_levels; levels.py)
        # input_rate=(P, Q): u8 IQ at 1536000 P / Q samples per second, resampled on the GPU (tfrec_amd_create_rate, resample.py).
        # block_bytes: the bytes of one block of one input row -- a fraction when Q does not divide 65536 P; input_bytes(n_blocks)
        # is what a submit takes
        self.input_rate = (10, 1) if input_10x else (1, 1)
        self.cfg = Config(n_streams, types_mask, thresh, filter_type, device, max_blocks, max_events, flags)
        self.h = C.c_void_p()
        # input_format="s8" | "s16" | "f32" (or a TFREC_AMD_FMT_* number; "u8", the default, is the context as it always was): what
        # the input rows hold (tfrec_amd_create_format, formats.py), at input_rate or -- without one -- at 1.536 MS/s.  Rows stay
        # uint8 arrays or tensors, of input_bytes(n_blocks) bytes.
        self.input_format = "u8"
        # dc_windows=K (1 .. 4096): the DC blocker ahead of everything, averaging over K windows of 512 input samples, for at most
        # dc_rows input rows (default: n_streams) -- with any input_format ("u8" included) and input_rate (tfrec_amd_create_dc,
        # dcblock.py)
        # iq_windows=K (1 .. 4096): the IQ balancer behind the DC blocker (dc_windows=K') or without one (dc_windows None or 0),
        # estimating over K of the same windows, for at most dc_rows input rows (tfrec_amd_create_iq, iqbal.py)
        # decimated=True: the rows hold int16 (I, Q) pairs at 384 kS/s, the decimated samples themselves (tfrec_amd_create_decimated,
        # decin.py): 32768 bytes per block.  submit() takes them as uint8 rows like every input, or as int16 arrays.
        self.is_decimated = bool(decimated)
        if decimated:
            if dc_windows is not None or iq_windows is not None or input_format is not None or input_rate is not None:
                raise TfrecAmdError(E_INVAL, "decimated input has no other format, rate, DC blocker or IQ balancer")
            _check(self.L, self.L.tfrec_amd_create_decimated(C.byref(self.cfg), C.byref(self.h)))
            self.input_rate = (1, 4)
            self.input_format = "dec16"
        elif iq_windows is not None or dc_windows is not None or input_format is not None:
            from . import formats

            fix = iq_windows is not None or dc_windows is not None
            p, q = (int(v) for v in (input_rate if input_rate is not None else (1, 1)))
            fmt = "u8" if input_format is None else input_format
            fmt = formats.FORMATS.get(fmt, fmt) if isinstance(fmt, str) else fmt
            rows = n_streams if dc_rows is None or not fix else int(dc_rows)
            k_dc = 0 if dc_windows is None else int(dc_windows)
            k_iq = 0 if iq_windows is None else int(iq_windows)
            if not isinstance(fmt, int) or not all(-2 ** 31 <= v < 2 ** 31 for v in (p, q, fmt, k_dc, k_iq, rows)):
                raise TfrecAmdError(E_INVAL, "input_format, input_rate, dc_windows, iq_windows or dc_rows: unknown name or outside int32")
            if iq_windows is not None:
                rc = self.L.tfrec_amd_create_iq(C.byref(self.cfg), fmt, p, q, k_dc, k_iq, rows, C.byref(self.h))
            elif dc_windows is not None:
                rc = self.L.tfrec_amd_create_dc(C.byref(self.cfg), fmt, p, q, k_dc, rows, C.byref(self.h))
            else:
                rc = self.L.tfrec_amd_create_format(C.byref(self.cfg), fmt, p, q, C.byref(self.h))
            _check(self.L, rc)
            if not input_10x:  # (u8 alone goes with the 10:1 stage)
                self.input_rate = (p, q)
            got = C.c_int32(-1)
            _check(self.L, self.L.tfrec_amd_get_input_format(self.h, C.byref(got)))
            self.input_format = formats.NAMES[got.value]
        elif input_rate is None:
            _check(self.L, self.L.tfrec_amd_create(C.byref(self.cfg), C.byref(self.h)))
        else:
            p, q = (int(v) for v in input_rate)
            if not all(-2 ** 31 <= v < 2 ** 31 for v in (p, q)):  # (refused before int32 could wrap a value into range)
                raise TfrecAmdError(E_INVAL, "input_rate outside int32")
            _check(self.L, self.L.tfrec_amd_create_rate(C.byref(self.cfg), p, q, C.byref(self.h)))
            self.input_rate = (p, q)
        bb = Fraction(BLOCK_BYTES * self.input_rate[0] * {"s16": 2, "f32": 4, "dec16": 2}.get(self.input_format, 1), self.input_rate[1])
        self.block_bytes = int(bb) if bb.denominator == 1 else bb
        self.n_streams = n_streams
        self.max_events = max_events
        self._keep = ()
        self._rows = None  # map_streams: every stream's input row (None: the identity)
        # burst_meter=True: the burst meter alone (burst.py) -- the recorder with room for every run a submit can hold and a pool of
        # one pair, and the meter on it.  A receiver that sizes its recorder itself calls enable_capture, then enable_burst_meter.
        if burst_meter:
            self.enable_capture(n_streams * (max_blocks * BLOCK_DEC // 356 + 3), 1)
            self.enable_burst_meter()

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.tfrec_amd_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def submit(self, iq, n_blocks: int | None = None, stream=None):
        """iq: torch uint8 CUDA tensor [n_streams, n_bytes] (resident in HBM) or a numpy/host array."""
        if isinstance(iq, np.ndarray):
            if self.is_decimated and iq.dtype == np.int16:  # [rows, M, 2] or [rows, 2 M] pairs: their bytes
                iq = np.ascontiguousarray(iq).reshape(iq.shape[0], -1).astype("<i2", copy=False).view(np.uint8)
            a = np.ascontiguousarray(iq, dtype=np.uint8)
            a = a.reshape(a.shape[0] if a.ndim == 2 and self.rows_in_use <= a.shape[0] <= self.n_streams else self.n_streams, -1)
            nb = a.shape[1] // self.block_bytes if n_blocks is None else n_blocks
            _check(self.L, self.L.tfrec_amd_submit_host(self.h, a.ctypes.data, a.strides[0], nb))
            return nb
        import torch

        assert iq.is_cuda and iq.dtype == torch.uint8 and iq.dim() == 2 and self.rows_in_use <= iq.shape[0] <= self.n_streams
        assert iq.stride(1) == 1
        nb = iq.shape[1] // self.block_bytes if n_blocks is None else n_blocks
        st = torch.cuda.current_stream(iq.device) if stream is None else stream
        self._keep = (getattr(self, "_keep", ()) + (iq,))[-FIFO_DEPTH:]  # inputs stay alive while their submit may be in flight
        _check(self.L, self.L.tfrec_amd_submit_device(self.h, C.c_void_p(iq.data_ptr()), iq.stride(0), nb,
                                                      C.c_void_p(st.cuda_stream)))
        return nb

    def input_bytes(self, n_blocks: int) -> int:
        """Bytes one input row of a submit of n_blocks blocks holds (tfrec_amd_input_bytes); E_INVAL for a block count the
        context's input rate does not permit."""
        v = C.c_size_t(0)
        _check(self.L, self.L.tfrec_amd_input_bytes(self.h, int(n_blocks), C.byref(v)))
        return int(v.value)

    def sync(self):
        _check(self.L, self.L.tfrec_amd_sync(self.h))

    def reset_streams(self, streams):
        """Restart the given streams as fresh receivers from the next submit on (tfrec_amd_reset_streams): submits already
        queued drain unchanged; afterwards seq restarts at 0 and end_sample counts from the reset."""
        idx = [int(s) for s in streams]
        if any(s < 0 or s >= self.n_streams for s in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "stream index outside [0, %d)" % self.n_streams)
        a = np.ascontiguousarray(idx, dtype=np.int32)
        _check(self.L, self.L.tfrec_amd_reset_streams(self.h, a.ctypes.data if len(a) else None, len(a)))

    @property
    def state_bytes(self) -> int:
        """Bytes of one stream's state blob in this receiver (tfrec_amd_stream_state_bytes; state.py restates its header)."""
        v = C.c_size_t(0)
        _check(self.L, self.L.tfrec_amd_stream_state_bytes(self.h, C.byref(v)))
        return int(v.value)

    def _stream_list(self, streams):
        idx = [int(s) for s in streams]
        if any(s < 0 or s >= self.n_streams for s in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "stream index outside [0, %d)" % self.n_streams)
        return np.ascontiguousarray(idx, dtype=np.int32)

    def save_streams(self, streams) -> np.ndarray:
        """The listed streams' receiver state behind the last submit made (tfrec_amd_save_streams) -> uint8 [n, state_bytes], one
        blob per stream.  Waits for everything queued and drains nothing.  TfrecAmdError(E_STATE) for a stream with a restart
        pending, (E_INVAL) for a repeated index or a mapped stream."""
        a = self._stream_list(streams)
        out = np.zeros((len(a), self.state_bytes), dtype=np.uint8)
        _check(self.L, self.L.tfrec_amd_save_streams(self.h, a.ctypes.data if len(a) else None, len(a),
                                                     out.ctypes.data if len(a) else None, out.nbytes))
        return out

    def load_streams(self, streams, blobs):
        """Continue the saved receivers blobs[i] in streams[i] (tfrec_amd_load_streams): their settings, tunes, sample count and all
        carried state, from the next submit on.  A blob this receiver cannot continue -- another build, input, types mask,
        levels / recorder / serial-chains setting -- raises TfrecAmdError(E_INVAL) and nothing changes."""
        a = self._stream_list(streams)
        b = np.ascontiguousarray(blobs, dtype=np.uint8).reshape(len(a), -1) if len(a) else np.zeros((0, 0), dtype=np.uint8)
        _check(self.L, self.L.tfrec_amd_load_streams(self.h, a.ctypes.data if len(a) else None, len(a),
                                                     b.ctypes.data if len(a) else None, b.nbytes))

    def configure_streams(self, streams, types_mask=None, thresh=None, filter_type=None):
        """Give the listed streams their own settings (tfrec_amd_configure_streams): each of types_mask, thresh and filter_type
        is one value for all of them or one per listed stream; None keeps each stream's current value.  The streams restart
        as fresh receivers with these settings at the next submit, exactly as after reset_streams."""
        idx = [int(s) for s in streams]
        if any(s < 0 or s >= self.n_streams for s in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "stream index outside [0, %d)" % self.n_streams)

        def per_stream(v):
            if v is None or np.ndim(v) == 0:
                return [v] * len(idx)
            v = list(v)
            if len(v) != len(idx):
                raise ValueError("%d values for %d streams" % (len(v), len(idx)))
            return v

        cur = {}
        cfgs = (StreamConfig * max(1, len(idx)))()
        for i, (s, t, th, w) in enumerate(zip(idx, per_stream(types_mask), per_stream(thresh), per_stream(filter_type))):
            c = cur[s] if s in cur else self.stream_config(s)  # (a duplicate index builds on the value before it)
            c = {"types_mask": c["types_mask"] if t is None else int(t), "thresh": c["thresh"] if th is None else int(th),
                 "filter_type": c["filter_type"] if w is None else int(w)}
            cur[s] = c
            cfgs[i] = StreamConfig(c["types_mask"], c["thresh"], c["filter_type"], 0)
        a = np.ascontiguousarray(idx, dtype=np.int32)
        _check(self.L, self.L.tfrec_amd_configure_streams(self.h, a.ctypes.data if len(a) else None,
                                                          C.cast(cfgs, C.c_void_p) if len(a) else None, len(a)))

    def stream_config(self, stream: int) -> dict:
        """The settings the next submit uses for one stream (tfrec_amd_get_stream_config)."""
        c = StreamConfig()
        _check(self.L, self.L.tfrec_amd_get_stream_config(self.h, int(stream), C.byref(c)))
        return {"types_mask": c.types_mask, "thresh": c.thresh, "filter_type": c.filter_type}

    def tune_streams(self, streams, tune_hz):
        """Tune the listed streams (tfrec_amd_tune_streams): tune_hz is one value for all of them or one per listed stream, the
        offset in Hz of the wanted channel from the recording's centre (|tune_hz| < 768000; 0 = untuned; see tune.py).  The
        streams restart as fresh receivers at the next submit, exactly as after reset_streams."""
        idx = [int(s) for s in streams]
        if any(s < 0 or s >= self.n_streams for s in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "stream index outside [0, %d)" % self.n_streams)
        hz = [int(tune_hz)] * len(idx) if np.ndim(tune_hz) == 0 else [int(v) for v in tune_hz]
        if len(hz) != len(idx):
            raise ValueError("%d values for %d streams" % (len(hz), len(idx)))
        if any(not -2 ** 31 <= v < 2 ** 31 for v in hz):  # (refused before int32 could wrap a value into range)
            raise TfrecAmdError(E_INVAL, "tune_hz outside int32")
        a = np.ascontiguousarray(idx, dtype=np.int32)
        t = np.ascontiguousarray(hz, dtype=np.int32)
        _check(self.L, self.L.tfrec_amd_tune_streams(self.h, a.ctypes.data if len(a) else None,
                                                     t.ctypes.data if len(t) else None, len(a)))

    def stream_tune(self, stream: int) -> int:
        """The tune in Hz the next submit uses for one stream (tfrec_amd_get_stream_tune)."""
        v = C.c_int32(0)
        _check(self.L, self.L.tfrec_amd_get_stream_tune(self.h, int(stream), C.byref(v)))
        return int(v.value)

    def _pairs(self, fn, streams, values, what, name):
        idx = [int(s) for s in streams]
        if any(s < 0 or s >= self.n_streams for s in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "stream index outside [0, %d)" % self.n_streams)
        v = [int(values)] * len(idx) if np.ndim(values) == 0 else [int(x) for x in values]
        if len(v) != len(idx):
            raise ValueError("%d values for %d streams" % (len(v), len(idx)))
        if any(not -2 ** 31 <= x < 2 ** 31 for x in v):  # (refused before int32 could wrap a value into range)
            raise TfrecAmdError(E_INVAL, "%s outside int32" % name)
        a = np.ascontiguousarray(idx, dtype=np.int32)
        t = np.ascontiguousarray(v, dtype=np.int32)
        _check(self.L, fn(self.h, a.ctypes.data if len(a) else None, t.ctypes.data if len(t) else None, len(a)))
        return idx, v

    def map_streams(self, streams, inputs):
        """Let the listed streams read the given input rows (tfrec_amd_map_streams): `inputs` is one row for all of them or one
        per listed stream.  Several streams may share a row; a submit then needs rows 0 .. rows_in_use - 1 only.  The streams
        restart as fresh receivers at the next submit, exactly as after reset_streams."""
        idx, rows = self._pairs(self.L.tfrec_amd_map_streams, streams, inputs, "map", "input row")
        if idx:
            if self._rows is None:
                self._rows = list(range(self.n_streams))
            for s, r in zip(idx, rows):
                self._rows[s] = r

    def stream_input(self, stream: int) -> int:
        """The input row the next submit reads for one stream (tfrec_amd_get_stream_input)."""
        v = C.c_int32(0)
        _check(self.L, self.L.tfrec_amd_get_stream_input(self.h, int(stream), C.byref(v)))
        return int(v.value)

    @property
    def rows_in_use(self) -> int:
        """Rows of the input batch a submit must provide: n_streams, or 1 + the highest row mapped."""
        return self.n_streams if self._rows is None else 1 + max(self._rows)

    def tune_streams_wide(self, streams, tune_hz):
        """Wideband tune of the listed streams (tfrec_amd_tune_streams_wide, input_10x contexts): the offset in Hz of the wanted
        channel from the centre of the 15.36 MS/s input (|tune_hz| < 7680000; 0 = none; see tune.py: mix10_s16).  The streams
        restart as fresh receivers at the next submit, exactly as after reset_streams."""
        self._pairs(self.L.tfrec_amd_tune_streams_wide, streams, tune_hz, "tune", "tune_hz")

    def stream_tune_wide(self, stream: int) -> int:
        """The wide tune in Hz the next submit uses for one stream (tfrec_amd_get_stream_tune_wide)."""
        v = C.c_int32(0)
        _check(self.L, self.L.tfrec_amd_get_stream_tune_wide(self.h, int(stream), C.byref(v)))
        return int(v.value)

    def tune_streams_input(self, streams, tune_hz):
        """Input-rate tune of the listed streams (tfrec_amd_tune_streams_input, input_rate and input_10x contexts): the offset in
        Hz of the wanted channel from the centre of the recording, applied ahead of the resampling stage (|tune_hz| < half the
        input rate; 0 = none; see tune.py: mix_in_s16).  The streams restart as fresh receivers at the next submit."""
        self._pairs(self.L.tfrec_amd_tune_streams_input, streams, tune_hz, "tune", "tune_hz")

    def stream_tune_input(self, stream: int) -> int:
        """The input-rate tune in Hz the next submit uses for one stream (tfrec_amd_get_stream_tune_input)."""
        v = C.c_int32(0)
        _check(self.L, self.L.tfrec_amd_get_stream_tune_input(self.h, int(stream), C.byref(v)))
        return int(v.value)

    def drain(self, allow_overflow: bool = False) -> np.ndarray:
        out = np.empty(self.max_events, dtype=EVENT_DTYPE)
        n = C.c_int(0)
        rc = self.L.tfrec_amd_drain_events(self.h, out.ctypes.data, self.max_events, C.byref(n))
        _check(self.L, rc, ok=(E_OK, E_OVERFLOW) if allow_overflow else (E_OK,))
        return out[: n.value]

    def read_levels(self) -> np.ndarray:
        """levels=True: the level records of the OLDEST undrained submit (tfrec_amd_read_levels; call it before the drain that pops
        that submit) as a LEVEL_DTYPE array [n_streams, n_blocks].  TfrecAmdError(E_INVAL) on a context without levels,
        (E_STATE) when nothing is waiting to be drained."""
        out = np.empty(self.n_streams * self.cfg.max_blocks, dtype=LEVEL_DTYPE)
        nb = C.c_int(0)
        _check(self.L, self.L.tfrec_amd_read_levels(self.h, out.ctypes.data, len(out), C.byref(nb)))
        return out[: self.n_streams * nb.value].reshape(self.n_streams, nb.value).copy()

    def enable_capture(self, max_runs: int, max_samples: int):
        """Turn the squelched recorder on (tfrec_amd_enable_capture; before the first submit): per submit at most max_runs runs and
        max_samples (I, Q) pairs are kept on the device.  read_captures returns them."""
        if not (0 <= int(max_runs) < 2 ** 32 and 0 <= int(max_samples) < 2 ** 64):  # (refused before ctypes could wrap a value)
            raise TfrecAmdError(E_INVAL, "max_runs or max_samples outside their types")
        _check(self.L, self.L.tfrec_amd_enable_capture(self.h, int(max_runs), int(max_samples)))
        self._capture = (int(max_runs), int(max_samples))

    def read_captures(self, allow_overflow: bool = False, pre: bool = False):
        """The captures of the OLDEST undrained submit (tfrec_amd_read_captures; call it before the drain that pops that submit)
        -> (runs, samples): a RUN_DTYPE array ordered by (stream, start_sample) and the pool, int16 [n_pairs, 2]; run r's pairs are
        samples[r.pool_offset : r.pool_offset + r.n_samples].  A device-side overflow (E_OVERFLOW) raises unless allow_overflow,
        as for drain(); then the longest prefix of whole runs that fitted is returned.  capture_totals holds the submit's true
        (n_runs, n_pairs) and capture_overflow whether it overflowed.  TfrecAmdError(E_INVAL) on a context without enable_capture,
        (E_STATE) when nothing is waiting to be drained.  pre=True (after enable_capture_pre): -> (runs, samples, pre), pre as
        read_capture_pre returns it."""
        if pre:
            runs, samples = self.read_captures(allow_overflow)
            return runs, samples, self.read_capture_pre(allow_overflow)[:len(runs)]
        ok = (E_OK, E_OVERFLOW) if allow_overflow else (E_OK,)
        nr, npairs = C.c_uint32(0), C.c_uint64(0)
        max_runs, max_samples = getattr(self, "_capture", (0, 0))
        rc = self.L.tfrec_amd_read_captures(self.h, None, 0, C.byref(nr), None, 0, C.byref(npairs))  # the counts (no room: E_INVAL)
        if max_runs == 0 or rc == E_STATE or (rc == E_INVAL and nr.value == 0):
            _check(self.L, rc)
        runs = np.zeros(min(nr.value, max_runs) + 1, dtype=RUN_DTYPE)  # (+ 1: the entry that ends an overflowed table)
        samples = np.empty((min(npairs.value, max_samples) + 1, 2), dtype=np.int16)
        rc = self.L.tfrec_amd_read_captures(self.h, runs.ctypes.data, len(runs), C.byref(nr), samples.ctypes.data, len(samples),
                                            C.byref(npairs))
        self.capture_totals = (int(nr.value), int(npairs.value))
        self.capture_overflow = rc == E_OVERFLOW
        _check(self.L, rc, ok=ok)
        k = nr.value
        if rc == E_OVERFLOW:
            k = int(np.flatnonzero(runs["n_samples"] == 0)[0])
        runs = runs[:k].copy()
        n = int(runs["pool_offset"][-1] + runs["n_samples"][-1]) if k else 0
        return runs, samples[:n].copy()

    def enable_capture_pre(self):
        """Let the recorder also keep the sample ahead of every run (tfrec_amd_enable_capture_pre; after enable_capture, before the
        first submit).  read_capture_pre, or read_captures(pre=True), returns them."""
        _check(self.L, self.L.tfrec_amd_enable_capture_pre(self.h))

    def read_capture_pre(self, allow_overflow: bool = False) -> np.ndarray:
        """The pair ahead of every run of the table read_captures returns for the same -- the OLDEST undrained -- submit
        (tfrec_amd_read_capture_pre; decin.pre_samples) -> int16 [n_runs, 2].  Overflow as for read_captures."""
        ok = (E_OK, E_OVERFLOW) if allow_overflow else (E_OK,)
        nr = C.c_uint32(0)
        rc = self.L.tfrec_amd_read_capture_pre(self.h, None, 0, C.byref(nr))  # the count (no room: E_INVAL)
        if rc != E_INVAL or nr.value == 0:
            _check(self.L, rc, ok=ok)
            return np.zeros((0, 2), dtype=np.int16)
        max_runs = getattr(self, "_capture", (0, 0))[0]
        pre = np.zeros((min(nr.value, max_runs), 2), dtype=np.int16)
        rc = self.L.tfrec_amd_read_capture_pre(self.h, pre.ctypes.data, len(pre), C.byref(nr))
        _check(self.L, rc, ok=ok)
        if rc == E_OVERFLOW:  # the delivered prefix is the table's
            pre = pre[:len(self.read_captures(allow_overflow=True)[0])]
        return pre

    def _read_run_records(self, fn, dtype, total_attr, allow_overflow, words=False):
        """What the reads of the five burst stages share: the records of the oldest undrained submit by `fn` -- the count first
        (no room: E_INVAL), then the records, and with `words` the bitmap's uint32 words beside them.  `total_attr` is given the
        submit's true run count; E_OVERFLOW raises unless allow_overflow."""
        ok = (E_OK, E_OVERFLOW) if allow_overflow else (E_OK,)
        nr, nw = C.c_uint32(0), C.c_uint64(0)
        counts = (None, 0, C.byref(nw)) if words else ()
        rc = fn(self.h, None, 0, C.byref(nr), *counts)  # the counts (no room: E_INVAL)
        setattr(self, total_attr, int(nr.value))
        bits = np.zeros(0, dtype=np.uint32)
        if rc != E_INVAL or nr.value == 0:
            _check(self.L, rc, ok=ok)
            out = np.zeros(0, dtype=dtype)
            return (out, bits) if words else out
        out = np.zeros(min(nr.value, getattr(self, "_capture", (0, 0))[0]), dtype=dtype)
        if words:
            bits = np.zeros(int(nw.value), dtype=np.uint32)
            counts = (bits.ctypes.data if len(bits) else None, len(bits), C.byref(nw))
        _check(self.L, fn(self.h, out.ctypes.data, len(out), C.byref(nr), *counts), ok=ok)
        return (out, bits) if words else out

    def enable_burst_meter(self):
        """Turn the burst meter on (tfrec_amd_enable_burst_meter; after enable_capture, before the first submit).  read_bursts
        returns its records."""
        _check(self.L, self.L.tfrec_amd_enable_burst_meter(self.h))

    def read_bursts(self, allow_overflow: bool = False) -> np.ndarray:
        """The burst records of the OLDEST undrained submit (tfrec_amd_read_bursts; call it before the drain that pops that
        submit) -> a BURST_DTYPE array, one record per entry of that submit's run table (burst.py).  They do not depend on the pool:
        a table with more than max_runs entries (E_OVERFLOW) raises unless allow_overflow, then its first max_runs records are
        returned; burst_total holds the submit's true run count."""
        return self._read_run_records(self.L.tfrec_amd_read_bursts, BURST_DTYPE, "burst_total", allow_overflow)

    def enable_burst_envelope(self):
        """Turn the burst envelope on (tfrec_amd_enable_burst_envelope; after enable_capture, before the first submit; with or
        without the burst meter).  read_burst_envelopes returns its records."""
        _check(self.L, self.L.tfrec_amd_enable_burst_envelope(self.h))

    def read_burst_envelopes(self, allow_overflow: bool = False) -> np.ndarray:
        """The envelope records of the OLDEST undrained submit (tfrec_amd_read_burst_envelopes; call it before the drain that pops
        that submit) -> an ENVELOPE_DTYPE array, one record per entry of that submit's run table (envelope.py).  They do not depend
        on the pool: a table with more than max_runs entries (E_OVERFLOW) raises unless allow_overflow, then its first max_runs
        records are returned; envelope_total holds the submit's true run count."""
        return self._read_run_records(self.L.tfrec_amd_read_burst_envelopes, ENVELOPE_DTYPE, "envelope_total", allow_overflow)

    def enable_burst_clock(self):
        """Turn the burst clock on (tfrec_amd_enable_burst_clock; after enable_capture, before the first submit; with or without
        the burst meter and the envelope).  read_burst_clocks returns its records."""
        _check(self.L, self.L.tfrec_amd_enable_burst_clock(self.h))

    def read_burst_clocks(self, allow_overflow: bool = False) -> np.ndarray:
        """The clock records of the OLDEST undrained submit (tfrec_amd_read_burst_clocks; call it before the drain that pops that
        submit) -> a CLOCK_DTYPE array, one record per entry of that submit's run table (clock.py).  They do not depend on the
        pool: a table with more than max_runs entries (E_OVERFLOW) raises unless allow_overflow, then its first max_runs records
        are returned; clock_total holds the submit's true run count."""
        return self._read_run_records(self.L.tfrec_amd_read_burst_clocks, CLOCK_DTYPE, "clock_total", allow_overflow)

    def enable_burst_track(self, smooth: int):
        """Turn the burst track on (tfrec_amd_enable_burst_track; after enable_capture, before the first submit; with or without
        the meter, the envelope and the clock): a bit per captured sample, the sign of a discriminator about the stream's centre
        smoothed over `smooth` (1 .. 16) products.  read_burst_tracks returns the records and the bitmap."""
        if not -2 ** 31 <= int(smooth) < 2 ** 31:  # (refused before ctypes could wrap a value into range)
            raise TfrecAmdError(E_INVAL, "smooth outside its type")
        _check(self.L, self.L.tfrec_amd_enable_burst_track(self.h, int(smooth)))

    def set_burst_track_centre(self, streams, hz):
        """The listed streams' centres in Hz (tfrec_amd_set_burst_track_centre): one value for all of them or one per listed
        stream, |hz| <= 192000, in force from the next submit on.  Not a restart."""
        idx = [int(s) for s in streams]
        if any(s < 0 or s >= self.n_streams for s in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "stream index outside [0, %d)" % self.n_streams)
        v = [int(hz)] * len(idx) if np.ndim(hz) == 0 else [int(x) for x in hz]
        if len(v) != len(idx):
            raise ValueError("%d values for %d streams" % (len(v), len(idx)))
        if any(abs(x) >= 2 ** 31 for x in v):
            raise TfrecAmdError(E_INVAL, "centre outside its type")
        a, b = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(v, dtype=np.int32)
        _check(self.L, self.L.tfrec_amd_set_burst_track_centre(self.h, a.ctypes.data if len(a) else None,
                                                               b.ctypes.data if len(a) else None, len(a)))

    def enable_burst_track_amplitude(self, smooth: int):
        """Turn the burst track on in amplitude mode (tfrec_amd_enable_burst_track_amplitude; enable_burst_track's rules, and
        instead of it): a bit per captured sample, 1 where the sum of `smooth` (1 .. 16) powers |I| + |Q| lies above `smooth`
        times the stream's level -- an on-off keyed burst's track.  read_burst_tracks returns the records and the bitmap."""
        if not -2 ** 31 <= int(smooth) < 2 ** 31:  # (refused before ctypes could wrap a value into range)
            raise TfrecAmdError(E_INVAL, "smooth outside its type")
        _check(self.L, self.L.tfrec_amd_enable_burst_track_amplitude(self.h, int(smooth)))

    def set_burst_track_level(self, streams, level):
        """The listed streams' levels (tfrec_amd_set_burst_track_level): one value for all of them or one per listed stream,
        0 .. 65535 in the trigger's unit, in force from the next submit on.  Not a restart."""
        idx = [int(s) for s in streams]
        if any(s < 0 or s >= self.n_streams for s in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "stream index outside [0, %d)" % self.n_streams)
        v = [int(level)] * len(idx) if np.ndim(level) == 0 else [int(x) for x in level]
        if len(v) != len(idx):
            raise ValueError("%d values for %d streams" % (len(v), len(idx)))
        if any(abs(x) >= 2 ** 31 for x in v):
            raise TfrecAmdError(E_INVAL, "level outside its type")
        a, b = np.ascontiguousarray(idx, dtype=np.int32), np.ascontiguousarray(v, dtype=np.int32)
        _check(self.L, self.L.tfrec_amd_set_burst_track_level(self.h, a.ctypes.data if len(a) else None,
                                                              b.ctypes.data if len(a) else None, len(a)))

    def enable_burst_track_auto(self, smooth: int, head: int = 1024):
        """Turn the burst track on in auto-centre mode (tfrec_amd_enable_burst_track_auto; enable_burst_track's rules, and instead
        of it): every chain is tracked about a centre measured on the first `head` (64 .. 4096) samples of its first piece;
        set_burst_track_centre sets the fallback.  read_burst_tracks returns the records and the bitmap,
        read_burst_track_centres every entry's centre."""
        if not (-2 ** 31 <= int(smooth) < 2 ** 31 and -2 ** 31 <= int(head) < 2 ** 31):  # (refused before ctypes could wrap a value into range)
            raise TfrecAmdError(E_INVAL, "smooth or head outside its type")
        _check(self.L, self.L.tfrec_amd_enable_burst_track_auto(self.h, int(smooth), int(head)))

    def enable_burst_track_phase(self, smooth: int, head: int = 1024, lag: int = 1):
        """Turn the burst track on in phase mode (tfrec_amd_enable_burst_track_phase; enable_burst_track's rules, and instead of
        it), for phase-keyed bursts: a differential phase detector at a lag of `lag` (1 .. 64) samples, boxcar `smooth`, about
        the carrier measured on the first `head` (64 .. 4096) samples of every chain's first piece; set_burst_track_centre sets the
        fallback.  read_burst_tracks returns the records and the bitmap, read_burst_track_centres every entry's carrier."""
        if not all(-2 ** 31 <= int(v) < 2 ** 31 for v in (smooth, head, lag)):  # (refused before ctypes could wrap a value into range)
            raise TfrecAmdError(E_INVAL, "smooth, head or lag outside its type")
        _check(self.L, self.L.tfrec_amd_enable_burst_track_phase(self.h, int(smooth), int(head), int(lag)))

    def read_burst_track_centres(self, allow_overflow: bool = False) -> np.ndarray:
        """The centre records of the OLDEST undrained submit (tfrec_amd_read_burst_track_centres; call it before the drain that
        pops that submit) -> a CENTRE_DTYPE array, one record per entry of that submit's run table (track.py).  They do not depend
        on the pool: a table with more than max_runs entries (E_OVERFLOW) raises unless allow_overflow, then its first max_runs
        records are returned; centre_total holds the submit's true run count."""
        from .track import CENTRE_DTYPE
        return self._read_run_records(self.L.tfrec_amd_read_burst_track_centres, CENTRE_DTYPE, "centre_total", allow_overflow)

    def read_burst_tracks(self, allow_overflow: bool = False):
        """The track of the OLDEST undrained submit (tfrec_amd_read_burst_tracks; call it before the drain that pops that submit)
        -> (a TRACK_DTYPE array, one record per entry of that submit's run table; the bitmap's uint32 words): track.bits_of(rec,
        words) is a record's track.  An overflowed table or pool (E_OVERFLOW) raises unless allow_overflow; then the records below
        max_runs and the words of the pairs read_captures delivers are returned.  track_total holds the submit's true run count."""
        return self._read_run_records(self.L.tfrec_amd_read_burst_tracks, TRACK_DTYPE, "track_total", allow_overflow, words=True)

    def enable_burst_sync(self, rate: int, pattern: int, n_bits: int, max_errors: int = 0, both: bool = False):
        """Turn the burst sync on (tfrec_amd_enable_burst_sync; after enable_burst_track, before the first submit): a bit per
        captured sample, 1 where the track read at `rate` bit/s ends in the low `n_bits` (8 .. 64) bits of `pattern`, MSB first,
        but for at most `max_errors` places; `both`: the complemented pattern too.  read_burst_syncs returns the records and the
        match bitmap."""
        for v, name in ((rate, "rate"), (n_bits, "n_bits"), (max_errors, "max_errors")):
            if not -2 ** 31 <= int(v) < 2 ** 31:  # (refused before ctypes could wrap a value into range)
                raise TfrecAmdError(E_INVAL, name + " outside its type")
        _check(self.L, self.L.tfrec_amd_enable_burst_sync(self.h, int(rate), int(pattern) & (2 ** 64 - 1), int(n_bits), int(max_errors),
                                                          1 if both else 0))

    def read_burst_syncs(self, allow_overflow: bool = False):
        """The sync of the OLDEST undrained submit (tfrec_amd_read_burst_syncs; call it before the drain that pops that submit)
        -> (a SYNC_DTYPE array, one record per entry of that submit's run table; the match bitmap's uint32 words): sync.bits_of(rec,
        words) is a record's match track.  Overflow as for read_burst_tracks.  sync_total holds the submit's true run count."""
        return self._read_run_records(self.L.tfrec_amd_read_burst_syncs, SYNC_DTYPE, "sync_total", allow_overflow, words=True)

    def enable_burst_code(self, rate: int, taps: int, invert: bool = False):
        """Turn the line code on (tfrec_amd_enable_burst_code; after enable_burst_track in any mode, before the first submit,
        before or after enable_burst_sync): a bit per captured sample, the track XORed with itself delayed by j symbols at `rate`
        bit/s for every set bit j - 1 of `taps` (linecode.NAMED: g3ruh, nrzi, nrzs), complemented under `invert`.
        read_burst_codes returns the records and the coded bitmap; the sync then works on the coded track."""
        if not -2 ** 31 <= int(rate) < 2 ** 31 or not 0 <= int(taps) < 2 ** 32:  # (refused before ctypes could wrap a value into range)
            raise TfrecAmdError(E_INVAL, "rate or taps outside its type")
        _check(self.L, self.L.tfrec_amd_enable_burst_code(self.h, int(rate), int(taps), 1 if invert else 0))

    def read_burst_codes(self, allow_overflow: bool = False):
        """The coded track of the OLDEST undrained submit (tfrec_amd_read_burst_codes; call it before the drain that pops that
        submit) -> (a TRACK_DTYPE array, one record per entry of that submit's run table; the coded bitmap's uint32 words):
        track.bits_of(rec, words) is a record's coded track.  Overflow as for read_burst_tracks.  code_total holds the submit's
        true run count."""
        return self._read_run_records(self.L.tfrec_amd_read_burst_codes, TRACK_DTYPE, "code_total", allow_overflow, words=True)

    def enable_burst_crc(self, rate: int, n_bytes: int, width: int, poly: int, init: int = 0, xorout: int = 0, skip: int = 0,
                         lsb: bool = False, invert: bool = False):
        """Turn the frame check on (tfrec_amd_enable_burst_crc; after enable_burst_track in any mode, before the first submit, in
        any order with enable_burst_code and enable_burst_sync, or without them): a bit per captured sample, 1 where the n_bytes
        bytes whose last bit sits at the sample -- read at symbol centres at `rate` bit/s from the sync's input track -- carry
        their own CRC (crc.Settings).  read_burst_crcs returns the records and the check bitmap."""
        args = (rate, n_bytes, skip, width)
        if not all(-2 ** 31 <= int(a) < 2 ** 31 for a in args) or not all(0 <= int(a) < 2 ** 32 for a in (poly, init, xorout)):
            raise TfrecAmdError(E_INVAL, "a setting outside its type")  # (refused before ctypes could wrap a value into range)
        _check(self.L, self.L.tfrec_amd_enable_burst_crc(self.h, int(rate), int(n_bytes), int(skip), int(width), int(poly), int(init),
                                                         int(xorout), (1 if lsb else 0) | (2 if invert else 0)))

    def read_burst_crcs(self, allow_overflow: bool = False):
        """The check track of the OLDEST undrained submit (tfrec_amd_read_burst_crcs; call it before the drain that pops that
        submit) -> (a CRC_DTYPE array, one record per entry of that submit's run table; the check bitmap's uint32 words):
        crc.bits_of(rec, words) is a record's check track.  Overflow as for read_burst_tracks.  crc_total holds the submit's true
        run count."""
        return self._read_run_records(self.L.tfrec_amd_read_burst_crcs, CRC_DTYPE, "crc_total", allow_overflow, words=True)

    def enable_runs_input(self, max_runs: int, max_samples: int):
        """Turn sparse submits on (tfrec_amd_enable_runs_input; decimated receivers, before the first submit): a submit_runs may
        carry at most max_runs runs and max_samples pairs."""
        if not (0 <= int(max_runs) < 2 ** 32 and 0 <= int(max_samples) < 2 ** 64):  # (refused before ctypes could wrap a value)
            raise TfrecAmdError(E_INVAL, "max_runs or max_samples outside their types")
        _check(self.L, self.L.tfrec_amd_enable_runs_input(self.h, int(max_runs), int(max_samples)))

    def submit_runs(self, runs, samples, pre, n_blocks: int):
        """One submit of n_blocks blocks given as a run table (RUN_DTYPE, start_sample relative to the submit), its pool and the
        pair ahead of every run (tfrec_amd_submit_runs): exactly submit() of decin.expand(runs, samples, pre, ...)."""
        t = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
        p = np.ascontiguousarray(samples, dtype="<i2").reshape(-1, 2)
        q = np.ascontiguousarray(pre, dtype="<i2").reshape(-1, 2)
        if len(q) != len(t):
            raise ValueError("%d pre samples for %d runs" % (len(q), len(t)))
        if not -2 ** 31 <= int(n_blocks) < 2 ** 31:
            raise TfrecAmdError(E_INVAL, "n_blocks outside int32")
        _check(self.L, self.L.tfrec_amd_submit_runs(self.h, t.ctypes.data if len(t) else None, len(t), p.ctypes.data if len(p) else None,
                                                    len(p), q.ctypes.data if len(q) else None, int(n_blocks)))
        return int(n_blocks)

    def enable_spectrum(self, n_bins: int, frames_per_record: int, max_rows: int | None = None):
        """Turn the per-input power spectrum on (tfrec_amd_enable_spectrum; before the first submit): an exact integer DFT of
        n_bins bins over rows 0 .. max_rows - 1 (default: every row) of each submit, frames_per_record frames per record
        (spectrum.py).  read_spectrum returns the records."""
        rows = self.n_streams if max_rows is None else int(max_rows)
        if not all(-2 ** 31 <= int(v) < 2 ** 31 for v in (n_bins, frames_per_record, rows)):  # (refused before int32 could wrap)
            raise TfrecAmdError(E_INVAL, "n_bins, frames_per_record or max_rows outside int32")
        _check(self.L, self.L.tfrec_amd_enable_spectrum(self.h, int(n_bins), int(frames_per_record), rows))
        self._spectrum_bins = int(n_bins)

    def read_spectrum(self, row: int):
        """The spectrum records of input row `row` of the OLDEST undrained submit (tfrec_amd_read_spectrum; call it before the drain
        that pops that submit) -> (sum[n_records, N] uint64, peak[n_records, N] uint64, n_frames[n_records] uint32).
        TfrecAmdError(E_INVAL) on a context without enable_spectrum or for a row the submit's spectrum does not cover, (E_STATE)
        when nothing is waiting to be drained."""
        if not -2 ** 31 <= int(row) < 2 ** 31:
            raise TfrecAmdError(E_INVAL, "row outside int32")
        nr = C.c_int(0)
        rc = self.L.tfrec_amd_read_spectrum(self.h, int(row), None, None, 0, None, C.byref(nr))  # the count (no room: E_INVAL)
        n = getattr(self, "_spectrum_bins", 0)
        if n == 0 or rc == E_STATE or (rc == E_INVAL and nr.value == 0):
            _check(self.L, rc)
        s = np.zeros((nr.value, n), dtype=np.uint64)
        p = np.zeros((nr.value, n), dtype=np.uint64)
        f = np.zeros(nr.value, dtype=np.uint32)
        if nr.value:
            _check(self.L, self.L.tfrec_amd_read_spectrum(self.h, int(row), s.ctypes.data, p.ctypes.data, nr.value, f.ctypes.data,
                                                          C.byref(nr)))
        return s, p, f

    def enable_occupancy(self, ratio: int = 32, rel: int = 16):
        """Turn the occupancy detector on (tfrec_amd_enable_occupancy; after enable_spectrum, before the first submit): per
        spectrum record a noise floor and a bitmap of the bins whose peak stands `ratio` times above it and within 1 / `rel` of the
        record's strongest (occupancy.py).  read_occupancy returns them."""
        if not all(0 <= int(v) < 2 ** 32 for v in (ratio, rel)):  # (refused before ctypes could wrap a value)
            raise TfrecAmdError(E_INVAL, "ratio or rel outside uint32")
        _check(self.L, self.L.tfrec_amd_enable_occupancy(self.h, int(ratio), int(rel)))
        self._occupancy = True

    def read_occupancy(self, row: int):
        """The occupancy records of input row `row` of the OLDEST undrained submit (tfrec_amd_read_occupancy; call it before the
        drain that pops that submit) -> (records: OCC_DTYPE [n_records], bitmap: uint32 [n_records, N / 32]); occupancy.unpack
        turns the bitmap into booleans.  TfrecAmdError(E_INVAL) on a context without enable_occupancy or for a row the submit's
        spectrum does not cover, (E_STATE) when nothing is waiting to be drained."""
        if not -2 ** 31 <= int(row) < 2 ** 31:
            raise TfrecAmdError(E_INVAL, "row outside int32")
        nr = C.c_int(0)
        rc = self.L.tfrec_amd_read_occupancy(self.h, int(row), None, None, 0, C.byref(nr))  # the count (no room: E_INVAL)
        n = getattr(self, "_spectrum_bins", 0)
        if not getattr(self, "_occupancy", False) or n == 0 or rc == E_STATE or (rc == E_INVAL and nr.value == 0):
            _check(self.L, rc)
        recs = np.zeros(nr.value, dtype=OCC_DTYPE)
        bits = np.zeros((nr.value, n // 32), dtype=np.uint32)
        if nr.value:
            _check(self.L, self.L.tfrec_amd_read_occupancy(self.h, int(row), recs.ctypes.data, bits.ctypes.data, nr.value, C.byref(nr)))
        return recs, bits

    def dc(self) -> tuple:
        """(avg_windows, max_rows) of a dc_windows context, (0, 0) of every other (tfrec_amd_get_dc)."""
        k, rows = C.c_int32(-1), C.c_int32(-1)
        _check(self.L, self.L.tfrec_amd_get_dc(self.h, C.byref(k), C.byref(rows)))
        return int(k.value), int(rows.value)

    def _read_estimates(self, read, row: int) -> np.ndarray:
        if not -2 ** 31 <= int(row) < 2 ** 31:
            raise TfrecAmdError(E_INVAL, "row outside int32")
        nw = C.c_int(0)
        rc = read(self.h, int(row), None, 0, C.byref(nw))  # the count (no room: E_INVAL)
        if rc != E_INVAL or nw.value == 0:
            _check(self.L, rc)
        out = np.zeros((nw.value, 2), dtype=np.int16)
        if nw.value:
            _check(self.L, read(self.h, int(row), out.ctypes.data, nw.value, C.byref(nw)))
        return out

    def _reset_rows(self, reset, rows) -> None:
        idx = [int(r) for r in rows]
        if any(not -2 ** 31 <= r < 2 ** 31 for r in idx):  # (refused before int32 could wrap an index into range)
            raise TfrecAmdError(E_INVAL, "row outside int32")
        a = np.ascontiguousarray(idx, dtype=np.int32)
        _check(self.L, reset(self.h, a.ctypes.data if len(a) else None, len(a)))

    def read_dc(self, row: int) -> np.ndarray:
        """The DC estimates d[w] of input row `row` of the OLDEST undrained submit (tfrec_amd_read_dc; call it before the drain that
        pops that submit) -> int16 [n_windows, 2], (I, Q).  TfrecAmdError(E_INVAL) on a context without the blocker or for a row the
        submit did not use, (E_STATE) when nothing is waiting to be drained."""
        return self._read_estimates(self.L.tfrec_amd_read_dc, row)

    def iq(self) -> tuple:
        """(iq_windows, max_rows) of an iq_windows context, (0, 0) of every other (tfrec_amd_get_iq)."""
        k, rows = C.c_int32(-1), C.c_int32(-1)
        _check(self.L, self.L.tfrec_amd_get_iq(self.h, C.byref(k), C.byref(rows)))
        return int(k.value), int(rows.value)

    def read_iq(self, row: int) -> np.ndarray:
        """The balancer's (t, g) of input row `row` of the OLDEST undrained submit (tfrec_amd_read_iq; call it before the drain that
        pops that submit) -> int16 [n_windows, 2].  TfrecAmdError(E_INVAL) on a context without the balancer or for a row the submit
        did not use, (E_STATE) when nothing is waiting to be drained."""
        return self._read_estimates(self.L.tfrec_amd_read_iq, row)

    def reset_iq_rows(self, rows):
        """Clear the balancer's state of the listed input rows at the next submit (tfrec_amd_reset_iq_rows); the streams are not
        restarted and the DC blocker's state is reset_dc_rows's."""
        self._reset_rows(self.L.tfrec_amd_reset_iq_rows, rows)

    def reset_dc_rows(self, rows):
        """Clear the DC state of the listed input rows at the next submit (tfrec_amd_reset_dc_rows); the streams are not restarted."""
        self._reset_rows(self.L.tfrec_amd_reset_dc_rows, rows)

    def stage0(self, stream: int, n_pairs: int) -> np.ndarray:
        """input_10x or input_rate: the 1.536 MS/s int16 IQ the 10:1 or the resampling stage produced for the last submit."""
        out = np.empty(2 * n_pairs, dtype=np.int16)
        _check(self.L, self.L.tfrec_amd_read_stage0(self.h, stream, out.ctypes.data, n_pairs))
        return out

    def decimated(self, stream: int, n_pairs: int) -> np.ndarray:
        out = np.empty(2 * n_pairs, dtype=np.int16)
        _check(self.L, self.L.tfrec_amd_read_decimated(self.h, stream, out.ctypes.data, n_pairs))
        return out

    def biquad_row(self, slot: int, stream: int) -> np.ndarray:
        """Parity probe: the window-relative biquad output row of (slot, stream) in the most recently drained submit, int32 --
        32 values per slot of the row, the TFA_2 family's int16 outputs widened (tfrec_amd_read_biquad_row).  Window j of the
        chain, opened at sample og, owns the slots (og >> 5) + j ...; its slot i holds the outputs of samples og + 32 i ..."""
        n = C.c_uint32(0)
        _check(self.L, self.L.tfrec_amd_read_biquad_row(self.h, slot, stream, None, 0, C.byref(n)))
        out = np.empty(32 * n.value, dtype=np.int32)
        _check(self.L, self.L.tfrec_amd_read_biquad_row(self.h, slot, stream, out.ctypes.data, out.size, C.byref(n)))
        return out

    def atan_uncertain(self) -> int:
        n = C.c_uint64(0)
        _check(self.L, self.L.tfrec_amd_atan_uncertain(self.h, C.byref(n)))
        return int(n.value)

    def fm_stats(self) -> dict:
        """fm_dev samples decided by the exact slow path / checked against the host's libm at drain / differing from it /
        too close to an atan2 rounding midpoint for glibc's error bound (tfrec_amd_get_fm_stats)."""
        st = FmStats()
        _check(self.L, self.L.tfrec_amd_get_fm_stats(self.h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in FmStats._fields_[:4]}

    def thresh(self, stream: int) -> int:
        v = C.c_int(0)
        _check(self.L, self.L.tfrec_amd_read_thresh(self.h, stream, C.byref(v)))
        return int(v.value)

    def timings(self) -> dict:
        t = Timings()
        _check(self.L, self.L.tfrec_amd_get_timings(self.h, C.byref(t)))
        return {n: float(getattr(t, n)) for n, _ in Timings._fields_}

    def layout(self) -> int:
        """Internal HIP streams of the pipeline: 6 deep, 4 shallow, 2 serial cross-check (tfrec_amd_get_layout)."""
        n = C.c_int(0)
        _check(self.L, self.L.tfrec_amd_get_layout(self.h, C.byref(n)))
        return int(n.value)

    def memory(self) -> dict:
        """Bytes of device memory / page-locked host memory the context holds (the caller's input batches not counted)."""
        d, h = C.c_uint64(), C.c_uint64()
        _check(self.L, self.L.tfrec_amd_get_memory(self.h, C.byref(d), C.byref(h)))
        return {"device_bytes": int(d.value), "pinned_host_bytes": int(h.value)}

    def stats(self) -> dict:
        """Counters of the speculative stages (how the work was done; results never depend on them)."""
        st = Stats()
        _check(self.L, self.L.tfrec_amd_get_stats(self.h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in Stats._fields_}


def fm_dev_nrzs_probe(records: np.ndarray, device: int = 0) -> np.ndarray:
    """The device's fm_dev_nrzs (dsp_stuff.cpp:269-279) on int32 quadruples [n, 4] = (ar, aj, br, bj) -> int32[n]."""
    L = load_library()
    q = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 4)
    out = np.empty(len(q), dtype=np.int32)
    _check(L, L.tfrec_amd_fm_dev_probe(device, 2, q.ctypes.data, len(q), out.ctypes.data, None))
    return out


def iir_probe(cutoff: float, x: np.ndarray, form: int = 1, device: int = 0) -> np.ndarray:
    """The device's iir2 (dsp_stuff.cpp:28-56) with set(cutoff) over the doubles x from the zero state -> float64[n].
    form 0: iir_step (the reference's association), form 1: iir_step_t (the form the kernels run)."""
    L = load_library()
    xin = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(len(xin), dtype=np.float64)
    _check(L, L.tfrec_amd_iir_probe(device, float(cutoff), int(form), xin.ctypes.data, len(xin), out.ctypes.data))
    return out


def fm_dev_probe(records: np.ndarray, device: int = 0, cross: bool = False):
    """The device's fm_dev (dsp_stuff.cpp:284-292) on int32 quadruples [n, 4] = (ar, aj, br, bj), or (cross=True) on
    int64 cross terms [n, 2] = (cr, cj) -> (int32[n], stats)."""
    L = load_library()
    q = (np.ascontiguousarray(records, dtype=np.int64).reshape(-1, 2) if cross
         else np.ascontiguousarray(records, dtype=np.int32).reshape(-1, 4))
    out = np.empty(len(q), dtype=np.int32)
    st = FmStats()
    _check(L, L.tfrec_amd_fm_dev_probe(device, 1 if cross else 0, q.ctypes.data, len(q), out.ctypes.data, C.byref(st)))
    return out, {n: int(getattr(st, n)) for n, _ in FmStats._fields_[:4]}


def events_canon(events: np.ndarray):
    """Vector form of event_tuples_full for whole batches: (stream[n], int64 matrix [n, 5 + 64 + 2] with the columns slot,
    end_sample, byte_cnt, rssi_db, offset, rdata, rssi_raw, status) -- the layout of oracle.canon()."""
    L = load_library()
    events = events[events["status"] != STATUS_BITS]
    m = np.empty((len(events), 71), dtype=np.int64)
    m[:, 0] = events["slot"]
    m[:, 1] = events["end_sample"]
    m[:, 2] = events["byte_cnt"]
    slots = events["slot"].tolist()
    raws = events["rssi_raw"].tolist()
    m[:, 3] = [L.tfrec_amd_rssi_db(sl, rw) for sl, rw in zip(slots, raws)]
    m[:, 4] = events["offset"]
    m[:, 5:69] = events["rdata"]
    m[:, 69] = events["rssi_raw"]
    m[:, 70] = events["status"]
    return events["stream"].astype(np.int64), m


def bits_by_flush(events: np.ndarray, stream: int):
    """TFREC_AMD_F_BITS: {(slot, seq): "0110..."} -- the bits handed to decoder::store_bit before flush number seq of the
    slot, from the BITS chunks of `events` (drain order; concatenate the drains of consecutive submits first)."""
    out = {}
    for e in events:
        if int(e["stream"]) != stream or int(e["status"]) != STATUS_BITS:
            continue
        n = int(e["byte_cnt"])
        bits = np.unpackbits(e["rdata"], bitorder="little")[:n]
        key = (int(e["slot"]), int(e["seq"]))
        out[key] = out.get(key, "") + "".join("01"[b] for b in bits)
    return out


def event_tuples_full(events: np.ndarray, stream: int | None = None):
    """event_tuples + (rssi_raw, status): the raw RSSI accumulator itself (tfa1.cpp:161, tfa2.cpp:373, whb.cpp:678) and the
    verdict of the decoder's acceptance tests computed on the GPU -- what oracle.Oracle.events_full() returns."""
    L = load_library()
    out = []
    for e in events:
        if (stream is not None and int(e["stream"]) != stream) or int(e["status"]) == STATUS_BITS:
            continue
        out.append((int(e["slot"]), int(e["end_sample"]), int(e["byte_cnt"]),
                    int(L.tfrec_amd_rssi_db(int(e["slot"]), int(e["rssi_raw"]))), int(e["offset"]),
                    bytes(e["rdata"]), int(e["rssi_raw"]), int(e["status"])))
    return out


def event_tuples(events: np.ndarray, stream: int | None = None):
    """Canonical comparable form (slot, end_sample, byte_cnt, rssi_db, offset, rdata) of flush events,
    in per-(stream, slot) order -- the same tuple the oracle and the reference harness produce."""
    L = load_library()
    out = []
    for e in events:
        if (stream is not None and int(e["stream"]) != stream) or int(e["status"]) == STATUS_BITS:
            continue
        out.append((int(e["slot"]), int(e["end_sample"]), int(e["byte_cnt"]),
                    int(L.tfrec_amd_rssi_db(int(e["slot"]), int(e["rssi_raw"]))), int(e["offset"]),
                    bytes(e["rdata"])))
    return out
