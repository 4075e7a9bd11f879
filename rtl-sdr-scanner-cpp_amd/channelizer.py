"""ctypes view of include/specscan_channelizer.h — the recorder channeliser: for every recording slot
of a device, rotator -> cascaded rational resamplers -> int8, what the reference's Recorder builds per slot out of GNU
Radio blocks (reference sources/radio/recorder.cpp:14-46). Test and tooling plumbing; the compute is csrc/channelizer.hip."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import SpecscanError
from .engine import load_library

SC_ABI_VERSION = 1
SC_MAX_CHANNELS = 16

EXPORTS = ("sc_default_config", "sc_create", "sc_destroy", "sc_last_error", "sc_stage_count", "sc_stage_info", "sc_stage_taps",
           "sc_output_capacity", "sc_start", "sc_stop", "sc_is_recording", "sc_process", "sc_process_device", "sc_sync",
           "sc_transmission_payload", "sc_set_input_format", "sc_process_ranges", "sc_process_ranges_device",
           "sc_process_ranges_upload")
SC_MAX_RANGES = 64

# what process() / process_device() take for each input format (ss_format): integers interleaved re,im
_NP_DTYPE = {abi.SS_FMT_CS8: np.int8, abi.SS_FMT_CU8: np.uint8, abi.SS_FMT_CS16: np.int16}


class ScConfig(C.Structure):  # sc_config
    _fields_ = [("abi_version", C.c_uint32), ("sample_rate", C.c_int32), ("bandwidth", C.c_int32), ("threshold", C.c_int32),
                ("channels", C.c_int32), ("max_samples", C.c_int32), ("pack_scale", C.c_float), ("device_id", C.c_int32)]


class ScRange(C.Structure):  # sc_range
    _fields_ = [("channel", C.c_int32), ("shift_hz", C.c_int32), ("begin", C.c_int32), ("end", C.c_int32)]


def _ranges(ranges):
    """[(channel, shift_hz, begin, end), ...] or ScRange objects -> a C array of sc_range (None when empty)."""
    rs = [r if isinstance(r, ScRange) else ScRange(*(int(v) for v in r)) for r in ranges]
    return ((ScRange * len(rs))(*rs) if rs else None), len(rs)


def _bind(lib):
    if getattr(lib, "_sc_bound", False):
        return lib
    i32p = C.POINTER(C.c_int32)
    lib.sc_default_config.argtypes = [C.POINTER(ScConfig), C.c_int32, C.c_int32]
    lib.sc_default_config.restype = None
    lib.sc_create.argtypes = [C.POINTER(ScConfig), C.POINTER(C.c_void_p)]
    lib.sc_destroy.argtypes = [C.c_void_p]
    lib.sc_destroy.restype = None
    lib.sc_last_error.argtypes = [C.c_void_p]
    lib.sc_last_error.restype = C.c_char_p
    lib.sc_stage_count.argtypes = [C.c_void_p]
    lib.sc_stage_info.argtypes = [C.c_void_p, C.c_int32, i32p, i32p, i32p]
    lib.sc_stage_taps.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_float)]
    lib.sc_output_capacity.argtypes = [C.c_void_p, C.c_int32]
    lib.sc_output_capacity.restype = C.c_int32
    lib.sc_start.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.sc_stop.argtypes = [C.c_void_p, C.c_int32]
    lib.sc_is_recording.argtypes = [C.c_void_p, C.c_int32]
    lib.sc_process.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, i32p, C.c_int32]
    lib.sc_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, i32p, C.c_int32]
    lib.sc_sync.argtypes = [C.c_void_p]
    if hasattr(lib, "sc_process_ranges"):  # (A/B builds of older trees, scripts/ab: measurement runs only)
        lib.sc_process_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ScRange), C.c_int32, C.c_void_p, C.c_void_p, i32p, i32p, C.c_int32]
        lib.sc_process_ranges_device.argtypes = lib.sc_process_ranges.argtypes
    if hasattr(lib, "sc_process_ranges_upload"):
        lib.sc_process_ranges_upload.argtypes = lib.sc_process_ranges.argtypes + [C.POINTER(C.c_uint64)]
    lib.sc_set_input_format.argtypes = [C.c_void_p, C.c_int32, C.c_float]
    lib.sc_transmission_payload.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    lib._sc_bound = True
    return lib


def transmission_payload(time_ms: int, frequency: int, sample_rate: int, iq_i8: np.ndarray) -> bytes:
    """DataController::pushTransmission's MQTT payload (reference sources/network/data_controller.cpp:27-42)."""
    lib = _bind(load_library())
    a = np.ascontiguousarray(iq_i8, dtype=np.int8).reshape(-1, 2)
    n = lib.sc_transmission_payload(time_ms, frequency, sample_rate, None, a.shape[0], None, 0)
    out = np.zeros(n, np.uint8)
    got = lib.sc_transmission_payload(time_ms, frequency, sample_rate, a.ctypes.data, a.shape[0], out.ctypes.data, n)
    if got != n:
        raise ValueError("payload")
    return out.tobytes()


class Channelizer:
    """All recording slots of one device (Recorder x recordersCount, reference sources/radio/sdr_device.cpp:39-41)."""

    def __init__(self, sample_rate: int, bandwidth: int, in_format: int = abi.SS_FMT_CF32, int_scale: float = 0.0, **overrides):
        self._lib = _bind(load_library())
        cfg = ScConfig()
        self._lib.sc_default_config(C.byref(cfg), int(sample_rate), int(bandwidth))
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown sc_config field {k}")
            setattr(cfg, k, v)
        self.cfg = cfg
        h = C.c_void_p()
        st = self._lib.sc_create(C.byref(cfg), C.byref(h))
        if st != 0:
            raise SpecscanError(st, (self._lib.sc_last_error(None) or b"").decode())
        self._h = h
        self.stages = []
        for s in range(self._lib.sc_stage_count(h)):
            i, d, t = C.c_int32(), C.c_int32(), C.c_int32()
            self._lib.sc_stage_info(h, s, C.byref(i), C.byref(d), C.byref(t))
            self.stages.append((i.value, d.value, t.value))
        self.in_format = abi.SS_FMT_CF32
        self.set_input_format(in_format, int_scale)

    def set_input_format(self, fmt: int, scale: float = 0.0):
        """sc_set_input_format: the ss_format of the stream from the next call on (0 scale: the format's full-scale default)."""
        self._check(self._lib.sc_set_input_format(self._h, int(fmt), float(scale)))
        self.in_format = int(fmt)

    def _check(self, st):
        if st != 0:
            raise SpecscanError(st, (self._lib.sc_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.sc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stage_taps(self, stage: int) -> np.ndarray:
        t = np.zeros(self.stages[stage][2], np.float32)
        self._check(self._lib.sc_stage_taps(self._h, stage, t.ctypes.data_as(C.POINTER(C.c_float))))
        return t

    def output_capacity(self, nsamples: int) -> int:
        return int(self._lib.sc_output_capacity(self._h, int(nsamples)))

    def start(self, channel: int, shift_hz: int):
        self._check(self._lib.sc_start(self._h, int(channel), int(shift_hz)))

    def stop(self, channel: int):
        self._check(self._lib.sc_stop(self._h, int(channel)))

    def is_recording(self, channel: int) -> bool:
        return bool(self._lib.sc_is_recording(self._h, int(channel)))

    def _host_input(self, iq) -> tuple:
        """The stream as the library reads it, and its sample count. An integer dtype must be the format's own: bytes are never
        reinterpreted and integers never converted here."""
        want = _NP_DTYPE.get(self.in_format)
        dt = np.asarray(iq).dtype
        if want is None:
            if dt.kind in "iu":
                raise TypeError(f"{dt} samples given to a CF32 channeliser (set_input_format first)")
            x = np.ascontiguousarray(iq, dtype=np.complex64)
            return x, x.size
        if dt != want:
            raise TypeError(f"input format {self.in_format} takes interleaved {np.dtype(want)} (re, im), not {dt}")
        x = np.ascontiguousarray(iq)
        if x.size % 2 or (x.ndim > 1 and x.shape[-1] != 2):
            raise ValueError("integer samples are (n, 2) or flat interleaved re, im")
        return x, x.size // 2

    def process(self, iq: np.ndarray, want_cf32: bool = True):
        """iq: the device stream — complex64 [n] (CF32), or int8 / uint8 / int16 [n, 2] or flat interleaved [2n] for CS8 / CU8 /
        CS16. Returns {channel: (int8 [m, 2], complex64 [m] or None)} for the active slots."""
        x, nsamples = self._host_input(iq)
        cap = max(self.output_capacity(nsamples), 1)
        nch = self.cfg.channels
        i8 = np.zeros((nch, cap, 2), np.int8)
        cf = np.zeros((nch, cap), np.complex64) if want_cf32 else None
        counts = np.zeros(nch, np.int32)
        self._check(self._lib.sc_process(self._h, x.ctypes.data, nsamples, i8.ctypes.data, cf.ctypes.data if want_cf32 else None,
                                         counts.ctypes.data_as(C.POINTER(C.c_int32)), cap))
        return {ch: (i8[ch, :counts[ch]].copy(), cf[ch, :counts[ch]].copy() if want_cf32 else None)
                for ch in range(nch) if self.is_recording(ch)}

    def process_device(self, iq, nsamples: int, out_i8=None, out_cf32=None, cap: int = 0):
        """torch tensors on this context's device (plain HBM allocations); iq in the context's format: float32 / complex64 (CF32),
        int8 (CS8), uint8 (CU8), int16 (CS16), interleaved re, im. Returns the per-channel counts (numpy); async: call sync()."""
        if iq is not None:
            import torch
            want = {abi.SS_FMT_CS8: (torch.int8,), abi.SS_FMT_CU8: (torch.uint8,), abi.SS_FMT_CS16: (torch.int16,)}.get(
                self.in_format, (torch.float32, torch.complex64))
            if iq.dtype not in want:
                raise TypeError(f"input format {self.in_format} takes a {want[0]} tensor, not {iq.dtype}")
        counts = np.zeros(self.cfg.channels, np.int32)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self._check(self._lib.sc_process_device(self._h, p(iq), int(nsamples), p(out_i8), p(out_cf32),
                                                counts.ctypes.data_as(C.POINTER(C.c_int32)), int(cap)))
        return counts

    def process_ranges(self, iq: np.ndarray, ranges, want_cf32: bool = True, cap: int | None = None):
        """sc_process_ranges: iq as process() takes it; ranges = [(channel, shift_hz, begin, end), ...] in samples of iq.
        Returns ({channel: (int8 [m, 2], complex64 [m] or None)} for every channel with a range, range_counts): a channel's
        ranges concatenated, range_counts[i] outputs from ranges[i]. With cap below a channel's total only cap are kept."""
        x, nsamples = self._host_input(iq)
        arr, n = _ranges(ranges)
        cap = max(self.output_capacity(nsamples), 1) if cap is None else int(cap)
        nch = self.cfg.channels
        i8 = np.zeros((nch, max(cap, 1), 2), np.int8)
        cf = np.zeros((nch, max(cap, 1)), np.complex64) if want_cf32 else None
        counts = np.zeros(nch, np.int32)
        rc = np.zeros(max(n, 1), np.int32)
        i32p = C.POINTER(C.c_int32)
        self._check(self._lib.sc_process_ranges(self._h, x.ctypes.data, nsamples, arr, n, i8.ctypes.data, cf.ctypes.data if want_cf32 else None,
                                                counts.ctypes.data_as(i32p), rc.ctypes.data_as(i32p), cap))
        kept = np.minimum(counts, cap)
        chans = sorted({int(arr[i].channel) for i in range(n)})
        return ({ch: (i8[ch, :kept[ch]].copy(), cf[ch, :kept[ch]].copy() if want_cf32 else None) for ch in chans}, rc[:n].copy())

    def process_ranges_device(self, iq, nsamples: int, ranges, out_i8=None, out_cf32=None, cap: int = 0):
        """sc_process_ranges_device: tensors as process_device() takes them. Returns (counts, range_counts) (numpy); async: sync()."""
        if iq is not None:
            import torch
            want = {abi.SS_FMT_CS8: (torch.int8,), abi.SS_FMT_CU8: (torch.uint8,), abi.SS_FMT_CS16: (torch.int16,)}.get(
                self.in_format, (torch.float32, torch.complex64))
            if iq.dtype not in want:
                raise TypeError(f"input format {self.in_format} takes a {want[0]} tensor, not {iq.dtype}")
        arr, n = _ranges(ranges)
        counts = np.zeros(self.cfg.channels, np.int32)
        rc = np.zeros(max(n, 1), np.int32)
        i32p = C.POINTER(C.c_int32)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self._check(self._lib.sc_process_ranges_device(self._h, p(iq), int(nsamples), arr, n, p(out_i8), p(out_cf32),
                                                       counts.ctypes.data_as(i32p), rc.ctypes.data_as(i32p), int(cap)))
        return counts, rc[:n].copy()

    def process_ranges_upload(self, iq: np.ndarray, ranges, out_i8=None, out_cf32=None, cap: int = 0):
        """sc_process_ranges_upload: iq on the host as process() takes it, outputs as process_ranges_device() takes them; only the
        union of the ranges is uploaded. Returns (counts, range_counts, uploaded_bytes). Waits (sync()) before it returns, so iq
        need not outlive the call."""
        x, nsamples = self._host_input(iq)
        arr, n = _ranges(ranges)
        counts = np.zeros(self.cfg.channels, np.int32)
        rc = np.zeros(max(n, 1), np.int32)
        up = C.c_uint64(0)
        i32p = C.POINTER(C.c_int32)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        self._check(self._lib.sc_process_ranges_upload(self._h, x.ctypes.data, nsamples, arr, n, p(out_i8), p(out_cf32),
                                                       counts.ctypes.data_as(i32p), rc.ctypes.data_as(i32p), int(cap), C.byref(up)))
        self.sync()
        return counts, rc[:n].copy(), int(up.value)

    def sync(self):
        self._check(self._lib.sc_sync(self._h))
