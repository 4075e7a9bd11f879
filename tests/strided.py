"""Decimated input as ss_process_device takes it: items of N * decim samples of which the chain reads the first N. strided_items puts
compact frames into such items and fills the rest of every item — the gap [N, N * decim) — with values that cannot go unnoticed
where a kernel reads them: a quiet NaN in both parts for CF32 (every bin of the frame becomes NaN), the two extremes of the format
in turn along the interleaved I, Q values for the integer formats (I at one end of the range, Q at the other: a full-scale constant, whose
line at the centre bin stands above every bin a synthetic band holds). The buffer
always holds the whole nframes * N * decim samples: a kernel that strode by N would read poison, never beyond the allocation."""
import numpy as np

FORMATS = {  # fmt: (dtype of the items, the two poison values in turn)
    "cf32": (np.complex64, None),
    "cs8": (np.int8, (127, -128)),
    "cu8": (np.uint8, (0, 255)),
    "cs16": (np.int16, (32767, -32768)),
}


def poison(fmt, count):
    """`count` gap samples of the format: [count] complex64, or [count, 2] integers (the pair alternates along the flattened I, Q order)."""
    dtype, pair = FORMATS[fmt]
    if pair is None:
        return np.full(count, np.nan + 1j * np.nan, dtype=np.complex64)
    return np.tile(np.array(pair, dtype=dtype), count).reshape(count, 2)


def strided_items(frames, decim, fmt):
    """frames: [nframes, N] complex64 (cf32) or [nframes, N, 2] int8 / uint8 / int16 (cs8 / cu8 / cs16), compact.
    Returns [nframes, N * decim(, 2)] of the same dtype, C-contiguous: the frame, bit for bit, then (decim - 1) * N samples of poison."""
    dtype, pair = FORMATS[fmt]
    frames = np.asarray(frames)
    if frames.dtype != dtype or frames.ndim != (2 if pair is None else 3) or (pair is not None and frames.shape[2] != 2):
        raise ValueError(f"{fmt} frames are [nframes, N{'' if pair is None else ', 2'}] {np.dtype(dtype).name}, not {frames.shape} {frames.dtype}")
    if decim < 1:
        raise ValueError("decim >= 1")
    nframes, n = frames.shape[:2]
    out = np.empty((nframes, n * decim) + frames.shape[2:], dtype=dtype)
    out[:, :n] = frames
    if decim > 1:
        out[:, n:] = poison(fmt, n * (decim - 1))[None]
    return out
