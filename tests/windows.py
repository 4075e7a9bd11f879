"""Test windows for ss_config.window (a plain helper): taps chosen so that a mistake in a kernel's tap indexing or tap forming shows.

The default Hamming taps cannot show one: hamming_f32 is exactly symmetric (a mirrored tap table gives the same bits) and smooth (at
65536 and 2^20 points a table shifted by one tap or with neighbours swapped leaves the parity contract in < 0.3 % of the bins — the
sizes whose tap tables are permuted by hand). tests/test_window_oracle.py holds the measurement as a test."""
import numpy as np

from parity import hamming_f32


def rough(n, a=0.1, seed=0):
    """hamming * (1 + 0.3 (k / (n - 1) - 0.5)) * (1 + a u_k), u uniform in [-1, 1]: asymmetric and not smooth, so every tap index
    matters (mirrored, shifted by one or pair-swapped taps put > 99 % of the bins outside the contract). In double, stored as float."""
    k = np.arange(n, dtype=np.float64)
    ham = 0.54 - 0.46 * np.cos(2.0 * np.pi * k / (n - 1))
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    return (ham * (1.0 + 0.3 * (k / (n - 1) - 0.5)) * (1.0 + a * u)).astype(np.float32)


def blackman_harris4(n):
    """The 4-term Blackman-Harris window (symmetric form): edge taps of 6e-5, so the taps span four decades."""
    x = 2.0 * np.pi * np.arange(n, dtype=np.float64) / (n - 1)
    return (0.35875 - 0.48829 * np.cos(x) + 0.14128 * np.cos(2 * x) - 0.01168 * np.cos(3 * x)).astype(np.float32)


def rect(n):
    """All ones: every product sample x tap is exact, and whatever forms Hamming taps inside a kernel must be off."""
    return np.ones(n, dtype=np.float32)


WINDOWS = {"rough": rough, "bh4": blackman_harris4, "rect": rect, "hamming": hamming_f32}


def mirrored(w):
    return np.ascontiguousarray(w[::-1])


def rolled(w):
    return np.roll(w, 1)


def pair_swapped(w):
    return np.ascontiguousarray(w.reshape(-1, 2)[:, ::-1]).reshape(-1)
