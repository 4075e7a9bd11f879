"""A numpy restatement of the tracking digest (include/specscan_track.h; kernels in csrc/track_digest.h), written from the
semantics of the host tracker, not from the kernels:

  window of key k:   [max(0, k - g // 2), min(N, k + g // 2 + 1))
  arg-max:           std::max_element — best = lo; for i in lo + 1 .. hi - 1: if v[best] < v[i]: best = i. The first maximum wins, a NaN at
                     lo wins the window, a NaN anywhere else never wins
  cand_best(f, c):   in each of the ceil(grouping_y / 2) newest rel rows (frames f - R + 1 .. f; frames before the batch from the kept tail,
                     zeros after a reset) the window's arg-max, kept if start_level <= row[best]; of the kept values those with the
                     highest count, ascending, the one at position size // 2; none kept: c
  cand_avg:          avg[f][c]
  watch:             sort(unique(keys U cand_best))
  peak_idx/peak_avg: arg-max and value of avg[f] over the window of every watch key

The CPU tests hold it to the host tracker on the planes (and so to the reference); the GPU tests hold the kernels to it."""
import numpy as np


def argmax_literal(row, lo, hi):
    best = lo
    for i in range(lo + 1, hi):
        if row[best] < row[i]:
            best = i
    return best


def window_argmax(row, keys, half):
    """The arg-max of row over the window of every key, all keys at once: NaNs behind lo never win (they are ranked with -inf, and
    np.argmax takes the first maximum), a first maximum that falls into the padding means every real value is -inf: lo; a NaN at lo: lo."""
    keys = np.asarray(keys, np.int64)
    if keys.size == 0:
        return np.zeros(0, np.int64)
    n = row.shape[0]
    rank = np.where(np.isnan(row), -np.inf, row).astype(np.float32)
    padded = np.concatenate([np.full(half, -np.inf, np.float32), rank, np.full(half, -np.inf, np.float32)])
    windows = np.lib.stride_tricks.sliding_window_view(padded, 2 * half + 1)[keys]  # window w starts at bin keys[w] - half
    lo = np.maximum(0, keys - half)
    best = np.maximum(keys - half + np.argmax(windows, axis=1), lo)
    best = np.minimum(best, n - 1)  # (unreachable: a maximum in the right padding is never the first one)
    return np.where(np.isnan(row[lo]), lo, best)


def most_frequent(values):
    uniq, counts = np.unique(np.asarray(values), return_counts=True)
    tied = uniq[counts == counts.max()]
    return int(tied[tied.size // 2])


class DigestRef:
    def __init__(self, n, group_size, start_level=8.0, grouping_y=21):
        self.n, self.half, self.start = n, group_size // 2, np.float32(start_level)
        self.rows = (grouping_y + 1) // 2
        self.reset()

    def reset(self):
        self.tail = np.zeros((self.rows - 1, self.n), np.float32)

    def digest(self, rel, avg, cand_off, cand_idx, keys):
        rel, avg = np.asarray(rel, np.float32), np.asarray(avg, np.float32)
        nframes = rel.shape[0]
        cand_off = np.asarray(cand_off, np.int64)
        cand_idx = np.asarray(cand_idx, np.int32)
        ext = np.concatenate([self.tail, rel])  # frame f of the batch is row f + rows - 1
        ncand = int(cand_off[nframes])
        cand_best = np.empty(ncand, np.int32)
        cand_avg = np.empty(ncand, np.float32)
        for f in range(nframes):
            a, b = int(cand_off[f]), int(cand_off[f + 1])
            if a == b:
                continue
            c = cand_idx[a:b]
            per_row = []
            for r in range(self.rows):
                row = ext[f + r]
                best = window_argmax(row, c, self.half)
                per_row.append((best, self.start <= row[best]))
            for j in range(b - a):
                kept = [int(best[j]) for best, ok in per_row if ok[j]]
                cand_best[a + j] = most_frequent(kept) if kept else c[j]
            cand_avg[a:b] = avg[f, c]
        watch = np.unique(np.concatenate([np.asarray(keys, np.int32).reshape(-1), cand_best])).astype(np.int32)
        peak_idx = np.empty((nframes, watch.size), np.int32)
        peak_avg = np.empty((nframes, watch.size), np.float32)
        for f in range(nframes):
            peak_idx[f] = window_argmax(avg[f], watch, self.half)
            peak_avg[f] = avg[f, peak_idx[f]]
        if self.rows > 1:
            self.tail = ext[ext.shape[0] - (self.rows - 1):].copy()
        return {"nframes": nframes, "cand_off": cand_off[:nframes + 1].astype(np.int32), "cand_idx": cand_idx[:ncand].copy(), "cand_best": cand_best,
                "cand_avg": cand_avg, "watch": watch, "peak_idx": peak_idx, "peak_avg": peak_avg}


def assert_digest_equal(got, want, what=""):
    """Integers equal, floats bit-equal (NaNs included: compared as their bit patterns)."""
    for k in ("cand_off", "cand_idx", "cand_best", "watch", "peak_idx"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what} {k}")
    for k in ("cand_avg", "peak_avg"):
        np.testing.assert_array_equal(np.asarray(got[k], np.float32).view(np.uint32), np.asarray(want[k], np.float32).view(np.uint32), err_msg=f"{what} {k}")
