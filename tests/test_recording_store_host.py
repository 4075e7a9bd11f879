"""specscan::RecordingStore (host/recording_store.h) through srs_* against a Python restatement kept here (``StoreModel``: the
``gather`` of tests/test_gpu_record_feed.py, the cutting into 100 ms items and the item-time rule of the header), without a GPU.
The plans are test_range_planner_host.py's sessions; the outputs are synthetic int8 made from the sample's index in the slot's
output stream, and the range counts are chosen so that items complete in the middle of ranges, at range ends and from ``pending``
carried across a stop, and several complete in one range. Published (time, frequency, bytes) lists and the drop counts must be
equal. ``StoreModel`` is also the store of the Python route tests/test_gpu_replay_record.py compares ``specscan_replay
--record-out`` with."""
import numpy as np

from rtl_sdr_scanner_cpp_amd.recorder import HostRecordingStore, RangePlanner
from test_range_planner_host import session

CENTER, BW, FS = 145_000_000, 16_000, 1_024_000


def item_samples(bandwidth):
    raw = bandwidth * 100 // 1000  # roundUp(recordingBandwidth * RECORDER_FLUSH_INTERVAL / 1000, 4096), recorder.cpp:35
    return raw if raw % 4096 == 0 else (raw // 4096 + 1) * 4096


class StoreModel:
    """Per slot ``pending`` (less than one item: what sits inside stream_to_vector; it survives stop and start) and ``items``
    (the Buffer: (time, bytes), cleared by a stop). A range that ends with a flush publishes every gathered item of its slot, in
    order; a stop then drops what is left; ``finish`` drops like a stop. The item completed by output q (1-based) of the range's
    ``count`` outputs carries the time of the frame that holds sample begin + ceil(q * (end - begin) / count) - 1 of the batch."""

    def __init__(self, channels, center, bandwidth, stride, frame_time):
        self.center, self.bandwidth, self.stride, self.frame_time = center, bandwidth, stride, frame_time
        self.item = item_samples(bandwidth)
        self.pending = [np.zeros((0, 2), np.int8) for _ in range(channels)]
        self.items = [[] for _ in range(channels)]
        self.published, self.dropped = [], 0
        self.seen = {"mid_range": 0, "at_range_end": 0, "from_pending": 0, "pending_across_stop": 0, "several": 0}
        self._stopped_with_pending = [False] * channels

    def feed(self, rng, end, flush, iq, first_frame):
        ch, shift, begin, stop = (int(v) for v in rng)
        iq = np.asarray(iq, np.int8).reshape(-1, 2)
        count, had = len(iq), len(self.pending[ch])
        stream = np.concatenate([self.pending[ch], iq])
        whole = len(stream) // self.item
        for j in range(whole):
            q = (j + 1) * self.item - had  # the output of this range that completed item j
            p = begin + -(-(q * (stop - begin)) // count) - 1
            p = min(max(p, begin), max(begin, stop - 1))
            self.items[ch].append((int(self.frame_time(first_frame + p // self.stride)), stream[j * self.item:(j + 1) * self.item].tobytes()))
            self.seen["at_range_end" if q == count else "mid_range"] += 1
            if j == 0 and had:
                self.seen["from_pending"] += 1
                self.seen["pending_across_stop"] += self._stopped_with_pending[ch]
        self.seen["several"] += whole > 1
        if whole:
            self._stopped_with_pending[ch] = False
        self.pending[ch] = stream[whole * self.item:]
        if flush:
            self.published += [(t, self.center + shift, self.bandwidth, data) for t, data in self.items[ch]]
            self.items[ch] = []
        if end == "stop":
            self.dropped += len(self.items[ch])
            self.items[ch] = []
            self._stopped_with_pending[ch] = len(self.pending[ch]) > 0

    def finish(self):
        self.dropped += sum(len(x) for x in self.items)
        self.items = [[] for _ in self.items]


def outputs(slot, first, count):
    """int8 [count, 2] from the sample's index in the slot's output stream"""
    j = first + np.arange(count, dtype=np.int64)
    return np.stack([(j * 7 + slot * 31) & 0xff, (j // 256 + j // 4096 * 3) & 0xff], axis=-1).astype(np.uint8).view(np.int8)


def test_item_samples_is_the_reference_rounding():
    assert [item_samples(b) for b in (16_000, 32_000, 40_960, 40_970, 409_600)] == [4096, 4096, 4096, 8192, 40960]
    store = HostRecordingStore(2, CENTER, 40_970, 1024, lambda f: f)
    assert store.item_samples == 8192
    store.close()


def test_sessions_equal_the_restatement():
    total = {}
    for seed in range(120):
        slots, stride, batches = session(seed)
        rng = np.random.default_rng(10_000 + seed)
        frame_time = lambda frame, stride=stride: 1000 * frame * stride // FS  # noqa: E731
        planner = RangePlanner(slots, stride)
        host, model = HostRecordingStore(slots, CENTER, BW, stride, frame_time), StoreModel(slots, CENTER, BW, stride, frame_time)
        assert host.item_samples == model.item == 4096
        produced, first_frame = [0] * slots, 0
        for batch in batches:
            ranges, ends, flushes = planner.plan(batch)
            for r, end, flush in zip(ranges, ends, flushes):
                ch, length = r[0], r[3] - r[2]
                count = length // int(rng.choice([4, 16, 64]))  # long ranges hold several items
                if count and rng.random() < 0.3:
                    count = model.item - len(model.pending[ch]) + model.item * int(rng.integers(0, 2))  # the range ends on an item's last sample
                iq = outputs(ch, produced[ch], count)
                produced[ch] += count
                host.feed(r, end, flush, iq, first_frame)
                model.feed(r, end, flush, iq, first_frame)
                assert host.pending_samples(ch) == len(model.pending[ch]) and host.held_items(ch) == len(model.items[ch])
            first_frame += len(batch)
            assert host.published == model.published, seed
            assert (host.dropped, host.published_items) == (model.dropped, len(model.published)), seed
        host.finish()
        model.finish()
        assert (host.dropped, host.published) == (model.dropped, model.published), seed
        assert model.dropped + len(model.published) == sum(n // model.item for n in produced)
        host.close()
        for k, v in model.seen.items():
            total[k] = total.get(k, 0) + v
        total["published"] = total.get("published", 0) + len(model.published)
        total["dropped"] = total.get("dropped", 0) + model.dropped
    print(total)
    assert min(total.values()) > 10, total


def test_bad_arguments_are_refused_without_an_exception():
    import pytest
    for args in ((0, CENTER, BW, 1024), (17, CENTER, BW, 1024), (2, CENTER, 0, 1024), (2, CENTER, BW, 0)):
        with pytest.raises(ValueError):
            HostRecordingStore(*args, lambda f: f)
    store = HostRecordingStore(2, CENTER, BW, 1024, lambda f: f)
    with pytest.raises(ValueError):
        store.feed((2, 0, 0, 1024), "stop", False, outputs(0, 0, 4), 0)  # a channel the store does not have
    store.feed((1, 0, 0, 0), "batch", True, outputs(0, 0, 0), 0)  # an empty range with no outputs is nothing
    assert store.published == [] and store.dropped == 0
    store.close()
