"""SS_FLAG_SPECTROGRAM at the long transform sizes (16384 .. 2^20 points), where the flag changes which scan runs (csrc/scan_form.h,
decide_form; csrc/specscan.hip, run_batch): the radix-8 / radix-16 fold is refused (fold_ok), 262144 points leave the culled
256 x 1024 chain (x256_ok), a 65536- or 2^20-point context stays cull_long but makes no plan, takes no ring-only call and no merged
launch, and the accumulation itself is the SPEC = true form of the detect stage — riding one or two launches behind its call — or
the two stand-alone kernels. Per case three sessions over one stream and one ragged cut into calls: device calls with a sync() after
each, the same device calls back to back (a read without a sync, a retune and a retune back on the way), and host calls that hand
out the planes. Held to: each other (bits), a context without the flag (bits, CF32 rows), the oracle chain with one
orc_spectrogram_* accumulator per centre, and an fp64 restatement of the accumulation on the engine's own dB plane.
Needs an MI355X: run with -m gpu (-s prints the figures)."""
import ctypes as C

import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from parity import check_all, check_candidates, dont_care_limit, error_quantiles, format_quantiles
from test_gpu_cs16 import CENTER, _ragged, _retune, _same

pytestmark = pytest.mark.gpu

A = pkg.abi
CF32, CS8, CU8 = A.SS_FMT_CF32, A.SS_FMT_CS8, A.SS_FMT_CU8
FRAMES = {CF32: "frames_cf32", CS8: "frames_cs8", CU8: "frames_cu8"}
CAND_PER_FRAME = 2048  # capacity of a call's candidate buffers, per frame (four 48-bin combs widened by the 21-bin mean: ~300 a frame)

# The form each row reaches, read from decide_form and run_batch with SS_FLAG_SPECTROGRAM set (m = n / ss_spectrogram_size):
#   16384 cf32      m 4    step_path, no culling: the 256-point column half as k_scan_step's FFT role, detect(k - 1) and emit(k - 2) riding
#   32768 cu8       m 4    the same, int8 load
#   65536 cf32      m 4    det_lag2 + rows256_step + cull_long: run maxima written, hist_by_fft, NO plan (!spec), no ring-only call, no merged
#                          launch; detect(k - 2) on the column launch of call k reads the internal PSD plane (of two) that call k's row
#                          launch writes behind it: run_batch's `clashes` check drains first, every second overlapped call
#   65536 cs8       m 4    fold refused (fold_ok) -> the same four-step form with the int8 load
#   131072 cs8      m 8    fold refused -> det_lag2 off, tw_rowsR (512-point rows), cull_long off: four-step int8, not culled
#   262144 cf32     m 16   x256_ok false -> det_lag2 off, cull_long off; x256_tile rows (k_fft_rows1024_psd<8>) behind the column launch
#   2^20 cf32       m 64   two_pass, cull_long without a plan: the row half as the FFT role, detect(k - 1) riding
#   65536 @ 128 kS/s m 512 spec_in_detect false (m > 256): k_spec_partial / k_spec_combine behind the step path's launches
#   65536 gy = 3    m 4    not fused -> no step path: launch_fft, the stand-alone kernels, run_backend_unfused
# columns: id, n, fs, in_format, grouping_y, nframes, learn_frames, max_batch, largest call, seed of the cut
# (nframes and seed: a stream as short as the averager allows — it hands out -100 until 21 frames are in, so the ORACLE alone lists its
# first candidates at frame learn + 17 — and a cut of it with at least six calls behind the learning call that puts more than 50 of the
# oracle's candidates, in two calls or more, between the learning call and the retune; found with _plan and _oracle below on
# the CPU, the engine not involved. The largest call is below max_batch so that a 32- or 40-frame stream makes eleven or twelve calls.)
CASES = [
    ("16384_cf32", 16384, 4_096_000, CF32, 21, 40, 4, 12, 8, 0),
    ("32768_cu8", 32768, 6_000_000, CU8, 21, 40, 5, 16, 8, 0),
    ("65536_cf32", 65536, 20_000_000, CF32, 21, 40, 6, 25, 8, 0),
    ("65536_cs8", 65536, 20_000_000, CS8, 21, 40, 4, 12, 8, 0),
    ("131072_cs8", 131072, 20_000_000, CS8, 21, 40, 4, 20, 8, 0),
    ("262144_cf32", 262144, 61_440_000, CF32, 21, 32, 3, 12, 4, 28),
    ("1048576_cf32", 1 << 20, 61_440_000, CF32, 21, 32, 3, 12, 4, 28),
    ("65536_cf32_m512", 65536, 128_000, CF32, 21, 40, 4, 16, 8, 0),
    ("65536_cf32_gy3", 65536, 20_000_000, CF32, 3, 40, 5, 16, 8, 0),
]
EXPECT_M = {"16384_cf32": 4, "32768_cu8": 4, "65536_cf32": 4, "65536_cs8": 4, "131072_cs8": 8, "262144_cf32": 16, "1048576_cf32": 64,
            "65536_cf32_m512": 512, "65536_cf32_gy3": 4}


def _plan(nframes, learn, largest, seed):
    """The cut into calls and what happens between them: the learning frames as a call of their own, ragged calls behind it (a one-frame
    call put in where the draw has none), a read ahead of call K // 2, a retune ahead of call 2 K // 3, the retune back three calls
    later (at the latest ahead of the last call), and at the end a read under each centre.
    Returns (call sizes, ops); ops: ("call", k) | ("read",) | ("tune", centre index, reset)."""
    rng = np.random.default_rng(seed)
    chunks = [learn] + _ragged(nframes - learn - 1, largest, rng)
    if 1 in chunks[1:]:
        chunks[-1] += 1
    else:
        chunks.insert(1 + (len(chunks) - 1) // 2, 1)
    k_all = len(chunks)
    read_at, tune_at = k_all // 2, (2 * k_all) // 3
    back_at = min(tune_at + 3, k_all - 1)
    ops = []
    for k in range(k_all):
        if k == read_at:
            ops.append(("read",))
        if k == tune_at:
            ops.append(("tune", 1, True))
        if k == back_at:
            ops.append(("tune", 0, True))
        ops.append(("call", k))
    ops += [("read",), ("tune", 1, False), ("read",)]  # (the last retune only selects the other centre's container)
    return chunks, ops


def _tune(e, fs, centre, reset):
    if centre == 1:
        _retune(fs)(e) if reset else e.set_frequency_range(CENTER + fs // 2, CENTER + fs + fs // 2)
    else:
        e.set_frequency_range(CENTER - fs // 2, CENTER + fs // 2)
        if reset:
            e.reset()


def _stream(case):
    cid, n, fs, fmt, gy, nframes, learn, max_batch, largest, seed = case
    band = pkg.synth.SyntheticBand(n, seed=n % 89 + gy + fmt, on_frame=learn + 3, off_frame=nframes + 1)
    return getattr(band, FRAMES[fmt])(nframes)


def _kw(case, flags):
    cid, n, fs, fmt, gy, nframes, learn, max_batch, largest, seed = case
    return dict(fft_size=n, decim=1, in_format=fmt, grouping_y=gy, learn_frames=learn, max_batch=max_batch, flags=flags)


def _cat(outs, planes):
    res = {k: np.concatenate([o[k] for o in outs]) for k in planes + ("cand_idx", "cand_avg")}
    counts = np.concatenate([np.diff(o["cand_off"]) for o in outs])
    res["cand_off"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return res


def _oracle(O, case, iq, chunks, ops):
    """oracle_chain over the same calls and retunes, one orc_spectrogram_* accumulator per centre fed with the oracle's dB rows.
    Returns (planes and lists of the whole stream, lists per call, reads as (row, means, count), the frames behind each read)."""
    cid, n, fs = case[:3]
    L = O.lib()
    orc = O.oracle_chain(fs, CENTER, **_kw(case, 0))
    acc = [L.orc_spectrogram_create(n, fs), L.orc_spectrogram_create(n, fs)]
    size = L.orc_spectrogram_size(acc[0])
    since = [[], []]  # frames accumulated under each centre since its last read
    starts = np.concatenate([[0], np.cumsum(chunks)])
    centre, outs, reads, read_frames = 0, [], [], []
    for op in ops:
        if op[0] == "call":
            a, b = starts[op[1]], starts[op[1] + 1]
            o = orc.process(iq[a:b])
            for row in o["psd"]:
                L.orc_spectrogram_process(acc[centre], row.ctypes.data_as(C.POINTER(C.c_float)))
            since[centre] += list(range(a, b))
            outs.append(o)
        elif op[0] == "tune":
            centre = op[1]
            _tune(orc, fs, centre, op[2])
        else:
            row, mean = np.zeros(size, np.int8), np.zeros(size, np.float32)
            cnt = L.orc_spectrogram_send(acc[centre], row.ctypes.data_as(C.POINTER(C.c_int8)), mean.ctypes.data_as(C.POINTER(C.c_float)))
            assert cnt == len(since[centre]) > 0
            reads.append((row, mean, cnt))
            read_frames.append(since[centre])
            since[centre] = []
    for g in acc:
        L.orc_spectrogram_destroy(g)
    orc.close()
    return _cat(outs, ("psd", "rel", "avg")), outs, reads, read_frames


def _device_session(case, flags, d_iq, chunks, ops, every_call_synced):
    """process_device with candidate buffers only. every_call_synced: sync() behind every call; otherwise back to back, sync() at the
    end alone — a read in between drains by itself. Returns (lists per call, reads, ss_get_stats)."""
    import torch
    cid, n, fs = case[:3]
    dev = d_iq[0].device
    eng = pkg.SpectrumEngine(fs, CENTER, **_kw(case, flags))
    try:
        outs = [(torch.full((s + 1,), -1, dtype=torch.int32, device=dev), torch.full((s * CAND_PER_FRAME,), -1, dtype=torch.int32, device=dev),
                 torch.full((s * CAND_PER_FRAME,), -7.0, dtype=torch.float32, device=dev)) for s in chunks]
        torch.cuda.synchronize()  # (torch fills these on ITS stream: they must have landed before the engine writes on its own)
        reads = []
        for op in ops:
            if op[0] == "call":
                off, idx, cav = outs[op[1]]
                eng.process_device(d_iq[op[1]], chunks[op[1]], cand_off=off, cand_idx=idx, cand_avg=cav)
                if every_call_synced:
                    eng.sync()
            elif op[0] == "tune":
                _tune(eng, fs, op[1], op[2])
            elif flags & A.SS_FLAG_SPECTROGRAM:
                reads.append(eng.spectrogram_read())
        eng.sync()
        stats = eng.stats()
        lists = []
        for off, idx, cav in outs:
            off = off.cpu().numpy()
            assert off[0] == 0 and 0 <= off[-1] <= idx.numel(), (cid, off[0], off[-1])
            lists.append({"cand_off": off, "cand_idx": idx[:off[-1]].cpu().numpy(), "cand_avg": cav[:off[-1]].cpu().numpy()})
    finally:
        eng.close()
    return lists, reads, stats


def _host_session(case, iq, chunks, ops):
    cid, n, fs = case[:3]
    eng = pkg.SpectrumEngine(fs, CENTER, **_kw(case, A.SS_FLAG_SPECTROGRAM))
    try:
        size = eng._lib.ss_spectrogram_size(eng._h)
        starts = np.concatenate([[0], np.cumsum(chunks)])
        outs, reads = [], []
        for op in ops:
            if op[0] == "call":
                outs.append(eng.process(iq[starts[op[1]]:starts[op[1] + 1]], want=("psd", "rel", "avg")))
            elif op[0] == "tune":
                _tune(eng, fs, op[1], op[2])
            else:
                reads.append(eng.spectrogram_read())
    finally:
        eng.close()
    return _cat(outs, ("psd", "rel", "avg")), reads, size


def _restated_means(psd, frames, m):
    """Spectrogram::process on the engine's own dB rows in fp64: the mean over each group of m bins, summed over the frames, / count."""
    rows = psd[np.asarray(frames)].astype(np.float64)
    return rows.reshape(len(frames), -1, m).mean(axis=2).sum(axis=0) / len(frames)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_spectrogram_branch_at_long_sizes(oracle_mod, case):
    import torch
    cid, n, fs, fmt, gy, nframes, learn, max_batch, largest, seed = case
    dev = torch.device("cuda:0")
    iq = _stream(case)
    chunks, ops = _plan(nframes, learn, largest, seed)
    k_all = len(chunks)
    assert sum(chunks) == nframes and max(chunks) <= max_batch and chunks[0] == learn and 1 in chunks[1:] and k_all >= 7
    assert any(sum(chunks[:k]) % 16 for k in range(1, k_all))  # (batches that start inside a 16-frame tile)
    starts = np.concatenate([[0], np.cumsum(chunks)])
    ref, ref_calls, ref_reads, read_frames = _oracle(oracle_mod, case, iq, chunks, ops)
    assert max(int(o["cand_off"][-1]) // len(o["cand_off"][1:]) for o in ref_calls) < CAND_PER_FRAME // 2
    before_retune = sum(1 for op in ops[:ops.index(("tune", 1, True))] if op[0] == "call")
    assert sum(1 for o in ref_calls[1:before_retune] if o["cand_off"][-1] > 0) >= 2  # (the oracle's candidates fall into calls that overlap)

    d_iq = []
    for k in range(k_all):
        chunk = np.ascontiguousarray(iq[starts[k]:starts[k + 1]])
        d_iq.append(torch.from_numpy(chunk.view(np.float32) if fmt == CF32 else chunk).to(dev))
    spec = A.SS_FLAG_SPECTROGRAM
    l1, r1, _ = _device_session(case, spec, d_iq, chunks, ops, every_call_synced=True)
    l2, r2, stats = _device_session(case, spec, d_iq, chunks, ops, every_call_synced=False)
    l4 = _device_session(case, 0, d_iq, chunks, ops, every_call_synced=False)[0] if fmt == CF32 else None
    del d_iq
    got3, r3, size = _host_session(case, iq, chunks, ops)
    m = n // size
    assert m == EXPECT_M[cid] and size == ref_reads[0][0].size

    # --- no tolerance involved ---
    for k in range(k_all):
        for key in ("cand_off", "cand_idx", "cand_avg"):
            _same(f"{cid} call {k} {key}: overlapped against call by call", l2[k][key], l1[k][key])
            if l4 is not None:
                # (culling, ring-only calls and the merged launch are exact decisions over the same transform kernels; the int8 rows at
                # 65536 and 131072 points are exempt: there the plain context takes the radix-8 / radix-16 fold, another transform)
                _same(f"{cid} call {k} {key}: with the flag against without", l2[k][key], l4[k][key])
    assert len(r1) == len(r2) == len(r3) == len(ref_reads) == 3
    for j, (a, b, c3, r) in enumerate(zip(r1, r2, r3, ref_reads)):
        assert a[2] == b[2] == c3[2] == r[2] > 0, (cid, j, a[2], b[2], c3[2], r[2])
        _same(f"{cid} read {j} row", b[0], a[0])
        _same(f"{cid} read {j} means", b[1], a[1])

    # --- against the oracle ---
    errs, ncand, ndc = check_all(got3, ref, gy=gy)
    got2 = _cat(l2, ())
    ncand2, ndc2 = check_candidates(got2["cand_off"], got2["cand_idx"], ref["cand_off"], ref["cand_idx"], ref["avg"], 8.0)
    print(f"\n{cid}: m {m}, {k_all} calls {chunks}; {ncand} reference candidates, inside the 1e-3 dB band: {ndc} (planes session) {ndc2} (overlapped session); "
          f"|err| dB: {format_quantiles(error_quantiles(got3, ref))}")
    assert ncand > 50 and ncand2 == ncand
    assert ndc <= dont_care_limit(ncand) and ndc2 <= dont_care_limit(ncand), (ncand, ndc, ndc2)
    for j, r in enumerate(ref_reads):
        frac = np.abs(r[1] - np.trunc(r[1]))
        decided = (frac > 1e-3) & (frac < 1 - 1e-3)
        assert decided.mean() > 0.99
        for name, g in (("call by call", r1[j]), ("overlapped", r2[j]), ("planes", r3[j])):
            err = float(np.max(np.abs(g[1].astype(np.float64) - r[1])))
            print(f"{cid} read {j} ({r[2]} frames) {name}: max |mean - oracle| {err:.2e} dB, {int((g[0] != r[0]).sum())} of {size} bytes differ")
            assert err < 1e-4 * 60, (cid, j, name, err)
            np.testing.assert_array_equal(g[0][decided], r[0][decided], err_msg=f"{cid} read {j} {name}")

    # --- against an fp64 restatement of the engine's own plane ---
    # (first-order bound of fp32 recursive summation of m terms, a division, `count` terms and a division, whatever the order of additions)
    for j, frames in enumerate(read_frames):
        want = _restated_means(got3["psd"], frames, m)
        bound = (m + len(frames) + 1) * 2.0 ** -24 * float(np.abs(got3["psd"][np.asarray(frames)]).max())
        err3 = float(np.max(np.abs(r3[j][1].astype(np.float64) - want)))
        err2 = float(np.max(np.abs(r2[j][1].astype(np.float64) - want)))
        print(f"{cid} read {j}: means against the fp64 restatement of the handed-out dB plane: {err3:.2e} dB = {err3 / bound:.3f} of the summation bound {bound:.2e} "
              f"(overlapped session, no plane handed out: {err2 / bound:.3f})")
        assert err3 <= bound, (cid, j, err3, bound)
    print(f"{cid} overlapped session: calls {stats['calls']}, calls_overlapped {stats['calls_overlapped']}, drains {stats['drains']}")
