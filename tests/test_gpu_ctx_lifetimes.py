"""A context created where another one has just been destroyed computes what the first one computed, bit for bit: the memory it is
handed holds the first lifetime's data, so a buffer ss_create must zero and does not (alloc_ctx_buffers, csrc/ctx_buffers.h) shows up as
a difference in the candidate lists, the ring rows ss_read_window hands out or the spectrogram row. One case per family of forms: the
8192-point deep pipeline, the same with the spectrogram in the detect tiles, the radix-8 fold of 65536-point int8 frames, and the unfused
back end of another grouping. Parity with the reference for these shapes is held elsewhere (test_gpu_parity.py,
test_gpu_stated_configs.py). Needs an MI355X: run with -m gpu."""
import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg

pytestmark = pytest.mark.gpu

CENTER = 145_000_000
CASES = {
    "8192_cf32": dict(n=8192, fs=2_048_000, nb=64, cs8=False, cfg={}),
    "8192_spectrogram": dict(n=8192, fs=2_048_000, nb=64, cs8=False, cfg=dict(flags=pkg.abi.SS_FLAG_SPECTROGRAM)),
    "65536_cs8": dict(n=65536, fs=20_000_000, nb=16, cs8=True, cfg=dict(in_format=pkg.abi.SS_FMT_CS8)),
    "256_5x3": dict(n=256, fs=64_000, nb=64, cs8=False, cfg=dict(grouping_x=5, grouping_y=3)),
}
CALLS = 3


def _frames(rng, count, n, amplitude, cs8):
    z = rng.standard_normal((count, n, 2)).astype(np.float32) * np.float32(amplitude)
    if cs8:
        return np.clip(np.rint(z * 128.0), -127, 127).astype(np.int8)
    return np.ascontiguousarray(z).view(np.complex64).reshape(count, n)


def _lifetime(case, learn_iq, learn_t, loud):
    """One context from ss_create to ss_destroy: a learning call (the host entry point, with its clock), CALLS device calls, and
    everything a caller can read back."""
    import torch
    dev = torch.device("cuda", 0)
    n, nb = case["n"], case["nb"]
    eng = pkg.SpectrumEngine(case["fs"], CENTER, fft_size=n, decim=1, max_batch=nb, **case["cfg"])
    out = {}
    first = eng.process(learn_iq, t_ms=learn_t, want=("psd",))
    out["learn_psd"], out["learn_off"] = first["psd"], first["cand_off"]
    d_iq = [torch.from_numpy(loud[k].view(np.float32) if not case["cs8"] else loud[k]).to(dev) for k in range(CALLS)]
    sets = [dict(off=torch.zeros(nb + 1, dtype=torch.int32, device=dev), idx=torch.zeros(nb * n, dtype=torch.int32, device=dev),
                 avg=torch.zeros(nb * n, dtype=torch.float32, device=dev)) for _ in range(CALLS)]
    torch.cuda.synchronize()
    for k in range(CALLS):
        eng.process_device(d_iq[k], nb, cand_off=sets[k]["off"], cand_idx=sets[k]["idx"], cand_avg=sets[k]["avg"])
    eng.sync()
    for k, s in enumerate(sets):
        off = s["off"].cpu().numpy()
        out[f"off{k}"], out[f"idx{k}"], out[f"avg{k}"] = off, s["idx"].cpu().numpy()[:off[-1]], s["avg"].cpu().numpy()[:off[-1]].view(np.uint32)
    for f in (-2, -1, 0, nb - 1):  # ring rows from before the last call, and rows of the last call
        out[f"rel{f}"] = eng.read_window(pkg.abi.SS_PLANE_REL, f, 0, n).view(np.uint32)
    if case["cfg"].get("flags", 0) & pkg.abi.SS_FLAG_SPECTROGRAM:
        row, mean, count = eng.spectrogram_read()
        out["spec_row"], out["spec_mean"], out["spec_count"] = row, mean.view(np.uint32), np.array([count])
    eng.close()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_a_second_lifetime_computes_what_the_first_did(name):
    case = CASES[name]
    n, nb = case["n"], case["nb"]
    rng = np.random.default_rng(20241020)
    learn_iq = _frames(rng, 16, n, 0.01, case["cs8"])
    learn_t = (1_000 + 250 * np.arange(16)).astype(np.int64)  # NOISE_LEARNING_TIME (2000 ms) ends with frame 8
    loud = [_frames(rng, nb, n, 0.01 * (4.0 + 2.0 * k), case["cs8"]) for k in range(CALLS)]
    one = _lifetime(case, learn_iq, learn_t, loud)
    two = _lifetime(case, learn_iq, learn_t, loud)
    assert sum(int(one[f"off{k}"][-1]) for k in range(CALLS)) > nb * n  # loud: the lists are long, every stage has had work
    assert one.keys() == two.keys()
    for key in one:
        np.testing.assert_array_equal(one[key], two[key], err_msg=f"{name}: {key} differs between the first and the second lifetime")
