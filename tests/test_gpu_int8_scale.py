"""CS8 / CU8 input under a caller's ss_config.int_scale (1.0, 1/100, 0.0123 — not the defaults 1/128 and 1/127.5 every other int8
test runs at), against the oracle under the same scale and, on every path but the fold, bit for bit against a CF32 engine fed
((float)p - offset) * (float)scale: every load stage in csrc/ writes exactly that expression. The radix-8 / radix-16 fold (65536 and
131072 points, calls that hand out no plane) multiplies the scale into its twiddle table in double (dif8_host_tables) instead, so it
is held to the oracle alone. Run with -m gpu."""
import numpy as np
import pytest

import rtl_sdr_scanner_cpp_amd as pkg
from parity import check_all, dont_care_limit, error_quantiles, format_quantiles
from test_gpu_cs16 import KEYS, _ragged, _same

pytestmark = pytest.mark.gpu

A = pkg.abi
CENTER = 145_000_000
SCALES = [1.0, 1.0 / 100, 0.0123]
CASES = [  # n, fs, nframes, max_batch, learn — the frame counts of test_gpu_cs16.BIT_CASES
    (512, 128_000, 100, 40, 15), (2048, 512_000, 90, 32, 12), (8192, 2_048_000, 96, 48, 12), (32768, 6_000_000, 60, 24, 8),
    (65536, 20_000_000, 40, 16, 6), (131072, 20_000_000, 40, 20, 4), (262144, 61_440_000, 24, 12, 3), (1 << 20, 61_440_000, 24, 16, 3),
]


def _cat(outs):
    res = {k: np.concatenate([o[k] for o in outs]) for k in ("psd", "rel", "avg", "cand_idx", "cand_avg") if k in outs[0]}
    res["cand_off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(o["cand_off"]) for o in outs]))]).astype(np.int32)
    return res


def _raw(n, nframes, learn, fmt, seed):
    band = pkg.synth.SyntheticBand(n, seed=seed, on_frame=learn + 3, off_frame=nframes - 3)
    return (band.frames_cs8(nframes), A.SS_FMT_CS8, np.float32(0.0)) if fmt == "cs8" else (band.frames_cu8(nframes), A.SS_FMT_CU8, np.float32(127.5))


@pytest.mark.parametrize("n,fs,nframes,max_batch,learn", CASES)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_int8_scale_matches_oracle_and_the_cf32_conversion(oracle_mod, fmt, scale, n, fs, nframes, max_batch, learn):
    """Calls that keep their planes (at 65536 / 131072 points: the four-step forms), ragged sizes."""
    raw, in_format, offset = _raw(n, nframes, learn, fmt, n % 97)
    cf = np.ascontiguousarray((raw.astype(np.float32) - offset) * np.float32(scale)).view(np.complex64)[..., 0]
    kw = dict(fft_size=n, decim=1, learn_frames=learn, max_batch=max_batch)
    e8 = pkg.SpectrumEngine(fs, CENTER, in_format=in_format, int_scale=scale, **kw)
    e32 = pkg.SpectrumEngine(fs, CENTER, **kw)
    orc = oracle_mod.oracle_chain(fs, CENTER, in_format=in_format, int_scale=scale, **kw)
    outs_e, outs_o, pos = [], [], 0
    for k, size in enumerate(_ragged(nframes, max_batch, np.random.default_rng(n))):
        g8, g32 = e8.process(raw[pos:pos + size]), e32.process(cf[pos:pos + size])
        for key in KEYS:
            _same(f"call {k} {key}", g8[key], g32[key])
        outs_e.append(g8)
        outs_o.append(orc.process(raw[pos:pos + size]))
        pos += size
    got, ref = _cat(outs_e), _cat(outs_o)
    errs, ncand, ndc = check_all(got, ref)
    print(f"\n[{fmt} x {scale:.4g}, {n} points] {ncand} reference candidates, {ndc} inside the band; |err| dB: {format_quantiles(error_quantiles(got, ref))}")
    assert ncand > 50 and ndc <= dont_care_limit(ncand), (ncand, ndc)


@pytest.mark.parametrize("n,fs,learn,chunk,ncalls", [(65536, 20_000_000, 6, 25, 3), (131072, 20_000_000, 21, 32, 4)])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_int8_scale_on_the_fold_matches_oracle(oracle_mod, fmt, scale, n, fs, learn, chunk, ncalls):
    """ss_process_device calls that hand out no plane; those after the learning frames are the calls the fold takes (run_batch: dif_call),
    its table carrying the scale. The combs come on once the averager is full and the ceiling is learned from 21 frames at 131072
    points (the vector of test_gpu_stated_configs' getFft case), so that the band has tiles to cull.
    That the fold is what ran follows from ss_create's condition — fold_ok does not look at int_scale — and is WITNESSED at 131072 points: culling exists there only with the fold (det_lag2 needs fold_ok), so tiles_culled > 0
    on a run with empty tiles says the fold ran. (At 65536 points the four-step form culls too: the counters cannot tell the two apart.)"""
    import torch
    nframes = chunk * ncalls
    band = pkg.synth.SyntheticBand(n, seed=46, on_frame=learn + 24, off_frame=nframes - 12)
    raw, in_format = (band.frames_cs8(nframes), A.SS_FMT_CS8) if fmt == "cs8" else (band.frames_cu8(nframes), A.SS_FMT_CU8)
    kw = dict(fft_size=n, decim=1, learn_frames=learn, in_format=in_format, int_scale=scale)
    ref = oracle_mod.oracle_chain(fs, CENTER, max_batch=nframes, **kw).process(raw)
    eng = pkg.SpectrumEngine(fs, CENTER, max_batch=chunk, **kw)
    cuts = [chunk * k for k in range(ncalls + 1)]
    dev = torch.device("cuda", 0)
    d_iq = [torch.from_numpy(raw[a:b]).to(dev) for a, b in zip(cuts, cuts[1:])]
    outs = [dict(off=torch.zeros(b - a + 1, dtype=torch.int32, device=dev), idx=torch.empty((b - a) * 2048, dtype=torch.int32, device=dev),
                 avg=torch.empty((b - a) * 2048, dtype=torch.float32, device=dev)) for a, b in zip(cuts, cuts[1:])]
    torch.cuda.synchronize()
    for d, o in zip(d_iq, outs):
        eng.process_device(d, d.shape[0], cand_off=o["off"], cand_idx=o["idx"], cand_avg=o["avg"])
    eng.sync()
    st = eng.stats()
    res = []
    for o in outs:
        off = o["off"].cpu().numpy()
        res.append({"cand_off": off, "cand_idx": o["idx"].cpu().numpy()[:off[-1]], "cand_avg": o["avg"].cpu().numpy()[:off[-1]]})
    errs, ncand, ndc = check_all(_cat(res), ref)
    print(f"\n[{fmt} x {scale:.4g}, {n} points, fold] {ncand} reference candidates, {ndc} inside the band; tiles {st['tiles_total']}, tested {st['tiles_tested']}, culled {st['tiles_culled']}")
    assert ncand > 50 and ndc <= dont_care_limit(ncand), (ncand, ndc)
    if n == 131072:
        assert st["culling"] and st["tiles_tested"] > 0 and st["tiles_culled"] > 0, st
