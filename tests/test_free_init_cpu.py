"""CPU: FreeInit noise re-initialisation (free_init_iters= ...) -- the host-side low-pass table against the literal triple loop, the identity
the kernel's form rests on, the outer loop of MikuDanceVideoPipeline.denoise() on emulated operators against the oracle loop composed with
the literal float64 mix (tests/free_init_ref.py), every refusal, a three-rank gloo run and the script's flags."""
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd import free_init as FI
from mikudance_amd import ops
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import fake_ops
import free_init_ref as FR
from loop_helpers import (CountingUNet, cosine, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401
                          worker_setup, zero_inputs)

SHAPES = [(5, 6, 9), (3, 7, 10), (1, 8, 8), (16, 12, 12)]
KINDS = ["butterworth", "gaussian", "ideal"]


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _log():
    """The tail operators and the mixes, in call order."""
    return [(n, d) for n, d in fake_ops.CALLS if n in fake_ops.TAIL or n == "free_init_mix"]


# ---- 1. the filter table
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_freq_filter_matches_the_literal_table(shape, kind):
    want = FR.symmetrised(FR.lpf_literal(*shape, kind, 4, 0.25, 0.25))
    got = FI.freq_filter(*shape, kind, 4, 0.25, 0.25)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    g = got.double().numpy()
    assert (np.abs(g - want) <= 2.0 ** -24 * np.abs(want) + 1e-45).all(), float(np.abs(g - want).max())
    assert np.array_equal(g, FR.reflect(g))                              # symmetric under k -> -k
    other = FI.freq_filter(*shape, kind, 2, 0.3, 0.2).double().numpy()   # other parameters reach the formula
    want2 = FR.symmetrised(FR.lpf_literal(*shape, kind, 2, 0.3, 0.2))
    assert (np.abs(other - want2) <= 2.0 ** -24 * np.abs(want2) + 1e-45).all()


@pytest.mark.parametrize("kind", KINDS)
def test_zero_stop_frequency_gives_zeros(kind):
    assert not FI.freq_filter(5, 6, 9, kind, 4, 0.0, 0.25).any() and not FI.freq_filter(5, 6, 9, kind, 4, 0.25, 0.0).any()
    assert not FR.lpf_literal(5, 6, 9, kind, 4, 0.0, 0.25).any()


def test_ideal_filter_compares_against_twice_the_stop_frequency():
    """Frequency (0, 0, 2) of a 12-wide axis: d2 = (2 * 8 / 12 - 1)^2 = 1 / 9, above ds^2 = 1 / 16 and below 2 ds = 1 / 2."""
    d2, ds = (2 * 8 / 12 - 1) ** 2, 0.25
    assert ds ** 2 < d2 <= 2 * ds
    t = FI.freq_filter(16, 12, 12, "ideal", 4, ds, ds)
    assert t[0, 0, 2] == 1.0 and t[0, 0, 10] == 1.0 and t[0, 0, 0] == 1.0 and t[8, 6, 6] == 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_form_equals_the_literal_mix(shape, kind):
    lpf = FR.lpf_literal(*shape, kind, 4, 0.25, 0.25)
    lsym = FR.symmetrised(lpf)
    x0, n0, z = (t.double().numpy() for t in FR.random_case(*shape, seed=11))
    a, b = 0.07, 0.9975
    alt = z + np.fft.ifftn(lsym[..., None] * np.fft.fftn(a * x0 + b * n0 - z, axes=(0, 1, 2)), axes=(0, 1, 2)).real
    lit = FR.mix_literal(x0, n0, z, a, b, lpf).numpy()
    assert np.abs(alt - lit).max() <= 1e-12
    for dt in (np.float64, np.float32):                                 # and the dense per-axis restatement computes the same thing
        d = FR.mix_dense(x0, n0, z, a, b, lsym, dt)
        assert np.abs(d - lit).max() <= (1e-12 if dt == np.float64 else 1e-5)


# ---- 2. the loop on the emulated operators
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_default_makes_no_mix_call_and_keeps_the_bits(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 81))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim() if sampler == "ddim" else _dpm())
    a = pipe.denoise(lat, rl, emb, 3, 3.5)
    log_a = _log()
    del fake_ops.CALLS[:]
    b = pipe.denoise(lat, rl, emb, 3, 3.5, free_init_iters=1, free_init_filter="gaussian", free_init_fast=True)
    assert torch.equal(a, b) and _log() == log_a and not [r for r in log_a if r[0] == "free_init_mix"]
    del fake_ops.CALLS[:]
    c = pipe.denoise(lat, rl, emb, 3, 3.5, free_init_iters=2, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(a, c) and len([r for r in _log() if r[0] == "free_init_mix"]) == 1      # the keyword is not silently ignored


def test_three_iterations_log_two_mixes_and_three_full_passes(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 82))
    sch = _ddim()
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    steps = []
    pipe.denoise(lat, rl, emb, 2, 3.5, free_init_iters=3, generator=torch.Generator().manual_seed(2), callback=lambda i, t, x: steps.append((i, t)))
    one_pass = ["window_accumulate", "cfg_ddim_step"] * 2
    assert [n for n, _ in _log()] == one_pass + ["free_init_mix"] + one_pass + ["free_init_mix"] + one_pass
    a, b = sch.noise_coefficients(999)
    assert [d for n, d in _log() if n == "free_init_mix"] == [dict(a=a, b=b)] * 2 and a < 0.1 and b > 0.99
    assert steps == [(0, 999), (1, 499)] * 3                             # callback counts from 0 in every pass


def test_banks_are_written_once_for_all_passes(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 83))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    writes = []
    orig = pipe._write_banks
    monkeypatch.setattr(pipe, "_write_banks", lambda *a, **k: (writes.append(1), orig(*a, **k))[1])
    pipe.denoise(lat, rl, emb, 2, 3.5, free_init_iters=3, generator=torch.Generator().manual_seed(2))
    assert len(writes) == 1


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_fast_sampling_runs_2_4_6_steps(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 84))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim() if sampler == "ddim" else _dpm())
    steps = []
    pipe.denoise(lat, rl, emb, 6, 3.5, free_init_iters=3, free_init_fast=True, generator=torch.Generator().manual_seed(3),
                 callback=lambda i, t, x: steps.append((i, t)))
    assert [i for i, _ in steps] == [0, 1] + [0, 1, 2, 3] + [0, 1, 2, 3, 4, 5]
    assert [t for _, t in steps] == [999, 499] + [999, 749, 499, 249] + [999, 832, 666, 499, 332, 166]
    if sampler == "2m":
        # every pass starts first order again; so is the step after t = 999 (lambda = -inf there: no step ratio) and the final one
        first_order = [d["c_m1"] == 0.0 for _, d in fake_ops.tail_calls("cfg_multistep_step")]
        assert first_order == [True, True] + [True, True, False, True] + [True, True, False, False, False, True]
    assert [FI.pass_steps(6, 3, i, True) for i in range(3)] == [2, 4, 6] and FI.pass_steps(2, 3, 0, True) == 1


@pytest.mark.parametrize("sampler", ["ddim", "ddim-eta", "2m"])
def test_host_loop_matches_oracle_with_literal_mix(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 85)
    eta = 0.5 if sampler == "ddim-eta" else 0.0
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _dpm() if sampler == "2m" else _ddim())
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 3, 3.5, eta=eta, free_init_iters=2, generator=torch.Generator().manual_seed(5))
    make = (lambda: R.Restated(2, "dpmsolver++", "midpoint")) if sampler == "2m" else None
    with torch.no_grad():
        want = FR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 3, 2, torch.Generator().manual_seed(5), make_scheduler=make, guidance_scale=3.5,
                               reduced=True, eta=eta, noise_dtype=torch.float16)
        once = FR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 3, 1, torch.Generator().manual_seed(5), make_scheduler=make, guidance_scale=3.5,
                               reduced=True, eta=eta, noise_dtype=torch.float16)
    r, c = rel_l2(out.float(), want), cosine(out.float(), want)
    print(f"\nFREE_INIT_HOST_LOOP {sampler} 2 passes of 3 steps rel_l2 {r:.3e} cos {c:.7f} (from one pass {rel_l2(want, once):.3e})")
    assert torch.isfinite(out).all() and r <= 3e-2 and c >= 0.999, (r, c)
    assert rel_l2(want, once) > 0.1                                      # the second pass matters


def test_z_is_the_first_draw_of_a_pass(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 86))
    seen = []
    monkeypatch.setattr(ops, "free_init_mix", lambda out, x0, n0, z, lpf, a, b: (seen.append((z.clone(), n0.clone())), FR.free_init_mix(out, x0, n0, z, lpf, a, b))[1])
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    pipe.denoise(lat, rl, emb, 2, 3.5, eta=0.5, free_init_iters=2, generator=torch.Generator().manual_seed(6))
    g = torch.Generator().manual_seed(6)
    for _ in range(2):                                                   # pass 0: one eta draw per step
        torch.randn(lat.shape, generator=g, dtype=torch.float16)
    z = torch.randn(lat.shape, generator=g, dtype=torch.float16)
    assert len(seen) == 1 and torch.equal(seen[0][0], z[0].permute(1, 2, 3, 0)) and torch.equal(seen[0][1], lat[0].permute(1, 2, 3, 0))
    assert [d["keywords"] for _, d in fake_ops.tail_calls("cfg_ddim_step")] == [("variance_noise",)] * 4


# ---- 3. refusals, all before any model runs
BAD = [(dict(free_init_iters=0), "free_init_iters"), (dict(free_init_iters=-1), "free_init_iters"), (dict(free_init_iters=2.0), "free_init_iters"),
       (dict(free_init_iters=True), "free_init_iters"), (dict(free_init_iters="3"), "free_init_iters"),
       (dict(free_init_filter="box"), "free_init_filter"), (dict(free_init_iters=2, free_init_filter=None), "free_init_filter"),
       (dict(free_init_order=0), "free_init_order"), (dict(free_init_order=1.5), "free_init_order"),
       (dict(free_init_spatial_stop=float("nan")), "free_init_spatial_stop"), (dict(free_init_spatial_stop=-0.1), "free_init_spatial_stop"),
       (dict(free_init_temporal_stop=float("inf")), "free_init_temporal_stop"), (dict(free_init_temporal_stop=-1), "free_init_temporal_stop"),
       (dict(free_init_iters=2, init_latents=torch.zeros(1, 4, 2, 2, 2, dtype=torch.float16), strength=0.5), "discards what strength means"),
       (dict(free_init_iters=2, init_latents=torch.zeros(1, 4, 2, 2, 2, dtype=torch.float16)), "discards what strength means")]


@pytest.mark.parametrize("kw,msg", BAD)
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_bad_arguments_raise_before_any_unet(kw, msg, make):
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, make())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 4, 3.5, **kw)
    assert refu.calls == 0 and den.calls == 0


@pytest.mark.parametrize("shape", [(257, 2, 2), (2, 257, 2), (2, 2, 257)])
def test_a_clip_outside_the_kernel_range_is_refused(shape):
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, _ddim())
    F, h, w = shape
    args = (torch.zeros(1, 4, F, h, w, dtype=torch.float16), torch.zeros(1, F, 22, h, w, dtype=torch.float16), torch.zeros(2, 5, 64, dtype=torch.float16))
    with pytest.raises(ValueError, match="outside the FreeInit kernel's range"):
        pipe.denoise(*args, 4, 3.5, free_init_iters=2)
    assert refu.calls == 0 and den.calls == 0
    assert FI.MAX_AXIS == 256


def test_call_refuses_before_clip_and_vae_and_forwards_the_keywords(monkeypatch):
    from PIL import Image
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append({k: v for k, v in kw.items() if k.startswith("free_init_")})
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    defaults = dict(free_init_iters=1, free_init_filter="butterworth", free_init_order=4, free_init_spatial_stop=0.25, free_init_temporal_stop=0.25,
                    free_init_fast=False)
    custom = dict(free_init_iters=3, free_init_filter="gaussian", free_init_order=2, free_init_spatial_stop=0.3, free_init_temporal_stop=0.2,
                  free_init_fast=True)
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        del seen[:]
        clip = fake_ops.FakeCLIP()
        calls = []
        clip.register_forward_hook(lambda *a: calls.append(1))
        pipe = cls(vae=fake_ops.FakeVAE(), image_encoder=clip, reference_unet=None, denoising_unet=types.SimpleNamespace(in_channels=4),
                   scheduler=_ddim())
        args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5)
        for kw, msg in [(dict(free_init_iters=0), "free_init_iters"), (dict(free_init_filter="box"), "free_init_filter"),
                        (dict(free_init_iters=2, video=[img, img], strength=0.5), "discards what strength means")]:
            with pytest.raises(ValueError, match=msg):
                pipe(*args, generator=torch.Generator().manual_seed(0), **kw)
        assert not calls and not seen
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), **custom)
        assert seen == [defaults, custom]


# ---- 4. the script
def test_script_flags_parse():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.free_init_iters, a.free_init_filter, a.free_init_order, a.free_init_spatial_stop, a.free_init_temporal_stop, a.free_init_fast) == \
        (1, "butterworth", 4, 0.25, 0.25, False)
    a = IV.parse_args(["--free_init_iters", "3", "--free_init_filter", "ideal", "--free_init_order", "2", "--free_init_spatial_stop", "0.3",
                       "--free_init_temporal_stop", "0.2", "--free_init_fast"])
    assert (a.free_init_iters, a.free_init_filter, a.free_init_order, a.free_init_spatial_stop, a.free_init_temporal_stop, a.free_init_fast) == \
        (3, "ideal", 2, 0.3, 0.2, True)
    for argv in (["--free_init_filter", "box"], ["--free_init_iters", "many"]):
        with pytest.raises(SystemExit):
            IV.parse_args(argv)


def test_script_flags_reach_the_pipeline(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append(tuple(kw[k] for k in ("free_init_iters", "free_init_filter", "free_init_order", "free_init_spatial_stop",
                                          "free_init_temporal_stop", "free_init_fast")))
        return latents

    monkeypatch.setattr(IV, "build_pipeline", fake_pipeline_builder(IV))
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base)
    IV.main(base + ["--free_init_iters", "3", "--free_init_filter", "gaussian", "--free_init_order", "2", "--free_init_spatial_stop", "0.3",
                    "--free_init_temporal_stop", "0.2", "--free_init_fast"])
    assert seen == [(1, "butterworth", 4, 0.25, 0.25, False), (3, "gaussian", 2, 0.3, 0.2, True)]


# ---- 5. window parallelism: three gloo ranks, the mix replicated on every rank
def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=421))
    # F = 16, windows of 8 with overlap 2, open: [0..7], [6..13], [8..15] -- one per rank, every fp32 sum has at most two non-zero terms
    kw = dict(context_frames=8, context_stride=1, context_overlap=2, context_schedule="uniform_open", free_init_iters=2, eta=0.5)
    pipe = MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat, rl, emb, 2, 3.5, window_parallel=dp.WindowParallel(), generator=torch.Generator().manual_seed(7), **kw)
    got = dp.gather_latents(out)
    if rank == 0:
        mixes = len([c for c in fake_ops.CALLS if c[0] == "free_init_mix"])
        one = pipe.denoise(lat, rl, emb, 2, 3.5, generator=torch.Generator().manual_seed(7), **kw)
        plain = pipe.denoise(lat, rl, emb, 2, 3.5, generator=torch.Generator().manual_seed(7), **dict(kw, free_init_iters=1))
        q.put(dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                   finite=bool(torch.isfinite(out).all()), one_mix=mixes == 1, mixed=not torch.equal(out, plain)))
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    res = run_world(3, _wp_worker)
    assert all(res.values()), res
