"""CPU: guidance rescale (guidance_rescale, arXiv 2305.08891 section 3.4) -- the float64 / fp32 restatement of tests/rescale_ref.py anchored
to the oracle at phi = 0 and to diffusers' formula on an analytic case, the host loop of MikuDanceVideoPipeline.denoise() on emulated
operators against it (one rank and three gloo ranks), the argument checks, and the script's --guidance_rescale."""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import fake_ops
import rescale_ref as RR
from loop_helpers import (CountingUNet, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401 (small_cpu: fixture)
                          worker_setup, zero_inputs)

WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)      # f = 12: two windows, the second wraps


def _steps():
    """(operator, optional tensors given) of every rescale / step call so far."""
    return [(n, d["keywords"]) for n, d in fake_ops.tail_calls("cfg_guidance_rescale", "cfg_ddim_step", "cfg_multistep_step")]


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


# ---- 1. the restatement is the oracle's loop at phi = 0
@pytest.mark.parametrize("frames,win", [(4, {}), (12, WRAP12)], ids=["f4", "f12-wrap"])
def test_restatement_equals_oracle_at_phi_0(small_cpu, frames, win):
    from oracle import cpu_ref as O
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(frames, 40 + frames)
    with torch.no_grad():
        want = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True, **win)
        got = RR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True, guidance_rescale=0.0, **win)
        got7 = RR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True, guidance_rescale=0.7, **win)
    assert torch.equal(got, want)
    assert not torch.equal(got7, want)


# ---- 2. the formula on an analytic case
def test_rescale_formula_analytic():
    g = torch.Generator().manual_seed(0)
    c = torch.randn((1, 4, 3, 5, 7), generator=g, dtype=torch.float64) * 0.8 + 0.3
    u = torch.randn((1, 4, 3, 5, 7), generator=g, dtype=torch.float64) * 0.5
    v = u + 7.5 * (c - u)
    one = RR.rescale_noise_cfg(v, c, 1.0)
    assert abs(float(one.std()) - float(c.std())) <= 1e-12 * float(c.std())
    assert torch.allclose(one, v * (c.std() / v.std()), rtol=1e-14, atol=0)
    # hand-written diffusers rescale_noise_cfg at phi = 0.7
    std_text = c.std(dim=[1, 2, 3, 4], keepdim=True)
    std_cfg = v.std(dim=[1, 2, 3, 4], keepdim=True)
    want = 0.7 * (v * (std_text / std_cfg)) + 0.3 * v
    assert torch.allclose(RR.rescale_noise_cfg(v, c, 0.7), want, rtol=1e-14, atol=0)
    # by hand in numpy, unbiased std over all 4 * 3 * 5 * 7 elements
    vn, cn = v.numpy().ravel(), c.numpy().ravel()
    f = 1 - 0.7 + 0.7 * np.sqrt(((cn - cn.mean()) ** 2).sum() / (cn.size - 1)) / np.sqrt(((vn - vn.mean()) ** 2).sum() / (vn.size - 1))
    assert np.allclose(RR.rescale_noise_cfg(v, c, 0.7).numpy().ravel(), vn * f, rtol=1e-13, atol=0)
    # the documented deviation: a constant v is left unscaled
    k = torch.full((1, 4, 2, 3, 3), 0.25, dtype=torch.float64)
    assert torch.equal(RR.rescale_noise_cfg(k, c[:, :, :2, :3, :3], 0.7), k)


# ---- 3. the host loop of denoise() on the emulated operators, against the restatement
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_host_loop_matches_restatement(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 7)
    sch = M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _dpm()
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 4, 3.5, guidance_rescale=0.7)
    step = "cfg_ddim_step" if sampler == "ddim" else "cfg_multistep_step"
    assert _steps() == [("cfg_guidance_rescale", ()), (step, ("vscale",))] * 4, _steps()
    assert all(d["phi"] == 0.7 for _, d in fake_ops.tail_calls("cfg_guidance_rescale"))
    rs = None if sampler == "ddim" else R.Restated(2, "dpmsolver++", "midpoint")
    with torch.no_grad():
        want = RR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, guidance_scale=3.5, reduced=True, scheduler=rs, guidance_rescale=0.7)
        plain = RR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, guidance_scale=3.5, reduced=True, scheduler=rs, guidance_rescale=0.0)
    r, d = rel_l2(out.float(), want), rel_l2(plain, want)
    print(f"\nRESCALE_HOST_LOOP {sampler} rel_l2 {r:.3e} (phi 0 vs 0.7 restated: {d:.3e})")
    assert torch.isfinite(out).all() and r < 2e-2, r
    assert r < 0.5 * d, (r, d)                                            # closer to the rescaled loop than to the plain one


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_phi_0_calls_only_the_unscaled_entry_points(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 9))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _dpm())
    a = pipe.denoise(lat, rl, emb, 2, 3.5, guidance_rescale=0.0)
    calls_a = fake_ops.tail_calls()
    del fake_ops.CALLS[:]
    b = pipe.denoise(lat, rl, emb, 2, 3.5)
    step = "cfg_ddim_step" if sampler == "ddim" else "cfg_multistep_step"
    assert calls_a == fake_ops.tail_calls() and [(n, d["keywords"]) for n, d in calls_a if n.startswith("cfg_")] == [(step, ())] * 2
    assert torch.equal(a, b)


# ---- 4. argument checks
@pytest.mark.parametrize("phi", [-0.1, 1.0001, float("nan"), float("inf")])
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_bad_phi_raises_before_any_unet(monkeypatch, phi, sampler):
    fake_ops.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _dpm())
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe.denoise(*zero_inputs(), 4, 3.5, guidance_rescale=phi)
    assert refu.calls == 0 and den.calls == 0 and fake_ops.CALLS == []


def test_phi_without_cfg_runs_the_unscaled_path(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 11))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    a = pipe.denoise(lat, rl, emb[1:], 2, 1.0, guidance_rescale=0.7)
    assert _steps() == [("cfg_ddim_step", ())] * 2
    b = pipe.denoise(lat, rl, emb[1:], 2, 1.0)
    assert torch.equal(a, b)


def test_call_forwards_guidance_rescale(monkeypatch):
    """MikuDanceVideoPipeline.__call__ and Pose2VideoPipeline.__call__ hand the keyword to denoise() (default 0.0)."""
    from PIL import Image
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append(kw.get("guidance_rescale"))
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    den = types.SimpleNamespace(in_channels=4)
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        pipe = cls(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=None, denoising_unet=den,
                   scheduler=M.DDIMScheduler(**SCHED_KWARGS))
        motion = np.zeros((2, 2, 4, 4), dtype=np.float32)
        args = (img, img, [img, img], [img, img], [img, img], motion, 32, 32, 2, 2, 3.5)
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), guidance_rescale=0.7)
    assert seen == [0.0, 0.7, 0.0, 0.7]


# ---- 5. window parallelism: three gloo ranks
def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=321))
    kw = dict(context_frames=8, context_stride=1, context_overlap=2, guidance_rescale=0.7)     # 3 windows, the last one wraps
    res = {}
    for name, sch in (("ddim", M.DDIMScheduler(**SCHED_KWARGS)), ("2m", _dpm())):
        pipe = MikuDanceVideoPipeline(None, None, ref, den, sch)
        out = pipe.denoise(lat, rl, emb, 3, 3.5, window_parallel=dp.WindowParallel(), **kw)
        got = dp.gather_latents(out)
        if rank == 0:
            one = pipe.denoise(lat, rl, emb, 3, 3.5, **kw)
            plain = pipe.denoise(lat, rl, emb, 3, 3.5, **dict(kw, guidance_rescale=0.0))
            res[name] = dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                             finite=bool(torch.isfinite(out).all()), rescaled=not torch.equal(out, plain))
    if rank == 0:
        q.put(res)
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    res = run_world(3, _wp_worker)
    assert sorted(res) == ["2m", "ddim"]
    for name, r in res.items():
        assert all(r.values()), (name, r)


# ---- 6. the script
def test_script_flag_parses_and_defaults_to_0():
    from mikudance_amd import inference_video as IV
    assert IV.parse_args([]).guidance_rescale == 0.0
    assert IV.parse_args(["--guidance_rescale", "0.7", "--sampler", "dpmpp_2m"]).guidance_rescale == 0.7
    with pytest.raises(SystemExit):
        IV.parse_args(["--guidance_rescale", "high"])


@pytest.mark.parametrize("argv,want", [([], 0.0), (["--guidance_rescale", "0.7"], 0.7), (["--guidance_rescale", "0.5", "--sampler", "dpmpp_2m_sde"], 0.5)])
def test_script_flag_reaches_denoise(monkeypatch, tmp_path, argv, want):
    from mikudance_amd import inference_video as IV
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append((kw["guidance_rescale"], type(self.scheduler).__name__))
        return latents

    monkeypatch.setattr(IV, "build_pipeline", fake_pipeline_builder(IV))
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    out = IV.main(["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")] + argv)
    assert os.path.exists(out) and len(seen) == 1 and seen[0][0] == want and math.isfinite(seen[0][0])
