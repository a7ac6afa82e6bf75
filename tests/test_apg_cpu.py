"""CPU: adaptive projected guidance (apg=, arXiv 2410.02416 Algorithm 1, per frame on the data prediction) -- the restatement of
tests/apg_ref.py anchored to the oracle with APG off and to the definition on analytic float64 cases, the host loop of
MikuDanceVideoPipeline.denoise() on emulated operators against it (one rank and three gloo ranks, FreeInit passes), the argument checks of both
entry points, and the script's --apg flags."""
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd.selftest import SCHED_KWARGS

import apg_ref as A
import dpmpp_ref as R
import fake_ops
from loop_helpers import (CountingUNet, cosine, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401
                          worker_setup, zero_inputs)

WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)      # f = 12: two windows, the second wraps
DEFAULTS = dict(apg=False, apg_eta=0.0, apg_norm_threshold=0.0, apg_momentum=0.0)


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


def _names():
    return [n for n, _ in A.apg_calls()]


# ---- 1. the restatement is the oracle's loop with APG off
@pytest.mark.parametrize("frames,win", [(4, {}), (12, WRAP12)], ids=["f4", "f12-wrap"])
def test_restatement_equals_oracle_with_apg_off(small_cpu, frames, win):
    from oracle import cpu_ref as O
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(frames, 60 + frames)
    with torch.no_grad():
        want = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True, **win)
        got = A.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True, apg_on=False, apg_eta=0.3, apg_momentum=-0.5, **win)
        on = A.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True, apg_on=True, apg_eta=0.0, apg_momentum=-0.5, **win)
    assert torch.equal(got, want)
    assert not torch.equal(on, want)


# ---- 2. the definition on analytic float64 cases: (F, HW, 4) tensors, one frame = dims (1, 2)
def _case(seed, F=3, hw=35):
    g = torch.Generator().manual_seed(seed)
    u, c, x = (torch.randn((F, hw, 4), generator=g, dtype=torch.float64) * k for k in (0.5, 0.8, 1.0))
    return u, c + 0.3, x


def _dot(p, q):
    return (p * q).sum((1, 2))


def test_eta_1_without_cap_or_momentum_is_plain_cfg():
    u, c, x = _case(0)
    for a, s in ((0.6, 0.8), (0.0, 1.0), (0.9995, 0.0316)):
        v = A.apg(u, c, x, a, s, 7.5, 1.0, 0.0, 0.0, None, (1, 2))["v"]
        assert float((v - (u + 7.5 * (c - u))).abs().max()) <= 1e-12


def test_eta_0_update_is_orthogonal_to_the_conditional_prediction():
    u, c, x = _case(1)
    for r in (0.0, 2.0):
        res = A.apg(u, c, x, 0.6, 0.8, 7.5, 0.0, r, 0.0, None, (1, 2))
        d = res["D_g"] - res["D_c"]
        rel = _dot(d, res["D_c"]).abs() / (_dot(d, d).sqrt() * _dot(res["D_c"], res["D_c"]).sqrt())
        assert float(rel.max()) <= 1e-12, rel
        # and eta scales the parallel part: D_g(eta) - D_g(0) = eta (g - 1) S proj D_c
        half = A.apg(u, c, x, 0.6, 0.8, 7.5, 0.5, r, 0.0, None, (1, 2))
        assert torch.allclose(half["D_g"] - res["D_g"], 0.5 * 6.5 * res["S"] * res["proj"] * res["D_c"], rtol=1e-12, atol=1e-14)


def test_threshold_caps_the_norm_of_the_update():
    u, c, x = _case(2, F=4)
    u = c + (u - c) * torch.tensor([0.1, 1.0, 3.0, 10.0], dtype=torch.float64).view(-1, 1, 1)      # frames of very different ||u - c||
    free = A.apg(u, c, x, 0.6, 0.8, 7.5, 1.0, 0.0, 0.0, None, (1, 2))
    norms = _dot(free["m"], free["m"]).sqrt()
    r = float(norms.sort().values[1:3].mean())                                                     # two frames below, two above
    res = A.apg(u, c, x, 0.6, 0.8, 7.5, 1.0, r, 0.0, None, (1, 2))
    capped = (res["S"] * res["m"])
    got = _dot(capped, capped).sqrt()
    assert torch.allclose(got, torch.clamp(norms, max=r), rtol=1e-12, atol=0)
    assert (res["S"].view(-1) < 1).sum() == 2 and (res["S"].view(-1) == 1).sum() == 2


def test_two_steps_of_negative_momentum():
    u1, c1, x1 = _case(3)
    u2, c2, x2 = _case(4)
    s1, s2 = 0.9, 0.7
    one = A.apg(u1, c1, x1, (1 - s1 * s1) ** 0.5, s1, 7.5, 0.0, 0.0, -0.5, torch.zeros_like(u1), (1, 2))
    two = A.apg(u2, c2, x2, (1 - s2 * s2) ** 0.5, s2, 7.5, 0.0, 0.0, -0.5, one["m"], (1, 2))
    d1, d2 = s1 * (u1 - c1), s2 * (u2 - c2)                                # D_c - D_u of each step
    assert float((one["m"] - d1).abs().max()) <= 1e-15
    assert float((two["m"] - (d2 - 0.5 * d1)).abs().max()) <= 1e-15
    # beta == 0 never reads the state
    nan = torch.full_like(u1, float("nan"))
    assert torch.isfinite(A.apg(u1, c1, x1, 0.6, 0.8, 7.5, 0.0, 1.0, 0.0, nan, (1, 2))["v"]).all()


def test_vanishing_norms_follow_the_two_rules():
    u, c, x = _case(5)
    u[0] = c[0]                                                            # frame 0: no update at all -> N2 = 0 -> S = 1
    x[1], c[1] = 0.0, 0.0                                                  # frame 1: D_c = 0 -> Q = 0 -> proj = 0
    res = A.apg(u, c, x, 0.6, 0.8, 7.5, 0.0, 0.5, 0.0, None, (1, 2))
    assert float(res["N2"][0]) == 0.0 and float(res["S"][0]) == 1.0 and float(res["Q"][1]) == 0.0 and float(res["proj"][1]) == 0.0
    assert torch.isfinite(res["v"]).all()
    assert torch.equal(res["v"][0], c[0])                                  # no update: the conditional prediction
    assert float(res["S"][2]) < 1.0 and float(res["proj"][2]) != 0.0       # an ordinary frame is capped and projected


# ---- 3. the host loop of denoise() on the emulated operators, against the restatement
def _threshold(ref_sd, den_sd, inputs, steps, rs, momentum, **win):
    """A threshold that caps some (step, frame) pairs and not others: the median norm of the uncapped run."""
    norms = []
    with torch.no_grad():
        A.denoise_loop(ref_sd, den_sd, *inputs, steps, guidance_scale=3.5, reduced=True, scheduler=rs, apg_on=True, apg_momentum=momentum,
                       on_apg=lambda t, res: norms.append(res["N2"].flatten().sqrt()), **win)
    return float(torch.cat(norms).median())


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_host_loop_matches_restatement(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 17)
    mk_rs = lambda: None if sampler == "ddim" else R.Restated(2, "dpmsolver++", "midpoint")
    r = _threshold(ref_sd, den_sd, (lat, rl, emb), 4, mk_rs(), -0.5)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim() if sampler == "ddim" else _dpm())
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 4, 3.5, apg=True, apg_eta=0.0, apg_norm_threshold=r, apg_momentum=-0.5)
    step = "cfg_ddim_step_apg" if sampler == "ddim" else "cfg_multistep_step_apg"
    assert _names() == ["cfg_apg_prepare", step] * 4, _names()
    pre = [d for n, d in A.apg_calls() if n == "cfg_apg_prepare"]
    assert all((d["momentum"], d["eta"], d["norm_threshold"]) == (-0.5, 0.0, r) for d in pre)
    assert [d["momentum_buf_was_zero"] for d in pre] == [True, False, False, False]
    for d in pre:                                                          # a = sqrt(abar_t), s = sqrt(1 - abar_t) of the step
        assert abs(d["alpha_s"] ** 2 + d["sigma_s"] ** 2 - 1.0) <= 1e-6 and d["sigma_s"] > 0
    caps = []
    with torch.no_grad():
        kw = dict(guidance_scale=3.5, reduced=True)
        want = A.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, scheduler=mk_rs(), apg_on=True, apg_eta=0.0, apg_norm_threshold=r, apg_momentum=-0.5,
                              on_apg=lambda t, res: caps.append(res["S"].flatten()), **kw)
        plain = A.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, scheduler=mk_rs(), apg_on=False, **kw)
    caps = torch.cat(caps)
    assert (caps < 1).any() and (caps == 1).any()                          # the threshold caps some frames and not others
    e, c, d = rel_l2(out.float(), want), cosine(out.float(), want), rel_l2(plain, want)
    print(f"\nAPG_HOST_LOOP {sampler} rel_l2 {e:.3e} cos {c:.7f} (plain vs APG restated: {d:.3e})")
    assert torch.isfinite(out).all() and e <= 3e-2 and c >= 0.999, (e, c)
    assert e < 0.5 * d, (e, d)                                             # closer to the APG loop than to the plain one


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_default_makes_no_apg_call_and_keeps_the_bits(monkeypatch, small_cpu, sampler):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 19))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim() if sampler == "ddim" else _dpm())
    a = pipe.denoise(lat, rl, emb, 2, 3.5)
    calls_a = fake_ops.tail_calls()
    del fake_ops.CALLS[:]
    b = pipe.denoise(lat, rl, emb, 2, 3.5, apg=False, apg_eta=0.3, apg_norm_threshold=2.0, apg_momentum=-0.5)
    step = "cfg_ddim_step" if sampler == "ddim" else "cfg_multistep_step"
    assert torch.equal(a, b) and calls_a == fake_ops.tail_calls() and _names() == [step] * 2
    del fake_ops.CALLS[:]
    c = pipe.denoise(lat, rl, emb, 2, 3.5, apg=True)
    assert not torch.equal(a, c) and _names().count("cfg_apg_prepare") == 2          # the keyword is not silently ignored


def test_apg_without_cfg_runs_the_plain_path(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 21))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    a = pipe.denoise(lat, rl, emb[1:], 2, 1.0, apg=True, apg_momentum=-0.5)
    assert _names() == ["cfg_ddim_step"] * 2
    assert torch.equal(a, pipe.denoise(lat, rl, emb[1:], 2, 1.0))


def test_eta_and_sde_draws_reach_the_apg_steps(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 22))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    pipe.denoise(lat, rl, emb, 2, 3.5, apg=True, eta=0.5, generator=torch.Generator().manual_seed(1))
    assert [(n, d["keywords"]) for n, d in A.apg_calls() if n != "cfg_apg_prepare"] == [("cfg_ddim_step_apg", ("variance_noise",))] * 2
    del fake_ops.CALLS[:]
    sde = M.DPMSolverMultistepScheduler(**SCHED_KWARGS, algorithm_type="sde-dpmsolver++")
    M.MikuDanceVideoPipeline(None, None, ref, den, sde).denoise(lat, rl, emb, 2, 3.5, apg=True, generator=torch.Generator().manual_seed(1))
    assert [(n, d["keywords"]) for n, d in A.apg_calls() if n != "cfg_apg_prepare"] == [("cfg_multistep_step_apg", ("variance_noise",))] * 2


def test_momentum_buffer_is_zeroed_once_per_free_init_pass(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 23))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    pipe.denoise(lat, rl, emb, 3, 3.5, apg=True, apg_momentum=-0.5, free_init_iters=2, generator=torch.Generator().manual_seed(2))
    names = [n for n, _ in fake_ops.CALLS if n.startswith("cfg_") or n == "free_init_mix"]
    one_pass = ["cfg_apg_prepare", "cfg_ddim_step_apg"] * 3
    assert names == one_pass + ["free_init_mix"] + one_pass
    assert [d["momentum_buf_was_zero"] for n, d in A.apg_calls() if n == "cfg_apg_prepare"] == [True, False, False] * 2


# ---- 4. argument checks, both entry points
BAD = [(dict(apg_eta=-0.1), "apg_eta"), (dict(apg_eta=1.0001), "apg_eta"), (dict(apg_eta=float("nan")), "apg_eta"),
       (dict(apg_eta=float("inf")), "apg_eta"), (dict(apg_norm_threshold=-1.0), "apg_norm_threshold"),
       (dict(apg_norm_threshold=float("nan")), "apg_norm_threshold"), (dict(apg_norm_threshold=float("inf")), "apg_norm_threshold"),
       (dict(apg_momentum=1.0), "apg_momentum"), (dict(apg_momentum=-1.0), "apg_momentum"), (dict(apg_momentum=float("nan")), "apg_momentum"),
       (dict(apg_momentum=-float("inf")), "apg_momentum"), (dict(apg=True, apg_eta=2.0), "apg_eta"),
       (dict(apg=True, guidance_rescale=0.7), "cannot be combined with guidance_rescale")]


@pytest.mark.parametrize("kw,msg", BAD)
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_bad_arguments_raise_before_any_unet(monkeypatch, kw, msg, make):
    fake_ops.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, make())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 4, 3.5, **kw)
    assert refu.calls == 0 and den.calls == 0 and fake_ops.CALLS == []


def test_call_refuses_before_clip_and_vae_and_forwards_the_keywords(monkeypatch):
    from PIL import Image
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append({k: v for k, v in kw.items() if k.startswith("apg")})
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    custom = dict(apg=True, apg_eta=0.25, apg_norm_threshold=12.5, apg_momentum=-0.5)
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        del seen[:]
        clip = fake_ops.FakeCLIP()
        calls = []
        clip.register_forward_hook(lambda *a: calls.append(1))
        pipe = cls(vae=fake_ops.FakeVAE(), image_encoder=clip, reference_unet=None, denoising_unet=types.SimpleNamespace(in_channels=4),
                   scheduler=_ddim())
        args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5)
        for kw, msg in BAD:
            with pytest.raises(ValueError, match=msg):
                pipe(*args, generator=torch.Generator().manual_seed(0), **kw)
        assert not calls and not seen
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), **custom)
        assert seen == [DEFAULTS, custom]


# ---- 5. window parallelism: three gloo ranks, every rank its own identical momentum buffer
def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=521))
    # 3 windows, the last one wraps
    kw = dict(context_frames=8, context_stride=1, context_overlap=2, apg=True, apg_eta=0.0, apg_norm_threshold=8.0, apg_momentum=-0.5)
    res = {}
    for name, sch in (("ddim", M.DDIMScheduler(**SCHED_KWARGS)), ("2m", M.DPMSolverMultistepScheduler(**SCHED_KWARGS))):
        pipe = MikuDanceVideoPipeline(None, None, ref, den, sch)
        out = pipe.denoise(lat, rl, emb, 3, 3.5, window_parallel=dp.WindowParallel(), **kw)
        got = dp.gather_latents(out)
        if rank == 0:
            one = pipe.denoise(lat, rl, emb, 3, 3.5, **kw)
            plain = pipe.denoise(lat, rl, emb, 3, 3.5, **dict(kw, apg=False))
            res[name] = dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                             finite=bool(torch.isfinite(out).all()), projected=not torch.equal(out, plain))
    if rank == 0:
        q.put(res)
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    res = run_world(3, _wp_worker)
    assert sorted(res) == ["2m", "ddim"]
    for name, r in res.items():
        assert all(r.values()), (name, r)


# ---- 6. the script
def test_script_flags_parse():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.apg, a.apg_eta, a.apg_norm_threshold, a.apg_momentum) == (False, 0.0, 0.0, 0.0)
    a = IV.parse_args(["--apg", "--apg_eta", "0.25", "--apg_norm_threshold", "12.5", "--apg_momentum", "-0.5", "--sampler", "dpmpp_2m"])
    assert (a.apg, a.apg_eta, a.apg_norm_threshold, a.apg_momentum) == (True, 0.25, 12.5, -0.5)
    with pytest.raises(SystemExit):
        IV.parse_args(["--apg_eta", "low"])
    assert "apg=--apg" in IV.__doc__


def test_script_help_marks_the_flags_as_additions(capsys):
    from mikudance_amd import inference_video as IV
    with pytest.raises(SystemExit):
        IV.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for flag in ("--apg (addition)", "--apg_eta APG_ETA (addition)", "--apg_norm_threshold APG_NORM_THRESHOLD (addition)",
                 "--apg_momentum APG_MOMENTUM (addition)"):
        assert flag in text, flag


def test_script_flags_reach_denoise(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append(tuple(kw[k] for k in ("apg", "apg_eta", "apg_norm_threshold", "apg_momentum")) + (type(self.scheduler).__name__,))
        return latents

    monkeypatch.setattr(IV, "build_pipeline", fake_pipeline_builder(IV))
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base)
    IV.main(base + ["--apg", "--apg_eta", "0", "--apg_momentum", "-0.5"])
    IV.main(base + ["--apg", "--apg_eta", "0.25", "--apg_norm_threshold", "12.5", "--apg_momentum", "-0.75", "--sampler", "dpmpp_2m"])
    assert seen == [(False, 0.0, 0.0, 0.0, "DDIMScheduler"), (True, 0.0, 0.0, -0.5, "DDIMScheduler"),
                    (True, 0.25, 12.5, -0.75, "DPMSolverMultistepScheduler")]
