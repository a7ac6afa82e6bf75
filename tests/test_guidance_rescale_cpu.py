"""CPU: guidance rescale (guidance_rescale, arXiv 2305.08891 section 3.4) -- the float64 / fp32 restatement of tests/rescale_ref.py anchored
to the oracle at phi = 0 and to diffusers' formula on an analytic case, the host loop of MikuDanceVideoPipeline.denoise() on emulated
operators against it (one rank and three gloo ranks), the argument checks, and the script's --guidance_rescale."""
import math
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mikudance_amd as M
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import rescale_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)      # f = 12: two windows, the second wraps


# ---- the operators of md_cfg_guidance_rescale / md_cfg_*_step_scaled, emulated in PyTorch (fp32 arithmetic, one rounding of the latents)
CALLS = []


def _guided(noise_sum, counter, guidance, halves):
    if halves == 2:
        u, c = (noise_sum / counter.view(1, -1, 1, 1)).unbind(0)
        return u + guidance * (c - u), c
    return noise_sum[0], None


def fake_cfg_guidance_rescale(noise_sum, counter, ftot, hw, guidance, phi, out=None):
    v, c = _guided(noise_sum, counter, guidance, 2)
    sc, sv = float(c.double().std()), float(v.double().std())
    f = 1.0 if sv == 0.0 else 1.0 - phi + phi * sc / sv
    CALLS.append(("rescale", phi))
    if out is None:
        out = torch.empty((1,), dtype=torch.float32)
    out.fill_(f)
    return out


def fake_cfg_ddim_step(latents, noise_sum, counter, ftot, hw, guidance, alpha_t, alpha_prev, halves=2, eta=0.0, variance_noise=None, **kw):
    CALLS.append(("ddim", tuple(kw)))
    v, _ = _guided(noise_sum, counter, guidance, halves)
    if "vscale" in kw:
        v = v * kw["vscale"]
    x = latents.float().view(ftot, hw, 4)
    x0 = alpha_t ** 0.5 * x - (1 - alpha_t) ** 0.5 * v
    ep = alpha_t ** 0.5 * v + (1 - alpha_t) ** 0.5 * x
    std = eta * ((1 - alpha_prev) / (1 - alpha_t) * (1 - alpha_t / alpha_prev)) ** 0.5 if eta else 0.0
    out = alpha_prev ** 0.5 * x0 + max(1 - alpha_prev - std ** 2, 0.0) ** 0.5 * ep
    if eta:
        out = out + std * variance_noise.float().view(ftot, hw, 4)
    latents.copy_(out.view(latents.shape).to(torch.float16))


def fake_cfg_multistep_step(latents, noise_sum, counter, history, ftot, hw, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z, halves=2,
                            variance_noise=None, **kw):
    CALLS.append(("multistep", tuple(kw)))
    v, _ = _guided(noise_sum, counter, guidance, halves)
    if "vscale" in kw:
        v = v * kw["vscale"]
    x = latents.float().view(ftot, hw, 4)
    m0 = alpha_s * x - sigma_s * v
    out = c_x * x + c_m0 * m0
    if c_m1 != 0.0:
        out = out + c_m1 * history.view(ftot, hw, 4)
    history.view(ftot, hw, 4).copy_(m0)
    if c_z != 0.0:
        out = out + c_z * variance_noise.float().view(ftot, hw, 4)
    latents.copy_(out.view(latents.shape).to(torch.float16))


def _install_process():
    import fake_ops
    from mikudance_amd import ops
    fake_ops.install_process()
    ops.cfg_guidance_rescale, ops.cfg_ddim_step, ops.cfg_multistep_step = fake_cfg_guidance_rescale, fake_cfg_ddim_step, fake_cfg_multistep_step
    del CALLS[:]


def _install(monkeypatch):
    import fake_ops
    from mikudance_amd import ops
    fake_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "cfg_guidance_rescale", fake_cfg_guidance_rescale)
    monkeypatch.setattr(ops, "cfg_ddim_step", fake_cfg_ddim_step)
    monkeypatch.setattr(ops, "cfg_multistep_step", fake_cfg_multistep_step)
    del CALLS[:]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


@pytest.fixture(scope="module")
def small_cpu():
    from mikudance_amd.selftest import build_models
    return build_models(device="cpu")


def _inputs(frames, seed):
    from mikudance_amd.synth import synth_inputs
    return tuple(t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=seed))


# ---- 1. the restatement is the oracle's loop at phi = 0
@pytest.mark.parametrize("frames,win", [(4, {}), (12, WRAP12)], ids=["f4", "f12-wrap"])
def test_restatement_equals_oracle_at_phi_0(small_cpu, frames, win):
    from oracle import cpu_ref as O
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = _inputs(frames, 40 + frames)
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
    _install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = _inputs(4, 7)
    sch = M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _dpm()
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 4, 3.5, guidance_rescale=0.7)
    kinds = [k for k, _ in CALLS]
    step = "ddim" if sampler == "ddim" else "multistep"
    assert kinds == ["rescale", step] * 4, kinds
    assert all(kw == ("vscale",) for k, kw in CALLS if k == step)
    rs = None if sampler == "ddim" else R.Restated(2, "dpmsolver++", "midpoint")
    with torch.no_grad():
        want = RR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, guidance_scale=3.5, reduced=True, scheduler=rs, guidance_rescale=0.7)
        plain = RR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, guidance_scale=3.5, reduced=True, scheduler=rs, guidance_rescale=0.0)
    r, d = _rel(out.float(), want), _rel(plain, want)
    print(f"\nRESCALE_HOST_LOOP {sampler} rel_l2 {r:.3e} (phi 0 vs 0.7 restated: {d:.3e})")
    assert torch.isfinite(out).all() and r < 2e-2, r
    assert r < 0.5 * d, (r, d)                                            # closer to the rescaled loop than to the plain one


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_phi_0_calls_only_the_unscaled_entry_points(monkeypatch, small_cpu, sampler):
    _install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in _inputs(4, 9))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _dpm())
    a = pipe.denoise(lat, rl, emb, 2, 3.5, guidance_rescale=0.0)
    calls_a = list(CALLS)
    del CALLS[:]
    b = pipe.denoise(lat, rl, emb, 2, 3.5)
    assert calls_a == list(CALLS) and all(kw == () for _, kw in calls_a) and "rescale" not in [k for k, _ in calls_a]
    assert torch.equal(a, b)


# ---- 4. argument checks
class _CountingUNet:
    def __init__(self):
        self.calls = 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def f(*a, **k):
            self.calls += 1
        return f


def _cpu_inputs():
    return torch.zeros(1, 4, 2, 2, 2, dtype=torch.float16), torch.zeros(1, 2, 22, 2, 2, dtype=torch.float16), torch.zeros(2, 5, 64, dtype=torch.float16)


@pytest.mark.parametrize("phi", [-0.1, 1.0001, float("nan"), float("inf")])
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_bad_phi_raises_before_any_unet(monkeypatch, phi, sampler):
    _install(monkeypatch)
    refu, den = _CountingUNet(), _CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _dpm())
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe.denoise(*_cpu_inputs(), 4, 3.5, guidance_rescale=phi)
    assert refu.calls == 0 and den.calls == 0 and CALLS == []


def test_phi_without_cfg_runs_the_unscaled_path(monkeypatch, small_cpu):
    _install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in _inputs(4, 11))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    a = pipe.denoise(lat, rl, emb[1:], 2, 1.0, guidance_rescale=0.7)
    assert [k for k, _ in CALLS] == ["ddim", "ddim"] and all(kw == () for _, kw in CALLS)
    b = pipe.denoise(lat, rl, emb[1:], 2, 1.0)
    assert torch.equal(a, b)


def test_call_forwards_guidance_rescale(monkeypatch):
    """MikuDanceVideoPipeline.__call__ and Pose2VideoPipeline.__call__ hand the keyword to denoise() (default 0.0)."""
    import fake_ops
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
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _wp_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    _install_process()
    dp.init(backend="gloo")
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
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_wp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for name, r in res.items():
        assert all(r.values()), (name, r)


# ---- 6. the script
def test_script_flag_parses_and_defaults_to_0():
    from mikudance_amd import inference_video as IV
    assert IV.parse_args([]).guidance_rescale == 0.0
    assert IV.parse_args(["--guidance_rescale", "0.7", "--sampler", "dpmpp_2m"]).guidance_rescale == 0.7
    with pytest.raises(SystemExit):
        IV.parse_args(["--guidance_rescale", "high"])


def _script_tree(tmp_path, frames=2, size=32):
    import yaml
    from PIL import Image
    from mikudance_amd import io_utils as U
    os.makedirs(tmp_path / "inputs")
    rng = np.random.default_rng(0)
    img = lambda: Image.fromarray(rng.integers(0, 255, (size, size, 3), dtype=np.uint8))
    img().save(tmp_path / "inputs" / "ref.png")
    img().save(tmp_path / "inputs" / "skel.png")
    U.save_videos_from_pil([img() for _ in range(frames)], str(tmp_path / "inputs" / "pose.mp4"), fps=12)
    yaml.safe_dump({"noise_scheduler_kwargs": SCHED_KWARGS}, open(tmp_path / "infer.yaml", "w"))
    yaml.safe_dump({"inference_config": str(tmp_path / "infer.yaml"), "weight_dtype": "fp16", "ref_image_path": str(tmp_path / "inputs" / "ref.png"),
                    "ref_skel_path": str(tmp_path / "inputs" / "skel.png"), "ref_depth_path": "None", "tgt_pose_path": str(tmp_path / "inputs" / "pose.mp4"),
                    "tgt_face_path": "None", "tgt_hand_path": "None", "tgt_w2c_path": "None", "tgt_c2w_path": "None"}, open(tmp_path / "cfg.yaml", "w"))
    return str(tmp_path / "cfg.yaml"), size


@pytest.mark.parametrize("argv,want", [([], 0.0), (["--guidance_rescale", "0.7"], 0.7), (["--guidance_rescale", "0.5", "--sampler", "dpmpp_2m_sde"], 0.5)])
def test_script_flag_reaches_denoise(monkeypatch, tmp_path, argv, want):
    import fake_ops
    from mikudance_amd import inference_video as IV
    seen = []

    def build(config, infer_config, weight_dtype, device="cuda", video_decoder=False, sampler="ddim"):
        pipe = M.MikuDanceVideoPipeline(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=None,
                                        denoising_unet=types.SimpleNamespace(in_channels=4), scheduler=IV.build_scheduler(infer_config, sampler))
        pipe._device = torch.device("cpu")
        return pipe

    def spy(self, latents, *a, **kw):
        seen.append((kw["guidance_rescale"], type(self.scheduler).__name__))
        return latents

    monkeypatch.setattr(IV, "build_pipeline", build)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = _script_tree(tmp_path)
    out = IV.main(["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")] + argv)
    assert os.path.exists(out) and len(seen) == 1 and seen[0][0] == want and math.isfinite(seen[0][0])
