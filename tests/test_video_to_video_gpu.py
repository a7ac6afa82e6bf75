"""GPU: video-to-video sampling on the MI355X -- md_add_noise_f16 against float64 (the a == 0 rule, the argument checks), both schedulers'
add_noise, DPM-Solver++ step() after set_begin_index, strength 1.0 with init_latents bitwise equal to the plain loop, strength 0.5 / 0.3 at
reduced width against the CPU oracle on a truncated, pre-noised schedule (tests/v2v_ref.py), and the drop-in script with --init_video.
Bounds as tests/test_dpmsolver_gpu.py."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

import dpmpp_ref as R  # noqa: E402
import v2v_ref as V  # noqa: E402

DEV = torch.device("cuda:0")
U16 = 2.0 ** -11                      # half an fp16 ulp, relative


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _ab(t):
    abar = float(O.DDIM().alphas_cumprod[t])
    return math.sqrt(abar), math.sqrt(1.0 - abar)


def _close(got, want, scale):
    return ((got - want).abs() <= U16 * want.abs() + 1e-6 * scale + 2.0 ** -24).all()


# ---- 1. the kernel
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 4099, 65536 + 7, 4096 * 256 + 77])
@pytest.mark.parametrize("t", [999, 624, 249, 0])
def test_kernel_matches_float64(n, t):
    g = torch.Generator().manual_seed(n + t)
    x0 = (torch.randn(n, generator=g) * 3).half()
    z = torch.randn(n, generator=g).half()
    a, b = _ab(t)
    lat = z.to(DEV)
    ops.add_noise(lat, x0.to(DEV), a, b)
    torch.cuda.synchronize()
    want = a * x0.double() + b * z.double()
    got = lat.cpu().double()
    assert _close(got, want, (a * x0.double()).abs() + (b * z.double()).abs()), float((got - want).abs().max())
    if t == 999:
        assert a == 0.0 and b == 1.0 and torch.equal(lat.cpu(), z)


def test_a_zero_never_reads_x0():
    z = torch.randn(1000, generator=torch.Generator().manual_seed(1)).half()
    x0 = torch.full((1000,), float("nan"), dtype=torch.float16)
    x0[::3] = float("inf")
    x0[1::3] = -float("inf")
    for b in (1.0, 0.75):
        lat = z.to(DEV)
        ops.add_noise(lat, x0.to(DEV), 0.0, b)
        torch.cuda.synchronize()
        assert torch.equal(lat.cpu(), (z.float() * b).half())
    lat = z.to(DEV)
    ops.add_noise(lat, x0.to(DEV), 0.5, 0.5)                       # a != 0: x0 is read, NaN / Inf propagate
    torch.cuda.synchronize()
    assert not torch.isfinite(lat.cpu()).any()


def test_kernel_refuses_bad_arguments():
    lat = torch.zeros(64, device=DEV, dtype=torch.float16)
    x0 = torch.zeros(64, device=DEV, dtype=torch.float16)
    p, q, st = lat.data_ptr(), x0.data_ptr(), ops._st()
    for args in ((p, q, 0, 0.5, 0.5), (p, q, -4, 0.5, 0.5), (0, q, 8, 0.5, 0.5), (p, 0, 8, 0.0, 1.0), (p + 1, q, 8, 0.5, 0.5), (p, q + 1, 8, 0.5, 0.5),
                 (p, q, 8, float("nan"), 0.5), (p, q, 8, 0.5, float("inf")), (p, q, 8, -0.5, 0.5), (p, q, 8, 0.5, -0.5)):
        with pytest.raises(M._lib.MdanceHipError, match="md_add_noise_f16"):
            M._lib.call("md_add_noise_f16", *args, st)
        assert M._lib.load().md_add_noise_f16(*args, st) == -1       # MD_ERR_ARG
    torch.cuda.synchronize()
    assert not lat.any()
    with pytest.raises(AssertionError):
        ops.add_noise(lat, x0[:32], 0.5, 0.5)


# ---- 2. the schedulers' add_noise and DPM step() from a begin index
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_scheduler_add_noise(make):
    s = make()
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn((3, 4, 2, 5, 7), generator=g)
    z = torch.randn((3, 4, 2, 5, 7), generator=g)
    for ts in (torch.tensor(499), torch.tensor([624]), torch.tensor([999, 499, 0])):
        out = s.add_noise(x0.to(DEV), z.to(DEV), ts.to(DEV))
        assert out.shape == x0.shape and out.dtype == torch.float32 and out.is_cuda
        tl = ts.reshape(-1).tolist() * (3 if ts.numel() == 1 else 1)
        for k, t in enumerate(tl):
            a, b = _ab(t)
            xh, zh = x0[k].half().double(), z[k].half().double()
            want = a * xh + b * zh
            assert _close(out[k].cpu().double(), want, (a * xh).abs() + (b * zh).abs()), (t, k)
            if t == 999:
                assert torch.equal(out[k].cpu(), z[k].half().float())
    with pytest.raises(ValueError):
        s.add_noise(x0.to(DEV), z.to(DEV), torch.tensor([1, 2]))
    with pytest.raises(RuntimeError, match="GPU"):
        s.add_noise(x0, z, torch.tensor(10))


@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
def test_dpm_step_honours_the_begin_index(algo):
    s = _dpm(algorithm_type=algo)
    s.set_timesteps(8)
    ts, kept = s.get_timesteps(8, 0.5)
    assert kept == 4 and s.begin_index == 4
    g = torch.Generator().manual_seed(8)
    x = torch.randn((1, 4, 2, 9, 7), generator=g).half().to(DEV)
    m1 = None
    for j, t in enumerate(ts.tolist()[:3]):
        v = torch.randn(x.shape, generator=g).half().to(DEV)
        z = torch.randn(x.shape, generator=g).half().to(DEV) if algo.startswith("sde") else None
        out = s.step(v, t, x, variance_noise=z).prev_sample          # step 4 first: no history needed
        a_s, s_s, c_x, c_m0, c_m1, c_z = s.multistep_coefficients(4 + j)
        xd, vd = x.double(), v.double()
        m0 = a_s * xd - s_s * vd
        want = c_x * xd + c_m0 * m0 + (c_m1 * m1 if c_m1 else 0.0) + (c_z * z.double() if z is not None else 0.0)
        scale = (c_x * xd).abs() + (c_m0 * m0).abs() + ((c_m1 * m1).abs() if c_m1 else 0.0) + (a_s * xd).abs() + (s_s * vd).abs()
        assert (c_m1 == 0.0) == (j == 0)
        assert ((out.double() - want).abs() <= U16 * want.abs() + 2e-6 * scale + 2.0 ** -24).all(), (j, float((out.double() - want).abs().max()))
        x, m1 = out, m0


# ---- 3. the loop
@pytest.fixture(scope="module")
def small():
    return build_models()


def _inputs(frames, seed):
    lat, rl, emb = (t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=seed))
    x0 = (torch.randn(lat.shape, generator=torch.Generator().manual_seed(seed + 1)) * 0.8).half().float()
    return lat, rl, emb, x0


def _loop(sch, models, inputs, steps, seed=None, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    gen = torch.Generator().manual_seed(seed) if seed is not None else None
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, 3.5, generator=gen, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


SAMPLERS = {"ddim": (_ddim, {}), "ddim-eta": (_ddim, dict(eta=0.5)), "2m": (lambda: _dpm(), {}),
            "2m-sde": (lambda: _dpm(algorithm_type="sde-dpmsolver++"), {})}


@pytest.mark.parametrize("phi", [0.0, 0.7], ids=["plain", "rescale"])
@pytest.mark.parametrize("sampler", list(SAMPLERS))
def test_strength_1_is_bitwise_the_plain_loop(small, sampler, phi):
    make, kw = SAMPLERS[sampler]
    lat, rl, emb, x0 = _inputs(4, 61)
    x0[0, 0, 0, 0, 0], x0[0, 3, 3, 2, 1] = float("nan"), float("inf")   # never read at t = 999
    a = _loop(make(), small, (lat, rl, emb), 4, seed=13, guidance_rescale=phi, **kw)
    b = _loop(make(), small, (lat, rl, emb), 4, seed=13, guidance_rescale=phi, init_latents=x0.half().to(DEV), strength=1.0, **kw)
    print(f"\nV2V_STRENGTH1 {sampler} phi {phi}: torch.equal {torch.equal(a, b)}")
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("strength", [0.5, 0.3])
def test_loop_vs_cpu_oracle_reduced_width(small, strength):
    _, _, ref_sd, den_sd = small
    lat, rl, emb, x0 = _inputs(4, 71)
    with torch.no_grad():
        plain = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 8, guidance_scale=3.5, reduced=True)
    ddim_err = rel_l2(_loop(_ddim(), small, (lat, rl, emb), 8), plain)
    modes = [("ddim", None), ("dpmsolver++", None)] + ([("sde-dpmsolver++", 17)] if strength == 0.5 else [])
    for algo, seed in modes:
        sch = _ddim() if algo == "ddim" else _dpm(algorithm_type=algo)
        out = _loop(sch, small, (lat, rl, emb), 8, seed=seed, init_latents=x0.half().to(DEV), strength=strength)
        inner = O.DDIM() if algo == "ddim" else R.Restated(2, algo, "midpoint", generator=torch.Generator().manual_seed(seed) if seed else None)
        with torch.no_grad():
            want = V.denoise_loop(ref_sd, den_sd, lat, rl, emb, 8, x0, strength, scheduler=inner, guidance_scale=3.5, reduced=True)
        r, c = rel_l2(out, want), cosine(out, want)
        print(f"\nV2V_LOOP strength {strength} {algo} 8 steps ({V.kept_steps(8, strength)} kept) rel_l2 {r:.3e} cos {c:.7f} "
              f"(plain DDIM loop same clip {ddim_err:.3e})")
        factor = 4.0 if algo.startswith("sde") else 2.0            # as tests/test_dpmsolver_gpu.py
        assert r <= 3e-2 and c >= 0.999 and r <= factor * ddim_err, (r, c, ddim_err)
        assert rel_l2(want, plain) > 0.1                           # the start matters


def test_script_init_video_strength_half(tmp_path, golden_dir):
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir)
    rng = np.random.default_rng(5)
    from PIL import Image
    init = str(tmp_path / "inputs" / "init.mp4")
    U.save_videos_from_pil([Image.fromarray(rng.integers(0, 255, (H, W, 3), dtype=np.uint8)) for _ in range(F_)], init, fps=12)
    out = inference_video.main(["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "4", "--seed", "7", "--init_video", init,
                                "--strength", "0.5", "--output_dir", str(tmp_path / "output")])
    frames = U.read_frames(out)
    a = np.asarray(frames[0], dtype=np.float32)
    assert len(frames) == F_ and np.isfinite(a).all() and a[:, 2 * (W + 2):].std() > 0
