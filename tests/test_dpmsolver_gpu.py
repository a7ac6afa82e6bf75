"""GPU: DPM-Solver++ multistep sampling on the MI355X -- md_cfg_multistep_step against an fp32 restatement, the standalone
DPMSolverMultistepScheduler.step, the whole loop against the CPU oracle carrying tests/dpmpp_ref.py (reduced width) and the fp32
restatement on the GPU (full width), order 1 against DDIM, and the drop-in script with --sampler dpmpp_2m.  Plain bounds."""
import json
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

import dpmpp_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
U16 = 2.0 ** -11                      # half an fp16 ulp, relative


def _sched(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _restated_update(lat, ns, cnt, hist, z, halves, g, co):
    """float64 restatement of the kernel on its own inputs -> (latents, m0, scale of the terms)."""
    a_s, s_s, c_x, c_m0, c_m1, c_z = co
    ns, x = ns.double(), lat.double()
    if halves == 2:
        u, c = (ns / cnt.double().view(1, -1, 1, 1)).unbind(0)
        v = u + g * (c - u)
        vabs = u.abs() + g * (c.abs() + u.abs())                      # what the fp32 guidance arithmetic is relative to
    else:
        v = ns[0]
        vabs = v.abs()
    m0 = a_s * x - s_s * v
    out, scale = c_x * x + c_m0 * m0, (c_x * x).abs() + (c_m0 * m0).abs() + (abs(c_m0) + 1.0) * s_s * vabs
    if c_m1:
        out, scale = out + c_m1 * hist.double(), scale + (c_m1 * hist.double()).abs()
    if c_z:
        out, scale = out + c_z * z.double(), scale + (c_z * z.double()).abs()
    return out, m0, scale + (a_s * x).abs() + (s_s * v).abs()


CASES = [  # (halves, Ftot, h, w, step kind)
    (2, 4, 16, 16, "first"), (1, 3, 13, 11, "first"), (2, 32, 13, 11, "second"), (1, 5, 13, 11, "second"),
    (2, 8, 16, 16, "sde"), (2, 32, 13, 11, "sde-second"), (2, 1, 1, 1, "second")]


@pytest.mark.parametrize("halves,ftot,h,w,kind", CASES)
def test_kernel_matches_fp32_restatement(halves, ftot, h, w, kind):
    g = torch.Generator().manual_seed(ftot * 131 + h + halves)
    hw = h * w
    sde = kind.startswith("sde")
    s = _sched(algorithm_type="sde-dpmsolver++" if sde else "dpmsolver++")
    s.set_timesteps(10)
    co = s.multistep_coefficients(0 if kind == "first" else 4)
    assert (co[4] == 0.0) == (kind == "first") and (co[5] != 0.0) == sde
    lat = torch.randn((ftot, hw, 4), generator=g).half()
    ns = torch.randn((halves, ftot, hw, 4), generator=g) * 2
    cnt = torch.randint(1, 4, (ftot,), generator=g).float()          # counters 1..3
    hist = torch.full((ftot, hw, 4), float("nan")) if kind == "first" else torch.randn((ftot, hw, 4), generator=g)
    z = torch.randn((ftot, hw, 4), generator=g).half() if sde else None
    want, m0, scale = _restated_update(lat, ns, cnt, hist, z, halves, 3.5, co)
    ld, hd = lat.to(DEV), hist.to(DEV)
    ops.cfg_multistep_step(ld, ns.to(DEV), cnt.to(DEV), hd, ftot, hw, 3.5, *co, halves=halves, variance_noise=None if z is None else z.to(DEV))
    torch.cuda.synchronize()
    got, gh = ld.cpu().double(), hd.cpu().double()
    assert torch.isfinite(got).all() and torch.isfinite(gh).all()   # the NaN history of a first step is never read
    assert ((got - want).abs() <= U16 * want.abs() + 2e-6 * scale + 2.0 ** -24).all(), float((got - want).abs().max())
    assert float((gh - m0).abs().max()) <= 1e-6 * float(m0.abs().max()), float((gh - m0).abs().max())


def test_kernel_refuses_bad_arguments():
    lat = torch.zeros((2, 8, 4), device=DEV, dtype=torch.float16)
    ns, cnt, hist = torch.zeros((2, 2, 8, 4), device=DEV), torch.ones(2, device=DEV), torch.zeros((2, 8, 4), device=DEV)
    with pytest.raises(M._lib.MdanceHipError):
        M._lib.call("md_cfg_multistep_step", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), hist.data_ptr(), 0, 2, 8, 2, 3.5,
                    0.5, 0.5, 1.0, 1.0, 0.0, 0.5, ops._st())                    # c_z != 0 without variance noise
    with pytest.raises(M._lib.MdanceHipError):
        M._lib.call("md_cfg_multistep_step", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), hist.data_ptr(), 0, 2, 8, 2, 3.5,
                    0.5, 0.5, float("nan"), 1.0, 0.0, 0.0, ops._st())
    with pytest.raises(AssertionError):
        ops.cfg_multistep_step(lat, ns, cnt, hist[:1], 2, 8, 3.5, 0.5, 0.5, 1.0, 1.0, 0.0, 0.0)


@pytest.mark.parametrize("algo", ["dpmsolver++", "sde-dpmsolver++"])
def test_standalone_step_three_calls(algo):
    s = _sched(algorithm_type=algo, solver_type="heun")
    s.set_timesteps(8)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((1, 4, 3, 13, 11), generator=g).half().to(DEV)
    m1 = None
    for i, t in enumerate(s.timesteps.tolist()[:3]):
        v = torch.randn((1, 4, 3, 13, 11), generator=g).half().to(DEV)
        z = torch.randn((1, 4, 3, 13, 11), generator=g).half().to(DEV) if algo.startswith("sde") else None
        out = s.step(v, t, x, variance_noise=z).prev_sample
        a_s, s_s, c_x, c_m0, c_m1, c_z = s.multistep_coefficients(i)
        xd, vd = x.double(), v.double()
        m0 = a_s * xd - s_s * vd
        want = c_x * xd + c_m0 * m0 + (c_m1 * m1 if c_m1 else 0.0) + (c_z * z.double() if z is not None else 0.0)
        scale = (c_x * xd).abs() + (c_m0 * m0).abs() + ((c_m1 * m1).abs() if c_m1 else 0.0) + (a_s * xd).abs() + (s_s * vd).abs()
        assert out.shape == x.shape and out.dtype == torch.float16
        assert ((out.double() - want).abs() <= U16 * want.abs() + 2e-6 * scale + 2.0 ** -24).all(), (i, float((out.double() - want).abs().max()))
        assert (c_m1 != 0.0) == (i == 2)
        x, m1 = out, m0
    s2 = _sched(algorithm_type=algo)
    s2.set_timesteps(8)
    with pytest.raises(RuntimeError, match="second order"):
        s2.step(v, s2.timesteps[2], x)                               # step 2 before steps 0 and 1


@pytest.fixture(scope="module")
def small():
    return build_models()


def _loop(pipe_sched, models, inputs, steps, seed=None, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, pipe_sched)
    gen = torch.Generator().manual_seed(seed) if seed is not None else None
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, 3.5, generator=gen, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _oracle(models, inputs, steps, scheduler=None, **kw):
    _, _, ref_sd, den_sd = models
    with torch.no_grad():
        return O.denoise_loop(ref_sd, den_sd, *inputs, steps, guidance_scale=3.5, reduced=True, scheduler=scheduler, **kw)


@pytest.mark.parametrize("frames,win", [(4, {}), (12, dict(context_frames=8, context_stride=1, context_overlap=4))], ids=["f4", "f12-wrap"])
def test_loop_vs_cpu_oracle_reduced_width(small, frames, win):
    inputs = tuple(t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=200 + frames))
    ddim_err = rel_l2(_loop(M.DDIMScheduler(**SCHED_KWARGS), small, inputs, 8, **win), _oracle(small, inputs, 8, **win))
    modes = [("dpmsolver++", None)] + ([("sde-dpmsolver++", 17)] if frames == 4 else [])
    for algo, seed in modes:
        out = _loop(_sched(algorithm_type=algo), small, inputs, 8, seed=seed, **win)
        want = _oracle(small, inputs, 8, R.Restated(2, algo, "midpoint", generator=torch.Generator().manual_seed(seed) if seed else None), **win)
        r, c = rel_l2(out, want), cosine(out, want)
        print(f"\nDPM_LOOP f={frames} {algo} 8 steps rel_l2 {r:.3e} cos {c:.7f} (DDIM same clip {ddim_err:.3e})")
        # The SDE variant measured 2.65x the DDIM loop's error on this clip (1.32e-2 vs 4.99e-3, MI355X), the ODE 2M 1.1x.  It keeps less
        # of the carried state (x is scaled by e^-h once more) and gives each step's data prediction the weight alpha_t (1 - e^-2h) instead of
        # alpha_t (1 - e^-h), so the fp16 error of each UNet evaluation counts for more.  The emulated operators show the same ordering on the
        # CPU (tests/test_dpmsolver_cpu.py::test_host_loop_matches_oracle).  Its factor is therefore 4; SURVEY 8c's plain bound holds for both.
        factor = 4.0 if algo.startswith("sde") else 2.0
        assert r <= 3e-2 and c >= 0.999 and r <= factor * ddim_err, (r, c, ddim_err)


def test_full_width_10_steps_2m_vs_fp32_restatement(full):
    from e2e_parity import _oracle_run
    ref, den, ref_sd, den_sd = full
    inputs = tuple(t.half().float() for t in synth_inputs(4, 96, 96, ctx_len=257, ctx_dim=768, seed=100))
    out = _loop(_sched(), full, inputs, 10)
    o32, _ = _oracle_run(O, ref_sd, den_sd, inputs, 10, 3.5, torch.float32, DEV, scheduler=R.Restated(2, "dpmsolver++", "midpoint"))
    r, c = rel_l2(out, o32), cosine(out, o32)
    print("\nDPM_FULL_WIDTH " + json.dumps({"frames": 4, "latent": 96, "steps": 10, "sampler": "dpmpp_2m", "rel_l2": r, "cosine": c}))
    assert r <= 3e-2 and c >= 0.999, (r, c)


def test_order1_solver_vs_ddim_20_steps_full_width(full):
    inputs = tuple(t.half().float() for t in synth_inputs(4, 96, 96, ctx_len=257, ctx_dim=768, seed=100))
    a = _loop(_sched(solver_order=1), full, inputs, 20)
    b = _loop(M.DDIMScheduler(**SCHED_KWARGS), full, inputs, 20)
    r, c = rel_l2(a, b), cosine(a, b)
    print("\nDPM_ORDER1_VS_DDIM " + json.dumps({"frames": 4, "latent": 96, "steps": 20, "rel_l2": r, "cosine": c}))
    assert r <= 1e-2 and c >= 0.9999, (r, c)


def test_script_sampler_dpmpp_2m(tmp_path, golden_dir):
    import numpy as np
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir)
    out = inference_video.main(["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "3", "--seed", "7", "--sampler", "dpmpp_2m",
                                "--output_dir", str(tmp_path / "output")])
    frames = U.read_frames(out)
    a = np.asarray(frames[0], dtype=np.float32)
    assert len(frames) == F_ and np.isfinite(a).all() and a[:, 2 * (W + 2):].std() > 0
    assert math.isfinite(float(a.mean()))
