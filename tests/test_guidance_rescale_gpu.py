"""GPU: guidance rescale on the MI355X -- md_cfg_guidance_rescale's factor against float64 over many shapes, determinism, the scaled DDIM /
DPM-Solver++ steps against a float64 restatement on their own inputs, the std(v) == 0 rule and the argument checks, bitwise equality at
phi = 0, the whole loop against tests/rescale_ref.py (reduced width on the CPU oracle, full width against the fp32 restatement on the GPU),
and the drop-in script with --guidance_rescale.  Plain bounds, those of tests/test_dpmsolver_gpu.py."""
import contextlib
import json
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

import dpmpp_ref as R  # noqa: E402
import rescale_ref as RR  # noqa: E402

DEV = torch.device("cuda:0")
U16 = 2.0 ** -11                      # half an fp16 ulp, relative
WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)


def _sched(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _data(ftot, h, w, seed, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    hw = h * w
    cnt = torch.randint(1, 4, (ftot,), generator=g).float()                # counters 1..3
    ns = (torch.randn((2, ftot, hw, 4), generator=g) * torch.tensor([0.7, 1.3]).view(2, 1, 1, 1) + offset) * cnt.view(1, -1, 1, 1)
    return ns, cnt


def _factor64(ns, cnt, g, phi):
    u, c = (ns.double() / cnt.double().view(1, -1, 1, 1)).unbind(0)
    v = u + g * (c - u)
    sc, sv = float(c.std()), float(v.std())
    return 1.0 if sv == 0.0 else 1.0 - phi + phi * sc / sv


# ---- 1. the statistics kernel against float64
FACTOR_CASES = [  # (Ftot, h, w, common offset)
    (1, 1, 1, 0.0), (1, 13, 11, 0.0), (3, 13, 11, 0.0), (16, 13, 11, 0.0), (48, 13, 11, 0.0), (3, 1, 1, 0.0), (16, 16, 16, 0.0),
    (5, 7, 9, 0.0), (48, 128, 128, 0.0), (3, 13, 11, 1000.0), (16, 96, 96, 300.0), (48, 128, 128, 1000.0)]


@pytest.mark.parametrize("ftot,h,w,offset", FACTOR_CASES)
def test_factor_matches_float64(ftot, h, w, offset):
    ns, cnt = _data(ftot, h, w, seed=ftot * 7 + h + w, offset=offset)
    nd, cd = ns.to(DEV), cnt.to(DEV)
    for g, phi in ((3.5, 1.0), (3.5, 0.7), (7.5, 0.25)):
        want = _factor64(ns, cnt, g, phi)
        got = float(ops.cfg_guidance_rescale(nd, cd, ftot, h * w, g, phi).cpu())
        assert math.isfinite(got) and abs(got - want) <= 1e-5 * abs(want), (ftot, h, w, offset, g, phi, got, want)


def test_factor_and_step_are_deterministic():
    ns, cnt = _data(48, 128, 128, seed=3, offset=0.5)
    nd, cd = ns.to(DEV), cnt.to(DEV)
    lat0 = torch.randn((48, 128 * 128, 4), generator=torch.Generator().manual_seed(4)).half().to(DEV)
    outs = []
    for _ in range(2):
        f = ops.cfg_guidance_rescale(nd, cd, 48, 128 * 128, 3.5, 0.7)
        lat = lat0.clone()
        ops.cfg_ddim_step(lat, nd, cd, 48, 128 * 128, 3.5, 0.3, 0.5, vscale=f)
        hist = torch.zeros((48, 128 * 128, 4), device=DEV)
        lat2 = lat0.clone()
        ops.cfg_multistep_step(lat2, nd, cd, hist, 48, 128 * 128, 3.5, 0.5, 0.8, 0.9, 0.4, 0.0, 0.0, vscale=f)
        torch.cuda.synchronize()
        outs.append((f.cpu(), lat.cpu(), lat2.cpu(), hist.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- 2. the scaled steps against float64 on their own inputs (the factor read back and fed to the restatement)
def _ddim64(lat, ns, cnt, g, f, a_t, a_p, eta, z):
    u, c = (ns.double() / cnt.double().view(1, -1, 1, 1)).unbind(0)
    v = (u + g * (c - u)) * f
    vabs = (u.abs() + g * (c.abs() + u.abs())) * abs(f)
    x = lat.double()
    std = eta * math.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p)) if eta else 0.0
    sa, sb, sap, sdir = math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_p), math.sqrt(max(1 - a_p - std * std, 0.0))
    x0, ep = sa * x - sb * v, sa * v + sb * x
    out = sap * x0 + sdir * ep
    scale = sap * (sa * x.abs() + sb * vabs) + sdir * (sa * vabs + sb * x.abs())
    if eta:
        out, scale = out + std * z.double(), scale + (std * z.double()).abs()
    return out, scale


def _dpm64(lat, ns, cnt, hist, z, g, f, co):
    a_s, s_s, c_x, c_m0, c_m1, c_z = co
    u, c = (ns.double() / cnt.double().view(1, -1, 1, 1)).unbind(0)
    v = (u + g * (c - u)) * f
    vabs = (u.abs() + g * (c.abs() + u.abs())) * abs(f)
    x = lat.double()
    m0 = a_s * x - s_s * v
    out, scale = c_x * x + c_m0 * m0, (c_x * x).abs() + (c_m0 * m0).abs() + (abs(c_m0) + 1.0) * s_s * vabs
    if c_m1:
        out, scale = out + c_m1 * hist.double(), scale + (c_m1 * hist.double()).abs()
    if c_z:
        out, scale = out + c_z * z.double(), scale + (c_z * z.double()).abs()
    return out, m0, scale + (a_s * x).abs() + (s_s * v).abs()


STEP_CASES = [(4, 16, 16), (3, 13, 11), (32, 13, 11), (1, 1, 1)]


@pytest.mark.parametrize("ftot,h,w", STEP_CASES)
@pytest.mark.parametrize("kind", ["ddim", "ddim-eta", "2m", "2m-sde"])
def test_scaled_step_matches_float64(ftot, h, w, kind):
    hw = h * w
    g = torch.Generator().manual_seed(ftot * 31 + hw)
    ns, cnt = _data(ftot, h, w, seed=ftot + hw)
    lat = torch.randn((ftot, hw, 4), generator=g).half()
    z = torch.randn((ftot, hw, 4), generator=g).half()
    nd, cd = ns.to(DEV), cnt.to(DEV)
    vs = ops.cfg_guidance_rescale(nd, cd, ftot, hw, 3.5, 0.7)
    f = float(vs.cpu())
    assert abs(f - _factor64(ns, cnt, 3.5, 0.7)) <= 1e-5 * abs(f)
    ld = lat.to(DEV)
    if kind.startswith("ddim"):
        eta = 0.6 if kind == "ddim-eta" else 0.0
        d = M.DDIMScheduler(**SCHED_KWARGS)
        d.set_timesteps(10)
        a_t, a_p = d.step_coefficients(int(d.timesteps[3]))
        want, scale = _ddim64(lat, ns, cnt, 3.5, f, a_t, a_p, eta, z)
        ops.cfg_ddim_step(ld, nd, cd, ftot, hw, 3.5, a_t, a_p, eta=eta, variance_noise=z.to(DEV) if eta else None, vscale=vs)
        torch.cuda.synchronize()
        got = ld.cpu().double()
    else:
        s = _sched(algorithm_type="sde-dpmsolver++" if kind == "2m-sde" else "dpmsolver++")
        s.set_timesteps(10)
        co = s.multistep_coefficients(4)
        assert co[4] != 0.0 and (co[5] != 0.0) == (kind == "2m-sde")
        hist = torch.randn((ftot, hw, 4), generator=g)
        want, m0, scale = _dpm64(lat, ns, cnt, hist, z, 3.5, f, co)
        hd = hist.to(DEV)
        ops.cfg_multistep_step(ld, nd, cd, hd, ftot, hw, 3.5, *co, variance_noise=z.to(DEV) if co[5] else None, vscale=vs)
        torch.cuda.synchronize()
        got = ld.cpu().double()
        assert float((hd.cpu().double() - m0).abs().max()) <= 1e-6 * float(m0.abs().max())
    assert torch.isfinite(got).all()
    assert ((got - want).abs() <= U16 * want.abs() + 2e-6 * scale + 2.0 ** -24).all(), float((got - want).abs().max())


def test_constant_clip_is_left_unscaled():
    ftot, hw = 3, 143
    ns = torch.full((2, ftot, hw, 4), 0.375, device=DEV)
    cnt = torch.full((ftot,), 2.0, device=DEV)
    f = ops.cfg_guidance_rescale(ns, cnt, ftot, hw, 3.5, 0.7)
    assert float(f.cpu()) == 1.0
    lat0 = torch.randn((ftot, hw, 4), generator=torch.Generator().manual_seed(2)).half().to(DEV)
    a, b = lat0.clone(), lat0.clone()
    ops.cfg_ddim_step(a, ns, cnt, ftot, hw, 3.5, 0.3, 0.5)
    ops.cfg_ddim_step(b, ns, cnt, ftot, hw, 3.5, 0.3, 0.5, vscale=f)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_bad_arguments_raise():
    ftot, hw = 2, 8
    ns, cnt = torch.zeros((2, ftot, hw, 4), device=DEV), torch.ones(ftot, device=DEV)
    lat, hist = torch.zeros((ftot, hw, 4), device=DEV, dtype=torch.float16), torch.zeros((ftot, hw, 4), device=DEV)
    out = torch.zeros(2, device=DEV)
    need = _lib.load().md_cfg_rescale_workspace_bytes(ftot, hw)
    ws = torch.zeros(1024, device=DEV, dtype=torch.float64)
    assert 0 < need <= 16384
    rescale = lambda nsp=ns.data_ptr(), halves=2, g=3.5, phi=0.7, wsb=ws.numel() * 8, o=out.data_ptr(): _lib.call(
        "md_cfg_guidance_rescale", nsp, cnt.data_ptr(), ftot, hw, halves, g, phi, ws.data_ptr(), wsb, o, ops._st())
    rescale()                                                              # the valid call
    for kw in (dict(phi=-0.1), dict(phi=1.5), dict(phi=float("nan")), dict(g=float("inf")), dict(halves=1), dict(wsb=need - 8),
               dict(nsp=ns.data_ptr() + 4), dict(o=out.data_ptr() + 2), dict(o=0)):
        with pytest.raises(_lib.MdanceHipError):
            rescale(**kw)
    with pytest.raises(_lib.MdanceHipError):                               # the scaled steps: no factor, one clip-half
        _lib.call("md_cfg_ddim_step_scaled", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), 0, 0, ftot, hw, 2, 3.5, 0.3, 0.5, 0.0, ops._st())
    with pytest.raises(_lib.MdanceHipError):
        _lib.call("md_cfg_ddim_step_scaled", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), 0, out.data_ptr(), ftot, hw, 1, 3.5, 0.3, 0.5, 0.0,
                  ops._st())
    with pytest.raises(_lib.MdanceHipError):
        _lib.call("md_cfg_multistep_step_scaled", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), hist.data_ptr(), 0, 0, ftot, hw, 2, 3.5,
                  0.5, 0.5, 1.0, 1.0, 0.0, 0.0, ops._st())
    with pytest.raises(_lib.MdanceHipError):
        _lib.call("md_cfg_multistep_step_scaled", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), hist.data_ptr(), 0, out.data_ptr(), ftot, hw,
                  2, 3.5, 0.5, 0.5, 1.0, 1.0, 0.0, 0.5, ops._st())            # c_z != 0 without variance noise
    # the unscaled DDIM entries share those checks: a null buffer or a non-finite coefficient is refused and the latents stay as they were
    lat.copy_(torch.randn(lat.shape, generator=torch.Generator().manual_seed(3)))
    keep, z = lat.clone(), torch.zeros_like(lat)
    nan, inf = float("nan"), float("inf")
    plain = lambda l=lat.data_ptr(), n=ns.data_ptr(), c=cnt.data_ptr(), halves=2, g=3.5, a_t=0.3, a_p=0.5: _lib.call(
        "md_cfg_ddim_step", l, n, c, ftot, hw, halves, g, a_t, a_p, ops._st())
    with_eta = lambda l=lat.data_ptr(), n=ns.data_ptr(), c=cnt.data_ptr(), zp=z.data_ptr(), halves=2, g=3.5, a_t=0.3, a_p=0.5, eta=0.5: _lib.call(
        "md_cfg_ddim_step_eta", l, n, c, zp, ftot, hw, halves, g, a_t, a_p, eta, ops._st())
    common = (dict(l=0), dict(n=0), dict(c=0), dict(a_t=nan), dict(a_p=nan), dict(g=inf), dict(g=nan), dict(halves=3))
    for call, cases in ((plain, common), (with_eta, common + (dict(eta=nan), dict(eta=inf), dict(eta=-0.5), dict(zp=0)))):
        for kw in cases:
            with pytest.raises(_lib.MdanceHipError):
                call(**kw)
            assert torch.equal(lat, keep), kw
    plain(c=0, halves=1)                                                   # no CFG: the counter is not read and may be NULL
    with_eta(zp=0, eta=0.0)                                                # eta == 0: neither is the noise
    assert torch.isfinite(lat).all() and not torch.equal(lat, keep)
    torch.cuda.synchronize()


# ---- 3. the loop
@pytest.fixture(scope="module")
def small():
    return build_models()


def _loop(sch, models, inputs, steps, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, 3.5, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_phi_0_is_bitwise_the_unscaled_loop(small, monkeypatch, sampler):
    inputs = synth_inputs(4, 16, 16, ctx_len=5, ctx_dim=64, seed=71)
    mk = lambda: M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _sched()
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    a = _loop(mk(), small, inputs, 4, guidance_rescale=0.0)
    seen_a = [n for n in names if n.startswith("md_cfg")]
    del names[:]
    b = _loop(mk(), small, inputs, 4)
    assert torch.equal(a, b)
    assert seen_a == [n for n in names if n.startswith("md_cfg")] == ["md_cfg_ddim_step" if sampler == "ddim" else "md_cfg_multistep_step"] * 4
    del names[:]
    c = _loop(mk(), small, inputs, 4, guidance_rescale=0.7)
    assert [n for n in names if n.startswith("md_cfg")] == ["md_cfg_guidance_rescale", "md_cfg_ddim_step_scaled" if sampler == "ddim"
                                                            else "md_cfg_multistep_step_scaled"] * 4
    d = rel_l2(c, b)
    print(f"\nRESCALE_EFFECT {sampler} rel_l2(phi 0.7, phi 0) {d:.3e}")
    assert d > 1e-2, d                                                     # the keyword is not silently ignored


def _restated(models, inputs, steps, scheduler=None, phi=0.7, **win):
    _, _, ref_sd, den_sd = models
    with torch.no_grad():
        return RR.denoise_loop(ref_sd, den_sd, *inputs, steps, guidance_scale=3.5, reduced=True, scheduler=scheduler, guidance_rescale=phi, **win)


@pytest.mark.parametrize("frames,win", [(4, {}), (12, WRAP12)], ids=["f4", "f12-wrap"])
def test_loop_vs_restatement_reduced_width(small, frames, win):
    inputs = tuple(t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=300 + frames))
    ddim_err = rel_l2(_loop(M.DDIMScheduler(**SCHED_KWARGS), small, inputs, 8, **win), _restated(small, inputs, 8, phi=0.0, **win))
    for name, sch, rs in (("ddim", M.DDIMScheduler(**SCHED_KWARGS), None), ("2m", _sched(), R.Restated(2, "dpmsolver++", "midpoint"))):
        out = _loop(sch, small, inputs, 8, guidance_rescale=0.7, **win)
        want = _restated(small, inputs, 8, scheduler=rs, phi=0.7, **win)
        r, c = rel_l2(out, want), cosine(out, want)
        print(f"\nRESCALE_LOOP f={frames} {name} phi 0.7 8 steps rel_l2 {r:.3e} cos {c:.7f} (DDIM without rescale, same clip {ddim_err:.3e})")
        assert r <= 3e-2 and c >= 0.999 and r <= 2.0 * ddim_err, (r, c, ddim_err)


def test_full_width_10_steps_vs_fp32_restatement(full):
    ref, den, ref_sd, den_sd = full
    inputs = tuple(t.half().float() for t in synth_inputs(4, 96, 96, ctx_len=257, ctx_dim=768, seed=100))
    out = _loop(M.DDIMScheduler(**SCHED_KWARGS), full, inputs, 10, guidance_rescale=0.7)
    cast = lambda sd: {k: v.to(device=DEV, dtype=torch.float32 if v.is_floating_point() else v.dtype) for k, v in sd.items()}
    rs, ds = cast(ref_sd), cast(den_sd)
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):      # exact fp32 convolutions, as tests/e2e_parity.py
        o32 = RR.denoise_loop(rs, ds, *(t.to(DEV) for t in inputs), 10, guidance_scale=3.5, reduced=True, guidance_rescale=0.7).float().cpu()
    del rs, ds
    torch.cuda.empty_cache()
    r, c = rel_l2(out, o32), cosine(out, o32)
    print("\nRESCALE_FULL_WIDTH " + json.dumps({"frames": 4, "latent": 96, "steps": 10, "sampler": "ddim", "guidance_rescale": 0.7,
                                                "rel_l2": r, "cosine": c}))
    assert r <= 3e-2 and c >= 0.999, (r, c)


def test_script_guidance_rescale(tmp_path, golden_dir):
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir)
    out = inference_video.main(["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "3", "--seed", "7", "--guidance_rescale", "0.7",
                                "--output_dir", str(tmp_path / "output")])
    frames = U.read_frames(out)
    a = np.asarray(frames[0], dtype=np.float32)
    assert len(frames) == F_ and np.isfinite(a).all() and a[:, 2 * (W + 2):].std() > 0
