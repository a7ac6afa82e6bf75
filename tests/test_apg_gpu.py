"""GPU: adaptive projected guidance on the MI355X -- md_cfg_apg_prepare's per-frame coefficients and momentum buffer against float64 on the
same inputs over many shapes and settings, the *_apg steps against a float64 restatement on their own inputs, determinism, the argument
checks, bitwise equality with apg=False, the whole loop against tests/apg_ref.py at reduced width, and the drop-in script with --apg.
Plain bounds, those of tests/test_guidance_rescale_gpu.py.

Measured on an MI355X (profiles/apg_tests.log holds every printed figure): S within 1e-7 relative, m within 1.2e-7 max|m|, the loop at
eta = 0, beta = -0.5 and a median threshold rel_l2 4.1e-3 ... 1.2e-2 (1.0 - 1.4 x the plain DDIM loop's error on the same clip)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

import apg_ref as A  # noqa: E402
import dpmpp_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
U16 = 2.0 ** -11                      # half an fp16 ulp, relative
WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)
G = 7.5


def _sched(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _data(ftot, h, w, seed):
    """(noise_sum, counter, latents, previous momentum) on the host.  The frames' u - c are scaled very differently (so that a threshold
    caps some and not others); with three frames or more, frame 1 has u == c (and no previous momentum) and frame 2 has D_c == 0."""
    g = torch.Generator().manual_seed(seed)
    hw = h * w
    cnt = torch.randint(1, 4, (ftot,), generator=g).float()                # counters 1..3
    u, c = (torch.randn((2, ftot, hw, 4), generator=g) * torch.tensor([0.7, 1.3]).view(2, 1, 1, 1)).unbind(0)
    scale = torch.tensor([0.1, 1.0, 3.0, 10.0])[torch.arange(ftot) % 4].view(-1, 1, 1)
    u = c + (u - c) * scale
    lat = torch.randn((ftot, hw, 4), generator=g).half()
    mprev = torch.randn((ftot, hw, 4), generator=g) * 0.5
    if ftot >= 3:
        u[1] = c[1]
        mprev[1] = 0.0
        c[2] = 0.0
        lat[2] = 0.0
    ns = torch.stack([u, c]) * cnt.view(1, -1, 1, 1)
    if ftot >= 3:
        assert torch.equal(ns[0, 1] / cnt[1], ns[1, 1] / cnt[1])
    return ns, cnt, lat, mprev


def _ref64(ns, cnt, lat, mprev, a, s, beta, eta, r):
    u, c = (ns.double() / cnt.double().view(1, -1, 1, 1)).unbind(0)
    return A.apg(u, c, lat.double(), a, s, G, eta, r, beta, mprev.double(), (1, 2))


def _prepare(ns, cnt, lat, mbuf, a, s, beta, eta, r):
    ftot, hw = lat.shape[0], lat.shape[1]
    coef = torch.empty((ftot, 2), device=DEV)
    ops.cfg_apg_prepare(lat, ns, cnt, mbuf, coef, ftot, hw, a, s, beta, eta, r)
    return coef


# ---- 1. coef and the momentum buffer against float64 on the same fp32 / fp16 inputs
PREPARE_CASES = [(1, 1, 1), (3, 1, 1), (3, 13, 11), (5, 7, 9), (32, 13, 11), (16, 16, 16), (16, 96, 96), (48, 128, 128)]
SETTINGS = [(0.0, 0.0, False), (-0.5, 0.0, True), (0.5, 0.3, True)]       # (beta, eta, with a threshold r_mid)


@pytest.mark.parametrize("ftot,h,w", PREPARE_CASES)
def test_coef_and_momentum_match_float64(ftot, h, w):
    ns, cnt, lat, mprev = _data(ftot, h, w, seed=ftot * 11 + h + w)
    a, s = 0.6, 0.8
    nd, cd, ld = ns.to(DEV), cnt.to(DEV), lat.to(DEV)
    for beta, eta, capped in SETTINGS:
        free = _ref64(ns, cnt, lat, mprev, a, s, beta, eta, 0.0)
        norms = free["N2"].flatten().sqrt()
        # r_mid from the data: the median norm of the frames that have one (one frame: half its norm)
        r = float(np.float32(norms[norms > 0].median() * (0.5 if ftot == 1 else 1.0))) if capped and (norms > 0).any() else 0.0
        want = _ref64(ns, cnt, lat, mprev, a, s, beta, eta, r)
        S64, p64, N2, Q = (want[k].flatten() for k in ("S", "proj", "N2", "Q"))
        if capped and ftot >= 3:
            assert (S64 < 1).any() and (S64 == 1).any(), S64              # some frames are capped and some are not
        if ftot >= 3:
            assert float(Q[2]) == 0.0 and (beta != 0.0 or float(N2[1]) == 0.0)
        mbuf = mprev.to(DEV) if beta != 0.0 else torch.full(mprev.shape, float("nan"), device=DEV)      # beta == 0 never reads it
        coef = _prepare(nd, cd, ld, mbuf, a, s, beta, eta, r)
        torch.cuda.synchronize()
        got, m = coef.cpu().double(), mbuf.cpu().double()
        assert torch.isfinite(got).all() and torch.isfinite(m).all()
        S, K = got[:, 0], got[:, 1]
        proj = K / ((1.0 - eta) * S)
        size = torch.where(Q == 0, torch.zeros_like(Q), (N2 / torch.where(Q == 0, torch.ones_like(Q), Q)).sqrt())      # |proj| <= sqrt(N2 / Q)
        es, ep = float(((S - S64).abs() / S64).max()), float(((proj - p64).abs() - 1e-5 * size).max())
        em = float((m - want["m"]).abs().max()) / max(float(want["m"].abs().max()), 1e-30)
        print(f"\nAPG_PREPARE ({ftot},{h},{w}) beta {beta} eta {eta} r {r:.4g}: dS/S {es:.2e}  max(|dproj| - 1e-5 sqrt(N2/Q)) {ep:.2e}  dm/max|m| {em:.2e}")
        assert ((S - S64).abs() <= 1e-5 * S64).all(), (S, S64)
        assert ((proj - p64).abs() <= 1e-5 * size).all(), (proj, p64, size)
        assert (K[Q == 0] == 0).all() and (S[N2 == 0] == 1).all()
        assert float((m - want["m"]).abs().max()) <= 1e-6 * float(want["m"].abs().max()) or float(want["m"].abs().max()) == 0.0


# ---- 2. each *_apg step against float64 on its own inputs, coef and the momentum buffer read back from the device
def _vg64(ns, cnt, lat, m, coef, a, s):
    """(v_g, sum of the absolute values of its terms) from what the device left in m and coef."""
    _, c = (ns.double() / cnt.double().view(1, -1, 1, 1)).unbind(0)
    x = lat.double()
    S, K = coef[:, 0].double().view(-1, 1, 1), coef[:, 1].double().view(-1, 1, 1)
    k = (G - 1.0) / s
    v = c - k * (S * m.double() - K * (a * x - s * c))
    vabs = c.abs() + k * ((S * m.double()).abs() + K.abs() * (a * x.abs() + s * c.abs()))
    return v, vabs


def _ddim64(lat, v, vabs, a_t, a_p, eta, z):
    x = lat.double()
    std = eta * math.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p)) if eta else 0.0
    sa, sb, sap, sdir = math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_p), math.sqrt(max(1 - a_p - std * std, 0.0))
    x0, ep = sa * x - sb * v, sa * v + sb * x
    out = sap * x0 + sdir * ep
    scale = sap * (sa * x.abs() + sb * vabs) + sdir * (sa * vabs + sb * x.abs())
    if eta:
        out, scale = out + std * z.double(), scale + (std * z.double()).abs()
    return out, scale


def _dpm64(lat, v, vabs, hist, z, co):
    a_s, s_s, c_x, c_m0, c_m1, c_z = co
    x = lat.double()
    m0 = a_s * x - s_s * v
    out, scale = c_x * x + c_m0 * m0, (c_x * x).abs() + abs(c_m0) * ((a_s * x).abs() + s_s * vabs)
    if c_m1:
        out, scale = out + c_m1 * hist.double(), scale + (c_m1 * hist.double()).abs()
    if c_z:
        out, scale = out + c_z * z.double(), scale + (c_z * z.double()).abs()
    return out, m0, scale + (a_s * x).abs() + s_s * vabs


STEP_CASES = [(4, 16, 16), (3, 13, 11), (32, 13, 11), (1, 1, 1)]


@pytest.mark.parametrize("ftot,h,w", STEP_CASES)
@pytest.mark.parametrize("kind", ["ddim", "ddim-eta", "2m", "2m-sde"])
def test_apg_step_matches_float64(ftot, h, w, kind):
    hw = h * w
    g = torch.Generator().manual_seed(ftot * 31 + hw)
    ns, cnt, lat, mprev = _data(ftot, h, w, seed=ftot + hw)
    z = torch.randn((ftot, hw, 4), generator=g).half()
    nd, cd, ld, md = ns.to(DEV), cnt.to(DEV), lat.to(DEV), mprev.to(DEV)
    if kind.startswith("ddim"):
        eta = 0.6 if kind == "ddim-eta" else 0.0
        d = M.DDIMScheduler(**SCHED_KWARGS)
        d.set_timesteps(10)
        a_t, a_p = d.step_coefficients(int(d.timesteps[3]))
        a, s = math.sqrt(a_t), math.sqrt(1.0 - a_t)
    else:
        sch = _sched(algorithm_type="sde-dpmsolver++" if kind == "2m-sde" else "dpmsolver++")
        sch.set_timesteps(10)
        co = sch.multistep_coefficients(4)
        assert co[4] != 0.0 and (co[5] != 0.0) == (kind == "2m-sde")
        a, s = co[0], co[1]
    norms = _ref64(ns, cnt, lat, mprev, a, s, -0.5, 0.0, 0.0)["N2"].flatten().sqrt()
    r = float(norms.median()) * (0.5 if ftot == 1 else 1.0)
    coef = _prepare(nd, cd, ld, md, a, s, -0.5, 0.0, r)
    torch.cuda.synchronize()
    ch, mh = coef.cpu(), md.cpu()
    assert (ch[:, 0] < 1).any()                                            # the cap is at work
    v, vabs = _vg64(ns, cnt, lat, mh, ch, a, s)
    if kind.startswith("ddim"):
        want, scale = _ddim64(lat, v, vabs, a_t, a_p, eta, z)
        ops.cfg_ddim_step_apg(ld, nd, cd, md, coef, ftot, hw, G, a_t, a_p, eta=eta, variance_noise=z.to(DEV) if eta else None)
        torch.cuda.synchronize()
    else:
        hist = torch.randn((ftot, hw, 4), generator=g)
        want, m0, scale = _dpm64(lat, v, vabs, hist, z, co)
        hd = hist.to(DEV)
        ops.cfg_multistep_step_apg(ld, nd, cd, hd, md, coef, ftot, hw, G, *co, variance_noise=z.to(DEV) if co[5] else None)
        torch.cuda.synchronize()
        assert float((hd.cpu().double() - m0).abs().max()) <= 1e-6 * float(m0.abs().max())
    got = ld.cpu().double()
    assert torch.isfinite(got).all()
    excess = ((got - want).abs() - (U16 * want.abs() + 2e-6 * scale + 2.0 ** -24)).max()
    print(f"\nAPG_STEP {kind} ({ftot},{h},{w}): max |got - want| {float((got - want).abs().max()):.3e}, worst excess over the bound {float(excess):.3e}")
    assert ((got - want).abs() <= U16 * want.abs() + 2e-6 * scale + 2.0 ** -24).all(), float((got - want).abs().max())
    assert torch.equal(md.cpu(), mh) and torch.equal(coef.cpu(), ch)       # the steps only read them


def test_eta_1_no_cap_no_momentum_is_the_plain_step():
    """With eta = 1, r = 0, beta = 0 the APG step is u + g (c - u) up to rounding: within the step bound of the plain kernel's result."""
    ftot, h, w = 5, 7, 9
    hw = h * w
    ns, cnt, lat, _ = _data(ftot, h, w, seed=77)
    nd, cd = ns.to(DEV), cnt.to(DEV)
    a_t, a_p = 0.3, 0.5
    a, s = math.sqrt(a_t), math.sqrt(1 - a_t)
    mbuf = torch.full((ftot, hw, 4), float("nan"), device=DEV)
    la, lb = lat.to(DEV), lat.to(DEV)
    coef = _prepare(nd, cd, la, mbuf, a, s, 0.0, 1.0, 0.0)
    ops.cfg_ddim_step_apg(la, nd, cd, mbuf, coef, ftot, hw, G, a_t, a_p)
    ops.cfg_ddim_step(lb, nd, cd, ftot, hw, G, a_t, a_p)
    torch.cuda.synchronize()
    assert (coef.cpu() == torch.tensor([1.0, 0.0])).all()
    u, c = (ns.double() / cnt.double().view(1, -1, 1, 1)).unbind(0)
    vabs = u.abs() + G * (c.abs() + u.abs())
    want, scale = _ddim64(lat, u + G * (c - u), vabs, a_t, a_p, 0.0, None)
    for got in (la.cpu().double(), lb.cpu().double()):
        assert ((got - want).abs() <= U16 * want.abs() + 2e-6 * scale + 2.0 ** -24).all()


# ---- 3. determinism and refusals
def test_prepare_and_steps_are_deterministic():
    ftot, h, w = 48, 128, 128
    hw = h * w
    ns, cnt, lat, mprev = _data(ftot, h, w, seed=5)
    nd, cd, l0, m0 = ns.to(DEV), cnt.to(DEV), lat.to(DEV), mprev.to(DEV)
    outs = []
    for _ in range(2):
        mbuf, la, lb = m0.clone(), l0.clone(), l0.clone()                  # restored buffers
        coef = _prepare(nd, cd, la, mbuf, 0.6, 0.8, -0.5, 0.0, 40.0)
        ops.cfg_ddim_step_apg(la, nd, cd, mbuf, coef, ftot, hw, G, 0.36, 0.5)
        hist = torch.zeros((ftot, hw, 4), device=DEV)
        ops.cfg_multistep_step_apg(lb, nd, cd, hist, mbuf, coef, ftot, hw, G, 0.6, 0.8, 0.9, 0.4, 0.0, 0.0)
        torch.cuda.synchronize()
        outs.append((coef.cpu(), mbuf.cpu(), la.cpu(), lb.cpu(), hist.cpu()))
    for p, q in zip(*outs):
        assert torch.equal(p, q)
    assert (outs[0][0][:, 0] < 1).any() and (outs[0][0][:, 0] == 1).any() and not torch.equal(outs[0][2], lat)


def test_bad_arguments_raise_and_leave_the_latents_alone():
    ftot, hw = 2, 8
    ns, cnt = torch.randn((2, ftot, hw, 4), device=DEV), torch.ones(ftot, device=DEV)
    lat = torch.randn((ftot, hw, 4), generator=torch.Generator().manual_seed(3)).half().to(DEV)
    keep = lat.clone()
    hist, mom, z = torch.zeros((ftot, hw, 4), device=DEV), torch.zeros((ftot, hw, 4), device=DEV), torch.zeros_like(lat)
    mom_keep = mom.clone()
    coef = torch.zeros((ftot + 1, 2), device=DEV)
    need = _lib.load().md_cfg_apg_workspace_bytes(ftot, hw)
    ws = torch.zeros(1024, device=DEV, dtype=torch.float64)
    assert 0 < need <= 384 * ftot and _lib.load().md_cfg_apg_workspace_bytes(0, hw) == 0
    nan, inf = float("nan"), float("inf")
    L, N, C, Mo, Co, Hi, Z = (t.data_ptr() for t in (lat, ns, cnt, mom, coef, hist, z))
    prepare = lambda l=L, n=N, c=C, m=Mo, halves=2, a=0.6, s=0.8, beta=-0.5, eta=0.0, r=1.0, w=ws.data_ptr(), wsb=ws.numel() * 8, co=Co: _lib.call(
        "md_cfg_apg_prepare", l, n, c, m, ftot, hw, halves, a, s, beta, eta, r, w, wsb, co, ops._st())
    ddim = lambda l=L, n=N, c=C, zp=0, m=Mo, co=Co, halves=2, g=G, a_t=0.3, a_p=0.5, eta=0.0: _lib.call(
        "md_cfg_ddim_step_apg", l, n, c, zp, m, co, ftot, hw, halves, g, a_t, a_p, eta, ops._st())
    multi = lambda l=L, n=N, c=C, h=Hi, zp=0, m=Mo, co=Co, halves=2, g=G, a=0.6, s=0.8, c_x=1.0, c_m0=1.0, c_m1=0.0, c_z=0.0: _lib.call(
        "md_cfg_multistep_step_apg", l, n, c, h, zp, m, co, ftot, hw, halves, g, a, s, c_x, c_m0, c_m1, c_z, ops._st())
    shared = (dict(l=0), dict(n=0), dict(c=0), dict(m=0), dict(co=0), dict(halves=1), dict(halves=3), dict(l=L + 2), dict(n=N + 4), dict(m=Mo + 4),
              dict(co=Co + 2))
    table = ((prepare, shared + (dict(beta=1.0), dict(beta=-1.0), dict(beta=nan), dict(eta=-0.1), dict(eta=1.5), dict(eta=nan), dict(r=-1.0),
                                 dict(r=inf), dict(r=nan), dict(a=nan), dict(s=inf), dict(w=0), dict(wsb=need - 8), dict(w=ws.data_ptr() + 4))),
             (ddim, shared + (dict(g=inf), dict(g=nan), dict(a_t=nan), dict(a_p=nan), dict(a_t=1.0), dict(eta=nan), dict(eta=-0.5),
                              dict(eta=0.5, zp=0), dict(eta=0.5, zp=Z + 2))),
             (multi, shared + (dict(h=0), dict(h=Hi + 4), dict(g=nan), dict(a=nan), dict(s=0.0), dict(c_x=inf), dict(c_m1=nan), dict(c_z=0.5, zp=0))))
    for call, cases in table:
        for kw in cases:
            with pytest.raises(_lib.MdanceHipError):
                call(**kw)
            torch.cuda.synchronize()
            assert torch.equal(lat, keep) and torch.equal(mom, mom_keep), kw      # nothing was launched
    prepare()                                                              # the valid calls
    ddim(eta=0.5, zp=Z)
    multi(c_z=0.5, zp=Z)
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all() and not torch.equal(lat, keep) and not torch.equal(mom, mom_keep)
    assert not coef[ftot].any()                                            # coef is written for ftot frames only


# ---- 4. the loop
@pytest.fixture(scope="module")
def small():
    return build_models()


def _loop(sch, models, inputs, steps, guidance=3.5, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, guidance, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _restated(models, inputs, steps, scheduler=None, **kw):
    _, _, ref_sd, den_sd = models
    with torch.no_grad():
        return A.denoise_loop(ref_sd, den_sd, *inputs, steps, guidance_scale=3.5, reduced=True, scheduler=scheduler, **kw)


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_apg_off_is_bitwise_the_plain_loop(small, monkeypatch, sampler):
    inputs = synth_inputs(4, 16, 16, ctx_len=5, ctx_dim=64, seed=91)
    mk = lambda: M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _sched()
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    a = _loop(mk(), small, inputs, 4, guidance=G, apg=False, apg_eta=0.3, apg_norm_threshold=2.0, apg_momentum=-0.5)
    seen_a = [n for n in names if n.startswith("md_cfg")]
    del names[:]
    b = _loop(mk(), small, inputs, 4, guidance=G)
    assert torch.equal(a, b)
    assert seen_a == [n for n in names if n.startswith("md_cfg")] == ["md_cfg_ddim_step" if sampler == "ddim" else "md_cfg_multistep_step"] * 4
    del names[:]
    c = _loop(mk(), small, inputs, 4, guidance=G, apg=True, apg_eta=0.0)
    assert [n for n in names if n.startswith("md_cfg")] == ["md_cfg_apg_prepare", "md_cfg_ddim_step_apg" if sampler == "ddim"
                                                            else "md_cfg_multistep_step_apg"] * 4
    d = rel_l2(c, b)
    print(f"\nAPG_EFFECT {sampler} guidance {G} rel_l2(apg eta 0, plain) {d:.3e}")
    assert d > 1e-2, d                                                     # the keyword is not silently ignored


@pytest.mark.parametrize("frames,win", [(4, {}), (12, WRAP12)], ids=["f4", "f12-wrap"])
def test_loop_vs_restatement_reduced_width(small, frames, win):
    inputs = tuple(t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=400 + frames))
    plain = _restated(small, inputs, 8, **win)
    ddim_err = rel_l2(_loop(M.DDIMScheduler(**SCHED_KWARGS), small, inputs, 8, **win), plain)
    # eta = 1, no cap, no momentum: plain guidance up to rounding -- the plain bounds against the PLAIN loop's restatement
    same = _loop(M.DDIMScheduler(**SCHED_KWARGS), small, inputs, 8, apg=True, apg_eta=1.0, **win)
    r1, c1 = rel_l2(same, plain), cosine(same, plain)
    print(f"\nAPG_LOOP f={frames} ddim eta 1 r 0 beta 0 vs the plain restatement rel_l2 {r1:.3e} cos {c1:.7f} (plain DDIM loop {ddim_err:.3e}, "
          f"ratio {r1 / ddim_err:.2f})")
    assert r1 <= 3e-2 and c1 >= 0.999, (r1, c1)
    # a threshold that caps some (step, frame) pairs and not others: the median norm of the uncapped restated run
    norms = []
    _restated(small, inputs, 8, apg_on=True, apg_momentum=-0.5, on_apg=lambda t, res: norms.append(res["N2"].flatten().sqrt()), **win)
    r = float(torch.cat(norms).median())
    for name, mk, rs in (("ddim", lambda: M.DDIMScheduler(**SCHED_KWARGS), lambda: None), ("2m", _sched, lambda: R.Restated(2, "dpmsolver++", "midpoint"))):
        out = _loop(mk(), small, inputs, 8, apg=True, apg_eta=0.0, apg_norm_threshold=r, apg_momentum=-0.5, **win)
        caps = []
        want = _restated(small, inputs, 8, scheduler=rs(), apg_on=True, apg_eta=0.0, apg_norm_threshold=r, apg_momentum=-0.5,
                         on_apg=lambda t, res: caps.append(res["S"].flatten()), **win)
        caps = torch.cat(caps)
        assert (caps < 1).any() and (caps == 1).any(), caps
        e, c = rel_l2(out, want), cosine(out, want)
        print(f"\nAPG_LOOP f={frames} {name} eta 0 r {r:.3f} beta -0.5 8 steps rel_l2 {e:.3e} cos {c:.7f} (plain DDIM loop, same clip {ddim_err:.3e}, "
              f"ratio {e / ddim_err:.2f}; capped {int((caps < 1).sum())} of {caps.numel()} frame-steps)")
        assert e <= 3e-2 and c >= 0.999, (e, c, ddim_err)


def test_script_apg(tmp_path, golden_dir):
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir)
    out = inference_video.main(["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "3", "--seed", "7", "--apg", "--apg_eta", "0",
                                "--apg_momentum", "-0.5", "--output_dir", str(tmp_path / "output")])
    frames = U.read_frames(out)
    a = np.asarray(frames[0], dtype=np.float32)
    assert len(frames) == F_ and np.isfinite(a).all() and a[:, 2 * (W + 2):].std() > 0
