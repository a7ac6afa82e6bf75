"""GPU: perturbed-attention guidance on the MI355X -- the two *_pag step entries against float64 on their own inputs (every sampler form,
halves 1 and 2, odd sizes), bitwise equality with the plain entries at pag_scale = 0, determinism, the argument checks, one TransformerBlock
in read mode (perturbed and selected / perturbed and unselected), the whole loop against tests/pag_ref.py at reduced width, and the drop-in
script with --pag_scale.  Plain bounds: the step error model of tests/test_apg_gpu.py section 2, the operator bound of tests/test_blocks_gpu.py,
the loop bound rel-L2 <= 3e-2 and cosine >= 0.999.  profiles/pag_tests.log holds every printed figure of a run on an MI355X."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, blocks, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs, synth_state_dict  # noqa: E402

import dpmpp_ref as R  # noqa: E402
import pag_ref as P  # noqa: E402
from test_apg_gpu import U16, _ddim64, _dpm64  # noqa: E402  (the float64 updates with their magnitude sums)

DEV = torch.device("cuda:0")
WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)
G = 3.5


def _sched(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


# ---- 1. the two step entries against float64 on their own inputs
def _data(ftot, h, w, halves, seed):
    """(noise_sum (halves, ftot, hw, 4), perturbed_sum, counter 1..3, latents, z, history) on the host; the planes are counter * a prediction."""
    g = torch.Generator().manual_seed(seed)
    hw = h * w
    cnt = torch.randint(1, 4, (ftot,), generator=g).float()
    planes = torch.randn((halves + 1, ftot, hw, 4), generator=g) * torch.tensor([0.7, 1.3, 1.1][3 - (halves + 1):]).view(-1, 1, 1, 1)
    planes = planes * cnt.view(1, -1, 1, 1)
    lat = torch.randn((ftot, hw, 4), generator=g).half()
    z = torch.randn((ftot, hw, 4), generator=g).half()
    hist = torch.randn((ftot, hw, 4), generator=g)
    return planes[:halves].contiguous(), planes[halves].contiguous(), cnt, lat, z, hist


def _v64(ns, pp, cnt, halves, s):
    """(v, sum of the absolute values of its terms): guided_v plus the PAG term, inv = 1 / counter under CFG and 1 without."""
    ns, pp = ns.double(), pp.double()
    inv = 1.0 / cnt.double().view(-1, 1, 1) if halves == 2 else 1.0
    if halves == 2:
        u, c = ns[0] * inv, ns[1] * inv
        v, vabs = u + G * (c - u), u.abs() + G * (c.abs() + u.abs())
    else:
        v, vabs = ns[0], ns[0].abs()
    return v + s * inv * (ns[halves - 1] - pp), vabs + s * inv * (ns[halves - 1].abs() + pp.abs())


def _coefficients(kind):
    if kind.startswith("ddim"):
        d = M.DDIMScheduler(**SCHED_KWARGS)
        d.set_timesteps(10)
        return tuple(d.step_coefficients(int(d.timesteps[3]))) + (0.6 if kind == "ddim-eta" else 0.0,)
    sch = _sched(algorithm_type="sde-dpmsolver++" if kind.endswith("sde") else "dpmsolver++")
    sch.set_timesteps(10)
    co = sch.multistep_coefficients(1 if kind.startswith("1st") else 4)
    assert (co[4] != 0.0) == kind.startswith("2m") and (co[5] != 0.0) == kind.endswith("sde"), (kind, co)
    return co


def _run(kind, co, lat, ns, pp, cnt, z, hist, halves, s, pag=True):
    """One step on the device -> (latents, history or None) on the host."""
    ftot, hw = lat.shape[0], lat.shape[1]
    ld, nd, pd, cd, zd = lat.to(DEV), ns.to(DEV), pp.to(DEV), cnt.to(DEV), z.to(DEV)
    hd = None
    if kind.startswith("ddim"):
        a_t, a_p, eta = co
        if pag:
            ops.cfg_ddim_step_pag(ld, nd, cd, pd, ftot, hw, G, s, a_t, a_p, halves=halves, eta=eta, variance_noise=zd if eta else None)
        else:
            ops.cfg_ddim_step(ld, nd, cd, ftot, hw, G, a_t, a_p, halves=halves, eta=eta, variance_noise=zd if eta else None)
    else:
        # first order never reads the history: it may hold NaN
        hd = hist.to(DEV) if co[4] != 0.0 else torch.full(hist.shape, float("nan"), device=DEV)
        if pag:
            ops.cfg_multistep_step_pag(ld, nd, cd, hd, pd, ftot, hw, G, s, *co, halves=halves, variance_noise=zd if co[5] else None)
        else:
            ops.cfg_multistep_step(ld, nd, cd, hd, ftot, hw, G, *co, halves=halves, variance_noise=zd if co[5] else None)
    torch.cuda.synchronize()
    return ld.cpu(), None if hd is None else hd.cpu()


STEP_CASES = [(1, 1, 1), (3, 13, 11), (5, 7, 9), (16, 16, 16)]
KINDS = ["ddim", "ddim-eta", "1st", "2m", "1st-sde", "2m-sde"]


@pytest.mark.parametrize("ftot,h,w", STEP_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_pag_step_matches_float64(ftot, h, w, kind):
    co = _coefficients(kind)
    for halves in (1, 2):
        ns, pp, cnt, lat, z, hist = _data(ftot, h, w, halves, seed=ftot * 31 + h * w + halves)
        for s in (0.5, 3.0):
            v, vabs = _v64(ns, pp, cnt, halves, s)
            if kind.startswith("ddim"):
                want, scale = _ddim64(lat, v, vabs, co[0], co[1], co[2], z)
            else:
                want, m0, scale = _dpm64(lat, v, vabs, hist, z, co)
            got, h_got = _run(kind, co, lat, ns, pp, cnt, z, hist, halves, s)
            got = got.double()
            assert torch.isfinite(got).all()
            if h_got is not None:
                assert float((h_got.double() - m0).abs().max()) <= 2e-6 * float(((co[0] * lat.double()).abs() + co[1] * vabs).max())
            bound = U16 * want.abs() + 2e-6 * scale + 2.0 ** -24
            excess = ((got - want).abs() - bound).max()
            print(f"\nPAG_STEP {kind} ({ftot},{h},{w}) halves {halves} s {s}: max |got - want| {float((got - want).abs().max()):.3e}, "
                  f"worst excess over the bound {float(excess):.3e}")
            assert ((got - want).abs() <= bound).all(), float((got - want).abs().max())
            # the term is really there: the plain step on the same planes differs
            plain, _ = _run(kind, co, lat, ns, pp, cnt, z, hist, halves, s, pag=False)
            assert ftot * h * w == 1 or not torch.equal(plain, got.half())


@pytest.mark.parametrize("kind", KINDS)
def test_scale_zero_is_the_plain_entry_bitwise_and_runs_repeat(kind):
    co = _coefficients(kind)
    for halves in (1, 2):
        for ftot, h, w in ((3, 13, 11), (16, 16, 16)):
            ns, pp, cnt, lat, z, hist = _data(ftot, h, w, halves, seed=7 + halves)
            a = _run(kind, co, lat, ns, pp, cnt, z, hist, halves, 0.0)
            b = _run(kind, co, lat, ns, pp, cnt, z, hist, halves, 0.0, pag=False)
            assert torch.equal(a[0], b[0]) and (a[1] is None or torch.equal(a[1], b[1]))
            c, d = (_run(kind, co, lat, ns, pp, cnt, z, hist, halves, 3.0) for _ in range(2))
            assert torch.equal(c[0], d[0]) and (c[1] is None or torch.equal(c[1], d[1])) and not torch.equal(c[0], a[0])


def test_bad_arguments_raise_and_leave_the_latents_alone():
    ftot, hw = 2, 8
    ns, cnt = torch.randn((3, ftot, hw, 4), device=DEV), torch.ones(ftot, device=DEV)
    lat = torch.randn((ftot, hw, 4), generator=torch.Generator().manual_seed(3)).half().to(DEV)
    keep = lat.clone()
    hist, z = torch.zeros((ftot, hw, 4), device=DEV), torch.zeros_like(lat)
    nan, inf = float("nan"), float("inf")
    L, N, C, Hi, Z = (t.data_ptr() for t in (lat, ns, cnt, hist, z))
    Pp = ns[2].data_ptr()
    ddim = lambda l=L, n=N, c=C, zp=0, p=Pp, halves=2, g=G, s=3.0, a_t=0.3, a_p=0.5, eta=0.0: _lib.call(
        "md_cfg_ddim_step_pag", l, n, c, zp, p, ftot, hw, halves, g, s, a_t, a_p, eta, ops._st())
    multi = lambda l=L, n=N, c=C, h=Hi, zp=0, p=Pp, halves=2, g=G, s=3.0, a=0.6, sg=0.8, c_x=1.0, c_m0=1.0, c_m1=0.0, c_z=0.0: _lib.call(
        "md_cfg_multistep_step_pag", l, n, c, h, zp, p, ftot, hw, halves, g, s, a, sg, c_x, c_m0, c_m1, c_z, ops._st())
    shared = (dict(l=0), dict(n=0), dict(c=0), dict(p=0), dict(halves=3), dict(halves=0), dict(s=nan), dict(s=inf), dict(s=-inf), dict(s=-1.0),
              dict(g=nan))
    # misalignment: the DDIM entry accesses single elements (2-byte latents / noise, 4-byte planes), the multistep entry one pixel at a time
    table = ((ddim, shared + (dict(a_t=nan), dict(a_p=inf), dict(eta=nan), dict(eta=-0.5), dict(eta=0.5, zp=0), dict(l=L + 1), dict(n=N + 2),
                              dict(p=Pp + 2), dict(c=C + 2), dict(eta=0.5, zp=Z + 1))),
             (multi, shared + (dict(h=0), dict(h=Hi + 4), dict(a=nan), dict(c_x=inf), dict(c_m1=nan), dict(c_z=0.5, zp=0), dict(c_z=0.5, zp=Z + 2),
                               dict(l=L + 2), dict(n=N + 4), dict(p=Pp + 4))))
    for call, cases in table:
        for kw in cases:
            with pytest.raises(_lib.MdanceHipError):
                call(**kw)
            torch.cuda.synchronize()
            assert torch.equal(lat, keep), kw                              # nothing was launched
    ddim(halves=1, c=0)                                                    # the valid calls; without CFG the counter is never read
    multi(c_z=0.5, zp=Z)
    torch.cuda.synchronize()
    assert torch.isfinite(lat).all() and not torch.equal(lat, keep)


# ---- 2. one TransformerBlock in read mode
def _close(got, ref, what):
    """The operator bound of tests/test_blocks_gpu.py."""
    got, ref = got.float().cpu(), ref.float()
    err, bound = (got - ref).abs().max().item(), 1e-2 * ref.abs().max().item() + 1e-3
    print(f"\nPAG_BLOCK {what}: max err {err:.4g} (bound {bound:.4g})")
    assert got.shape == ref.shape and err <= bound, f"{what}: max err {err:.4g} > {bound:.4g}"


def test_transformer_block_perturbed_rows():
    dim, L, f, lk, dctx = 320, 64, 2, 5, 64
    blk = blocks.TransformerBlock(dim, dctx)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items()}, seed=21)
    blk.load_state_dict(sd, strict=True)
    blk = blk.half().to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn((f, L, dim), generator=g).half()                       # the conditional frames' tokens
    bank = (torch.randn((f, L, dim), generator=g) * 0.5).half()
    ctx = torch.randn((1, lk, dctx), generator=g).half()
    lpad = 8
    buf = torch.zeros((2, lpad, dctx), dtype=torch.float16)
    buf[1, :lk] = ctx[0]
    cross = blocks.CrossContext(buf.view(2 * lpad, dctx).to(DEV), torch.tensor([0, 0, 1, 1], dtype=torch.int32, device=DEV), lk, lpad, zero_frames=f)
    blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [bank.to(DEV)]
    sdf = {k: v.half().float() for k, v in sd.items()}
    with torch.no_grad():
        h_cond = x.reshape(f * L, dim).to(DEV)
        # perturbed and selected: the identity attention map, against the restated block
        got = blk(h_cond.clone(), f, L, cross.rows(f, 2 * f), sa=blocks.SelfAttnCall(identity=(blk,)))
        want = P._read_identity(sdf, "", x.float(), ctx.float().repeat(f, 1, 1), bank.float())
        _close(got.view(f, L, dim), want, "perturbed, selected vs pag_ref")
        plain = P.O.transformer_block_read(sdf, "", x.float(), ctx.float().repeat(f, 1, 1), bank.float(), cfg=False)
        assert float((plain - want).abs().max()) > 10 * (1e-2 * float(want.abs().max()) + 1e-3)      # the perturbation is far above the bound
        # perturbed and unselected: the conditional half of a normal CFG call on the same rows, BITWISE.  Every operator of the block works
        # row by row (LayerNorm, the GEMMs' fp32 sums over K in a fixed order per tile flavour) or frame by frame (attention), so a row's bits
        # depend on the kernel flavour alone, not on how many rows the launch has; at these sizes (128 rows in the perturbed call, 256 in the
        # CFG call, K = 320, L = 64) the pinned dispatch gives both calls the same flavours.  A wrong bank row or a wrong first bank row on
        # the perturbed path changes the bits.  (At sizes where the smaller call gets another tile flavour the two agree to fp16 rounding only.)
        un = blk(h_cond.clone(), f, L, cross.rows(f, 2 * f), sa=blocks.SelfAttnCall(identity=()))
        both = blk(torch.cat([h_cond, h_cond]).contiguous(), 2 * f, L, cross)
        torch.cuda.synchronize()
        print(f"\nPAG_BLOCK unselected vs the CFG call's conditional half: max |difference| {float((un.float() - both[f * L:].float()).abs().max()):.3g}")
        assert torch.equal(un, both[f * L:])
        assert not torch.equal(un, both[:f * L])                           # ... and it is not the unconditional half, which ignores the bank
        _close(un.view(f, L, dim), plain, "perturbed, unselected vs the oracle's conditional read")
    blk.bank = []


# ---- 3. the loop
@pytest.fixture(scope="module")
def small():
    return build_models()


def _loop(sch, models, inputs, steps, guidance=G, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, guidance, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_scale_zero_is_bitwise_the_plain_loop(small, monkeypatch, sampler):
    inputs = synth_inputs(4, 16, 16, ctx_len=5, ctx_dim=64, seed=91)
    mk = lambda: M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _sched()
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    a = _loop(mk(), small, inputs, 4, pag_scale=0.0, pag_adaptive_scale=0.01, pag_applied_layers=("up_blocks.1",))
    seen_a = list(names)
    del names[:]
    b = _loop(mk(), small, inputs, 4)
    step = "md_cfg_ddim_step" if sampler == "ddim" else "md_cfg_multistep_step"
    assert torch.equal(a, b) and seen_a == names and [n for n in names if n.startswith("md_cfg")] == [step] * 4      # launch for launch
    del names[:]
    c = _loop(mk(), small, inputs, 4, pag_scale=3.0, pag_applied_layers=("up_blocks.1",))
    assert [n for n in names if n.startswith("md_cfg")] == [step + "_pag"] * 4
    d = rel_l2(c, b)
    print(f"\nPAG_EFFECT {sampler} rel_l2(pag_scale 3 on up_blocks.1, plain) {d:.3e}")
    assert d > 3e-2, d                                                     # the keywords are not silently ignored


LOOPS = {"a-f4-cfg-mid": dict(frames=4, kw=dict(pag_scale=3.0, pag_applied_layers=("mid",))),
         "b-f12-wrap-pyramid-2m": dict(frames=12, win=WRAP12, fuse="pyramid", sampler="2m", kw=dict(pag_scale=3.0, pag_applied_layers=("mid",))),
         "c-f4-no-cfg": dict(frames=4, guidance=1.0, kw=dict(pag_scale=3.0, pag_applied_layers=("mid",))),
         "d-f4-adaptive": dict(frames=4, adaptive=True, kw=dict(pag_scale=3.0, pag_applied_layers=("mid",)))}


@pytest.mark.parametrize("case", list(LOOPS))
def test_loop_vs_restatement_reduced_width(small, case):
    cfg = LOOPS[case]
    steps, g, win, fuse = 4, cfg.get("guidance", G), cfg.get("win", {}), cfg.get("fuse", "flat")
    lat, rl, emb = (t.half().float() for t in synth_inputs(cfg["frames"], 16, 16, ctx_len=5, ctx_dim=64, seed=500 + cfg["frames"]))
    if g <= 1.0:
        emb = emb[1:]
    two_m = cfg.get("sampler") == "2m"
    mk = (lambda: _sched()) if two_m else (lambda: M.DDIMScheduler(**SCHED_KWARGS))
    mk_rs = lambda: R.Restated(2, "dpmsolver++", "midpoint") if two_m else None
    kw = dict(cfg["kw"])
    if cfg.get("adaptive"):
        sch = mk()
        sch.set_timesteps(steps)
        ts = [int(t) for t in sch.timesteps]
        kw["pag_adaptive_scale"] = 3.0 / (1000 - ts[2])                    # s_t = 0 at the last two steps
        assert [P.pag_scale_at(3.0, kw["pag_adaptive_scale"], t) > 0 for t in ts] == [True, True, False, False]
    _, _, ref_sd, den_sd = small
    rkw = dict(guidance_scale=g, fuse=fuse, pag_layers=kw["pag_applied_layers"], **win)
    with torch.no_grad():
        want = P.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, scheduler=mk_rs(), pag_scale=3.0,
                              pag_adaptive_scale=kw.get("pag_adaptive_scale", 0.0), **rkw)
        plain_want = P.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, scheduler=mk_rs(), pag_scale=0.0, **rkw)
    out = _loop(mk(), small, (lat, rl, emb), steps, guidance=g, context_fuse=fuse, **win, **kw)
    plain = _loop(mk(), small, (lat, rl, emb), steps, guidance=g, context_fuse=fuse, **win)
    e, c, e0, d = rel_l2(out, want), cosine(out, want), rel_l2(plain, plain_want), rel_l2(plain_want, want)
    print(f"\nPAG_LOOP {case} {steps} steps rel_l2 {e:.3e} cos {c:.7f} (plain loop, same clip {e0:.3e}, ratio {e / e0:.2f}; "
          f"restated pag_scale 0 vs 3: {d:.3e})")
    assert torch.isfinite(out).all() and e <= 3e-2 and c >= 0.999, (e, c, e0)


def test_script_pag(tmp_path, golden_dir):
    """The drop-in script end to end, with and without --pag_scale 3 --pag_layers mid.  The tree is dpm_script_tree.make_tree, the synthetic
    weight tree of the other GPU script tests, not loop_helpers.script_tree: that one holds configs and media only and goes with a stand-in
    pipeline that has no UNets, so nothing would run.  128 x 128 pixels: a 16 x 16 latent gives the mid block 2 x 2 tokens per frame; at the
    64 x 64 of the other script tests it sees one token, where the identity IS the softmax and the two runs would be equal."""
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir, width=128, height=128)      # a 16 x 16 latent: the mid block sees 2 x 2 tokens
    base = ["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "3", "--seed", "7"]
    on = U.read_frames(inference_video.main(base + ["--pag_scale", "3", "--pag_layers", "mid", "--output_dir", str(tmp_path / "on")]))
    off = U.read_frames(inference_video.main(base + ["--output_dir", str(tmp_path / "off")]))
    a, b = (np.stack([np.asarray(fr, dtype=np.float32) for fr in frames]) for frames in (on, off))
    assert len(on) == len(off) == F_ and np.isfinite(a).all() and a[:, :, 2 * (W + 2):].std() > 0
    print(f"\nPAG_SCRIPT mean |on - off| over the generated panel {float(np.abs(a - b)[:, :, 2 * (W + 2):].mean()):.3f} (of 255)")
    assert not np.array_equal(a, b)
