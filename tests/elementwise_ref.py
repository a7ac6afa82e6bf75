"""TEST INFRASTRUCTURE: plain-torch references for the kernels of mikudance_amd/csrc/elementwise.hip, shared by tests/test_elementwise_gpu.py
(the kernels against these) and tests/test_elementwise_ref_cpu.py (these against tests/fake_ops.py, without a GPU).

Layout kernels (md_pack_nhwc_f16, md_unpack_nhwc_f16, md_concat_channels_f16): expected values are EXACT and stated with permute / slicing /
torch.cat on the logical tensors, never with the strides the kernels are given -- tests/fake_ops.py gathers by offset arithmetic, like the
kernels do, so the two statements are independent.  One fp32 -> fp16 rounding where the source is fp32, the bits unchanged where it is fp16.
LAYOUT_FORMS has one row per `ops.pack_nhwc(` / `ops.unpack_nhwc(` call of the package, named after its call site.

Step tail (md_cfg_ddim_step*, md_cfg_multistep_step*): nothing is restated here.  The float64 updates with their magnitude sums are
test_apg_gpu._ddim64 / _dpm64 / _vg64 and test_pag_gpu._v64; the guided v of the plain and the *_scaled entries is _v64 at scale 0, whose
CFG part is word for word the float64 guided-v statement of test_dpmsolver_gpu._restated_update (u + g (c - u), |u| + g (|c| + |u|); the
window SUM without CFG).  The bound is the project's step error model, |got - want| <= U16 |want| + 2e-6 scale + 2^-24."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from test_apg_gpu import G as G_APG, U16, _ddim64, _dpm64, _vg64  # noqa: F401  (the float64 updates with their magnitude sums)
from test_pag_gpu import G as G_PAG, _coefficients, _v64  # noqa: F401

F16, F32 = torch.float16, torch.float32
DTYPES = {"f16": F16, "f32": F32}


# ------------------------------------------------------------------------------------------------ pack / unpack / concat
def nearest_index(n_out, n_in):
    """PyTorch's nearest rule, written out: min(floor(float32(y) * float32(n_in / n_out)), n_in - 1), the scale one fp32 division."""
    scale = np.float32(n_in) / np.float32(n_out)
    return torch.tensor([min(int(math.floor(np.float32(y) * scale)), n_in - 1) for y in range(n_out)], dtype=torch.long)


# layout -> what the source / destination tensor is and which five strides (sB, sF, sC, sY, sX) its call sites hand over
#   NCHW    (B, C, H, W) images, one per n                       (st0, 0, st1, st2, st3), F = 1
#   NCFHW   (b, C, f, H, W) clips, n = b f                       (st0, st2, st1, st3, st4), F = f
#   1CFHW   (1, C, F, H, W) one clip, n = F, batch stride zero   (0, st2, st1, st3, st4), F = F
#   HALVES  (f, H, W, 4) packed latents, n = 2 f: BOTH clip-halves read the same frames (batch stride zero, F = f)
#   NHWC    (B, H, W, C) channel-innermost, a channel slice of a wider tensor (sC = 1), F = 1
def _row(site, op, layout, dtypes, ctot, c_begin, c_count, cpad, resize=None):
    return dict(site=site, op=op, layout=layout, dtypes=dtypes, F={"NCHW": 1, "NHWC": 1}.get(layout, "f"), ctot=ctot, c_begin=c_begin,
                c_count=c_count, cpad=cpad, resize=resize)


BOTH, HALF = ("f16", "f32"), ("f16",)
LAYOUT_FORMS = [
    # ---- pack: cpad is Cpad, ctot the channels of the source
    _row("unet_2d_mix.py:forward/sample", "pack", "NCHW", BOTH, 6, 0, 4, 64),
    _row("unet_2d_mix.py:forward/motion_at", "pack", "NCHW", BOTH, 6, 4, 2, 64, "shrink"),
    _row("vae.py:encode", "pack", "NCHW", BOTH, 3, 0, 3, 64),
    _row("vae.py:decode", "pack", "NCHW", BOTH, 4, 0, 4, 64),
    _row("vae_temporal.py:encode", "pack", "NCHW", BOTH, 3, 0, 3, 64),
    _row("vae_temporal.py:decode", "pack", "NCHW", BOTH, 4, 0, 4, 64),
    _row("unet_3d_mix.py:forward", "pack", "NCFHW", BOTH, 4, 0, 4, 64),
    _row("pipeline_mikudance.py:denoise/latents", "pack", "1CFHW", BOTH, 4, 0, 4, 4),
    _row("pipeline_mikudance.py:denoise/init_latents", "pack", "1CFHW", BOTH, 4, 0, 4, 4),
    _row("pipeline_mikudance.py:denoise/window", "pack", "HALVES", HALF, 4, 0, 4, 64),
    _row("pipeline_mikudance.py:_variance_noise", "pack", "1CFHW", BOTH, 4, 0, 4, 4),
    _row("pipeline_mikudance.py:_write_banks/guide", "pack", "NCHW", BOTH, 22, 0, 20, 64),
    _row("pipeline_mikudance.py:_write_banks/motion_at", "pack", "NCHW", BOTH, 22, 20, 2, 64, "shrink"),
    _row("pipeline_mikudance.py:upscale_latents", "pack", "1CFHW", BOTH, 4, 0, 4, 4),
    _row("blocks.py:Resample", "pack", "NHWC", HALF, 8, 0, 8, 8, "enlarge"),
    # ---- unpack: c_count is C, cpad is ldc (the channel pitch of the NHWC source), dtypes those of the destination
    _row("unet_2d_mix.py:forward", "unpack", "NCHW", BOTH, 8, 0, 8, 8),
    _row("vae.py:encode", "unpack", "NCHW", BOTH, 8, 0, 8, 64),
    _row("vae.py:decode", "unpack", "NCHW", BOTH, 3, 0, 3, 3),
    _row("vae_temporal.py:encode", "unpack", "NCHW", BOTH, 8, 0, 8, 64),
    _row("vae_temporal.py:decode", "unpack", "NCHW", BOTH, 3, 0, 3, 8),
    _row("unet_3d_mix.py:forward", "unpack", "NCFHW", BOTH, 4, 0, 4, 4),
    _row("pipeline_mikudance.py:_latents_out", "unpack", "1CFHW", BOTH, 4, 0, 4, 4),
    _row("pipeline_mikudance.py:upscale_latents", "unpack", "1CFHW", BOTH, 4, 0, 4, 4),
]
PACK_FORMS = [r for r in LAYOUT_FORMS if r["op"] == "pack"]
UNPACK_FORMS = [r for r in LAYOUT_FORMS if r["op"] == "unpack"]

# (Hin, Win, Ho, Wo): shrinking 16 -> 5, 16 -> 3, 9 -> 4, 7 -> 3; enlarging 5 -> 8, 7 -> 12, 3 -> 7; the identity; H and W scaled differently
RESIZE_CASES = [(16, 16, 5, 3), (9, 7, 4, 3), (16, 9, 3, 4), (5, 7, 8, 12), (3, 5, 7, 8), (3, 3, 7, 7), (7, 5, 7, 5), (7, 16, 12, 5), (16, 3, 5, 7)]
ODD = (7, 5)                                                               # H != W, neither a multiple of 8


def strided_tensor(layout, ctot, b, f, h, w, dtype, fill):
    """(whole, view): `view` is the tensor of `layout` a call site would hold, cut out of the larger `whole` (three more columns, or twice the
    channels for NHWC) so that no stride is the product of the sizes inside it.  fill: a generator (normal values) or a number.  HALVES is
    contiguous: its call site writes the strides out from the sizes."""
    shape = {"NCHW": (b, ctot, h, w + 3), "NCFHW": (b, ctot, f, h, w + 3), "1CFHW": (1, ctot, f, h, w + 3), "HALVES": (f, h, w, ctot),
             "NHWC": (b, h, w, 2 * ctot)}[layout]
    whole = torch.randn(shape, generator=fill).to(dtype) if isinstance(fill, torch.Generator) else torch.full(shape, fill, dtype=dtype)
    view = whole if layout == "HALVES" else whole[..., ctot // 2:ctot // 2 + ctot] if layout == "NHWC" else whole[..., 1:1 + w]
    return whole, view


def call_strides(layout, t):
    """(n, F, (sB, sF, sC, sY, sX)) as the call sites of `layout` form them from the tensor they hold."""
    st = t.stride()
    if layout == "NCHW":
        return t.shape[0], 1, (st[0], 0, st[1], st[2], st[3])
    if layout == "NCFHW":
        return t.shape[0] * t.shape[2], t.shape[2], (st[0], st[2], st[1], st[3], st[4])
    if layout == "1CFHW":
        return t.shape[2], t.shape[2], (0, st[2], st[1], st[3], st[4])
    if layout == "HALVES":
        f, h, w, c = t.shape
        return 2 * f, f, (0, h * w * c, 1, w * c, c)
    if layout == "NHWC":
        return t.shape[0], 1, (st[0], 0, 1, st[1], st[2])
    raise KeyError(layout)


def _as_nhwc(layout, t):
    """The logical (n, H, W, C) tensor a call site's tensor stands for."""
    if layout == "NCHW":
        return t.permute(0, 2, 3, 1)
    if layout == "NCFHW":
        b, c, f, h, w = t.shape
        return t.permute(0, 2, 3, 4, 1).reshape(b * f, h, w, c)
    if layout == "1CFHW":
        return t[0].permute(1, 2, 3, 0)
    if layout == "HALVES":
        return torch.cat([t, t])
    if layout == "NHWC":
        return t
    raise KeyError(layout)


def pack_reference(src, layout, c_begin, c_count, cpad, ho, wo):
    """(n, ho, wo, cpad) fp16: channels [c_begin, c_begin + c_count) of `src`, rows and columns by the nearest rule, zero channel padding."""
    x = _as_nhwc(layout, src)
    n, hin, win, _ = x.shape
    x = x[..., c_begin:c_begin + c_count][:, nearest_index(ho, hin)][:, :, nearest_index(wo, win)].to(F16)
    return torch.cat([x, torch.zeros((n, ho, wo, cpad - c_count), dtype=F16)], -1).contiguous()


def unpack_reference(src, dst, layout, c):
    """Writes channels [0, c) of the NHWC fp16 `src` (n, ho, wo, ldc) into `dst`, a tensor of `layout` (a view: its surroundings stay)."""
    x = src[..., :c].to(dst.dtype)
    n, ho, wo, _ = x.shape
    if layout == "NCHW":
        dst.copy_(x.permute(0, 3, 1, 2))
    elif layout == "NCFHW":
        b, f = dst.shape[0], dst.shape[2]
        dst.copy_(x.reshape(b, f, ho, wo, c).permute(0, 4, 1, 2, 3))
    elif layout == "1CFHW":
        dst.copy_(x.permute(3, 0, 1, 2)[None])
    else:
        raise KeyError(layout)
    return dst


def concat_reference(a, b):
    return torch.cat([a, b], dim=-1).contiguous()


def bits(t):
    """fp16 as its 16 bits: equality of these is equality of every bit, -0 and NaN payloads included."""
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ window accumulate
def accumulate_case(f, ftot, hw, halves, seed):
    """(pred fp16 (halves f, hw, 4), noise_sum fp32 (halves, ftot, hw, 4), counter fp32 (ftot,)): a start that is not zero anywhere."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn((halves * f, hw, 4), generator=g).half()
    return pred, torch.randn((halves, ftot, hw, 4), generator=g), torch.randint(1, 4, (ftot,), generator=g).float()


def accumulate_reference(pred, noise_sum, counter, window, f, halves):
    """fp32 s + p on the host, slot by slot: one IEEE addition per element, so the kernel's result is these bits."""
    ns, cnt = noise_sum.clone(), counter.clone()
    p = pred.float().view(halves, f, -1, 4)
    for i, fr in enumerate(window):
        if fr >= 0:
            ns[:, fr] = ns[:, fr] + p[:, i]
            cnt[fr] = cnt[fr] + 1.0
    return ns, cnt


# ------------------------------------------------------------------------------------------------ the step tail
FLAVOURS = ("plain", "scaled", "apg", "pag")
VSCALE = 0.8125                                                            # exact in fp32 (and in fp16)
PAG_S = 3.0
APG_BETA, APG_ETA = -0.5, 0.0
ROUND = 4096 * 256                                                         # threads of one grid round of the step kernels
SMALL_STEP_CASES = [(1, 1, 1), (3, 13, 11), (5, 7, 9), (16, 16, 16)]
KINDS = ["ddim", "ddim-eta", "1st", "2m", "1st-sde", "2m-sde"]
# past one grid round: (kind, Ftot, h, w).  DDIM flavours count ELEMENTS (5 x 229 x 229 x 4 = 1 048 820, 244 past the round), the multistep
# flavours PIXELS (5 x 459 x 457 = 1 048 815, 239 past it); in both the round boundary lies inside frame 4, not on a frame boundary.
LARGE_STEP_CASES = [("ddim-eta", 5, 229, 229), ("2m-sde", 5, 459, 457)]
LARGE_FLAVOURS = [("plain", 2), ("plain", 1), ("scaled", 2), ("apg", 2), ("pag", 2), ("pag", 1)]
BOUNDARY_CASES = [(16, 128, 128), (16, 16385, 1)]                          # total = 4096 x 256 exactly (no second round), and 64 past it


def step_seed(flavour, ftot, hw, halves):
    return 1000 * FLAVOURS.index(flavour) + ftot * 31 + hw % 997 + halves


def guidance(flavour):
    return G_APG if flavour == "apg" else G_PAG                            # the G the imported float64 statements were written with


def step_case(kernel, ftot, hw, halves, seed):
    """The inputs of one step case of flavour `kernel` (plain / scaled / apg / pag), on the host:
    ns (halves, ftot, hw, 4) and pp (ftot, hw, 4) fp32, the planes, counter x a prediction as in test_pag_gpu._data; cnt (ftot,) from {1, 2, 3}
    with NEIGHBOURING frames different and, from three frames on, the last different from the first (a frame index taken modulo the grid round
    lands on frame 0), so that a wrong frame index changes the value; lat, z fp16; hist, mprev (APG's previous momentum) fp32."""
    assert kernel in FLAVOURS
    g = torch.Generator().manual_seed(seed)
    while True:
        steps = torch.randint(1, 3, (ftot,), generator=g)
        cnt = ((torch.cumsum(steps, 0) + int(torch.randint(0, 3, (1,), generator=g))) % 3 + 1).float()
        if ftot < 3 or cnt[0] != cnt[-1]:
            break
    planes = torch.randn((halves + 1, ftot, hw, 4), generator=g) * torch.tensor([0.7, 1.3, 1.1][3 - (halves + 1):]).view(-1, 1, 1, 1)
    planes = planes * cnt.view(1, -1, 1, 1)
    lat = torch.randn((ftot, hw, 4), generator=g).half()
    z = torch.randn((ftot, hw, 4), generator=g).half()
    hist = torch.randn((ftot, hw, 4), generator=g)
    mprev = torch.randn((ftot, hw, 4), generator=g) * 0.5
    return SimpleNamespace(kernel=kernel, ftot=ftot, hw=hw, halves=halves, ns=planes[:halves].contiguous(), pp=planes[halves].contiguous(), cnt=cnt,
                           lat=lat, z=z, hist=hist, mprev=mprev)


def _alpha_sigma(kind, co):
    return (math.sqrt(co[0]), math.sqrt(1.0 - co[0])) if kind.startswith("ddim") else (co[0], co[1])


def apg_threshold(case, a, s):
    """A norm threshold that caps some frames and not others: the median over the frames of |m|, m = s (u - c) + beta m_prev (an input of
    the case, not a reference: whatever it is, the float64 statement uses what the prepare call under test left behind)."""
    u, c = (case.ns.double() / case.cnt.double().view(1, -1, 1, 1)).unbind(0)
    m = s * (u - c) + APG_BETA * case.mprev.double()
    norms = m.pow(2).sum((1, 2)).sqrt()
    return float(norms.median()) * (0.5 if case.ftot == 1 else 1.0)


def run_step(impl, case, kind, co, put=lambda t: t.clone()):
    """One step of flavour case.kernel through `impl` (mikudance_amd.ops on the device, or a namespace of the CPU emulations: the signatures
    are the same) -> (latents, history or None, extra) on the host.  put: host tensor -> a fresh tensor where impl wants it.  Without CFG the
    counter handed over holds NaN: it must not be read.  A first-order history holds NaN, as in test_pag_gpu.  extra: for apg (coef, momentum)
    as impl.cfg_apg_prepare left them, read back after the step (the step only reads them)."""
    fl, ftot, hw, halves = case.kernel, case.ftot, case.hw, case.halves
    g = guidance(fl)
    cnt = case.cnt if halves == 2 else torch.full_like(case.cnt, float("nan"))
    ld, nd, cd = put(case.lat), put(case.ns), put(cnt)
    ddim = kind.startswith("ddim")
    noise = co[2] if ddim else co[5]
    zd = put(case.z) if noise else None
    hd = None
    if not ddim:
        hd = put(case.hist if co[4] != 0.0 else torch.full_like(case.hist, float("nan")))
    extra, kw = None, {}
    if fl == "scaled":
        kw["vscale"] = put(torch.tensor([VSCALE], dtype=F32))
    if fl in ("plain", "scaled"):
        if ddim:
            impl.cfg_ddim_step(ld, nd, cd, ftot, hw, g, co[0], co[1], halves=halves, eta=co[2], variance_noise=zd, **kw)
        else:
            impl.cfg_multistep_step(ld, nd, cd, hd, ftot, hw, g, *co, halves=halves, variance_noise=zd, **kw)
    elif fl == "pag":
        pd = put(case.pp)
        if ddim:
            impl.cfg_ddim_step_pag(ld, nd, cd, pd, ftot, hw, g, PAG_S, co[0], co[1], halves=halves, eta=co[2], variance_noise=zd)
        else:
            impl.cfg_multistep_step_pag(ld, nd, cd, hd, pd, ftot, hw, g, PAG_S, *co, halves=halves, variance_noise=zd)
    else:
        assert halves == 2
        a, s = _alpha_sigma(kind, co)
        md, coef = put(case.mprev), put(torch.zeros((ftot, 2), dtype=F32))
        impl.cfg_apg_prepare(ld, nd, cd, md, coef, ftot, hw, a, s, APG_BETA, APG_ETA, apg_threshold(case, a, s))
        before = (coef.cpu().clone(), md.cpu().clone())
        if ddim:
            impl.cfg_ddim_step_apg(ld, nd, cd, md, coef, ftot, hw, g, co[0], co[1], eta=co[2], variance_noise=zd)
        else:
            impl.cfg_multistep_step_apg(ld, nd, cd, hd, md, coef, ftot, hw, g, *co, variance_noise=zd)
        extra = (coef.cpu(), md.cpu())
        assert torch.equal(extra[0], before[0]) and torch.equal(extra[1], before[1])      # the steps only read them
    return ld.cpu(), None if hd is None else hd.cpu(), extra


def step_want(case, kind, co, extra=None):
    """float64 -> (want, bound, m0 or None, history bound or None): the imported statements on the case's inputs.  bound is the step error model
    per element; the history is held to the bound of test_pag_gpu: max |h - m0| <= 2e-6 max(|alpha_s x| + sigma_s vabs)."""
    fl, halves = case.kernel, case.halves
    if fl == "apg":
        a, s = _alpha_sigma(kind, co)
        v, vabs = _vg64(case.ns, case.cnt, case.lat, extra[1], extra[0], a, s)
    else:
        v, vabs = _v64(case.ns, case.pp, case.cnt, halves, PAG_S if fl == "pag" else 0.0)
        if fl == "scaled":
            v, vabs = v * VSCALE, vabs * VSCALE
    if kind.startswith("ddim"):
        want, scale = _ddim64(case.lat, v, vabs, co[0], co[1], co[2], case.z)
        m0 = hb = None
    else:
        want, m0, scale = _dpm64(case.lat, v, vabs, case.hist, case.z, co)
        hb = 2e-6 * float(((co[0] * case.lat.double()).abs() + co[1] * vabs).max())
    return want, U16 * want.abs() + 2e-6 * scale + 2.0 ** -24, m0, hb


def check_step(tag, case, kind, got, h_got, want, bound, m0, hb, second_round_from=None):
    """Prints the figures, then asserts the bound over all elements, over the elements from `second_round_from` (an element index) on, and the
    history bound.  Returns (max error, worst excess, worst |err| / bound of the second round or None)."""
    got = got.double()
    err = (got - want).abs()
    excess = float((err - bound).max())
    line = f"\n{tag} {case.kernel} {kind} ({case.ftot},{case.hw}) halves {case.halves}: max |got - want| {float(err.max()):.3e}, " \
           f"worst excess over the bound {excess:.3e}"
    ratio = None
    if second_round_from is not None:
        e2, b2 = err.reshape(-1)[second_round_from:], bound.reshape(-1)[second_round_from:]
        ratio = float((e2 / b2).max())
        line += f"; second round ({e2.numel()} elements): worst excess {float((e2 - b2).max()):.3e}, worst |err| / bound {ratio:.3f}"
    if h_got is not None:
        line += f"; history max |h - m0| {float((h_got.double() - m0).abs().max()):.3e} (bound {hb:.3e})"
    print(line)
    assert torch.isfinite(got).all()
    assert (err <= bound).all(), (float(err.max()), excess)
    if second_round_from is not None:
        assert e2.numel() > 0 and (e2 <= b2).all(), float((e2 - b2).max())
    if h_got is not None:
        assert torch.isfinite(h_got).all() and float((h_got.double() - m0).abs().max()) <= hb
    return float(err.max()), excess, ratio
