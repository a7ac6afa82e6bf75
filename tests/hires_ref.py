"""TEST INFRASTRUCTURE of two-pass high-resolution sampling (hires_scale=): the float64 reference of md_latent_resize_f16, the bound the kernel is
held to, the kernel test's shapes and inputs, and the emulation of ops.latent_resize for the CPU tests of the host side.

    resize_ref(x, ho, wo, mode)      x (F, hi, wi, 4) fp16 -> float64 (F, ho, wo, 4): torch.nn.functional.interpolate on the fp16 values cast to
                                     float64 (align_corners=False, antialias=False; "nearest" = torch's nearest-exact)
    within_one_ulp(y, ref)           |y - ref| <= 2^-10 max(|ref|, 2^-14) for every element: one rounding to fp16 (half an ulp, an ulp being at
                                     most 2^-10 |ref| and 2^-24 below the normal range) plus room for the accumulation to cross a rounding
                                     boundary.  Where fp16(ref) is infinite (bicubic overshoot of +-65504) y must be that infinity
    latent_resize(...)               the operator's emulation: the reference rounded to fp16, logged in fake_ops.CALLS
"""
import torch
import torch.nn.functional as F

F16 = torch.float16
TORCH_MODES = {"nearest": "nearest-exact", "bilinear": "bilinear", "bicubic": "bicubic"}
# (F, (Hi, Wi), (Ho, Wo)): exact 2x; 1.5x; unequal non-integer ratios at odd sizes; every tap clamped; the identity; down; more than one grid round
SHAPES = [(3, (8, 6), (16, 12)), (3, (6, 10), (9, 15)), (3, (5, 7), (12, 9)), (3, (1, 1), (4, 4)), (3, (2, 3), (2, 3)), (3, (12, 8), (6, 4)),
          (1, (64, 64), (128, 128))]


def resize_ref(x, ho, wo, mode):
    assert x.dtype == F16 and x.dim() == 4 and x.shape[-1] == 4
    kw = {} if mode == "nearest" else dict(align_corners=False, antialias=False)
    return F.interpolate(x.double().permute(0, 3, 1, 2), size=(ho, wo), mode=TORCH_MODES[mode], **kw).permute(0, 2, 3, 1).contiguous()


def within_one_ulp(y, ref):
    """(ok, worst |y - ref| / bound over the elements whose fp16 reference is finite)."""
    y, want = y.double(), ref.to(F16)
    inf = torch.isinf(want)
    ok_inf = torch.equal(y[inf], want[inf].double())
    bound = 2.0 ** -10 * ref.abs().clamp_min(2.0 ** -14)
    ratio = ((y - ref).abs() / bound)[~inf]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    return ok_inf and bool(torch.isfinite(y[~inf]).all()) and worst <= 1.0, worst


def random_latents(f, hi, wi, seed):
    """Uniform in [-4, 4], rounded to fp16."""
    return (torch.rand((f, hi, wi, 4), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 8 - 4).to(F16)


def extreme_latents(f, hi, wi, seed):
    """+-65504 (the largest fp16), fp16 subnormals of both signs (the smallest, the largest, random ones) and a few ordinary values."""
    g = torch.Generator().manual_seed(seed)
    n = f * hi * wi * 4
    sub = (torch.randint(1, 1024, (n,), generator=g).double() * 2.0 ** -24) * (torch.randint(0, 2, (n,), generator=g).double() * 2 - 1)
    pick = torch.randint(0, 6, (n,), generator=g)
    vals = torch.where(pick == 0, torch.full((n,), 65504.0, dtype=torch.float64), sub)
    vals = torch.where(pick == 1, torch.full((n,), -65504.0, dtype=torch.float64), vals)
    vals = torch.where(pick == 2, torch.rand((n,), generator=g, dtype=torch.float64) * 8 - 4, vals)
    fixed = torch.tensor([2.0 ** -24, -2.0 ** -24, 1023 * 2.0 ** -24, -1023 * 2.0 ** -24, 65504.0, -65504.0], dtype=torch.float64)
    vals[:min(6, n)] = fixed[:min(6, n)]                          # every kind is there, whatever the draw
    return vals.to(F16).view(f, hi, wi, 4)


def latent_resize(x, F_, hi, wi, ho, wo, mode="bicubic", out=None):
    """The emulation of mikudance_amd.ops.latent_resize: same argument meaning, the float64 reference rounded once to fp16."""
    import fake_ops
    assert x.dtype == F16 and x.is_contiguous() and x.numel() == F_ * hi * wi * 4 and mode in TORCH_MODES
    fake_ops.CALLS.append(("latent_resize", dict(F=F_, hi=hi, wi=wi, ho=ho, wo=wo, mode=mode)))
    y = resize_ref(x.view(F_, hi, wi, 4), ho, wo, mode).to(F16)
    if out is None:
        return y
    assert out.is_contiguous() and out.numel() == y.numel()
    out.view(y.shape).copy_(y)
    return out


def install(monkeypatch):
    """fake_ops.install and this operator on top of it."""
    import fake_ops
    from mikudance_amd import ops
    fake_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "latent_resize", latent_resize, raising=False)
