"""References for the kernel-level GEMM / conv tests (tests/test_gemm_flavours_gpu.py, tests/gemm_flavours_check.py,
tests/test_gemm_floor_cpu.py).  Plain PyTorch, independent of the library; every function runs on the device its operands live on (the
CPU, or float64 / float32 torch matmul on the GPU for the cases whose float64 product would take seconds on the CPU).

`reference`   float64 on the fp16-rounded operands.  GEMM: A W^T (+ bias) (+ rowadd[row // rows_per_group]), SiLU / ReLU / QuickGELU
              (x sigmoid(1.702 x), the CLIP vision tower's MLP), (+ residual) --
              the residual is added LAST, after the activation, as include/mdance_hip.h states for md_gemm_f16 -- or GEGLU
              h * gelu_erf(g) on the UNPACKED halves (w = [h rows | g rows], packing.geglu_weight interleaves them for the kernel);
              transpose_out returns the transpose of the same.  Conv: `conv_patches` writes the implicit-GEMM A matrix out from shifted
              slices of the zero-padded (and nearest-2x upsampled) input -- row (b, oy, ox), column (ky, kx, c) -- so the padding rule is
              stated here and not inherited from F.conv2d: pad_lo zero rows / columns before the image, ONE after it, stride 1 / 2,
              kw = 1 keeps the centre column only (taps along H, no padding along W).  tests/test_gemm_floor_cpu.py checks it against
              F.conv2d / F.conv3d.
`emulation`   the arithmetic md_gemm_f16 / md_conv_nhwc_f16 document and nothing of the kernels' structure: the products accumulated in
              fp32; bias, row term and residual added in fp32; the activation in fp32 (GEGLU: gelu_fast of tests/test_gelu_scheme_cpu.py,
              the kernels' erf-GELU formula, product h * gelu(g) formed in fp32); ONE rounding to fp16.
`rel_l2`      relative L2 against the float64 reference.

rel_l2(emulation) is the FLOOR of a case: what a correct kernel of this arithmetic costs on these very operands, about 2.07e-4 for a
plain GEMM (the one fp16 rounding of the output; pinned in tests/test_gemm_floor_cpu.py).  It is computed per case from the reference alone and
never recorded, so a wrong kernel cannot bless itself.  A kernel passes a case with
    |err| <= 1e-2 max|ref| + 1e-3  elementwise   and   rel_l2 <= parity_budget.KERNEL_FACTOR (1.25) x floor."""
import torch

from parity_budget import KERNEL_FACTOR  # noqa: F401  (re-exported: the factor of the pass rule)
from test_gelu_scheme_cpu import gelu_fast

ACT_NONE, ACT_SILU, ACT_RELU, ACT_GEGLU, ACT_QUICKGELU = 0, 1, 2, 3, 4


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def rel_l2(got, ref64):
    g, r = got.detach().double(), ref64.double()
    return float((g - r).norm() / r.norm())


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def conv_patches(x, kw=3, stride=1, upsample=False, pad_lo=1):
    """x (B, H, W, Cin) -> (A [B*Ho*Wo, 3*kw*Cin] in x's dtype, (Ho, Wo)): the A operand of the implicit GEMM, columns ordered (ky, kx, c)."""
    B, H, W, C = x.shape
    if upsample:                                                   # nearest 2x: pixel (y, x) of the upsampled image is input pixel (y // 2, x // 2)
        x = x[:, torch.arange(2 * H, device=x.device) // 2][:, :, torch.arange(2 * W, device=x.device) // 2]
        H, W = 2 * H, 2 * W
    Ho = (H + pad_lo + 1 - 3) // stride + 1
    Wo = (W + pad_lo + 1 - 3) // stride + 1 if kw == 3 else W
    xp = torch.zeros((B, H + pad_lo + 1, W + (pad_lo + 1 if kw == 3 else 0), C), dtype=x.dtype, device=x.device)
    xp[:, pad_lo:pad_lo + H, (pad_lo if kw == 3 else 0):(pad_lo if kw == 3 else 0) + W] = x
    taps = []
    for ky in range(3):
        for kx in (range(3) if kw == 3 else (0,)):
            taps.append(xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride])
    return torch.cat(taps, dim=-1).reshape(B * Ho * Wo, 3 * kw * C), (Ho, Wo)


def _epilogue(acc, bias, rowadd, rows_per_group, residual, act, gelu):
    dt = acc.dtype
    M = acc.shape[0]
    if bias is not None:
        acc = acc + bias.to(dt)
    if rowadd is not None:
        acc = acc + rowadd.to(dt)[torch.arange(M, device=acc.device) // rows_per_group]
    if act == ACT_SILU:
        acc = torch.nn.functional.silu(acc)
    elif act == ACT_RELU:
        acc = acc.clamp_min(0)
    elif act == ACT_QUICKGELU:
        acc = acc * torch.sigmoid(1.702 * acc)                      # in acc's dtype: float64 (reference) or fp32 (emulation)
    elif act == ACT_GEGLU:
        inner = acc.shape[1] // 2
        acc = acc[:, :inner] * gelu(acc[:, inner:]).to(dt)
    else:
        assert act == ACT_NONE, act
    if residual is not None:
        acc = acc + residual.reshape(M, -1).to(dt)
    return acc


def _compute(dt, gelu, a, w, bias, rowadd, rows_per_group, residual, act, transpose_out):
    out = _epilogue(a.to(dt) @ w.to(dt).t(), bias, rowadd, rows_per_group, residual, act, gelu)
    return out.t() if transpose_out else out


def reference(a, w, bias=None, rowadd=None, rows_per_group=0, residual=None, act=ACT_NONE, transpose_out=False):
    """a [M, K], w [N, K] (GEGLU: unpacked [h | g] rows), fp16 -> float64 [M, N] ([M, N/2] GEGLU, [N, M] transposed)."""
    return _compute(torch.float64, gelu_erf, a, w, bias, rowadd, rows_per_group, residual, act, transpose_out)


def emulation(a, w, bias=None, rowadd=None, rows_per_group=0, residual=None, act=ACT_NONE, transpose_out=False, gelu=gelu_fast):
    """Same operands -> fp16 by the documented arithmetic (see the module docstring)."""
    return _compute(torch.float32, gelu, a, w, bias, rowadd, rows_per_group, residual, act, transpose_out).half()


def conv_reference(x, wpk, kw=3, stride=1, upsample=False, pad_lo=1, **epi):
    """x (B, H, W, Cin) fp16, wpk [Cout, 3*kw*Cin] packed (ky, kx, c) -> float64 (B, Ho, Wo, Cout)."""
    A, (Ho, Wo) = conv_patches(x, kw, stride, upsample, pad_lo)
    return reference(A, wpk, **epi).reshape(x.shape[0], Ho, Wo, -1)


def conv_emulation(x, wpk, kw=3, stride=1, upsample=False, pad_lo=1, **epi):
    A, (Ho, Wo) = conv_patches(x, kw, stride, upsample, pad_lo)
    return emulation(A, wpk, **epi).reshape(x.shape[0], Ho, Wo, -1)


def pass_rule(name, got, ref64, floor, prefix="gemm_flavour"):
    """The pass rule of a case: finite, the elementwise bound of the older tests, and relative L2 <= KERNEL_FACTOR x the case's floor."""
    g, r = got.detach().double(), ref64.double()
    assert g.shape == r.shape, (name, g.shape, r.shape)
    value = rel_l2(g, r)
    print(f"PARITY_MEASURE {prefix}:{name} floor={floor:.6e} got={value:.6e}", flush=True)
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite output (an element that was never written stays NaN)"
    err, bound = float((g - r).abs().max()), 1e-2 * float(r.abs().max()) + 1e-3
    assert err <= bound, f"{name}: max err {err:.4g} > {bound:.4g}"
    assert value <= KERNEL_FACTOR * floor, f"{name}: relative L2 {value:.3e} > {KERNEL_FACTOR} x the floor {floor:.3e}"
    return value
