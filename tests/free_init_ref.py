"""TEST INFRASTRUCTURE: FreeInit noise re-initialisation (Wu et al., arXiv 2312.07537; diffusers FreeInitMixin) restated for the tests.
Latents are (F, h, w, C) arrays, channels last like the loop's internal layout; transforms run over the first three axes.

    lpf_literal(F, h, w, kind, order, ds, dt)   diffusers' low-pass table in SHIFTED order, the triple loop, float64
    symmetrised(LPF)                            (U + reflect(U)) / 2 with U = ifftshift(LPF), by explicit index arithmetic
    mix_literal(x0, noise0, z, a, b, LPF)       diffusers' literal form in float64 with torch.fft (LPF shifted)
    mix_dense(x0, noise0, z, a, b, lpf, dtype)  the dense per-axis DFT of md_free_init_mix_f16 restated in numpy (lpf unshifted), before
                                                the rounding to fp16, returned as float64
    half_ulp_f16(v)                             half the fp16 spacing at |v| (2^-25 below 2^-14)
    free_init_mix                               emulation of ops.free_init_mix for the CPU loop tests (mix_literal, one rounding to fp16)
    denoise_loop(...)                           the oracle loop once per FreeInit pass with mix_literal in between
"""
import math

import numpy as np
import torch


def lpf_literal(F, h, w, kind="butterworth", order=4, ds=0.25, dt=0.25):
    out = np.zeros((F, h, w), dtype=np.float64)
    if ds == 0 or dt == 0:
        return out
    for t in range(F):
        for y in range(h):
            for x in range(w):
                d2 = ((ds / dt) * (2 * t / F - 1)) ** 2 + (2 * y / h - 1) ** 2 + (2 * x / w - 1) ** 2
                if kind == "butterworth":
                    out[t, y, x] = 1 / (1 + (d2 / ds ** 2) ** order)
                elif kind == "gaussian":
                    out[t, y, x] = math.exp(-1 / (2 * ds ** 2) * d2)
                elif kind == "ideal":
                    out[t, y, x] = 1.0 if d2 <= ds * 2 else 0.0
                else:
                    raise ValueError(kind)
    return out


def reflect(u):
    """k -> (-k) mod n on the first three axes."""
    F, h, w = u.shape[:3]
    return u[(-np.arange(F)) % F][:, (-np.arange(h)) % h][:, :, (-np.arange(w)) % w]


def symmetrised(lpf_shifted):
    F, h, w = lpf_shifted.shape
    u = lpf_shifted[(np.arange(F) + F // 2) % F][:, (np.arange(h) + h // 2) % h][:, :, (np.arange(w) + w // 2) % w]     # ifftshift
    return 0.5 * (u + reflect(u))


def _t64(v):
    return torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(torch.float64)


def mix_literal(x0, noise0, z, a, b, lpf_shifted):
    """real(ifftn(ifftshift(fftshift(fftn(a x0 + b noise0)) LPF + fftshift(fftn(z)) (1 - LPF)))), float64 tensor.  a == 0: x0 is not read.
    The transforms run channels first, contiguous, over the LAST three axes -- diffusers' own layout (B, C, F, H, W), dim=(-3, -2, -1).
    (torch 2.10's CPU fftn over the leading axes of a channels-last (2, 3, 256, 4) or (2, 3, 130, 4) tensor corrupts the heap.)"""
    first = lambda t: _t64(t).permute(3, 0, 1, 2).contiguous()
    x0, noise0, z = first(x0), first(noise0), first(z)
    lpf = _t64(lpf_shifted)[None]
    dims = (-3, -2, -1)
    z_t = b * noise0 if a == 0 else a * x0 + b * noise0
    xf = torch.fft.fftshift(torch.fft.fftn(z_t, dim=dims), dim=dims)
    nf = torch.fft.fftshift(torch.fft.fftn(z, dim=dims), dim=dims)
    mixed = xf * lpf + nf * (1 - lpf)
    return torch.fft.ifftn(torch.fft.ifftshift(mixed, dim=dims), dim=dims).real.permute(1, 2, 3, 0).contiguous()


def shifted(lpf_unshifted):
    """fftshift of an unshifted table: what mix_literal takes."""
    return np.fft.fftshift(np.asarray(lpf_unshifted, dtype=np.float64))


def _dft_matrix(n, dtype, sign):
    """M[k, j] = table[(j k) mod n] with table[m] = (cos, sign sin)(2 pi m / n) computed in float64 and rounded to `dtype`."""
    m = np.arange(n)
    c, s = np.cos(2 * np.pi * m / n), np.sin(2 * np.pi * m / n)
    c[0], s[0] = 1.0, 0.0
    if n % 4 == 0:
        c[n // 4], c[3 * n // 4] = 0.0, 0.0                       # sincospi is exact there
    if n % 2 == 0:
        s[n // 2] = 0.0
    table = (c.astype(dtype) + 1j * (sign * s).astype(dtype)).astype(np.complex64 if dtype == np.float32 else np.complex128)
    return table[(m[:, None] * m[None, :]) % n]


def mix_dense(x0, noise0, z, a, b, lpf_unshifted, dtype=np.float32):
    """z + IDFT3(lpf DFT3(a x0 + b noise0 - z)) the way the kernel does it: every operand in `dtype`, one axis per pass (W, H, F forward,
    the table times 1 / (F h w), F, H, W inverse), a matrix product with the twiddle table per pass.  Returns float64, NOT rounded to fp16."""
    f = dtype
    x0, noise0, z = (np.asarray(v, dtype=np.float64).astype(f) for v in (x0, noise0, z))
    F, h, w, _ = z.shape
    d = (f(b) * noise0 - z) if a == 0 else (f(a) * x0 + f(b) * noise0 - z)
    cx = np.complex64 if f == np.float32 else np.complex128
    v = d.astype(cx)
    v = np.einsum("kj,fyjc->fykc", _dft_matrix(w, f, -1), v).astype(cx)
    v = np.einsum("kj,fjxc->fkxc", _dft_matrix(h, f, -1), v).astype(cx)
    v = np.einsum("kj,jyxc->kyxc", _dft_matrix(F, f, -1), v).astype(cx)
    gain = f(1.0 / (F * h * w))
    v = (v * (np.asarray(lpf_unshifted, dtype=f) * gain)[..., None]).astype(cx)
    v = np.einsum("kj,jyxc->kyxc", _dft_matrix(F, f, +1), v).astype(cx)
    v = np.einsum("kj,fjxc->fkxc", _dft_matrix(h, f, +1), v).astype(cx)
    v = np.einsum("kj,fyjc->fykc", _dft_matrix(w, f, +1), v).astype(cx)
    return (z + v.real.astype(f)).astype(np.float64)


def half_ulp_f16(v):
    """Half the spacing of fp16 at |v|, elementwise (float64 tensor): 2^(e - 11) for 2^e <= |v| < 2^(e + 1), 2^-25 below 2^-14."""
    v = _t64(v).abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(v)) - 11)


def random_symmetric_table(F, h, w, seed):
    """Uniform [0, 1], symmetric under k -> -k, fp32 numpy (unshifted order): every frequency takes part."""
    u = np.random.default_rng(seed).random((F, h, w))
    return (0.5 * (u + reflect(u))).astype(np.float32)


def random_case(F, h, w, seed):
    """(x0, noise0, z): fp16 tensors (F, h, w, 4), a sample-like x0 and two N(0, 1) draws."""
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.randn((F, h, w, 4), generator=g) * 0.8).half()
    return x0, torch.randn((F, h, w, 4), generator=g).half(), torch.randn((F, h, w, 4), generator=g).half()


# ---- the operator emulated for the CPU loop tests (installed by fake_ops.install)
def free_init_mix(out, x0, noise0, z, lpf, a, b):
    import fake_ops
    fake_ops.CALLS.append(("free_init_mix", dict(a=a, b=b)))
    out.copy_(mix_literal(x0, noise0, z, a, b, shifted(lpf.numpy())).to(torch.float16))
    return out


# ---- the oracle loop composed with the literal mix
def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, iters, generator, make_scheduler=None, fast=False,
                 kind="butterworth", order=4, ds=0.25, dt=0.25, **kw):
    """oracle.cpu_ref.denoise_loop once per FreeInit pass; between passes z is drawn in fp16 from `generator` (the pipeline's draw), the
    result is re-noised to t = T - 1 of the oracle's own table and mixed by mix_literal in float64.  make_scheduler() -> a fresh oracle
    scheduler per pass (None: the oracle's DDIM)."""
    from oracle import cpu_ref as O
    abar = float(O.DDIM().alphas_cumprod[-1])
    a, b = math.sqrt(abar), math.sqrt(1.0 - abar)
    _, _, F, h, w = latents.shape
    lpf = lpf_literal(F, h, w, kind, order, ds, dt)
    pack = lambda t: t[0].permute(1, 2, 3, 0)                        # (1, 4, F, h, w) -> (F, h, w, 4)
    x = latents
    for i in range(iters):
        if i > 0:
            z = torch.randn(latents.shape, generator=generator, dtype=torch.float16)
            mixed = mix_literal(pack(x), pack(latents), pack(z), a, b, lpf)
            x = mixed.permute(3, 0, 1, 2)[None].to(latents.dtype)
        n = max(1, int(num_steps / iters * (i + 1))) if fast else num_steps
        x = O.denoise_loop(ref_sd, den_sd, x, ref_latents, embeds, n, scheduler=make_scheduler() if make_scheduler else None, generator=generator, **kw)
    return x
