"""FreeInit noise re-initialisation (Wu et al., arXiv 2312.07537; diffusers FreeInitMixin): the host side.

Between two sampling passes the loop re-noises the clip to the last training timestep and keeps only the low spatio-temporal frequencies of
that latent; the high ones come from a fresh draw (ops.free_init_mix, md_free_init_mix_f16).  This module builds the low-pass table the
kernel multiplies with and holds the argument checks of the `free_init_*` keywords of MikuDanceVideoPipeline.denoise().

diffusers builds the table in SHIFTED order (frequency 0 in the middle), with d2 = ((ds / dt) (2 t / F - 1))^2 + (2 y / h - 1)^2 +
(2 x / w - 1)^2 for the spatial / temporal stop frequencies ds / dt:
    butterworth  1 / (1 + (d2 / ds^2)^order)
    gaussian     exp(-d2 / (2 ds^2))
    ideal        1 if d2 <= 2 ds else 0          (against 2 ds, not ds^2: diffusers' and the FreeInit repository's own rule, kept)
    ds == 0 or dt == 0: all zeros
and mixes real(ifftn(ifftshift(fftshift(fftn(z_t)) LPF + fftshift(fftn(z)) (1 - LPF)))).  The mix is linear, so the kernel evaluates
z + IDFT3(Lsym DFT3(z_t - z)) with Lsym = (U + reflect(U)) / 2, U = ifftshift(LPF), reflect: k -> (-k mod n) on every axis.  For even
sizes U is symmetric already; for odd sizes it is not, and `.real` discards exactly its antisymmetric part."""
import functools
import math

import numpy as np
import torch

FILTERS = ("butterworth", "gaussian", "ideal")
MAX_AXIS = 256          # md_free_init_plan: every axis of the clip between 1 and 256


def _shifted_lpf(F, h, w, kind, order, ds, dt):
    """diffusers' table, float64, shifted order."""
    if ds == 0 or dt == 0:
        return np.zeros((F, h, w), dtype=np.float64)
    t = ((ds / dt) * (2.0 * np.arange(F, dtype=np.float64) / F - 1.0)) ** 2
    y = (2.0 * np.arange(h, dtype=np.float64) / h - 1.0) ** 2
    x = (2.0 * np.arange(w, dtype=np.float64) / w - 1.0) ** 2
    d2 = t[:, None, None] + y[None, :, None] + x[None, None, :]
    if kind == "butterworth":
        return 1.0 / (1.0 + (d2 / ds ** 2) ** order)
    if kind == "gaussian":
        return np.exp(-d2 / (2.0 * ds ** 2))
    return (d2 <= 2.0 * ds).astype(np.float64)


@functools.lru_cache(maxsize=16)
def _freq_filter(F, h, w, kind, order, ds, dt):
    u = np.fft.ifftshift(_shifted_lpf(F, h, w, kind, order, ds, dt))
    refl = u
    for ax in range(3):                                           # k -> -k mod n: index 0 stays, the rest is reversed
        refl = np.roll(np.flip(refl, ax), 1, ax)
    return torch.from_numpy(((u + refl) * 0.5).astype(np.float32))


def freq_filter(F, h, w, kind="butterworth", order=4, ds=0.25, dt=0.25):
    """The (F, h, w) fp32 table of md_free_init_mix_f16 on the host: computed in float64, unshifted (fftn) order, symmetric under k -> -k;
    cached per argument tuple (treat it as read-only)."""
    check_filter(kind, order, ds, dt)
    return _freq_filter(int(F), int(h), int(w), kind, int(order), float(ds), float(dt))


def check_filter(kind, order, ds, dt):
    if kind not in FILTERS:
        raise ValueError(f"free_init_filter must be one of {FILTERS}, got {kind!r}")
    if isinstance(order, bool) or not isinstance(order, int) or order < 1:
        raise ValueError(f"free_init_order must be an int >= 1, got {order!r}")
    for name, v in (("free_init_spatial_stop", ds), ("free_init_temporal_stop", dt)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")


def check_arguments(iters, kind, order, ds, dt, has_init, shape=None):
    """The refusals of denoise()'s free_init_* keywords, all of them before any model runs.  shape: (F, h, w) of the clip."""
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
        raise ValueError(f"free_init_iters must be an int >= 1, got {iters!r}")
    check_filter(kind, order, ds, dt)
    if iters > 1 and has_init:
        raise ValueError("free_init_iters > 1 cannot be combined with init_latents / video: FreeInit re-noises the clip to the last training "
                         "timestep before every further pass, which discards what strength means")
    if iters > 1 and shape is not None and not all(1 <= int(d) <= MAX_AXIS for d in shape):
        raise ValueError(f"free_init_iters > 1: a clip of (F, h, w) = {tuple(int(d) for d in shape)} latent pixels is outside the FreeInit "
                         f"kernel's range (every axis 1..{MAX_AXIS})")


def pass_steps(num_inference_steps, iters, i, fast):
    """Steps of FreeInit pass i of `iters`: all of them, or diffusers' use_fast_sampling ramp max(1, int(N / iters * (i + 1)))."""
    return max(1, int(num_inference_steps / iters * (i + 1))) if fast else num_inference_steps
