"""TEST INFRASTRUCTURE: video-to-video sampling (diffusers img2img / video2video `strength`) restated for the CPU oracle.  The oracle loop
(oracle/cpu_ref.py) is run unchanged on a truncated, pre-noised schedule: the clean latent is noised in float64 from the oracle's own DDIM
table, and the scheduler handed to the loop returns only the kept tail of its timesteps (DPM-Solver++: tests/dpmpp_ref.Restated starting
at the first kept step with that step's ORDER-1 coefficients, nothing in its history).

    kept_steps(n, strength)                   number of steps run, restated with floor() on diffusers' float product
    noised(x0, noise, t)                      sqrt(abar_t) x0 + sqrt(1 - abar_t) noise in float64, returned in noise's dtype
    Truncated(scheduler, strength)            an oracle scheduler (O.DDIM or dpmpp_ref.Restated) limited to the kept tail
    denoise_loop(..., init_latents, strength) oracle.cpu_ref.denoise_loop from the noised start
"""
import math

import torch

from oracle import cpu_ref as O

import dpmpp_ref as R


def kept_steps(n, strength):
    """diffusers: init_timestep = min(int(n * strength), n), t_start = max(n - init_timestep, 0); kept = n - t_start."""
    return max(0, min(math.floor(n * strength), n))


def noised(x0, noise, t):
    abar = float(O.DDIM().alphas_cumprod[int(t)])
    return (math.sqrt(abar) * x0.double() + math.sqrt(1.0 - abar) * noise.double()).to(noise.dtype)


class Truncated:
    def __init__(self, inner, strength):
        self.inner, self.strength = inner, strength
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n):
        full = self.inner.set_timesteps(n)
        start = n - kept_steps(n, self.strength)
        if isinstance(self.inner, R.Restated):                    # first kept step: order 1, no history
            self.inner.i = start
            self.inner.co[start] = R.coefficients(n, 1, self.inner.algorithm, self.inner.solver)[start]
        self.timesteps = full[start:]
        return self.timesteps

    def step(self, *a, **kw):
        return self.inner.step(*a, **kw)


def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, init_latents, strength, scheduler=None, **kw):
    sch = Truncated(scheduler or O.DDIM(), strength)
    t0 = O.DDIM().set_timesteps(num_steps)[num_steps - kept_steps(num_steps, strength)]
    return O.denoise_loop(ref_sd, den_sd, noised(init_latents, latents, t0), ref_latents, embeds, num_steps, scheduler=sch, **kw)
