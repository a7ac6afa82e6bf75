"""TEST INFRASTRUCTURE: an independent float64 restatement of DPM-Solver++ multistep sampling (Lu et al., arXiv 2211.01095) on the
model's own discrete schedule, written the way diffusers' DPMSolverMultistepScheduler writes its updates (lambda, h, D0 / D1), with
numpy's infinities carrying the zero-terminal-SNR ends (lambda = -inf at t = 999, +inf at the clean end).  The product
(mikudance_amd.DPMSolverMultistepScheduler) writes the same coefficients in a ratio form instead; the tests compare the two.

    coefficients(n, order, algorithm, solver) -> [(alpha_s, sigma_s, c_x, c_m0, c_m1, c_z)] per step
    Restated(...)                              a scheduler for oracle.cpu_ref.denoise_loop(..., scheduler=)
"""
import numpy as np
import torch

from oracle import cpu_ref as O


def schedule(n):
    """(timesteps, abar per step with the clean end appended) from the oracle's DDIM table."""
    d = O.DDIM()
    ts = [int(t) for t in d.set_timesteps(n)]
    abar = np.array([float(d.alphas_cumprod[t]) for t in ts] + [1.0], dtype=np.float64)
    return ts, abar


def coefficients(n, order=2, algorithm="dpmsolver++", solver="midpoint"):
    _, abar = schedule(n)
    alpha, sigma = np.sqrt(abar), np.sqrt(1.0 - abar)
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(sigma)                        # -inf at t = 999, +inf at the clean end
    out = []
    for i in range(n):
        a_s, s_s, a_t, s_t = alpha[i], sigma[i], alpha[i + 1], sigma[i + 1]
        h = lam[i + 1] - lam[i]
        emh = np.exp(-h)
        o = 1 if (order == 1 or i == 0 or i == n - 1) else 2
        r = (h / (lam[i] - lam[i - 1])) if o == 2 else 0.0        # 1 / r0 = h / h_0; 0 when lambda_{i-1} = -inf
        if algorithm == "dpmsolver++":
            c_x, c_d0, c_z = s_t / s_s, -a_t * (emh - 1.0), 0.0
            c_d1 = -0.5 * a_t * (emh - 1.0) if solver == "midpoint" else a_t * ((emh - 1.0) / h + 1.0)
        else:
            e2 = np.exp(-2.0 * h)
            c_x, c_d0, c_z = s_t / s_s * emh, a_t * (1.0 - e2), s_t * np.sqrt(1.0 - e2)
            c_d1 = 0.5 * a_t * (1.0 - e2) if solver == "midpoint" else a_t * ((1.0 - e2) / (-2.0 * h) + 1.0)
        if o == 1 or r == 0.0:
            c_m0, c_m1 = c_d0, 0.0
        else:                                                      # D1 = r (m0 - m1)
            c_m0, c_m1 = c_d0 + c_d1 * r, -c_d1 * r
        out.append(tuple(float(v) for v in (a_s, s_s, c_x, c_m0, c_m1, c_z)))
    return out


class Restated:
    """DPM-Solver++ for oracle.cpu_ref.denoise_loop: set_timesteps(n) -> timesteps, step(v, t, x) -> x'.  The SDE variant draws its
    own z every step from `generator` (on the generator's device, in `noise_dtype`: the pipeline draws in its latents' dtype, fp16)."""

    def __init__(self, order=2, algorithm="dpmsolver++", solver="midpoint", generator=None, noise_dtype=torch.float16):
        self.order, self.algorithm, self.solver = order, algorithm, solver
        self.generator, self.noise_dtype = generator, noise_dtype
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n):
        ts, _ = schedule(n)
        self.co = coefficients(n, self.order, self.algorithm, self.solver)
        self.timesteps = torch.tensor(ts)
        self.i, self.m1 = 0, None
        return self.timesteps

    def step(self, v, t, x, eta=0.0, noise=None):
        assert eta == 0.0 and int(t) == int(self.timesteps[self.i])
        a_s, s_s, c_x, c_m0, c_m1, c_z = self.co[self.i]
        m0 = a_s * x - s_s * v
        out = c_x * x + c_m0 * m0
        if c_m1:
            out = out + c_m1 * self.m1
        if self.algorithm == "sde-dpmsolver++":
            gdev = self.generator.device if self.generator is not None else x.device
            z = torch.randn(x.shape, generator=self.generator, device=gdev, dtype=self.noise_dtype).to(x)
            out = out + c_z * z
        self.m1, self.i = m0, self.i + 1
        return out
