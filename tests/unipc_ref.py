"""TEST INFRASTRUCTURE: an independent float64 restatement of UniPC sampling (Zhao et al., arXiv 2302.04867) on the model's own discrete
schedule, written the way diffusers' UniPCMultistepScheduler writes its data-prediction updates (lambda, h, rks, R, b, numpy.linalg.solve, the D1s
differences), with numpy's infinities carrying the zero-terminal-SNR ends (lambda = -inf at t = 999, +inf at the clean end).  The product
(mikudance_amd.UniPCMultistepScheduler) forms lambda differences from ratios, solves its systems with its own elimination and hands the
kernel one row of weights per step; the tests compare the two.

    table(zero_snr)                                      abar per training timestep, the product's fp32 table restated
    orders(n, order, zero_snr, begin)                    the predictor order of every step
    coefficients(n, order, solver, zero_snr, begin, disable_corrector) -> one row per step, laid out like
                                                         UniPCMultistepScheduler.unipc_coefficients
    Restated(...)                                        a scheduler for oracle.cpu_ref.denoise_loop(..., scheduler=): the updates in
                                                         diffusers' D1s form on tensors, no weights
    row_update(x, v, state, row)                         one step of the product's row on float64 tensors (what the kernel computes)
    cfg_unipc_step, cfg_unipc_step_apg, cfg_unipc_step_pag   CPU emulations of the three operator wrappers for tests/fake_ops.py's call log
"""
import math

import numpy as np
import torch

import apg_ref
import fake_ops
import pag_ref

NAMES = ("cfg_unipc_step", "cfg_unipc_step_apg", "cfg_unipc_step_pag")


def table(zero_snr=True, n_train=1000, beta_start=0.00085, beta_end=0.012):
    """alphas_cumprod as the product's schedulers build it: fp32 linear betas, optionally rescaled to zero terminal SNR."""
    betas = torch.linspace(beta_start, beta_end, n_train, dtype=torch.float32)
    if zero_snr:
        s = torch.cumprod(1.0 - betas, dim=0).sqrt()
        s0, sT = s[0].clone(), s[-1].clone()
        s = (s - sT) * (s0 / (s0 - sT))
        ab = s ** 2
        betas = 1 - torch.cat([ab[0:1], ab[1:] / ab[:-1]])
    return torch.cumprod(1.0 - betas, dim=0)


def schedule(n, zero_snr=True):
    """(timesteps, alpha, sigma, lambda), the clean end appended to the last three."""
    ts = (np.round(np.arange(1000, 0, -1000 / n)).astype(np.int64) - 1).tolist()
    ac = table(zero_snr)
    abar = np.array([float(ac[t]) for t in ts] + [1.0], dtype=np.float64)
    alpha, sigma = np.sqrt(abar), np.sqrt(1.0 - abar)
    with np.errstate(divide="ignore"):
        lam = np.log(alpha) - np.log(sigma)                        # -inf at t = 999 under zero terminal SNR, +inf at the clean end
    return ts, alpha, sigma, lam


def orders(n, order, zero_snr=True, begin=0):
    """Predictor order per step: min(order, steps left, 1 + the run of earlier steps >= the start whose lambda is finite)."""
    lam = schedule(n, zero_snr)[3]
    out = []
    for i in range(n):
        lo = begin if i >= begin else 0
        hist = 0
        while i - 1 - hist >= lo and np.isfinite(lam[i - 1 - hist]):
            hist += 1
        out.append(min(order, n - i, hist + 1))
    return out


def _rho(rks, hh, B, order, corrector):
    """diffusers multistep_uni_p_bh_update / multistep_uni_c_bh_update: R, b over rks + [1.0], then the hard-coded 0.5 or the solve."""
    rks = list(rks) + [1.0]
    R, b = [], []
    h_phi_k = np.expm1(hh) / hh - 1.0 if np.isfinite(hh) else -1.0
    factorial_i = 1
    for i in range(1, order + 1):
        R.append(np.power(np.array(rks, dtype=np.float64), i - 1))
        b.append(h_phi_k * factorial_i / B)
        factorial_i *= i + 1
        h_phi_k = h_phi_k / hh - 1.0 / factorial_i
    R, b = np.stack(R), np.array(b, dtype=np.float64)
    if corrector:
        return np.array([0.5]) if order == 1 else np.linalg.solve(R, b)
    if order == 1:
        return np.array([])
    return np.array([0.5]) if order == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])


def _update(lam, alpha, sigma, s, t, order, solver, corrector):
    """(h_phi_1, B, rks, rho) of UniP / UniC of `order` from point s to point t, or None where B is unbounded (bh1 out of lambda = -inf)."""
    h = lam[t] - lam[s]
    hh = -h
    h_phi_1 = np.expm1(hh)
    B = hh if solver == "bh1" else np.expm1(hh)
    if (corrector or order > 1) and not np.isfinite(B):
        return None
    rks = [(lam[s - k] - lam[s]) / h for k in range(1, order)]
    return h_phi_1, B, rks, _rho(rks, hh, B, order, corrector)


def corrects(i, n, begin, disable_corrector):
    return i > (begin if i >= begin else 0) and i not in set(disable_corrector)


def coefficients(n, order=2, solver="bh2", zero_snr=True, begin=0, disable_corrector=()):
    """One row per step: (alpha_s, sigma_s, corrector weights on (x_last, m_t, H0, H1, H2), predictor weights on (x^c, m_t, H0, H1), flag)."""
    _, alpha, sigma, lam = schedule(n, zero_snr)
    po = orders(n, order, zero_snr, begin)
    rows = []
    for i in range(n):
        cw, on = [0.0] * 5, False
        if corrects(i, n, begin, disable_corrector):
            up = _update(lam, alpha, sigma, i - 1, i, po[i - 1], solver, True)
            if up is not None:
                on = True
                phi1, B, rks, rho = up
                p = po[i - 1]
                # x_t = sigma_t / sigma_s x - alpha_t h_phi_1 m0 - alpha_t B (sum_k rho_k (m_k - m0) / r_k + rho_p (m_t - m0))
                hist = [-alpha[i] * B * rho[k] / rks[k] for k in range(p - 1)]
                w_t = -alpha[i] * B * rho[p - 1]
                cw = [sigma[i] / sigma[i - 1], w_t, -alpha[i] * phi1 - sum(hist) - w_t] + hist + [0.0] * (3 - p)
        phi1, B, rks, rho = _update(lam, alpha, sigma, i, i + 1, po[i], solver, False)
        hist = [-alpha[i + 1] * B * rho[k] / rks[k] for k in range(po[i] - 1)]
        pw = [sigma[i + 1] / sigma[i], -alpha[i + 1] * phi1 - sum(hist)] + hist + [0.0] * (3 - po[i])
        rows.append(tuple(float(v) + 0.0 for v in [alpha[i], sigma[i]] + cw[:5] + pw[:4]) + (on,))
    return rows


class Restated:
    """UniPC for oracle.cpu_ref.denoise_loop: set_timesteps(n) -> the timesteps from `begin` on, step(v, t, x) -> x'.  Written on tensors as
    diffusers writes it: model_outputs (the last `order` data predictions), last_sample, D1s, einsum-free sums; no weights."""

    def __init__(self, order=2, solver="bh2", zero_snr=True, begin=0, disable_corrector=()):
        self.order, self.solver, self.zero_snr, self.begin, self.off = order, solver, zero_snr, begin, tuple(disable_corrector)
        self.init_noise_sigma = 1.0

    def set_timesteps(self, n):
        ts, self.alpha, self.sigma, self.lam = schedule(n, self.zero_snr)
        self.n, self.po = n, orders(n, self.order, self.zero_snr, self.begin)
        self.timesteps = torch.tensor(ts[self.begin:])
        self.i, self.outputs, self.last = self.begin, [], None        # outputs[-1]: the newest data prediction
        return self.timesteps

    def _terms(self, up, s, t, x_s, m0, older):
        phi1, B, rks, rho = up
        x_t = float(self.sigma[t] / self.sigma[s]) * x_s - float(self.alpha[t] * phi1) * m0
        D1s = [(m - m0) / float(rk) for m, rk in zip(older, rks)]
        return x_t, B, rho, D1s

    def step(self, v, t, x, eta=0.0, noise=None):
        i = self.i
        assert eta == 0.0 and int(t) == int(self.timesteps[i - self.begin])
        m_t = float(self.alpha[i]) * x - float(self.sigma[i]) * v
        if corrects(i, self.n, self.begin, self.off):
            p = self.po[i - 1]
            up = _update(self.lam, self.alpha, self.sigma, i - 1, i, p, self.solver, True)
            if up is not None:
                m0 = self.outputs[-1]
                older = [self.outputs[-(k + 1)] for k in range(1, p)]
                x_t, B, rho, D1s = self._terms(up, i - 1, i, self.last, m0, older)
                corr = sum((float(r) * d for r, d in zip(rho[:-1], D1s)), torch.zeros_like(x))
                x = x_t - float(self.alpha[i] * B) * (corr + float(rho[-1]) * (m_t - m0))
        self.outputs = (self.outputs + [m_t])[-3:]
        self.last = x
        p = self.po[i]
        up = _update(self.lam, self.alpha, self.sigma, i, i + 1, p, self.solver, False)
        older = [self.outputs[-(k + 1)] for k in range(1, p)]
        x_t, B, rho, D1s = self._terms(up, i, i + 1, x, m_t, older)
        if D1s:
            x_t = x_t - float(self.alpha[i + 1] * B) * sum((float(r) * d for r, d in zip(rho, D1s)), torch.zeros_like(x))
        self.i += 1
        return x_t


# ------------------------------------------------------------------ the product's row on tensors, and the operator emulations
def row_update(x, v, state, row):
    """One step of a row on tensors of x's dtype: state = [x_last, H0, H1, H2] (a list, entries may be None / NaN where never written) ->
    (x', the new state), with the kernel's rule for what is read and what moves down."""
    a_s, s_s, cx, cm, c0, c1, c2, px, pm, p0, p1, on = row
    xl, H0, H1, H2 = state
    m_t = a_s * x - s_s * v
    xc = x
    if on:
        xc = cx * xl + cm * m_t
        for w, h in ((c0, H0), (c1, H1), (c2, H2)):
            if w != 0.0:
                xc = xc + w * h
    out = px * xc + pm * m_t
    for w, h in ((p0, H0), (p1, H1)):
        if w != 0.0:
            out = out + w * h
    rd0, rd1 = c0 != 0.0 or p0 != 0.0, c1 != 0.0 or p1 != 0.0
    return out, [xc, m_t, H0 if rd0 else H1, H1 if rd1 else H2]


def _run(name, latents, v, state, ftot, hw, row, **scalars):
    fake_ops._log(name, ftot=ftot, hw=hw, row=[float(c) for c in row[:11]], correct=bool(row[11]), **scalars)
    st = state.view(4, ftot, hw, 4)
    out, new = row_update(latents.float().view(ftot, hw, 4), v, [st[k].clone() for k in range(4)], tuple(float(np.float32(c)) for c in row[:11]) + (row[11],))
    for k in range(4):
        st[k].copy_(new[k])
    latents.copy_(out.view(latents.shape).to(torch.float16))


def cfg_unipc_step(latents, noise_sum, counter, state, ftot, hw, guidance, row, halves=2, vscale=None):
    v, _ = fake_ops._guided(noise_sum, counter, guidance, halves, vscale)
    _run("cfg_unipc_step", latents, v, state, ftot, hw, row, halves=halves, guidance=guidance, scaled=vscale is not None)


def cfg_unipc_step_apg(latents, noise_sum, counter, state, momentum_buf, coef, ftot, hw, guidance, row):
    v = apg_ref._v_g(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, guidance, row[0], row[1])
    _run("cfg_unipc_step_apg", latents, v, state, ftot, hw, row, halves=2, guidance=guidance)


def cfg_unipc_step_pag(latents, noise_sum, counter, state, perturbed_sum, ftot, hw, guidance, pag_scale, row, halves=2):
    v = pag_ref._v(noise_sum, counter, perturbed_sum, ftot, hw, guidance, pag_scale, halves)
    _run("cfg_unipc_step_pag", latents, v, state, ftot, hw, row, halves=halves, guidance=guidance, pag_scale=pag_scale)


def install(monkeypatch):
    """fake_ops.install plus the three emulations above."""
    from mikudance_amd import ops
    fake_ops.install(monkeypatch)
    for name in NAMES:
        monkeypatch.setattr(ops, name, globals()[name])
