"""TEST INFRASTRUCTURE: adaptive projected guidance (APG; Sadat, Hilliges, Weber, arXiv 2410.02416, Algorithm 1) as this project defines it --
on the data prediction, with PER-FRAME statistics and a momentum state -- stated in torch at the caller's dtype, the denoising loop of
oracle/cpu_ref.py restated with it (rebuilt from the oracle's own parts exactly as tests/rescale_ref.py does: oracle.cpu_ref.denoise_loop hands
only the guided v to its scheduler, APG also needs c, x and the step's abar), and CPU emulations of the three operators the feature adds to
mikudance_amd.ops, which tests/fake_ops.py installs with its own.

    apg(u, c, x, a, s, g, eta, r, beta, m_prev, dims)   the definition: -> dict(v, m, S, proj, K, D_c, D_g, N2, Q)
    coefficients(N2, P, Q, eta, r)                       (S, proj, K) from a frame's three sums
    denoise_loop(..., apg_on=, apg_eta=, ...)            oracle.cpu_ref.denoise_loop's signature; apg_on=False is that loop op for op
    cfg_apg_prepare / cfg_ddim_step_apg / cfg_multistep_step_apg   the operators' emulations (installed by fake_ops.install)
"""
import torch

from oracle import cpu_ref as O

import fake_ops


def coefficients(N2, P, Q, eta, r):
    """(S, proj, K) from a frame's sums, with the two rules for a vanishing norm."""
    one, zero = torch.ones_like(N2), torch.zeros_like(N2)
    S = one if r == 0 else torch.where(N2 == 0, one, torch.clamp(r / torch.where(N2 == 0, one, N2).sqrt(), max=1.0))
    proj = torch.where(Q == 0, zero, P / torch.where(Q == 0, one, Q))
    return S, proj, (1 - eta) * S * proj


def apg(u, c, x, a, s, g, eta, r, beta, m_prev, dims):
    """One step of APG on tensors of one layout.  `dims`: the dimensions of ONE frame (every dimension but the frame axis), over which the
    statistics are taken.  a = sqrt(abar_t), s = sqrt(1 - abar_t) > 0.  beta == 0 never reads m_prev (it may be None, or hold NaN).

        D_c = a x - s c ;  m = s (u - c) + beta m_prev                       (= (D_c - D_u) + beta m_prev)
        N2 = sum m^2, P = sum m D_c, Q = sum D_c^2                           per frame
        S = 1 if r == 0 or N2 == 0 else min(1, r / sqrt(N2));  proj = 0 if Q == 0 else P / Q;  K = (1 - eta) S proj
        D_g = D_c + (g - 1) (S m - K D_c);   v_g = c - (g - 1) (S m - K D_c) / s
    """
    D_c = a * x - s * c
    m = s * (u - c)
    if beta != 0:
        m = m + beta * m_prev
    N2 = (m * m).sum(dims, keepdim=True)
    P = (m * D_c).sum(dims, keepdim=True)
    Q = (D_c * D_c).sum(dims, keepdim=True)
    S, proj, K = coefficients(N2, P, Q, eta, r)
    upd = S * m - K * D_c
    return dict(v=c - (g - 1) * upd / s, m=m, S=S, proj=proj, K=K, D_c=D_c, D_g=D_c + (g - 1) * upd, N2=N2, Q=Q)


def alpha_sigma(t):
    """(sqrt(abar_t), sqrt(1 - abar_t)) of the oracle's table as Python floats."""
    abar = float(O.DDIM().alphas_cumprod[int(t)])
    return abar ** 0.5, (1.0 - abar) ** 0.5


def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, guidance_scale=3.5,
                 context_frames=30, context_stride=1, context_overlap=8, scheduler=None, reduced=False,
                 on_step=None, eta=0.0, generator=None, noise_dtype=None, apg_on=False, apg_eta=0.0, apg_norm_threshold=0.0, apg_momentum=0.0,
                 on_apg=None):
    """oracle.cpu_ref.denoise_loop with APG in place of u + g (c - u) under CFG (reference src/pipelines/pipeline_mikudance.py between :670-674
    and :678); the momentum state lives for this call.  on_apg(t, result dict of apg()) is called every step."""
    sch = scheduler or O.DDIM()
    timesteps = sch.set_timesteps(num_steps)
    F_ = latents.shape[2]
    cache = {}
    cfg = guidance_scale > 1.0
    nb = 2 if cfg else 1
    m_prev = torch.zeros_like(latents)
    for t in timesteps:
        noise_pred = torch.zeros((nb,) + tuple(latents.shape[1:]), dtype=latents.dtype, device=latents.device)
        counter = torch.zeros((1, 1, F_, 1, 1), dtype=latents.dtype, device=latents.device)
        windows = O.uniform_windows(0, num_steps, F_, context_frames, context_stride, context_overlap)
        for wi, win in enumerate(windows):
            f = len(win)
            x = latents[:, :, win].repeat(nb, 1, 1, 1, 1)
            if reduced:
                if wi not in cache:
                    g = ref_latents[0, win]
                    ctx = torch.stack([embeds[(f + j) % 2] for j in range(f)]) if cfg else embeds[:1].repeat(f, 1, 1)
                    b_, _ = O.reference_unet_forward(ref_sd, g, ctx)
                    cache[wi] = {k: v.half().to(latents.dtype) for k, v in b_.items()}
                cond = cache[wi]
                banks = {k: torch.cat([torch.zeros_like(v), v]) for k, v in cond.items()} if cfg else cond
            else:
                g = ref_latents[:, win].repeat(nb, 1, 1, 1, 1).reshape((nb * f,) + tuple(ref_latents.shape[2:]))
                ctx = embeds[:nb].repeat((f, 1, 1))
                b_, _ = O.reference_unet_forward(ref_sd, g, ctx)
                banks = {k: v.half().to(latents.dtype) for k, v in b_.items()}
            pred = O.denoising_unet_forward(den_sd, x, t, embeds[:nb], banks, cfg=cfg)
            if len(set(win)) == len(win):
                noise_pred[:, :, win] = noise_pred[:, :, win] + pred
                counter[:, :, win] = counter[:, :, win] + 1
            else:                                                            # duplicate frames: the LAST occurrence lands (as the oracle)
                last = {fr: j for j, fr in enumerate(win)}
                frs, js = list(last.keys()), list(last.values())
                noise_pred[:, :, frs] = noise_pred[:, :, frs] + pred[:, :, js]
                counter[:, :, frs] = counter[:, :, frs] + 1
        if cfg:
            u, c = (noise_pred / counter).chunk(2)
            if apg_on:
                a, s = alpha_sigma(t)
                res = apg(u, c, latents, a, s, guidance_scale, apg_eta, apg_norm_threshold, apg_momentum, m_prev, dims=(0, 1, 3, 4))
                v, m_prev = res["v"], res["m"]
                if on_apg is not None:
                    on_apg(int(t), res)
            else:
                v = u + guidance_scale * (c - u)
        else:
            v = noise_pred
        z = None
        if eta > 0:
            gdev = generator.device if generator is not None else latents.device
            z = torch.randn(latents.shape, generator=generator, device=gdev, dtype=noise_dtype or latents.dtype).to(latents)
        latents = sch.step(v, t, latents, eta=eta, noise=z)
        if on_step is not None:
            on_step(int(t), latents)
    return latents


# ------------------------------------------------------------------ the three operators, emulated like tests/fake_ops.py emulates the others
# fp32 arithmetic on the (ftot, hw, 4) layout, the statistics in float64, one rounding of the latents.  The update itself is fake_ops' own
# step emulation run on v_g (its one-clip-half form takes v as it is), so there is one restatement of each scheduler update.
NAMES = ("cfg_apg_prepare", "cfg_ddim_step_apg", "cfg_multistep_step_apg")


def apg_calls():
    """(name, record) of every step-tail operator so far that starts with cfg_, the three above included, in call order."""
    return [(n, d) for n, d in fake_ops.CALLS if n.startswith("cfg_")]


def _halves(noise_sum, counter):
    u, c = (noise_sum / counter.view(1, -1, 1, 1)).unbind(0)
    return u, c


def cfg_apg_prepare(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, alpha_s, sigma_s, momentum, eta, norm_threshold):
    fake_ops._log("cfg_apg_prepare", ftot=ftot, hw=hw, alpha_s=alpha_s, sigma_s=sigma_s, momentum=momentum, eta=eta, norm_threshold=norm_threshold,
                  momentum_buf_was_zero=not bool(momentum_buf.any()))
    assert momentum_buf.dtype == torch.float32 and tuple(momentum_buf.shape) == (ftot, hw, 4) and tuple(coef.shape) == (ftot, 2)
    u, c = _halves(noise_sum, counter)
    x = latents.float().view(ftot, hw, 4)
    m = sigma_s * (u - c)
    if momentum != 0.0:
        m = m + momentum * momentum_buf
    momentum_buf.copy_(m)
    md, dc = m.double(), (alpha_s * x - sigma_s * c).double()
    S, _, K = coefficients((md * md).sum((1, 2)), (md * dc).sum((1, 2)), (dc * dc).sum((1, 2)), eta, norm_threshold)
    coef.copy_(torch.stack([S, K], 1).float())
    return coef


def _v_g(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, guidance, a, s):
    _, c = _halves(noise_sum, counter)
    x = latents.float().view(ftot, hw, 4)
    S, K = coef[:, 0].view(-1, 1, 1), coef[:, 1].view(-1, 1, 1)
    return c - (guidance - 1.0) * (S * momentum_buf - K * (a * x - s * c)) / s


def cfg_ddim_step_apg(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, guidance, alpha_t, alpha_prev, eta=0.0, variance_noise=None):
    v = _v_g(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, guidance, alpha_t ** 0.5, (1 - alpha_t) ** 0.5)
    n = len(fake_ops.CALLS)
    fake_ops.cfg_ddim_step(latents, v[None], None, ftot, hw, guidance, alpha_t, alpha_prev, halves=1, eta=eta, variance_noise=variance_noise)
    del fake_ops.CALLS[n:]
    fake_ops._log("cfg_ddim_step_apg", dict(variance_noise=variance_noise), ftot=ftot, hw=hw, guidance=guidance, alpha_t=alpha_t,
                  alpha_prev=alpha_prev, eta=eta)


def cfg_multistep_step_apg(latents, noise_sum, counter, history, momentum_buf, coef, ftot, hw, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                           variance_noise=None):
    v = _v_g(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, guidance, alpha_s, sigma_s)
    n = len(fake_ops.CALLS)
    fake_ops.cfg_multistep_step(latents, v[None], None, history, ftot, hw, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z, halves=1,
                                variance_noise=variance_noise)
    del fake_ops.CALLS[n:]
    fake_ops._log("cfg_multistep_step_apg", dict(variance_noise=variance_noise), ftot=ftot, hw=hw, guidance=guidance, alpha_s=alpha_s,
                  sigma_s=sigma_s, c_x=c_x, c_m0=c_m0, c_m1=c_m1, c_z=c_z)
