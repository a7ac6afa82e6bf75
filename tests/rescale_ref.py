"""TEST INFRASTRUCTURE: the denoising loop of oracle/cpu_ref.py restated with guidance rescale (rescaled classifier-free guidance, Lin et al.,
arXiv 2305.08891 section 3.4, as diffusers writes it in rescale_noise_cfg).  oracle.cpu_ref.denoise_loop hands only the guided output v to
its scheduler, and the rescale also needs the conditional half c, so the loop is rebuilt here from the oracle's own parts
(uniform_windows, reference_unet_forward, denoising_unet_forward, DDIM; tests/dpmpp_ref.Restated plugs in as the scheduler like there).

    rescale_noise_cfg(v, c, phi)           diffusers' formula on (1, 4, F, h, w) tensors, std over every non-batch dimension
    denoise_loop(..., guidance_rescale=)   oracle.cpu_ref.denoise_loop's signature and device-agnostic behaviour; 0.0 is that loop op for op
"""
import torch

from oracle import cpu_ref as O


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale):
    """diffusers rescale_noise_cfg: std over all dimensions but the batch (unbiased, torch.std), v * std(c) / std(v) blended with v by phi.
    The one deviation the product documents: std(v) == 0 leaves v unscaled (diffusers would divide by zero)."""
    dims = list(range(1, noise_pred_text.ndim))
    std_text = noise_pred_text.std(dim=dims, keepdim=True)
    std_cfg = noise_cfg.std(dim=dims, keepdim=True)
    ratio = torch.where(std_cfg == 0, torch.ones_like(std_cfg), std_text / std_cfg)
    noise_pred_rescaled = noise_cfg * ratio
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, guidance_scale=3.5,
                 context_frames=30, context_stride=1, context_overlap=8, scheduler=None, reduced=False,
                 on_step=None, eta=0.0, generator=None, noise_dtype=None, guidance_rescale=0.0):
    """oracle.cpu_ref.denoise_loop with `guidance_rescale` (phi) applied to v after CFG and before the scheduler step (reference
    src/pipelines/pipeline_mikudance.py between :670-674 and :678), under CFG only, as in diffusers."""
    sch = scheduler or O.DDIM()
    timesteps = sch.set_timesteps(num_steps)
    F_ = latents.shape[2]
    cache = {}
    cfg = guidance_scale > 1.0
    nb = 2 if cfg else 1
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
            v = u + guidance_scale * (c - u)
            if guidance_rescale > 0.0:
                v = rescale_noise_cfg(v, c, guidance_rescale)
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
