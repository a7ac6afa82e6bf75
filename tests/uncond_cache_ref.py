"""TEST INFRASTRUCTURE: guidance_interval= / uncond_cache_interval= (guidance in a limited interval, arXiv 2404.07724; the CFG cache of FasterCache,
arXiv 2410.19355, the idea only) as this project defines them, and the CPU emulation of the operator the feature adds to mikudance_amd.ops.

    store64 / restore64                  md_cfg_uncond_cache's two modes in float64
    step_kinds(N, ks, lo, hi, n)         "off" | "full" | "cached" per schedule index, by a rule of its own (the distance to the last full step)
    denoise_loop(pipe, ...)              the sampling loop restated: the pipeline's own UNet calls (bank write, forward_nhwc on both clip-halves or
                                         with conditional=True, PAG's perturbed call), everything behind them -- window sums, u / c / d, the guidance
                                         c + (g - 1) d, PAG's term, the scheduler step (oracle DDIM or tests/dpmpp_ref.py) -- in float64 torch.
                                         The latents are rounded to fp16 after every step, as the product keeps them
    cfg_uncond_cache                     the operator's emulation in fp32, in the kernel's rounding order; install() / install_process() put it
                                         beside the emulations of tests/fake_ops.py (which stays as it is)
"""
import torch

import fake_ops


# ---- the operator in float64
def store64(noise_sum, counter):
    """noise_sum (2, F, HW, 4), counter (F,) -> delta = c_sum / cnt - u_sum / cnt, float64."""
    cnt = counter.double().view(-1, 1, 1)
    return noise_sum[1].double() / cnt - noise_sum[0].double() / cnt


def restore64(noise_sum, counter, delta, scale):
    """-> the u plane u_sum = c_sum - scale delta cnt, float64; scale == 0 never looks at delta."""
    c = noise_sum[1].double()
    return c.clone() if scale == 0 else c - scale * delta.double() * counter.double().view(-1, 1, 1)


# ---- the operator emulated (fp32, the kernel's order: inv, u, c, c - u / delta cnt, scale t, c_sum - t)
def cfg_uncond_cache(noise_sum, counter, delta, ftot, hw, mode, scale=1.0):
    fake_ops._log("cfg_uncond_cache", dict(delta=delta), ftot=ftot, hw=hw, mode=mode, scale=scale)
    assert noise_sum.dtype == counter.dtype == torch.float32 and noise_sum.numel() == 2 * ftot * hw * 4 and mode in (0, 1)
    ns = noise_sum.view(2, ftot, hw, 4)
    cnt = counter[:ftot].view(-1, 1, 1)
    if mode == 0:
        inv = 1.0 / cnt
        delta.view(ftot, hw, 4).copy_(ns[1] * inv - ns[0] * inv)
    elif scale == 0.0:
        ns[0].copy_(ns[1])
    else:
        ns[0].copy_(ns[1] - torch.tensor(scale, dtype=torch.float32) * (delta.view(ftot, hw, 4) * cnt))


def install(monkeypatch):
    """fake_ops.install plus the emulation above: every operator the loop can call with the new keywords."""
    from mikudance_amd import ops
    fake_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "cfg_uncond_cache", cfg_uncond_cache)


def install_process():
    from mikudance_amd import ops
    fake_ops.install_process()
    ops.cfg_uncond_cache = cfg_uncond_cache


def calls():
    """(name, record) of every logged cfg_uncond_cache call, in order."""
    return [(n, d) for n, d in fake_ops.CALLS if n == "cfg_uncond_cache"]


# ---- the step kinds, by a rule of its own
def step_kinds(num_steps, ks, lo, hi, n):
    """The kind of every schedule index in `ks` (the indices one pass runs, in order) of a num_steps-step schedule."""
    out, last_full = [], None
    for k in ks:
        if not (lo * num_steps <= k < hi * num_steps):
            out.append("off")
            last_full = None
        elif last_full is None or k - last_full >= n:
            out.append("full")
            last_full = k
        else:
            out.append("cached")
    return out


# ---- the loop restated
def _planes(pred, f, hw, nb):
    return pred.view(nb, f, hw, 4).double().cpu()


@torch.no_grad()
def denoise_loop(pipe, latents, ref_latents, embeds, num_steps, guidance_scale, scheduler, interval=(0.0, 1.0), n=1, context_frames=None,
                 context_stride=1, context_overlap=8, pag_scale=0.0, pag_layers=("mid",), on_step=None):
    """latents (1, 4, F, h, w), ref_latents (1, F, 22, h, w), embeds (2, L, D) = [zeros, CLIP tokens], fp16 on the models' device; `scheduler`:
    oracle.cpu_ref.DDIM() or dpmpp_ref.Restated().  Classifier-free guidance (guidance_scale > 1), "uniform" windows, flat fusion.
    on_step(k, kind) is called every step.  -> latents (1, 4, F, h, w) float32 on the host."""
    from mikudance_amd import ReferenceAttentionControl, ops
    from mikudance_amd.context import get_context_scheduler
    den, refu = pipe.denoising_unet, pipe.reference_unet
    dev = latents.device
    _, ch, F_, hh, ww = latents.shape
    hw = hh * ww
    g = float(guidance_scale)
    timesteps = [int(t) for t in scheduler.set_timesteps(num_steps)]
    kinds = step_kinds(num_steps, range(num_steps), interval[0], interval[1], n)
    windows = [list(w) for w in get_context_scheduler("uniform")(0, num_steps, F_, context_frames or pipe.default_context_frames, context_stride,
                                                                 context_overlap)]
    writer = ReferenceAttentionControl(refu, do_classifier_free_guidance=True, mode="write", batch_size=1, fusion_blocks="full")
    reader = ReferenceAttentionControl(den, do_classifier_free_guidance=True, mode="read", batch_size=1, fusion_blocks="full")
    blocks = reader._blocks(den)
    pag = den.pag_blocks(tuple(pag_layers)) if pag_scale > 0 else None
    x64 = latents.double().cpu()
    banks, d_last = {}, None
    den.clear_context_cache()
    refu.clear_context_cache()
    try:
        for k, t in enumerate(timesteps):
            kind = kinds[k]
            if on_step is not None:
                on_step(k, kind)
            u_sum, c_sum, p_sum = (torch.zeros((F_, hw, 4), dtype=torch.float64) for _ in range(3))
            cnt = torch.zeros((F_,), dtype=torch.float64)
            lat16 = x64.half().to(dev)
            for wi, win in enumerate(windows):
                f = len(win)
                idx = torch.tensor(win, dtype=torch.long, device=dev)
                if wi not in banks:
                    pipe._write_banks(writer, reader, embeds, ref_latents, idx, f, True, literal=False)
                    banks[wi] = [blk.bank for blk in blocks]
                else:
                    for blk, bk in zip(blocks, banks[wi]):
                        blk.bank = bk
                sample = lat16[:, :, idx].repeat(2, 1, 1, 1, 1).contiguous()                 # (2, 4, f, h, w): both clip-halves, the same latents
                st = sample.stride()
                x = ops.pack_nhwc(sample, 2 * f, f, (st[0], st[2], st[1], st[3], st[4]), 0, ch, 64, hh, ww)
                cross = den._cross(embeds[:2], [i // f for i in range(2 * f)], dev)
                last = {fr: j for j, fr in enumerate(win)}                                  # a frame named twice: the last occurrence lands
                frs, js = list(last.keys()), list(last.values())
                if kind == "full":
                    pred = _planes(den.forward_nhwc(x, 2, f, torch.full((2,), float(t)), cross), f, hw, 2)
                    u_sum[frs] += pred[0][js]
                    c_sum[frs] += pred[1][js]
                else:
                    pred = _planes(den.forward_nhwc(x[f:], 1, f, torch.full((1,), float(t)), cross.rows(f, 2 * f), conditional=True), f, hw, 1)
                    c_sum[frs] += pred[0][js]
                cnt[frs] += 1
                if pag is not None:
                    pred = _planes(den.forward_nhwc(x[f:], 1, f, torch.full((1,), float(t)), cross.rows(f, 2 * f), pag=pag), f, hw, 1)
                    p_sum[frs] += pred[0][js]
                reader.clear()
                writer.clear()
            c = c_sum / cnt.view(-1, 1, 1)
            if kind == "full":
                u = u_sum / cnt.view(-1, 1, 1)
                v = u + g * (c - u)
                if n > 1:
                    d_last = c - u
            elif kind == "cached":
                v = c + (g - 1.0) * d_last
            else:
                v = c
            if pag is not None:
                v = v + pag_scale * (c - p_sum / cnt.view(-1, 1, 1))
            v5 = v.view(F_, hh, ww, 4).permute(3, 0, 1, 2)[None]
            x64 = scheduler.step(v5, t, x64).half().double()                                # fp16 latents between the steps, as the product's
    finally:
        reader.clear()
        writer.clear()
        den.clear_context_cache()
        refu.clear_context_cache()
    return x64.float()
