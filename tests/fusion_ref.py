"""TEST INFRASTRUCTURE: open-ended windows and weighted window fusion, restated from their definitions, not imported from the product.

    open_windows(F, s, o, levels)    the `uniform_open` layout, written from its rule in this file's own words
    pyramid(L), diffusers_pyramid(L) slot weights min(j + 1, L - j) and diffusers' FreeNoise list construction of the same numbers
    slots(win), shares(windows, F)   which slots accumulate (the reference's last-occurrence rule) and the float64 per-frame-normalised weights
    denoise_loop(..., schedule=, fuse=)  the loop of tests/rescale_ref.py (itself the oracle's loop rebuilt from the oracle's parts) taking a
                                     window list and a weight rule; with the oracle's uniform windows and fuse="flat" it is that loop op for op
The operator's CPU emulation is tests/fake_ops.window_accumulate_weighted.
"""
import math

import torch

from oracle import cpu_ref as O

import rescale_ref as RR


# ---- the open layout
def open_windows(F, s, o, levels):
    """No window leaves the clip.  Per level l < levels (and l <= ceil(log2(F / s))): step d = 2^l between a window's frames, so a window
    covers (s - 1) d + 1 frames; windows begin every s d - o frames from 0 and the first one that would not fit is moved back to end on
    frame F - 1 and is the level's last.  Levels stop at the first whose windows are longer than the clip.  No window twice."""
    if F <= s:
        return [list(range(F))]
    if s - o <= 0:
        raise ValueError("overlap >= size")
    n_levels = min(levels, int(math.ceil(math.log2(F / s))) + 1)
    seen, out = set(), []
    for lvl in range(n_levels):
        d = 1 << lvl
        cover = (s - 1) * d + 1
        if cover > F:
            break
        b = 0
        while True:
            fits = b + cover <= F
            start = b if fits else F - cover
            win = tuple(start + k * d for k in range(s))
            if win not in seen:
                seen.add(win)
                out.append(list(win))
            if not fits or start + cover == F:
                break
            b += s * d - o
    return out


# ---- the weights
def pyramid(L):
    return [min(j + 1, L - j) for j in range(L)]


def diffusers_pyramid(L):
    """diffusers FreeNoise (free_noise_utils, weighting_scheme == "pyramid"), its list construction verbatim in spirit: an ascending run,
    the peak once for odd lengths, the run mirrored."""
    if L % 2 == 0:
        mid = L // 2
        weights = list(range(1, mid + 1))
        return weights + weights[::-1]
    mid = (L + 1) // 2
    weights = list(range(1, mid))
    return weights + [mid] + weights[::-1]


def slots(win):
    """Frame per slot, -1 where a LATER slot of the same window names the same frame (index_put with duplicates: the last one lands)."""
    last = {fr: j for j, fr in enumerate(win)}
    return [fr if last[fr] == j else -1 for j, fr in enumerate(win)]


def shares(windows, F, rule="pyramid"):
    """Per window a float64 tensor of per-slot shares: weight / (sum of the weights of every accumulating slot on that frame, all windows)."""
    assert rule == "pyramid"
    tot = torch.zeros(F, dtype=torch.float64)
    for win in windows:
        for fr, w in zip(slots(win), pyramid(len(win))):
            if fr >= 0:
                tot[fr] += w
    out = []
    for win in windows:
        out.append(torch.tensor([w / float(tot[fr]) if fr >= 0 else 0.0 for fr, w in zip(slots(win), pyramid(len(win)))], dtype=torch.float64))
    return out


def make_windows(schedule, F, context_frames, context_stride, context_overlap, num_steps=1):
    if schedule == "uniform":
        return [list(w) for w in O.uniform_windows(0, num_steps, F, context_frames, context_stride, context_overlap)]
    assert schedule == "uniform_open"
    return open_windows(F, context_frames, context_overlap, context_stride)


# ---- the loop
def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, guidance_scale=3.5, context_frames=30, context_stride=1,
                 context_overlap=8, scheduler=None, reduced=False, on_step=None, eta=0.0, generator=None, noise_dtype=None,
                 guidance_rescale=0.0, schedule="uniform", fuse="flat"):
    """tests/rescale_ref.denoise_loop with the windows of `schedule` and the fusion rule `fuse`.  flat: += pred, counter += 1, divided under
    CFG only (the oracle).  pyramid: += share * pred with the normalised shares above; the buffer is the weighted mean with and without CFG
    (the counter, the sum of the shares, is 1).  Video-to-video: hand in tests/v2v_ref.Truncated as the scheduler and v2v_ref.noised latents."""
    sch = scheduler or O.DDIM()
    timesteps = sch.set_timesteps(num_steps)
    F_ = latents.shape[2]
    cache = {}
    cfg = guidance_scale > 1.0
    nb = 2 if cfg else 1
    for t in timesteps:
        noise_pred = torch.zeros((nb,) + tuple(latents.shape[1:]), dtype=latents.dtype, device=latents.device)
        counter = torch.zeros((1, 1, F_, 1, 1), dtype=latents.dtype, device=latents.device)
        windows = make_windows(schedule, F_, context_frames, context_stride, context_overlap, num_steps)
        wts = shares(windows, F_) if fuse == "pyramid" else None
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
            if wts is not None:
                sl = slots(win)
                js = [j for j, fr in enumerate(sl) if fr >= 0]
                frs = [sl[j] for j in js]
                w = wts[wi][js].to(device=pred.device, dtype=pred.dtype).view(1, 1, -1, 1, 1)
                noise_pred[:, :, frs] = noise_pred[:, :, frs] + w * pred[:, :, js]
                counter[:, :, frs] = counter[:, :, frs] + w
            elif len(set(win)) == len(win):
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
                v = RR.rescale_noise_cfg(v, c, guidance_rescale)
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

