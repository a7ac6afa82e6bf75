"""TEST INFRASTRUCTURE: perturbed-attention guidance (PAG; Ahn et al., arXiv 2403.17377; diffusers PAGMixin) as this project defines it, stated
in torch at the caller's dtype on top of oracle/cpu_ref.py, and CPU emulations of the two operators the feature adds to mikudance_amd.ops,
which tests/fake_ops.py installs with its own.

    combine(u, c, p, g, s) / combine_sum(c_sum, p_sum, s)   the combination rule, under CFG and without
    pag_scale_at(scale, adaptive, t)                        diffusers' _get_pag_scale
    block_prefixes(sd), select(prefixes, names)             the attention blocks of a state dict and the layer-name matching, on strings
    perturbed_forward(den_sd, x, t, ctx, banks, names)      oracle.cpu_ref.denoising_unet_forward as the perturbed conditional evaluation
    denoise_loop(..., pag_scale=, pag_adaptive_scale=, pag_layers=)   tests/fusion_ref.denoise_loop with PAG; pag_scale=0 is that loop op for op
    cfg_ddim_step_pag / cfg_multistep_step_pag              the operators' emulations (installed by fake_ops.install)
The oracle is not edited: the perturbed block and the patcher that swaps it in for the selected prefixes are tests/selfattn_ref.py's.
"""
import re

import torch

from oracle import cpu_ref as O

import fake_ops
import fusion_ref as FR
import selfattn_ref as SA


# ---- the definition
def combine(u, c, p, g, s):
    """Under CFG: diffusers' u + g (c - u) + s (c - p)."""
    return u + g * (c - u) + s * (c - p)


def combine_sum(c_sum, p_sum, s):
    """Without CFG the loop hands the scheduler what the windows added up to: c + s (c - p) on those."""
    return c_sum + s * (c_sum - p_sum)


def pag_scale_at(scale, adaptive, t):
    """diffusers PAGMixin._get_pag_scale (do_pag_adaptive_scaling): scale - adaptive * (1000 - t), not below 0."""
    return max(scale - adaptive * (1000 - int(t)), 0.0)


# ---- layer names, on strings
def block_prefixes(sd):
    """Key prefixes "....attentions.J" of every spatial transformer of a denoising-UNet state dict, in key order."""
    out = []
    for k in sd:
        m = re.match(r"^((?:down_blocks\.\d+|up_blocks\.\d+|mid_block)\.attentions\.\d+)\.transformer_blocks\.0\.norm1\.weight$", k)
        if m:
            out.append(m.group(1))
    return out


def select(prefixes, names):
    """The prefixes that `names` select: equal to a name or starting with name + "."; "mid" stands for "mid_block".  Raises ValueError for an
    empty list of names and for a name that selects nothing."""
    names = [names] if isinstance(names, str) else list(names)
    if not names:
        raise ValueError("no layer names")
    picked = []
    for name in names:
        key = "mid_block" if name == "mid" else name
        hit = [p for p in prefixes if p == key or p.startswith(key + ".")]
        if not hit:
            raise ValueError(f"{name!r} selects no block")
        picked += [p for p in hit if p not in picked]
    return picked


# ---- the perturbed evaluation on the oracle
def _read_identity(sd, p, x, ctx, bank):
    """oracle transformer_block_read(cfg=False) with the identity for softmax(q k^T d^-1/2): attn1 = to_out(to_v(norm1(x) + bank))."""
    return SA.block_read(sd, p, x, ctx, bank, False, identity=True)


def perturbed(selected):
    """Within the block, the oracle's read blocks whose key prefix is in `selected` use the identity attention map (selfattn_ref.modified)."""
    return SA.modified(identity=selected)


def perturbed_forward(den_sd, x, t, ctx, banks, names):
    """x (1, 4, f, h, w), ctx (1, L, D) the CLIP tokens, banks the CONDITIONAL frames' banks: every row reads its bank row (cfg=False)."""
    sel = select(block_prefixes(den_sd), names)
    with perturbed(sel) as seen:
        out = O.denoising_unet_forward(den_sd, x, t, ctx, banks, cfg=False)
    assert sorted(s[0] for s in seen) == sorted(p + ".transformer_blocks.0." for p in sel), (seen, sel)
    return out


# ---- the loop
def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, guidance_scale=3.5, context_frames=30, context_stride=1,
                 context_overlap=8, scheduler=None, on_step=None, eta=0.0, generator=None, noise_dtype=None, schedule="uniform", fuse="flat",
                 pag_scale=0.0, pag_adaptive_scale=0.0, pag_layers=("mid",), on_pag=None):
    """tests/fusion_ref.denoise_loop (reduced=True) with perturbed-attention guidance.  on_pag(t, s_t) is called every step."""
    sch = scheduler or O.DDIM()
    timesteps = sch.set_timesteps(num_steps)
    F_ = latents.shape[2]
    cache = {}
    cfg = guidance_scale > 1.0
    nb = 2 if cfg else 1
    for t in timesteps:
        s_t = pag_scale_at(pag_scale, pag_adaptive_scale, t) if pag_scale > 0 else 0.0
        if on_pag is not None:
            on_pag(int(t), s_t)
        noise_pred = torch.zeros((nb,) + tuple(latents.shape[1:]), dtype=latents.dtype, device=latents.device)
        pert = torch.zeros((1,) + tuple(latents.shape[1:]), dtype=latents.dtype, device=latents.device)
        counter = torch.zeros((1, 1, F_, 1, 1), dtype=latents.dtype, device=latents.device)
        windows = FR.make_windows(schedule, F_, context_frames, context_stride, context_overlap, num_steps)
        wts = FR.shares(windows, F_) if fuse == "pyramid" else None
        for wi, win in enumerate(windows):
            f = len(win)
            x = latents[:, :, win].repeat(nb, 1, 1, 1, 1)
            if wi not in cache:
                g = ref_latents[0, win]
                ctx = torch.stack([embeds[(f + j) % 2] for j in range(f)]) if cfg else embeds[:1].repeat(f, 1, 1)
                b_, _ = O.reference_unet_forward(ref_sd, g, ctx)
                cache[wi] = {k: v.half().to(latents.dtype) for k, v in b_.items()}
            cond = cache[wi]
            banks = {k: torch.cat([torch.zeros_like(v), v]) for k, v in cond.items()} if cfg else cond
            preds = [(noise_pred, O.denoising_unet_forward(den_sd, x, t, embeds[:nb], banks, cfg=cfg), True)]
            if s_t > 0:
                preds.append((pert, perturbed_forward(den_sd, x[nb - 1:], t, embeds[nb - 1:nb], cond, pag_layers), False))
            for acc, pred, count in preds:
                if wts is not None:
                    sl = FR.slots(win)
                    js = [j for j, fr in enumerate(sl) if fr >= 0]
                    frs = [sl[j] for j in js]
                    w = wts[wi][js].to(device=pred.device, dtype=pred.dtype).view(1, 1, -1, 1, 1)
                    acc[:, :, frs] = acc[:, :, frs] + w * pred[:, :, js]
                    if count:
                        counter[:, :, frs] = counter[:, :, frs] + w
                else:                                                        # duplicate frames: the LAST occurrence lands (as the oracle)
                    last = {fr: j for j, fr in enumerate(win)}
                    frs, js = list(last.keys()), list(last.values())
                    acc[:, :, frs] = acc[:, :, frs] + pred[:, :, js]
                    if count:
                        counter[:, :, frs] = counter[:, :, frs] + 1
        if cfg:
            u, c = (noise_pred / counter).chunk(2)
            v = combine(u, c, pert / counter, guidance_scale, s_t) if s_t > 0 else u + guidance_scale * (c - u)
        else:
            v = combine_sum(noise_pred, pert, s_t) if s_t > 0 else noise_pred
        z = None
        if eta > 0:
            gdev = generator.device if generator is not None else latents.device
            z = torch.randn(latents.shape, generator=generator, device=gdev, dtype=noise_dtype or latents.dtype).to(latents)
        latents = sch.step(v, t, latents, eta=eta, noise=z)
        if on_step is not None:
            on_step(int(t), latents)
    return latents


# ------------------------------------------------------------------ the two operators, emulated like tests/fake_ops.py emulates the others
# fp32 arithmetic on the (ftot, hw, 4) layout, one rounding of the latents.  The update itself is fake_ops' own step emulation run on the
# PAG-guided v (its one-clip-half form takes v as it is), so there is one restatement of each scheduler update.
NAMES = ("cfg_ddim_step_pag", "cfg_multistep_step_pag")


def step_calls():
    """(name, record) of every operator so far whose name starts with cfg_, the two above included, in call order."""
    return [(n, d) for n, d in fake_ops.CALLS if n.startswith("cfg_")]


def _v(noise_sum, counter, perturbed_sum, ftot, hw, guidance, pag_scale, halves):
    assert noise_sum.dtype == perturbed_sum.dtype == torch.float32 and noise_sum.numel() == halves * ftot * hw * 4 and perturbed_sum.numel() == ftot * hw * 4
    ns = noise_sum.view(halves, ftot, hw, 4)
    v, _ = fake_ops._guided(ns, counter, guidance, halves)
    d = ns[halves - 1] - perturbed_sum.view(ftot, hw, 4)
    if halves == 2:
        d = d / counter.view(-1, 1, 1)
    return v + torch.tensor(pag_scale, dtype=torch.float32) * d


def cfg_ddim_step_pag(latents, noise_sum, counter, perturbed_sum, ftot, hw, guidance, pag_scale, alpha_t, alpha_prev, halves=2, eta=0.0,
                      variance_noise=None):
    v = _v(noise_sum, counter, perturbed_sum, ftot, hw, guidance, pag_scale, halves)
    n = len(fake_ops.CALLS)
    fake_ops.cfg_ddim_step(latents, v[None], None, ftot, hw, guidance, alpha_t, alpha_prev, halves=1, eta=eta, variance_noise=variance_noise)
    del fake_ops.CALLS[n:]
    fake_ops._log("cfg_ddim_step_pag", dict(variance_noise=variance_noise), ftot=ftot, hw=hw, halves=halves, guidance=guidance, pag_scale=pag_scale,
                  alpha_t=alpha_t, alpha_prev=alpha_prev, eta=eta)


def cfg_multistep_step_pag(latents, noise_sum, counter, history, perturbed_sum, ftot, hw, guidance, pag_scale, alpha_s, sigma_s, c_x, c_m0, c_m1,
                           c_z, halves=2, variance_noise=None):
    v = _v(noise_sum, counter, perturbed_sum, ftot, hw, guidance, pag_scale, halves)
    n = len(fake_ops.CALLS)
    fake_ops.cfg_multistep_step(latents, v[None], None, history, ftot, hw, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z, halves=1,
                                variance_noise=variance_noise)
    del fake_ops.CALLS[n:]
    fake_ops._log("cfg_multistep_step_pag", dict(variance_noise=variance_noise), ftot=ftot, hw=hw, halves=halves, guidance=guidance,
                  pag_scale=pag_scale, alpha_s=alpha_s, sigma_s=sigma_s, c_x=c_x, c_m0=c_m0, c_m1=c_m1, c_z=c_z)
