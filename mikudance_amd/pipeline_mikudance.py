"""MikuDanceVideoPipeline -- API mirror of reference src/pipelines/pipeline_mikudance.py:36-704 whose denoising
loop (:573-686) runs on the MI355X-native UNets / HIP kernels of this package.

`__call__` keeps the reference signature and call order (CLIP embed -> VAE-encode every condition image -> 22-channel
guidance tensor -> loop -> VAE decode).  The VAE and the CLIP vision tower are whatever modules the caller passes
(`vae.encode(x).latent_dist.mean`, `vae.decode(z).sample`, `image_encoder(...)`) exactly as in the reference --
mikudance_amd.AutoencoderKL / mikudance_amd.CLIPVisionModelWithProjection run them on the same HIP kernels.  `denoise()` is the hot path itself on
tensors and is what bench.py and the parity tests drive.

Result-preserving reductions (proven identical on the CPU oracle in tests/test_oracle.py):
  * the reference UNet's inputs and t == 0 are step-invariant -> it is evaluated ONCE per window, not once per step;
  * only the conditional half of its banks is ever consumed -> it is evaluated on the f conditional frames only,
    each with the context row the reference's `[u,c,u,c,...]` interleaving would have given it;
  * the sample after its last bank write is discarded -> that tail is skipped;
  * unconditional rows ignore the bank -> one attention pass with a per-row K/V source replaces two.
`reference_reuse=False` restores the literal per-step evaluation (same results, for A/B timing).
"""
import contextlib
import math
import os
from dataclasses import dataclass, replace
from typing import Callable, List, NamedTuple, Optional, Union

import numpy as np
import torch

from . import free_init, ops
from .context import get_context_scheduler
from .mutual_mix_attention import ReferenceAttentionControl
from .windows import accumulate_slots, fuse_weights


# ---- latent interpolation helpers: API mirror of reference src/pipelines/utils.py (a module-level method switch that the
# caller sets; nothing in the reference sets it, so interpolation_factor >= 2 without it fails there exactly like here)
tensor_interpolation = None


def get_tensor_interpolation_method():
    return tensor_interpolation


def set_tensor_interpolation_method(is_slerp):
    global tensor_interpolation
    tensor_interpolation = slerp if is_slerp else linear


def linear(v1, v2, t):
    return (1.0 - t) * v1 + t * v2


def slerp(v0, v1, t, DOT_THRESHOLD=0.9995):
    """Spherical interpolation of two latent frames treated as single vectors (src/pipelines/utils.py:20-31); falls back to
    the straight line when they are nearly parallel."""
    u0 = v0 / v0.norm()
    u1 = v1 / v1.norm()
    dot = (u0 * u1).sum()
    if dot.abs() > DOT_THRESHOLD:
        return (1.0 - t) * v0 + t * v1
    omega = dot.acos()
    return (((1.0 - t) * omega).sin() * v0 + (t * omega).sin() * v1) / omega.sin()


@dataclass
class MikuDanceVideoPipelineOutput:
    videos: Union[torch.Tensor, np.ndarray]


# ---- the sampling plan: what denoise()'s keywords resolve to, once every refusal has been made (MikuDanceVideoPipeline.sampling_plan).
# The step forms its v in exactly one way -- plain, or one of:
#   Rescale  v * (1 - phi + phi std(c) / std(v)): md_cfg_guidance_rescale, then the step with vscale=
#   APG      adaptive projected guidance: md_cfg_apg_prepare, then md_cfg_*_step_apg
#   Perturb  a second, perturbed conditional evaluation p of the selected `blocks` (layer names until _resolve_plan has asked the UNet) and
#            v + s_t (c - p) through md_cfg_*_step_pag: PAG (kind "identity", the scale decaying by `adaptive` per timestep, sigma None) or
#            SEG (kind "blur" with `sigma` in tokens, adaptive 0)
Rescale = NamedTuple("Rescale", [("phi", float)])
APG = NamedTuple("APG", [("momentum", float), ("eta", float), ("threshold", float)])
Perturb = NamedTuple("Perturb", [("kind", str), ("scale", float), ("adaptive", float), ("blocks", tuple), ("sigma", Optional[float])])


@dataclass(frozen=True)
class SamplingPlan:
    fuse: str                  # "flat" | "pyramid"
    free_init: tuple           # (iters, filter, order, spatial_stop, temporal_stop, fast)
    strength: float
    kv: Union[None, tuple, dict]   # None: no K / V downsampling; (factors, mode), resolved: UNet3DConditionModel.kv_downsample_plan
    guide: Union[None, Rescale, APG, Perturb]      # None: plain (u + g (c - u), or c without CFG)
    tile: Union[None, tuple] = None                # None: no tiled self-attention; (factors, shift), resolved: (UNet3DConditionModel.tile_attention_plan, shift)
    deep: Union[None, tuple] = None                # None: deep_cache_interval == 1, no DeepCache; (interval N, depth d), d checked against the UNet by _resolve_plan
    uncond: Union[None, tuple] = None              # None: guidance on every step from a full evaluation (the defaults, or no CFG); (lo, hi, n) of guidance_interval / uncond_cache_interval
    deep_threshold: Optional[float] = None         # None: DeepCache's fixed rule (a key step every N-th step); a float > 0: the adaptive rule, N the cap
    sampler: str = "ddim"                          # which step the loop calls: "ddim" (md_cfg_ddim_step*), "dpm" (md_cfg_multistep_step*) or "unipc" (md_cfg_unipc_step*)


# the step forms v in ONE way: (asked for, beside, why not), in the order the refusals are made
_ONE_GUIDE = (("apg=True", "guidance_rescale > 0", "the rescale would need a second statistics pass over APG's guided output"),
              ("pag_scale > 0", "guidance_rescale > 0", "the rescale would need its statistics taken over the PAG-guided output"),
              ("pag_scale > 0", "apg=True", "APG's statistics would have to be taken over the PAG-guided output"),
              ("seg_scale > 0", "pag_scale > 0", "the loop carries one perturbed plane"),
              ("seg_scale > 0", "guidance_rescale > 0", "the rescale would need its statistics taken over the SEG-guided output"),
              ("seg_scale > 0", "apg=True", "APG's statistics would have to be taken over the SEG-guided output"))


def _pil_to_tensor(img, height, width, normalize):
    """VaeImageProcessor(do_convert_rgb=True[, do_normalize]).preprocess for one PIL image -> (1,3,H,W) fp32."""
    from PIL import Image
    img = img.convert("RGB").resize((width, height), resample=Image.LANCZOS)
    arr = torch.from_numpy(np.asarray(img).astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    return arr * 2.0 - 1.0 if normalize else arr


class MikuDanceVideoPipeline:
    _optional_components = []
    default_context_frames = 30

    def __init__(self, vae, image_encoder, reference_unet, denoising_unet, scheduler, image_proj_model=None, tokenizer=None,
                 text_encoder=None, video_decoder=False):
        self.vae, self.image_encoder = vae, image_encoder
        self.reference_unet, self.denoising_unet, self.scheduler = reference_unet, denoising_unet, scheduler
        self.image_proj_model, self.tokenizer, self.text_encoder = image_proj_model, tokenizer, text_encoder
        self.video_decoder = video_decoder
        self.decode_chunk_size = 16                                          # reference :81
        self.vae_scale_factor = 8
        self.vae_batch = 8                                                   # images per VAE call (the reference: 1)
        self.reference_reuse = True
        self.share_first_layers = True                                       # denoising UNet: conv_in + first resnet once for both CFG halves
        # ... and, behind them, OPTIONALLY the unconditional and the conditional half as two kernel queues (UNet3DConditionModel._two_queues;
        # needs share_first_layers; pipe.two_queues = True or MD_TWO_QUEUES=1).  Off by default: on MI355X two queues of B = f kernels finish 7 % sooner
        # than the same launches back to back, but one queue of B = 2f kernels is already that much more efficient -- +0.2-0.35 % end to end
        # (profiles/r06_ab_two_queue_halves.log): measured, validated (tests/test_two_queues_gpu.py), not worth a second evaluation order by default
        self.two_queues = os.environ.get("MD_TWO_QUEUES", "0") == "1"
        self._device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")

    # ------------------------------------------------------------------------------------------ plumbing
    def to(self, device=None, dtype=None):
        for m in (self.vae, self.image_encoder, self.reference_unet, self.denoising_unet):
            if m is not None and hasattr(m, "to"):
                m.to(device=device, dtype=dtype) if dtype is not None else m.to(device)
        if device is not None:
            self._device = torch.device(device)
        return self

    @property
    def _execution_device(self):
        return self._device

    # ---- VAE tiling / slicing: diffusers' pipeline-level names, forwarded to the VAE (AutoencoderKL.enable_tiling / enable_slicing)
    def enable_vae_tiling(self):
        self.vae.enable_tiling()

    def disable_vae_tiling(self):
        self.vae.disable_tiling()

    def enable_vae_slicing(self):
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        self.vae.disable_slicing()

    @contextlib.contextmanager
    def vae_tiling_scope(self, sizes, vae_tiling=False, vae_tile_size=None):
        """__call__'s vae_tiling= / vae_tile_size=: checks them against the (height, width) pairs in `sizes` -- every image size the call
        encodes and decodes at -- and holds the VAE's tiling state for the duration of the `with` block; the state the VAE had comes back
        afterwards.  With the defaults the VAE's state is not changed (whatever enable_vae_tiling() set stays in force, and its tile grid
        is checked here all the same).  ValueError, before
        the block runs, for a vae_tiling that is no bool, a vae_tile_size that is no positive multiple of 32 or comes without tiling, a VAE
        without tiling (the temporal decoder) and a tile grid the VAE's operators cannot run (AutoencoderKL.tile_grid names the tile)."""
        if not isinstance(vae_tiling, bool):
            raise ValueError(f"vae_tiling must be True or False, got {vae_tiling!r}")
        vae = self.vae
        if not vae_tiling and vae_tile_size is None and not (getattr(vae, "use_tiling", False) and hasattr(vae, "tile_grid")):
            yield
            return
        if not all(hasattr(vae, a) for a in ("enable_tiling", "set_tile_size", "tile_grid")):
            raise ValueError(f"vae_tiling / vae_tile_size: {type(vae).__name__} has no tiling (AutoencoderKL has; the temporal decoder has none)")
        if not (vae_tiling or vae.use_tiling):
            raise ValueError(f"vae_tile_size={vae_tile_size!r} needs vae_tiling=True (or enable_vae_tiling())")
        saved = (vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size)
        try:
            if vae_tile_size is not None:
                vae.set_tile_size(vae_tile_size)
            vae.enable_tiling(vae_tiling or vae.use_tiling)
            for h, w in sizes:
                if max(h, w) > vae.tile_sample_min_size:
                    vae.tile_grid(h, w, encode=True)
                if max(h, w) // self.vae_scale_factor > vae.tile_latent_min_size:
                    vae.tile_grid(h // self.vae_scale_factor, w // self.vae_scale_factor, encode=False)
            yield
        finally:
            vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size = saved

    def progress_bar(self, iterable=None, total=None):
        from tqdm import tqdm
        return tqdm(iterable, total=total, disable=getattr(self, "_progress_disabled", True))

    def prepare_latents(self, batch_size, num_channels_latents, width, height, video_length, dtype, device, generator,
                        latents=None):
        """reference :173-207 -- noise is drawn from the caller's generator on ITS device (CPU for the script's
        torch.manual_seed generator, quirk 11), then moved."""
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            gdev = generator.device if generator is not None and not isinstance(generator, list) else torch.device("cpu")
            latents = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
        else:
            latents = latents.to(device)
        return latents * self.scheduler.init_noise_sigma

    # ------------------------------------------------------------------------------------------ the hot path
    @torch.no_grad()
    def denoise(self, latents, ref_latents, image_prompt_embeds, num_inference_steps, guidance_scale, context_schedule="uniform",
                context_frames=None, context_stride=1, context_overlap=8, callback=None, callback_steps=1, eta=0.0, generator=None,
                window_parallel=None, guidance_rescale=0.0, init_latents=None, strength=1.0, context_fuse="flat", free_init_iters=1,
                free_init_filter="butterworth", free_init_order=4, free_init_spatial_stop=0.25, free_init_temporal_stop=0.25,
                free_init_fast=False, apg=False, apg_eta=0.0, apg_norm_threshold=0.0, apg_momentum=0.0, pag_scale=0.0, pag_adaptive_scale=0.0,
                pag_applied_layers=("mid",), kv_downsample=1, kv_downsample_mode="nearest", seg_scale=0.0, seg_blur_sigma=100.0,
                seg_applied_layers=("mid",), tile_attention=1, tile_attention_shift="cycle", deep_cache_interval=1, deep_cache_depth=3,
                guidance_interval=(0.0, 1.0), uncond_cache_interval=1, deep_cache_threshold=None):
        """The loop of reference src/pipelines/pipeline_mikudance.py:573-686.

        latents             (1, 4, F, h, w)  initial noise (any float dtype, on the GPU)
        ref_latents         (1, F, 22, h, w) 20 VAE-latent guidance channels + 2 scene-motion channels
        image_prompt_embeds (2, L, D) = [zeros, CLIP tokens] when guidance_scale > 1, else (1, L, D)
        scheduler           self.scheduler: DDIMScheduler (md_cfg_ddim_step), DPMSolverMultistepScheduler (md_cfg_multistep_step with a
                            fp32 data-prediction history of (F, h*w, 4) for this call; its SDE variant draws z every step like eta below) or
                            UniPCMultistepScheduler (md_cfg_unipc_step: the corrector of the last step and the predictor of this one in one
                            launch per step, on a fp32 state of (4, F, h*w, 4) for this call -- the corrected sample and three data
                            predictions; two denoise() calls, as under hires_scale, have a state each.  The state starts over with every
                            FreeInit pass and at a video-to-video start: the first row of a schedule reads none of it, so it is allocated
                            uninitialised and never cleared.  Every guide, approximation, window schedule and fuse mode acts in front of the
                            step and composes with it; under window_parallel the step and its state are replicated on every rank.  eta > 0 is
                            refused with it: UniPC has no stochastic variant here)
        eta, generator      DDIM's stochastic variant (reference :152-171 -> scheduler.step(eta=, generator=)): one N(0, 1) draw of
                            the latents' shape and dtype per step from `generator` (on ITS device, like diffusers' randn_tensor).
                            The kernels compute in fp16: the draw is ROUNDED TO fp16 on its way into md_cfg_ddim_step_eta, so an
                            fp32-dtype caller does not get a noise stream bit-comparable with an fp32 reference run
        window_parallel     mikudance_amd.dp.WindowParallel or None: the context windows of a step (:625-668, independent UNet evaluations)
                            are shared out over the ranks of a process group, ONE all_reduce(sum) of the per-frame accumulators per step
                            (:662-674) and the CFG + DDIM update replicated on every rank; every rank returns the full latents
        guidance_rescale    phi of rescaled classifier-free guidance (Lin et al., arXiv 2305.08891 section 3.4; diffusers `guidance_rescale` /
                            rescale_noise_cfg), finite, in [0, 1], applied only under CFG (guidance_scale > 1): every step, after all windows
                            (and the all_reduce) have accumulated, md_cfg_guidance_rescale takes std(c) and std(v) over the whole clip on the
                            device and the step runs on v * (1 - phi + phi std(c) / std(v)) (md_cfg_*_step_scaled; a clip with std(v) == 0
                            keeps v unscaled, where diffusers divides by zero).  0.0 (the default) calls the unscaled entry points: the
                            output is bitwise that of a call without the keyword
        init_latents        video-to-video (diffusers img2img / video2video `strength`): a clean VAE latent of latents' shape, already scaled by
                            0.18215.  The loop starts at the first timestep kept by scheduler.get_timesteps(num_inference_steps, strength)
                            from md_add_noise_f16(x0 = init_latents, noise = latents) and runs the kept steps only (callback's step_i counts
                            them from 0; DPM-Solver++ starts first order there, set_begin_index).  No new collective or host sync per step.
                            strength 1.0 starts at t = 999 where abar = 0: bitwise the plain loop, whatever init_latents holds
        strength            finite, in (0, 1]; < 1 needs init_latents.  None of it is read without init_latents
        context_schedule    "uniform" (the reference's windows: every schedule a closed loop, windows wrap round the end of the clip) or
                            "uniform_open" (windows.WindowLayout.open_windows: the same levels and advance, no window wraps, the last one of
                            a level ends on the last frame; fewer windows for the same clip)
        context_fuse        how the predictions of overlapping windows are merged per frame: "flat" (the reference: every window counts the
                            same, md_window_accumulate) or "pyramid" (slot j of an L-frame window weighs min(j + 1, L - j), diffusers'
                            FreeNoise pyramid; normalised per frame over ALL windows of the step on the host, windows.fuse_weights, and
                            accumulated by md_window_accumulate_weighted, so the buffers hold the weighted mean and a counter of 1 and every
                            step kernel, the guidance rescale and window_parallel's all-reduce work on them unchanged).  One difference:
                            WITHOUT classifier-free guidance the reference, and "flat", hand the scheduler the window SUM
                            (src/pipelines/pipeline_mikudance.py:670-674 divides under CFG only); "pyramid" always hands it the mean.
                            "flat" is bitwise the loop without the keyword; a clip of one window is the same bits under both
        free_init_iters     FreeInit (Wu et al., arXiv 2312.07537; diffusers enable_free_init): n >= 1 sampling passes.  Pass 0 is the loop as
                            it is.  Before every further pass one z ~ N(0, 1) is drawn (the pass's first draw, ahead of any eta / SDE draw)
                            and md_free_init_mix_f16 replaces the latents by the low spatio-temporal frequencies of the result re-noised
                            to the last training timestep (sqrt(abar_T) x + sqrt(1 - abar_T) noise0, noise0 = the `latents` passed in) plus
                            the high frequencies of z; then the loop runs again from its first timestep (set_timesteps per pass, so
                            DPM-Solver++ starts first order again; the reference-UNet banks are kept: they do not depend on the latents).
                            callback's step_i counts from 0 in every pass.  Under window_parallel the mix is replicated on every rank (seed
                            the ranks' generators alike, as for eta); no new collective.  Not with init_latents: re-noising to T discards
                            what strength means.  1 (the default) is bitwise the loop without the keyword and makes no new operator call
        free_init_filter    "butterworth" | "gaussian" | "ideal", with free_init_order (butterworth), free_init_spatial_stop and
                            free_init_temporal_stop (normalised stop frequencies): diffusers' low-pass table, free_init.freq_filter
        free_init_fast      diffusers' use_fast_sampling: pass i runs max(1, int(N / n * (i + 1))) steps instead of N
        apg                 adaptive projected guidance (Sadat, Hilliges, Weber, arXiv 2410.02416, Algorithm 1; diffusers
                            AdaptiveProjectedGuidance) in place of u + g (c - u), under CFG only (guidance_scale > 1).  Every step, after all
                            windows (and the all_reduce) have accumulated, md_cfg_apg_prepare forms on the DATA prediction, with a = sqrt(abar_t),
                            s = sqrt(1 - abar_t): D_c = a x - s c and the update m = s (u - c) + apg_momentum m_prev (= D_c - D_u plus the
                            running average, one fp32 (F, h*w, 4) buffer per call, zeroed at the start of the loop and of every FreeInit pass;
                            under window_parallel every rank keeps its own identical copy, no new collective), then PER FRAME over that
                            frame's h*w*4 elements S = min(1, apg_norm_threshold / ||m||) (1 when the threshold or ||m|| is 0) and
                            proj = <m, D_c> / <D_c, D_c> (0 when D_c is 0); the step (md_cfg_*_step_apg) runs on
                            v_g = c - (g - 1) (S m - (1 - apg_eta) S proj D_c) / s, i.e. D_g = D_c + (g - 1) (orthogonal + apg_eta * parallel
                            part of the capped update).  One departure from diffusers, which takes the norm and the projection over every
                            non-batch dimension and so over the whole clip: here each frame is one sample of the paper, so
                            apg_norm_threshold does not depend on the clip's length or the window layout.  The paper's settings (eta = 0, a
                            negative momentum, a threshold chosen per model) are the paper's; nothing here validates image quality.  Works with
                            every sampler, eta, init_latents / strength, window schedule and fuse mode; not with guidance_rescale > 0 (that
                            would need a second statistics pass over v_g).  False (the default) is bitwise the loop without the keywords and
                            makes no new operator call
        apg_eta             finite, in [0, 1]: the weight of the part of the update parallel to D_c (1 keeps it, 0 removes it)
        apg_norm_threshold  finite, >= 0: the cap on the per-frame norm of the update; 0 = no cap
        apg_momentum        finite, in (-1, 1): beta of the running average over steps (the paper uses a negative value); with
                            apg_eta = 1, apg_norm_threshold = 0, apg_momentum = 0 the result is u + g (c - u) up to rounding
        pag_scale           perturbed-attention guidance (Ahn et al., arXiv 2403.17377; diffusers PAGMixin / AnimateDiffPAGPipeline), finite, >= 0.
                            Every step and every window the denoising UNet is evaluated once more on the window's conditional frames (CLIP
                            tokens, every row reads the reference bank) with the self-attention map of the blocks pag_applied_layers selects
                            replaced by the identity, attn1(x) = to_out(to_v(norm1(x) + bank)) + x (no q, no k, no attention launch there;
                            cross-attention, feed-forward and the motion modules are never perturbed; the reference UNet and the bank cache
                            do not depend on it).  That prediction p is accumulated over the windows into one more plane of the fp32
                            accumulator, with the same window weights (under window_parallel the rank that owns a window evaluates both
                            of its branches and the one all_reduce carries the plane; no new collective), and the step (md_cfg_*_step_pag)
                            runs on v + s_t (c - p): under CFG diffusers' u + g (c - u) + s (c - p), without CFG c + s (c - p) on what the
                            loop hands the scheduler (the window sum for "flat", see context_fuse).  Works with both samplers, eta / SDE
                            noise, init_latents / strength, every window schedule and fuse mode, FreeInit (every pass) and window_parallel;
                            not with guidance_rescale > 0 and not with apg=True (each would need its statistics taken over the PAG-guided
                            v).  Costs one conditional clip-half per window and step, less the self-attention of the selected blocks.
                            0.0 (the default) is bitwise the loop without the keywords, makes no new operator call and allocates no buffer
        pag_adaptive_scale  finite, >= 0: diffusers' _get_pag_scale, s_t = max(pag_scale - pag_adaptive_scale (1000 - t), 0) per step on the
                            host; at a step with s_t == 0 the perturbed evaluation is skipped and the plain step entry runs.  0.0: no decay
        pag_applied_layers  names of the denoising UNet's attention blocks, checkpoint-key prefixes: "mid_block" (alias "mid"),
                            "down_blocks.I", "up_blocks.I", "down_blocks.I.attentions.J", "up_blocks.I.attentions.J"; a block is selected
                            when its key prefix equals a name or starts with name + ".".  An empty sequence (with pag_scale > 0) and a
                            name that selects no block raise ValueError
        kv_downsample       K / V token downsampling in the spatial self-attention of the denoising UNet (ToDo: Token Downsampling, Smith et al.,
                            arXiv 2402.13573), an opt-in APPROXIMATION that trades accuracy for time at high resolution: an integer factor 1..8
                            per resolution level from the highest down (an int n stands for (n,); level i = down_blocks.i and the up block of
                            the same resolution, the last level also mid_block; missing levels and 1 = untouched).  At a level with factor s,
                            Q keeps every token while to_k / to_v read the token grid reduced by s per axis (ops.token_pool, after the
                            reference bank has been added), so that level's attention FLOPs and K / V projection rows fall by s^2; the
                            price is one pass over the K / V source and a q-only GEMM where the plain path fuses q|k.  The reference UNet, its
                            banks (full resolution), cross-attention and the motion modules are untouched; with PAG the unselected blocks of
                            the perturbed evaluation pool like the main one.  Sits inside the UNet: works with every sampler, eta, init_latents,
                            window schedule, fuse mode, FreeInit, APG, PAG, guidance_rescale, window_parallel and two_queues.  ValueError, before
                            anything runs, for other values, more factors than levels, a level without attention, or a factor that leaves a
                            level of THIS latent size without a single s x s block (levels halve with ceil).  1 (the default) and all ones:
                            bitwise the loop without the keyword, no new operator call
        kv_downsample_mode  "nearest" (the paper's: the token at the top-left of each s x s block, F.interpolate nearest) or "mean" (the block's
                            mean, F.avg_pool2d)
        seg_scale           smoothed-energy guidance (SEG; Hong, arXiv 2408.00760), finite, >= 0.  With seg_scale > 0 every window of every step
                            gets one more evaluation of the denoising UNet on the conditional frames, PAG's perturbed evaluation with a
                            tunable perturbation: in the blocks seg_applied_layers selects the self-attention QUERIES are Gaussian-blurred
                            over the block's own token grid (ops.token_blur on the q-only GEMM's output; K and V unblurred), so the map
                            stays a softmax of real energies, only flatter.  Its prediction p is PAG's extra plane of the accumulator and
                            the step is PAG's: v + seg_scale (c - p) through md_cfg_*_step_pag, with or without CFG; no new step kernel.
                            Works with every sampler, eta, init_latents, window schedule, fuse mode, FreeInit, kv_downsample and
                            window_parallel.  ValueError, before anything runs, together with pag_scale > 0 (there is one perturbed
                            plane), guidance_rescale > 0 or apg=True (PAG's reasons).  0.0 (the default): exactly the loop without the
                            keywords, no new operator call
        seg_blur_sigma      the blur's sigma in tokens: a finite number > 0 (taps ceil(6 sigma) rounded up to odd, clamped to the grid, reflect
                            padding: the official implementation's gaussian_blur_2d, per axis) or math.inf (every query becomes its frame's mean
                            query: the official inf_blur).  100.0, the paper's default, spans every grid of a 768 x 768 clip
        seg_applied_layers  as pag_applied_layers
        tile_attention      shifted-tile self-attention in the spatial self-attention of the denoising UNet (MSW-MSA of HiDiffusion, Zhang et al.,
                            arXiv 2311.17528), an opt-in APPROXIMATION that trades accuracy for time at high resolution: an integer factor 1..8
                            per resolution level from the highest down (levels as kv_downsample; missing levels and 1 = untouched).  At a level
                            with factor t every frame's token grid is cut into t x t tiles and attention runs inside each tile at full key
                            resolution (ops.token_tile / ops.token_untile round the existing attention entry, B t^2 batch items of L / t^2
                            tokens), so that level's attention FLOPs fall by t^2; the price is three reorder passes per block that reads the
                            bank, two otherwise.  The reference UNet, its banks, cross-attention and the motion modules are untouched; the main
                            evaluation and PAG's / SEG's perturbed evaluation of a step use the same plan and shift (SEG blurs over the whole
                            frame, then tiles; an identity-map block of PAG has no attention to tile).  With kv_downsample on the same level
                            the pooling runs inside each tile.  The wrap-around of a shifted tile is not masked (the paper's code does not
                            mask it either): on shifted steps tokens of opposite frame edges may share a tile.  Sits inside the UNet: works
                            with both samplers, eta, init_latents, every window schedule and fuse mode, FreeInit, every guide, kv_downsample,
                            window_parallel and two_queues.  ValueError, before anything runs, for other values, more factors than levels, a
                            level without attention, a factor that does not divide both sides of its level's grid for THIS latent size
                            (levels halve with ceil), or tiles smaller than that level's kv_downsample factor.  Image quality on real
                            weights has not been assessed.  1 (the default) and all ones: bitwise the loop without the keyword, no new
                            operator call, no buffer, no new keyword to forward_nhwc
        tile_attention_shift  "cycle" (default): at step index k = t_start + step_i (video-to-video keeps the shifts of the steps it keeps; every
                            FreeInit pass starts over), q = k mod 4 and a level whose tiles hold th x tw tokens shifts its tiling by
                            (q th // 4, q tw // 4), so no tile border stays put; "none": no shift.  The paper's code draws the shift at random
                            per call; here it is a pure function of the step, so that runs are reproducible and the ranks of window_parallel
                            agree without talking
        deep_cache_interval DeepCache (Ma, Fang, Wang, arXiv 2312.00858: the idea only), an opt-in APPROXIMATION that trades accuracy for time: an integer
                            N >= 1.  Executed step k of a pass (k counts from 0 at the first step the loop actually runs: the first KEPT step under
                            strength < 1; every FreeInit pass starts at k = 0 with an empty cache) is a KEY step iff k % N == 0: the denoising UNet
                            is evaluated in full and keeps the hidden state that meets skip deep_cache_depth - 1 on its up path.  Every other step
                            is a SHALLOW step: the UNet runs its outermost layers only (unet_3d_mix.DeepCacheSlot says which) on the
                            current latents, time rows, context and banks, and takes the deep hidden state of the last key step.  No new kernel
                            and no copy: every launch of a shallow step is one the full step makes at the same shape, and the cache is the
                            concat buffer of skip deep_cache_depth - 1, kept.  One slot per (window of the step, plane), the planes being the main
                            evaluation and PAG's / SEG's perturbed one (its scale only falls with t, so a perturbed evaluation that finds no
                            slot is at a key step and fills it; asserted).  The window list is the same at every step of the loop (the window
                            scheduler is called once, with step index 0: see the note on context_schedule below), so a shallow
                            step meets the frames its key step cached, and under window_parallel the window-to-rank assignment is fixed: slots
                            stay rank-local, no new collective.  Slots are dropped at the end of denoise() and between FreeInit passes.
                            Memory per slot: one (nb f, H, W, C1 + Cs) fp16 buffer of skip deep_cache_depth - 1, 566 MB per window at 768 x 768,
                            16 frames, CFG, depth 3 (32 x 96 x 96 x 960 x 2 bytes), half of that for a perturbed plane.  kv_downsample,
                            tile_attention (its shift stays a function of the step), every guide, sampler, eta, init_latents, fuse mode, two_queues
                            and share_first_layers act on the layers that run.  Image quality on real weights has not been assessed.  1 (the
                            default): bitwise the loop without the keyword, the same operator calls, no cache allocated, nothing kept
        deep_cache_depth    d >= 1, this project's own index (the mapping to DeepCache's cache_branch_id is not asserted): skip tensors are counted
                            in production order -- conv_in, down_blocks.0 layer 0, layer 1, its downsampler, down_blocks.1 layer 0, ... -- and a
                            shallow step runs conv_in, the first d - 1 of those operators and the last d up-block layers; d must be smaller
                            than the number of skips (12).  3 (the default): all of the highest-resolution level on both sides.  Checked even
                            when deep_cache_interval is 1
                            Long clips, A STATED DEVIATION: the "uniform" / "uniform_open" window list is a function of a step index, and a cache
                            keyed by window would meet other frames if a shallow step used another index than its key step.  With N > 1 the
                            list of a whole cache period is therefore the key step's.  This loop calls the window scheduler once, with index 0,
                            for every step (as the oracle does), so that holds by construction; a loop that moved its windows per step
                            would have to hold them still over each period
        deep_cache_threshold  None (the default): DeepCache's fixed rule above, bitwise what it is without the keyword: the same operator calls,
                            nothing allocated.  A number > 0: ADAPTIVE DeepCache, the accumulated relative-L1 rule of TeaCache (arXiv 2411.19108)
                            on the "first block output" of first-block cache, which here is skip deep_cache_depth - 1: a shallow step computes
                            it from the current latents anyway.  Needs deep_cache_interval >= 2, which becomes the CAP: at most N - 1 shallow
                            steps in a row.  Every evaluation behind the first of a pass is an auto call (unet_3d_mix.DeepCacheSlot.auto): it
                            runs the shallow part of the down path into a fresh buffer, ops.rel_l1 (md_rel_l1_f16, deterministic) gives
                            r = sum |skip - skip of the step before| / sum |skip of the step before|, the host reads it -- ONE host
                            synchronisation per UNet call, which the fixed rule does not have -- and adds it to the slot's accumulator; the
                            call goes on as a key step iff the accumulator has reached the threshold, N calls have been made since the last
                            key step, r is not finite or its denominator is 0, and resets the accumulator then; otherwise as a shallow step,
                            after one copy of one channel slice.  math.inf: the cap alone decides, bitwise deep_cache_interval's fixed rule.
                            The first step of every pass (FreeInit, each pass of hires_scale) is a key step.  One accumulator per (window,
                            plane) slot: PAG's / SEG's plane decides on its own, and so does every window -- decisions are local, so
                            window_parallel needs no new collective.  Composes with what deep_cache_interval > 1 composes with, two_queues
                            included (one distance per clip-half queue, summed before the division).  ValueError, before anything runs, for
                            zero, a negative number, NaN, a value that is no number, deep_cache_interval < 2, and together with
                            guidance_interval / uncond_cache_interval.  self.last_deep_cache_trace lists what every evaluation of the last
                            denoise() did, (step_i, window, plane, "key" | "shallow", r), step_i counting from 0 in every pass, on this rank;
                            under the fixed rule r is None; None when DeepCache is off.  Image quality on real weights has not been assessed
        guidance_interval   (lo, hi), two finite numbers with 0 <= lo <= hi <= 1 (Kynkaanniemi et al., "Applying Guidance in a Limited Interval",
                            arXiv 2404.07724; the start / stop of diffusers' ClassifierFreeGuidance guider), an opt-in APPROXIMATION that trades
                            accuracy for time: classifier-free guidance is applied at schedule index k = t_start + step_i (video-to-video keeps the
                            indices of the steps it keeps; every FreeInit pass counts from 0, against the number of steps of ITS schedule) of an
                            N-step schedule iff lo N <= k < hi N.  At every other step ("off") the denoising UNet evaluates the conditional
                            clip-half only -- forward_nhwc(conditional=True) on the window's conditional frames, the unperturbed twin of PAG's
                            evaluation and the conditional queue of two_queues, launch for launch -- its prediction is accumulated into the c plane
                            with the real counter, and after the all-reduce ops.cfg_uncond_cache(mode 1, scale 0) copies the c plane over the u
                            plane, so that c - u is exactly 0 and every step entry, the rescale, APG and PAG / SEG work on the planes unchanged:
                            the guided v is the conditional mean.  A STATED DEVIATION: outside the interval the loop stays in CFG form, so the
                            step sees the window MEAN of c, where a guidance_scale <= 1 call under context_fuse="flat" hands the scheduler the
                            window sum (see context_fuse).  The reference banks are written for both halves as always, i.e. with the
                            reference's interleaved [u, c, u, c, ...] contexts over the frames: the conditional half of a CFG run is therefore
                            not the prediction of a run without CFG, with or without this keyword.  Checked whether or not
                            guidance is on; inert (no call, no buffer) with guidance_scale <= 1.  Image quality on real weights has not been
                            assessed.  (0.0, 1.0) (the default): bitwise the loop without the keyword, the same operator calls, no buffer
        uncond_cache_interval  an integer n >= 1 (the CFG cache of FasterCache, arXiv 2410.19355: the idea only), an opt-in APPROXIMATION: inside the
                            guidance interval the unconditional half is evaluated on every n-th step only.  A step inside the interval is FULL
                            when no guidance direction has been stored since the pass began (or since the interval was entered) or n steps
                            have passed since the last full step: today's two-half evaluation, after which (and after the all-reduce)
                            ops.cfg_uncond_cache(mode 0) stores d = c - u, one fp32 (F, h*w, 4) buffer per call, allocated only when n > 1.
                            Every other step inside the interval is CACHED: the conditional-only evaluation, then
                            ops.cfg_uncond_cache(mode 1, scale 1) writes u_sum = c_sum - d cnt, so that the step forms c + (g - 1) d_last in
                            place of u + g (c - u).  The kind of a step is decided on the host from integers: no sync.  PAG's / SEG's
                            evaluation is made on all three kinds.  Composes with both samplers, eta / SDE noise, init_latents / strength, every
                            window schedule and fuse mode, FreeInit (every pass starts with an empty cache), guidance_rescale, APG, PAG / SEG
                            (they read the restored planes), kv_downsample, tile_attention and window_parallel (the restore runs after the
                            all-reduce, replicated: every rank holds an identical d, no new collective).  ValueError, before anything runs,
                            together with deep_cache_interval > 1 (a DeepCache slot is shaped by the batch of the evaluation that filled it; a
                            conditional-only step would meet a slot of the other shape), for this keyword and for guidance_interval alike.
                            Image quality on real weights has not been assessed.  1 (the default): as for guidance_interval
        returns latents (1, 4, F, h, w) in the input dtype.
        """
        plan = self.sampling_plan(
            num_inference_steps, guidance_scale, init_latents is not None, tuple(latents.shape[2:]), sampler=self._sampler(), eta=eta, guidance_rescale=guidance_rescale, strength=strength, context_fuse=context_fuse, free_init_iters=free_init_iters,
            free_init_filter=free_init_filter, free_init_order=free_init_order, free_init_spatial_stop=free_init_spatial_stop,
            free_init_temporal_stop=free_init_temporal_stop, free_init_fast=free_init_fast, apg=apg, apg_eta=apg_eta,
            apg_norm_threshold=apg_norm_threshold, apg_momentum=apg_momentum, pag_scale=pag_scale, pag_adaptive_scale=pag_adaptive_scale,
            pag_applied_layers=pag_applied_layers, kv_downsample=kv_downsample, kv_downsample_mode=kv_downsample_mode, seg_scale=seg_scale,
            seg_blur_sigma=seg_blur_sigma, seg_applied_layers=seg_applied_layers, tile_attention=tile_attention,
            tile_attention_shift=tile_attention_shift, deep_cache_interval=deep_cache_interval, deep_cache_depth=deep_cache_depth,
            guidance_interval=guidance_interval, uncond_cache_interval=uncond_cache_interval, deep_cache_threshold=deep_cache_threshold)
        if init_latents is not None and tuple(init_latents.shape) != tuple(latents.shape):
            raise ValueError(f"init_latents of shape {tuple(init_latents.shape)} do not match latents of shape {tuple(latents.shape)}")
        ops.require_gpu(latents, "MikuDanceVideoPipeline.denoise")
        plan = self._resolve_plan(plan)                                  # a name that selects no block, too many factors: raised here
        rescale, projected, pert = (plan.guide if isinstance(plan.guide, kind) else None for kind in (Rescale, APG, Perturb))
        n_fi, *fi_filter, fi_fast = plan.free_init
        dev = latents.device
        context_frames = context_frames or self.default_context_frames
        do_cfg = guidance_scale > 1.0
        nb = 2 if do_cfg else 1
        den, refu, sch = self.denoising_unet, self.reference_unet, self.scheduler
        from .scheduler import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
        multistep, unipc = isinstance(sch, DPMSolverMultistepScheduler), plan.sampler == "unipc"
        if not multistep and not unipc and not isinstance(sch, DDIMScheduler):
            raise TypeError(f"MikuDanceVideoPipeline.denoise: unsupported scheduler {type(sch).__name__}; the supported ones are "
                            "mikudance_amd.DDIMScheduler and mikudance_amd.DPMSolverMultistepScheduler")
        if multistep and eta > 0:
            raise ValueError("eta applies to DDIMScheduler only; for stochastic DPM-Solver++ sampling use "
                             "DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++')")
        fi_steps = [free_init.pass_steps(num_inference_steps, n_fi, i, fi_fast) for i in range(n_fi)]
        sch.set_timesteps(fi_steps[0])
        timesteps = [int(t) for t in sch.timesteps]
        t_start = 0
        if init_latents is not None:                                     # video-to-video: the tail of the schedule (DPM: begin index set)
            timesteps = [int(t) for t in sch.get_timesteps(num_inference_steps, plan.strength)[0]]
            t_start = num_inference_steps - len(timesteps)
        _, c, F_, hh, ww = latents.shape
        HW = hh * ww
        writer = ReferenceAttentionControl(refu, do_classifier_free_guidance=do_cfg, mode="write", batch_size=1, fusion_blocks="full")
        reader = ReferenceAttentionControl(den, do_classifier_free_guidance=do_cfg, mode="read", batch_size=1, fusion_blocks="full")
        reader_blocks = reader._blocks(den)

        # internal latents: (F, h, w, 4) fp16 NHWC frames
        st = latents.stride()
        lat = ops.pack_nhwc(latents, F_, F_, (0, st[2], st[1], st[3], st[4]), 0, c, 4, hh, ww)
        if init_latents is not None:                                     # noise x0 to the first kept timestep, every rank the same
            x0 = init_latents.to(dev)
            sx = x0.stride()
            ops.add_noise(lat, ops.pack_nhwc(x0, F_, F_, (0, sx[2], sx[1], sx[3], sx[4]), 0, c, 4, hh, ww), *sch.noise_coefficients(timesteps[0]))
        if n_fi > 1:                                                     # FreeInit: the packed initial noise, the table, (a, b) of t = T
            noise0 = lat.clone()
            lpf = free_init.freq_filter(F_, hh, ww, *fi_filter).to(dev)
            fi_ab = sch.noise_coefficients(sch.num_train_timesteps - 1)
        # a perturbation (PAG / SEG): its prediction is one more plane of the accumulator (the all_reduce carries it), summed by the same kernels
        # at halves = 1 against a scratch counter (they add to their counter: the real one would count every window twice)
        noise_sum = torch.zeros((nb + 1 if pert else nb, F_, HW, 4), device=dev, dtype=torch.float32)
        counter = torch.zeros((F_,), device=dev, dtype=torch.float32)
        ns_main, ns_pert, pert_counter = noise_sum, None, None
        if pert:
            ns_main, ns_pert, pert_counter = noise_sum[:nb], noise_sum[nb:], torch.zeros((F_,), device=dev, dtype=torch.float32)
            pert_kw = dict(pag=pert.blocks) if pert.kind == "identity" else dict(seg=(pert.blocks, pert.sigma))
        kv_kw = {} if plan.kv is None else dict(kv_downsample=plan.kv)             # no plan: no keyword
        tile_plan, tile_shift = plan.tile or (None, None)                          # no plan: no keyword either
        if tile_plan is not None:
            from .unet_3d_mix import tile_shift_at
        # DeepCache: one slot per (window, plane) of this rank, plane 0 the main evaluation, 1 the perturbed one; no plan: no dict, no keyword
        dc_slots = None
        if plan.deep is not None:
            from .unet_3d_mix import DeepCacheSlot
            dc_slots = {}

        self.last_deep_cache_trace = None if dc_slots is None else []       # what every evaluation of this call did: traced() below

        def deep_kw(wi, plane, key):
            """forward_nhwc's deep_cache keyword for window wi: a key step fills the window's slot, a shallow step reuses it.  Under
            deep_cache_threshold the call decides (DeepCacheSlot.auto, one accumulator per slot; an empty slot, as at the first step of every
            pass, makes it a fill) and `key` is not read."""
            if dc_slots is None:
                return {}
            slot = dc_slots.get((wi, plane))
            if slot is None:
                assert key or plan.deep_threshold is not None, f"DeepCache: no slot for window {wi}, plane {plane} at a shallow step"
                slot = dc_slots[(wi, plane)] = DeepCacheSlot(plan.deep[1])
            if plan.deep_threshold is not None:
                return dict(deep_cache=slot.auto(plan.deep_threshold, plan.deep[0]))
            return dict(deep_cache=slot.fill() if key else slot.reuse())

        def traced(step_i, wi, plane, key, kw):
            """kw, the keyword of deep_kw, once its evaluation has been made: one more row (step_i, window, plane, "key" | "shallow", r) of
            self.last_deep_cache_trace; r: the distance an adaptive call measured (None: the fixed rule, or a fill of an empty slot)."""
            if kw:
                slot = kw["deep_cache"]
                fixed = plan.deep_threshold is None
                self.last_deep_cache_trace.append((step_i, wi, plane, ("key" if key else "shallow") if fixed else slot.last,
                                                   None if fixed else slot.last_distance))
        # guidance interval / cached unconditional half: d = c - u of the last full step, kept only when some step reuses it; no plan: no buffer,
        # no new call.  Under window_parallel every rank keeps its own identical copy (written after the all_reduce)
        uc_delta = None
        if plan.uncond is not None and plan.uncond[2] > 1:
            uc_delta = torch.empty((F_, HW, 4), device=dev, dtype=torch.float32)
        windows =[list(w) for w in get_context_scheduler(context_schedule)(0, num_inference_steps, F_, context_frames,
                                                                            context_stride, context_overlap)]
        mm_len = getattr(den, "temporal_position_encoding_max_len", None)
        if mm_len is not None and max(len(w) for w in windows) > mm_len:
            raise ValueError(f"windows of {max(len(w) for w in windows)} frames exceed the motion module's positional-encoding "
                             f"table (temporal_position_encoding_max_len = {mm_len})")
        # A wrapped, dilated window (context_stride >= 2, F < 2*size) can name a frame twice.  The reference's
        # `noise_pred[:, :, c] = noise_pred[:, :, c] + pred` (:662-666) is an index_put with duplicate indices: the LAST
        # occurrence's value lands and the counter grows by one.  Earlier occurrences get slot -1 = "do not accumulate".
        win_dev = [torch.tensor(accumulate_slots(w), dtype=torch.int32, device=dev) for w in windows]
        # pyramid fuse: every rank normalises over ALL windows of the step, its own or not (float64 on the host, fp32 on the device)
        wts_dev = None
        if plan.fuse == "pyramid":
            wts_dev = [torch.tensor(w, dtype=torch.float64).to(device=dev, dtype=torch.float32) for w in fuse_weights(windows, F_, "pyramid")]
        win_long = [torch.tensor(w, dtype=torch.long, device=dev) for w in windows]     # gather indices: the real frames
        whole = len(windows) == 1 and windows[0] == list(range(F_))
        embeds = image_prompt_embeds
        # DPM-Solver++: the previous step's data prediction, fp32, per call (under window_parallel every rank keeps its own identical copy)
        history = torch.zeros((F_, HW, 4), device=dev, dtype=torch.float32) if multistep else None
        # UniPC: x_last and the data predictions of the last three steps, fp32, per call; the first row of a schedule reads none of it
        unipc_state = torch.empty((4, F_, HW, 4), device=dev, dtype=torch.float32) if unipc else None
        # guidance rescale: one fp32 factor per step; APG: the momentum buffer and the per-frame (S, K).  All written and read on the device
        # (no host sync); another guide: none of them, and the other entry points called exactly as without the keywords
        if rescale:
            vscale = torch.empty((1,), device=dev, dtype=torch.float32)
        if projected:
            apg_m = torch.zeros((F_, HW, 4), device=dev, dtype=torch.float32)
            apg_coef = torch.empty((F_, 2), device=dev, dtype=torch.float32)

        def accumulate(pred, planes, count, wi, halves):
            if wts_dev is None:
                ops.window_accumulate(pred, planes, count, win_dev[wi], len(windows[wi]), F_, HW, halves=halves)
            else:
                ops.window_accumulate_weighted(pred, planes, count, win_dev[wi], wts_dev[wi], len(windows[wi]), F_, HW, halves=halves)

        def step(step_i, t, s_t):
            """The CFG + scheduler update of lat from the accumulated planes: ops.cfg_ddim_step / ops.cfg_multistep_step / ops.cfg_unipc_step, or
            the guide's flavour of it (_apg, _pag).  The same statistics on every rank: same buffers, same arithmetic."""
            if unipc:
                row = sch.unipc_coefficients(t_start + step_i)
                name, state, (a, s), co, kw = "cfg_unipc_step", (unipc_state,), row[:2], (row,), {}
            elif multistep:
                z = self._draw_noise(latents, generator) if sch.is_sde else None       # every step, like the eta path
                co = sch.multistep_coefficients(t_start + step_i)
                name, state, (a, s), kw = "cfg_multistep_step", (history,), co[:2], dict(variance_noise=z)
            else:
                co = sch.step_coefficients(t)                                          # (abar_t, abar_prev)
                z = self._draw_noise(latents, generator) if eta > 0 else None
                name, state, (a, s), kw = "cfg_ddim_step", (), (math.sqrt(co[0]), math.sqrt(1.0 - co[0])), dict(eta=float(eta), variance_noise=z)
            if projected:
                ops.cfg_apg_prepare(lat, noise_sum, counter, apg_m, apg_coef, F_, HW, a, s, *projected)
                getattr(ops, name + "_apg")(lat, noise_sum, counter, *state, apg_m, apg_coef, F_, HW, guidance_scale, *co, **kw)
            elif s_t > 0.0:
                getattr(ops, name + "_pag")(lat, ns_main, counter, *state, ns_pert[0], F_, HW, guidance_scale, s_t, *co, halves=nb, **kw)
            else:
                if rescale:
                    ops.cfg_guidance_rescale(noise_sum, counter, F_, HW, guidance_scale, rescale.phi, out=vscale)
                    kw["vscale"] = vscale
                getattr(ops, name)(lat, ns_main, counter, *state, F_, HW, guidance_scale, *co, halves=nb, **kw)

        bank_cache = {}
        refu.skip_dead_tail = True
        den.clear_context_cache()
        refu.clear_context_cache()
        try:
            for fi in range(n_fi):
                if fi > 0:                                               # re-initialise the noise, every rank the same, and start over
                    z = self._draw_noise(latents, generator)
                    ops.free_init_mix(lat, lat, noise0, z, lpf, *fi_ab)
                    sch.set_timesteps(fi_steps[fi])
                    timesteps = [int(t) for t in sch.timesteps]
                if projected:
                    apg_m.zero_()                                        # the running average starts over with every pass
                if dc_slots is not None:
                    dc_slots.clear()                                     # every pass starts at k = 0 with an empty cache
                uc_since = None                                          # steps since the last full step; None: no d stored (in this pass / interval)
                for step_i, t in enumerate(timesteps):
                    noise_sum.zero_()
                    counter.zero_()
                    s_t = self._pag_scale_at(pert.scale, pert.adaptive, t) if pert else 0.0     # a pure function of t: no sync
                    # tiled self-attention: the main and the perturbed evaluation of a step share the plan and the step's shift
                    sa_kw = kv_kw if tile_plan is None else dict(kv_kw, tile_attention=tile_plan, tile_shift=tile_shift_at(tile_shift, t_start + step_i))
                    dc_key = plan.deep is None or step_i % plan.deep[0] == 0      # k counts the steps this pass actually runs
                    # the step's kind, from integers on the host: "full" (both clip-halves, today's step), "off" (outside the guidance interval)
                    # or "cached" (inside it, on the last full step's d); the last two evaluate the conditional clip-half only
                    kind = "full"
                    if plan.uncond is not None:
                        gi_lo, gi_hi, uc_n = plan.uncond
                        if not gi_lo * fi_steps[fi] <= t_start + step_i < gi_hi * fi_steps[fi]:
                            kind, uc_since = "off", None
                        elif uc_since is None or uc_since + 1 >= uc_n:
                            uc_since = 0
                        else:
                            kind, uc_since = "cached", uc_since + 1
                    for wi, win in enumerate(windows):
                        if window_parallel is not None and not window_parallel.mine(wi):
                            continue                                         # another rank's window (its share arrives in the all_reduce)
                        f = len(win)
                        # ---- reference UNet (write): once per window unless reference_reuse is off
                        if wi not in bank_cache or not self.reference_reuse:
                            self._write_banks(writer, reader, embeds, ref_latents, win_long[wi], f, do_cfg, literal=not self.reference_reuse)
                            banks = [blk.bank for blk in reader_blocks]
                            if self.reference_reuse:
                                bank_cache[wi] = banks
                        else:
                            for blk, bk in zip(reader_blocks, bank_cache[wi]):
                                blk.bank = bk
                        # ---- denoising UNet (read)
                        src = lat if whole else lat.index_select(0, win_long[wi])
                        x = ops.pack_nhwc(src, nb * f, f, (0, HW * 4, 1, ww * 4, 4), 0, 4, 64, hh, ww)
                        cross = den._cross(embeds[:nb], [i // f for i in range(nb * f)], dev)
                        # both clip-halves are packed from the SAME latents (batch stride 0 above): the layers in front of the first attention
                        # run once (self.share_first_layers = False: the literal evaluation of both halves, bit-identical)
                        if kind == "full":
                            dkw = deep_kw(wi, 0, dc_key)
                            pred = den.forward_nhwc(x, nb, f, torch.full((nb,), float(t)), cross, halves_identical=self.share_first_layers,
                                                    two_queues=self.two_queues, **sa_kw, **dkw)
                            traced(step_i, wi, 0, dc_key, dkw)
                            accumulate(pred, ns_main, counter, wi, nb)
                        else:
                            # ---- the conditional frames only (PAG's call below without its perturbation), into the c plane with the real counter;
                            # the u plane stays empty until cfg_uncond_cache fills it
                            pred = den.forward_nhwc(x[f:], 1, f, torch.full((1,), float(t)), cross.rows(f, 2 * f), conditional=True, **sa_kw)
                            accumulate(pred, ns_main[1:], counter, wi, 1)
                        if s_t > 0.0:
                            # ---- PAG / SEG: the conditional frames once more (the banks are still in place), the selected self-attention maps
                            # = identity / from blurred queries
                            dkw = deep_kw(wi, 1, dc_key)
                            pred = den.forward_nhwc(x[(nb - 1) * f:], 1, f, torch.full((1,), float(t)), cross.rows(f, 2 * f) if do_cfg else cross,
                                                    **pert_kw, **sa_kw, **dkw)
                            traced(step_i, wi, 1, dc_key, dkw)
                            accumulate(pred, ns_pert, pert_counter, wi, 1)
                        reader.clear()
                        writer.clear()
                    if window_parallel is not None:
                        window_parallel.reduce(noise_sum, counter)
                    # the planes as every consumer below expects them (replicated on every rank, after the all_reduce: no new collective)
                    if kind == "off":
                        ops.cfg_uncond_cache(ns_main, counter, None, F_, HW, 1, scale=0.0)       # u_sum = c_sum: c - u == 0 exactly
                    elif kind == "cached":
                        ops.cfg_uncond_cache(ns_main, counter, uc_delta, F_, HW, 1, scale=1.0)   # u_sum = c_sum - d cnt
                    elif uc_delta is not None:
                        ops.cfg_uncond_cache(ns_main, counter, uc_delta, F_, HW, 0)              # a full step: d = c - u for the steps behind it
                    step(step_i, t, s_t)
                    if callback is not None and step_i % callback_steps == 0:
                        callback(step_i, t, self._latents_out(lat, latents))
        finally:
            if dc_slots is not None:
                dc_slots.clear()                                         # nothing outlives the clip
            refu.skip_dead_tail = False
            reader.clear()
            writer.clear()
            den.clear_context_cache()
            refu.clear_context_cache()
        return self._latents_out(lat, latents)

    @staticmethod
    def sampling_plan(num_inference_steps, guidance_scale, has_init, shape, *, guidance_rescale, strength, context_fuse,
                      free_init_iters, free_init_filter, free_init_order, free_init_spatial_stop, free_init_temporal_stop, free_init_fast, apg, apg_eta,
                      apg_norm_threshold, apg_momentum, pag_scale, pag_adaptive_scale, pag_applied_layers, kv_downsample, kv_downsample_mode,
                      seg_scale, seg_blur_sigma, seg_applied_layers, tile_attention=1, tile_attention_shift="cycle", deep_cache_interval=1,
                      deep_cache_depth=3, guidance_interval=(0.0, 1.0), uncond_cache_interval=1, sampler="ddim", eta=0.0, deep_cache_threshold=None):
        """Every refusal of denoise()'s sampling keywords (see its docstring) that needs no model -- every value is checked whether or not its
        feature is on, and neither UNet is called -- then what they resolve to -> SamplingPlan, still holding the layer names and the
        (factors, mode) that _resolve_plan hands to the denoising UNet.  has_init: there is a clip to start from (init_latents / video);
        shape: the latents' shape behind (batch, channels), (F, h, w).  sampler: "ddim", "dpm" or "unipc", what self.scheduler selects (_sampler);
        eta: denoise()'s, refused here with "unipc" (with "dpm" denoise() refuses it itself, behind the plan)."""
        from .unet_3d_mix import (check_kv_downsample, check_kv_downsample_grid, check_pag_layer_names, check_tile_attention,
                                  check_tile_attention_grid)
        asked = []

        def ask(guide):                                                  # one more of the ways to form v is asked for
            for new, old, why in _ONE_GUIDE:
                if new == guide and old in asked:
                    raise ValueError(f"{new} cannot be combined with {old}: {why}")
            asked.append(guide)

        if context_fuse not in ("flat", "pyramid"):
            raise ValueError(f"context_fuse must be 'flat' or 'pyramid', got {context_fuse!r}")
        free_init.check_arguments(free_init_iters, free_init_filter, free_init_order, free_init_spatial_stop, free_init_temporal_stop, has_init, shape if len(shape) == 3 else None)
        phi = float(guidance_rescale)
        if not (math.isfinite(phi) and 0.0 <= phi <= 1.0):
            raise ValueError(f"guidance_rescale must be a finite number in [0, 1], got {guidance_rescale}")
        if phi > 0.0:
            ask("guidance_rescale > 0")
        # video-to-video (diffusers' wording for a schedule with no step left)
        st = float(strength)
        if not (math.isfinite(st) and 0.0 < st <= 1.0):
            raise ValueError(f"strength must be a finite number in (0, 1], got {strength}")
        if st < 1.0 and not has_init:
            raise ValueError(f"strength={strength} < 1 needs a clip to start from: pass init_latents (denoise) or video (__call__)")
        if has_init and min(int(num_inference_steps * strength), num_inference_steps) < 1:
            raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline steps is "
                             f"{min(int(num_inference_steps * strength), num_inference_steps)} which is < 1 and not appropriate for this pipeline.")
        e, r, b = float(apg_eta), float(apg_norm_threshold), float(apg_momentum)
        if not (math.isfinite(e) and 0.0 <= e <= 1.0):
            raise ValueError(f"apg_eta must be a finite number in [0, 1], got {apg_eta}")
        if not (math.isfinite(r) and r >= 0.0):
            raise ValueError(f"apg_norm_threshold must be a finite number >= 0, got {apg_norm_threshold}")
        if not (math.isfinite(b) and -1.0 < b < 1.0):
            raise ValueError(f"apg_momentum must be a finite number in (-1, 1), got {apg_momentum}")
        if apg:
            ask("apg=True")
        pag_s, pag_a = float(pag_scale), float(pag_adaptive_scale)
        if not (math.isfinite(pag_s) and pag_s >= 0.0):
            raise ValueError(f"pag_scale must be a finite number >= 0, got {pag_scale}")
        if not (math.isfinite(pag_a) and pag_a >= 0.0):
            raise ValueError(f"pag_adaptive_scale must be a finite number >= 0, got {pag_adaptive_scale}")
        pag_names = check_pag_layer_names(pag_applied_layers)
        if pag_s > 0.0 and not pag_names:
            raise ValueError("pag_applied_layers is empty: perturbed-attention guidance needs at least one attention block")
        if pag_s > 0.0:
            ask("pag_scale > 0")
        kv_factors, kv_mode = check_kv_downsample(kv_downsample, kv_downsample_mode)
        check_kv_downsample_grid(kv_factors, int(shape[-2]), int(shape[-1]))      # every selected level keeps at least one s x s block
        tile_factors, tile_shift = check_tile_attention(tile_attention, tile_attention_shift)
        check_tile_attention_grid(tile_factors, int(shape[-2]), int(shape[-1]), kv_factors)      # t divides the level's grid; a tile holds an s x s block
        try:
            seg_s, sigma = float(seg_scale), float(seg_blur_sigma)
        except (TypeError, ValueError):
            raise ValueError(f"seg_scale and seg_blur_sigma must be numbers, got {seg_scale!r} and {seg_blur_sigma!r}") from None
        if not (math.isfinite(seg_s) and seg_s >= 0.0):
            raise ValueError(f"seg_scale must be a finite number >= 0, got {seg_scale}")
        if math.isnan(sigma) or not sigma > 0.0:
            raise ValueError(f"seg_blur_sigma must be a finite number > 0 or math.inf, got {seg_blur_sigma}")
        seg_names = check_pag_layer_names(seg_applied_layers, "seg_applied_layers")
        if seg_s > 0.0 and not seg_names:
            raise ValueError("seg_applied_layers is empty: smoothed-energy guidance needs at least one attention block")
        if seg_s > 0.0:
            ask("seg_scale > 0")
        import numbers
        for name, v in (("deep_cache_interval", deep_cache_interval), ("deep_cache_depth", deep_cache_depth)):
            if not isinstance(v, numbers.Integral) or isinstance(v, bool) or v < 1:
                raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
        try:
            gi = tuple(guidance_interval)
            gi_lo, gi_hi = (float(v) for v in gi)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_interval must be two finite numbers (lo, hi) with 0 <= lo <= hi <= 1, got {guidance_interval!r}") from None
        if any(isinstance(v, (bool, str)) for v in gi) or not (math.isfinite(gi_lo) and math.isfinite(gi_hi) and 0.0 <= gi_lo <= gi_hi <= 1.0):
            raise ValueError(f"guidance_interval must be two finite numbers (lo, hi) with 0 <= lo <= hi <= 1, got {guidance_interval!r}")
        if not isinstance(uncond_cache_interval, numbers.Integral) or isinstance(uncond_cache_interval, bool) or uncond_cache_interval < 1:
            raise ValueError(f"uncond_cache_interval must be an integer >= 1, got {uncond_cache_interval!r}")
        skips_uncond = (gi_lo, gi_hi) != (0.0, 1.0) or uncond_cache_interval > 1
        if skips_uncond and deep_cache_interval > 1:
            raise ValueError("guidance_interval / uncond_cache_interval cannot be combined with deep_cache_interval > 1: a DeepCache slot is shaped by "
                             "the batch of the evaluation that filled it (both clip-halves), and a conditional-only step would meet a slot of the "
                             "other shape")
        deep_thr = None
        if deep_cache_threshold is not None:
            from .unet_3d_mix import check_deep_cache_threshold
            deep_thr = check_deep_cache_threshold(deep_cache_threshold)
            if skips_uncond:
                raise ValueError("guidance_interval / uncond_cache_interval cannot be combined with deep_cache_threshold: a DeepCache slot is shaped "
                                 "by the batch of the evaluation that filled it (both clip-halves), and a conditional-only step would meet a slot "
                                 "of the other shape")
            if deep_cache_interval < 2:
                raise ValueError(f"deep_cache_threshold={deep_cache_threshold!r} needs deep_cache_interval >= 2: the interval is the cap, at most "
                                 f"deep_cache_interval - 1 shallow steps in a row, got deep_cache_interval={deep_cache_interval}")
        if sampler not in ("ddim", "dpm", "unipc"):
            raise ValueError(f"sampler must be 'ddim', 'dpm' or 'unipc', got {sampler!r}")
        if sampler == "unipc" and eta != 0:
            raise ValueError(f"eta={eta} cannot be combined with UniPCMultistepScheduler: UniPC is a deterministic solver here (eta applies to "
                             "DDIMScheduler only; for stochastic sampling use DPMSolverMultistepScheduler(algorithm_type='sde-dpmsolver++'))")
        guide = None
        if pag_s > 0.0:
            guide = Perturb("identity", pag_s, pag_a, pag_names, None)
        elif seg_s > 0.0:                                                # PAG's evaluation, plane and step with blurred queries in the selected blocks
            guide = Perturb("blur", seg_s, 0.0, seg_names, sigma)
        elif apg and guidance_scale > 1.0:                               # APG and the rescale act on CFG's v: without CFG, the plain step
            guide = APG(b, e, r)
        elif phi > 0.0 and guidance_scale > 1.0:
            guide = Rescale(phi)
        return SamplingPlan(context_fuse, (free_init_iters, free_init_filter, free_init_order, free_init_spatial_stop, free_init_temporal_stop,
                                           free_init_fast), strength, (kv_factors, kv_mode) if any(f > 1 for f in kv_factors) else None, guide,
                            (tile_factors, tile_shift) if any(f > 1 for f in tile_factors) else None,
                            (int(deep_cache_interval), int(deep_cache_depth)) if deep_cache_interval > 1 else None,
                            (gi_lo, gi_hi, int(uncond_cache_interval)) if skips_uncond and guidance_scale > 1.0 else None, deep_thr, sampler)

    def _sampler(self):
        """The sampling plan's name for what self.scheduler selects; any other scheduler counts as "ddim" until denoise() refuses it."""
        from .scheduler import DPMSolverMultistepScheduler, UniPCMultistepScheduler
        return "unipc" if isinstance(self.scheduler, UniPCMultistepScheduler) else "dpm" if isinstance(self.scheduler, DPMSolverMultistepScheduler) else "ddim"

    def _resolve_plan(self, plan):
        """The refusals only the denoising UNet can make (a layer name that selects no block, more factors than levels, a level without
        attention) -> the plan with the selected blocks for the names and the per-block K / V plan for (factors, mode)."""
        den, guide = self.denoising_unet, plan.guide
        if plan.deep is not None:
            den.check_deep_cache_depth(plan.deep[1])
        if isinstance(guide, Perturb):
            what = () if guide.kind == "identity" else ("seg_applied_layers", "smoothed-energy guidance")
            guide = guide._replace(blocks=den.pag_blocks(guide.blocks, *what))
        return replace(plan, guide=guide, kv=None if plan.kv is None else den.kv_downsample_plan(*plan.kv),
                       tile=None if plan.tile is None else (den.tile_attention_plan(plan.tile[0]), plan.tile[1]))

    @staticmethod
    def _pag_scale_at(pag_scale, pag_adaptive_scale, t):
        """diffusers PAGMixin._get_pag_scale: the scale decays linearly as t falls from 1000 and stops at 0."""
        return max(pag_scale - pag_adaptive_scale * (1000 - int(t)), 0.0)

    @staticmethod
    def _draw_noise(latents, generator):
        """One N(0, 1) draw of the latents' shape and dtype from `generator` (on ITS device, diffusers randn_tensor), packed to the
        (F, h, w, 4) fp16 layout of the internal latents."""
        from .scheduler import randn_tensor
        _, c, F_, hh, ww = latents.shape
        zn = randn_tensor(latents.shape, generator=generator, device=latents.device, dtype=latents.dtype)      # (1, 4, F, h, w)
        zs = zn.stride()
        return ops.pack_nhwc(zn, F_, F_, (0, zs[2], zs[1], zs[3], zs[4]), 0, c, 4, hh, ww)

    def _latents_out(self, lat, like):
        out = torch.empty(like.shape, device=like.device, dtype=like.dtype)
        _, c, F_, hh, ww = like.shape
        so = out.stride()
        ops.unpack_nhwc(lat, out, F_, F_, (0, so[2], so[1], so[3], so[4]), c, hh, ww)
        return out

    def _write_banks(self, writer, reader, embeds, ref_latents, win_long, f, do_cfg, literal):
        """Run the reference UNet in write mode for one window and hand its banks to the reader blocks."""
        refu = self.reference_unet
        dev = ref_latents.device
        g = ref_latents[0].index_select(0, win_long)                         # (f, 22, h, w)
        if literal and do_cfg:
            g = g.repeat(2, 1, 1, 1)                                         # [uncond f | cond f] (:636-643)
            index = [k % 2 for k in range(2 * f)]                            # embeds.repeat((f,1,1)) = [u,c,u,c,...] (:645)
        elif do_cfg:
            index = [(f + j) % 2 for j in range(f)]                          # what cond frame j sees under that interleaving
        else:
            index = [0] * f
        B, nch, hh, ww = g.shape
        st = g.stride()
        x = ops.pack_nhwc(g, B, 1, (st[0], 0, st[1], st[2], st[3]), 0, nch - 2, 64, hh, ww)

        def motion_at(h2, w2):
            return ops.pack_nhwc(g, B, 1, (st[0], 0, st[1], st[2], st[3]), nch - 2, 2, 64, h2, w2, hin=hh, win=ww)

        cross = refu._cross(embeds, index, dev)
        refu.forward_nhwc(x, motion_at, cross)
        reader.update(writer)

    # ------------------------------------------------------------------------------------------ VAE glue (caller's modules)
    def _encode(self, tensor):
        return self.vae.encode(tensor.to(dtype=self.vae.dtype, device=self.vae.device)).latent_dist.mean * 0.18215

    dedupe_encodes = True      # False: every image goes through the VAE, duplicates included (A/B and the bit-identity test)

    @staticmethod
    def _unique_images(x):
        """x (N, 3, H, W) on one device -> (rep, inverse): rep = indices of the first occurrence of every DISTINCT image, inverse[i] =
        position in rep of image i's representative.  Exact: a cheap per-image signature (two partial sums) only proposes candidates,
        membership is decided by an element-wise comparison with the candidate (one batched compare and one host sync per signature)."""
        n = x.shape[0]
        flat = x.reshape(n, -1)
        sig = torch.stack([flat.sum(1, dtype=torch.float32), flat[:, 1::3].sum(1, dtype=torch.float32)], 1).cpu().tolist()
        by_sig = {}
        for i, s in enumerate(sig):
            by_sig.setdefault(tuple(s), []).append(i)
        rep, inverse = [], [0] * n
        for idxs in by_sig.values():
            todo = idxs
            while todo:                                                  # a signature collision leaves several distinct images in one group
                r = todo[0]
                same = (flat[todo] == flat[r]).all(1).cpu().tolist() if len(todo) > 1 else [True]
                same[0] = True                                           # the representative itself (an image holding NaNs is not == itself)
                pos = len(rep)
                rep.append(r)
                for i, eq in zip(todo, same):
                    if eq:
                        inverse[i] = pos
                todo = [i for i, eq in zip(todo, same) if not eq]
        order = sorted(range(len(rep)), key=lambda k: rep[k])            # representatives in input order (stable batches)
        rank = {k: j for j, k in enumerate(order)}
        return [rep[k] for k in order], [rank[k] for k in inverse]

    def _encode_many(self, tensors):
        """The reference encodes the 3F + 2 condition images one at a time (:456-549).  Two result-preserving reductions:
          * the VAE is per-image arithmetic (its GroupNorms and its attention never mix samples), so batches of `vae_batch` images give
            the same latents with an eighth of the launches and full-size GEMM / conv tiles;
          * an image that occurs several times is encoded ONCE and its latent copied: when face / hand guidance is absent the script
            substitutes F black frames each (scripts/inference_video.py:156-180), i.e. 2F of the 3F + 2 inputs of configs[1] are the same
            image (32 of 50 encodes at F = 16).  Deterministic kernels + per-image arithmetic make the copy bit-identical to a second
            encode (tests/test_vae_cpu.py::test_deduped_encodes_are_bit_identical on the host side, tests/test_vae_gpu.py on the HIP path)."""
        dev, dt = self.vae.device, self.vae.dtype
        x = torch.cat([t.to(device=dev, dtype=dt) for t in tensors], dim=0)
        if self.dedupe_encodes and x.shape[0] > 1:
            rep, inverse = self._unique_images(x)
        else:
            rep, inverse = list(range(x.shape[0])), list(range(x.shape[0]))
        self.last_encode_stats = dict(images=x.shape[0], encoded=len(rep))
        u = x if len(rep) == x.shape[0] else x[torch.tensor(rep, device=x.device)]
        lat = torch.cat([self._encode(u[i:i + self.vae_batch]) for i in range(0, u.shape[0], self.vae_batch)], dim=0)
        return lat if len(rep) == x.shape[0] else lat[torch.tensor(inverse, device=lat.device)]

    def _decode_frames(self, latents, batch, temporal, per_batch, display=False):
        """The one road from (b, c, f, h, w) latents to frames on the host, shared by the float, the bytes and the colour-matched output: the
        scaling and the frame order of the reference, VAE batches of `batch` frames (num_frames= for the temporal decoder), clips again, ONE
        device-to-host copy.  per_batch(i, chunk, kw, rows) decodes frames i .. i + len(chunk) - 1 of the `total` = b f: it either returns
        them (the batches are concatenated) or writes them to rows(i, n, frame_shape, dtype, device) -- rows i .. i + n - 1 of ONE
        (total, *frame_shape) device buffer, allocated at the first call, which alone needs the last three: the first batch tells the frame
        size (the VAE's factor is its own) -- and returns None.  uint8 frames are (H, W, 3): the result is the CPU (b, f, H, W, 3) tensor.  Other frames are (c, H, W): the
        result is the float32 (b, c, f, H, W) numpy array, after (x / 2 + 0.5).clamp(0, 1) if `display`."""
        video_length = latents.shape[2]
        latents = 1 / 0.18215 * latents
        latents = latents.permute(0, 2, 1, 3, 4).reshape((-1,) + tuple(latents.shape[1:2]) + tuple(latents.shape[3:]))
        total, parts, whole = latents.shape[0], [], []

        def rows(i, n, frame_shape=None, dtype=None, device=None):
            if not whole:
                whole.append(torch.empty((total,) + tuple(frame_shape), device=device, dtype=dtype))
            return whole[0][i:i + n]

        for i in range(0, total, batch):
            chunk = latents[i:i + batch].to(self.vae.dtype)
            parts.append(per_batch(i, chunk, dict(num_frames=chunk.shape[0]) if temporal else {}, rows))
        video = whole[0] if whole else torch.cat(parts)                     # per-frame arithmetic: batching changes nothing
        video = video.reshape((-1, video_length) + tuple(video.shape[1:]))
        if video.dtype == torch.uint8:
            return video.cpu()
        video = video.permute(0, 2, 1, 3, 4)
        if display:
            video = (video / 2 + 0.5).clamp(0, 1)
        return video.cpu().float().numpy()

    def _decode_u8(self, latents, batch, temporal=False):
        """The uint8 twin of decode_latents / decode_temporal: every batch through the VAE's decode_u8 (md_frames_u8: quantised on the device,
        straight into its rows of the one buffer) -> a CPU torch.uint8 (b, f, H, W, 3) tensor: bit for bit (the float path's array * 255)
        cast to uint8 and permuted."""
        if not hasattr(self.vae, "decode_u8"):
            raise ValueError(f"output_type 'uint8' / 'pil': {type(self.vae).__name__} has no decode_u8")

        def per_batch(i, chunk, kw, rows):
            if i:
                self.vae.decode_u8(chunk, out=rows(i, chunk.shape[0]), **kw)
            else:
                first = self.vae.decode_u8(chunk, **kw)
                rows(0, first.shape[0], first.shape[1:], torch.uint8, first.device)[:] = first
        return self._decode_frames(latents, batch, temporal, per_batch)

    def color_match_plan(self, color_match, color_match_strength, color_match_target, color_match_scope, ref_image, height, width, clips):
        """__call__'s color_match keywords, checked before anything runs -> None (off) or the plan _decode_color_matched takes:
        dict(mode, strength, scope, targets), targets one entry per clip, "first_frame" or the (sums, n) of a target image
        (color_match.moments_of_image of the image resized to height x width like the reference image).  ValueError for a bad value, for a
        keyword given without color_match, for a VAE without decode_image_view and for one whose images do not have 3 channels."""
        from . import color_match as CM
        if color_match is None:
            if color_match_strength != 1.0 or color_match_target is not None or color_match_scope != "frame":
                raise ValueError("color_match_strength / color_match_target / color_match_scope need color_match='mean_std' or 'mkl'")
            return None
        if color_match not in CM.MODES:
            raise ValueError(f"color_match must be None or one of {CM.MODES}, got {color_match!r}")
        a = color_match_strength
        if isinstance(a, bool) or not isinstance(a, (int, float)) or not math.isfinite(a) or not 0.0 <= a <= 1.0:
            raise ValueError(f"color_match_strength must be a finite number in [0, 1], got {a!r}")
        if color_match_scope not in CM.SCOPES:
            raise ValueError(f"color_match_scope must be one of {CM.SCOPES}, got {color_match_scope!r}")
        targets = list(color_match_target) if isinstance(color_match_target, (list, tuple)) else [color_match_target] * clips
        if len(targets) != clips:
            raise ValueError(f"color_match_target lists {len(targets)} targets for {clips} clips: one per clip")
        is_image = lambda t: hasattr(t, "convert") and hasattr(t, "resize")
        if not all(t is None or (t == "first_frame" if isinstance(t, str) else is_image(t)) for t in targets):
            raise ValueError(f"color_match_target must be None (the reference image), a PIL image or 'first_frame' (or a list of them, one per clip), "
                             f"got {color_match_target!r}")
        if not hasattr(self.vae, "decode_image_view"):
            raise ValueError(f"color_match: {type(self.vae).__name__} has no decode_image_view")
        channels = getattr(getattr(self.vae, "config", None), "out_channels", 3)
        if channels != 3:
            raise ValueError(f"color_match: the VAE decodes images of {channels} channels, colour matching needs 3")
        known = {}

        def sums_of(img):
            if id(img) not in known:
                known[id(img)] = CM.moments_of_image(_pil_to_tensor(img, height, width, normalize=False)[0].permute(1, 2, 0).numpy())
            return known[id(img)]
        return dict(mode=color_match, strength=float(a), scope=color_match_scope,
                    targets=[t if t == "first_frame" else sums_of(ref_image if t is None else t) for t in targets])

    def _decode_color_matched(self, latents, batch, plan, temporal=False, as_bytes=False):
        """decode_latents / decode_temporal / _decode_u8 with colour matching (plan: color_match_plan's): the same scaling, frame order and VAE
        batches; per batch the VAE's decode_image_view (the image where the decoder left it), ops.color_moments, ONE host read of B x 9
        doubles, color_match.transform per frame, ops.color_apply straight into the output buffer -- bytes (as_bytes: the CPU uint8
        (b, f, H, W, 3) tensor of _decode_u8) or fp32 (the float32 (b, c, f, H, W) numpy array of decode_latents).  scope "clip": the decoded
        views of every batch stay on the device until the last batch's sums are in, the frames' sums of a clip are added into ONE transform,
        then every batch is applied.  Target "first_frame": the sums of the clip's own frame 0.  self.last_color_match: (M', t', fallback)
        per frame, in frame order, float64."""
        from . import color_match as CM
        video_length, total = latents.shape[2], latents.shape[0] * latents.shape[2]
        mode, strength, per_clip, targets = plan["mode"], plan["strength"], plan["scope"] == "clip", plan["targets"]
        held, sums, maps = [], np.empty((total, 9), dtype=np.float64), []

        def target_of(clip, pixels):
            t = targets[clip]
            return (sums[clip * video_length], pixels) if t == "first_frame" else t

        def apply(i, view, maps, rows):
            n, _, H, W = view.shape
            out = rows(i, n, (H, W, 3) if as_bytes else (3, H, W), torch.uint8 if as_bytes else torch.float32, view.device)
            ops.color_apply(view, torch.from_numpy(CM.coefficients(maps)).to(view.device), out=out, dtype=out.dtype)

        def per_batch(i, chunk, kw, rows):
            view = self.vae.decode_image_view(chunk, **kw)
            n, pixels = view.shape[0], view.shape[2] * view.shape[3]
            sums[i:i + n] = ops.color_moments(view).cpu().numpy()          # the one host read of this batch
            if not per_clip:
                maps.extend(CM.transform(sums[j], pixels, *target_of(j // video_length, pixels), mode, strength) for j in range(i, i + n))
                apply(i, view, maps[i:], rows)
                return
            held.append((i, view))
            if i + n == total:                                             # the last batch's sums are in
                clip_maps = [CM.transform(sums[c * video_length:(c + 1) * video_length].sum(0), pixels * video_length, *target_of(c, pixels), mode, strength)
                             for c in range(total // video_length)]
                maps.extend(clip_maps[j // video_length] for j in range(total))
                for j, held_view in held:
                    apply(j, held_view, maps[j:j + held_view.shape[0]], rows)
                del held[:]
        video = self._decode_frames(latents, batch, temporal, per_batch)
        self.last_color_match = maps
        return video

    def decode_latents(self, latents, output_type=None):
        """reference :115-130 -- per-frame VAE decode, (x/2+0.5).clamp(0,1), float32 numpy (b,c,f,h,w).  output_type "uint8": a CPU torch.uint8
        (b, f, H, W, 3) tensor instead (_decode_u8); None: the reference's array."""
        if output_type is not None:
            if output_type != "uint8":
                raise ValueError(f"decode_latents: output_type must be None or 'uint8', got {output_type!r}")
            return self._decode_u8(latents, self.vae_batch)
        return self._decode_frames(latents, self.vae_batch, False, lambda i, chunk, kw, rows: self.vae.decode(chunk, **kw).sample, display=True)

    def decode_temporal(self, latents, decode_chunk_size=None, output_type=None):
        """reference :132-150 (AutoencoderKLTemporalDecoder in chunks of self.decode_chunk_size = 16 frames).  output_type as decode_latents."""
        decode_chunk_size = decode_chunk_size or self.decode_chunk_size
        if output_type is not None:
            if output_type != "uint8":
                raise ValueError(f"decode_temporal: output_type must be None or 'uint8', got {output_type!r}")
            return self._decode_u8(latents, decode_chunk_size, temporal=True)
        return self._decode_frames(latents, decode_chunk_size, True, lambda i, chunk, kw, rows: self.vae.decode(chunk, **kw).sample, display=True)

    def interpolate_latents(self, latents, interpolation_factor, device):
        """reference :317-360 -- (F - 1) * factor + 1 frames: every original frame, and factor - 1 blends between neighbours
        (method chosen with set_tensor_interpolation_method; a few elementwise ops on 1 MB of latents, once per clip)."""
        if interpolation_factor < 2:
            return latents
        method = get_tensor_interpolation_method()
        if method is None:
            raise TypeError("interpolate_latents: call set_tensor_interpolation_method(is_slerp) first (the reference's module-level "
                            "`tensor_interpolation` is None until then, src/pipelines/utils.py:3-12)")
        b, c, f, h, w = latents.shape
        out = torch.zeros((b, c, (f - 1) * interpolation_factor + 1, h, w), device=latents.device, dtype=latents.dtype)
        rate = [i / interpolation_factor for i in range(interpolation_factor)][1:]
        idx = 0
        v1 = None
        for i0 in range(f - 1):
            v0, v1 = latents[:, :, i0], latents[:, :, i0 + 1]
            out[:, :, idx] = v0
            idx += 1
            for r in rate:
                out[:, :, idx] = method(v0.to(device=device), v1.to(device=device), r).to(latents.device)
                idx += 1
        out[:, :, idx] = v1
        return out

    def clip_embeds(self, ref_image):
        """reference :406-416 -- all 257 tokens: last_hidden_state -> post_layernorm -> visual_projection.
        `image_encoder` is mikudance_amd.CLIPVisionModelWithProjection (HIP kernels) or any module with the transformers
        surface (`(pixel_values).last_hidden_state`, `.vision_model.post_layernorm`, `.visual_projection`)."""
        from .clip_vision import clip_preprocess
        clip_image = clip_preprocess(ref_image.resize((224, 224)))             # == CLIPImageProcessor().preprocess(...).pixel_values
        enc = self.image_encoder
        px = clip_image.to(self._device, dtype=enc.dtype)
        if hasattr(enc, "image_prompt_embeds"):
            return enc.image_prompt_embeds(px)
        emb = enc(px).last_hidden_state
        return enc.visual_projection(enc.vision_model.post_layernorm(emb))

    def _condition_latents(self, ref_image, ref_skel_image, groups, video, scene_motion, height, width, f):
        """The VAE latents of every condition image at height x width and the flow -> (ref_latents (1, F, 22, h, w), init_latents (1, 4, F, h, w) or
        None).  All 3F + 2 condition images in ONE pass through the VAE (reference :456-549 encodes them one by one, same arithmetic per image),
        and the video-to-video frames after them, in the same pass."""
        rep = lambda z: z.unsqueeze(1).repeat(1, f, 1, 1, 1).reshape((-1,) + tuple(z.shape[1:]))
        lat_all = self._encode_many([_pil_to_tensor(ref_image, height, width, True), _pil_to_tensor(ref_skel_image, height, width, False)]
                                    + [_pil_to_tensor(im, height, width, False) for grp in groups for im in grp]
                                    + [_pil_to_tensor(im, height, width, True) for im in ([] if video is None else video)])
        ref_image_latents, pose_ref_latents = rep(lat_all[0:1]), rep(lat_all[1:2])
        o = [2]
        for grp in groups:
            o.append(o[-1] + len(grp))
        pose_tgt, face_tgt, hand_tgt = (lat_all[a:b] for a, b in zip(o[:-1], o[1:]))
        init_latents = None if video is None else lat_all[o[-1]:o[-1] + f].permute(1, 0, 2, 3)[None]     # (1, 4, F, h, w)
        tracker = torch.from_numpy(np.asarray(scene_motion)).to(dtype=ref_image_latents.dtype, device=ref_image_latents.device)
        return torch.cat([ref_image_latents, pose_ref_latents, pose_tgt, face_tgt, hand_tgt, tracker], dim=1)[None], init_latents

    # ------------------------------------------------------------------------------------------ two-pass high-resolution sampling
    hires_min_side = 64        # px: the smallest side pass 1 may have (8 latent cells; the UNets halve three times)

    def hires_plan(self, height, width, num_inference_steps, hires_scale=1, hires_strength=0.5, hires_mode="bicubic", hires_steps=None):
        """Every refusal of __call__'s hires_* keywords that needs neither a model nor a sampling plan (each value is checked whether or not
        hires_scale is > 1) -> None for hires_scale == 1, else (H_lo, W_lo, pass 2's num_inference_steps) with
        H_lo = 8 round(height / hires_scale / 8), W_lo likewise (Python's round).  A low side below self.hires_min_side is refused."""
        import numbers
        try:
            s, st = float(hires_scale), float(hires_strength)
        except (TypeError, ValueError):
            raise ValueError(f"hires_scale and hires_strength must be numbers, got {hires_scale!r} and {hires_strength!r}") from None
        if not (math.isfinite(s) and s >= 1.0):
            raise ValueError(f"hires_scale must be a finite number >= 1, got {hires_scale}")
        if not (math.isfinite(st) and 0.0 < st < 1.0):
            raise ValueError(f"hires_strength must be a finite number in (0, 1), got {hires_strength}")
        if hires_mode not in ops.RESIZE_MODES:
            raise ValueError(f"hires_mode must be one of {sorted(ops.RESIZE_MODES)}, got {hires_mode!r}")
        if hires_steps is not None and (not isinstance(hires_steps, numbers.Integral) or isinstance(hires_steps, bool) or hires_steps < 1):
            raise ValueError(f"hires_steps must be None or an integer >= 1, got {hires_steps!r}")
        if s == 1.0:
            return None
        height_lo, width_lo = 8 * round(height / s / 8), 8 * round(width / s / 8)
        if height_lo < self.hires_min_side or width_lo < self.hires_min_side:
            raise ValueError(f"hires_scale={hires_scale}: the low size {width_lo} x {height_lo} of {width} x {height} has a side below "
                             f"{self.hires_min_side}")
        if height_lo == height or width_lo == width:
            raise ValueError(f"hires_scale={hires_scale}: the low size {width_lo} x {height_lo} has a side of the full size {width} x {height}; "
                             "use hires_scale=1 or a larger scale")
        return height_lo, width_lo, int(num_inference_steps if hires_steps is None else hires_steps)

    @staticmethod
    def lowres_scene_motion(scene_motion, h_lo, w_lo):
        """Pass 1's flow DERIVED from the full-size one, on the host: (F, 2, h, w) -> float64 numpy (F, 2, h_lo, w_lo) by
        F.interpolate(mode="bilinear", align_corners=False), channel 0 (x) times w_lo / w and channel 1 (y) times h_lo / h, the flow being
        in latent-grid units.  An approximation of camera_to_scene_motion at the low grid (its clip to mean +- 3 std and the depth resize do
        not commute with the resampling)."""
        import torch.nn.functional as F
        flow = torch.from_numpy(np.asarray(scene_motion, dtype=np.float64))
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise ValueError(f"scene motion must be (F, 2, h, w), got {tuple(flow.shape)}")
        h, w = flow.shape[2:]
        low = F.interpolate(flow, size=(h_lo, w_lo), mode="bilinear", align_corners=False)
        return (low * torch.tensor([w_lo / w, h_lo / h], dtype=torch.float64).view(1, 2, 1, 1)).numpy()

    def upscale_latents(self, latents, height, width, mode="bicubic"):
        """latents (1, 4, F, h_lo, w_lo) on the GPU -> (1, 4, F, height / 8, width / 8) in the same dtype: packed to the loop's (F, h, w, 4) fp16
        layout, resampled by ops.latent_resize (md_latent_resize_f16: mode "nearest", "bilinear" or "bicubic", F.interpolate's rules without
        antialiasing, fp32 arithmetic, one rounding) and unpacked.  No host copy.  height, width: the target size in pixels."""
        ops.require_gpu(latents, "MikuDanceVideoPipeline.upscale_latents")
        if latents.dim() != 5 or latents.shape[0] != 1 or latents.shape[1] != 4:
            raise ValueError(f"upscale_latents: latents must be (1, 4, F, h, w), got {tuple(latents.shape)}")
        _, c, F_, hl, wl = latents.shape
        hh, ww = height // self.vae_scale_factor, width // self.vae_scale_factor
        st = latents.stride()
        lat = ops.pack_nhwc(latents, F_, F_, (0, st[2], st[1], st[3], st[4]), 0, c, 4, hl, wl)
        out = torch.empty((1, c, F_, hh, ww), device=latents.device, dtype=latents.dtype)
        so = out.stride()
        ops.unpack_nhwc(ops.latent_resize(lat, F_, hl, wl, hh, ww, mode), out, F_, F_, (0, so[2], so[1], so[3], so[4]), c, hh, ww)
        return out

    # ------------------------------------------------------------------------------------------ reference-compatible call
    @torch.no_grad()
    def __call__(self, ref_image, ref_skel_image, tgt_pose_images, tgt_face_images, tgt_hand_images, scene_motion_npy, width,
                 height, video_length, num_inference_steps, guidance_scale, num_images_per_prompt=1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None, output_type: Optional[str] = "tensor",
                 return_dict: bool = True, callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
                 callback_steps: Optional[int] = 1, context_schedule="uniform", context_frames=None, context_stride=1,
                 context_overlap=8, context_batch_size=1, interpolation_factor=1, guidance_rescale: float = 0.0, video=None, strength: float = 1.0,
                 context_fuse="flat", free_init_iters=1, free_init_filter="butterworth", free_init_order=4, free_init_spatial_stop=0.25,
                 free_init_temporal_stop=0.25, free_init_fast=False, apg=False, apg_eta=0.0, apg_norm_threshold=0.0, apg_momentum=0.0,
                 pag_scale: float = 0.0, pag_adaptive_scale: float = 0.0, pag_applied_layers=("mid",), kv_downsample=1,
                 kv_downsample_mode="nearest", seg_scale: float = 0.0, seg_blur_sigma: float = 100.0, seg_applied_layers=("mid",), tile_attention=1,
                 tile_attention_shift="cycle", deep_cache_interval=1, deep_cache_depth=3, guidance_interval=(0.0, 1.0), uncond_cache_interval=1,
                 hires_scale=1, hires_strength=0.5, hires_mode="bicubic", hires_steps=None, scene_motion_lowres_npy=None, vae_tiling=False,
                 vae_tile_size=None, deep_cache_threshold=None, color_match=None, color_match_strength=1.0, color_match_target=None,
                 color_match_scope="frame", **kwargs):
        """The reference call (src/pipelines/pipeline_mikudance.py:362-704) with denoise()'s sampling keywords (see its docstring), and:

        output_type         "tensor" (the default): `videos` is the reference's float32 (b, c, f, H, W) CPU tensor in [0, 1]; "uint8": a CPU
                            torch.uint8 (b, f, H, W, 3) tensor, the frames quantised on the device (AutoencoderKL.decode_u8 / md_frames_u8) and
                            copied to the host as bytes -- bit for bit (the "tensor" result * 255) cast to uint8 and permuted, what
                            save_videos_grid's own cast makes of it; "pil": a list over b of lists of PIL.Image built from those bytes; any
                            other value: the reference's float32 numpy array, as before.  vae_batch, decode_chunk_size, vae_tiling and
                            interpolation_factor act as in the float path
        vae_tiling          True: the VAE encodes and decodes this call's images tile by tile (AutoencoderKL.enable_tiling(): diffusers' tiled
                            VAE, overlapping tiles with blended seams; memory and the mid-block attention then scale with the tile, not the
                            image).  A different result by design, each tile's GroupNorm and attention see that tile only; image quality on
                            real weights has not been assessed.  For this call only: the VAE's own state (enable_vae_tiling()) comes back
                            afterwards.  False (the default): the VAE is left as it is, and the call is bitwise what it was.  ValueError,
                            before the CLIP tower or the VAE runs, for a tile grid the VAE cannot run at this call's sizes (both of them under
                            hires_scale) and for a VAE without tiling (video_decoder)
        color_match         "mean_std" or "mkl": every decoded frame gets an affine colour transfer y = M s + t toward a target image before it is
                            quantised, the stock post-process of the SD-1.5 front ends (A1111 "apply color correction", Deforum "color
                            coherence", ComfyUI ColorMatch) against the colour drift of windows, hires pass 2, video-to-video and the opt-in
                            approximations.  On the device: per VAE batch the decoder's image is read where it lies (decode_image_view) by
                            ops.color_moments (nine sums per frame, deterministic), ONE host read of B x 9 doubles, a 3 x 3 solve in float64
                            (color_match.transform: "mean_std" scales every channel to the target's mean and standard deviation, "mkl" is the
                            Monge-Kantorovich linear map of Pitie & Kokaram 2007, which matches the whole covariance), and ops.color_apply
                            writes the result: bytes for output_type "uint8" / "pil" (bit for bit the "tensor" result * 255 cast), the
                            float32 tensor otherwise.  A frame that is flat in a channel (variance < color_match.COLOR_MATCH_EPS) or holds
                            a NaN gets the mean shift alone.  pipe.last_color_match lists (M', t', fallback) per frame.  Composes with
                            interpolation_factor, vae_tiling, hires_scale and both decoders.  Image quality on real weights has not been
                            assessed.  None (the default): bitwise the call without the keywords, the same operator calls, nothing allocated.
                            ValueError, before the CLIP tower or the VAE runs, for a bad value of any of the four keywords, for one of the
                            other three without color_match, and for a VAE without decode_image_view or with other than 3 image channels
        color_match_strength  a finite number in [0, 1]: M' = (1 - a) I + a M, t' = a t; 0 leaves the frames as they are
        color_match_target  None: ref_image, resized to width x height like the reference image itself (LANCZOS); a PIL image: that image, the
                            same way; "first_frame": the clip's own decoded frame 0 (Deforum's colour coherence); a list: one of these per clip
        color_match_scope   "frame": one transform per frame; "clip": the sums of a clip's frames are added into ONE transform for the clip,
                            which removes the global drift and keeps the clip's own variation over time (the decoded images of every VAE
                            batch then stay on the device until the last batch's sums are in)
        vae_tile_size       the tile side in image pixels, a positive multiple of 32 (sets tile_sample_min_size and tile_latent_min_size
                            together); None: the VAE's own (config.sample_size).  Needs tiling on

        hires_scale         two-pass high-resolution sampling (the "hires fix" of the SD-1.5 front ends), an opt-in APPROXIMATION of the
                            one-pass clip: a finite number >= 1.  With s > 1 the WHOLE schedule is sampled at the low size
                            H_lo = 8 round(height / s / 8), W_lo = 8 round(width / s / 8) (Python's round: halves to even), the latents
                            are enlarged on the device (upscale_latents: md_latent_resize_f16, no host copy, no VAE round trip), re-noised to
                            an intermediate timestep, and only the tail of the schedule runs at height x width: pass 2 is
                            denoise(init_latents=the enlarged latents, strength=hires_strength).  ValueError, before the CLIP tower or the
                            VAE runs, if a low side is below 64 (self.hires_min_side) or equals the full side, together with video= (pass 2 is itself the
                            video-to-video pass), and for everything either pass's sampling plan refuses at ITS latent grid (a kv_downsample
                            or tile_attention factor that fits one grid and not the other: the message names the pass).  Every sampling keyword
                            goes to both passes unchanged (guides, kv_downsample, tile_attention, deep_cache_*, guidance_interval and
                            uncond_cache_interval -- each pass against its own schedule --, context_*, eta), except that
                            FreeInit belongs to pass 1 only (it refuses init_latents) and `strength` is pass 1's (1.0).  Not with
                            window_parallel / dp (denoise() keeps supporting both).  Image quality on real weights has not been assessed.
                            NOISE ORDER: prepare_latents draws the low-size noise FIRST, then the full-size noise, both from `generator`;
                            the per-step draws of eta / SDE follow in pass order.  1 (the default): bitwise the call without the keywords,
                            the same operator calls and generator draws, nothing allocated
        hires_strength      finite, in (0, 1): pass 2 runs int(hires_steps * hires_strength) steps, the tail of its schedule
        hires_mode          "nearest" (nearest-exact), "bilinear" or "bicubic": F.interpolate's rules without antialiasing (ops.latent_resize)
        hires_steps         pass 2's num_inference_steps before hires_strength cuts it, an integer >= 1; None: num_inference_steps
        scene_motion_lowres_npy  pass 1's flow (F, 2, H_lo / 8, W_lo / 8).  None: DERIVED from scene_motion_npy (lowres_scene_motion: bilinear
                            resampling of the full-size flow, x times W_lo / width and y times H_lo / height, the flow being in latent-grid
                            units).  That is an approximation: the exact flow is camera_to_scene_motion at the low grid with the depth map
                            resized to it, which mikudance_amd.inference_video computes and passes
        callback            sees pass 1's steps, then pass 2's: pass 2's k-th kept step arrives as step_i = num_inference_steps + k (the
                            count goes on across the passes), with latents of the full size; callback_steps thins each pass from its own
                            first step
        """
        # context_batch_size: the reference concatenates that many windows along the batch axis (:601-622).  With one window per
        # context batch (every clip of <= context_frames frames, whatever the value) that is the evaluation below; with two or
        # more windows in a batch the reference itself fails at `noise_pred[:, :, c] + pred` (:662, batch 2 vs 2k), so there is
        # no behaviour to reproduce: the windows are evaluated one at a time here, which is what the sum over a batch would be.
        if context_batch_size < 1:
            raise ValueError(f"context_batch_size must be >= 1, got {context_batch_size}")
        get_context_scheduler(context_schedule)                          # the name is checked here, before the CLIP tower and the VAE run
        # video / strength: video-to-video (denoise's init_latents), `video` = video_length PIL frames preprocessed like the reference image
        if video is not None and len(video) != video_length:
            raise ValueError(f"video has {len(video)} frames, video_length is {video_length}: they must be equal")
        # denoise()'s sampling keywords: every refusal is made here too, against the clip's latent shape and the UNet's blocks, before anything runs
        loop_kw = dict(guidance_rescale=guidance_rescale, strength=strength, context_fuse=context_fuse, free_init_iters=free_init_iters,
                       free_init_filter=free_init_filter, free_init_order=free_init_order, free_init_spatial_stop=free_init_spatial_stop,
                       free_init_temporal_stop=free_init_temporal_stop, free_init_fast=free_init_fast, apg=apg, apg_eta=apg_eta,
                       apg_norm_threshold=apg_norm_threshold, apg_momentum=apg_momentum, pag_scale=pag_scale, pag_adaptive_scale=pag_adaptive_scale,
                       pag_applied_layers=pag_applied_layers, kv_downsample=kv_downsample, kv_downsample_mode=kv_downsample_mode,
                       seg_scale=seg_scale, seg_blur_sigma=seg_blur_sigma, seg_applied_layers=seg_applied_layers, tile_attention=tile_attention,
                       tile_attention_shift=tile_attention_shift, deep_cache_interval=deep_cache_interval, deep_cache_depth=deep_cache_depth,
                       guidance_interval=guidance_interval, uncond_cache_interval=uncond_cache_interval, deep_cache_threshold=deep_cache_threshold)
        hires =self.hires_plan(height or 768, width or 768, num_inference_steps, hires_scale, hires_strength, hires_mode, hires_steps)
        if hires is None:
            self._resolve_plan(self.sampling_plan(num_inference_steps, guidance_scale, video is not None,
                                                  (video_length, (height or 768) // 8, (width or 768) // 8), sampler=self._sampler(), eta=eta, **loop_kw))
        else:
            # two passes, two plans: both are built and resolved here, before the CLIP tower or the VAE runs
            if video is not None:
                raise ValueError("video= cannot be combined with hires_scale > 1: pass 2 is itself the video-to-video pass, from pass 1's result")
            height_lo, width_lo, steps_hi = hires
            hi_kw = dict(loop_kw, strength=hires_strength, free_init_iters=1)     # FreeInit refuses init_latents: pass 1 only
            for what, steps, has_init, (hp, wp), kw in ((f"hires pass 1 ({width_lo} x {height_lo})", num_inference_steps, False, (height_lo, width_lo), loop_kw),
                                                        (f"hires pass 2 ({width or 768} x {height or 768})", steps_hi, True, (height or 768, width or 768), hi_kw)):
                try:
                    self._resolve_plan(self.sampling_plan(steps, guidance_scale, has_init, (video_length, hp // 8, wp // 8), sampler=self._sampler(), eta=eta, **kw))
                except ValueError as e:
                    raise ValueError(f"{what}: {e}") from None
            if scene_motion_lowres_npy is not None and tuple(np.shape(scene_motion_lowres_npy)) != (video_length, 2, height_lo // 8, width_lo // 8):
                raise ValueError(f"scene_motion_lowres_npy has shape {tuple(np.shape(scene_motion_lowres_npy))}, pass 1 needs "
                                 f"{(video_length, 2, height_lo // 8, width_lo // 8)}")
        color_plan = self.color_match_plan(color_match, color_match_strength, color_match_target, color_match_scope, ref_image, height or 768,
                                           width or 768, num_images_per_prompt)
        if context_batch_size > 1 and not getattr(self, "_warned_context_batch", False):
            import warnings
            warnings.warn("context_batch_size > 1: the windows of a context batch are evaluated one at a time (the reference itself "
                          "fails for two or more windows per batch, pipeline_mikudance.py:662); results are those of context_batch_size = 1")
            self._warned_context_batch = True
        # vae_tiling / vae_tile_size: checked against every size this call runs the VAE at, in force inside the block only
        sizes = [(height or 768, width or 768)] + ([] if hires is None else [(hires[0], hires[1])])
        with self.vae_tiling_scope(sizes, vae_tiling, vae_tile_size):
            height = height or 768
            width = width or 768
            device = self._execution_device
            do_cfg = guidance_scale > 1.0
            batch_size = 1
            image_prompt_embeds = self.clip_embeds(ref_image)
            if do_cfg:
                image_prompt_embeds = torch.cat([torch.zeros_like(image_prompt_embeds), image_prompt_embeds], dim=0)
            images = (ref_image, ref_skel_image, [list(tgt_pose_images), list(tgt_face_images), list(tgt_hand_images)])
            noise_args = (video_length, image_prompt_embeds.dtype, device, generator)
            window_args = (context_schedule, context_frames, context_stride, context_overlap)
            if hires is None:
                latents = self.prepare_latents(batch_size * num_images_per_prompt, self.denoising_unet.in_channels, width, height, *noise_args)
                # (the noise is drawn before the video-to-video frames are encoded, so the generator stream does not depend on video=)
                ref_latents, init_latents = self._condition_latents(*images, video, scene_motion_npy, height, width, video_length)
                latents = self.denoise(latents, ref_latents, image_prompt_embeds, num_inference_steps, guidance_scale, *window_args, callback,
                                       callback_steps, eta=eta, generator=generator, init_latents=init_latents, **loop_kw)
            else:
                # the noise of the low size FIRST, then of the full size (the order the docstring states); the images of each size through the VAE
                # in batches of their own; the CLIP embeddings above serve both passes
                noise_lo = self.prepare_latents(batch_size * num_images_per_prompt, self.denoising_unet.in_channels, width_lo, height_lo, *noise_args)
                noise = self.prepare_latents(batch_size * num_images_per_prompt, self.denoising_unet.in_channels, width, height, *noise_args)
                motion_lo = scene_motion_lowres_npy
                if motion_lo is None:
                    motion_lo = self.lowres_scene_motion(scene_motion_npy, height_lo // 8, width_lo // 8)
                ref_latents_lo, _ = self._condition_latents(*images, None, motion_lo, height_lo, width_lo, video_length)
                ref_latents, _ = self._condition_latents(*images, None, scene_motion_npy, height, width, video_length)
                latents = self.denoise(noise_lo, ref_latents_lo, image_prompt_embeds, num_inference_steps, guidance_scale, *window_args, callback,
                                       callback_steps, eta=eta, generator=generator, init_latents=None, **loop_kw)
                latents = self.upscale_latents(latents, height, width, hires_mode)
                callback_hi = None if callback is None else (lambda i, t, x: callback(num_inference_steps + i, t, x))
                latents = self.denoise(noise, ref_latents, image_prompt_embeds, steps_hi, guidance_scale, *window_args, callback_hi,
                                       callback_steps, eta=eta, generator=generator, init_latents=latents, **hi_kw)
            if interpolation_factor > 0:
                latents = self.interpolate_latents(latents, interpolation_factor, device)
            if color_plan is not None:
                # colour matched on the device between the decode and the quantisation (md_color_moments / md_color_apply)
                images = self._decode_color_matched(latents, self.decode_chunk_size if self.video_decoder else self.vae_batch, color_plan,
                                                    temporal=bool(self.video_decoder), as_bytes=output_type in ("uint8", "pil"))
            elif output_type in ("uint8", "pil"):
                # frames quantised on the device (md_frames_u8), in the layout the writers take: half the bytes of the fp16 transfer, a quarter of the fp32 host array's
                images = self.decode_temporal(latents, output_type="uint8") if self.video_decoder else self.decode_latents(latents, output_type="uint8")
            else:
                images = self.decode_temporal(latents) if self.video_decoder else self.decode_latents(latents)
            if output_type == "pil":
                from PIL import Image
                images = [[Image.fromarray(frame.numpy()) for frame in clip] for clip in images]
            if output_type == "tensor":
                images = torch.from_numpy(images)
            if not return_dict:
                return images
            return MikuDanceVideoPipelineOutput(videos=images)
