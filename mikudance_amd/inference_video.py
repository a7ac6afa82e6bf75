"""`python -m mikudance_amd.inference_video --config configs/inference/inference_video.yaml [-W 768 -H 768 --steps 30 ...]`

Drop-in for the reference's scripts/inference_video.py (its `main`, :61-234) with every module served by this package: same
command line, same YAML keys, same call order, same output file naming.  Nothing third party is needed beyond what this image
has (no omegaconf / diffusers / PyAV / cv2 / torchvision / scikit-image): see mikudance_amd/io_utils.py for the adapters.

    vae            = AutoencoderKL.from_pretrained(config.pretrained_vae_path)                     (:76-79)
    unet           = UNet2DConditionModel.from_pretrained(base, subfolder="unet")                  (:81-84)  -> UNet2DConditionModelPlain
    reference_unet = UNet2DConditionModel_MIX.from_unet(unet)                                      (:85)
    denoising_unet = UNet3DConditionModel.from_pretrained_2d(base, motion_module_path, subfolder="unet",
                                                             unet_additional_kwargs=infer_config.unet_additional_kwargs)  (:90-95)
    image_enc      = CLIPVisionModelWithProjection.from_pretrained(config.image_encoder_path)      (:97-99)
    scheduler      = DDIMScheduler(**infer_config.noise_scheduler_kwargs)                          (:101-102)
                     (--sampler dpmpp_2m / dpmpp_2m_sde: DPMSolverMultistepScheduler from the same kwargs; --sampler unipc:
                     UniPCMultistepScheduler from the same kwargs with --solver_order and --unipc_solver_type; additions)
    pipe(..., guidance_rescale=--guidance_rescale)                                                 (an addition; default 0.0 = off)
    pipe(..., video=read_frames(--init_video), strength=--strength)                                (an addition: video-to-video)
    pipe(..., context_schedule=, context_fuse=, context_frames=, context_overlap=)                 (additions: how a clip longer than the
                     temporal context is cut into windows and how their overlaps are merged; defaults = the reference's call)
    pipe(..., free_init_iters=, free_init_filter=, free_init_order=, free_init_spatial_stop=, free_init_temporal_stop=, free_init_fast=)
                     (an addition: FreeInit noise re-initialisation, arXiv 2312.07537; default 1 pass = off)
    pipe(..., apg=--apg, apg_eta=, apg_norm_threshold=, apg_momentum=)                             (an addition: adaptive projected guidance,
                     arXiv 2410.02416, per frame on the data prediction; default off)
    pipe(..., pag_scale=--pag_scale, pag_adaptive_scale=--pag_adaptive_scale, pag_applied_layers=--pag_layers)
                     (an addition: perturbed-attention guidance, arXiv 2403.17377; default 0.0 = off)
    pipe(..., kv_downsample=--kv_downsample, kv_downsample_mode=--kv_downsample_mode)
                     (an addition: K / V token downsampling in the spatial self-attention, arXiv 2402.13573; default 1 = off)
    pipe(..., seg_scale=--seg_scale, seg_blur_sigma=--seg_blur_sigma, seg_applied_layers=--seg_layers)
                     (an addition: smoothed-energy guidance, arXiv 2408.00760; default 0.0 = off)
    pipe(..., tile_attention=--tile_attention, tile_attention_shift=--tile_attention_shift)
                     (an addition: shifted-tile spatial self-attention, arXiv 2311.17528; default 1 = off)
    pipe(..., deep_cache_interval=--deep_cache_interval, deep_cache_depth=--deep_cache_depth, deep_cache_threshold=--deep_cache_threshold)
                     (an addition: DeepCache, arXiv 2312.00858: the deep part of the denoising UNet every N-th step only; default 1 = off)
    pipe(..., guidance_interval=--guidance_interval, uncond_cache_interval=--uncond_cache_interval)
                     (an addition: guidance on a stretch of the schedule only, arXiv 2404.07724, and the unconditional half on every N-th guided
                     step only, after arXiv 2410.19355; opt-in approximations, image quality on real weights not assessed; defaults 0,1 and 1 = off)
    pipe(..., hires_scale=--hires_scale, hires_strength=--hires_strength, hires_mode=--hires_mode, hires_steps=--hires_steps,
         scene_motion_lowres_npy=camera_to_scene_motion at the first pass's grid)
                     (an addition: two-pass high-resolution sampling, the whole schedule at -W / S x -H / S, the latents enlarged on the GPU,
                     the tail of the schedule at -W x -H; default 1 = off)
    pipe(..., vae_tiling=--vae_tiling, vae_tile_size=--vae_tile_size)
                     (an addition: tiled VAE encode / decode, diffusers' enable_vae_tiling; default off)
    pipe(..., color_match=--color_match, color_match_strength=--color_match_strength, color_match_scope=--color_match_scope,
         color_match_target=Image.open(--color_match_image) | "first_frame")
                     (an addition: colour matching of the output frames on the GPU toward the reference image; default off)
    pipe(..., output_type="uint8") + save_frames_grid_u8 with --u8_output
                     (an addition: frames quantised on the GPU and kept as bytes up to the writer; the same file; default off)
    *.load_state_dict(torch.load(...))                                                             (:111-117)
    pipe(ref_image, ref_skel, pose, face, hand, scene_motion, W, H, F, steps, cfg, generator)      (:211-224)
    save_videos_grid(cat([ref, pose, video]), ".../{skel}_{ref}_{H}x{W}_{cfg}_{time}.mp4", n_rows=3, fps)     (:228-234)

`--video_decoder` selects mikudance_amd.AutoencoderKLTemporalDecoder (config.pretrained_temporal_vae_path), like the reference (:72-75)."""
import argparse
import os
import warnings
from datetime import datetime
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from . import (AutoencoderKL, AutoencoderKLTemporalDecoder, CLIPVisionModelWithProjection, DDIMScheduler, DPMSolverMultistepScheduler,
               MikuDanceVideoPipeline, UNet2DConditionModel, UNet2DConditionModelPlain, UNet3DConditionModel, UniPCMultistepScheduler)
from .free_init import FILTERS as FREE_INIT_FILTERS
from .io_utils import (frames_to_tensor, frames_to_u8, get_fps, load_config, read_frames, resize_depth, save_frames_grid_u8, save_videos_grid,
                       to_container)
from .scene_motion import camera_to_scene_motion


# --sampler -> the scheduler built from the YAML's noise_scheduler_kwargs (the YAML's own `sampler: DDIM` key stays ignored, as in the
# reference script); "unipc" also takes the solver's own keywords (--solver_order -> solver_order, --unipc_solver_type -> solver_type)
SAMPLERS = {"ddim": lambda kw: DDIMScheduler(**kw),
            "dpmpp_2m": lambda kw: DPMSolverMultistepScheduler.from_config(kw, solver_order=2, algorithm_type="dpmsolver++"),
            "dpmpp_2m_sde": lambda kw: DPMSolverMultistepScheduler.from_config(kw, solver_order=2, algorithm_type="sde-dpmsolver++"),
            "unipc": lambda kw, **solver: UniPCMultistepScheduler.from_config(kw, **solver)}


def _factors(text):
    """--kv_downsample / --tile_attention: "2" or "4,2" -> a tuple of integers (their range is the pipeline's business)."""
    import argparse
    try:
        return tuple(int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected comma-separated integers, got {text!r}") from None


def _interval(text):
    """--guidance_interval: "0.1,0.8" -> (0.1, 0.8) (the range is the pipeline's business)."""
    import argparse
    try:
        lo, hi = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected two comma-separated numbers lo,hi, got {text!r}") from None
    return lo, hi


def _layer_names(text):
    """--pag_layers / --seg_layers: "mid, up_blocks.1" -> a tuple of names (their form is the pipeline's business)."""
    return tuple(n.strip() for n in text.split(",") if n.strip())


def parse_args(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument("--config")
    parser.add_argument("-W", type=int, default=768)
    parser.add_argument("-H", type=int, default=768)
    parser.add_argument("--seed", type=int, default=100)
    parser.add_argument("--cfg", type=float, default=3.5)
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--fps", type=int)
    parser.add_argument("--video_decoder", action="store_true",
                        help="The temporal decoder produces less noise in the results but leads to longer inference times.")
    parser.add_argument("--output_dir", default="output", help="(addition) root of the dated output tree")
    parser.add_argument("--sampler", choices=tuple(SAMPLERS), default="ddim",
                        help="(addition) ddim (the reference's), dpmpp_2m or dpmpp_2m_sde (DPM-Solver++ 2M, ODE / SDE) or unipc (UniPC, "
                             "arXiv 2302.04867: a predictor-corrector multistep solver, no extra UNet evaluation), all built from "
                             "noise_scheduler_kwargs")
    parser.add_argument("--solver_order", type=int, choices=(1, 2, 3), default=2,
                        help="(addition) with --sampler unipc: the order of the predictor (the corrector follows it); 2 = diffusers' default")
    parser.add_argument("--unipc_solver_type", choices=("bh1", "bh2"), default="bh2",
                        help="(addition) with --sampler unipc: B(h) = h (bh1) or expm1(h) (bh2, diffusers' default)")
    parser.add_argument("--guidance_rescale", type=float, default=0.0,
                        help="(addition) phi of rescaled classifier-free guidance (arXiv 2305.08891 section 3.4, diffusers guidance_rescale), "
                             "in [0, 1]; 0.0 = off (the reference's behaviour), 0.7 the paper's value.  Works with every --sampler")
    parser.add_argument("--init_video",
                        help="(addition) video-to-video: a clip to start from, read like the pose video (a frame directory, .npy / .npz, .gif / "
                             ".png, or an .mp4 of this package's own writer; convert H.264 first with `python -m mikudance_amd.io_utils "
                             "convert`).  Its frame count must equal the pose video's")
    parser.add_argument("--strength", type=float, default=1.0,
                        help="(addition) with --init_video: the share of the schedule that is run, in (0, 1] (diffusers img2img strength); "
                             "1.0 starts from pure noise")
    parser.add_argument("--context_schedule", choices=("uniform", "uniform_open"), default="uniform",
                        help="(addition) windows of a clip longer than --context_frames: uniform (the reference's: a closed loop, windows "
                             "wrap round the end of the clip) or uniform_open (no window wraps; fewer windows)")
    parser.add_argument("--context_fuse", choices=("flat", "pyramid"), default="flat",
                        help="(addition) how overlapping windows are merged per frame: flat (the reference's plain average) or pyramid "
                             "(triangular weight per window slot, diffusers FreeNoise weighting_scheme='pyramid')")
    parser.add_argument("--context_frames", type=int, default=None,
                        help="(addition) frames per window; default: the pipeline's (30, the motion module's temporal context)")
    parser.add_argument("--context_overlap", type=int, default=8, help="(addition) frames shared by neighbouring windows")
    parser.add_argument("--free_init_iters", type=int, default=1,
                        help="(addition) FreeInit (arXiv 2312.07537, diffusers enable_free_init): sampling passes; before every pass after the "
                             "first the result is re-noised and only its low spatio-temporal frequencies are kept.  1 = off, 3 diffusers' value")
    parser.add_argument("--free_init_filter", choices=FREE_INIT_FILTERS, default="butterworth", help="(addition) FreeInit's low-pass filter")
    parser.add_argument("--free_init_order", type=int, default=4, help="(addition) order of the butterworth filter")
    parser.add_argument("--free_init_spatial_stop", type=float, default=0.25, help="(addition) FreeInit: normalised spatial stop frequency")
    parser.add_argument("--free_init_temporal_stop", type=float, default=0.25, help="(addition) FreeInit: normalised temporal stop frequency")
    parser.add_argument("--free_init_fast", action="store_true",
                        help="(addition) FreeInit: pass i of n runs int(steps / n * (i + 1)) steps (diffusers use_fast_sampling)")
    parser.add_argument("--apg", action="store_true",
                        help="(addition) adaptive projected guidance (arXiv 2410.02416, diffusers AdaptiveProjectedGuidance) in place of plain "
                             "classifier-free guidance, per frame on the data prediction.  Works with every --sampler; not with "
                             "--guidance_rescale")
    parser.add_argument("--apg_eta", type=float, default=0.0,
                        help="(addition) APG: weight of the part of the guidance update parallel to the conditional prediction, in [0, 1]")
    parser.add_argument("--apg_norm_threshold", type=float, default=0.0,
                        help="(addition) APG: cap on the per-frame norm of the guidance update, >= 0; 0 = no cap")
    parser.add_argument("--apg_momentum", type=float, default=0.0,
                        help="(addition) APG: momentum of the update's running average over steps, in (-1, 1); the paper uses a negative value")
    parser.add_argument("--pag_scale", type=float, default=0.0,
                        help="(addition) perturbed-attention guidance (arXiv 2403.17377, diffusers PAGMixin): the weight of the step away from a "
                             "second conditional prediction made with the self-attention map of --pag_layers replaced by the identity, >= 0; "
                             "0.0 = off, 3.0 the paper's value.  Works with every --sampler and without --cfg; not with --guidance_rescale or --apg")
    parser.add_argument("--pag_adaptive_scale", type=float, default=0.0,
                        help="(addition) PAG: decay of the scale per timestep below 1000 (diffusers pag_adaptive_scale), >= 0; 0.0 = none")
    parser.add_argument("--pag_layers", default="mid",
                        help="(addition) PAG: comma-separated attention blocks of the denoising UNet, e.g. mid or "
                             "down_blocks.2,up_blocks.1.attentions.0")
    parser.add_argument("--kv_downsample", type=_factors, default=(1,), metavar="N[,N...]",
                        help="(addition) K / V token downsampling in the spatial self-attention of the denoising UNet (ToDo, arXiv 2402.13573), "
                             "an approximation that saves attention time at high resolution: one integer factor 1..8 per resolution level from "
                             "the highest down, e.g. 2 or 4,2; 1 = off")
    parser.add_argument("--kv_downsample_mode", choices=("nearest", "mean"), default="nearest",
                        help="(addition) how the K / V token grid is reduced: nearest (the paper's) or the mean of each block")
    parser.add_argument("--tile_attention", type=_factors, default=(1,), metavar="N[,N...]",
                        help="(addition) shifted-tile spatial self-attention in the denoising UNet (MSW-MSA of HiDiffusion, arXiv 2311.17528), "
                             "an approximation that saves attention time at high resolution: one integer 1..8 per resolution level from the "
                             "highest down, the number of tiles per axis, e.g. 2 or 2,2; it must divide the level's token grid; 1 = off")
    parser.add_argument("--tile_attention_shift", choices=("cycle", "none"), default="cycle",
                        help="(addition) how the tiling moves from step to step: cycle (a quarter tile further every step, period 4) or none")
    parser.add_argument("--seg_scale", type=float, default=0.0,
                        help="(addition) smoothed-energy guidance scale (SEG, arXiv 2408.00760): steer away from a second conditional "
                             "prediction made with the self-attention queries of --seg_layers Gaussian-blurred over the token grid, >= 0; "
                             "0.0 = off; not with --pag_scale, --guidance_rescale or --apg")
    parser.add_argument("--seg_blur_sigma", type=float, default=100.0,
                        help="(addition) SEG: sigma of the query blur in tokens, > 0; inf = every query becomes its frame's mean query")
    parser.add_argument("--seg_layers", default="mid",
                        help="(addition) SEG: comma-separated attention blocks of the denoising UNet, as --pag_layers")
    parser.add_argument("--deep_cache_interval", type=int, default=1, metavar="N",
                        help="(addition) DeepCache (arXiv 2312.00858), an approximation that saves the deep levels of the denoising UNet: only "
                             "every N-th step evaluates the whole UNet, the steps between run its outermost layers on the deep hidden state "
                             "of the last full step; 1 = off")
    parser.add_argument("--deep_cache_depth", type=int, default=3, metavar="D",
                        help="(addition) DeepCache: how many skip connections, counted from conv_in, the steps between still evaluate "
                             "(this project's own index); 3 = the whole highest-resolution level on both sides")
    parser.add_argument("--deep_cache_threshold", type=float, default=None, metavar="R",
                        help="(addition) adaptive DeepCache (the accumulated relative-L1 rule of TeaCache, arXiv 2411.19108): a step evaluates "
                             "the whole UNet when the relative change of its first skipped feature map, summed since the last full step, reaches "
                             "R (> 0); --deep_cache_interval N (>= 2) then caps the shallow steps in a row at N - 1.  One host synchronisation "
                             "per UNet call.  Default: the fixed every-N-th rule")
    parser.add_argument("--guidance_interval", type=_interval, default=(0.0, 1.0), metavar="LO,HI",
                        help="(addition) guidance in a limited interval (arXiv 2404.07724), an approximation that saves the unconditional half "
                             "of the denoising UNet: classifier-free guidance is applied at step k of --steps N only where LO N <= k < HI N, the "
                             "other steps run on the conditional prediction alone; 0 <= LO <= HI <= 1; 0,1 = off.  Image quality on real "
                             "weights has not been assessed.  Not with --deep_cache_interval")
    parser.add_argument("--uncond_cache_interval", type=int, default=1, metavar="N",
                        help="(addition) reuse of the guidance direction (the CFG cache of FasterCache, arXiv 2410.19355), an approximation: the "
                             "unconditional half is evaluated on every N-th guided step only, the steps between reuse the last difference "
                             "between the conditional and the unconditional prediction; 1 = off.  Image quality on real weights has not been "
                             "assessed.  Not with --deep_cache_interval")
    parser.add_argument("--hires_scale", type=float, default=1.0, metavar="S",
                        help="(addition) two-pass high-resolution sampling, an approximation that saves most full-resolution steps: the whole "
                             "schedule runs at -W / S x -H / S (rounded to multiples of 8), the latents are enlarged on the GPU and re-noised, and "
                             "only the last --hires_strength of the schedule runs at -W x -H; 1 = off.  Not with --init_video")
    parser.add_argument("--hires_strength", type=float, default=0.5,
                        help="(addition) with --hires_scale: the share of the second pass's schedule that is run, in (0, 1)")
    parser.add_argument("--hires_mode", choices=("nearest", "bilinear", "bicubic"), default="bicubic",
                        help="(addition) with --hires_scale: how the latents are enlarged")
    parser.add_argument("--hires_steps", type=int, default=None,
                        help="(addition) with --hires_scale: steps of the second pass's schedule before --hires_strength cuts it; default --steps")
    parser.add_argument("--vae_tiling", action="store_true",
                        help="(addition) tiled VAE encode / decode (diffusers' enable_vae_tiling): overlapping tiles with blended seams, so that "
                             "memory and the VAE's attention scale with the tile and not with -W x -H.  A different result by design (each "
                             "tile is normalised on its own); image quality on real weights has not been assessed.  Not with --video_decoder")
    parser.add_argument("--vae_tile_size", type=int, default=None, metavar="PIXELS",
                        help="(addition) with --vae_tiling: the tile side in image pixels, a multiple of 32; default: the VAE's sample_size")
    parser.add_argument("--u8_output", action="store_true",
                        help="(addition) take the frames from the pipeline as uint8 (output_type='uint8': quantised on the GPU, a quarter of the "
                             "bytes of the float32 clip on the host) and write the grid video from bytes; the file is byte-identical to the default's")
    parser.add_argument("--color_match", choices=["mean_std", "mkl"], default=None,
                        help="(addition) colour matching of the output frames on the GPU (ComfyUI's ColorMatch, A1111's 'apply color correction'): "
                             "every frame gets an affine colour transfer toward the reference image (or --color_match_image) before it is "
                             "quantised; mean_std matches each channel's mean and standard deviation, mkl the whole colour covariance "
                             "(Monge-Kantorovich).  Image quality on real weights has not been assessed; default off")
    parser.add_argument("--color_match_strength", type=float, default=1.0, metavar="A",
                        help="(addition) with --color_match: blend between the frames as they are (0) and the full transfer (1)")
    parser.add_argument("--color_match_scope", choices=["frame", "clip"], default="frame",
                        help="(addition) with --color_match: one transform per frame, or one for the whole clip from the frames' summed "
                             "statistics (removes the global drift, keeps the clip's own variation over time)")
    parser.add_argument("--color_match_image", type=str, default=None, metavar="PATH",
                        help="(addition) with --color_match: the target image, or 'first_frame' for the clip's own first frame (Deforum's "
                             "colour coherence); default: the reference image")
    args = parser.parse_args(argv)
    if args.color_match is None and (args.color_match_strength != 1.0 or args.color_match_scope != "frame" or args.color_match_image is not None):
        parser.error("--color_match_strength / --color_match_scope / --color_match_image need --color_match")
    if args.vae_tile_size is not None and not args.vae_tiling:
        parser.error(f"--vae_tile_size {args.vae_tile_size} needs --vae_tiling")
    if args.vae_tiling and args.video_decoder:
        parser.error("--vae_tiling cannot be combined with --video_decoder: the temporal decoder has no tiling")
    if args.strength != 1.0 and args.init_video is None:
        parser.error(f"--strength {args.strength} needs --init_video")
    if args.hires_scale != 1.0 and args.init_video is not None:
        parser.error("--hires_scale cannot be combined with --init_video: the second pass is itself the video-to-video pass")
    return args


def _none(v):
    return v is None or v == "None"


def build_scheduler(infer_config, sampler="ddim", **solver):
    """scripts/inference_video.py:101-102 (`--sampler ddim`), or the DPM-Solver++ 2M / UniPC scheduler from the same keyword arguments.
    solver: with "unipc" only, the solver's own keywords (solver_order, solver_type, disable_corrector)."""
    if solver and sampler != "unipc":
        raise ValueError(f"sampler {sampler!r} takes no solver keywords, got {sorted(solver)}")
    return SAMPLERS[sampler](to_container(infer_config.noise_scheduler_kwargs), **solver)


def build_pipeline(config, infer_config, weight_dtype, device="cuda", video_decoder=False, sampler="ddim", solver=None):
    """scripts/inference_video.py:72-130.  solver: build_scheduler's keywords for `sampler`."""
    if video_decoder:
        vae = AutoencoderKLTemporalDecoder.from_pretrained(config.pretrained_temporal_vae_path).to(device, dtype=weight_dtype)
    else:
        vae = AutoencoderKL.from_pretrained(config.pretrained_vae_path).to(device, dtype=weight_dtype)
    unet = UNet2DConditionModelPlain.from_pretrained(config.pretrained_base_model_path, subfolder="unet")
    reference_unet = UNet2DConditionModel.from_unet(unet)
    del unet
    denoising_unet = UNet3DConditionModel.from_pretrained_2d(
        config.pretrained_base_model_path, config.motion_module_path, subfolder="unet",
        unet_additional_kwargs=infer_config.unet_additional_kwargs).to(dtype=weight_dtype, device=device)
    image_enc = CLIPVisionModelWithProjection.from_pretrained(config.image_encoder_path).to(dtype=weight_dtype, device=device)
    scheduler = build_scheduler(infer_config, sampler, **(solver or {}))
    denoising_unet.load_state_dict(torch.load(config.denoising_unet_path, map_location="cpu", weights_only=True), strict=False)
    reference_unet.load_state_dict(torch.load(config.reference_unet_path, map_location="cpu", weights_only=True))
    denoising_unet.eval()
    reference_unet.eval()
    pipe = MikuDanceVideoPipeline(vae=vae, image_encoder=image_enc, reference_unet=reference_unet, denoising_unet=denoising_unet,
                                  scheduler=scheduler, video_decoder=video_decoder)
    return pipe.to(device, dtype=weight_dtype)


def main(argv=None):
    args = parse_args(argv)
    config = load_config(args.config)
    weight_dtype = torch.float16 if config.weight_dtype == "fp16" else torch.float32
    if weight_dtype != torch.float16:
        # reference scripts/inference_video.py:66-69 runs the whole model in fp32 then.  Here parameters, latents and images keep
        # the requested dtype at every module boundary, and the kernels underneath still round operands to fp16 and accumulate in
        # fp32: over the 20-step loop that is 2.4e-3 relative L2 from the fp32 restatement (profiles/r04_e2e_parity.json)
        warnings.warn("weight_dtype: fp32 -- tensors are kept in fp32 at the module boundaries; the MI355X kernels compute with fp16 "
                      "operands and fp32 accumulation")
    infer_config = load_config(config.inference_config)
    generator = torch.manual_seed(args.seed)
    width, height = args.W, args.H
    assert width % 8 == 0 and height % 8 == 0      # the vae works at 1/8 resolution (scripts/inference_video.py:108)
    solver = dict(solver=dict(solver_order=args.solver_order, solver_type=args.unipc_solver_type)) if args.sampler == "unipc" else {}
    pipe = build_pipeline(config, infer_config, weight_dtype, video_decoder=args.video_decoder, sampler=args.sampler, **solver)

    date_str = datetime.now().strftime("%Y%m%d")
    time_str = datetime.now().strftime("%H%M%S")
    save_dir = Path(f"{args.output_dir}/{date_str}/{time_str}--seed_{args.seed}-{args.W}x{args.H}")
    save_dir.mkdir(exist_ok=True, parents=True)

    if _none(config.tgt_pose_path):
        raise ValueError("Target pose is required!")
    pose_pils = read_frames(config.tgt_pose_path)
    src_fps = get_fps(config.tgt_pose_path)
    num_frames = len(pose_pils)
    black = lambda: [Image.new("RGB", pose_pils[0].size, (0, 0, 0)) for _ in range(num_frames)]
    face_pils = black() if _none(config.get("tgt_face_path")) else read_frames(config.tgt_face_path)
    hand_pils = black() if _none(config.get("tgt_hand_path")) else read_frames(config.tgt_hand_path)
    if _none(config.get("tgt_w2c_path")) or _none(config.get("tgt_c2w_path")):
        w2c_npy = np.eye(4).reshape((1, 4, 4)).repeat(num_frames, axis=0)
        c2w_npy = np.eye(4).reshape((1, 4, 4)).repeat(num_frames, axis=0)
    else:
        w2c_npy, c2w_npy = np.load(config.tgt_w2c_path), np.load(config.tgt_c2w_path)
    depth_map = np.zeros((1, height, width)) if _none(config.get("ref_depth_path")) else np.load(config.ref_depth_path)
    w2cs, c2ws = [w2c_npy[k] for k in range(w2c_npy.shape[0])], [c2w_npy[k] for k in range(c2w_npy.shape[0])]
    scene_motion_npy = camera_to_scene_motion(w2cs, c2ws, [3.2, 3.2, 1.6, 1.6], resize_depth(depth_map, (1, height // 8, width // 8)), width // 8,
                                              height // 8, False)
    # --hires_scale: the first pass gets the EXACT flow of its own grid (the depth map resized to it), not the pipeline's resampled one
    scene_motion_lowres_npy = None
    hires = pipe.hires_plan(height, width, args.steps, args.hires_scale, args.hires_strength, args.hires_mode, args.hires_steps)
    if hires is not None:
        h_lo, w_lo = hires[0] // 8, hires[1] // 8
        scene_motion_lowres_npy = camera_to_scene_motion(w2cs, c2ws, [3.2, 3.2, 1.6, 1.6], resize_depth(depth_map, (1, h_lo, w_lo)), w_lo, h_lo, False)
    print("Total frames: {}".format(num_frames))
    init_pils = None
    if args.init_video is not None:
        init_pils = read_frames(args.init_video)
        if len(init_pils) != num_frames:
            raise ValueError(f"--init_video has {len(init_pils)} frames, the pose video {num_frames}: they must be equal")

    skel_name = os.path.splitext(os.path.basename(config.tgt_pose_path))[0]
    ref_name = os.path.splitext(os.path.basename(config.ref_image_path))[0]
    ref_image_pil = Image.open(config.ref_image_path).convert("RGB")
    ref_skel_pil = Image.open(config.ref_skel_path).convert("RGB")
    if args.u8_output:                                                     # (1, f, h, w, 3) bytes; the float clips are never made
        pose_tensor = frames_to_u8(pose_pils, height, width)
        ref_image_tensor = frames_to_u8([ref_image_pil], height, width).repeat(1, num_frames, 1, 1, 1)
    else:
        pose_tensor = frames_to_tensor(pose_pils, height, width)
        ref_image_tensor = frames_to_tensor([ref_image_pil], height, width).repeat(1, 1, num_frames, 1, 1)
    color_kw = {}
    if args.color_match is not None:                                       # passed only when asked for: the default call keeps its keywords
        target = args.color_match_image
        if target is not None and target != "first_frame":
            target = Image.open(target).convert("RGB")
        color_kw = dict(color_match=args.color_match, color_match_strength=args.color_match_strength, color_match_scope=args.color_match_scope,
                        color_match_target=target)

    out = pipe(ref_image_pil, ref_skel_pil, pose_pils, face_pils, hand_pils, scene_motion_npy, width, height, num_frames,
               args.steps, args.cfg, generator=generator, guidance_rescale=args.guidance_rescale,
               video=init_pils, strength=args.strength, context_schedule=args.context_schedule, context_fuse=args.context_fuse,
               context_frames=args.context_frames, context_overlap=args.context_overlap, free_init_iters=args.free_init_iters,
               free_init_filter=args.free_init_filter, free_init_order=args.free_init_order, free_init_spatial_stop=args.free_init_spatial_stop,
               free_init_temporal_stop=args.free_init_temporal_stop, free_init_fast=args.free_init_fast,
               apg=args.apg, apg_eta=args.apg_eta, apg_norm_threshold=args.apg_norm_threshold, apg_momentum=args.apg_momentum,
               pag_scale=args.pag_scale, pag_adaptive_scale=args.pag_adaptive_scale, pag_applied_layers=_layer_names(args.pag_layers),
               kv_downsample=args.kv_downsample, kv_downsample_mode=args.kv_downsample_mode,
               seg_scale=args.seg_scale, seg_blur_sigma=args.seg_blur_sigma, seg_applied_layers=_layer_names(args.seg_layers),
               tile_attention=args.tile_attention, tile_attention_shift=args.tile_attention_shift,
               deep_cache_interval=args.deep_cache_interval, deep_cache_depth=args.deep_cache_depth,
               deep_cache_threshold=args.deep_cache_threshold, guidance_interval=args.guidance_interval, uncond_cache_interval=args.uncond_cache_interval,
               hires_scale=args.hires_scale, hires_strength=args.hires_strength, hires_mode=args.hires_mode, hires_steps=args.hires_steps,
               scene_motion_lowres_npy=scene_motion_lowres_npy, vae_tiling=args.vae_tiling, vae_tile_size=args.vae_tile_size,
               **(dict(output_type="uint8") if args.u8_output else {}), **color_kw)
    video = torch.cat([ref_image_tensor, pose_tensor, out.videos], dim=0)
    path = f"{save_dir}/{skel_name}_{ref_name}_{args.H}x{args.W}_{int(args.cfg)}_{time_str}.mp4"
    (save_frames_grid_u8 if args.u8_output else save_videos_grid)(video, path, n_rows=3, fps=src_fps if args.fps is None else args.fps)
    return path


if __name__ == "__main__":
    main()
