#!/usr/bin/env python
"""Per-clip denoising-loop time of each sampler at BASELINE.json configs[1] (768 x 768, 16 frames, CFG 3.5, full-width UNets, seeded
weights): DDIM-20 (the headline), DPM-Solver++ 2M-10 and 2M-20.  One warm-up loop per sampler, then --reps timed loops, each bracketed
by HIP events on the current stream; prints one JSON line.  --guidance_rescale PHI (> 0) times every sampler with and without guidance
rescale, the two alternated rep by rep after one warm-up loop each, and adds the cost of the rescale per clip and per step.  --strength S
(< 1) does the same for video-to-video (denoise(init_latents=, strength=S) against the plain loop) and adds the VAE encode of the F extra
frames that __call__(video=) puts in front of the loop (sd-vae-ft-mse geometry, seeded weights, median of three after a warm-up).

    python tools/time_samplers.py [--reps 2] [--guidance_rescale 0.7 | --strength 0.5] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLERS = (("ddim", 20), ("dpmpp_2m", 10), ("dpmpp_2m", 20))
WINDOW_MODES = (("uniform", "flat"), ("uniform_open", "flat"), ("uniform_open", "pyramid"))


def time_windows(a):
    """configs[4] per clip under each (context_schedule, context_fuse) of WINDOW_MODES; one JSON record."""
    from mikudance_amd import DDIMScheduler, MikuDanceVideoPipeline, _lib, ops
    from mikudance_amd.context import get_context_scheduler
    from mikudance_amd.selftest import SCHED_KWARGS, build_models
    from mikudance_amd.synth import synth_inputs
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    frames, size, steps, ctx, overlap = a.window_frames, a.window_size, a.window_steps, 30, 8
    ref, den, _, _ = build_models(geom=dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768), device=dev,
                                  keep_state_dicts=False)
    h = size // 8
    lat, rl, emb = (t.half().to(dev) for t in synth_inputs(frames, h, h, ctx_len=257, ctx_dim=768, seed=100))
    pipe = MikuDanceVideoPipeline(None, None, ref, den, DDIMScheduler(**SCHED_KWARGS))
    kw = lambda m: dict(context_schedule=m[0], context_fuse=m[1], context_frames=ctx, context_stride=1, context_overlap=overlap)
    rec = {"config": {"frames": frames, "size": size, "steps": steps, "guidance": 3.5, "context_frames": ctx, "context_overlap": overlap,
                      "reps": a.reps},
           "windows": {name: len(list(get_context_scheduler(name)(0, steps, frames, ctx, 1, overlap))) for name in ("uniform", "uniform_open")},
           "ms_per_clip": {}}

    def timed(m):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pipe.denoise(lat, rl, emb, steps, 3.5, **kw(m))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for m in WINDOW_MODES:
        pipe.denoise(lat, rl, emb, steps, 3.5, **kw(m))                             # warm-up
    torch.cuda.synchronize()
    times = {m: [] for m in WINDOW_MODES}
    for _ in range(a.reps):
        for m in WINDOW_MODES:                                                       # alternated: drift hits all alike
            times[m].append(timed(m))
    for m in WINDOW_MODES:
        rec["ms_per_clip"]["/".join(m)] = {"min": min(times[m]), "all": times[m]}
        print(f"{m}: {times[m]}", file=sys.stderr, flush=True)
    best = {m: min(times[m]) for m in WINDOW_MODES}
    rec["open_over_closed"] = best[WINDOW_MODES[1]] / best[WINDOW_MODES[0]]
    rec["pyramid_over_flat"] = best[WINDOW_MODES[2]] / best[WINDOW_MODES[1]]
    # the two accumulate launches alone: one window of `ctx` slots, both clip-halves, on this clip's buffers
    hw = h * h
    pred = torch.randn((2 * ctx, hw, 4), device=dev).half()
    ns, cnt = torch.zeros((2, frames, hw, 4), device=dev), torch.zeros((frames,), device=dev)
    win = torch.arange(ctx, dtype=torch.int32, device=dev)
    wts = torch.full((ctx,), 0.5, device=dev)
    launch = {"md_window_accumulate": lambda: ops.window_accumulate(pred, ns, cnt, win, ctx, frames, hw),
              "md_window_accumulate_weighted": lambda: ops.window_accumulate_weighted(pred, ns, cnt, win, wts, ctx, frames, hw)}
    rec["accumulate_us_per_launch"] = {}
    for _ in range(2):                                                               # the second pass is the one kept
        for name, fn in launch.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            torch.cuda.synchronize()
            rec["accumulate_us_per_launch"][name] = e0.elapsed_time(e1) * 1000.0 / 200
    rec["accumulate_bytes_per_launch"] = 2 * ctx * hw * 4 * (2 + 4 + 4)
    rec["device"] = torch.cuda.get_device_name(0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--guidance_rescale", type=float, default=0.0)
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--windows", action="store_true", help="time one long clip under the three window schedule / fuse pairs instead")
    ap.add_argument("--window_frames", type=int, default=48)
    ap.add_argument("--window_size", type=int, default=1024)
    ap.add_argument("--window_steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.windows:
        assert torch.cuda.is_available(), "needs an MI355X"
        rec = time_windows(a)
        print(json.dumps(rec))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(rec, fh, indent=1)
        return
    if a.guidance_rescale > 0 and a.strength < 1:
        ap.error("--guidance_rescale and --strength: one at a time")
    assert torch.cuda.is_available(), "needs an MI355X"
    from mikudance_amd import DDIMScheduler, DPMSolverMultistepScheduler, MikuDanceVideoPipeline, _lib
    from mikudance_amd.selftest import SCHED_KWARGS, build_models
    from mikudance_amd.synth import synth_inputs
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ref, den, _, _ = build_models(geom=dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768), device=dev,
                                  keep_state_dicts=False)
    h = a.size // 8
    lat, rl, emb = (t.half().to(dev) for t in synth_inputs(a.frames, h, h, ctx_len=257, ctx_dim=768, seed=100))
    phis = (0.0, a.guidance_rescale) if a.guidance_rescale > 0 else (0.0,)
    if a.strength < 1:                                                               # a clean latent to start from
        init = (torch.randn(lat.shape, generator=torch.Generator().manual_seed(101)) * 0.8).half().to(dev)
        phis = (0.0, ("strength", a.strength))
    rec = {"config": {"frames": a.frames, "size": a.size, "guidance": 3.5, "reps": a.reps, "guidance_rescale": a.guidance_rescale,
                      "strength": a.strength}, "ms_per_clip": {}}

    def kwargs(phi):
        return dict(init_latents=init, strength=phi[1]) if isinstance(phi, tuple) else dict(guidance_rescale=phi)

    def timed(pipe, steps, phi):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pipe.denoise(lat, rl, emb, steps, 3.5, **kwargs(phi))
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for name, steps in SAMPLERS:
        sch = DDIMScheduler(**SCHED_KWARGS) if name == "ddim" else DPMSolverMultistepScheduler(**SCHED_KWARGS)
        pipe = MikuDanceVideoPipeline(None, None, ref, den, sch)
        for phi in phis:
            pipe.denoise(lat, rl, emb, steps, 3.5, **kwargs(phi))                   # warm-up
        torch.cuda.synchronize()
        times = {phi: [] for phi in phis}
        for _ in range(a.reps):
            for phi in phis:                                                         # alternated: drift hits both alike
                times[phi].append(timed(pipe, steps, phi))
        for phi in phis:
            key = f"{name}-{steps}" + (f"-strength{phi[1]:g}" if isinstance(phi, tuple) else f"-rescale{phi:g}" if phi else "")
            rec["ms_per_clip"][key] = {"min": min(times[phi]), "all": times[phi]}
            print(f"{key}: {times[phi]}", file=sys.stderr, flush=True)
        if len(phis) == 2:
            d = min(times[phis[1]]) - min(times[0.0])
            if isinstance(phis[1], tuple):
                rec.setdefault("strength_ratio", {})[f"{name}-{steps}"] = min(times[phis[1]]) / min(times[0.0])
            else:
                rec.setdefault("rescale_cost", {})[f"{name}-{steps}"] = {"ms_per_clip": d, "ms_per_step": d / steps}
    if a.strength < 1:                                                               # __call__(video=): F more images through the VAE
        import time
        from mikudance_amd import AutoencoderKL
        from mikudance_amd.synth import synth_state_dict
        vae = AutoencoderKL()
        vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=77), strict=True)
        vae = vae.half().to(dev).eval()
        vpipe = MikuDanceVideoPipeline(vae, None, None, None, None)
        g = torch.Generator(device=dev).manual_seed(7)
        imgs = (torch.rand(a.frames, 3, a.size, a.size, device=dev, generator=g) * 2 - 1).half()
        views = [imgs[i:i + 1] for i in range(a.frames)]
        times = []
        with torch.no_grad():
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                vpipe._encode_many(views)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
        rec["video_encode_ms_per_clip"] = sorted(times[1:])[1]
        del vae, vpipe
    if len(phis) == 2 and not isinstance(phis[1], tuple):                                                               # the statistics launches alone, on this clip's shape
        from mikudance_amd import ops
        ns = torch.randn((2, a.frames, h * h, 4), device=dev)
        cnt = torch.ones((a.frames,), device=dev)
        f = ops.cfg_guidance_rescale(ns, cnt, a.frames, h * h, 3.5, a.guidance_rescale)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            ops.cfg_guidance_rescale(ns, cnt, a.frames, h * h, 3.5, a.guidance_rescale, out=f)
        e1.record()
        torch.cuda.synchronize()
        rec["rescale_statistics_us_per_step"] = e0.elapsed_time(e1) * 1000.0 / 200
    base = rec["ms_per_clip"]["ddim-20"]["min"]
    rec["ratio_to_ddim20"] = {k: v["min"] / base for k, v in rec["ms_per_clip"].items()}
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
