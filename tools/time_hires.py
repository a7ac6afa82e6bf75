#!/usr/bin/env python
"""Per-clip denoising-loop time of two-pass high-resolution sampling (hires_scale=) against the plain loop, full-width UNets, seeded weights, CFG 3.5,
DDIM, one queue, 16 frames, 20 steps: plain 1024 x 1024 against hires_scale=2 (all 20 steps at 512 x 512, then the tail at 1024 x 1024) at
hires_strength 0.3, 0.5 and 0.7, and plain 768 x 768 against hires_scale=1.5 (512 x 512 first) at hires_strength 0.5.  A two-pass clip is what
MikuDanceVideoPipeline.__call__ runs between the VAE encode and decode: denoise() at the low size, upscale_latents() (md_latent_resize_f16), then
denoise(init_latents=, strength=) at the full size; the low-size conditions are the full-size ones resampled.  One warm-up clip per setting, then
--reps timed clips ALTERNATED setting by setting, each bracketed by HIP events on the current stream; the plain clip it is compared with runs in the
same process.  The warm-up clip's result gives the relative L2 distance and the cosine to the plain clip of its size (synthetic weights: the size of
the approximation, not a statement about image quality).  Prints one JSON line.

    python tools/time_hires.py [--reps 2] [--frames 16] [--steps 20] [--out profiles/hires_timing.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, full size, low size or None, hires_strength)
SETTINGS = (("plain 1024", 1024, None, None), ("hires 2 s0.3 1024", 1024, 512, 0.3), ("hires 2 s0.5 1024", 1024, 512, 0.5), ("hires 2 s0.7 1024", 1024, 512, 0.7),
            ("plain 768", 768, None, None), ("hires 1.5 s0.5 768", 768, 512, 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mode", default="bicubic")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    import torch.nn.functional as F
    from mikudance_amd import DDIMScheduler, MikuDanceVideoPipeline, _lib
    from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2
    from mikudance_amd.synth import synth_inputs
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ref, den, _, _ = build_models(geom=dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768), device=dev, keep_state_dicts=False)
    pipe = MikuDanceVideoPipeline(None, None, ref, den, DDIMScheduler(**SCHED_KWARGS))
    pipe.two_queues = False
    inputs = {}
    for size in sorted({s[1] for s in SETTINGS}):
        lat, rl, emb = (t.half().to(dev) for t in synth_inputs(a.frames, size // 8, size // 8, ctx_len=257, ctx_dim=768, seed=100))
        inputs[size] = dict(noise=lat, ref=rl, emb=emb)
    for _, size, low, _ in SETTINGS:
        if low is not None and (size, low) not in inputs:
            rl = inputs[size]["ref"]
            rl_lo = F.interpolate(rl[0].float(), size=(low // 8, low // 8), mode="bilinear", align_corners=False)
            rl_lo[:, 20:] *= low / size                                                  # the flow is in latent-grid units
            noise_lo = synth_inputs(a.frames, low // 8, low // 8, ctx_len=257, ctx_dim=768, seed=101)[0].half().to(dev)
            inputs[(size, low)] = dict(noise=noise_lo, ref=rl_lo.half()[None].contiguous())

    def clip(size, low, strength):
        full = inputs[size]
        if low is None:
            return pipe.denoise(full["noise"], full["ref"], full["emb"], a.steps, 3.5)
        first = inputs[(size, low)]
        x = pipe.denoise(first["noise"], first["ref"], full["emb"], a.steps, 3.5)
        x = pipe.upscale_latents(x, size, size, a.mode)
        return pipe.denoise(full["noise"], full["ref"], full["emb"], a.steps, 3.5, init_latents=x, strength=strength)

    def timed(setting):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = clip(*setting[1:])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    rec = {"config": {"frames": a.frames, "steps": a.steps, "guidance": 3.5, "reps": a.reps, "two_queues": False, "mode": a.mode, "sampler": "ddim"},
           "full_size_steps": {}, "ms_per_clip": {}, "s_per_clip": {}, "frames_per_s": {}, "ratio_to_plain": {}, "rel_l2_to_plain": {}, "cosine_to_plain": {},
           "peak_allocated_MB": {}}
    results = {}
    for s in SETTINGS:                                                                   # warm-up; the result and the peak memory are kept
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        results[s[0]] = timed(s)[1].float().cpu()
        rec["peak_allocated_MB"][s[0]] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        print(f"{s[0]}: warm, peak {rec['peak_allocated_MB'][s[0]]:.0f} MB", file=sys.stderr, flush=True)
    times = {s[0]: [] for s in SETTINGS}
    for _ in range(a.reps):
        for s in SETTINGS:                                                               # alternated: drift hits all alike
            times[s[0]].append(timed(s)[0])
    for name, size, low, strength in SETTINGS:
        plain = f"plain {size}"
        rec["full_size_steps"][name] = a.steps if low is None else int(a.steps * strength)
        rec["ms_per_clip"][name] = {"min": min(times[name]), "all": times[name]}
        rec["s_per_clip"][name] = min(times[name]) / 1e3
        rec["frames_per_s"][name] = a.frames / (min(times[name]) / 1e3)
        rec["ratio_to_plain"][name] = min(times[name]) / min(times[plain])
        rec["rel_l2_to_plain"][name] = rel_l2(results[name], results[plain])
        rec["cosine_to_plain"][name] = cosine(results[name], results[plain])
        print(f"{name}: {times[name]}", file=sys.stderr, flush=True)
    # the resampler alone, 48 x 64 x 64 -> 128 x 128 packed latents (the size of BASELINE.json configs[4])
    x = torch.randn((48, 64, 64, 4), device=dev).half()
    from mikudance_amd import ops
    ops.latent_resize(x, 48, 64, 64, 128, 128, a.mode)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        ops.latent_resize(x, 48, 64, 64, 128, 128, a.mode)
    e1.record()
    torch.cuda.synchronize()
    rec["latent_resize_us_48x64x64_to_128x128"] = e0.elapsed_time(e1) * 1e3 / 10
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
