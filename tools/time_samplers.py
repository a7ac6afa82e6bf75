#!/usr/bin/env python
"""Per-clip denoising-loop time of each sampler at BASELINE.json configs[1] (768 x 768, 16 frames, CFG 3.5, full-width UNets, seeded
weights): DDIM-20 (the headline), DPM-Solver++ 2M-10 and 2M-20.  One warm-up loop per sampler, then --reps timed loops, each bracketed
by HIP events on the current stream; prints one JSON line.  --guidance_rescale PHI (> 0) times every sampler with and without guidance
rescale, the two alternated rep by rep after one warm-up loop each, and adds the cost of the rescale per clip and per step.

    python tools/time_samplers.py [--reps 2] [--guidance_rescale 0.7] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLERS = (("ddim", 20), ("dpmpp_2m", 10), ("dpmpp_2m", 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--guidance_rescale", type=float, default=0.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
    rec = {"config": {"frames": a.frames, "size": a.size, "guidance": 3.5, "reps": a.reps, "guidance_rescale": a.guidance_rescale},
           "ms_per_clip": {}}

    def timed(pipe, steps, phi):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pipe.denoise(lat, rl, emb, steps, 3.5, guidance_rescale=phi)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for name, steps in SAMPLERS:
        sch = DDIMScheduler(**SCHED_KWARGS) if name == "ddim" else DPMSolverMultistepScheduler(**SCHED_KWARGS)
        pipe = MikuDanceVideoPipeline(None, None, ref, den, sch)
        for phi in phis:
            pipe.denoise(lat, rl, emb, steps, 3.5, guidance_rescale=phi)          # warm-up
        torch.cuda.synchronize()
        times = {phi: [] for phi in phis}
        for _ in range(a.reps):
            for phi in phis:                                                         # alternated: drift hits both alike
                times[phi].append(timed(pipe, steps, phi))
        for phi in phis:
            key = f"{name}-{steps}" + (f"-rescale{phi:g}" if phi else "")
            rec["ms_per_clip"][key] = {"min": min(times[phi]), "all": times[phi]}
            print(f"{key}: {times[phi]}", file=sys.stderr, flush=True)
        if len(phis) == 2:
            d = min(times[phis[1]]) - min(times[0.0])
            rec.setdefault("rescale_cost", {})[f"{name}-{steps}"] = {"ms_per_clip": d, "ms_per_step": d / steps}
    if len(phis) == 2:                                                               # the statistics launches alone, on this clip's shape
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
