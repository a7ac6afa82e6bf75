#!/usr/bin/env python
"""Per-clip denoising-loop time with guidance_interval= / uncond_cache_interval= at BASELINE.json configs[1] (768 x 768, 16 frames, CFG 3.5,
20 DDIM steps, full-width UNets, seeded weights, one queue): plain, uncond_cache_interval 2 and 3, guidance_interval=(0.0, 0.5), and
uncond_cache_interval=2 with kv_downsample=2.  One warm-up loop per setting, then --reps timed loops ALTERNATED setting by setting, each bracketed
by HIP events on the current stream.  The warm-up loop's result gives the relative L2 distance and the cosine to the plain loop (synthetic weights:
the size of the approximation, not a statement about image quality).  From each setting without kv_downsample the share of a full step that a
conditional-only step takes is solved: T = K T_full + (steps - K) T_cond with K full steps.  md_cfg_uncond_cache is timed on its own, per mode, over
--kernel_reps back-to-back calls between two events.  Prints one JSON line; the plain case of the same run is the baseline of every ratio.

    python tools/time_uncond_cache.py [--reps 2] [--only NAME[,NAME...]] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = (("plain", {}), ("n2", dict(uncond_cache_interval=2)), ("n3", dict(uncond_cache_interval=3)),
            ("interval 0-0.5", dict(guidance_interval=(0.0, 0.5))), ("n2 + kv 2", dict(uncond_cache_interval=2, kv_downsample=(2,))))


def full_steps(steps, kw):
    """How many of `steps` steps evaluate both clip-halves (the loop's rule, restated)."""
    lo, hi = kw.get("guidance_interval", (0.0, 1.0))
    n, full, last = kw.get("uncond_cache_interval", 1), 0, None
    for k in range(steps):
        if not lo * steps <= k < hi * steps:
            last = None
        elif last is None or k - last >= n:
            full, last = full + 1, k
    return full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kernel_reps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, help="comma-separated setting names; plain is always run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from mikudance_amd import DDIMScheduler, MikuDanceVideoPipeline, _lib, ops
    from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2
    from mikudance_amd.synth import synth_inputs
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    settings = [s for s in SETTINGS if a.only is None or s[0] == "plain" or s[0] in a.only.split(",")]
    ref, den, _, _ = build_models(geom=dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768), device=dev,
                                  keep_state_dicts=False)
    h = a.size // 8
    lat, rl, emb = (t.half().to(dev) for t in synth_inputs(a.frames, h, h, ctx_len=257, ctx_dim=768, seed=100))
    pipe = MikuDanceVideoPipeline(None, None, ref, den, DDIMScheduler(**SCHED_KWARGS))
    pipe.two_queues = False
    rec = {"config": {"frames": a.frames, "size": a.size, "steps": a.steps, "guidance": 3.5, "reps": a.reps, "two_queues": False},
           "s_per_clip": {}, "frames_per_s": {}, "rel_l2_to_plain": {}, "cosine_to_plain": {}, "full_steps": {}}

    def timed(kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipe.denoise(lat, rl, emb, a.steps, 3.5, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3, out

    results = {}
    for name, kw in settings:                                                        # warm-up; the result is kept
        results[name] = timed(kw)[1].float().cpu()
        print(f"{name}: warm", file=sys.stderr, flush=True)
    times = {name: [] for name, _ in settings}
    for _ in range(a.reps):
        for name, kw in settings:                                                    # alternated: drift hits all alike
            times[name].append(timed(kw)[0])
    for name, kw in settings:
        rec["s_per_clip"][name] = {"min": min(times[name]), "all": times[name]}
        rec["frames_per_s"][name] = a.frames / min(times[name])
        rec["rel_l2_to_plain"][name] = rel_l2(results[name], results["plain"])
        rec["cosine_to_plain"][name] = cosine(results[name], results["plain"])
        rec["full_steps"][name] = full_steps(a.steps, kw)
        print(f"{name}: {times[name]}", file=sys.stderr, flush=True)
    plain = rec["s_per_clip"]["plain"]["min"]
    rec["ratio_to_plain"] = {name: rec["s_per_clip"][name]["min"] / plain for name, _ in settings}
    rec["conditional_step_share_of_a_full_step"] = {}
    for name, kw in settings:
        k = rec["full_steps"][name]
        if k < a.steps and "kv_downsample" not in kw:
            rec["conditional_step_share_of_a_full_step"][name] = (rec["s_per_clip"][name]["min"] - k * plain / a.steps) / ((a.steps - k) * plain / a.steps)
    # the new kernel on its own, at the clip's size
    hw = h * h
    ns = torch.randn(2, a.frames, hw, 4, device=dev)
    cnt = torch.ones(a.frames, device=dev)
    delta = torch.empty(a.frames, hw, 4, device=dev)
    rec["kernel_us_per_call"] = {}
    for tag, args in (("store", (delta, a.frames, hw, 0)), ("restore scale 1", (delta, a.frames, hw, 1, 1.0)), ("restore scale 0", (None, a.frames, hw, 1, 0.0))):
        for _ in range(10):
            ops.cfg_uncond_cache(ns, cnt, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_reps):
            ops.cfg_uncond_cache(ns, cnt, *args)
        e1.record()
        torch.cuda.synchronize()
        rec["kernel_us_per_call"][tag] = e0.elapsed_time(e1) * 1e3 / a.kernel_reps
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
