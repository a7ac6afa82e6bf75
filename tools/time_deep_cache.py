#!/usr/bin/env python
"""Per-clip denoising-loop time with DeepCache (deep_cache_interval=N, deep_cache_depth=d) at BASELINE.json configs[1] (768 x 768, 16 frames,
CFG 3.5, 20 DDIM steps, full-width UNets, seeded weights, one queue) or, with --frames / --size / --steps / --context_frames, at another
geometry such as configs[4]: plain, N in {2, 3, 5} at d = 3, N = 3 at d in {1, 2}, and N = 3, d = 3 with kv_downsample=2 and tile_attention=2.
One warm-up loop per setting, then --reps timed loops ALTERNATED setting by setting, each bracketed by HIP events on the current stream.  The
warm-up loop's result gives the relative L2 distance and the cosine to the plain loop (synthetic weights: the size of the approximation, not a
statement about image quality) and its peak allocated memory.  From the times of the d = 3 settings the share of a plain step that a shallow step
takes is solved per N: T_N = K_N T_full + (steps - K_N) T_shallow with K_N key steps.  Prints one JSON line.

    python tools/time_deep_cache.py [--reps 2] [--only NAME[,NAME...]] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DC = lambda n, d: dict(deep_cache_interval=n, deep_cache_depth=d)
SETTINGS = (("plain", {}), ("N2 d3", DC(2, 3)), ("N3 d3", DC(3, 3)), ("N5 d3", DC(5, 3)), ("N3 d1", DC(3, 1)), ("N3 d2", DC(3, 2)),
            ("N3 d3 + kv 2 + tile 2", dict(DC(3, 3), kv_downsample=(2,), tile_attention=(2,))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--context_frames", type=int, default=None)
    ap.add_argument("--context_overlap", type=int, default=8)
    ap.add_argument("--only", default=None, help="comma-separated setting names; plain is always run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from mikudance_amd import DDIMScheduler, MikuDanceVideoPipeline, _lib
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
    win = {} if a.context_frames is None else dict(context_frames=a.context_frames, context_stride=1, context_overlap=a.context_overlap)
    rec = {"config": {"frames": a.frames, "size": a.size, "steps": a.steps, "guidance": 3.5, "reps": a.reps, "two_queues": False, **win},
           "ms_per_clip": {}, "frames_per_s": {}, "rel_l2_to_plain": {}, "cosine_to_plain": {}, "peak_allocated_MB": {}}

    def timed(kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipe.denoise(lat, rl, emb, a.steps, 3.5, **win, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    results = {}
    for name, kw in settings:                                                        # warm-up; the result and the peak memory are kept
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        results[name] = timed(kw)[1].float().cpu()
        rec["peak_allocated_MB"][name] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        print(f"{name}: warm, peak {rec['peak_allocated_MB'][name]:.0f} MB", file=sys.stderr, flush=True)
    times = {name: [] for name, _ in settings}
    for _ in range(a.reps):
        for name, kw in settings:                                                    # alternated: drift hits all alike
            times[name].append(timed(kw)[0])
    for name, _ in settings:
        rec["ms_per_clip"][name] = {"min": min(times[name]), "all": times[name]}
        rec["frames_per_s"][name] = a.frames / (min(times[name]) / 1e3)
        rec["rel_l2_to_plain"][name] = rel_l2(results[name], results["plain"])
        rec["cosine_to_plain"][name] = cosine(results[name], results["plain"])
        print(f"{name}: {times[name]}", file=sys.stderr, flush=True)
    plain = rec["ms_per_clip"]["plain"]["min"]
    rec["ratio_to_plain"] = {name: rec["ms_per_clip"][name]["min"] / plain for name, _ in settings}
    rec["shallow_step_share_d3"] = {}
    for name, kw in settings:
        if kw.get("deep_cache_depth") == 3 and "kv_downsample" not in kw:
            keys = len(range(0, a.steps, kw["deep_cache_interval"]))
            rec["shallow_step_share_d3"][name] = (rec["ms_per_clip"][name]["min"] - keys * plain / a.steps) / ((a.steps - keys) * plain / a.steps)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
