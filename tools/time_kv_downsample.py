#!/usr/bin/env python
"""Per-clip denoising-loop time with K / V token downsampling at BASELINE.json configs[1] (768 x 768, 16 frames, CFG 3.5, 20 DDIM steps,
full-width UNets, seeded weights): kv_downsample 1 (the plain loop), 2 and (4, 2), nearest.  One warm-up loop per setting, then --reps timed
loops ALTERNATED setting by setting, each bracketed by HIP events on the current stream.  Then one more loop per setting under the per-launch
event profiler (_lib.PROFILER, serialising the two queues as bench.py's timing pass does) for the time of the level-0 self-attention
launches, of token_pool and of the q / k / v projections per clip, and the relative L2 distance between each pooled result and the plain
one (synthetic weights: the size of the approximation, not a statement about image quality).  Prints one JSON line.

    python tools/time_kv_downsample.py [--reps 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = (("1", 1), ("2", (2,)), ("4,2", (4, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from mikudance_amd import DDIMScheduler, MikuDanceVideoPipeline, _lib
    from mikudance_amd.selftest import SCHED_KWARGS, build_models, rel_l2
    from mikudance_amd.synth import synth_inputs
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ref, den, _, _ = build_models(geom=dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768), device=dev,
                                  keep_state_dicts=False)
    h = a.size // 8
    lat, rl, emb = (t.half().to(dev) for t in synth_inputs(a.frames, h, h, ctx_len=257, ctx_dim=768, seed=100))
    pipe = MikuDanceVideoPipeline(None, None, ref, den, DDIMScheduler(**SCHED_KWARGS))
    rec = {"config": {"frames": a.frames, "size": a.size, "steps": a.steps, "guidance": 3.5, "reps": a.reps, "two_queues": bool(pipe.two_queues)},
           "ms_per_clip": {}, "frames_per_s": {}, "rel_l2_to_plain": {}, "profiled_ms_per_clip": {}}

    def timed(kv):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipe.denoise(lat, rl, emb, a.steps, 3.5, kv_downsample=kv)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    results = {}
    for name, kv in SETTINGS:
        results[name] = timed(kv)[1].float().cpu()                                   # warm-up; the result is kept for the distance
    times = {name: [] for name, _ in SETTINGS}
    for _ in range(a.reps):
        for name, kv in SETTINGS:                                                    # alternated: drift hits all alike
            times[name].append(timed(kv)[0])
    for name, _ in SETTINGS:
        rec["ms_per_clip"][name] = {"min": min(times[name]), "all": times[name]}
        rec["frames_per_s"][name] = a.frames / (min(times[name]) / 1e3)
        rec["rel_l2_to_plain"][name] = rel_l2(results[name], results["1"])
        print(f"kv_downsample {name}: {times[name]}", file=sys.stderr, flush=True)
    rec["ratio_to_plain"] = {name: rec["ms_per_clip"][name]["min"] / rec["ms_per_clip"]["1"]["min"] for name, _ in SETTINGS}
    # per-launch pass: the level-0 self-attention (Lq = h * h), token_pool, and the projections that feed them
    L0 = h * h
    den.serialize_queues = True
    try:
        for name, kv in SETTINGS:
            _lib.PROFILER.start()
            pipe.denoise(lat, rl, emb, a.steps, 3.5, kv_downsample=kv)
            torch.cuda.synchronize()
            _lib.PROFILER.stop()
            keep = {}
            for label, d in _lib.PROFILER.summary().items():
                if (label.startswith("attention") and f"Lq={L0} " in label and "Lk=257" not in label) or label.startswith("token_pool"):
                    keep[label] = {"count": d["count"], "ms": d["ms"]}
            tot = sum(d["ms"] for d in _lib.PROFILER.summary().values())
            rec["profiled_ms_per_clip"][name] = {"all_launches": tot, "launches": keep}
    finally:
        den.serialize_queues = False
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
