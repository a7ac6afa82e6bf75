#!/usr/bin/env python
"""Per-clip denoising-loop time with shifted-tile self-attention at BASELINE.json configs[1] (768 x 768, 16 frames, CFG 3.5, 20 DDIM steps,
full-width UNets, seeded weights, one queue): plain, tile_attention=2, tile_attention=2 with kv_downsample=2, and tile_attention=(2, 2).  One
warm-up loop per setting, then --reps timed loops ALTERNATED setting by setting, each bracketed by HIP events on the current stream.  Then one
more loop per setting under the per-launch event profiler (_lib.PROFILER) for the time of the level-0 self-attention launches and of
token_tile / token_untile / token_pool per clip, and the relative L2 distance between each result and the plain one (synthetic weights: the
size of the approximation, not a statement about image quality).  First of all the operator alone at (32, 96, 96, 320, t = 2), both
directions: the median of 200 launches after 20 warm-ups, HIP events, against the bytes it moves (one read and one write of the matrix).
Prints one JSON line.

    python tools/time_tile_attention.py [--reps 2] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = (("plain", {}), ("tile 2", dict(tile_attention=(2,))), ("tile 2 + kv 2", dict(tile_attention=(2,), kv_downsample=(2,))),
            ("tile 2,2", dict(tile_attention=(2, 2))))


def operator_time(dev, B=32, Hh=96, Ww=96, C=320, t=2, shift=(12, 24), launches=200, warm=20):
    from mikudance_amd import ops
    x = torch.randn((B * Hh * Ww, C), device=dev, dtype=torch.float16)
    y = torch.empty_like(x)
    out = {"shape": [B, Hh, Ww, C, t], "shift": list(shift), "bytes": 2 * x.numel() * 2}
    for name, fn, src, dst in (("tile", ops.token_tile, x, y), ("untile", ops.token_untile, y, x)):
        ms = []
        for i in range(warm + launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(src, B, Hh, Ww, t, shift, out=dst)
            e1.record()
            torch.cuda.synchronize()
            if i >= warm:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = ms[len(ms) // 2]
        out[name] = {"median_ms": med, "min_ms": ms[0], "TB_per_s": out["bytes"] / (med * 1e-3) / 1e12}
    return out


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
    rec = {"operator": operator_time(dev)}
    print(f"operator: {rec['operator']}", file=sys.stderr, flush=True)
    ref, den, _, _ = build_models(geom=dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768), device=dev,
                                  keep_state_dicts=False)
    h = a.size // 8
    lat, rl, emb = (t.half().to(dev) for t in synth_inputs(a.frames, h, h, ctx_len=257, ctx_dim=768, seed=100))
    pipe = MikuDanceVideoPipeline(None, None, ref, den, DDIMScheduler(**SCHED_KWARGS))
    pipe.two_queues = False
    rec.update({"config": {"frames": a.frames, "size": a.size, "steps": a.steps, "guidance": 3.5, "reps": a.reps, "two_queues": False},
                "ms_per_clip": {}, "frames_per_s": {}, "rel_l2_to_plain": {}, "profiled_ms_per_clip": {}})

    def timed(kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipe.denoise(lat, rl, emb, a.steps, 3.5, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    results = {}
    for name, kw in SETTINGS:
        results[name] = timed(kw)[1].float().cpu()                                   # warm-up; the result is kept for the distance
    times = {name: [] for name, _ in SETTINGS}
    for _ in range(a.reps):
        for name, kw in SETTINGS:                                                    # alternated: drift hits all alike
            times[name].append(timed(kw)[0])
    for name, _ in SETTINGS:
        rec["ms_per_clip"][name] = {"min": min(times[name]), "all": times[name]}
        rec["frames_per_s"][name] = a.frames / (min(times[name]) / 1e3)
        rec["rel_l2_to_plain"][name] = rel_l2(results[name], results["plain"])
        print(f"{name}: {times[name]}", file=sys.stderr, flush=True)
    rec["ratio_to_plain"] = {name: rec["ms_per_clip"][name]["min"] / rec["ms_per_clip"]["plain"]["min"] for name, _ in SETTINGS}
    # per-launch pass: the level-0 self-attention (whole frame: Lq = h * h; tiled: Lq = h * h / 4 at B * 4) and the reorder / pool passes
    L0 = h * h
    for name, kw in SETTINGS:
        _lib.PROFILER.start()
        pipe.denoise(lat, rl, emb, a.steps, 3.5, **kw)
        torch.cuda.synchronize()
        _lib.PROFILER.stop()
        keep = {}
        for label, d in _lib.PROFILER.summary().items():
            level0 = label.startswith("attention") and (f"Lq={L0} " in label or f"Lq={L0 // 4} " in label) and "Lk=257" not in label and " D=40 " in label
            if level0 or label.startswith("token_"):
                keep[label] = {"count": d["count"], "ms": d["ms"]}
        tot = sum(d["ms"] for d in _lib.PROFILER.summary().values())
        rec["profiled_ms_per_clip"][name] = {"all_launches": tot, "launches": keep}
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
