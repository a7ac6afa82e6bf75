#!/usr/bin/env python
"""Adaptive DeepCache (deep_cache_threshold=) against the fixed rule at BASELINE.json configs[1] (768 x 768, 16 frames, CFG 3.5, 20 DDIM steps,
full-width UNets, seeded weights, one queue), depth 3: the plain loop, the fixed rule at N = 2, 3, 5 and a handful of thresholds under the cap
N = 5, all in one run.  Per setting: the number of key steps (from pipe.last_deep_cache_trace), the time per clip (one warm-up loop, then
--reps timed loops ALTERNATED setting by setting, each bracketed by HIP events on the current stream) and the relative L2 distance of the final
latents to the plain loop's.  The weights are synthetic: the distances size the approximation, image quality is not assessed.  The claim the
record states, whichever way it falls: whether some threshold has a lower rel-L2 than a fixed-rule row at an equal or lower key-step count.

Also: md_rel_l1_f16 at the loop's shape (32 x 96 x 96 rows of C = 320 in buffers of pitch 960: 2 x 188 MB read), HIP events round --kernel_reps
back-to-back calls behind a warm-up, the minimum over 3 such groups, and the bandwidth that follows; and the wall cost of the mid-forward
synchronisation: the loop under threshold inf (an auto call at every step, none fires: the fixed N = 5 rule's evaluations bit for bit) against the
fixed N = 5 loop, host wall time with a device synchronisation at both ends, per shallow step.

    python tools/time_deep_cache_adaptive.py [--reps 2] [--thresholds 0.2,0.4,0.6,0.9,1.2] [--out profiles/deep_cache_adaptive.json]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP, DEPTH = 5, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--thresholds", default="0.2,0.4,0.6,0.9,1.2")
    ap.add_argument("--kernel_reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from mikudance_amd import DDIMScheduler, MikuDanceVideoPipeline, _lib, ops
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
    pipe.two_queues = False
    settings = [("plain", {})] + [(f"fixed N{n}", dict(deep_cache_interval=n, deep_cache_depth=DEPTH)) for n in (2, 3, 5)] \
        + [(f"threshold {t:g}", dict(deep_cache_interval=CAP, deep_cache_depth=DEPTH, deep_cache_threshold=t))
           for t in [float(v) for v in a.thresholds.split(",")] + [math.inf]]
    rec = {"config": {"frames": a.frames, "size": a.size, "steps": a.steps, "guidance": 3.5, "reps": a.reps, "two_queues": False, "depth": DEPTH,
                      "cap": CAP, "weights": "synthetic (seeded): image quality is not assessed"}, "rows": {}}

    def timed(kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        out = pipe.denoise(lat, rl, emb, a.steps, 3.5, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out, (time.perf_counter() - t0) * 1e3

    results, traces = {}, {}
    for name, kw in settings:                                            # warm-up; the result and the trace are kept
        results[name] = timed(kw)[1].float().cpu()
        traces[name] = pipe.last_deep_cache_trace
        print(f"{name}: warm", file=sys.stderr, flush=True)
    times, walls = {name: [] for name, _ in settings}, {name: [] for name, _ in settings}
    for _ in range(a.reps):
        for name, kw in settings:                                        # alternated: drift hits all alike
            ms, _, wall = timed(kw)
            times[name].append(ms)
            walls[name].append(wall)
    for name, _ in settings:
        tr = traces[name]
        rec["rows"][name] = {"key_steps": a.steps if tr is None else sum(1 for *_, k, _ in tr if k == "key"),
                             "seconds_per_clip": min(times[name]) / 1e3, "seconds_all": [t / 1e3 for t in times[name]],
                             "wall_seconds_per_clip": min(walls[name]) / 1e3,
                             "rel_l2_to_plain": rel_l2(results[name], results["plain"]),
                             "distances": None if tr is None else [None if r is None else round(r, 5) for *_, r in tr]}
        print(f"{name}: {rec['rows'][name]}", file=sys.stderr, flush=True)
    wins = []
    for tn, row in rec["rows"].items():
        for fname, frow in rec["rows"].items():
            if tn.startswith("threshold") and tn != "threshold inf" and fname.startswith("fixed") and row["key_steps"] <= frow["key_steps"] \
                    and row["rel_l2_to_plain"] < frow["rel_l2_to_plain"]:
                wins.append({"threshold_row": tn, "fixed_row": fname})
    rec["claim"] = {"some_threshold_beats_a_fixed_row_at_equal_or_fewer_key_steps": bool(wins), "pairs": wins}

    # ---- the kernel at the loop's shape: two skip slices of the (32, 96, 96, 960) concat buffers of skip 2
    rows, C, ld = 2 * a.frames * h * h, 320, 960
    g = torch.Generator().manual_seed(1)
    bufs = [torch.randn((rows, ld), generator=g, dtype=torch.float32).half().to(dev) for _ in range(2)]
    va, vb = bufs[0][:, ld - C:], bufs[1][:, ld - C:]
    out = torch.empty((2,), device=dev, dtype=torch.float32)
    ops.rel_l1(va, vb, out=out)
    torch.cuda.synchronize()
    groups = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_reps):
            ops.rel_l1(va, vb, out=out)
        e1.record()
        torch.cuda.synchronize()
        groups.append(e0.elapsed_time(e1) / a.kernel_reps)
    nbytes = 2 * rows * C * 2
    rec["kernel"] = {"rows": rows, "C": C, "pitch": ld, "bytes_read": nbytes, "ms": min(groups), "ms_groups": groups,
                     "GB_per_s": nbytes / (min(groups) * 1e-3) / 1e9,
                     "note": "back-to-back calls on the same 2 x 188 MB: the 256 MiB Infinity Cache cannot hold both operands, but serves part of them"}
    del bufs, va, vb

    # ---- the synchronisation: the cap-only adaptive loop makes the fixed N = 5 loop's evaluations plus, per shallow step, the distance, the
    # read-back and the copy
    shallow = a.steps - len(range(0, a.steps, CAP))
    fx, au = rec["rows"][f"fixed N{CAP}"], rec["rows"]["threshold inf"]
    assert au["key_steps"] == fx["key_steps"] and au["rel_l2_to_plain"] == fx["rel_l2_to_plain"], "threshold inf is not the fixed rule"
    rec["sync_cost"] = {"shallow_steps": shallow, "wall_ms_per_shallow_step": (au["wall_seconds_per_clip"] - fx["wall_seconds_per_clip"]) * 1e3 / shallow,
                        "event_ms_per_shallow_step": (au["seconds_per_clip"] - fx["seconds_per_clip"]) * 1e3 / shallow,
                        "note": "threshold inf (never fires) minus fixed N = cap, per shallow step: md_rel_l1_f16, the read-back that drains "
                                "the host's run-ahead, one 320-channel slice copy"}
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
