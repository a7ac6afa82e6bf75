#!/usr/bin/env python
"""Time and peak memory of tiled against untiled AutoencoderKL passes (enable_tiling(), 512-pixel tiles) at the sizes the pipeline is advertised
at: the decode of a clip of 16 frames and the encode of the 19 distinct images of configs[1], each in batches of the pipeline's vae_batch = 8, at
768 x 768, 1024 x 1024, 1536 x 1536 and 2048 x 2048, sd-vae-ft-mse geometry, seeded synthetic weights.  Every pass is bracketed by HIP events on the
current stream after one warm-up batch, and torch.cuda.max_memory_allocated is read over the timed pass (reset before it).  The untiled pass is
the parent path unchanged and runs in the same process.  One more tiled pass under the per-launch profiler gives md_tile_blend_f16's own time per
call.  The tiled and the untiled decode of the first batch give the relative L2 distance between them: a different result BY DESIGN (each tile's
GroupNorm and attention see that tile only), on synthetic weights the size of the difference and no statement about image quality.

Results are merged into --out size by size (an existing file is read first), so that the sizes can be measured in several runs.

    python tools/time_vae_tiling.py [--sizes 768,1024,1536,2048] [--reps 1] [--out profiles/vae_tiling_timing.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAMES, IMAGES, VAE_BATCH, TILE = 16, 19, 8, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="768,1024,1536,2048")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from mikudance_amd import AutoencoderKL, _lib
    from mikudance_amd.selftest import rel_l2
    from mikudance_amd.synth import synth_state_dict
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    vae = AutoencoderKL()
    vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=77), strict=True)
    vae = vae.half().to(dev).eval()
    vae.set_tile_size(TILE)
    result = {"config": dict(frames=FRAMES, images=IMAGES, vae_batch=VAE_BATCH, tile=TILE, reps=a.reps, weights="synthetic, seed 77"), "sizes": {}}
    if a.out and os.path.exists(a.out):
        result["sizes"] = json.load(open(a.out)).get("sizes", {})

    def batches(x):
        return [x[i:i + VAE_BATCH] for i in range(0, x.shape[0], VAE_BATCH)]

    def timed(fn, x):
        fn(x[:VAE_BATCH])                                                      # warm-up: one batch
        torch.cuda.synchronize()
        best, peak = None, 0
        for _ in range(a.reps):
            torch.cuda.reset_peak_memory_stats(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for b in batches(x):
                fn(b)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
            peak = max(peak, torch.cuda.max_memory_allocated(dev))
        return dict(ms=round(best, 2), peak_gib=round(peak / 2 ** 30, 3))

    for size in (int(s) for s in a.sizes.split(",")):
        g = torch.Generator().manual_seed(size)
        z = torch.randn(FRAMES, 4, size // 8, size // 8, generator=g).half().to(dev)
        x = (torch.rand(IMAGES, 3, size, size, generator=g) * 2 - 1).half().to(dev)
        rec = {}
        for name, on in (("untiled", False), ("tiled", True)):
            vae.enable_tiling(on)
            rec[f"decode_{name}"] = timed(lambda b: vae.decode(b).sample, z)
            rec[f"encode_{name}"] = timed(lambda b: vae.encode(b).latent_dist.mean, x)
            print(size, name, rec[f"decode_{name}"], rec[f"encode_{name}"], flush=True)
        vae.enable_tiling(True)
        rows, cols, _ = vae.tile_grid(size // 8, size // 8, encode=False)
        rec["tiles_per_pass"] = len(rows) * len(cols)
        _lib.PROFILER.start()
        try:
            tiled = vae.decode(z[:VAE_BATCH]).sample
            vae.encode(x[:VAE_BATCH])
        finally:
            _lib.PROFILER.stop()
        torch.cuda.synchronize()
        for label, r in _lib.PROFILER.summary().items():
            if label.startswith("tile_blend"):
                rec.setdefault("tile_blend_calls", {})[label] = dict(count=r["count"], ms_per_call=round(r["ms"] / r["count"], 4),
                                                                      gb_per_s=round(r["bytes"] / r["ms"] / 1e6, 1))
        vae.enable_tiling(False)
        rec["decode_tiled_vs_untiled_rel_l2"] = round(rel_l2(tiled.float(), vae.decode(z[:VAE_BATCH]).sample.float()), 5)
        del tiled
        result["sizes"][str(size)] = rec
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
        torch.cuda.empty_cache()
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
