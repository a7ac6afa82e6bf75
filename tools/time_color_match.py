#!/usr/bin/env python
"""Time of colour matching (color_match="mkl") at the pipeline's output tail, "final latents on the device -> bytes on the host", beside the uint8
path without it (output_type="uint8", md_frames_u8), in the same run: sd-vae-ft-mse geometry, seeded synthetic weights, 16 frames of 768 x 768
and 48 frames of 1024 x 1024 in VAE batches of 8, one MI355X.

    plain   vae.decode_u8 per batch straight into one (f, H, W, 3) device buffer, .cpu()
    frame   per batch: vae.decode_image_view, ops.color_moments, the host read of B x 9 doubles, color_match.transform per frame, the
            coefficients to the device, ops.color_apply into the buffer; .cpu()
    clip    the same with ONE transform from the summed sums: the decoded views of every batch are held until the last batch's sums are in

Each path restates MikuDanceVideoPipeline._decode_u8 / _decode_color_matched in the open; before anything is timed both are held to the package
on a small clip (the run stops if they differ).  Wall clock (time.perf_counter) around a pass that ends in the device-to-host copy, one warm-up
pass, then --reps timed passes: median (min - max).  The two kernels alone: 200 back-to-back calls between two HIP events on one VAE batch, NHWC
source (the decoder's) and NCHW source (the tiled decode's), microseconds and the bytes they move per second.  The per-batch host read: the
wall time of color_moments(...).cpu() on a batch against color_moments(...) + synchronize, 50 times each.

    python tools/time_color_match.py [--configs 16x768,48x1024] [--reps 5] [--out profiles/color_match_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VAE_BATCH = 8
MODE = "mkl"


def build_vae(dev):
    from mikudance_amd import AutoencoderKL
    from mikudance_amd.synth import synth_state_dict
    vae = AutoencoderKL()
    vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=77), strict=True)
    return vae.half().to(dev).eval()


def latents(frames, size, dev):
    g = torch.Generator().manual_seed(size + frames)
    return torch.randn(frames, 4, size // 8, size // 8, generator=g).half().to(dev)


def plain_path(vae, z, target):
    video = torch.empty((z.shape[0], 8 * z.shape[2], 8 * z.shape[3], 3), device=z.device, dtype=torch.uint8)
    for i in range(0, z.shape[0], VAE_BATCH):
        vae.decode_u8(z[i:i + VAE_BATCH], out=video[i:i + VAE_BATCH])
    return video.cpu()


def matched_path(scope):
    def run(vae, z, target):
        from mikudance_amd import color_match as CM, ops
        n, H, W = z.shape[0], 8 * z.shape[2], 8 * z.shape[3]
        video = torch.empty((n, H, W, 3), device=z.device, dtype=torch.uint8)
        sums, held = np.empty((n, 9)), []
        for i in range(0, n, VAE_BATCH):
            view = vae.decode_image_view(z[i:i + VAE_BATCH])
            sums[i:i + view.shape[0]] = ops.color_moments(view).cpu().numpy()
            if scope == "clip":
                held.append((i, view))
                continue
            maps = [CM.transform(s, H * W, *target, MODE, 1.0) for s in sums[i:i + view.shape[0]]]
            ops.color_apply(view, torch.from_numpy(CM.coefficients(maps)).to(z.device), out=video[i:i + view.shape[0]])
        if scope == "clip":
            one = CM.transform(sums.sum(0), H * W * n, *target, MODE, 1.0)
            for i, view in held:
                ops.color_apply(view, torch.from_numpy(CM.coefficients([one] * view.shape[0])).to(z.device), out=video[i:i + view.shape[0]])
        return video.cpu()
    return run


PATHS = {"plain": plain_path, "frame": matched_path("frame"), "clip": matched_path("clip")}


def target_sums(size):
    from mikudance_amd import color_match as CM
    return CM.moments_of_image(np.random.default_rng(5).uniform(0.1, 0.9, (size, size, 3)))


def paths_equal_the_package(vae, dev):
    """The timed paths against MikuDanceVideoPipeline's own methods on a small clip."""
    from mikudance_amd.pipeline_mikudance import MikuDanceVideoPipeline as P
    pipe = types.SimpleNamespace(vae=vae, vae_batch=VAE_BATCH)
    pipe._decode_frames = types.MethodType(P._decode_frames, pipe)
    lat = torch.randn(1, 4, 10, 32, 32, generator=torch.Generator().manual_seed(3)).half().to(dev)
    z = (1 / 0.18215 * lat).permute(0, 2, 1, 3, 4).reshape(-1, 4, 32, 32).to(vae.dtype)
    target = target_sums(256)
    ok = {"plain": bool(torch.equal(P._decode_u8(pipe, lat, VAE_BATCH)[0], plain_path(vae, z, target)))}
    for scope in ("frame", "clip"):
        plan = dict(mode=MODE, strength=1.0, scope=scope, targets=[target])
        ok[scope] = bool(torch.equal(P._decode_color_matched(pipe, lat, VAE_BATCH, plan, as_bytes=True)[0], PATHS[scope](vae, z, target)))
    return ok


def _stat(ms):
    return dict(median=round(statistics.median(ms), 2), min=round(min(ms), 2), max=round(max(ms), 2))


def _events(fn, calls=200):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="16x768,48x1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mikudance_amd import ops
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    vae = build_vae(dev)
    result = {"config": dict(vae_batch=VAE_BATCH, reps=a.reps, mode=MODE, weights="synthetic, seed 77", kernel_calls=200,
                             clock="perf_counter around a pass that ends in the device-to-host copy; kernels: HIP events around 200 calls"), "runs": {}}
    result["config"]["paths_equal_the_package"] = paths_equal_the_package(vae, dev)
    assert all(result["config"]["paths_equal_the_package"].values()), result["config"]["paths_equal_the_package"]
    for cfg in a.configs.split(","):
        frames, size = (int(v) for v in cfg.split("x"))
        z, target = latents(frames, size, dev), target_sums(size)
        rec = {}
        for name, fn in PATHS.items():
            fn(vae, z[:VAE_BATCH], target)                                     # warm-up
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn(vae, z, target)
                ms.append(1e3 * (time.perf_counter() - t0))
            rec[name] = dict(total_ms=_stat(ms))
            print(cfg, name, json.dumps(rec[name]), flush=True)
        for name in ("frame", "clip"):
            rec[name]["added_ms_median"] = round(rec[name]["total_ms"]["median"] - rec["plain"]["total_ms"]["median"], 2)
        # the kernels alone, one VAE batch
        g = torch.Generator().manual_seed(1)
        nhwc = (torch.rand(VAE_BATCH, size, size, 3, generator=g) * 3 - 1.5).half().to(dev)
        nchw = nhwc.permute(0, 3, 1, 2).contiguous()
        out = torch.empty((VAE_BATCH, size, size, 3), device=dev, dtype=torch.uint8)
        fout = torch.empty((VAE_BATCH, 3, size, size), device=dev, dtype=torch.float32)
        sums = torch.empty((VAE_BATCH, 9), device=dev, dtype=torch.float64)
        coef = (torch.eye(3).reshape(1, 9).repeat(VAE_BATCH, 1) * 0.9).to(dev)
        coef = torch.cat([coef, torch.full((VAE_BATCH, 3), 0.05, device=dev)], 1).contiguous()
        n = out.numel()
        ld8 = torch.zeros((VAE_BATCH, size, size, 8), device=dev, dtype=nhwc.dtype)                  # the temporal decoder's image: pixel pitch 8
        ld8[..., :3] = nhwc
        for label, src in (("nhwc", nhwc.permute(0, 3, 1, 2)), ("nchw", nchw), ("nhwc_ld8", ld8[..., :3].permute(0, 3, 1, 2))):
            us = _events(lambda: ops.color_moments(src, sums))
            rec[f"moments_{label}_batch8"] = dict(us_per_call=round(us, 2), gb_per_s=round(2.0 * n / us / 1e3, 1), launches=2)
            us = _events(lambda: ops.color_apply(src, coef, out))
            rec[f"apply_u8_{label}_batch8"] = dict(us_per_call=round(us, 2), gb_per_s=round(3.0 * n / us / 1e3, 1))
            us = _events(lambda: ops.color_apply(src, coef, fout, dtype=torch.float32))
            rec[f"apply_f32_{label}_batch8"] = dict(us_per_call=round(us, 2), gb_per_s=round(6.0 * n / us / 1e3, 1))
            us = _events(lambda: ops.frames_u8(src, out))
            rec[f"frames_u8_{label}_batch8"] = dict(us_per_call=round(us, 2), gb_per_s=round(3.0 * n / us / 1e3, 1))
        # the per-batch host read
        src = nhwc.permute(0, 3, 1, 2)
        reads, syncs = [], []
        for _ in range(50):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.color_moments(src, sums).cpu()
            reads.append(1e6 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            ops.color_moments(src, sums)
            torch.cuda.synchronize()
            syncs.append(1e6 * (time.perf_counter() - t0))
        rec["host_read_batch8"] = dict(moments_and_read_us=_stat(reads), moments_and_sync_us=_stat(syncs),
                                       read_over_sync_us_median=round(statistics.median(reads) - statistics.median(syncs), 2))
        del nhwc, nchw, out, fout, z
        torch.cuda.empty_cache()
        print(cfg, json.dumps(rec), flush=True)
        result["runs"][cfg] = rec
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
