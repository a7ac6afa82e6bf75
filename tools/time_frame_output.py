#!/usr/bin/env python
"""Time and host memory of the pipeline's output tail, "final latents on the device -> frames the writer accepts", for the float path and for the
uint8 path (output_type="uint8", md_frames_u8), sd-vae-ft-mse geometry, seeded synthetic weights, at 16 frames of 768 x 768 and 48 frames of
1024 x 1024 in batches of the pipeline's vae_batch = 8.

    float path   decode_latents as it stands: vae.decode per batch, torch.cat, (x / 2 + 0.5).clamp(0, 1) (three elementwise passes, fp16, on the
                 device), .cpu() (fp16 over the link), .float().numpy() (the permuted fp32 (b, c, f, H, W) array), and then save_videos_grid's own
                 cast per frame, permute(1, 2, 0) -> (x * 255).numpy().astype(uint8), WITHOUT the grid of three clips and without JPEG encoding
    uint8 path   vae.decode_u8 per batch straight into one (f, H, W, 3) device buffer, .cpu() (bytes over the link); the writer takes the frames
                 as they are (host conversion = 0 by construction: Image.fromarray shares the buffer)

Each path is split into VAE decode / tail on the device / copy to the host / host conversion with a device synchronisation between the stages
(wall clock, time.perf_counter): one warm-up pass, then --reps timed passes; the median, the minimum and the maximum of every stage are recorded.
The decode stages of the two paths differ by one md_unpack_nhwc_f16 per batch (float path) against one md_frames_u8 per batch (uint8 path); the
"tail on the device" of the uint8 path is therefore 0 and its kernel is timed alone: 200 back-to-back calls between two HIP events, NHWC source
(the decoder's) and NCHW source (the tiled decode's).  Peak host RSS: each path runs once more in a FRESH child process (a process's peak cannot
be reset), which reports ru_maxrss after its pass minus ru_maxrss before it.  Before anything is timed, both paths are held to the package on a small
clip: the float path's frames must be the images save_videos_grid builds from decode_latents' array, the uint8 path's those of
decode_latents(output_type="uint8"); the run stops if either differs.

    python tools/time_frame_output.py [--configs 16x768,48x1024] [--reps 5] [--out profiles/frame_output_timing.json]
"""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VAE_BATCH = 8
STAGES = ("vae_decode_ms", "device_tail_ms", "copy_to_host_ms", "host_conversion_ms")


def build_vae(dev):
    from mikudance_amd import AutoencoderKL
    from mikudance_amd.synth import synth_state_dict
    vae = AutoencoderKL()
    vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=77), strict=True)
    return vae.half().to(dev).eval()


def latents(frames, size, dev):
    g = torch.Generator().manual_seed(size + frames)
    return torch.randn(frames, 4, size // 8, size // 8, generator=g).half().to(dev)


def _lap(t):
    torch.cuda.synchronize()
    now = time.perf_counter()
    t.append(now)


def float_path(vae, z):
    """-> (the list of uint8 (H, W, 3) arrays the writer gets, the four stage times in ms)."""
    t = []
    _lap(t)
    video = torch.cat([vae.decode(z[i:i + VAE_BATCH]).sample for i in range(0, z.shape[0], VAE_BATCH)])
    _lap(t)
    video = video.reshape((-1, z.shape[0]) + tuple(video.shape[1:])).permute(0, 2, 1, 3, 4)
    video = (video / 2 + 0.5).clamp(0, 1)
    _lap(t)
    host = video.cpu()
    _lap(t)
    arr = torch.from_numpy(host.float().numpy())                              # what __call__(output_type="tensor") returns
    frames = [(x[0].permute(1, 2, 0) * 255).numpy().astype(np.uint8) for x in arr.permute(2, 0, 1, 3, 4)]        # save_videos_grid's cast, one clip
    _lap(t)
    return frames, [1e3 * (b - a) for a, b in zip(t, t[1:])]


def u8_path(vae, z):
    t = []
    _lap(t)
    H = 8 * z.shape[2]
    video = torch.empty((z.shape[0], H, 8 * z.shape[3], 3), device=z.device, dtype=torch.uint8)
    for i in range(0, z.shape[0], VAE_BATCH):
        vae.decode_u8(z[i:i + VAE_BATCH], out=video[i:i + VAE_BATCH])
    _lap(t)
    _lap(t)                                                                    # no tail on the device: the bytes are the decode's own output
    host = video.cpu()
    _lap(t)
    frames = list(host.numpy())                                                # views: the writer takes them as they are
    _lap(t)
    return frames, [1e3 * (b - a) for a, b in zip(t, t[1:])]


PATHS = {"float": float_path, "uint8": u8_path}


def paths_equal_the_package(vae, dev):
    """The two timed paths restate the package's code in stages; this holds them to it: on a small clip, float_path's frames must be the images
    save_videos_grid builds from MikuDanceVideoPipeline.decode_latents' array, and u8_path's the frames of decode_latents(output_type="uint8")."""
    import types
    from mikudance_amd import io_utils as U
    from mikudance_amd.pipeline_mikudance import MikuDanceVideoPipeline as P
    pipe = types.SimpleNamespace(vae=vae, vae_batch=VAE_BATCH)
    pipe._decode_u8, pipe._decode_frames = types.MethodType(P._decode_u8, pipe), types.MethodType(P._decode_frames, pipe)
    lat = torch.randn(1, 4, 10, 32, 32, generator=torch.Generator().manual_seed(3)).half().to(dev)
    images, keep = [], U.save_videos_from_pil
    U.save_videos_from_pil = lambda pils, path, fps=8: images.extend(pils)
    try:
        U.save_videos_grid(torch.from_numpy(P.decode_latents(pipe, lat)), "unused.mp4")
    finally:
        U.save_videos_from_pil = keep
    z = (1 / 0.18215 * lat).permute(0, 2, 1, 3, 4).reshape(-1, 4, 32, 32).to(vae.dtype)             # decode_latents' own first lines
    ok_float = len(images) == 10 and all(np.array_equal(np.asarray(im), f) for im, f in zip(images, float_path(vae, z)[0]))
    ok_u8 = all(np.array_equal(a, b) for a, b in zip(P.decode_latents(pipe, lat, output_type="uint8")[0].numpy(), u8_path(vae, z)[0]))
    return bool(ok_float), bool(ok_u8)


def child(path, frames, size):
    """One pass of one path in a fresh process -> its growth of the peak RSS, in MiB, as JSON on stdout."""
    dev = torch.device("cuda:0")
    vae = build_vae(dev)
    z = latents(frames, size, dev)
    PATHS[path](vae, z[:VAE_BATCH])                                            # warm-up: kernels loaded, allocator primed
    torch.cuda.synchronize()
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    out, _ = PATHS[path](vae, z)
    after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    held = sum(f.nbytes for f in out)
    print(json.dumps(dict(peak_rss_growth_mib=round((after - before) / 1024, 1), peak_rss_mib=round(after / 1024, 1),
                          frames_held_mib=round(held / 2 ** 20, 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="16x768,48x1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=3, metavar=("PATH", "FRAMES", "SIZE"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), int(a.child[2]))
    memory = {}
    for cfg in a.configs.split(","):                                           # first, before this process opens the device: a fresh process per pass
        frames, size = cfg.split("x")                                          # (a process's peak RSS cannot be reset), one at a time
        for name in PATHS:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, frames, size], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError(f"child {name} {cfg} failed ({p.returncode}): {p.stderr[-2000:]}")
            memory[cfg, name] = json.loads(p.stdout.strip().splitlines()[-1])
            print(cfg, name, "host memory", memory[cfg, name], flush=True)
    from mikudance_amd import ops
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    vae = build_vae(dev)
    result = {"config": dict(vae_batch=VAE_BATCH, reps=a.reps, weights="synthetic, seed 77", clock="perf_counter with a device synchronisation per stage",
                             kernel_calls=200), "runs": {}}
    result["config"]["float_path_equals_decode_latents_and_save_videos_grid"], result["config"]["uint8_path_equals_decode_latents_uint8"] = \
        paths_equal_the_package(vae, dev)
    assert result["config"]["float_path_equals_decode_latents_and_save_videos_grid"] and result["config"]["uint8_path_equals_decode_latents_uint8"]
    for cfg in a.configs.split(","):
        frames, size = (int(v) for v in cfg.split("x"))
        z = latents(frames, size, dev)
        rec = {}
        outs = {}
        for name, fn in PATHS.items():
            fn(vae, z[:VAE_BATCH])                                             # warm-up
            laps = []
            for _ in range(a.reps):
                outs[name], ms = fn(vae, z)
                laps.append(ms)
            cols = list(zip(*laps))
            rec[name] = {s: dict(median=round(statistics.median(c), 2), min=round(min(c), 2), max=round(max(c), 2)) for s, c in zip(STAGES, cols)}
            tails = [sum(l[1:]) for l in laps]
            totals = [sum(l) for l in laps]
            rec[name]["tail_after_decode_ms"] = dict(median=round(statistics.median(tails), 2), min=round(min(tails), 2), max=round(max(tails), 2))
            rec[name]["total_ms"] = dict(median=round(statistics.median(totals), 2), min=round(min(totals), 2), max=round(max(totals), 2))
            rec[name]["device_to_host_mib"] = round(frames * size * size * 3 * (2 if name == "float" else 1) / 2 ** 20, 1)
            print(cfg, name, json.dumps(rec[name]), flush=True)
        rec["frames_equal"] = bool(all(np.array_equal(x, y) for x, y in zip(outs["float"], outs["uint8"])))
        del outs
        # the kernel alone: 200 back-to-back calls between two events, the decoder's NHWC image and a finished NCHW tensor, one VAE batch
        g = torch.Generator().manual_seed(1)
        nhwc = (torch.rand(VAE_BATCH, size, size, 3, generator=g) * 3 - 1.5).half().to(dev)
        nchw = nhwc.permute(0, 3, 1, 2).contiguous()
        out = torch.empty((VAE_BATCH, size, size, 3), device=dev, dtype=torch.uint8)
        ld8 = torch.zeros((VAE_BATCH, size, size, 8), device=dev, dtype=nhwc.dtype)                  # the temporal decoder's image: pixel pitch 8
        ld8[..., :3] = nhwc
        for label, src in (("nhwc", nhwc.permute(0, 3, 1, 2)), ("nchw", nchw), ("nhwc_ld8", ld8[..., :3].permute(0, 3, 1, 2))):
            for _ in range(10):
                ops.frames_u8(src, out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                ops.frames_u8(src, out)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / 200
            rec[f"kernel_{label}_batch8"] = dict(us_per_call=round(us, 2), gb_per_s=round(3.0 * out.numel() / us / 1e3, 1))
        # the three torch passes the kernel replaces, on the same batch, the same way
        for _ in range(3):
            (nchw / 2 + 0.5).clamp(0, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            (nchw / 2 + 0.5).clamp(0, 1)
        e1.record()
        torch.cuda.synchronize()
        rec["torch_three_passes_batch8"] = dict(us_per_call=round(e0.elapsed_time(e1) * 1e3 / 200, 2))
        del nhwc, nchw, out, z
        torch.cuda.empty_cache()
        for name in PATHS:
            rec[name]["host_memory"] = memory[cfg, name]
        print(cfg, json.dumps(rec), flush=True)
        result["runs"][cfg] = rec
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(result, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
