#!/usr/bin/env python
"""How far each sampler is from a fine solve at few steps, on the synthetic weights (a GPU tool, not a test).

Full-width UNets with seeded weights (the geometry of tests/e2e_parity.py), 4 frames, 96 x 96 latents, CFG 3.5, one window.  The reference is
a 200-step DDIM run from the same noise; every other run is compared with it by relative L2 over the final latents:
DDIM, DPM-Solver++ 2M and UniPC (bh2) of orders 2 and 3, each with its corrector on and off, at 6 / 8 / 10 / 15 / 20 steps.
The record also holds the time per call of the three step kernels at the headline latent size (16 frames, 96 x 96, CFG), 200 calls between
two HIP events after a warm-up call.  One JSON line on stdout; --out writes the same record to a file.

What the numbers can and cannot say: the weights are random, so the network is not a trained denoiser and the distances are those of this
ODE, not of image quality.  "10 UniPC steps are as close as 20 DDIM steps" is the hypothesis the table tests, not a premise.

    python tools/unipc_convergence.py [--frames 4] [--latent 96] [--reference_steps 200] [--out profiles/unipc_convergence.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (6, 8, 10, 15, 20)


def samplers():
    from mikudance_amd import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
    from mikudance_amd.selftest import SCHED_KWARGS
    off = tuple(range(1000))
    return {"ddim": lambda: DDIMScheduler(**SCHED_KWARGS),
            "dpmpp_2m": lambda: DPMSolverMultistepScheduler(**SCHED_KWARGS),
            "unipc_2": lambda: UniPCMultistepScheduler(**SCHED_KWARGS, solver_order=2),
            "unipc_2_no_corrector": lambda: UniPCMultistepScheduler(**SCHED_KWARGS, solver_order=2, disable_corrector=off),
            "unipc_3": lambda: UniPCMultistepScheduler(**SCHED_KWARGS, solver_order=3),
            "unipc_3_no_corrector": lambda: UniPCMultistepScheduler(**SCHED_KWARGS, solver_order=3, disable_corrector=off)}


def step_kernel_times(dev, frames=16, latent=96, calls=200):
    """us per call of md_cfg_ddim_step, md_cfg_multistep_step (second order) and md_cfg_unipc_step (order 3, corrector on: every plane read)."""
    from mikudance_amd import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, ops
    from mikudance_amd.selftest import SCHED_KWARGS
    hw = latent * latent
    g = torch.Generator().manual_seed(1)
    lat = torch.randn((frames, hw, 4), generator=g).half().to(dev)
    ns = torch.randn((2, frames, hw, 4), generator=g).to(dev)
    cnt = torch.ones((frames,), device=dev)
    hist = torch.randn((frames, hw, 4), generator=g).to(dev)
    state = torch.randn((4, frames, hw, 4), generator=g).to(dev)
    d, m, u = DDIMScheduler(**SCHED_KWARGS), DPMSolverMultistepScheduler(**SCHED_KWARGS), UniPCMultistepScheduler(**SCHED_KWARGS, solver_order=3)
    for s in (d, m, u):
        s.set_timesteps(10)
    row = u.unipc_coefficients(4)
    assert row[11] and all(v != 0.0 for v in row[2:11])
    calls_ = {"md_cfg_ddim_step": lambda: ops.cfg_ddim_step(lat, ns, cnt, frames, hw, 3.5, *d.step_coefficients(int(d.timesteps[4]))),
              "md_cfg_multistep_step": lambda: ops.cfg_multistep_step(lat, ns, cnt, hist, frames, hw, 3.5, *m.multistep_coefficients(4)),
              "md_cfg_unipc_step": lambda: ops.cfg_unipc_step(lat, ns, cnt, state, frames, hw, 3.5, row)}
    n = frames * hw * 4
    nbytes = {"md_cfg_ddim_step": n * (2 + 2 + 8), "md_cfg_multistep_step": n * (2 + 2 + 8 + 4 + 4), "md_cfg_unipc_step": n * (2 + 2 + 8 + 16 + 16)}
    out = {}
    for name, fn in calls_.items():
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / calls
        out[name] = {"us_per_call": us, "bytes_per_call": nbytes[name], "GB_per_s": nbytes[name] / us / 1e3}
    return {"frames": frames, "latent": latent, "calls": calls, "kernels": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--latent", type=int, default=96)
    ap.add_argument("--reference_steps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from mikudance_amd import MikuDanceVideoPipeline, _lib
    from mikudance_amd.selftest import build_models, rel_l2
    from mikudance_amd.synth import synth_inputs
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ref, den, _, _ = build_models(geom=dict(block_out_channels=(320, 640, 1280, 1280), cross_attention_dim=768), device=dev, keep_state_dicts=False)
    lat, rl, emb = (t.half().to(dev) for t in synth_inputs(a.frames, a.latent, a.latent, ctx_len=257, ctx_dim=768, seed=100))
    make = samplers()

    def run(name, steps):
        out = MikuDanceVideoPipeline(None, None, ref, den, make[name]()).denoise(lat, rl, emb, steps, 3.5)
        torch.cuda.synchronize()
        return out.float().cpu()

    want = run("ddim", a.reference_steps)
    print(f"reference: ddim-{a.reference_steps}", file=sys.stderr, flush=True)
    rec = {"config": {"frames": a.frames, "latent": a.latent, "guidance": 3.5, "weights": "synthetic (seeded)", "reference": f"ddim-{a.reference_steps}",
                      "measure": "relative L2 of the final latents against the reference, same noise"},
           "rel_l2": {}}
    for name in make:
        rec["rel_l2"][name] = {}
        for steps in STEPS:
            rec["rel_l2"][name][str(steps)] = rel_l2(run(name, steps), want)
        print(f"{name}: {rec['rel_l2'][name]}", file=sys.stderr, flush=True)
    rec["step_kernel"] = step_kernel_times(dev)
    rec["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
