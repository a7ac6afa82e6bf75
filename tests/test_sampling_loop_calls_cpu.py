"""CPU: what MikuDanceVideoPipeline.denoise() and __call__ ask of the operators and of both UNets, and what they refuse, pinned against a recording.

tests/golden/sampling_loop_calls.json holds what the loop did BEFORE its keywords were resolved into one checked sampling plan and its step
into one call: for every case of LOOPS (four samplers x five guidance modes x CFG on / off, and the combinations below them), in order,
every emulated tail operator call (window_accumulate*, cfg_*, add_noise, free_init_mix) with its scalar record, the number of token_pool /
token_blur calls, and every forward_nhwc call of either UNet (nb, f, the timestep, which keywords were given, the number of selected blocks and
sigma of a perturbation, the sorted (factor, mode) pairs of a K / V plan, halves_identical, two_queues); and for every case of REFUSALS, through
denoise() and through __call__, the exception's type and full message, how many UNet methods had run (none) and which emulated operators (none).
The loop must still do exactly that: floats are compared to 1e-12 relative (the bound of the scheduler tests for host coefficients), everything
else exactly.  PARENT_RAISES is the checklist of the `raise` statements the entry points could reach then; every one is in the table.
One difference is permitted: __call__ then asked den.pag_blocks for PAG's blocks before it refused seg_scale > 0 beside pag_scale > 0, so the
recording holds one UNet call for "seg+pag" through __call__; no model-free refusal may now be preceded by any, and the test asks for none.

The recording was made at the parent commit with this module and the old spelling of the installer:

    import pytest, test_sampling_loop_calls_cpu as t
    import apg_ref, free_init_ref, seg_ref
    from mikudance_amd import ops
    from mikudance_amd.selftest import build_models
    def old(mp):
        seg_ref.install(mp)                              # fake_ops, the *_pag steps, token_pool, token_blur
        for name in apg_ref.NAMES:
            mp.setattr(ops, name, getattr(apg_ref, name), raising=False)
        mp.setattr(ops, "free_init_mix", free_init_ref.free_init_mix, raising=False)
    small = build_models(device="cpu")
    with pytest.MonkeyPatch.context() as mp:
        t.dump({"loops": t.trace_loops(mp, small, old)[0], "refusals": t.trace_refusals(mp, small, old)}, t.GOLDEN)
"""
import json
import math
import numbers
import os

import numpy as np
import pytest
import torch

import mikudance_amd as M
from mikudance_amd.selftest import SCHED_KWARGS

import fake_ops
from loop_helpers import CountingUNet, small_cpu, small_inputs, zero_inputs  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "sampling_loop_calls.json")
LAYERS = ("mid", "up_blocks.1")
STEPS = 3


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


def _sde():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, algorithm_type="sde-dpmsolver++")


def _adaptive(scale, steps):
    """The pag_adaptive_scale with which s_t = max(scale - adaptive (1000 - t), 0) is 0 at the last of `steps` timesteps, and only there."""
    sch = _ddim()
    sch.set_timesteps(steps)
    ts = [int(t) for t in sch.timesteps]
    adaptive = scale / (1000 - ts[-1])
    at = [M.MikuDanceVideoPipeline._pag_scale_at(scale, adaptive, t) for t in ts]
    assert all(s > 0.0 for s in at[:-1]) and at[-1] == 0.0, at
    return adaptive


SAMPLERS = {"ddim": (_ddim, 0.0), "ddim-eta": (_ddim, 0.5), "2m": (_dpm, 0.0), "2m-sde": (_sde, 0.0)}
GUIDES = {"plain": {}, "rescale": dict(guidance_rescale=0.7), "apg": dict(apg=True, apg_momentum=-0.5, apg_eta=0.5, apg_norm_threshold=2.0),
          "pag": dict(pag_scale=3.0, pag_adaptive_scale=_adaptive(3.0, STEPS), pag_applied_layers=LAYERS),
          "seg": dict(seg_scale=3.0, seg_blur_sigma=1.5, seg_applied_layers=LAYERS)}
# case -> sampler, guidance_scale, the keywords; and, where not the default, frames (2), steps (STEPS), init (False), reuse (True)
LOOPS = {f"{s}/{g}/{'cfg' if c > 1.0 else 'nocfg'}": dict(sampler=s, guidance=c, kw=GUIDES[g]) for s in SAMPLERS for g in GUIDES for c in (3.5, 1.0)}
LOOPS.update({
    "open-pyramid-pag": dict(sampler="ddim", guidance=3.5, frames=12, steps=2,
                             kw=dict(context_schedule="uniform_open", context_fuse="pyramid", context_frames=8, context_overlap=4, pag_scale=3.0,
                                     pag_applied_layers=LAYERS)),
    "free-init-fast-apg": dict(sampler="ddim", guidance=3.5, frames=4, steps=2,
                               kw=dict(free_init_iters=2, free_init_fast=True, apg=True, apg_momentum=-0.5, apg_eta=0.5, apg_norm_threshold=2.0)),
    "v2v-2m-seg": dict(sampler="2m", guidance=3.5, steps=4, init=True, kw=dict(strength=0.5, seg_scale=3.0, seg_blur_sigma=1.5, seg_applied_layers=LAYERS)),
    "kv-pag": dict(sampler="ddim", guidance=3.5, steps=2, kw=dict(kv_downsample=(2,), pag_scale=3.0, pag_applied_layers=LAYERS)),
    "literal-reference": dict(sampler="ddim", guidance=3.5, steps=2, reuse=False, kw={}),
    "seg-inf": dict(sampler="ddim", guidance=3.5, steps=2, kw=dict(seg_scale=3.0, seg_blur_sigma=math.inf, seg_applied_layers=LAYERS))})


# ---- recording
def jsonable(v):
    if isinstance(v, (bool, str)) or v is None:
        return v
    if isinstance(v, numbers.Integral):
        return int(v)
    if isinstance(v, numbers.Real):
        return float(v)
    if isinstance(v, dict):
        return {k: jsonable(x) for k, x in v.items()}
    return [jsonable(x) for x in v]


def dump(got, path):
    """One case per line, so that a changed case shows as a changed line."""
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(sec) + ": {\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(jsonable(v), sort_keys=True)}"
                                                                             for k, v in cases.items()) + "\n}" for sec, cases in got.items()) + "\n}\n")


def _inputs8(frames, seed):
    """small_inputs cut down to an 8 x 8 latent, fp16."""
    lat, rl, emb = small_inputs(frames, seed)
    return lat[..., :8, :8].contiguous().half(), rl[..., :8, :8].contiguous().half(), emb.half()


def _record_unets(monkeypatch, ref, den, log):
    real_ref, real_den = ref.forward_nhwc, den.forward_nhwc

    def ref_forward(x, *a, **kw):
        log.append(dict(unet="ref", rows=x.shape[0]))
        return real_ref(x, *a, **kw)

    def den_forward(x, nb, f, timesteps, cross, **kw):
        rec = dict(unet="den", nb=nb, f=f, t=float(timesteps[0]), keywords=sorted(kw), halves_identical=kw.get("halves_identical"),
                   two_queues=kw.get("two_queues"))
        if kw.get("pag") is not None:
            rec.update(blocks=len(kw["pag"]))
        if kw.get("seg") is not None:
            rec.update(blocks=len(kw["seg"][0]), sigma=repr(float(kw["seg"][1])))
        if kw.get("kv_downsample") is not None:
            rec.update(kv=sorted(kw["kv_downsample"].values()))
        log.append(rec)
        return real_den(x, nb, f, timesteps, cross, **kw)

    monkeypatch.setattr(ref, "forward_nhwc", ref_forward, raising=False)
    monkeypatch.setattr(den, "forward_nhwc", den_forward, raising=False)


def run_loop(small, spec, unet_log):
    """One denoise() of the case -> (its record, its output)."""
    ref, den, _, _ = small
    make, eta = SAMPLERS[spec["sampler"]]
    frames = spec.get("frames", 2)
    lat, rl, emb = _inputs8(frames, 300 + frames)
    kw = dict(spec["kw"])
    if spec.get("init"):
        kw["init_latents"] = _inputs8(frames, 400 + frames)[0] * 0.18215
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, make())
    pipe.reference_reuse = spec.get("reuse", True)
    del fake_ops.CALLS[:], unet_log[:]
    out = pipe.denoise(lat, rl, emb if spec["guidance"] > 1.0 else emb[1:], spec.get("steps", STEPS), spec["guidance"], eta=eta,
                       generator=torch.Generator().manual_seed(5), **kw)
    tail = [[n, d] for n, d in fake_ops.CALLS if n in fake_ops.TAIL or n.startswith("cfg_") or n == "free_init_mix"]
    tokens = {name: len([1 for n, _ in fake_ops.CALLS if n == name]) for name in ("token_pool", "token_blur")}
    return jsonable(dict(tail=tail, tokens=tokens, unets=list(unet_log))), out


def trace_loops(monkeypatch, small, install=fake_ops.install, cases=None):
    """({case: record}, {case: output}) of the named cases of LOOPS (all of them without names) on the emulated operators."""
    install(monkeypatch)
    log = []
    _record_unets(monkeypatch, small[0], small[1], log)
    records, outputs = {}, {}
    for case in cases or LOOPS:
        records[case], outputs[case] = run_loop(small, LOOPS[case], log)
    return records, outputs


# ---- refusals
nan, inf = float("nan"), float("inf")
PAG3, SEG3 = dict(pag_scale=3.0), dict(seg_scale=3.0)
# case -> kw, and where needed: init (an initial clip is given), entries (default both), model (the small UNets instead of CountingUNets),
#         latent (denoise: the latents' shape), size (__call__: (W, H)), scheduler, eta, init_shape, video_frames,
#         mid_without_attention (the small denoising UNet's mid block says it has no spatial transformer)
REFUSALS = {
    "fuse": dict(kw=dict(context_fuse="pyramids")),
    "fi-iters": dict(kw=dict(free_init_iters=0)),
    "fi-iters-bool": dict(kw=dict(free_init_iters=True)),
    "fi-filter": dict(kw=dict(free_init_filter="box")),
    "fi-order": dict(kw=dict(free_init_order=0)),
    "fi-spatial": dict(kw=dict(free_init_spatial_stop=-0.1)),
    "fi-temporal": dict(kw=dict(free_init_temporal_stop=nan)),
    "fi-with-init": dict(kw=dict(free_init_iters=2), init=True),
    "fi-axis": dict(kw=dict(free_init_iters=2), latent=(1, 4, 2, 2, 257), size=(2056, 32)),
    "rescale-high": dict(kw=dict(guidance_rescale=1.5)),
    "rescale-nan": dict(kw=dict(guidance_rescale=nan)),
    "strength-zero": dict(kw=dict(strength=0.0), init=True),
    "strength-high": dict(kw=dict(strength=1.5), init=True),
    "strength-without-init": dict(kw=dict(strength=0.5)),
    "strength-no-step": dict(kw=dict(strength=0.1), init=True),
    "apg-eta": dict(kw=dict(apg_eta=1.5)),
    "apg-threshold": dict(kw=dict(apg_norm_threshold=-1.0)),
    "apg-momentum": dict(kw=dict(apg_momentum=1.0)),
    "apg-off-eta": dict(kw=dict(apg=False, apg_eta=inf)),
    "apg+rescale": dict(kw=dict(apg=True, guidance_rescale=0.7)),
    "pag-scale": dict(kw=dict(pag_scale=-0.1)),
    "pag-scale-inf": dict(kw=dict(pag_scale=inf)),
    "pag-adaptive": dict(kw=dict(pag_adaptive_scale=-1e-3)),
    "pag-layers-not-a-sequence": dict(kw=dict(pag_applied_layers=3)),
    "pag-layer-unknown": dict(kw=dict(PAG3, pag_applied_layers=("middle",))),
    "pag-off-layer-unknown": dict(kw=dict(pag_applied_layers=("down_blocks.x",))),
    "pag-layers-empty": dict(kw=dict(PAG3, pag_applied_layers=())),
    "pag+rescale": dict(kw=dict(PAG3, guidance_rescale=0.7)),
    "pag+apg": dict(kw=dict(PAG3, apg=True)),
    "kv-not-a-sequence": dict(kw=dict(kv_downsample=2.5)),
    "kv-factor": dict(kw=dict(kv_downsample=(2, 9))),
    "kv-factor-bool": dict(kw=dict(kv_downsample=(True,))),
    "kv-mode": dict(kw=dict(kv_downsample_mode="max")),
    "kv-grid": dict(kw=dict(kv_downsample=8)),
    "seg-not-numbers": dict(kw=dict(seg_scale="high")),
    "seg-sigma-none": dict(kw=dict(seg_blur_sigma=None)),
    "seg-scale": dict(kw=dict(seg_scale=-1.0)),
    "seg-sigma-zero": dict(kw=dict(seg_blur_sigma=0.0)),
    "seg-sigma-nan": dict(kw=dict(seg_blur_sigma=nan)),
    "seg-layers-not-a-sequence": dict(kw=dict(seg_applied_layers=3)),
    "seg-layer-unknown": dict(kw=dict(SEG3, seg_applied_layers=("mid", "up_blocks.1.attn1"))),
    "seg-layers-empty": dict(kw=dict(SEG3, seg_applied_layers=())),
    "seg+pag": dict(kw=dict(SEG3, pag_scale=3.0)),
    "seg+rescale": dict(kw=dict(SEG3, guidance_rescale=0.7)),
    "seg+apg": dict(kw=dict(SEG3, apg=True)),
    "init-shape": dict(kw={}, init=True, init_shape=(1, 4, 2, 2, 3), entries=("denoise",)),
    "pag-selects-no-block": dict(kw=dict(PAG3, pag_applied_layers=("mid", "down_blocks.3")), model=True),
    "seg-selects-no-block": dict(kw=dict(SEG3, seg_applied_layers=("up_blocks.0",)), model=True),
    "kv-more-factors-than-levels": dict(kw=dict(kv_downsample=(1, 1, 1, 1, 2)), model=True, latent=(1, 4, 2, 32, 32), size=(256, 256)),
    "kv-level-without-attention": dict(kw=dict(kv_downsample=(1, 1, 1, 2)), model=True, mid_without_attention=True, latent=(1, 4, 2, 16, 16),
                                       size=(128, 128)),
    "scheduler-type": dict(kw={}, scheduler=lambda: object(), entries=("denoise",)),
    "eta-multistep": dict(kw={}, scheduler=_dpm, eta=0.5, entries=("denoise",)),
    "windows-exceed-motion-table": dict(kw=dict(context_frames=40), model=True, latent=(1, 4, 40, 2, 2), entries=("denoise",)),
    "context-batch-size": dict(kw=dict(context_batch_size=0), entries=("call",)),
    "context-schedule": dict(kw=dict(context_schedule="spiral"), entries=("call",)),
    "video-length": dict(kw={}, video_frames=1, entries=("call",))}

# one entry per `raise` the two entry points could reach at the parent commit, before the loop: a piece of its message -> where it stood
PARENT_RAISES = {
    "context_fuse must be 'flat' or 'pyramid'": "_check_fuse",
    "free_init_iters must be an int >= 1": "free_init.check_arguments",
    "free_init_filter must be one of": "free_init.check_filter",
    "free_init_order must be an int >= 1": "free_init.check_filter",
    "free_init_spatial_stop must be a finite number >= 0": "free_init.check_filter",
    "free_init_temporal_stop must be a finite number >= 0": "free_init.check_filter (the same statement, second name)",
    "free_init_iters > 1 cannot be combined with init_latents / video": "free_init.check_arguments",
    "is outside the FreeInit kernel's range": "free_init.check_arguments",
    "guidance_rescale must be a finite number in [0, 1]": "denoise",
    "strength must be a finite number in (0, 1]": "_check_strength",
    "needs a clip to start from": "_check_strength",
    "the number of pipeline steps is 0 which is < 1": "_check_strength",
    "apg_eta must be a finite number in [0, 1]": "_check_apg",
    "apg_norm_threshold must be a finite number >= 0": "_check_apg",
    "apg_momentum must be a finite number in (-1, 1)": "_check_apg",
    "apg=True cannot be combined with guidance_rescale > 0": "_check_apg",
    "pag_scale must be a finite number >= 0": "_check_pag",
    "pag_adaptive_scale must be a finite number >= 0": "_check_pag",
    "pag_applied_layers must be a sequence of layer names": "check_pag_layer_names",
    "pag_applied_layers: unknown layer name": "check_pag_layer_names",
    "pag_applied_layers is empty": "_check_pag",
    "pag_scale > 0 cannot be combined with guidance_rescale > 0": "_check_pag",
    "pag_scale > 0 cannot be combined with apg=True": "_check_pag",
    "kv_downsample must be an integer or a sequence of integers": "check_kv_downsample",
    "kv_downsample: every factor must be an integer in 1..8": "check_kv_downsample",
    "kv_downsample_mode must be one of": "check_kv_downsample",
    "nothing left to attend to": "check_kv_downsample_grid",
    "seg_scale and seg_blur_sigma must be numbers": "_check_seg",
    "seg_scale must be a finite number >= 0": "_check_seg",
    "seg_blur_sigma must be a finite number > 0 or math.inf": "_check_seg",
    "seg_applied_layers must be a sequence of layer names": "check_pag_layer_names",
    "seg_applied_layers: unknown layer name": "check_pag_layer_names",
    "seg_applied_layers is empty": "_check_seg",
    "seg_scale > 0 cannot be combined with pag_scale > 0": "_check_seg",
    "seg_scale > 0 cannot be combined with guidance_rescale > 0": "_check_seg",
    "seg_scale > 0 cannot be combined with apg=True": "_check_seg",
    "do not match latents of shape": "denoise",
    "pag_applied_layers: 'down_blocks.3' selects no attention block": "pag_blocks",
    "seg_applied_layers: 'up_blocks.0' selects no attention block": "pag_blocks",
    "kv_downsample: 5 factors for a UNet of 4 resolution levels": "kv_downsample_plan",
    "which has no attention block": "kv_downsample_plan",
    "unsupported scheduler": "denoise",
    "eta applies to DDIMScheduler only": "denoise",
    "exceed the motion module's positional-encoding table": "denoise",
    "context_batch_size must be >= 1": "__call__",
    "Unknown context_overlap policy": "__call__ (get_context_scheduler)",
    "they must be equal": "__call__"}


def _caught(fn, counted):
    del fake_ops.CALLS[:]
    with pytest.raises(Exception) as e:
        fn()
    return dict(type=type(e.value).__name__, message=str(e.value), unet_calls=None if counted is None else sum(u.calls for u in counted),
                ops=[n for n, _ in fake_ops.CALLS])


def refuse_denoise(small, spec):
    model = spec.get("model", False)
    refu, den = small[:2] if model else (CountingUNet(), CountingUNet())
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, spec.get("scheduler", _ddim)())
    lat, rl, emb = zero_inputs()
    if "latent" in spec:
        lat = torch.zeros(spec["latent"], dtype=torch.float16)
        rl = torch.zeros((1, lat.shape[2], 22) + tuple(lat.shape[3:]), dtype=torch.float16)
    kw = dict(spec["kw"])
    if spec.get("init"):
        kw["init_latents"] = torch.zeros(spec.get("init_shape", lat.shape), dtype=torch.float16)
    return _caught(lambda: pipe.denoise(lat, rl, emb, 4, 3.5, eta=spec.get("eta", 0.0), **kw), None if model else (refu, den))


def refuse_call(small, spec):
    from PIL import Image
    model = spec.get("model", False)
    refu, den = CountingUNet(), small[1] if model else CountingUNet()
    if not model:
        den.in_channels = 4
    pipe = M.MikuDanceVideoPipeline(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=refu, denoising_unet=den, scheduler=_ddim())
    pipe._device = torch.device("cpu")
    W, H = spec.get("size", (32, 32))
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    kw = dict(spec["kw"])
    if spec.get("init") or "video_frames" in spec:
        kw["video"] = [img] * spec.get("video_frames", 2)
    args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, H // 8, W // 8), dtype=np.float32), W, H, 2, 4, 3.5)
    return _caught(lambda: pipe(*args, generator=torch.Generator().manual_seed(0), **kw), (refu,) if model else (refu, den))


def trace_refusals(monkeypatch, small, install=fake_ops.install, cases=None):
    """{case: {entry point: record}} of the named cases of REFUSALS (all of them without names)."""
    install(monkeypatch)
    out = {}
    for case in cases or REFUSALS:
        spec = REFUSALS[case]
        if spec.get("mid_without_attention"):
            monkeypatch.setattr(small[1].mid_block, "has_cross_attention", False)
        out[case] = {entry: jsonable((refuse_denoise if entry == "denoise" else refuse_call)(small, spec)) for entry in spec.get("entries", ("denoise", "call"))}
        if spec.get("mid_without_attention"):
            monkeypatch.setattr(small[1].mid_block, "has_cross_attention", True)
    return out


# ---- the comparison
def assert_same(got, want, where):
    """Floats to 1e-12 relative, everything else (types, lengths, keys, names, integers, flags) exactly."""
    if isinstance(want, float) and isinstance(got, float):
        assert got == want or abs(got - want) <= 1e-12 * max(abs(got), abs(want)), (where, got, want)
    elif isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), (where, got, want)
        for k in want:
            assert_same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), (where, got, want)
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, f"{where}[{i}]")
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_recording_holds_every_case_and_no_other(recorded):
    assert sorted(recorded["loops"]) == sorted(LOOPS) and len(LOOPS) == 4 * 5 * 2 + 6
    assert sorted(recorded["refusals"]) == sorted(REFUSALS)
    for case, spec in REFUSALS.items():
        assert sorted(recorded["refusals"][case]) == sorted(spec.get("entries", ("denoise", "call"))), case
    # the adaptive scale of the "pag" cases reaches 0 at the last step: that step runs the plain entry and no perturbed evaluation
    for case, rec in recorded["loops"].items():
        if case.split("/")[1:2] == ["pag"]:
            steps = [n for n, _ in rec["tail"] if "_step" in n]
            assert steps[:-1] == [steps[0]] * (STEPS - 1) and steps[0] == steps[-1] + "_pag", (case, steps)
            assert len([u for u in rec["unets"] if "pag" in u.get("keywords", ())]) == STEPS - 1, case


def test_every_refusal_of_the_parent_is_in_the_table(recorded):
    messages = [r["message"] for case in recorded["refusals"].values() for r in case.values()]
    left_out = [piece for piece in PARENT_RAISES if not any(piece in m for m in messages)]
    assert not left_out and len(left_out) / len(PARENT_RAISES) == 0.0, left_out
    for case, entries in recorded["refusals"].items():
        for entry, r in entries.items():
            assert r["ops"] == [] and r["unet_calls"] in ((1,) if (case, entry) == ("seg+pag", "call") else (0, None)), (case, entry, r)
            assert (r["unet_calls"] is None) == (REFUSALS[case].get("model", False) and entry == "denoise"), (case, entry)


@pytest.mark.parametrize("case", list(LOOPS))
def test_loop_issues_the_recorded_calls(monkeypatch, small_cpu, recorded, case):
    got, out = trace_loops(monkeypatch, small_cpu, cases=[case])
    assert torch.isfinite(out[case]).all()
    assert_same(got[case], recorded["loops"][case], case)


@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusal_is_the_recorded_one(monkeypatch, small_cpu, recorded, case):
    got = trace_refusals(monkeypatch, small_cpu, cases=[case])
    want = recorded["refusals"][case]
    if case == "seg+pag":                                                  # the one permitted difference (module docstring)
        want = dict(want, call=dict(want["call"], unet_calls=0))
    assert_same(got[case], want, case)
