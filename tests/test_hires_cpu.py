"""CPU: two-pass high-resolution sampling (hires_scale=) -- the float64 reference of md_latent_resize_f16 (tests/hires_ref.py) against an independent
restatement of the three coordinate rules, the low size and every refusal of MikuDanceVideoPipeline.__call__ (made before the CLIP tower or the VAE
runs), hires_scale=1 against the call without the keyword, the two-pass call on emulated operators against the hand-written composition of two
denoise() calls, the derived low-size scene motion, ops.latent_resize's own checks and the script's flags."""
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mikudance_amd as M
from mikudance_amd import _lib, ops
from mikudance_amd.selftest import SCHED_KWARGS

import fake_ops
import hires_ref as R
from loop_helpers import CountingUNet, fake_pipeline_builder, script_tree, small_cpu  # noqa: F401 (small_cpu: fixture)


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


# ---- 1. the reference against a restatement with explicit loops
def _cubic_inner(s, A=-0.75):
    return ((A + 2.0) * s - (A + 3.0)) * s * s + 1.0


def _cubic_outer(s, A=-0.75):
    return ((A * s - 5.0 * A) * s + 8.0 * A) * s - 4.0 * A


def _axis(ni, no, mode):
    """[(indices, weights)] per output position of one axis: the rules of include/mdance_hip.h, in float64."""
    taps = []
    for o in range(no):
        if mode == "nearest":
            taps.append(([min(int(math.floor((o + 0.5) * ni / no)), ni - 1)], [1.0]))
            continue
        src = (o + 0.5) * ni / no - 0.5
        if mode == "bilinear":
            src = max(src, 0.0)
            i0 = int(math.floor(src))
            t = src - i0
            taps.append(([i0, min(i0 + 1, ni - 1)], [1.0 - t, t]))
        else:
            i0 = int(math.floor(src))
            t = src - i0
            taps.append(([min(max(i0 - 1 + k, 0), ni - 1) for k in range(4)], [_cubic_outer(t + 1.0), _cubic_inner(t), _cubic_inner(1.0 - t), _cubic_outer(2.0 - t)]))
    return taps


def _restated(x, ho, wo, mode):
    xd = x.double().numpy()
    f, hi, wi, _ = xd.shape
    ty, tx = _axis(hi, ho, mode), _axis(wi, wo, mode)
    y = np.zeros((f, ho, wo, 4))
    for oy in range(ho):
        for ox in range(wo):
            for iy, wy in zip(*ty[oy]):
                for ix, wx in zip(*tx[ox]):
                    y[:, oy, ox] += wy * wx * xd[:, iy, ix]
    return torch.from_numpy(y)


@pytest.mark.parametrize("mode", ["nearest", "bilinear", "bicubic"])
def test_reference_agrees_with_the_restated_rules(mode):
    for k, (f, (hi, wi), (ho, wo)) in enumerate(R.SHAPES):
        x = R.random_latents(f, hi, wi, 40 + k)
        ref, want = R.resize_ref(x, ho, wo, mode), _restated(x, ho, wo, mode)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (f, ho, wo, 4)
        assert float((ref - want).abs().max()) <= 1e-12, (mode, hi, wi, ho, wo)
        if (hi, wi) == (ho, wo) or mode == "nearest":
            assert torch.equal(ref.to(torch.float16).double(), ref)                 # a copy of fp16 values
    assert torch.equal(R.resize_ref(x, 128, 128, "nearest")[0, 1::2, 1::2], x[0].double())      # exact 2x: every input pixel four times


def test_the_bound_is_one_fp16_ulp():
    ref = torch.tensor([1.0, 1.0, 0.0, 0.0, 2.0 ** -20, 70000.0, 70000.0], dtype=torch.float64)
    ok = lambda y: R.within_one_ulp(torch.tensor(y, dtype=torch.float64), ref)[0]
    assert ok([1.0 + 2.0 ** -10, 1.0 - 2.0 ** -10, 2.0 ** -24, -2.0 ** -24, 2.0 ** -20 + 2.0 ** -24, math.inf, math.inf])
    assert not ok([1.0 + 2.0 ** -9, 1.0, 0.0, 0.0, 2.0 ** -20, math.inf, math.inf])
    assert not ok([1.0, 1.0, 2.0 ** -23, 0.0, 2.0 ** -20, math.inf, math.inf])
    assert not ok([1.0, 1.0, 0.0, 0.0, 2.0 ** -20, 65504.0, math.inf])               # the reference rounds to +inf: so must y


# ---- 2. the low size and the refusals
def _img(size=(32, 32)):
    from PIL import Image
    return Image.new("RGB", size, (40, 80, 120))


def _counting_pipe(den=None, scheduler=None):
    """The real pipeline on the duck-typed VAE / CLIP, counting the calls of clip_embeds and _encode_many."""
    den = den or CountingUNet()
    den.in_channels = 4
    pipe = M.MikuDanceVideoPipeline(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=CountingUNet(), denoising_unet=den,
                                    scheduler=scheduler or _ddim())
    pipe._device = torch.device("cpu")
    pipe.counts = dict(clip=0, encode=0)
    clip, enc = pipe.clip_embeds, pipe._encode_many

    def clip_embeds(*a, **k):
        pipe.counts["clip"] += 1
        return clip(*a, **k)

    def encode_many(*a, **k):
        pipe.counts["encode"] += 1
        return enc(*a, **k)

    pipe.clip_embeds, pipe._encode_many = clip_embeds, encode_many
    return pipe


def _args(W, H, frames=2, steps=4):
    img = _img()
    return (img, img, [img] * frames, [img] * frames, [img] * frames, np.zeros((frames, 2, H // 8, W // 8), dtype=np.float32), W, H, frames, steps, 3.5)


def test_low_size_rounding():
    pipe = _counting_pipe()
    plan = lambda h, w, s, **kw: pipe.hires_plan(h, w, 20, s, **kw)
    assert plan(1024, 1024, 2) == (512, 512, 20) and plan(768, 768, 1.5) == (512, 512, 20)
    assert plan(1024, 768, 2.0, hires_steps=30) == (512, 384, 30)
    assert plan(1000, 1000, 1.5) == (8 * round(1000 / 1.5 / 8), 8 * round(1000 / 1.5 / 8), 20) == (664, 664, 20)    # 83.33 -> 83
    assert plan(720, 1080, 1.7) == (8 * round(720 / 1.7 / 8), 8 * round(1080 / 1.7 / 8), 20) == (424, 632, 20)      # 52.9 -> 53, 79.4 -> 79
    assert plan(880, 880, 2) == (440, 440, 20) and plan(848, 848, 2) == (424, 424, 20)      # 55 exactly; 53 exactly
    assert plan(200, 200, 2) == (96, 96, 20) and plan(216, 216, 3) == (72, 72, 20)          # 12.5 -> 12 (halves to even); 9 exactly
    for one in (1, 1.0, np.float32(1.0)):
        assert plan(768, 768, one) is None
    assert plan(128, 128, 2) == (64, 64, 20)                                                # 64 is allowed, 56 is not
    with pytest.raises(ValueError, match="side below 64"):
        plan(128, 112, 2)


REFUSED = [  # (W, H, keywords, message)
    (128, 128, dict(hires_scale=0.5), "hires_scale must be"), (128, 128, dict(hires_scale=float("nan")), "hires_scale must be"),
    (128, 128, dict(hires_scale=float("inf")), "hires_scale must be"), (128, 128, dict(hires_scale="big"), "must be numbers"),
    (128, 128, dict(hires_scale=-2), "hires_scale must be"), (128, 128, dict(hires_scale=0), "hires_scale must be"),
    (128, 128, dict(hires_scale=2, hires_strength=0.0), "hires_strength must be"), (128, 128, dict(hires_scale=2, hires_strength=1.0), "hires_strength must be"),
    (128, 128, dict(hires_scale=2, hires_strength=1.5), "hires_strength must be"), (128, 128, dict(hires_scale=2, hires_strength=float("nan")), "hires_strength must be"),
    (128, 128, dict(hires_strength=1.0), "hires_strength must be"),                        # checked with the feature off too
    (128, 128, dict(hires_scale=2, hires_mode="lanczos"), "hires_mode must be"), (128, 128, dict(hires_mode="area"), "hires_mode must be"),
    (128, 128, dict(hires_scale=2, hires_steps=0), "hires_steps must be"), (128, 128, dict(hires_scale=2, hires_steps=2.5), "hires_steps must be"),
    (128, 128, dict(hires_scale=2, hires_steps=True), "hires_steps must be"),
    (96, 128, dict(hires_scale=2), "side below 64"), (128, 96, dict(hires_scale=2), "side below 64"), (256, 256, dict(hires_scale=5), "side below 64"),
    (128, 128, dict(hires_scale=1.01), "side of the full size"), (256, 128, dict(hires_scale=1.03), "side of the full size"),      # 248 x 128: one side is enough
    (128, 128, dict(hires_scale=2, video=2), "video= cannot be combined"),
    (128, 128, dict(hires_scale=2, strength=0.5), r"hires pass 1 \(64 x 64\): .*needs a clip"),
    (128, 128, dict(hires_scale=2, hires_steps=1), r"hires pass 2 \(128 x 128\): After adjusting the num_inference_steps"),
    (128, 128, dict(hires_scale=2, hires_strength=0.2), r"hires pass 2 \(128 x 128\): After adjusting"),             # int(4 * 0.2) = 0
    (144, 144, dict(hires_scale=2, tile_attention=2), r"hires pass 1 \(72 x 72\): "),       # 2 divides the 18 x 18 grid, not the 9 x 9 one
    (144, 144, dict(hires_scale=1.5, tile_attention=4), r"hires pass 2 \(144 x 144\): "),   # 4 divides the 12 x 12 grid, not the 18 x 18 one
    (128, 128, dict(hires_scale=2, kv_downsample=(1, 1, 1, 2)), r"hires pass 1 \(64 x 64\): "),      # the 1 x 1 level of 8 x 8 has no 2 x 2 block
    (128, 128, dict(hires_scale=2, guidance_rescale=2.0), r"hires pass 1 \(64 x 64\): guidance_rescale"),
    (128, 128, dict(hires_scale=2, scene_motion_lowres_npy=np.zeros((2, 2, 16, 16))), "scene_motion_lowres_npy has shape"),
    (128, 128, dict(hires_scale=2, scene_motion_lowres_npy=np.zeros((3, 2, 8, 8))), "scene_motion_lowres_npy has shape"),
]


@pytest.mark.parametrize("W,H,kw,msg", REFUSED, ids=[f"{i}-{'-'.join(k[2])}" for i, k in enumerate(REFUSED)])
def test_refusals_come_before_clip_and_vae(monkeypatch, W, H, kw, msg):
    R.install(monkeypatch)
    pipe = _counting_pipe()
    kw = dict(kw)
    if "video" in kw:
        kw["video"] = [_img()] * kw["video"]
    with pytest.raises(ValueError, match=msg):
        pipe(*_args(W, H), generator=torch.Generator().manual_seed(0), **kw)
    assert pipe.counts == dict(clip=0, encode=0)
    assert pipe.reference_unet.calls == 0 and not fake_ops.CALLS


def test_the_unets_own_refusals_name_the_pass(monkeypatch, small_cpu):
    """What only the denoising UNet can refuse (_resolve_plan) is asked for both passes as well, still before anything runs."""
    R.install(monkeypatch)
    pipe = _counting_pipe(den=small_cpu[1])
    for kw, msg in ((dict(deep_cache_interval=2, deep_cache_depth=12), r"hires pass 1 \(64 x 64\): "), (dict(pag_scale=1.0, pag_applied_layers=("nowhere",)), r"hires pass 1 \(64 x 64\): "),
                    (dict(kv_downsample=(1, 1, 1, 1, 2)), r"hires pass 1 \(64 x 64\): ")):
        with pytest.raises(ValueError, match=msg):
            pipe(*_args(128, 128), generator=torch.Generator().manual_seed(0), hires_scale=2, **kw)
    assert pipe.counts == dict(clip=0, encode=0) and not fake_ops.CALLS


# ---- 3. hires_scale = 1 is the call without the keyword
def _small_pipe(small_cpu, scheduler):
    ref, den, _, _ = small_cpu
    pipe = M.MikuDanceVideoPipeline(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=ref, denoising_unet=den, scheduler=scheduler)
    pipe._device = torch.device("cpu")
    pipe.hires_min_side = 48                                         # the tests' clips are 128 x 96 -> 64 x 48
    return pipe


def _clip(frames, W, H, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    img = lambda: Image.fromarray(rng.integers(0, 255, (40, 56, 3), dtype=np.uint8))
    return (img(), img(), [img() for _ in range(frames)], [img() for _ in range(frames)], [img() for _ in range(frames)],
            rng.uniform(-0.5, 0.5, (frames, 2, H // 8, W // 8)), W, H, frames)


def test_scale_1_is_the_call_without_the_keyword(monkeypatch, small_cpu):
    R.install(monkeypatch)
    pipe = _small_pipe(small_cpu, _ddim())
    clip = _clip(2, 64, 48, 3)
    runs = []
    for kw in (dict(), dict(hires_scale=1), dict(hires_scale=1.0, hires_strength=0.3, hires_mode="nearest", hires_steps=7)):
        del fake_ops.CALLS[:]
        g = torch.Generator().manual_seed(11)
        out = pipe(*clip, 2, 3.5, generator=g, eta=0.5, **kw).videos
        runs.append((out, list(fake_ops.CALLS), g.get_state()))
    (a, calls_a, state_a), *others = runs
    assert calls_a and fake_ops.tail_calls("cfg_ddim_step")
    for b, calls_b, state_b in others:
        assert torch.equal(a, b)
        assert calls_b == calls_a and not [c for c in calls_b if c[0] == "latent_resize"]
        assert torch.equal(state_a, state_b)                         # the same number of generator draws


# ---- 4. the two-pass call against its composition
@pytest.mark.parametrize("make,eta", [(_ddim, 0.0), (_ddim, 0.5), (_dpm, 0.0)], ids=["ddim", "ddim-eta", "dpm"])
def test_call_is_the_composition_of_two_denoise_calls(monkeypatch, small_cpu, make, eta):
    R.install(monkeypatch)
    pipe = _small_pipe(small_cpu, make())
    W, H, F_, steps, steps_hi, strength = 128, 96, 2, 3, 6, 0.5
    clip = _clip(F_, W, H, 5)
    seen = []
    out = pipe(*clip, steps, 3.5, generator=torch.Generator().manual_seed(21), eta=eta, hires_scale=2, hires_strength=strength, hires_steps=steps_hi,
               callback=lambda i, t, x: seen.append((i, t, tuple(x.shape))), output_type="tensor").videos
    calls = list(fake_ops.CALLS)

    # by hand: the noise of the low size first, then of the full size; conditions of both sizes; denoise, upscale, denoise
    del fake_ops.CALLS[:]
    g = torch.Generator().manual_seed(21)
    emb = pipe.clip_embeds(clip[0])
    emb = torch.cat([torch.zeros_like(emb), emb], dim=0)
    noise_lo = pipe.prepare_latents(1, 4, W // 2, H // 2, F_, emb.dtype, pipe._device, g)
    noise = pipe.prepare_latents(1, 4, W, H, F_, emb.dtype, pipe._device, g)
    assert tuple(noise_lo.shape) == (1, 4, F_, 6, 8) and tuple(noise.shape) == (1, 4, F_, 12, 16)
    images = (clip[0], clip[1], [list(clip[2]), list(clip[3]), list(clip[4])])
    rl_lo, _ = pipe._condition_latents(*images, None, pipe.lowres_scene_motion(clip[5], 6, 8), H // 2, W // 2, F_)
    rl, _ = pipe._condition_latents(*images, None, clip[5], H, W, F_)
    low = pipe.denoise(noise_lo, rl_lo, emb, steps, 3.5, eta=eta, generator=g)
    calls_1 = list(fake_ops.CALLS)
    up = pipe.upscale_latents(low, H, W, "bicubic")
    assert tuple(up.shape) == (1, 4, F_, 12, 16) and up.dtype == low.dtype
    calls_up = fake_ops.CALLS[len(calls_1):]
    del fake_ops.CALLS[:]
    high = pipe.denoise(noise, rl, emb, steps_hi, 3.5, eta=eta, generator=g, init_latents=up, strength=strength)
    calls_2 = list(fake_ops.CALLS)
    want = torch.from_numpy(pipe.decode_latents(high))

    assert torch.isfinite(out).all() and tuple(out.shape) == (1, 3, F_, H, W) and torch.equal(out, want)
    assert calls_up == [("latent_resize", dict(F=F_, hi=6, wi=8, ho=12, wo=16, mode="bicubic"))]
    assert calls == calls_1 + calls_up + calls_2                      # pass 1's calls, ONE latent_resize, pass 2's calls
    assert [c[0] for c in calls].count("latent_resize") == 1
    # pass 2 starts from add_noise at the first kept timestep and runs int(hires_steps * hires_strength) steps
    sch = pipe.scheduler
    sch.set_timesteps(steps_hi)
    kept = [int(t) for t in sch.get_timesteps(steps_hi, strength)[0]]
    assert len(kept) == int(steps_hi * strength) == 3
    step_name = "cfg_ddim_step" if make is _ddim else "cfg_multistep_step"
    tail_2 = [(n, d) for n, d in calls_2 if n in fake_ops.TAIL]
    a, b = sch.noise_coefficients(kept[0])
    assert tail_2[0] == ("add_noise", dict(a=a, b=b, keywords=())) and 0.0 < a < 1.0
    assert [n for n, _ in tail_2].count(step_name) == len(kept) and [n for n, _ in calls_1].count(step_name) == steps
    assert not [n for n, _ in calls_1 if n in ("add_noise", "latent_resize")]
    assert {d["hw"] for n, d in calls_1 if n == step_name} == {6 * 8} and {d["hw"] for n, d in tail_2 if n == step_name} == {12 * 16}
    # the callback: pass 1's steps, then pass 2's, the count going on
    sch.set_timesteps(steps)
    first = [int(t) for t in sch.timesteps]
    assert seen == [(i, t, (1, 4, F_, 6, 8)) for i, t in enumerate(first)] + [(steps + k, t, (1, 4, F_, 12, 16)) for k, t in enumerate(kept)]


def test_free_init_belongs_to_pass_1_and_modes_reach_the_operator(monkeypatch, small_cpu):
    R.install(monkeypatch)
    pipe = _small_pipe(small_cpu, _ddim())
    clip = _clip(2, 128, 96, 6)
    out = pipe(*clip, 2, 3.5, generator=torch.Generator().manual_seed(4), hires_scale=2, hires_mode="bilinear", free_init_iters=2).videos
    names = [n for n, _ in fake_ops.CALLS]
    cut = names.index("latent_resize")
    assert names[:cut].count("free_init_mix") == 1 and "free_init_mix" not in names[cut:]
    assert fake_ops.CALLS[cut][1]["mode"] == "bilinear" and torch.isfinite(out).all()
    assert names[:cut].count("cfg_ddim_step") == 4 and names[cut:].count("cfg_ddim_step") == 1


# ---- 5. the conditions of the two passes
def test_derived_scene_motion():
    flow = np.zeros((3, 2, 12, 16))
    flow[:, 0], flow[:, 1] = 2.0, -3.0
    low = M.MikuDanceVideoPipeline.lowres_scene_motion(flow, 6, 8)
    assert low.shape == (3, 2, 6, 8) and low.dtype == np.float64
    assert np.allclose(low[:, 0], 2.0 * 8 / 16, atol=1e-15) and np.allclose(low[:, 1], -3.0 * 6 / 12, atol=1e-15)
    rng = np.random.default_rng(0)
    flow = rng.uniform(-1, 1, (2, 2, 12, 16))
    low = M.MikuDanceVideoPipeline.lowres_scene_motion(flow, 8, 8)       # unequal ratios: x by 8 / 16, y by 8 / 12
    want = F.interpolate(torch.from_numpy(flow), size=(8, 8), mode="bilinear", align_corners=False).numpy()
    assert np.allclose(low[:, 0], want[:, 0] * 0.5, atol=1e-15) and np.allclose(low[:, 1], want[:, 1] * (8 / 12), atol=1e-15)
    with pytest.raises(ValueError, match=r"\(F, 2, h, w\)"):
        M.MikuDanceVideoPipeline.lowres_scene_motion(np.zeros((2, 3, 4, 4)), 2, 2)


def test_each_pass_gets_the_conditions_of_its_size(monkeypatch):
    """Noise order, one CLIP evaluation, one VAE pass per size with that size's images only, and the flow of each pass."""
    R.install(monkeypatch)
    seen = []

    def spy(self, latents, ref_latents, embeds, steps, *a, **kw):
        seen.append(dict(latents=latents.clone(), ref=ref_latents, steps=steps, init=kw.get("init_latents"), strength=kw["strength"], fi=kw["free_init_iters"]))
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    pipe = _counting_pipe()
    sizes = []
    enc = pipe._encode_many
    pipe._encode_many = lambda tensors: (sizes.append({tuple(t.shape[-2:]) for t in tensors}), enc(tensors))[1]
    clip = _clip(3, 160, 128, 8)
    g = torch.Generator().manual_seed(2)
    pipe(*clip, 10, 3.5, generator=g, hires_scale=2, hires_strength=0.3, free_init_iters=3)
    g2 = torch.Generator().manual_seed(2)
    n_lo = torch.randn((1, 4, 3, 8, 10), generator=g2)
    n_hi = torch.randn((1, 4, 3, 16, 20), generator=g2)
    p1, p2 = seen
    assert torch.equal(p1["latents"], n_lo) and torch.equal(p2["latents"], n_hi)      # low first, then full
    assert torch.equal(g.get_state(), g2.get_state())
    assert pipe.counts == dict(clip=1, encode=2) and sizes == [{(64, 80)}, {(128, 160)}]
    assert tuple(p1["ref"].shape) == (1, 3, 22, 8, 10) and tuple(p2["ref"].shape) == (1, 3, 22, 16, 20)
    assert (p1["steps"], p1["init"], p1["strength"], p1["fi"]) == (10, None, 1.0, 3)
    assert (p2["steps"], p2["strength"], p2["fi"]) == (10, 0.3, 1) and tuple(p2["init"].shape) == (1, 4, 3, 16, 20)
    assert torch.equal(p2["init"], pipe.upscale_latents(n_lo, 128, 160, "bicubic"))
    derived = torch.from_numpy(pipe.lowres_scene_motion(clip[5], 8, 10)).float()
    assert torch.equal(p1["ref"][0, :, 20:], derived) and torch.equal(p2["ref"][0, :, 20:], torch.from_numpy(clip[5]).float())
    # an exact low-size flow replaces the derived one
    exact = np.random.default_rng(1).uniform(-1, 1, (3, 2, 8, 10))
    del seen[:]
    pipe(*clip, 10, 3.5, generator=torch.Generator().manual_seed(2), hires_scale=2, scene_motion_lowres_npy=exact, hires_steps=4)
    assert torch.equal(seen[0]["ref"][0, :, 20:], torch.from_numpy(exact).float()) and (seen[0]["steps"], seen[1]["steps"], seen[1]["strength"]) == (10, 4, 0.5)


# ---- 6. the operator's own checks and the script
def test_operator_refuses_without_a_launch():
    x = torch.zeros((2, 4, 4, 4), dtype=torch.float16)
    with pytest.raises(_lib.MdanceHipError, match="GPU"):
        ops.latent_resize(x, 2, 4, 4, 8, 8)
    assert ops.RESIZE_MODES == {"nearest": 0, "bilinear": 1, "bicubic": 2}


def test_script_flags_and_exact_low_grid_flow(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    from mikudance_amd.io_utils import resize_depth
    from mikudance_amd.scene_motion import camera_to_scene_motion
    a = IV.parse_args([])
    assert (a.hires_scale, a.hires_strength, a.hires_mode, a.hires_steps) == (1.0, 0.5, "bicubic", None)
    a = IV.parse_args(["--hires_scale", "2", "--hires_strength", "0.4", "--hires_mode", "bilinear", "--hires_steps", "12"])
    assert (a.hires_scale, a.hires_strength, a.hires_mode, a.hires_steps) == (2.0, 0.4, "bilinear", 12)
    for argv in (["--hires_mode", "lanczos"], ["--hires_scale", "2", "--init_video", "x.mp4"]):
        with pytest.raises(SystemExit):
            IV.parse_args(argv)
    R.install(monkeypatch)
    seen = []

    def spy(self, latents, ref_latents, *a, **kw):
        seen.append((tuple(latents.shape), ref_latents[0, :, 20:].clone(), kw.get("init_latents") is not None, kw["strength"]))
        return latents

    monkeypatch.setattr(IV, "build_pipeline", fake_pipeline_builder(IV))
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path, frames=2, size=128)
    rng = np.random.default_rng(3)
    depth, pose = rng.uniform(0.2, 1.0, (1, size, size)), np.stack([np.eye(4)] * 2)
    pose[1, 0, 3] = 0.3
    np.save(tmp_path / "depth.npy", depth), np.save(tmp_path / "w2c.npy", pose), np.save(tmp_path / "c2w.npy", np.linalg.inv(pose))
    import yaml
    doc = yaml.safe_load(open(cfg))
    doc.update(ref_depth_path=str(tmp_path / "depth.npy"), tgt_w2c_path=str(tmp_path / "w2c.npy"), tgt_c2w_path=str(tmp_path / "c2w.npy"))
    yaml.safe_dump(doc, open(cfg, "w"))
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "4", "--output_dir", str(tmp_path / "out")]
    out = IV.main(base + ["--hires_scale", "2", "--hires_strength", "0.5"])
    assert os.path.exists(out) and len(seen) == 2
    (s1, flow1, init1, st1), (s2, flow2, init2, st2) = seen
    assert s1 == (1, 4, 2, 8, 8) and s2 == (1, 4, 2, 16, 16) and (init1, st1, init2, st2) == (False, 1.0, True, 0.5)
    w2cs, c2ws = [pose[0], pose[1]], [np.linalg.inv(pose)[0], np.linalg.inv(pose)[1]]
    exact = camera_to_scene_motion(w2cs, c2ws, [3.2, 3.2, 1.6, 1.6], resize_depth(depth, (1, 8, 8)), 8, 8, False)
    full = camera_to_scene_motion(w2cs, c2ws, [3.2, 3.2, 1.6, 1.6], resize_depth(depth, (1, 16, 16)), 16, 16, False)
    assert np.abs(exact).max() > 0 and torch.equal(flow1, torch.from_numpy(exact).float()) and torch.equal(flow2, torch.from_numpy(full).float())
    assert not np.allclose(exact, M.MikuDanceVideoPipeline.lowres_scene_motion(full, 8, 8))      # the derived flow is an approximation
    del seen[:]
    IV.main(base)
    assert len(seen) == 1 and seen[0][0] == (1, 4, 2, 16, 16)
