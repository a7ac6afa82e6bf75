"""CPU: colour matching (color_match=) off the device.  color_match.transform in float64 on random covariances (the MKL identity, mean_std's
moments, strength, the fallbacks, clip scope); the float32 restatement of md_color_apply tied to frames_ref.u8_ref over every fp16 bit pattern;
__call__(color_match=...) on the emulated operator layer (tests/fake_ops.py + tests/color_match_ref.py) for both modes, both scopes, every target
form, both decoders, tiling and slicing; the call log with and without the keyword; every refusal before the CLIP tower runs; the script's options."""
import types

import numpy as np
import pytest
import torch

import mikudance_amd as M
from mikudance_amd import AutoencoderKL, AutoencoderKLTemporalDecoder, color_match as CM
from mikudance_amd.synth import synth_state_dict

import color_match_ref as R
import fake_ops
import frames_ref
from loop_helpers import script_tree

F16 = torch.float16
CHANS = (64, 64, 64, 64)


# ---- transform
def _stats(rng, n=1000.0):
    """Random colour statistics as nine sums over n pixels: means in [0.2, 0.8], an SPD covariance with standard deviations around 0.1."""
    a = rng.normal(size=(3, 3))
    cov = 0.01 * (a @ a.T / 3 + 0.2 * np.eye(3))
    mu = rng.uniform(0.2, 0.8, 3)
    second = cov + np.outer(mu, mu)
    sums = n * np.array([mu[0], mu[1], mu[2], second[0, 0], second[1, 1], second[2, 2], second[0, 1], second[0, 2], second[1, 2]])
    return sums, n, mu, cov


@pytest.mark.parametrize("seed", range(8))
def test_transform_on_random_covariances(seed):
    rng = np.random.default_rng(seed)
    (ss, ns, mu_s, cov_s), (ts, nt, mu_t, cov_t) = _stats(rng), _stats(rng, 777.0)
    m, t, fb = CM.transform(ss, ns, ts, nt, "mkl", 1.0)
    assert not fb and np.array_equal(m, m.T)
    assert np.abs(m @ cov_s @ m.T - cov_t).max() <= 1e-9 * np.abs(cov_t).max()          # the Monge-Kantorovich map: the whole covariance
    assert np.abs(m @ mu_s + t - mu_t).max() <= 1e-12
    assert np.linalg.eigvalsh(m).min() > 0                                            # the SPD solution, not one of the other roots
    m, t, fb = CM.transform(ss, ns, ts, nt, "mean_std", 1.0)
    assert not fb and np.array_equal(m, np.diag(np.diag(m)))
    assert np.abs(m @ mu_s + t - mu_t).max() <= 1e-12                                 # the target's mean ...
    got_std, want_std = np.sqrt(np.diag(m @ cov_s @ m.T)), np.sqrt(np.diag(cov_t))
    assert np.abs(got_std - want_std).max() <= 1e-12 * want_std.max()                 # ... and its per-channel standard deviation
    for mode in CM.MODES:
        m1, t1, _ = CM.transform(ss, ns, ts, nt, mode, 1.0)
        m0, t0, fb0 = CM.transform(ss, ns, ts, nt, mode, 0.0)
        assert np.array_equal(m0, np.eye(3)) and np.array_equal(t0, np.zeros(3)) and not fb0          # strength 0: the identity, exactly
        for a in (0.25, 0.5, 0.9):                                                                      # linear in the strength
            ma, ta, _ = CM.transform(ss, ns, ts, nt, mode, a)
            assert np.abs(ma - ((1 - a) * np.eye(3) + a * m1)).max() <= 1e-15 and np.abs(ta - a * t1).max() <= 1e-15


def test_transform_falls_back_to_the_mean_shift():
    rng = np.random.default_rng(11)
    (ss, ns, mu_s, cov_s), (ts, nt, mu_t, _) = _stats(rng), _stats(rng)

    def with_variance(sums, n, c, var):
        out = sums.copy()
        out[3 + c] = n * (var + (sums[c] / n) ** 2)
        return out
    assert CM.COLOR_MATCH_EPS == 1e-6
    for mode in CM.MODES:
        for c in range(3):
            for flat in (with_variance(ss, ns, c, 0.9e-6), with_variance(ss, ns, c, 0.0)):
                m, t, fb = CM.transform(flat, ns, ts, nt, mode, 1.0)                     # a flat source channel
                assert fb and np.array_equal(m, np.eye(3)) and np.abs(t - (mu_t - mu_s)).max() <= 1e-15
                m, t, fb = CM.transform(ts, nt, flat, ns, mode, 0.5)                     # a flat target channel, at half strength
                assert fb and np.array_equal(m, np.eye(3)) and np.abs(t - 0.5 * (mu_s - mu_t)).max() <= 1e-15
        var0 = cov_s[0, 0]
        assert not CM.transform(with_variance(ss, ns, 0, max(var0, 1.1e-6)), ns, ts, nt, mode)[2]
        for bad in (np.nan, np.inf):
            broken = ss.copy()
            broken[0] = broken[3] = broken[6] = broken[7] = bad                           # what a NaN in channel 0 leaves
            m, t, fb = CM.transform(broken, ns, ts, nt, mode, 1.0)
            assert fb and np.array_equal(m, np.eye(3)) and t[0] == 0.0 and np.abs(t[1:] - (mu_t - mu_s)[1:]).max() <= 1e-15
    with pytest.raises(ValueError, match="color_match must be"):
        CM.transform(ss, ns, ts, nt, "histogram")


def test_moments_of_image_and_clip_scope():
    rng = np.random.default_rng(5)
    frames = rng.uniform(0, 1, (4, 6, 5, 3))
    per_frame = [CM.moments_of_image(f) for f in frames]
    assert all(n == 30 and s.dtype == np.float64 and s.shape == (9,) for s, n in per_frame)
    s, n = per_frame[0]
    flat = frames[0].reshape(-1, 3)
    mu, cov = CM.mean_cov(s, n)
    assert np.allclose(mu, flat.mean(0), rtol=0, atol=1e-14) and np.allclose(cov, np.cov(flat.T, bias=True), rtol=0, atol=1e-14)
    # the clip's statistics are those of its frames laid side by side: the sums add
    whole, n_whole = CM.moments_of_image(frames.reshape(24, 5, 3))
    summed = np.sum([s for s, _ in per_frame], axis=0)
    assert n_whole == 120 and np.allclose(whole, summed, rtol=1e-14, atol=0)
    tgt, nt = CM.moments_of_image(rng.uniform(0.2, 0.6, (7, 3, 3)))
    for mode in CM.MODES:
        a, b = CM.transform(summed, 120, tgt, nt, mode, 0.7), CM.transform(whole, n_whole, tgt, nt, mode, 0.7)
        assert np.allclose(a[0], b[0], rtol=0, atol=1e-10) and np.allclose(a[1], b[1], rtol=0, atol=1e-10) and not a[2]
    with pytest.raises(ValueError, match="moments_of_image"):
        CM.moments_of_image(np.zeros((4, 4)))
    coef = CM.coefficients([(np.arange(9.0).reshape(3, 3), np.array([9.0, 10, 11]), False)])
    assert coef.dtype == np.float32 and coef.tolist() == [list(map(float, range(12)))]


# ---- the apply restatement
def test_apply_restatement_is_the_fp32_chain_of_frames_u8_over_every_fp16_bit_pattern():
    """With M = I, t = 0 the new chain is s -> ((0 + 1 s_c) + 0 + 0) = s -> trunc(s * 255): the existing fp32 chain's bytes for every fp16 input
    (checked here: 0.5 v + 0.5 and v / 2 + 0.5 agree in fp32 on all 65 536 patterns, NaN -> 0 in both)."""
    x = frames_ref.all_fp16()
    planes = torch.stack([x, x, x]).view(1, 3, 256, 256)                       # the same value in the three channels: 0 * NaN stays in its pixel
    ident = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float32)
    got = torch.from_numpy(R.apply_ref(planes, ident, True))
    want = frames_ref.u8_ref(planes, True).permute(0, 2, 3, 1)
    assert torch.equal(got, want) and len(torch.unique(got)) == 256
    y = R.apply_ref(planes, ident, False)
    assert y.dtype == np.float32 and int(np.isnan(y).sum()) == 3 * 2046        # the float destination keeps a NaN
    assert np.array_equal((np.nan_to_num(y) * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1), got.numpy())


def test_apply_restatement_rows_and_clamp():
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 3, 4, 5, generator=g) * 3 - 1.5).half()
    coef = (torch.randn(3, 12, generator=g) * 1.5).float()
    y = R.apply_ref(x, coef, False)
    s = R.display32(x).astype(np.float64)
    m = coef.double().numpy()
    want = np.clip(np.einsum("bij,bjhw->bihw", m[:, :9].reshape(3, 3, 3), s) + m[:, 9:, None, None], 0, 1)
    assert np.abs(y - want).max() < 1e-5 and (y == 0).any() and (y == 1).any() and ((y > 0) & (y < 1)).any()
    assert np.array_equal(R.apply_ref(x, coef, True), (y * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1))


# ---- the pipeline
def _load(vae, seed=77):
    vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=seed), strict=True)
    return vae.half().eval()


@pytest.fixture(scope="module")
def vae():
    return _load(AutoencoderKL(block_out_channels=CHANS, sample_size=128))


@pytest.fixture(scope="module")
def temporal_vae():
    return _load(AutoencoderKLTemporalDecoder(block_out_channels=CHANS), seed=31)


def _pipe(monkeypatch, vae, cls=M.MikuDanceVideoPipeline, **kw):
    """The real pipeline class and a real (small) VAE on the emulated operators; the CLIP tower is duck-typed and denoise() hands its noise on."""
    R.install(monkeypatch)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", lambda self, latents, *a, **k: latents)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "_resolve_plan", lambda self, plan: plan)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "sampling_plan", lambda self, *a, **k: None)
    pipe = cls(vae=vae, image_encoder=fake_ops.FakeCLIP(), reference_unet=None, denoising_unet=types.SimpleNamespace(in_channels=4),
               scheduler=M.DDIMScheduler(**M.selftest.SCHED_KWARGS), **kw)
    pipe._device = torch.device("cpu")
    return pipe


def _img(rng, size=(24, 24)):
    from PIL import Image
    return Image.fromarray(rng.integers(0, 255, size + (3,), dtype=np.uint8))


def _args(W, H, frames):
    rng = np.random.default_rng(4)
    img = lambda: _img(rng)
    return (img(), img(), [img() for _ in range(frames)], [img()] * frames, [img()] * frames, np.zeros((frames, 2, H // 8, W // 8), dtype=np.float32), W, H,
            frames, 2, 3.5)


def _cast(videos):
    assert videos.dtype == torch.float32 and videos.dim() == 5
    return torch.from_numpy((videos * 255).numpy().astype(np.uint8)).permute(0, 2, 3, 4, 1)


def _both(pipe, args, **kw):
    del fake_ops.CALLS[:]
    want = pipe(*args, generator=torch.manual_seed(3), **kw).videos
    calls_f, maps_f = list(fake_ops.CALLS), getattr(pipe, "last_color_match", None)
    del fake_ops.CALLS[:]
    got = pipe(*args, generator=torch.manual_seed(3), output_type="uint8", **kw).videos
    return want, calls_f, got, list(fake_ops.CALLS), maps_f


def _named(calls, name):
    return [d for n, d in calls if n == name]


W, H, F_ = 32, 16, 3
TARGETS = {"ref_image": lambda: None, "image": lambda: _img(np.random.default_rng(8), (40, 30)), "first_frame": lambda: "first_frame"}


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("scope", CM.SCOPES)
@pytest.mark.parametrize("mode", CM.MODES)
def test_uint8_call_equals_the_float_call_cast(monkeypatch, vae, mode, scope, target):
    pipe = _pipe(monkeypatch, vae)
    pipe.vae_batch = 2
    args = _args(W, H, F_)
    plain = pipe(*args, generator=torch.manual_seed(3)).videos
    tgt = TARGETS[target]()
    want, calls_f, got, calls_u, maps_f = _both(pipe, args, color_match=mode, color_match_scope=scope, color_match_target=tgt)
    assert want.dtype == torch.float32 and tuple(want.shape) == (1, 3, F_, H, W) and float(want.min()) >= 0 and float(want.max()) <= 1
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, F_, H, W, 3) and torch.equal(got, _cast(want))
    assert len(torch.unique(got)) > 20 and not torch.equal(want, plain)            # a picture, and not the unmatched one
    # exactly one color_moments and one color_apply per VAE batch, on the decoder's own NHWC image; no frames_u8, no unpack of the decode
    for calls, dst in ((calls_f, "float32"), (calls_u, "uint8")):
        mo, ap = _named(calls, "color_moments"), _named(calls, "color_apply")
        assert [d["B"] for d in mo] == [2, 1] and [d["B"] for d in ap] == [2, 1] and not _named(calls, "frames_u8")
        assert all(d["strides"] == (H * W * 3, 1, W * 3, 3) and (d["H"], d["W"], d["src"]) == (H, W, "float16") for d in mo + ap)
        assert all(d["dst"] == dst for d in ap)
        order = [n for n, _ in calls if n.startswith("color_")]
        assert order == (["color_moments", "color_apply"] * 2 if scope == "frame" else ["color_moments"] * 2 + ["color_apply"] * 2)
    assert [c for c in calls_u if not c[0].startswith("color_")] == [c for c in calls_f if not c[0].startswith("color_")]
    # the maps: one per frame, the same in both calls; what they do to the frames' statistics
    maps = pipe.last_color_match
    assert len(maps) == F_ and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(maps, maps_f))
    assert not any(fb for _, _, fb in maps)
    if scope == "clip":
        assert all(np.array_equal(maps[0][0], m) and np.array_equal(maps[0][1], t) for m, t, _ in maps)
    else:
        assert not np.array_equal(maps[0][0], maps[1][0])
    if target == "first_frame" and scope == "frame":                               # frame 0 is its own target: the identity, to rounding
        assert np.abs(maps[0][0] - np.eye(3)).max() < 1e-9 and np.abs(maps[0][1]).max() < 1e-9
        assert float((want[0, :, 0] - plain[0, :, 0]).abs().max()) < 1e-3


def test_the_matched_frames_have_the_targets_statistics(monkeypatch, vae):
    """End to end on the emulated layer: after mean_std the frame's channel means and standard deviations are the target's, after mkl its whole
    covariance, up to what the clamp to [0, 1] cuts off (the target is chosen mid-grey and narrow so that it cuts nothing)."""
    from PIL import Image
    pipe = _pipe(monkeypatch, vae)
    rng = np.random.default_rng(12)
    base = rng.normal(0, 1, (20, 20, 3)) @ np.array([[0.05, 0.02, 0.0], [0.0, 0.04, 0.01], [0.0, 0.0, 0.03]])
    target = Image.fromarray(np.clip((0.5 + base) * 255, 0, 255).astype(np.uint8))
    tgt_sums, n_t = CM.moments_of_image(np.asarray(target.resize((W, H), resample=Image.LANCZOS)).astype(np.float32) / 255.0)
    mu_t, cov_t = CM.mean_cov(tgt_sums, n_t)
    for mode in CM.MODES:
        out = pipe(*_args(W, H, 2), generator=torch.manual_seed(3), color_match=mode, color_match_target=target).videos
        assert float(out.min()) > 0 and float(out.max()) < 1                      # nothing clamped
        for f in range(2):
            mu, cov = CM.mean_cov(*CM.moments_of_image(out[0, :, f].permute(1, 2, 0).numpy()))
            assert np.abs(mu - mu_t).max() < 1e-5
            if mode == "mkl":
                assert np.abs(cov - cov_t).max() < 1e-5 * max(1.0, np.abs(cov_t).max() / 1e-3)
            else:
                assert np.abs(np.sqrt(np.diag(cov)) - np.sqrt(np.diag(cov_t))).max() < 1e-5


def test_default_call_log_is_unchanged_and_strength_zero_is_the_plain_result(monkeypatch, vae):
    pipe = _pipe(monkeypatch, vae)
    pipe.vae_batch = 2
    args = _args(W, H, F_)
    plain_f, calls_f, plain_u, calls_u, _ = _both(pipe, args)
    assert not [n for n, _ in calls_f + calls_u if n.startswith("color_")] and not hasattr(pipe, "last_color_match")
    assert len(_named(calls_u, "frames_u8")) == 2 and not _named(calls_f, "frames_u8")                 # today's two logs, as they were
    none_f, calls_nf, none_u, calls_nu, _ = _both(pipe, args, color_match=None)
    assert calls_nf == calls_f and calls_nu == calls_u and torch.equal(none_f, plain_f) and torch.equal(none_u, plain_u)
    # strength 0: the identity map through the new road; its bytes are the fp32 chain's of the same image
    zero_f, _, zero_u, _, _ = _both(pipe, args, color_match="mkl", color_match_strength=0.0)
    assert all(np.array_equal(m, np.eye(3)) and np.array_equal(t, np.zeros(3)) for m, t, _ in pipe.last_color_match)
    assert torch.equal(zero_u, _cast(zero_f)) and float((zero_f - plain_f).abs().max()) < 1e-3                # fp32 s against the float path's fp16 chain


@pytest.mark.parametrize("cls", [M.MikuDanceVideoPipeline, M.Pose2VideoPipeline], ids=["mikudance", "stage2"])
def test_clips_strength_pil_and_numpy(monkeypatch, vae, cls):
    pipe = _pipe(monkeypatch, vae, cls)
    pipe.vae_batch = 4                                                       # a VAE batch that straddles the two clips
    args = _args(W, H, F_)
    other = _img(np.random.default_rng(21))
    kw = dict(num_images_per_prompt=2, color_match="mean_std", color_match_strength=0.6)
    want, calls_f, got, calls_u, _ = _both(pipe, args, color_match_target=[None, other], **kw)
    assert tuple(got.shape) == (2, F_, H, W, 3) and torch.equal(got, _cast(want))
    assert [d["B"] for d in _named(calls_u, "color_moments")] == [4, 2]
    maps = pipe.last_color_match
    assert len(maps) == 2 * F_
    one = pipe(*args, generator=torch.manual_seed(3), output_type="uint8", color_match_target=[other, "first_frame"], **kw).videos
    assert not torch.equal(one[0], got[0]) and not torch.equal(one[1], got[1])             # targets are per clip
    same = pipe(*args, generator=torch.manual_seed(3), output_type="uint8", color_match_target=[None, "first_frame"], **kw).videos
    assert torch.equal(same[0], got[0]) and torch.equal(same[1], one[1])
    # first_frame per clip, clip scope: clip 1's target is ITS frame 0
    pipe(*args, generator=torch.manual_seed(3), output_type="uint8", color_match_target="first_frame", color_match_scope="clip", **kw)
    m = pipe.last_color_match
    assert np.array_equal(m[0][0], m[F_ - 1][0]) and np.array_equal(m[F_][0], m[2 * F_ - 1][0]) and not np.array_equal(m[0][0], m[F_][0])
    pil = pipe(*args, generator=torch.manual_seed(3), output_type="pil", color_match_target=[None, other], **kw).videos
    assert len(pil) == 2 and all(im.size == (W, H) and im.mode == "RGB" for im in pil[1])
    assert torch.equal(torch.from_numpy(np.stack([np.stack([np.asarray(im) for im in clip]) for clip in pil])), got)
    arr = pipe(*args, generator=torch.manual_seed(3), output_type="numpy", color_match_target=[None, other], **kw).videos
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and np.array_equal(arr, want.numpy())
    assert torch.equal(pipe(*args, generator=torch.manual_seed(3), output_type="uint8", return_dict=False, color_match_target=[None, other], **kw), got)


def test_temporal_decoder(monkeypatch, temporal_vae):
    pipe = _pipe(monkeypatch, temporal_vae, video_decoder=True)
    pipe.decode_chunk_size = 2
    for scope in CM.SCOPES:
        want, calls_f, got, calls_u, _ = _both(pipe, _args(W, H, F_), color_match="mkl", color_match_scope=scope)
        assert tuple(got.shape) == (1, F_, H, W, 3) and torch.equal(got, _cast(want))
        mo, ap = _named(calls_u, "color_moments"), _named(calls_u, "color_apply")
        assert [d["B"] for d in mo] == [2, 1] == [d["B"] for d in ap]
        assert all(d["strides"] == (H * W * 8, 1, W * 8, 8) for d in mo + ap)                          # pixel pitch 8, 3 valid channels
    z = torch.randn(4, 4, 2, 4, generator=torch.Generator().manual_seed(1)).half()
    view = temporal_vae.decode_image_view(z, num_frames=2)
    assert tuple(view.shape) == (4, 3, 16, 32) and torch.equal(view, temporal_vae.decode(z, num_frames=2).sample)
    with pytest.raises(ValueError, match="decode_image_view expects"):
        temporal_vae.decode_image_view(z, num_frames=3)


def test_tiling_slicing_interpolation_and_hires(monkeypatch):
    v = _load(AutoencoderKL(block_out_channels=CHANS, sample_size=128))
    pipe = _pipe(monkeypatch, v)
    pipe.vae_batch = 2
    Wt, Ht = 128, 64
    want, calls_f, got, calls_u, _ = _both(pipe, _args(Wt, Ht, 2), vae_tiling=True, vae_tile_size=64, color_match="mkl")
    assert sum(n == "tile_blend" for n, _ in calls_f) > 0 and torch.equal(got, _cast(want))
    mo, ap = _named(calls_u, "color_moments"), _named(calls_u, "color_apply")
    assert len(mo) == 1 == len(ap) and mo[0]["strides"] == ap[0]["strides"] == (3 * Ht * Wt, Ht * Wt, Wt, 1)      # decode's NCHW result, read where it lies
    assert (v.use_tiling, v.tile_sample_min_size) == (False, 128)
    untiled = pipe(*_args(Wt, Ht, 2), generator=torch.manual_seed(3), output_type="uint8", color_match="mkl").videos
    assert not torch.equal(untiled, got)
    z = torch.randn(3, 4, 2, 4, generator=torch.Generator().manual_seed(2)).half()
    plain_view = v.decode_image_view(z)
    assert plain_view.stride() == (16 * 32 * 3, 1, 32 * 3, 3) and torch.equal(plain_view, v.decode(z).sample)
    v.enable_slicing()
    try:
        sliced = v.decode_image_view(z)
        assert sliced.is_contiguous() and torch.equal(sliced, v.decode(z).sample)
        want, _, got, calls_u, _ = _both(pipe, _args(W, H, F_), color_match="mean_std", color_match_scope="clip")
        assert torch.equal(got, _cast(want)) and [d["strides"] for d in _named(calls_u, "color_moments")] == [(3 * H * W, H * W, W, 1), (H * W * 3, 1, W * 3, 3)]
    finally:
        v.disable_slicing()
    with pytest.raises(ValueError, match="expects"):
        v.decode_image_view(torch.zeros(1, 3, 4, 4, dtype=F16))
    from mikudance_amd import pipeline_mikudance as PM
    monkeypatch.setattr(PM, "tensor_interpolation", PM.linear)
    want, _, got, _, _ = _both(pipe, _args(W, H, 2), interpolation_factor=2, color_match="mkl")
    assert tuple(got.shape) == (1, 3, H, W, 3) and torch.equal(got, _cast(want)) and len(pipe.last_color_match) == 3
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "upscale_latents", lambda self, lat, h, w, mode="bicubic": torch.nn.functional.interpolate(
        lat.float().flatten(0, 1), size=(h // 8, w // 8)).view(lat.shape[:3] + (h // 8, w // 8)).to(lat.dtype))
    pipe.hires_min_side = 8
    want, _, got, _, _ = _both(pipe, _args(64, 32, 2), hires_scale=2, color_match="mkl")
    assert tuple(got.shape) == (1, 2, 32, 64, 3) and torch.equal(got, _cast(want))


class NoViewVAE(fake_ops.FakeVAE):
    pass


class FourChannelVAE(fake_ops.FakeVAE):
    config = types.SimpleNamespace(out_channels=4)

    def decode_image_view(self, z):
        return self.decode(z).sample


def test_refusals_come_before_the_clip_tower(monkeypatch, vae):
    ran = []
    monkeypatch.setattr(fake_ops.FakeCLIP, "forward", lambda self, pixel_values: ran.append(1))
    args = _args(W, H, 2)
    pipe = _pipe(monkeypatch, vae)
    img = args[0]
    for kw, msg in ((dict(color_match="histogram"), "color_match must be"), (dict(color_match=True), "color_match must be"),
                    (dict(color_match="mkl", color_match_strength=1.5), "color_match_strength"), (dict(color_match="mkl", color_match_strength=-0.1), "color_match_strength"),
                    (dict(color_match="mkl", color_match_strength=float("nan")), "color_match_strength"), (dict(color_match="mkl", color_match_strength="1"), "color_match_strength"),
                    (dict(color_match="mkl", color_match_strength=True), "color_match_strength"), (dict(color_match="mkl", color_match_scope="window"), "color_match_scope"),
                    (dict(color_match="mkl", color_match_target="last_frame"), "color_match_target"), (dict(color_match="mkl", color_match_target=3), "color_match_target"),
                    (dict(color_match="mkl", color_match_target=[img, img]), "one per clip"), (dict(color_match_strength=0.5), "need color_match"),
                    (dict(color_match_scope="clip"), "need color_match"), (dict(color_match_target="first_frame"), "need color_match")):
        for out in ("tensor", "uint8"):
            with pytest.raises(ValueError, match=msg):
                pipe(*args, output_type=out, **kw)
    with pytest.raises(ValueError, match="NoViewVAE has no decode_image_view"):
        _pipe(monkeypatch, NoViewVAE())(*args, color_match="mkl")
    with pytest.raises(ValueError, match="4 channels"):
        _pipe(monkeypatch, FourChannelVAE())(*args, color_match="mean_std")
    assert ran == [] and not fake_ops.CALLS


# ---- the script
class ViewFakeVAE(fake_ops.FakeVAE):
    def decode_image_view(self, z):
        return self.decode(z).sample


def test_script_passes_the_keywords_through(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.color_match, a.color_match_strength, a.color_match_scope, a.color_match_image) == (None, 1.0, "frame", None)
    a = IV.parse_args(["--color_match", "mkl", "--color_match_strength", "0.5", "--color_match_scope", "clip", "--color_match_image", "x.png"])
    assert (a.color_match, a.color_match_strength, a.color_match_scope, a.color_match_image) == ("mkl", 0.5, "clip", "x.png")
    for bad in (["--color_match", "histogram"], ["--color_match_strength", "0.5"], ["--color_match_scope", "clip"], ["--color_match_image", "x.png"]):
        with pytest.raises(SystemExit):
            IV.parse_args(bad)
    R.install(monkeypatch)
    kwargs = []

    def build(config, infer_config, weight_dtype, device="cuda", video_decoder=False, sampler="ddim"):
        pipe = M.MikuDanceVideoPipeline(vae=ViewFakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=None,
                                        denoising_unet=types.SimpleNamespace(in_channels=4), scheduler=IV.build_scheduler(infer_config, sampler))
        pipe._device = torch.device("cpu")
        return pipe

    call = M.MikuDanceVideoPipeline.__call__
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "__call__", lambda self, *a, **k: (kwargs.append(k), call(self, *a, **k))[1])
    monkeypatch.setattr(IV, "build_pipeline", build)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", lambda self, latents, *a, **k: latents)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "_resolve_plan", lambda self, plan: plan)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "sampling_plan", lambda self, *a, **k: None)
    cfg, size = script_tree(tmp_path, frames=3, size=48)
    base = ["--config", cfg, "-W", str(size), "-H", "40", "--steps", "2", "--seed", "5"]
    IV.main(base + ["--output_dir", str(tmp_path / "plain")])
    assert not [k for k in kwargs[-1] if k.startswith("color_match")] and not [n for n, _ in fake_ops.CALLS if n.startswith("color_")]
    target = tmp_path / "target.png"
    _img(np.random.default_rng(1)).save(target)
    path = IV.main(base + ["--output_dir", str(tmp_path / "cm"), "--color_match", "mean_std", "--color_match_strength", "0.75", "--color_match_scope", "clip",
                           "--color_match_image", str(target)])
    k = kwargs[-1]
    assert (k["color_match"], k["color_match_strength"], k["color_match_scope"]) == ("mean_std", 0.75, "clip") and k["color_match_target"].size == (24, 24)
    assert [n for n, _ in fake_ops.CALLS if n.startswith("color_")] == ["color_moments", "color_apply"] and len(open(path, "rb").read()) > 1000
    IV.main(base + ["--output_dir", str(tmp_path / "ff"), "--color_match", "mkl", "--color_match_image", "first_frame", "--u8_output"])
    assert kwargs[-1]["color_match_target"] == "first_frame" and kwargs[-1]["output_type"] == "uint8" and fake_ops.CALLS[-1][1]["dst"] == "uint8"
    IV.main(base + ["--output_dir", str(tmp_path / "ref"), "--color_match", "mkl"])
    assert kwargs[-1]["color_match_target"] is None and kwargs[-1]["color_match_strength"] == 1.0 and kwargs[-1]["color_match_scope"] == "frame"
