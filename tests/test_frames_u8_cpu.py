"""CPU: uint8 frame output (output_type="uint8" / "pil") on the emulated operator layer (tests/fake_ops.py + tests/frames_ref.py).  The reference
itself over every fp16 bit pattern; __call__(output_type="uint8") against the float call's result cast the way save_videos_grid casts it, for both
VAEs, tiling, slicing and interpolation; "pil"; the operator calls of the default and of the uint8 call; the uint8 grid writer against
save_videos_grid; the script's --u8_output; the C ABI's three tables."""
import os
import re
import types

import numpy as np
import pytest
import torch

import mikudance_amd as M
from mikudance_amd import AutoencoderKL, AutoencoderKLTemporalDecoder, _lib, io_utils as U, ops
from mikudance_amd.synth import synth_state_dict

import fake_ops
import frames_ref as R
from loop_helpers import script_tree

F16 = torch.float16
CHANS = (64, 64, 64, 64)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference itself
def test_reference_over_every_fp16_bit_pattern():
    x = R.all_fp16()
    finite_or_inf = ~torch.isnan(x)
    assert int(finite_or_inf.sum()) == 63490
    chain16, chain32, single = R.u8_ref(x, False), R.u8_ref(x, True), R.one_expression(x)
    assert len(torch.unique(chain16[finite_or_inf])) == 256 and len(torch.unique(chain32[finite_or_inf])) == 256
    assert int((chain16 != single)[finite_or_inf].sum()) == 544                # the one-expression form is NOT the fp16 chain ...
    assert torch.equal(chain32[finite_or_inf], single[finite_or_inf])          # ... and is the fp32 chain on these inputs
    assert (chain16[~finite_or_inf] == 0).all() and (chain32[~finite_or_inf] == 0).all()              # NaN -> 0, the entry point's choice
    inf = torch.tensor([float("inf"), float("-inf")], dtype=F16)
    assert R.u8_ref(inf, False).tolist() == [255, 0] and R.u8_ref(inf, True).tolist() == [255, 0]
    k = torch.arange(256, dtype=torch.float32)
    assert torch.equal(torch.from_numpy((k / 255 * 255).numpy().astype(np.uint8)).long(), k.long())      # input clips need no table


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


def _args(W, H, frames):
    from PIL import Image
    rng = np.random.default_rng(4)
    img = lambda: Image.fromarray(rng.integers(0, 255, (24, 24, 3), dtype=np.uint8))
    return (img(), img(), [img() for _ in range(frames)], [img()] * frames, [img()] * frames, np.zeros((frames, 2, H // 8, W // 8), dtype=np.float32), W, H,
            frames, 2, 3.5)


def _cast(videos):
    """The float path's result as save_videos_grid casts it, in the uint8 path's layout: (b, c, f, H, W) float32 -> (b, f, H, W, c) uint8."""
    assert videos.dtype == torch.float32 and videos.dim() == 5
    return torch.from_numpy((videos * 255).numpy().astype(np.uint8)).permute(0, 2, 3, 4, 1)


def _both(pipe, args, **kw):
    del fake_ops.CALLS[:]
    want = pipe(*args, generator=torch.manual_seed(3), **kw).videos
    calls_f = list(fake_ops.CALLS)
    del fake_ops.CALLS[:]
    got = pipe(*args, generator=torch.manual_seed(3), output_type="uint8", **kw).videos
    return want, calls_f, got, list(fake_ops.CALLS)


@pytest.mark.parametrize("cls", [M.MikuDanceVideoPipeline, M.Pose2VideoPipeline], ids=["mikudance", "stage2"])
def test_uint8_call_equals_the_float_call_cast(monkeypatch, vae, cls):
    pipe = _pipe(monkeypatch, vae, cls)
    pipe.vae_batch = 2
    W, H, F_ = 32, 16, 3
    want, calls_f, got, calls_u = _both(pipe, _args(W, H, F_))
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and not got.is_cuda and tuple(got.shape) == (1, F_, H, W, 3)
    assert tuple(want.shape) == (1, 3, F_, H, W) and torch.equal(got, _cast(want))
    assert len(torch.unique(got)) > 20                                          # a picture, not a constant
    # the default call: no frames_u8, and the decode ends in one unpack_nhwc per VAE batch as before
    assert not [c for c in calls_f if c[0] == "frames_u8"]
    u8 = [d for n, d in calls_u if n == "frames_u8"]
    assert [d["B"] for d in u8] == [2, 1] and all((d["C"], d["H"], d["W"], d["src"], d["f32_math"]) == (3, H, W, "float16", False) for d in u8)
    assert all(d["strides"] == (H * W * 3, 1, W * 3, 3) for d in u8)            # the decoder's own NHWC image, as a permuted view
    # everything else is the float call's log: the uint8 call drops nothing but the decode's unpack
    assert [c for c in calls_u if c[0] != "frames_u8"] == calls_f
    pil = pipe(*_args(W, H, F_), generator=torch.manual_seed(3), output_type="pil").videos
    assert isinstance(pil, list) and len(pil) == 1 and len(pil[0]) == F_ and all(im.size == (W, H) and im.mode == "RGB" for im in pil[0])
    assert torch.equal(torch.from_numpy(np.stack([np.asarray(im) for im in pil[0]]))[None], got)
    # return_dict=False and every other value of output_type: as before
    assert torch.equal(pipe(*_args(W, H, F_), generator=torch.manual_seed(3), output_type="uint8", return_dict=False), got)
    arr = pipe(*_args(W, H, F_), generator=torch.manual_seed(3), output_type="numpy").videos
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and np.array_equal(arr, want.numpy())


def test_unpack_calls_of_the_decode(monkeypatch, vae):
    """fake_ops does not log unpack_nhwc, so the operator is wrapped: the float decode unpacks once per VAE batch, the uint8 decode never."""
    pipe = _pipe(monkeypatch, vae)
    pipe.vae_batch = 2
    seen = []
    unpack = ops.unpack_nhwc
    monkeypatch.setattr(ops, "unpack_nhwc", lambda src, dst, *a: (seen.append(tuple(dst.shape)), unpack(src, dst, *a))[1])
    lat = torch.randn(1, 4, 3, 2, 4, generator=torch.Generator().manual_seed(1)).half()
    want = pipe.decode_latents(lat)
    assert seen == [(2, 3, 16, 32), (1, 3, 16, 32)]
    del seen[:], fake_ops.CALLS[:]
    got = pipe.decode_latents(lat, output_type="uint8")
    assert seen == [] and [n for n, _ in fake_ops.CALLS].count("frames_u8") == 2
    assert torch.equal(got, _cast(torch.from_numpy(want)))
    assert isinstance(pipe.decode_latents(lat, None), np.ndarray)
    with pytest.raises(ValueError, match="output_type"):
        pipe.decode_latents(lat, output_type="pil")


def test_temporal_decoder(monkeypatch, temporal_vae):
    pipe = _pipe(monkeypatch, temporal_vae, video_decoder=True)
    pipe.decode_chunk_size = 2
    W, H, F_ = 32, 16, 3
    want, calls_f, got, calls_u = _both(pipe, _args(W, H, F_))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, F_, H, W, 3) and torch.equal(got, _cast(want))
    u8 = [d for n, d in calls_u if n == "frames_u8"]
    assert [d["B"] for d in u8] == [2, 1] and all(d["strides"] == (H * W * 8, 1, W * 8, 8) and d["C"] == 3 for d in u8)       # pixel pitch 8, 3 valid
    assert not [c for c in calls_f if c[0] == "frames_u8"] and [c for c in calls_u if c[0] != "frames_u8"] == calls_f
    lat = torch.randn(1, 4, 3, 2, 4, generator=torch.Generator().manual_seed(1)).half()
    assert torch.equal(pipe.decode_temporal(lat, 3, output_type="uint8"), _cast(torch.from_numpy(pipe.decode_temporal(lat, 3))))


def test_tiling_and_slicing(monkeypatch, vae):
    v = _load(AutoencoderKL(block_out_channels=CHANS, sample_size=128))
    pipe = _pipe(monkeypatch, v)
    pipe.vae_batch = 2
    W, H, F_ = 128, 64, 2
    want, calls_f, got, calls_u = _both(pipe, _args(W, H, F_), vae_tiling=True, vae_tile_size=64)
    assert sum(n == "tile_blend" for n, _ in calls_f) > 0 and torch.equal(got, _cast(want))
    u8 = [d for n, d in calls_u if n == "frames_u8"]
    assert len(u8) == 1 and u8[0]["strides"] == (3 * H * W, H * W, W, 1)       # decode as it stands, ONE frames_u8 from its NCHW result
    assert [c for c in calls_u if c[0] != "frames_u8"] == calls_f               # the tile loop is not touched
    plain = pipe(*_args(W, H, F_), generator=torch.manual_seed(3), output_type="uint8").videos
    assert not torch.equal(plain, got) and (v.use_tiling, v.tile_sample_min_size) == (False, 128)
    v.enable_slicing()
    z = torch.randn(3, 4, 2, 4, generator=torch.Generator().manual_seed(2)).half()
    del fake_ops.CALLS[:]
    sliced = v.decode_u8(z)
    assert [d["B"] for n, d in fake_ops.CALLS if n == "frames_u8"] == [3]
    assert torch.equal(sliced, R.u8_ref(v.decode(z).sample, False).permute(0, 2, 3, 1))
    out = torch.zeros(3, 16, 32, 3, dtype=torch.uint8)
    assert v.decode_u8(z, out=out) is out and torch.equal(out, sliced)
    v.disable_slicing()
    got32 = v.decode_u8(z.float())                                             # an fp32 boundary: the fp32 chain, as decode's dtype says
    assert fake_ops.CALLS[-1][1]["f32_math"] is True and torch.equal(got32, R.u8_ref(v.decode(z.float()).sample, True).permute(0, 2, 3, 1))
    with pytest.raises(ValueError, match="expects"):
        v.decode_u8(torch.zeros(1, 3, 4, 4, dtype=F16))


def test_interpolation_factor(monkeypatch, vae):
    pipe = _pipe(monkeypatch, vae)
    from mikudance_amd import pipeline_mikudance as PM
    monkeypatch.setattr(PM, "tensor_interpolation", PM.linear)                 # what set_tensor_interpolation_method(False) sets, undone after the test
    W, H, F_ = 32, 16, 2
    want, _, got, _ = _both(pipe, _args(W, H, F_), interpolation_factor=2)
    assert tuple(got.shape) == (1, 3, H, W, 3) and torch.equal(got, _cast(want))


def test_a_vae_without_decode_u8_is_refused(monkeypatch):
    pipe = _pipe(monkeypatch, fake_ops.FakeVAE())
    with pytest.raises(ValueError, match="FakeVAE has no decode_u8"):
        pipe(*_args(32, 16, 2), output_type="uint8")


# ---- the writers
def _clip(b, f, h, w, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (b, f, h, w, 3), dtype=np.uint8))


@pytest.mark.parametrize("ext", [".mp4", ".gif"])
@pytest.mark.parametrize("b,n_rows", [(3, 3), (3, 2), (1, 6)])
def test_save_frames_grid_u8_writes_save_videos_grids_file(tmp_path, ext, b, n_rows):
    clips = _clip(b, 3, 20, 12)
    floats = (clips.float() / 255).permute(0, 4, 1, 2, 3).contiguous()                    # what frames_to_tensor / the float path hold
    U.save_videos_grid(floats, str(tmp_path / ("a" + ext)), n_rows=n_rows, fps=12)
    U.save_frames_grid_u8(clips, str(tmp_path / ("b" + ext)), n_rows=n_rows, fps=12)
    a, bb = open(tmp_path / ("a" + ext), "rb").read(), open(tmp_path / ("b" + ext), "rb").read()
    assert len(a) > 500 and a == bb
    for t in range(3):                                                                    # and pixel for pixel before any encoder
        want = (U.make_grid(floats[:, :, t], nrow=n_rows).permute(1, 2, 0) * 255).numpy().astype(np.uint8)
        assert np.array_equal(U.make_grid_u8(clips[:, t], nrow=n_rows).numpy(), want)
    with pytest.raises(ValueError, match="uint8"):
        U.save_frames_grid_u8(floats, str(tmp_path / ("c" + ext)))


def test_frames_to_u8_is_frames_to_tensor_in_bytes():
    from PIL import Image
    rng = np.random.default_rng(2)
    pils = [Image.fromarray(rng.integers(0, 256, (30, 22, 3), dtype=np.uint8)) for _ in range(3)] + [Image.new("L", (8, 8), 77)]
    got, want = U.frames_to_u8(pils, 16, 24), U.frames_to_tensor(pils, 16, 24)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 4, 16, 24, 3)
    assert torch.equal(got, _cast(want))


class U8FakeVAE(fake_ops.FakeVAE):
    """The duck-typed VAE with the uint8 interface: decode, then the operator."""

    def decode_u8(self, z, out=None):
        return ops.frames_u8(self.decode(z).sample, out)


def test_script_u8_output_writes_the_same_file(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    assert IV.parse_args([]).u8_output is False and IV.parse_args(["--u8_output"]).u8_output is True
    R.install(monkeypatch)
    pipes, kwargs = [], []

    def build(config, infer_config, weight_dtype, device="cuda", video_decoder=False, sampler="ddim"):
        pipe = M.MikuDanceVideoPipeline(vae=U8FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=None,
                                        denoising_unet=types.SimpleNamespace(in_channels=4), scheduler=IV.build_scheduler(infer_config, sampler))
        pipe._device = torch.device("cpu")
        pipes.append(pipe)
        return pipe

    call = M.MikuDanceVideoPipeline.__call__
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "__call__", lambda self, *a, **k: (kwargs.append(k), call(self, *a, **k))[1])
    monkeypatch.setattr(IV, "build_pipeline", build)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", lambda self, latents, *a, **k: latents)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "_resolve_plan", lambda self, plan: plan)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "sampling_plan", lambda self, *a, **k: None)
    cfg, size = script_tree(tmp_path, frames=3, size=48)
    base = ["--config", cfg, "-W", str(size), "-H", "40", "--steps", "2", "--seed", "5"]
    plain = IV.main(base + ["--output_dir", str(tmp_path / "plain")])
    assert "frames_u8" not in [n for n, _ in fake_ops.CALLS] and "output_type" not in kwargs[-1]
    u8 = IV.main(base + ["--output_dir", str(tmp_path / "u8"), "--u8_output"])
    assert "frames_u8" in [n for n, _ in fake_ops.CALLS] and kwargs[-1]["output_type"] == "uint8"
    a, b = open(plain, "rb").read(), open(u8, "rb").read()
    assert plain != u8 and len(a) > 1000 and a == b
    frames = U.read_frames(u8)
    assert len(frames) == 3 and frames[0].size == (3 * size + 4 * 2, 40 + 2 * 2)          # ref | pose | video on make_grid's canvas


# ---- the C ABI
def test_header_exports_and_signature_table_agree():
    import ctypes
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdance_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(md_[a-z0-9_]+)\s*\(", text)))
    assert "md_frames_u8" in declared and set(_lib.SIGNATURES) == set(declared)
    assert len([s for s in declared if s not in ("md_version", "md_last_error")]) == 62      # the README's count: entry points beside those two
    proto = re.search(r"int md_frames_u8\(([^)]*)\)", text).group(1)
    kinds = [("P" if "*" in a else a.split()[0]) for a in proto.split(",")]
    table = {"P": ctypes.c_void_p, "int": ctypes.c_int, "long": ctypes.c_long}
    res, args = _lib.SIGNATURES["md_frames_u8"]
    assert res is ctypes.c_int and args == [table[k] for k in kinds] and len(args) == 15
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "md_frames_u8")
    assert "frames_u8.hip" in open(os.path.join(ROOT, "mikudance_amd", "csrc", "Makefile")).read()
