"""CPU: tiled / sliced AutoencoderKL on the emulated operator layer (tests/fake_ops.py + the tile_blend emulation of tests/vae_tiling_ref.py).
The default path makes the operator calls of the parent commit and returns equal tensors; diffusers' four methods and tile attributes exist;
the tile grid, crops and extents are those of the float64 restatement; tiled_encode / tiled_decode equal the restatement run on the same per-tile
outputs; every bad geometry is refused before an operator runs; the pipeline keywords and the script flags reach the VAE."""
import types

import numpy as np
import pytest
import torch

import mikudance_amd as M
from mikudance_amd import AutoencoderKL, ops
from mikudance_amd.blocks import tokens
from mikudance_amd.synth import synth_state_dict

import fake_ops
import vae_tiling_ref as R
from loop_helpers import script_tree

F16 = torch.float16
CHANS = (64, 64, 64, 64)


def _vae(sample_size=128, seed=77):
    vae = AutoencoderKL(block_out_channels=CHANS, sample_size=sample_size)
    vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=seed), strict=True)
    return vae.half().eval()


@pytest.fixture(scope="module")
def vae():
    return _vae()


def _rand(*shape, seed):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(F16)


# ---- the parent commit's encode / decode, operator call by operator call
def parent_encode(vae, x):
    pk = vae.packed()
    B, C, H, W = x.shape
    st = x.stride()
    x64 = ops.pack_nhwc(x, B, 1, (st[0], 0, st[1], st[2], st[3]), 0, C, 64, H, W)
    h = vae.encoder(x64)
    m64 = torch.zeros_like(h)
    ops.gemm(tokens(h), pk["q"], bias=pk["qb"], out=tokens(m64)[:, :2 * vae.zc])
    moments = torch.empty((B, 2 * vae.zc, H // 8, W // 8), dtype=x.dtype)
    so = moments.stride()
    ops.unpack_nhwc(m64, moments, B, 1, (so[0], 0, so[1], so[2], so[3]), 2 * vae.zc, H // 8, W // 8)
    return moments


def parent_decode(vae, z):
    pk = vae.packed()
    B, C, h, w = z.shape
    st = z.stride()
    z64 = ops.pack_nhwc(z, B, 1, (st[0], 0, st[1], st[2], st[3]), 0, C, 64, h, w)
    p64 = torch.zeros_like(z64)
    ops.gemm(tokens(z64), pk["pq"], bias=pk["pqb"], out=tokens(p64)[:, :vae.zc])
    y = vae.decoder(p64)
    img = torch.empty((B, y.shape[-1], 8 * h, 8 * w), dtype=z.dtype)
    so = img.stride()
    ops.unpack_nhwc(y, img, B, 1, (so[0], 0, so[1], so[2], so[3]), y.shape[-1], 8 * h, 8 * w)
    return img


def _logged(fn):
    del fake_ops.CALLS[:]
    out = fn()
    return out, list(fake_ops.CALLS)


def test_methods_and_attributes_exist_and_disable_restores(vae):
    big = AutoencoderKL()
    assert (big.use_tiling, big.use_slicing, big.tile_sample_min_size, big.tile_latent_min_size, big.tile_overlap_factor) == (False, False, 512, 64, 0.25)
    assert (vae.tile_sample_min_size, vae.tile_latent_min_size) == (128, 16)
    v = _vae()
    v.enable_tiling(); v.enable_slicing()
    assert v.use_tiling is True and v.use_slicing is True
    v.enable_tiling(False)
    assert v.use_tiling is False
    v.enable_tiling(); v.disable_tiling(); v.disable_slicing()
    assert v.use_tiling is False and v.use_slicing is False
    assert callable(v.tiled_encode) and callable(v.tiled_decode)
    v.set_tile_size(256)
    assert (v.tile_sample_min_size, v.tile_latent_min_size) == (256, 32)
    for bad in (0, -32, 100, 48, 64.0, True, None, "256"):
        with pytest.raises(ValueError, match="multiple of 32"):
            v.set_tile_size(bad)


def test_default_path_is_the_parent_commits(monkeypatch, vae):
    R.install(monkeypatch)
    x, z = _rand(2, 3, 32, 48, seed=1), _rand(2, 4, 4, 6, seed=2)
    want_m, calls_m = _logged(lambda: parent_encode(vae, x))
    want_x, calls_x = _logged(lambda: parent_decode(vae, z))
    assert len(calls_m) > 20 and len(calls_x) > 20 and not any(n == "tile_blend" for n, _ in calls_m + calls_x)
    post, calls = _logged(lambda: vae.encode(x).latent_dist)
    assert calls == calls_m and torch.equal(torch.cat([post.mean, post.logvar], 1), torch.cat([want_m[:, :4], want_m[:, 4:].clamp(-30, 20)], 1))
    got, calls = _logged(lambda: vae.decode(z).sample)
    assert calls == calls_x and torch.equal(got, want_x)
    # tiling on, but nothing larger than one tile (here exactly one tile): the same calls again; and after disable_* too
    v = _vae()
    x1, z1 = _rand(1, 3, 128, 128, seed=3)[:, :, :, :64], _rand(1, 4, 16, 8, seed=4)
    want_m, calls_m = _logged(lambda: parent_encode(v, x1))
    want_x, calls_x = _logged(lambda: parent_decode(v, z1))
    v.enable_tiling()
    got, calls = _logged(lambda: v.encode(x1).latent_dist.mean)
    assert calls == calls_m and torch.equal(got, want_m[:, :4])
    got, calls = _logged(lambda: v.decode(z1).sample)
    assert calls == calls_x and torch.equal(got, want_x)
    v.enable_slicing()                                                       # B = 1: nothing to slice
    got, calls = _logged(lambda: v.decode(z1).sample)
    assert calls == calls_x and torch.equal(got, want_x)
    v.disable_tiling(); v.disable_slicing()
    z2 = _rand(2, 4, 20, 4, seed=5)                                         # above one tile: untiled again after disable_tiling
    want, calls_p = _logged(lambda: parent_decode(v, z2))
    got, calls = _logged(lambda: v.decode(z2).sample)
    assert calls == calls_p and torch.equal(got, want)


# (rows, cols, encode) -> the literal grid: (start, size, out_start, keep) per axis, tiles of 128 pixels / 16 latents, a quarter overlapped
GRIDS = {
    (28, 40, False): ([(0, 16, 0, 96), (12, 16, 96, 96), (24, 4, 192, 32)], [(0, 16, 0, 96), (12, 16, 96, 96), (24, 16, 192, 96), (36, 4, 288, 32)], 32),
    (26, 32, False): ([(0, 16, 0, 96), (12, 14, 96, 96), (24, 2, 192, 16)], [(0, 16, 0, 96), (12, 16, 96, 96), (24, 8, 192, 64)], 32),
    (224, 320, True): ([(0, 128, 0, 12), (96, 128, 12, 12), (192, 32, 24, 4)], [(0, 128, 0, 12), (96, 128, 12, 12), (192, 128, 24, 12), (288, 32, 36, 4)], 4),
    (40, 8, False): ([(0, 16, 0, 96), (12, 16, 96, 96), (24, 16, 192, 96), (36, 4, 288, 32)], [(0, 8, 0, 64)], 32),           # a one-tile-wide strip
    (64, 320, True): ([(0, 64, 0, 8)], [(0, 128, 0, 12), (96, 128, 12, 12), (192, 128, 24, 12), (288, 32, 36, 4)], 4),       # and a one-tile-high one
}


@pytest.mark.parametrize("case", list(GRIDS), ids=lambda c: f"{c[0]}x{c[1]}-{'encode' if c[2] else 'decode'}")
def test_tile_grid_matches_the_restatement(vae, case):
    n_rows, n_cols, encode = case
    rows, cols, extent = vae.tile_grid(n_rows, n_cols, encode)
    assert (rows, cols, extent) == GRIDS[case]
    assert rows == R.axis_ref(n_rows, 128, 16, 0.25, 8, encode) and cols == R.axis_ref(n_cols, 128, 16, 0.25, 8, encode)
    assert extent == R.sizes_ref(128, 16, 0.25, encode)[2]
    f_out = (lambda n: n // 8) if encode else (lambda n: n * 8)
    assert rows[-1][2] + rows[-1][3] == f_out(n_rows) and cols[-1][2] + cols[-1][3] == f_out(n_cols)       # the kept parts fill the output


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("shape", [(28, 40), (26, 32), (40, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiled_decode_equals_the_restatement(monkeypatch, vae, shape):
    R.install(monkeypatch)
    z = _rand(1, 4, *shape, seed=sum(shape))
    want = R.tiled_ref(z, lambda t: _nhwc(vae.decode(t).sample), 128, 16, 0.25, 8, encode=False)
    got, calls = _logged(lambda: vae.tiled_decode(z).sample)
    rows, cols, _ = vae.tile_grid(*shape, encode=False)
    blends = [d for n, d in calls if n == "tile_blend"]
    assert len(blends) == len(rows) * len(cols) and all(d["extent"] == (32, 32) and d["c"] == 3 and d["ldc"] == 3 for d in blends)
    assert [d["keep"] for d in blends] == [(r[3], c[3]) for r in rows for c in cols]
    assert [(d["Ah"], d["Lw"]) for d in blends] == [(8 * rows[i - 1][1] if i else None, 8 * cols[j - 1][1] if j else None)
                                                    for i in range(len(rows)) for j in range(len(cols))]
    assert got.dtype == F16 and tuple(got.shape) == (1, 3, 8 * shape[0], 8 * shape[1])
    assert torch.equal(got, want.to(F16))
    v = _vae()
    v.enable_tiling()                                                          # decode() takes the same road, and says so by its calls
    got2, calls2 = _logged(lambda: v.decode(z).sample)
    assert torch.equal(got2, got) and calls2 == calls
    assert not torch.equal(got, parent_decode(vae, z))                         # tiling is a different result by design


def test_tiled_encode_equals_the_restatement(monkeypatch, vae):
    R.install(monkeypatch)
    x = _rand(1, 3, 224, 320, seed=9)
    want = R.tiled_ref(x, lambda t: _nhwc(parent_encode(vae, t)), 128, 16, 0.25, 8, encode=True)
    post, calls = _logged(lambda: vae.tiled_encode(x).latent_dist)
    blends = [d for n, d in calls if n == "tile_blend"]
    assert len(blends) == 12 and all(d["extent"] == (4, 4) and d["c"] == 8 and d["ldc"] == 64 for d in blends)     # the blend runs on the 2z moments
    want16 = want.to(F16)
    assert torch.equal(post.mean, want16[:, :4]) and torch.equal(post.logvar, want16[:, 4:].clamp(-30, 20))
    v = _vae()
    v.enable_tiling()
    assert torch.equal(v.encode(x).latent_dist.mean, post.mean)
    out32 = vae.tiled_encode(x.float()).latent_dist.mean                       # an fp32 caller gets the unrounded blend
    assert out32.dtype == torch.float32 and R.within_one_ulp(out32, want[:, :4])[0] and torch.equal(out32.to(F16), post.mean)


def test_slicing_is_one_image_per_call(monkeypatch, vae):
    R.install(monkeypatch)
    z, x = _rand(3, 4, 4, 6, seed=2), _rand(3, 3, 32, 48, seed=1)
    want_x, calls_x = _logged(lambda: vae.decode(z).sample)
    want_m = vae.encode(x).latent_dist.mean
    v = _vae()
    v.enable_slicing()
    got, calls = _logged(lambda: v.decode(z).sample)
    # per-image arithmetic: bitwise the images decoded one by one (the emulation's batched fp32 convolutions sum in another order)
    assert torch.equal(got, torch.cat([vae.decode(z[b:b + 1]).sample for b in range(3)])) and (got.float() - want_x.float()).norm() < 2e-3 * want_x.float().norm()
    convs = lambda log: [d for n, d in log if n == "conv"]
    assert len(convs(calls)) == 3 * len(convs(calls_x)) and all(d[0][0] == 1 for d in convs(calls)) and all(d[0][0] == 3 for d in convs(calls_x))
    assert torch.equal(v.encode(x).latent_dist.mean, torch.cat([vae.encode(x[b:b + 1]).latent_dist.mean for b in range(3)]))
    assert (v.encode(x).latent_dist.mean.float() - want_m.float()).norm() < 2e-3 * want_m.float().norm()
    v.enable_tiling()                                                          # both: every image tile by tile
    zt = _rand(2, 4, 20, 8, seed=3)
    got, calls = _logged(lambda: v.decode(zt).sample)
    assert sum(n == "tile_blend" for n, _ in calls) == 2 * 2 and all(d["B"] == 1 for n, d in calls if n == "tile_blend")
    assert torch.equal(got, torch.cat([v.tiled_decode(zt[b:b + 1]).sample for b in range(2)]))


def test_bad_geometry_is_refused_before_any_operator(monkeypatch, vae):
    R.install(monkeypatch)
    v = _vae()
    v.enable_tiling()
    z = lambda h, w: torch.zeros(1, 4, h, w, dtype=F16)
    x = lambda h, w: torch.zeros(1, 3, h, w, dtype=F16)
    del fake_ops.CALLS[:]
    # 25 x 40: rows of 16, 13, 1 and columns of 16, 16, 16, 4 -- 13 x 16 is fine (208 tokens), 13 x 4 is not; 17 x 17: a 5 x 5 corner
    for call, match in ((lambda: v.decode(z(25, 40)), r"tile \(row 1, column 3\).*13 x 4 latents.*multiple of 8 tokens.*rows work"),
                        (lambda: v.tiled_decode(z(17, 17)), r"tile \(row 1, column 1\).*5 x 5 latents"),
                        (lambda: v.tiled_decode(z(3, 5)), r"tile \(row 0, column 0\).*3 x 5"),
                        (lambda: v.encode(x(200, 320)), r"tile \(row 1, column 3\).*104 x 32 pixels.*13 x 4"),
                        (lambda: v.tiled_encode(x(136, 136)), r"tile \(row 1, column 1\).*40 x 40 pixels"),
                        (lambda: v.tiled_encode(x(100, 128)), "multiples of 8"),
                        (lambda: v.tiled_decode(torch.zeros(1, 3, 16, 16, dtype=F16)), "expects")):
        with pytest.raises(ValueError, match=match):
            call()
    with pytest.raises(ValueError) as e:
        v.decode(z(25, 40))
    assert "[24, 26]" in str(e.value) or "[24, 28]" in str(e.value), str(e.value)      # the sizes that would work are named
    v.tile_latent_min_size = 20                                                        # 128 pixels against 20 latents: the two disagree
    with pytest.raises(ValueError, match="do not agree"):
        v.decode(z(28, 40))
    v.tile_latent_min_size, v.tile_overlap_factor = 16, 1.0
    with pytest.raises(ValueError, match="tile_overlap_factor"):
        v.decode(z(28, 40))
    assert fake_ops.CALLS == []


def test_the_named_sizes_work(vae):
    v = _vae()
    with pytest.raises(ValueError) as e:
        v.tile_grid(25, 40, encode=False)
    import re
    rows = [int(n) for n in re.search(r"With 40 columns, \[([0-9, ]+)\] rows work", str(e.value)).group(1).split(",")]
    assert len(rows) == 2 and rows[0] < 25 < rows[1]
    for r in rows:
        v.tile_grid(r, 40, encode=False)


# ---- pipeline and script
class TilingSpyVAE(fake_ops.FakeVAE):
    """The duck-typed VAE with AutoencoderKL's tiling interface: records the state every encode / decode runs under."""

    def __init__(self):
        super().__init__()
        self.use_tiling, self.use_slicing, self.tile_sample_min_size, self.tile_latent_min_size = False, False, 512, 64
        self.seen, self.grids = [], []

    enable_tiling, disable_tiling = AutoencoderKL.enable_tiling, AutoencoderKL.disable_tiling
    enable_slicing, disable_slicing = AutoencoderKL.enable_slicing, AutoencoderKL.disable_slicing
    set_tile_size = AutoencoderKL.set_tile_size
    config = types.SimpleNamespace(block_out_channels=(128, 256, 512, 512))

    def tile_grid(self, h, w, encode):
        self.grids.append((h, w, encode, self.tile_sample_min_size))
        if (h, w) in ((200, 64), (25, 8)):
            raise ValueError("tile (row 1, column 0)")

    def encode(self, x):
        self.seen.append(("encode", self.use_tiling, self.tile_sample_min_size, self.tile_latent_min_size))
        return super().encode(x)

    def decode(self, z, **kw):
        self.seen.append(("decode", self.use_tiling, self.tile_sample_min_size, self.tile_latent_min_size))
        return super().decode(z, **kw)


def _spy_pipe(cls=M.MikuDanceVideoPipeline, vae=None):
    pipe = cls(vae=vae or TilingSpyVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=None, denoising_unet=types.SimpleNamespace(in_channels=4),
               scheduler=M.DDIMScheduler(**M.selftest.SCHED_KWARGS))
    pipe._device = torch.device("cpu")
    pipe.clips = 0
    clip = pipe.clip_embeds

    def clip_embeds(*a, **k):
        pipe.clips += 1
        return clip(*a, **k)
    pipe.clip_embeds = clip_embeds
    return pipe


def _call_args(W, H, frames=2):
    from PIL import Image
    img = Image.new("RGB", (24, 24), (40, 80, 120))
    return (img, img, [img] * frames, [img] * frames, [img] * frames, np.zeros((frames, 2, H // 8, W // 8), dtype=np.float32), W, H, frames, 2, 3.5)


@pytest.mark.parametrize("cls", [M.MikuDanceVideoPipeline, M.Pose2VideoPipeline], ids=["mikudance", "stage2"])
def test_pipeline_keywords_reach_the_vae(monkeypatch, cls):
    R.install(monkeypatch)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", lambda self, latents, *a, **k: latents)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "_resolve_plan", lambda self, plan: plan)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "sampling_plan", lambda self, *a, **k: None)
    pipe = _spy_pipe(cls)
    vae = pipe.vae
    pipe.enable_vae_tiling(); pipe.enable_vae_slicing()
    assert vae.use_tiling and vae.use_slicing
    pipe.disable_vae_tiling(); pipe.disable_vae_slicing()
    assert not vae.use_tiling and not vae.use_slicing
    pipe(*_call_args(64, 64))                                                  # the default: the VAE is not touched
    assert vae.seen and all(s[1:] == (False, 512, 64) for s in vae.seen) and vae.grids == []
    del vae.seen[:]
    pipe(*_call_args(64, 96), vae_tiling=True, vae_tile_size=32)
    assert vae.seen and {s[0] for s in vae.seen} == {"encode", "decode"} and all(s[1:] == (True, 32, 4) for s in vae.seen)
    assert vae.grids == [(96, 64, True, 32), (12, 8, False, 32)]               # both directions checked, at the call's size
    assert (vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size) == (False, 512, 64)        # and the VAE's own state is back
    del vae.seen[:], vae.grids[:]
    pipe.enable_vae_tiling()                                                   # diffusers' way: the state stays, the call needs no keyword
    pipe(*_call_args(64, 64))
    assert all(s[1:] == (True, 512, 64) for s in vae.seen) and vae.use_tiling
    pipe(*_call_args(64, 64), vae_tile_size=64)                                # a tile size alone is fine while tiling is on
    assert vae.seen[-1][1:] == (True, 64, 8) and vae.tile_sample_min_size == 512
    pipe.disable_vae_tiling()
    # refusals: before the CLIP tower or the VAE runs
    del vae.seen[:]
    pipe.clips = 0
    for kw, match in ((dict(vae_tiling=1), "True or False"), (dict(vae_tiling="yes"), "True or False"), (dict(vae_tile_size=256), "needs vae_tiling=True"),
                      (dict(vae_tiling=True, vae_tile_size=100), "multiple of 32"), (dict(vae_tiling=True, vae_tile_size=0), "multiple of 32"),
                      (dict(vae_tiling=True, vae_tile_size=64.0), "multiple of 32")):
        with pytest.raises(ValueError, match=match):
            pipe(*_call_args(64, 64), **kw)
    with pytest.raises(ValueError, match=r"tile \(row 1, column 0\)"):
        pipe(*_call_args(64, 200), vae_tiling=True, vae_tile_size=32)
    pipe.enable_vae_tiling()                                                   # diffusers' path, no keyword: the grid is checked as early
    vae.set_tile_size(32)
    with pytest.raises(ValueError, match=r"tile \(row 1, column 0\)"):
        pipe(*_call_args(64, 200))
    assert (vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size) == (True, 32, 4)
    pipe.disable_vae_tiling()
    vae.set_tile_size(512)
    plain = _spy_pipe(cls, vae=fake_ops.FakeVAE())
    with pytest.raises(ValueError, match="FakeVAE has no tiling"):
        plain(*_call_args(64, 64), vae_tiling=True)
    assert pipe.clips == 0 and plain.clips == 0 and vae.seen == []
    assert (vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size) == (False, 512, 64)


def test_script_flags_reach_the_vae(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert a.vae_tiling is False and a.vae_tile_size is None
    a = IV.parse_args(["--vae_tiling", "--vae_tile_size", "256"])
    assert a.vae_tiling is True and a.vae_tile_size == 256
    for argv in (["--vae_tile_size", "256"], ["--vae_tiling", "--video_decoder"], ["--vae_tiling", "--vae_tile_size", "big"]):
        with pytest.raises(SystemExit):
            IV.parse_args(argv)
    R.install(monkeypatch)
    pipes = []

    def build(config, infer_config, weight_dtype, device="cuda", video_decoder=False, sampler="ddim"):
        pipes.append(_spy_pipe())
        return pipes[-1]

    monkeypatch.setattr(IV, "build_pipeline", build)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", lambda self, latents, *a, **k: latents)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "_resolve_plan", lambda self, plan: plan)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "sampling_plan", lambda self, *a, **k: None)
    cfg, size = script_tree(tmp_path, frames=2, size=64)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base + ["--vae_tiling", "--vae_tile_size", "32"])
    IV.main(base)
    tiled, plain = (p.vae.seen for p in pipes)
    assert tiled and all(s[1:] == (True, 32, 4) for s in tiled)
    assert plain and all(s[1:] == (False, 512, 64) for s in plain)
