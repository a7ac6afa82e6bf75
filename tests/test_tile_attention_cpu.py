"""CPU: shifted-tile spatial self-attention (tile_attention=, MSW-MSA of HiDiffusion, arXiv 2311.17528) -- the operator's emulation against the
torch definition, every refusal through both entry points, the host graph of MikuDanceVideoPipeline.denoise() on emulated operators against
the restated loop of tests/tile_ref.py (values, and which block calls token_tile / attention with what), the default path, that the feature
acts, three gloo ranks, and the script's flags."""
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd import blocks
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import fake_ops
import tile_ref as TR
from loop_helpers import (CountingUNet, cosine, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401
                          worker_setup, zero_inputs)

BOUND = dict(rel=3e-2, cos=0.999)                                          # the project's loop bound
OPEN2 = dict(context_frames=8, context_stride=1, context_overlap=2)       # uniform_open on 12 frames: two windows
# the operator's shapes of tests/test_tile_attention_gpu.py: (B, Hh, Ww, C, t, tile_stride or None, shifts)
KERNEL_SHAPES = [(2, 8, 8, 64, 2, None, [(0, 0), (1, 3), (7, 7)]), (3, 6, 10, 320, 2, None, [(0, 0), (2, 7)]), (3, 6, 10, 320, 2, 16, [(0, 0), (5, 9)]),
                 (1, 8, 8, 8, 4, 8, [(0, 0), (3, 1)]), (2, 4, 4, 1280, 2, None, [(0, 0), (1, 1)]), (1, 16, 16, 64, 8, None, [(0, 0), (9, 4)])]


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


# ---- 1. the definition and the emulation
def test_definition_on_a_grid_computed_by_hand():
    """4 x 4, t = 2, token (y, x) holds 10 y + x: the tiles of the unshifted and of the (1, 3)-shifted grid."""
    x = torch.tensor([[10.0 * y + c for c in range(4)] for y in range(4)]).reshape(1, 16, 1)
    assert TR.tile(x, 1, 4, 4, 2)[:, :, 0].tolist() == [[0, 1, 10, 11], [2, 3, 12, 13], [20, 21, 30, 31], [22, 23, 32, 33]]
    assert TR.tile(x, 1, 4, 4, 2, (1, 3))[:, :, 0].tolist() == [[13, 10, 23, 20], [11, 12, 21, 22], [33, 30, 3, 0], [31, 32, 1, 2]]
    assert torch.equal(TR.untile(TR.tile(x, 1, 4, 4, 2, (1, 3)), 1, 4, 4, 2, (1, 3)), x)
    assert [TR.shift_at("cycle", k, 8, 6) for k in range(5)] == [(0, 0), (2, 1), (4, 3), (6, 4), (0, 0)] and TR.shift_at("none", 3, 8, 6) == (0, 0)


@pytest.mark.parametrize("B,Hh,Ww,C,t,stride,shifts", KERNEL_SHAPES)
def test_emulated_operator_is_the_definition(B, Hh, Ww, C, t, stride, shifts):
    g = torch.Generator().manual_seed(B * 100 + Hh + t)
    x = torch.randn((B * Hh * Ww, C), generator=g).half()
    Lt = (Hh // t) * (Ww // t)
    for shift in shifts:
        y, lt, st = TR.token_tile(x, B, Hh, Ww, t, shift, tile_stride=stride)
        assert lt == Lt and st == (stride or Lt) and y.shape == (B * t * t * st, C)
        yv = y.view(B * t * t, st, C)
        assert torch.equal(yv[:, :Lt], TR.tile(x, B, Hh, Ww, t, shift))
        assert (yv[:, Lt:] == 0).all() and not torch.signbit(yv[:, Lt:]).any()
        yv[:, Lt:] = float("nan")                                          # the inverse does not read the pad rows
        assert torch.equal(TR.token_untile(y, B, Hh, Ww, t, shift, tile_stride=stride), x)
        assert torch.equal(TR.untile(TR.tile(x, B, Hh, Ww, t, shift), B, Hh, Ww, t, shift).reshape(-1, C), x)


# ---- 2. refusals
def test_check_functions_refuse_what_they_document():
    from mikudance_amd.unet_3d_mix import check_tile_attention, check_tile_attention_grid, tile_shift_at
    assert check_tile_attention(2, "cycle") == ((2,), "cycle") and check_tile_attention((1, 4), "none") == ((1, 4), "none")
    assert check_tile_attention((), "cycle") == ((), "cycle")
    for bad, msg in ((0, "1..8"), (9, "1..8"), ((2, -1), "1..8"), (2.0, "integer or a sequence"), ((2, 1.5), "1..8"), ("2", "1..8"), (None, "integer or a sequence"),
                     ((True,), "1..8"), (True, "integer or a sequence")):
        with pytest.raises(ValueError, match=msg):
            check_tile_attention(bad, "cycle")
    for bad in ("random", None, 0):
        with pytest.raises(ValueError, match="tile_attention_shift must be one of"):
            check_tile_attention(2, bad)
    # levels halve with ceil: 5 x 7 -> 3 x 4 -> 2 x 2 -> 1 x 1
    with pytest.raises(ValueError, match="factor 2 on level 0, whose token grid is 5 x 7"):
        check_tile_attention_grid((2,), 5, 7, ())
    with pytest.raises(ValueError, match="factor 2 on level 1, whose token grid is 3 x 4"):
        check_tile_attention_grid((1, 2), 5, 7, ())
    check_tile_attention_grid((1, 1, 2), 5, 7, ())
    # 16 x 16: 16, 8, 4, 2
    check_tile_attention_grid((2, 2, 2, 2), 16, 16, ())
    with pytest.raises(ValueError, match="factor 4 on level 3, whose token grid is 2 x 2"):
        check_tile_attention_grid((2, 2, 2, 4), 16, 16, ())
    # tile then pool: a 4 x 4 tile has no 8 x 8 block
    with pytest.raises(ValueError, match="factor 4 on level 0 leaves tiles of 4 x 4 tokens, smaller than that level's kv_downsample factor 8"):
        check_tile_attention_grid((4,), 16, 16, (8,))
    check_tile_attention_grid((4,), 16, 16, (4,))
    check_tile_attention_grid((4,), 16, 16, (1, 8))
    assert [tile_shift_at("cycle", k) for k in (0, 1, 5, 7)] == [0, 1, 1, 3] and tile_shift_at("none", 3) == 0


def test_plan_covers_the_documented_blocks(monkeypatch, small_cpu):
    _, den, _, _ = small_cpu
    of = {a: p for p, b in den.attention_block_prefixes() for a in [_module(den, p)]}
    names = lambda plan: sorted(of[a] for a in plan)
    lvl0 = ["down_blocks.0.attentions.0", "down_blocks.0.attentions.1"] + [f"up_blocks.3.attentions.{j}" for j in range(3)]
    lvl1 = ["down_blocks.1.attentions.0", "down_blocks.1.attentions.1"] + [f"up_blocks.2.attentions.{j}" for j in range(3)]
    assert den.tile_attention_plan(1) is None and den.tile_attention_plan((1, 1, 1, 1)) is None and den.tile_attention_plan(()) is None
    plan = den.tile_attention_plan(2)
    assert names(plan) == sorted(lvl0) and set(plan.values()) == {2}
    plan = den.tile_attention_plan((4, 2))
    assert names(plan) == sorted(lvl0 + lvl1) and {of[a]: v for a, v in plan.items()}["up_blocks.2.attentions.1"] == 2
    assert names(den.tile_attention_plan((1, 1, 1, 2))) == ["mid_block.attentions.0"]
    with pytest.raises(ValueError, match="5 factors for a UNet of 4"):
        den.tile_attention_plan((2, 2, 2, 2, 2))
    with pytest.raises(ValueError, match="1..8"):
        den.tile_attention_plan((9,))
    # the pairs forward_nhwc forms for a 16 x 16 latent at shift index 3: level 0 tiles of 8 x 8, level 1 tiles of 2 x 2
    pairs = den._tile_pairs(den.tile_attention_plan((2, 4)), 16, 16, 3)
    assert {v for v in pairs.values()} == {(2, (6, 6)), (4, (1, 1))} and all(isinstance(b, blocks.TransformerBlock) for b in pairs)
    monkeypatch.setattr(den.mid_block, "has_cross_attention", False)      # a UNet whose last level has no spatial transformer at all
    with pytest.raises(ValueError, match=r"level 3, which has no attention block \(down_blocks.3, up_blocks.0, mid_block\)"):
        den.tile_attention_plan((1, 1, 1, 2))


def _module(den, prefix):
    m = den
    for part in prefix.split("."):
        m = m[int(part)] if part.isdigit() else getattr(m, part)
    return m


# zero_inputs() is a 2 x 2 latent: level 0 is 2 x 2, level 1 is 1 x 1
BAD = [(dict(tile_attention=0), "1..8"), (dict(tile_attention=9), "1..8"), (dict(tile_attention=(2, -1)), "1..8"), (dict(tile_attention=2.0), "integer"),
       (dict(tile_attention="2"), "1..8"), (dict(tile_attention=None), "integer"), (dict(tile_attention=2, tile_attention_shift="random"), "tile_attention_shift"),
       (dict(tile_attention_shift=None), "tile_attention_shift"), (dict(tile_attention=4), "factor 4 on level 0, whose token grid is 2 x 2"),
       (dict(tile_attention=(1, 2)), "factor 2 on level 1, whose token grid is 1 x 1"),
       (dict(tile_attention=2, kv_downsample=2), "leaves tiles of 1 x 1 tokens, smaller than that level's kv_downsample factor 2")]


@pytest.mark.parametrize("kw,msg", BAD)
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_bad_arguments_raise_before_any_unet(monkeypatch, kw, msg, make):
    fake_ops.install(monkeypatch)
    TR.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, make())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 4, 3.5, **kw)
    assert refu.calls == 0 and den.calls == 0 and fake_ops.CALLS == []


GRID_BAD = [((1, 4, 1, 5, 7), dict(tile_attention=2), "factor 2 on level 0, whose token grid is 5 x 7"),
            ((1, 4, 1, 16, 16), dict(tile_attention=(2, 2, 2, 4)), "factor 4 on level 3, whose token grid is 2 x 2"),
            ((1, 4, 1, 16, 16), dict(tile_attention=(4,), kv_downsample=(8,)), "tiles of 4 x 4 tokens, smaller than that level's kv_downsample factor 8")]


@pytest.mark.parametrize("shape,kw,msg", GRID_BAD)
def test_grid_refusals_raise_before_any_unet(monkeypatch, shape, kw, msg):
    fake_ops.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, _ddim())
    lat = torch.zeros(shape, dtype=torch.float16)
    rl = torch.zeros((1, shape[2], 22) + shape[3:], dtype=torch.float16)
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(lat, rl, zero_inputs()[2], 4, 3.5, **kw)
    assert refu.calls == 0 and den.calls == 0 and fake_ops.CALLS == []


def test_too_many_factors_raise_before_anything_runs(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    lat, rl, emb = (t.half() for t in small_inputs(2, 3))
    with pytest.raises(ValueError, match="5 factors for a UNet of 4"):
        pipe.denoise(lat, rl, emb, 2, 3.5, tile_attention=(2, 1, 1, 1, 1))
    assert fake_ops.CALLS == []


def test_call_refuses_before_clip_and_vae_and_forwards_the_keywords(monkeypatch):
    from PIL import Image
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append({k: v for k, v in kw.items() if k.startswith("tile_")})
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    custom = dict(tile_attention=(2, 2), tile_attention_shift="none")
    # a 32 x 32 image is a 4 x 4 latent: 4, 2, 1, 1
    bad = [b for b in BAD if "token" not in b[1]] + [(dict(tile_attention=8), "factor 8 on level 0, whose token grid is 4 x 4"),
                                                      (dict(tile_attention=(1, 1, 2)), "factor 2 on level 2, whose token grid is 1 x 1"),
                                                      (dict(tile_attention=2, kv_downsample=4), "tiles of 2 x 2 tokens, smaller than that level's kv_downsample factor 4")]
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        del seen[:]
        clip = fake_ops.FakeCLIP()
        calls = []
        clip.register_forward_hook(lambda *a: calls.append(1))
        asked = []
        stub = types.SimpleNamespace(in_channels=4, tile_attention_plan=lambda factors: asked.append(factors),
                                     kv_downsample_plan=lambda factors, mode: asked.append((factors, mode)))
        pipe = cls(vae=fake_ops.FakeVAE(), image_encoder=clip, reference_unet=None, denoising_unet=stub, scheduler=_ddim())
        args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5)
        for kw, msg in bad:
            with pytest.raises(ValueError, match=msg):
                pipe(*args, generator=torch.Generator().manual_seed(0), **kw)
        assert not calls and not seen and not asked
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), tile_attention=(1, 1))
        pipe(*args, generator=torch.Generator().manual_seed(0), **custom)
        assert seen == [dict(tile_attention=1, tile_attention_shift="cycle"), dict(tile_attention=(1, 1), tile_attention_shift="cycle"), custom]
        assert asked == [(2, 2)]                                           # the UNet is asked once, for the call with a factor > 1


def test_block_refuses_a_grid_that_is_not_its_token_count(monkeypatch):
    import todo_ref as T
    fake_ops.install(monkeypatch)
    TR.install(monkeypatch)
    st = T.block_setup(64, 64, 4, 4, 1, torch.device("cpu"))
    with pytest.raises(ValueError, match="does not hold L = 16"):
        st.blk(st.x.reshape(-1, 64), 2, 16, st.cross, sa=blocks.SelfAttnCall(tile={st.blk: (2, (0, 0))}), grid=(4, 5))


# ---- 3. one TransformerBlock on the emulated operators
@pytest.mark.parametrize("Hh,Ww,shift,pool", [(8, 8, (0, 0), None), (8, 8, (3, 5), None), (6, 10, (2, 7), None), (8, 8, (1, 2), (2, "mean"))])
def test_block_matches_restatement_in_every_reference_mode(monkeypatch, Hh, Ww, shift, pool):
    """token_tile calls over the five forward runs: plain, write and the unconditional half have no bank -- one reorder each where Lt % 8 == 0
    and nothing pools, 3 in all -- while the whole CFG batch and the conditional half reorder q's and K / V's source apart, 4 in all.  On
    6 x 10 (Lt = 15, K / V at a stride of 16) and under pooling every run reorders twice: 10."""
    import todo_ref as T
    fake_ops.install(monkeypatch)
    TR.install(monkeypatch)
    st = T.block_setup(64, 64, Hh, Ww, 2, torch.device("cpu"))
    TR.clear()
    plain = TR.block_runs(st, None, kv_pool=pool)
    assert not [n for n, _ in fake_ops.CALLS if n.startswith("token_t")]
    TR.clear()
    runs = TR.block_runs(st, (2, shift), kv_pool=pool)
    one = pool is None and (Hh // 2) * (Ww // 2) % 8 == 0
    assert len([n for n, _ in fake_ops.CALLS if n == "token_tile"]) == (3 * 1 + 2 * 2 if one else 5 * 2)
    assert len([n for n, _ in fake_ops.CALLS if n == "token_untile"]) == 5
    self_att = [d for b, n, d in TR.BLOCK_CALLS if n == "attention" and not d[4]]
    assert len(self_att) == 5 and all(d[1] == (Hh // 2) * (Ww // 2) and d[0] in (8, 16) for d in self_att)
    for case, (got, want) in runs.items():
        r, c, r0 = rel_l2(got, want), cosine(got, want), rel_l2(*plain[case])
        moved = rel_l2(plain[case][1], want)
        print(f"\nTILE_HOST_BLOCK {Hh}x{Ww} shift {shift} pool {pool} {case}: rel_l2 {r:.3e} cos {c:.7f} (tile=None {r0:.3e}; tiled vs untiled restated {moved:.3e})")
        assert r < BOUND["rel"] and c > BOUND["cos"], (case, r, c)
        if case == "write-bank":
            assert torch.equal(got, plain[case][0]) and got.shape == (4, Hh * Ww, 64)      # the bank is norm1(x) in frame order
        else:
            assert moved > 0.0


def test_seg_block_blurs_then_tiles_and_pag_block_ignores_the_field(monkeypatch):
    import todo_ref as T
    fake_ops.install(monkeypatch)
    TR.install(monkeypatch)
    st = T.block_setup(64, 64, 8, 8, 2, torch.device("cpu"))
    TR.clear()
    got, want = TR.block_runs(st, (2, (3, 1)), sigma=1.5)["seg"]
    order = [n for n, _ in fake_ops.CALLS if n in ("token_blur", "token_tile", "token_untile") or n == "attention"]
    assert order[:4] == ["token_blur", "token_tile", "token_tile", "attention"] and "token_untile" in order
    assert rel_l2(got, want) < BOUND["rel"] and cosine(got, want) > BOUND["cos"]
    untiled = TR.block_runs(st, None, sigma=1.5)["seg"][1]
    assert rel_l2(untiled, want) > 0.0
    # an identity-map block has no attention to tile
    blk = st.blk
    blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [st.bank]
    h = st.x[2:].reshape(-1, 64)
    a = blk(h.clone(), 2, 64, st.cross.rows(2, 4), sa=blocks.SelfAttnCall(identity=(blk,)))
    TR.clear()
    b = blk(h.clone(), 2, 64, st.cross.rows(2, 4), sa=blocks.SelfAttnCall(identity=(blk,), tile={blk: (2, (1, 1))}), grid=(8, 8))
    assert torch.equal(a, b) and not [n for n, _ in fake_ops.CALLS if n.startswith("token_t")]
    blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []


# ---- 4. the whole loop on the emulated operators, against the restated loop
PAG0 = dict(pag_scale=3.0, pag_applied_layers=("down_blocks.0",))
SEG0 = dict(seg_scale=3.0, seg_blur_sigma=1.5, seg_applied_layers=("down_blocks.0",))
LOOPS = {"1-cycle-ddim-cfg": dict(tile=(2,), shift="cycle"),
         "2-none-2m": dict(tile=(2, 2), shift="none", sampler="2m", steps=3),
         "3-kv-mean": dict(tile=(2,), steps=2, kw=dict(kv_downsample=(2,), kv_downsample_mode="mean")),
         "4-pag": dict(tile=(2,), steps=2, kw=PAG0),
         "4-seg": dict(tile=(2,), steps=2, kw=SEG0),
         "5-two-windows": dict(tile=(2,), frames=12, steps=2, kw=dict(context_schedule="uniform_open", **OPEN2)),
         "6-free-init": dict(tile=(2,), steps=2, kw=dict(free_init_iters=2)),
         "7-v2v": dict(tile=(2,), steps=4, kw=dict(strength=0.5), init=True)}


def _restated_kw(cfg, lat):
    """The keywords of tile_ref.denoise_loop for a case's denoise() keywords."""
    kw, out = dict(cfg.get("kw", {})), dict(guidance_scale=3.5)
    if "kv_downsample" in kw:
        out.update(kv_downsample=kw["kv_downsample"], kv_mode=kw["kv_downsample_mode"])
    if "pag_scale" in kw:
        out.update(pag_scale=kw["pag_scale"], pag_layers=kw["pag_applied_layers"])
    if "seg_scale" in kw:
        out.update(seg_scale=kw["seg_scale"], seg_blur_sigma=kw["seg_blur_sigma"], seg_layers=kw["seg_applied_layers"])
    if "context_schedule" in kw:
        out.update(schedule=kw["context_schedule"], **OPEN2)
    if "free_init_iters" in kw:
        out.update(free_init_iters=kw["free_init_iters"], generator=torch.Generator().manual_seed(11))
    if cfg.get("init"):
        out.update(init_latents=lat * 0.18215 + 0.1, strength=kw["strength"])
    return out


def _check_calls(den, factors):
    """token_tile in exactly the selected blocks, and no self-attention launch of a tiled block over the whole frame."""
    selected = {st.transformer_blocks[0] for st in den.tile_attention_plan(factors)}
    tiling = {b for b, n, _ in TR.BLOCK_CALLS if n == "token_tile"}
    assert tiling == selected and {b for b, n, _ in TR.BLOCK_CALLS if n == "token_untile"} <= selected
    grids = {b: d[1:3] + (d[4],) for b, n, d in TR.BLOCK_CALLS if n == "token_tile"}
    n_att = 0
    for b, n, d in TR.BLOCK_CALLS:
        if n == "attention" and b in selected and not d[4]:               # self-attention (no kv_index)
            Hh, Ww, t = grids[b]
            assert d[1] == (Hh // t) * (Ww // t) != Hh * Ww and d[0] % (t * t) == 0, d
            n_att += 1
    assert n_att > 0
    return selected


@pytest.mark.parametrize("case", list(LOOPS))
def test_host_loop_matches_restatement(monkeypatch, small_cpu, case):
    fake_ops.install(monkeypatch)
    TR.install(monkeypatch)
    cfg = LOOPS[case]
    ref, den, ref_sd, den_sd = small_cpu
    frames, steps = cfg.get("frames", 4), cfg.get("steps", 4)
    lat, rl, emb = small_inputs(frames, 230 + frames)
    two_m = cfg.get("sampler") == "2m"
    kw = dict(cfg.get("kw", {}))
    rkw = _restated_kw(cfg, lat)
    if cfg.get("init"):
        kw["init_latents"] = rkw["init_latents"].half()
        rkw["init_latents"] = kw["init_latents"].float()
    mk_rs = (lambda: R.Restated(2, "dpmsolver++", "midpoint")) if two_m else None
    if "free_init_iters" in kw:
        rkw["make_scheduler"] = mk_rs
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _dpm() if two_m else _ddim())
    gen = lambda: dict(generator=torch.Generator().manual_seed(11)) if "free_init_iters" in kw else {}
    TR.clear()
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), steps, 3.5, tile_attention=cfg["tile"], tile_attention_shift=cfg.get("shift", "cycle"), **kw, **gen())
    selected = _check_calls(den, cfg["tile"])
    shifts = {d[5] for _, n, d in TR.BLOCK_CALLS if n == "token_tile" and d[1] == 16}
    if case == "1-cycle-ddim-cfg":
        assert shifts == {(0, 0), (2, 2), (4, 4), (6, 6)}                 # all four shifts of the 8 x 8 tiles occur
    if cfg.get("shift") == "none":
        assert shifts == {(0, 0)}
    if case == "7-v2v":
        assert shifts == {(4, 4), (6, 6)}                                 # steps 2 and 3 of 4 are kept, with their own shifts
    if case == "6-free-init":
        b0 = next(iter(selected))
        assert [d[5] for b, n, d in TR.BLOCK_CALLS if n == "token_untile" and b is b0] == [(0, 0), (2, 2), (0, 0), (2, 2)]      # every pass starts over
    if case.startswith("4-"):                                             # a selected block is also a tiled one
        assert set(den.pag_blocks(("down_blocks.0",))) < selected
    plain_out = pipe.denoise(lat.half(), rl.half(), emb.half(), steps, 3.5, **kw, **gen())
    with torch.no_grad():
        sched = {} if "free_init_iters" in kw else dict(scheduler=mk_rs() if mk_rs else None)
        want = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, tile_attention=cfg["tile"], tile_attention_shift=cfg.get("shift", "cycle"), **rkw, **sched)
        if "generator" in rkw:
            rkw["generator"] = torch.Generator().manual_seed(11)
        sched = {} if "free_init_iters" in kw else dict(scheduler=mk_rs() if mk_rs else None)
        plain = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, tile_attention=1, **rkw, **sched)
    e, c, e0, d = rel_l2(out.float(), want), cosine(out.float(), want), rel_l2(plain_out.float(), plain), rel_l2(plain, want)
    print(f"\nTILE_HOST_LOOP {case} rel_l2 {e:.3e} cos {c:.7f} (plain loop {e0:.3e}, ratio {e / e0:.2f}; restated plain vs tiled {d:.3e})")
    assert torch.isfinite(out).all() and e <= BOUND["rel"] and c >= BOUND["cos"], (e, c)
    assert e <= 2.0 * e0, (e, e0)
    assert d > 0.0 and not torch.equal(out, plain_out)


def test_two_queues_flag_on_the_emulation(monkeypatch, small_cpu):
    """The emulation has no device, so forward_nhwc takes its one-queue path with the flag on or off: the flag must not change what the
    tiled loop computes there (the two-queue path itself runs in tests/test_tile_attention_gpu.py)."""
    fake_ops.install(monkeypatch)
    TR.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 61))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    outs = []
    for tq in (False, True):
        monkeypatch.setattr(pipe, "two_queues", tq, raising=False)
        TR.clear()
        outs.append(pipe.denoise(lat, rl, emb, 2, 3.5, tile_attention=(2,)))
        _check_calls(den, (2,))
    assert torch.equal(*outs)


def test_restated_loop_with_factor_one_is_the_oracle_loop(small_cpu):
    from oracle import cpu_ref as O
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 82)
    with torch.no_grad():
        want = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True)
        got = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, tile_attention=(1, 1), guidance_scale=3.5)
        moved = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, tile_attention=(2,), guidance_scale=3.5)
    assert torch.equal(got, want) and not torch.equal(moved, want)
    assert O.transformer_block_read.__module__ == "oracle.cpu_ref" and O.transformer_3d.__module__ == "oracle.cpu_ref"      # swapped back
    assert O.denoising_unet_forward.__module__ == "oracle.cpu_ref"


# ---- 5. the default path
def test_default_is_the_same_call_log_and_the_same_bits(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    TR.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 19))
    keywords = []
    real = den.forward_nhwc

    def forward_nhwc(*a, **kw):
        keywords.append(sorted(kw))
        return real(*a, **kw)

    monkeypatch.setattr(den, "forward_nhwc", forward_nhwc, raising=False)
    for make in (_ddim, _dpm):
        pipe = M.MikuDanceVideoPipeline(None, None, ref, den, make())
        TR.clear()
        a = pipe.denoise(lat, rl, emb, 2, 3.5)
        calls_a = list(fake_ops.CALLS)
        for kw in (dict(tile_attention=1), dict(tile_attention=(1, 1), tile_attention_shift="none"), dict(tile_attention=())):
            TR.clear()
            b = pipe.denoise(lat, rl, emb, 2, 3.5, **kw)
            assert torch.equal(a, b) and calls_a == fake_ops.CALLS         # the same operator calls, one for one
        assert not [n for n, _ in calls_a if n.startswith("token_t")]
        assert all(k == ["halves_identical", "two_queues"] for k in keywords), keywords      # no new keyword reaches forward_nhwc
        del keywords[:]
        TR.clear()
        c = pipe.denoise(lat, rl, emb, 2, 3.5, tile_attention=2)
        assert not torch.equal(a, c) and "token_tile" in [n for n, _ in fake_ops.CALLS]
        assert all(k == ["halves_identical", "tile_attention", "tile_shift", "two_queues"] for k in keywords), keywords
        del keywords[:]


# ---- 6. the feature acts
def test_restated_tiled_loop_is_far_from_the_restated_plain_loop(small_cpu):
    """On the restatement alone: 4 frames, seed 234 (case 1's clip), 4 DDIM steps under CFG, (2,) "cycle" -- the tiled loop's result lies at
    least 10 x the loop bound (rel-L2 3e-2) from the plain loop's, so a product that ignored the keyword could not pass case 1."""
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 234)
    with torch.no_grad():
        tiled = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, tile_attention=(2,), guidance_scale=3.5)
        plain = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, tile_attention=1, guidance_scale=3.5)
    d = rel_l2(tiled, plain)
    print(f"\nTILE_ACTS restated (2,) cycle vs plain: rel_l2 {d:.3e}")
    assert d >= 10 * BOUND["rel"], d


# ---- 7. window parallelism: three gloo ranks
WP = dict(context_frames=8, context_stride=1, context_overlap=2)           # 16 frames: 3 windows, the last one wraps


def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    import tile_ref
    tile_ref.install_process()
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=521))
    kw = dict(WP, tile_attention=(2,))
    pipe = MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat, rl, emb, 2, 3.5, window_parallel=dp.WindowParallel(), **kw)
    got = dp.gather_latents(out)
    if rank == 0:
        selected = {st.transformer_blocks[0] for st in den.tile_attention_plan((2,))}
        exact = {b for b, n, _ in tile_ref.BLOCK_CALLS if n == "token_tile"} == selected
        one = pipe.denoise(lat, rl, emb, 2, 3.5, **kw)
        plain = pipe.denoise(lat, rl, emb, 2, 3.5, **dict(kw, tile_attention=1))
        q.put(dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                   finite=bool(torch.isfinite(out).all()), tiled=not torch.equal(out, plain), exact_blocks=exact,
                   out=out.float().numpy(), plain=plain.float().numpy()))
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank_and_matches_restatement(small_cpu):
    res = run_world(3, _wp_worker)
    out, plain_out = torch.from_numpy(res.pop("out")), torch.from_numpy(res.pop("plain"))
    assert all(res.values()), res
    from mikudance_amd.synth import synth_inputs
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = (t.half().float() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=521))
    with torch.no_grad():
        want = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, tile_attention=(2,), guidance_scale=3.5, **WP)
        plain = TR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, tile_attention=1, guidance_scale=3.5, **WP)
    e, c, e0 = rel_l2(out, want), cosine(out, want), rel_l2(plain_out, plain)
    print(f"\nTILE_HOST_LOOP 9-window-parallel rel_l2 {e:.3e} cos {c:.7f} (plain loop {e0:.3e}, ratio {e / e0:.2f})")
    assert e <= BOUND["rel"] and c >= BOUND["cos"] and e <= 2.0 * e0, (e, c, e0)


# ---- 8. the script
def test_script_flags_parse():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.tile_attention, a.tile_attention_shift) == ((1,), "cycle")
    a = IV.parse_args(["--tile_attention", "2"])
    assert (a.tile_attention, a.tile_attention_shift) == ((2,), "cycle")
    a = IV.parse_args(["--tile_attention", "2,2", "--tile_attention_shift", "none"])
    assert (a.tile_attention, a.tile_attention_shift) == ((2, 2), "none")
    for bad in (["--tile_attention", "two"], ["--tile_attention", "2,"], ["--tile_attention_shift", "random"]):
        with pytest.raises(SystemExit):
            IV.parse_args(bad)
    assert "tile_attention=--tile_attention" in IV.__doc__


def test_script_flags_reach_denoise_and_refusals_keep_their_text(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append((kw["tile_attention"], kw["tile_attention_shift"]))
        return latents

    build = fake_pipeline_builder(IV)

    def build_with_plan(*a, **kw):
        pipe = build(*a, **kw)
        pipe.denoising_unet.tile_attention_plan = lambda factors: None    # the stand-in UNet of the builder has no blocks to ask
        return pipe

    monkeypatch.setattr(IV, "build_pipeline", build_with_plan)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)                                      # 32 x 32: a 4 x 4 latent
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base)
    IV.main(base + ["--tile_attention", "2"])
    IV.main(base + ["--tile_attention", "2,2", "--tile_attention_shift", "none"])
    assert seen == [((1,), "cycle"), ((2,), "cycle"), ((2, 2), "none")]
    with pytest.raises(ValueError, match="tile_attention: factor 8 on level 0, whose token grid is 4 x 4 for this latent size: 8 must divide both sides"):
        IV.main(base + ["--tile_attention", "8"])
    with pytest.raises(ValueError, match="tile_attention: every factor must be an integer in 1..8, got 9"):
        IV.main(base + ["--tile_attention", "9"])
    assert len(seen) == 3
