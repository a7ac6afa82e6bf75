"""CPU: K / V token downsampling (kv_downsample=, ToDo, arXiv 2402.13573) -- the torch definition against hand-computed grids, the operator's
emulation against the definition, the plan builder and every refusal, one TransformerBlock in every reference mode and the host graph of the
denoising UNet on emulated operators (values and call log), the whole loop of MikuDanceVideoPipeline.denoise() against the restated loop
(one rank and three gloo ranks), and the script's flags."""
import collections
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd import blocks
from mikudance_amd.selftest import SCHED_KWARGS
from oracle import cpu_ref as O

import dpmpp_ref as R
import fake_ops
import fusion_ref as FR
import pag_ref as P
import todo_ref as T
from loop_helpers import (CountingUNet, cosine, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401
                          worker_setup, zero_inputs)

BOUND = dict(rel=2e-2, cos=0.999)                                          # tests/test_host_graph_cpu.py, forward and loop alike
OPEN20 = dict(context_frames=8, context_stride=1, context_overlap=2)       # uniform_open on 12 frames: two windows


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


# ---- 1. the definition against grids computed by hand
def _grid(Hh, Ww, C=2):
    """Token (y, x) holds 10 y + x in channel 0 and its negative in channel 1; two frames, the second offset by 100."""
    g = torch.tensor([[10.0 * y + x for x in range(Ww)] for y in range(Hh)])
    one = torch.stack([g, -g], -1).reshape(Hh * Ww, C)
    return torch.stack([one, one + 100.0])


def test_pool_matches_hand_computed_grids():
    # 4 x 4, s = 2
    x = _grid(4, 4)
    assert T.pool(x, 2, 4, 4, 2, "nearest")[0, :, 0].tolist() == [0.0, 2.0, 20.0, 22.0]
    assert T.pool(x, 2, 4, 4, 2, "nearest")[1, :, 1].tolist() == [100.0, 98.0, 80.0, 78.0]
    assert T.pool(x, 2, 4, 4, 2, "mean")[0, :, 0].tolist() == [5.5, 7.5, 25.5, 27.5]
    # 5 x 7, s = 2: the last row and the last column are dropped (2 x 3 blocks)
    x = _grid(5, 7)
    assert T.pool(x, 2, 5, 7, 2, "nearest")[0, :, 0].tolist() == [0.0, 2.0, 4.0, 20.0, 22.0, 24.0]
    assert T.pool(x, 2, 5, 7, 2, "mean")[0, :, 0].tolist() == [5.5, 7.5, 9.5, 25.5, 27.5, 29.5]
    assert T.pool(x.reshape(-1, 2), 2, 5, 7, 2, "mean")[1, :, 1].tolist() == [94.5, 92.5, 90.5, 74.5, 72.5, 70.5]
    # 6 x 4, s = 3: one column dropped; 7 x 7, s = 3: one row and one column; 3 x 9, s = 3: exact
    x = _grid(6, 4)
    assert T.pool(x, 2, 6, 4, 3, "nearest")[0, :, 0].tolist() == [0.0, 30.0] and T.pool(x, 2, 6, 4, 3, "mean")[0, :, 0].tolist() == [11.0, 41.0]
    x = _grid(7, 7)
    assert T.pool(x, 2, 7, 7, 3, "nearest")[0, :, 0].tolist() == [0.0, 3.0, 30.0, 33.0]
    assert T.pool(x, 2, 7, 7, 3, "mean")[0, :, 0].tolist() == [11.0, 14.0, 41.0, 44.0]
    assert T.pool(_grid(3, 9), 2, 3, 9, 3, "nearest")[0, :, 0].tolist() == [0.0, 3.0, 6.0]
    # 8 x 8, s = 8 and s = 5 (one block each)
    x = _grid(8, 8)
    assert T.pool(x, 2, 8, 8, 8, "mean")[0, :, 0].tolist() == [38.5] and T.pool(x, 2, 8, 8, 5, "mean")[0, :, 0].tolist() == [22.0]
    assert T.pool(x, 2, 8, 8, 5, "nearest").shape == (2, 1, 2)


@pytest.mark.parametrize("B,Hh,Ww,C,s", [(2, 5, 7, 16, 2), (1, 8, 8, 8, 4), (3, 6, 4, 24, 3), (2, 16, 16, 8, 2), (1, 9, 23, 8, 7), (1, 8, 8, 8, 8)])
def test_emulated_operator_is_the_definition(B, Hh, Ww, C, s):
    """The emulation (slices, the kernel's order of additions) against the two torch calls.  Inputs on a 2^-6 grid in [-8, 8]: every fp32 sum
    of <= 64 of them is exact, so the mean differs from the float64 mean by the rounding of 1 / s^2 alone: within 1 fp16 ulp after rounding."""
    g = torch.Generator().manual_seed(B * 100 + Hh + s)
    x = (torch.randn((B * Hh * Ww, C), generator=g) * 2).clamp(-8, 8).mul(64).round().div(64).half()
    for mode in ("nearest", "mean"):
        y, Lk, stride = T.token_pool(x, B, Hh, Ww, s, mode)
        assert Lk == (Hh // s) * (Ww // s) and stride == (Lk + 7) // 8 * 8 and y.shape == (B * stride, C)
        yv = y.view(B, stride, C)
        assert (yv[:, Lk:] == 0).all() and not torch.signbit(yv[:, Lk:]).any()
        want = T.pool(x.double(), B, Hh, Ww, s, mode).half()
        if mode == "nearest":
            assert torch.equal(yv[:, :Lk], want)
        else:
            ulp = torch.maximum(torch.tensor(2.0 ** -24), 2.0 ** (torch.floor(torch.log2(want.double().abs().clamp_min(2.0 ** -14))) - 10))
            assert ((yv[:, :Lk].double() - want.double()).abs() <= ulp).all()
    assert [n for n, _ in fake_ops.CALLS if n == "token_pool"][-2:] == ["token_pool"] * 2


# ---- 2. the plan builder and the refusals
def test_plan_covers_the_documented_blocks(small_cpu):
    _, den, _, den_sd = small_cpu
    of = {a.transformer_blocks[0]: p for p, _ in den.attention_block_prefixes() for a in [_module(den, p)]}
    names = lambda plan: sorted(of[a.transformer_blocks[0]] for a in plan)
    lvl0 = ["down_blocks.0.attentions.0", "down_blocks.0.attentions.1"] + [f"up_blocks.3.attentions.{j}" for j in range(3)]
    lvl1 = ["down_blocks.1.attentions.0", "down_blocks.1.attentions.1"] + [f"up_blocks.2.attentions.{j}" for j in range(3)]
    assert den.kv_downsample_plan(1) is None and den.kv_downsample_plan((1, 1, 1, 1)) is None and den.kv_downsample_plan(()) is None
    plan = den.kv_downsample_plan(2)
    assert names(plan) == sorted(lvl0) and set(plan.values()) == {(2, "nearest")}
    plan = den.kv_downsample_plan((4, 2), "mean")
    assert names(plan) == sorted(lvl0 + lvl1) and {of[a.transformer_blocks[0]]: v for a, v in plan.items()}["up_blocks.2.attentions.1"] == (2, "mean")
    assert set(plan.values()) == {(4, "mean"), (2, "mean")}
    # the last level has no attention block in its down / up block: it covers mid_block
    assert names(den.kv_downsample_plan((1, 1, 1, 2))) == ["mid_block.attentions.0"]
    # the same assignment, from the key prefixes alone
    for factors in ((2,), (4, 2), (1, 3, 1, 2)):
        want = sorted(p for p in P.block_prefixes(den_sd) if T.factor_of(p + ".", factors, 4) > 1)
        assert names(den.kv_downsample_plan(factors)) == want
    for bad, msg in (((2, 2, 2, 2, 2), "5 factors for a UNet of 4"), ((0,), "1..8"), ((9,), "1..8"), ((2.0,), "1..8"), ((True,), "1..8"), ("2", "1..8"),
                     (None, "integer or a sequence"), (2.5, "integer or a sequence")):
        with pytest.raises(ValueError, match=msg):
            den.kv_downsample_plan(bad)
    with pytest.raises(ValueError, match="kv_downsample_mode"):
        den.kv_downsample_plan(2, "bilinear")


def _module(den, prefix):
    m = den
    for part in prefix.split("."):
        m = m[int(part)] if part.isdigit() else getattr(m, part)
    return m


def test_a_level_without_attention_is_refused_by_name(monkeypatch, small_cpu):
    _, den, _, _ = small_cpu
    monkeypatch.setattr(den.mid_block, "has_cross_attention", False)      # a UNet whose last level has no spatial transformer at all
    with pytest.raises(ValueError, match=r"level 3, which has no attention block \(down_blocks.3, up_blocks.0, mid_block\)"):
        den.kv_downsample_plan((1, 1, 1, 2))
    assert den.kv_downsample_plan((2, 1, 1, 1)) is not None


BAD = [(dict(kv_downsample=0), "1..8"), (dict(kv_downsample=9), "1..8"), (dict(kv_downsample=(2, -1)), "1..8"), (dict(kv_downsample=2.0), "integer"),
       (dict(kv_downsample=(2, 1.5)), "1..8"), (dict(kv_downsample="2"), "1..8"), (dict(kv_downsample=None), "integer"),
       (dict(kv_downsample=2, kv_downsample_mode="area"), "kv_downsample_mode"), (dict(kv_downsample_mode=None), "kv_downsample_mode"),
       # zero_inputs() is a 2 x 2 latent: level 0 has one 2 x 2 block, no 3 x 3 block; level 1 is 1 x 1
       (dict(kv_downsample=3), "factor 3 on level 0, whose token grid is 2 x 2"), (dict(kv_downsample=(1, 2)), "factor 2 on level 1, whose token grid is 1 x 1")]


@pytest.mark.parametrize("kw,msg", BAD)
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_bad_arguments_raise_before_any_unet(monkeypatch, kw, msg, make):
    fake_ops.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, make())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 4, 3.5, **kw)
    assert refu.calls == 0 and den.calls == 0 and fake_ops.CALLS == []


def test_levels_halve_with_ceil():
    from mikudance_amd.unet_3d_mix import check_kv_downsample_grid
    check_kv_downsample_grid((2, 2, 2), 5, 7)                              # 5 x 7 -> 3 x 4 -> 2 x 2
    with pytest.raises(ValueError, match="level 3, whose token grid is 1 x 1"):
        check_kv_downsample_grid((2, 2, 2, 2), 5, 7)
    with pytest.raises(ValueError, match="level 1, whose token grid is 3 x 4"):
        check_kv_downsample_grid((1, 4), 5, 7)
    check_kv_downsample_grid((1, 1, 1, 1), 1, 1)
    check_kv_downsample_grid((8, 1, 1, 1), 96, 96)


def test_too_many_factors_raise_before_anything_runs(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    lat, rl, emb = (t.half() for t in small_inputs(2, 3))
    with pytest.raises(ValueError, match="5 factors for a UNet of 4"):
        pipe.denoise(lat, rl, emb, 2, 3.5, kv_downsample=(2, 1, 1, 1, 1))
    assert fake_ops.CALLS == []


def test_call_refuses_before_clip_and_vae_and_forwards_the_keywords(monkeypatch):
    from PIL import Image
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append({k: v for k, v in kw.items() if k.startswith("kv_")})
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    custom = dict(kv_downsample=(2, 2), kv_downsample_mode="mean")
    bad = [b for b in BAD if "whose token grid" not in b[1]] + [(dict(kv_downsample=8), "factor 8 on level 0, whose token grid is 4 x 4")]
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        del seen[:]
        clip = fake_ops.FakeCLIP()
        calls = []
        clip.register_forward_hook(lambda *a: calls.append(1))
        asked = []
        stub = types.SimpleNamespace(in_channels=4, kv_downsample_plan=lambda factors, mode: asked.append((factors, mode)))
        pipe = cls(vae=fake_ops.FakeVAE(), image_encoder=clip, reference_unet=None, denoising_unet=stub, scheduler=_ddim())
        args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5)
        for kw, msg in bad:
            with pytest.raises(ValueError, match=msg):
                pipe(*args, generator=torch.Generator().manual_seed(0), **kw)
        assert not calls and not seen and not asked
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), kv_downsample=(1, 1))
        pipe(*args, generator=torch.Generator().manual_seed(0), **custom)
        assert seen == [dict(kv_downsample=1, kv_downsample_mode="nearest"), dict(kv_downsample=(1, 1), kv_downsample_mode="nearest"), custom]
        assert asked == [((2, 2), "mean")]                                 # the UNet is asked once, for the call with a factor > 1


# ---- 3. one TransformerBlock on the emulated operators, every reference mode
@pytest.mark.parametrize("Hh,Ww,s,mode", [(8, 8, 2, "nearest"), (5, 7, 2, "mean"), (6, 4, 3, "nearest")])
def test_block_matches_restatement_in_every_reference_mode(monkeypatch, Hh, Ww, s, mode):
    fake_ops.install(monkeypatch)
    st = T.block_setup(64, 64, Hh, Ww, 2, torch.device("cpu"))
    del fake_ops.CALLS[:]
    plain = T.block_runs(st, None)
    assert not [n for n, _ in fake_ops.CALLS if n == "token_pool"]
    runs = T.block_runs(st, (Hh, Ww, s, mode))
    assert len([n for n, _ in fake_ops.CALLS if n == "token_pool"]) == 5   # every run but the bank read-back
    for case, (got, want) in runs.items():
        r, c = rel_l2(got, want), cosine(got, want)
        r0 = rel_l2(*plain[case])
        moved = rel_l2(plain[case][1], want)
        print(f"\nTODO_HOST_BLOCK {Hh}x{Ww} s{s} {mode} {case}: rel_l2 {r:.3e} cos {c:.7f} (kv_pool=None {r0:.3e}; pooled vs plain restated {moved:.3e})")
        assert r < BOUND["rel"] and c > BOUND["cos"], (case, r, c)
        if case == "write-bank":
            assert torch.equal(got, plain[case][0]) and got.shape == (4, Hh * Ww, 64)      # the bank is the full-resolution norm1(x)
        else:
            assert moved > 0.0


def test_block_refuses_a_grid_that_is_not_its_token_count(monkeypatch):
    fake_ops.install(monkeypatch)
    st = T.block_setup(64, 64, 4, 4, 1, torch.device("cpu"))
    with pytest.raises(ValueError, match="does not hold L = 16"):
        st.blk(st.x.reshape(-1, 64), 2, 16, st.cross, sa=blocks.SelfAttnCall(pool={st.blk: (2, "nearest")}), grid=(4, 5))


def test_perturbed_block_ignores_kv_pool(monkeypatch):
    fake_ops.install(monkeypatch)
    st = T.block_setup(64, 64, 4, 4, 1, torch.device("cpu"))
    blk = st.blk
    blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [st.bank]
    h = st.x[1:].reshape(-1, 64)
    blk(h.clone(), 1, 16, st.cross.rows(1, 2), sa=blocks.SelfAttnCall(identity=(blk,)))                 # first call: projects the context K / V
    del fake_ops.CALLS[:]
    a = blk(h.clone(), 1, 16, st.cross.rows(1, 2), sa=blocks.SelfAttnCall(identity=(blk,)))
    log = list(fake_ops.CALLS)
    del fake_ops.CALLS[:]
    b = blk(h.clone(), 1, 16, st.cross.rows(1, 2), sa=blocks.SelfAttnCall(identity=(blk,), pool={blk: (2, "nearest")}), grid=(4, 4))
    assert torch.equal(a, b) and fake_ops.CALLS == log and "token_pool" not in [n for n, _ in log]
    c = blk(h.clone(), 1, 16, st.cross.rows(1, 2), sa=blocks.SelfAttnCall(identity=(), pool={blk: (2, "nearest")}), grid=(4, 4))   # unselected: pools as in the main evaluation
    assert "token_pool" in [n for n, _ in fake_ops.CALLS] and not torch.equal(a, c)
    blk.bank = []


# ---- 4. the host graph of the denoising UNet
def _attention_logged(monkeypatch):
    """fake_ops.attention does not log itself: record every launch in the same call list."""
    from mikudance_amd import ops
    real = ops.attention

    def attention(q, k, vt, B, H, D, Lq, Lk, kv_stride=None, kv_index=None, **kw):
        fake_ops.CALLS.append(("attention", (B, Lq, Lk, kv_stride, kv_index is not None, tuple(k.shape), tuple(vt.shape))))
        return real(q, k, vt, B, H, D, Lq, Lk, kv_stride=kv_stride, kv_index=kv_index, **kw)

    monkeypatch.setattr(ops, "attention", attention)


def _inputs10(frames, seed):
    """small_inputs cut down to a 10 x 10 latent: levels of 10 x 10, 5 x 5, 3 x 3 and 2 x 2 tokens, none a multiple of the next."""
    lat, rl, emb = small_inputs(frames, seed)
    return lat[..., :10, :10].contiguous(), rl[..., :10, :10].contiguous(), emb


def test_default_is_the_same_call_log_and_the_same_bits(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    _attention_logged(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 19))
    for make in (_ddim, _dpm):
        pipe = M.MikuDanceVideoPipeline(None, None, ref, den, make())
        del fake_ops.CALLS[:]
        a = pipe.denoise(lat, rl, emb, 2, 3.5)
        calls_a = list(fake_ops.CALLS)
        for kw in (dict(kv_downsample=1), dict(kv_downsample=(1, 1, 1, 1), kv_downsample_mode="mean"), dict(kv_downsample=())):
            del fake_ops.CALLS[:]
            b = pipe.denoise(lat, rl, emb, 2, 3.5, **kw)
            assert torch.equal(a, b) and calls_a == fake_ops.CALLS         # the same operator calls, one for one
        assert "token_pool" not in [n for n, _ in calls_a]
        del fake_ops.CALLS[:]
        c = pipe.denoise(lat, rl, emb, 2, 3.5, kv_downsample=2)
        assert not torch.equal(a, c) and "token_pool" in [n for n, _ in fake_ops.CALLS]


@pytest.mark.parametrize("factors,mode", [((2,), "nearest"), ((2, 2, 1, 2), "mean")], ids=["2-nearest", "2.2.1.2-mean"])
def test_host_graph_attention_calls_bank_and_values(monkeypatch, small_cpu, factors, mode):
    """One step of denoise() on a 2-frame 10 x 10 latent under CFG: which attention launch gets which Lk / kv_stride, what token_pool is
    handed, the bank it finds, and the result against the restated loop."""
    fake_ops.install(monkeypatch)
    _attention_logged(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = _inputs10(2, 41)
    f = 2
    grids = [(10, 10), (5, 5), (3, 3), (2, 2)]
    chans = [64, 128, 256, 256]
    level0 = [a.transformer_blocks[0] for a in den.kv_downsample_plan((2,))]
    banks_seen = []
    from mikudance_amd import ops
    emu = ops.token_pool

    def token_pool(x, B, Hh, Ww, s, mode="nearest", out=None):
        banks_seen.append([tuple(b.bank[0].shape) for b in level0 if b.bank])
        return emu(x, B, Hh, Ww, s, mode, out)

    monkeypatch.setattr(ops, "token_pool", token_pool)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 1, 3.5, kv_downsample=factors, kv_downsample_mode=mode)
    fac = list(factors) + [1] * (4 - len(factors))
    # the denoising UNet's self-attention launches (no kv_index; 2f frames, the reference UNet runs f), in evaluation order: 2 per down
    # level 0..2, mid, 3 per up level 2..0
    self_att = [d for n, d in fake_ops.CALLS if n == "attention" and not d[4] and d[0] == 2 * f]
    order = [0, 0, 1, 1, 2, 2, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0]
    assert len(self_att) == len(order)
    for lvl, (B, Lq, Lk, kv_stride, _, kshape, vtshape) in zip(order, self_att):
        Hh, Ww = grids[lvl]
        s = fac[lvl]
        assert B == 2 * f and Lq == Hh * Ww
        if s == 1:
            assert Lk == Lq and kv_stride is None and kshape == (B * Lq, chans[lvl])
        else:
            want_lk = (Hh // s) * (Ww // s)
            stride = (want_lk + 7) // 8 * 8
            assert (Lk, kv_stride) == (want_lk, stride) and kshape == (B * stride, chans[lvl]) and vtshape == (chans[lvl], B * stride)
    pools = [d for n, d in fake_ops.CALLS if n == "token_pool"]
    assert pools == [(2 * f, *grids[lvl], chans[lvl], fac[lvl], mode) for lvl in order if fac[lvl] > 1]
    # cross-attention is untouched: 5 context tokens at a stride of 8 everywhere
    assert {d[2:4] for n, d in fake_ops.CALLS if n == "attention" and d[4]} == {(5, 8)}
    # the bank a level-0 block reads is full resolution: (f, 100, 64), the conditional frames' norm1 rows of the reference UNet
    assert banks_seen and all(shapes and set(shapes) == {(f, 100, 64)} for shapes in banks_seen)
    with torch.no_grad():
        want = T.denoise_loop(ref_sd, den_sd, lat, rl, emb, 1, kv_downsample=factors, mode=mode, guidance_scale=3.5)
        plain = FR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 1, guidance_scale=3.5, reduced=True)
    e, c, d = rel_l2(out.float(), want), cosine(out.float(), want), rel_l2(plain, want)
    print(f"\nTODO_HOST_GRAPH {factors} {mode} rel_l2 {e:.3e} cos {c:.7f} (restated plain vs pooled: {d:.3e})")
    assert e < BOUND["rel"] and c > BOUND["cos"], (e, c)


# ---- 5. the whole loop on the emulated operators, against the restated loop
LOOPS = {"ddim-cfg": dict(frames=4, steps=3, guidance=3.5, kv=(2,), mode="nearest"),
         "ddim-no-cfg": dict(frames=4, steps=3, guidance=1.0, kv=(2, 2), mode="mean"),
         "2m-cfg": dict(frames=4, steps=3, guidance=3.5, kv=(2, 2), mode="mean", sampler="2m"),
         "2m-no-cfg": dict(frames=4, steps=3, guidance=1.0, kv=(2,), mode="nearest", sampler="2m"),
         "open-pyramid": dict(frames=12, steps=2, guidance=3.5, kv=(4, 2), mode="nearest", win=OPEN20, schedule="uniform_open", fuse="pyramid"),
         "pag": dict(frames=4, steps=2, guidance=3.5, kv=(2,), mode="nearest", pag=dict(pag_scale=3.0, pag_applied_layers=("mid", "up_blocks.1")))}


@pytest.mark.parametrize("case", list(LOOPS))
def test_host_loop_matches_restatement(monkeypatch, small_cpu, case):
    fake_ops.install(monkeypatch)
    cfg = LOOPS[case]
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(cfg["frames"], 170 + cfg["frames"])
    g, steps, win, fuse, schedule = cfg["guidance"], cfg["steps"], cfg.get("win", {}), cfg.get("fuse", "flat"), cfg.get("schedule", "uniform")
    if g <= 1.0:
        emb = emb[1:]
    two_m = cfg.get("sampler") == "2m"
    mk_rs = lambda: R.Restated(2, "dpmsolver++", "midpoint") if two_m else None
    pag = cfg.get("pag", {})
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _dpm() if two_m else _ddim())
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), steps, g, context_schedule=schedule, context_fuse=fuse, kv_downsample=cfg["kv"],
                       kv_downsample_mode=cfg["mode"], **win, **pag)
    n_win = len(FR.make_windows(schedule, cfg["frames"], **(win or dict(context_frames=30, context_stride=1, context_overlap=8))))
    assert n_win == (2 if win else 1)
    with torch.no_grad():
        kw = dict(guidance_scale=g, fuse=fuse, schedule=schedule, **win)
        if pag:
            kw.update(pag_scale=pag["pag_scale"], pag_layers=pag["pag_applied_layers"])
        want = T.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, kv_downsample=cfg["kv"], mode=cfg["mode"], scheduler=mk_rs(), **kw)
        plain = T.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, kv_downsample=1, scheduler=mk_rs(), **kw)
    e, c, d = rel_l2(out.float(), want), cosine(out.float(), want), rel_l2(plain, want)
    print(f"\nTODO_HOST_LOOP {case} rel_l2 {e:.3e} cos {c:.7f} (restated factor 1 vs {cfg['kv']}: {d:.3e})")
    assert torch.isfinite(out).all() and e < BOUND["rel"] and c > BOUND["cos"], (e, c)
    assert d > 0.0 and not torch.equal(out.float(), plain)


def test_restated_loop_with_factor_one_is_the_oracle_loop(small_cpu):
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 82)
    with torch.no_grad():
        want = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True)
        got = T.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, kv_downsample=(1, 1), guidance_scale=3.5)
        moved = T.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, kv_downsample=(2,), guidance_scale=3.5)
    assert torch.equal(got, want) and not torch.equal(moved, want)
    assert O.transformer_block_read.__module__ == "oracle.cpu_ref" and O.transformer_3d.__module__ == "oracle.cpu_ref"      # swapped back


# ---- 6. window parallelism: three gloo ranks
def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=521))
    kw = dict(context_frames=8, context_stride=1, context_overlap=2, kv_downsample=(2, 2))      # 3 windows, the last one wraps
    pipe = MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat, rl, emb, 2, 3.5, window_parallel=dp.WindowParallel(), **kw)
    got = dp.gather_latents(out)
    if rank == 0:
        one = pipe.denoise(lat, rl, emb, 2, 3.5, **kw)
        plain = pipe.denoise(lat, rl, emb, 2, 3.5, **dict(kw, kv_downsample=1))
        q.put(dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                   finite=bool(torch.isfinite(out).all()), pooled=not torch.equal(out, plain)))
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    res = run_world(3, _wp_worker)
    assert all(res.values()), res


# ---- 7. the script
def test_script_flags_parse():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.kv_downsample, a.kv_downsample_mode) == ((1,), "nearest")
    a = IV.parse_args(["--kv_downsample", "2"])
    assert (a.kv_downsample, a.kv_downsample_mode) == ((2,), "nearest")
    a = IV.parse_args(["--kv_downsample", "4,2", "--kv_downsample_mode", "mean"])
    assert (a.kv_downsample, a.kv_downsample_mode) == ((4, 2), "mean")
    for bad in (["--kv_downsample", "two"], ["--kv_downsample", "2,"], ["--kv_downsample_mode", "area"]):
        with pytest.raises(SystemExit):
            IV.parse_args(bad)
    assert "kv_downsample=--kv_downsample" in IV.__doc__


def test_script_flags_reach_denoise(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append((kw["kv_downsample"], kw["kv_downsample_mode"]))
        return latents

    build = fake_pipeline_builder(IV)

    def build_with_plan(*a, **kw):
        pipe = build(*a, **kw)
        pipe.denoising_unet.kv_downsample_plan = lambda factors, mode: None    # the stand-in UNet of the builder has no blocks to ask
        return pipe

    monkeypatch.setattr(IV, "build_pipeline", build_with_plan)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base)
    IV.main(base + ["--kv_downsample", "2"])
    IV.main(base + ["--kv_downsample", "2,2", "--kv_downsample_mode", "mean"])
    assert seen == [((1,), "nearest"), ((2,), "nearest"), ((2, 2), "mean")]
