"""CPU: host-side logic of the product package (no kernels): state-dict key layout vs the reference, window
scheduler, DDIM table, config handling."""
import json
import os

import pytest
import torch

import mikudance_amd as M
from mikudance_amd.selftest import MM_KWARGS, SCHED_KWARGS, SMALL
from oracle import cpu_ref as O


@pytest.mark.parametrize("name,geom", [("", {}), ("_small", SMALL)])
def test_state_dict_keys_match_reference(golden_dir, name, geom):
    gold = json.load(open(os.path.join(golden_dir, f"g6_state_dict_keys{name}.json")))
    with torch.device("meta"):
        den = M.UNet3DConditionModel(sample_size=16, **geom, **MM_KWARGS)
        ref = M.UNet2DConditionModel(sample_size=16, **geom)
    for m, g in ((den, gold["denoising_unet"]), (ref, gold["reference_unet"])):
        sd = {k: list(v.shape) for k, v in m.state_dict().items()}
        assert sd == g


def test_windows_match_reference(golden_dir):
    for case in json.load(open(os.path.join(golden_dir, "g1_windows.json"))):
        got = list(M.get_context_scheduler("uniform")(0, case["steps"], case["num_frames"], case["context_frames"], 1, case["overlap"]))
        assert got == case["windows"]
    with pytest.raises(ValueError):
        M.get_context_scheduler("nope")


def test_ddim_table_matches_oracle():
    s, o = M.DDIMScheduler(**SCHED_KWARGS), O.DDIM()
    assert torch.equal(s.alphas_cumprod, o.alphas_cumprod)
    for n in (4, 20, 30):
        s.set_timesteps(n); o.set_timesteps(n)
        assert torch.equal(s.timesteps, o.timesteps)
        for t in s.timesteps:
            assert s.step_coefficients(t) == o.coeffs(t)
    with pytest.raises(NotImplementedError):
        M.DDIMScheduler()                       # epsilon / leading defaults are not the MikuDance configuration


def test_reference_control_pairs_blocks_like_the_reference():
    with torch.device("meta"):
        den = M.UNet3DConditionModel(sample_size=16, **SMALL, **MM_KWARGS)
        ref = M.UNet2DConditionModel(sample_size=16, **SMALL)
    w = M.ReferenceAttentionControl(ref, mode="write", fusion_blocks="full")
    r = M.ReferenceAttentionControl(den, mode="read", do_classifier_free_guidance=True, fusion_blocks="full")
    names_r = {id(m): n for n, m in den.named_modules()}
    names_w = {id(m): n for n, m in ref.named_modules()}
    pr = [names_r[id(b)] for b in r._blocks(den)]
    pw = [names_w[id(b)] for b in w._blocks(ref)]
    assert pr == pw and len(pr) == 16
    assert [b.dim for b in r._blocks(den)] == [256] * 6 + [128] * 5 + [64] * 5
    assert pr[0].startswith("down_blocks.2") and pr[5].startswith("mid_block")


def test_unsupported_configs_fail_loudly():
    with pytest.raises(NotImplementedError):
        M.UNet3DConditionModel(use_linear_projection=True)
    with pytest.raises(RuntimeError):
        M.UNet3DConditionModel.from_pretrained_2d("/nonexistent", "/nonexistent.pth")


def test_scene_motion_matches_reference(golden_dir):
    import numpy as np
    from mikudance_amd.scene_motion import camera_to_scene_motion
    z = np.load(os.path.join(golden_dir, "g2_scene_motion.npz"))
    flow = camera_to_scene_motion(list(z["w2c"]), list(z["c2w"]), list(z["K"]), z["depth"], 24, 24, False)
    assert flow.shape == (16, 2, 24, 24) and np.abs(flow - z["flow"]).max() <= 1e-12
    eye = [np.eye(4)] * 5
    assert np.abs(camera_to_scene_motion(eye, eye, list(z["K"]), np.zeros((1, 24, 24)), 24, 24, False)).max() == 0


def test_hot_path_refuses_cpu_tensors_and_flags_odd_latents():
    from mikudance_amd.unet_3d_mix import _UNetBase
    with torch.device("meta"):
        den = M.UNet3DConditionModel(sample_size=16, **SMALL, **MM_KWARGS)
        ref = M.UNet2DConditionModel(sample_size=16, **SMALL)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    with pytest.raises(RuntimeError):
        pipe.denoise(torch.zeros(1, 4, 2, 16, 16), torch.zeros(1, 2, 22, 16, 16), torch.zeros(2, 5, 64), 1, 3.5)
    assert _UNetBase._needs_upsample_size(12, 16, 4)     # 12 is not a multiple of 8: the reference's upsample_size path
    assert _UNetBase._needs_upsample_size(90, 96, 4) and not _UNetBase._needs_upsample_size(96, 128, 4)
    with pytest.raises(AssertionError):
        den.forward(torch.zeros(1, 4, 16, 16), 0, torch.zeros(1, 5, 64))       # 5-D input required (transformer_3d.py:117-119)


def test_zero_context_detection_and_pe_fold_tables():
    """Host-side logic of two result-preserving shortcuts (no kernels involved): which leading frames have an all-zero
    context (cross-attention == to_out bias there), and the per-frame row term pe @ Wq^T that replaces the query-only
    positional-encoding add of the motion module (reference src/models/motion_module.py:416-417)."""
    import torch
    from mikudance_amd import UNet3DConditionModel
    from mikudance_amd.blocks import MotionModule
    from mikudance_amd.selftest import MM_KWARGS, SMALL
    den = UNet3DConditionModel(sample_size=16, **SMALL, **MM_KWARGS)
    ctx = torch.zeros(2, 5, 64)
    ctx[1] = torch.randn(5, 64)
    assert den._cross(ctx, [0] * 3 + [1] * 3, "cpu").zero_frames == 3                 # [uncond x3 | cond x3]
    assert den._cross(ctx, [1, 0, 1, 0], "cpu").zero_frames == 0                      # interleaved: no leading run
    assert den._cross(ctx.flip(0), [0] * 3 + [1] * 3, "cpu").zero_frames == 0
    assert den._cross(torch.zeros(2, 5, 64), [0, 0, 1, 1], "cpu").zero_frames == 4
    mm = MotionModule(64, max_len=32).float()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for prm in mm.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
    pk = mm._pack(torch.device("cpu"))
    ab = mm.temporal_transformer.transformer_blocks[0].attention_blocks[1]
    want = ab.pos_encoder.pe[0].float() @ ab.to_q.weight.float().t()
    assert tuple(pk["peq1"].shape) == (32, 192) and float(pk["peq1"][:, 64:].abs().max()) == 0.0
    assert torch.allclose(pk["peq1"][:, :64].float(), want, atol=2e-3, rtol=2e-3)
    assert torch.equal(pk["qkv1"].float()[64:128], ab.to_k.weight.half().float())


def test_cross_context_cache_never_matches_by_address_alone():
    """a freed context tensor's address is re-used by the next clip's tokens (same shape, _version 0).
    The cache entry owns its source tensor, so that cannot produce a stale hit (runs on CPU: `_cross` is host logic)."""
    with torch.device("meta"):
        den = M.UNet3DConditionModel(sample_size=16, **SMALL, **MM_KWARGS)
    idx = [0, 0, 1, 1]
    for trial in range(50):
        x = torch.cat([torch.zeros(1, 5, 64), torch.randn(1, 5, 64)], 0)
        hit = den._cross(x, idx, "cpu")
        assert torch.equal(hit.ctx.view(2, 8, 64)[:, :5].float(), x.half().float())
        assert hit.zero_frames == 2 and den._cross(x, idx, "cpu") is hit and den._cross(x[:2], idx, "cpu") is hit
        del x, hit
    x = torch.randn(2, 5, 64)
    h1 = den._cross(x, idx, "cpu")
    x.add_(1.0)
    assert den._cross(x, idx, "cpu") is not h1
    den.clear_context_cache()
    assert not den._cross_cache


def test_window_layout_rejects_non_advancing_windows():
    with pytest.raises(ValueError):
        list(M.get_context_scheduler("uniform")(0, 20, 48, 30, 1, 30))
    with pytest.raises(ValueError):
        list(M.get_context_scheduler("uniform")(0, 20, 48, 8, 1, 12))
    assert list(M.get_context_scheduler("uniform")(0, 20, 4, 8, 1, 12)) == [[0, 1, 2, 3]]     # one window: overlap unused


def test_clip_tower_key_layout_and_preprocess_match_transformers(golden_dir):
    """The CLIP tower's state-dict keys == transformers' CLIPVisionModelWithProjection's (pinned in g11_meta.json by the
    generator, which built the third-party model), and clip_preprocess == CLIPImageProcessor defaults (constants restated)."""
    import numpy as np
    from PIL import Image
    meta = json.load(open(os.path.join(golden_dir, "g11_meta.json")))["small"]
    with torch.device("meta"):
        m = M.CLIPVisionModelWithProjection(meta["config"])
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == meta["keys"]
    img = Image.fromarray(np.random.default_rng(0).integers(0, 255, (224, 224, 3), dtype=np.uint8))
    px = M.clip_preprocess(img)
    a = np.asarray(img).astype(np.float64) / 255.0
    want = (a - np.array([0.48145466, 0.4578275, 0.40821073])) / np.array([0.26862954, 0.26130258, 0.27577711])
    assert tuple(px.shape) == (1, 3, 224, 224) and np.abs(px[0].permute(1, 2, 0).numpy() - want).max() < 1e-5
    assert tuple(M.clip_preprocess(img.resize((300, 260))).shape) == (1, 3, 224, 224)
    with pytest.raises(NotImplementedError):
        M.CLIPVisionModelWithProjection(dict(meta["config"], hidden_act="gelu"))


def test_gemm_and_conv_dispatch_table_of_the_benchmark_shapes():
    """The automatic kernel choice for every MFMA-bound launch shape of configs[1] (768 x 768, 16 frames, CFG: 32-frame batches), as
    measured best on MI355X in same-box A/B runs (profiles/r03_ab_gemm_sp_tiles.log, r03_ab_gemm_sp_tile_128x256.log,
    r03_ab_transposed_sp.log).  md_gemm_plan / md_conv3x3_plan run the launcher's own decision code without
    touching a device: 135 / 134 / 124 / 132 / 142 = gemm_sp_kernel 192x320 / 192x256 / 128x256 / 192x128 / 256x128, 144 = its 256x256 GEGLU flavour, +1000 on
    swapped operands (transposed output), +2000 when a residual enters through the matrix core (round 6: K tiles > sub-tiles of the wave tile -- FF-out, the
    K >= 1280 out-projections, a resnet's second conv; short K keeps the epilogue form: 135), 210 / 220 / 230 = W-stationary streaming kernel, 301 / 303 = multi-workgroup kernel."""
    from mikudance_amd import _lib, ops
    lib = _lib.load()
    ncu, G = 256, ops.ACT_GEGLU
    gemm = {
        # level 0 (96 x 96): HBM-bound projections and the K = 320 GEGLU stream; FF-out on the big tile
        (294912, 320, 320, 0, 0, 5): 210, (294912, 960, 320, 0, 0, 0): 210, (294912, 2560, 320, G, 0, 4): 230, (294912, 320, 1280, 0, 0, 5): 2135,
        # level 1 (48 x 48)
        (73728, 640, 640, 0, 0, 5): 220, (73728, 5120, 640, G, 0, 4): 144, (73728, 640, 2560, 0, 0, 5): 2135,
        # level 2 (24 x 24): N = 1280 takes the 192 x 256 tile (480 tiles = 1.9 rounds instead of 384 = 1.5)
        (18432, 1280, 1280, 0, 0, 5): 2134, (18432, 10240, 1280, G, 0, 4): 144, (18432, 1280, 5120, 0, 0, 5): 2134, (18432, 3840, 1280, 0, 0, 0): 135,
        (18432, 2560, 1280, 0, 0, 0): 135,
        # level 3 (12 x 12): N = 1280 on 192 x 128 tiles (24 x 10 = 240 of them fill 256 CUs; 128 x 256 gives 180): +14..16 % same-box
        # (profiles/r04_ab_tile_192x128.log); the wider N keep the 192 x 256 tile
        (4608, 1280, 1280, 0, 0, 5): 2132, (4608, 10240, 1280, G, 0, 4): 144, (4608, 1280, 5120, 0, 0, 5): 2132, (4608, 2560, 1280, 0, 0, 0): 134,
        (4608, 3840, 1280, 0, 0, 0): 134,
        # V^T projections (transposed output): swapped operands
        (294912, 320, 320, 0, 1, 0): 1134, (73728, 640, 640, 0, 1, 0): 1124, (18432, 1280, 1280, 0, 1, 0): 1134, (4608, 1280, 1280, 0, 1, 0): 1124,
        # not sp: ragged / tiny N, few tiles
        (257 * 32, 768, 320, 0, 0, 4): 303, (294912, 4, 320, 0, 0, 4): 301, (2048, 320, 1280, 0, 0, 4): 303,
    }
    for args, want in gemm.items():
        assert lib.md_gemm_plan(*args, ncu) == want, (args, lib.md_gemm_plan(*args, ncu), want)
    conv = {  # (B, H = W, Cin, Cout, stride, upsample)
        (32, 96, 320, 320, 1, 0): 135, (32, 96, 640, 320, 1, 0): 135, (32, 96, 960, 320, 1, 0): 135, (32, 48, 640, 640, 1, 0): 135,
        (32, 48, 1920, 640, 1, 0): 135, (32, 24, 1280, 1280, 1, 0): 134, (32, 24, 2560, 1280, 1, 0): 134, (32, 12, 1280, 1280, 1, 0): 132,
        (32, 12, 2560, 1280, 1, 0): 132, (32, 48, 640, 640, 1, 1): 135, (32, 24, 1280, 1280, 1, 1): 135, (32, 12, 1280, 1280, 1, 1): 134,
        (32, 96, 320, 320, 2, 0): 135, (32, 48, 640, 640, 2, 0): 135, (32, 24, 1280, 1280, 2, 0): 132, (32, 96, 320, 4, 1, 0): 301,
        (2, 8, 64, 320, 1, 0): 303,
        # AutoencoderKL at 768 x 768, 8 images per call: the 128-channel layers (N % 128 only) on the 256 x 128 tile, 256 channels on 192 x 256
        (8, 768, 64, 128, 1, 0): 142, (8, 768, 128, 128, 1, 0): 142, (8, 384, 128, 256, 1, 0): 134, (8, 384, 256, 256, 1, 0): 134,
    }
    for (B, H, cin, cout, st, up), want in conv.items():
        got = lib.md_conv3x3_plan(B, H, H, cin, cout, st, up, 4, ncu)
        assert got == want, ((B, H, cin, cout, st, up), got, want)
    # a resnet's second conv (bias + shortcut): the residual through the matrix core; K = 640 with a residual (10 K tiles < 15 sub-tiles): the epilogue form
    assert lib.md_conv3x3_plan(32, 96, 96, 320, 320, 1, 0, 5, ncu) == 2135 and lib.md_conv3x3_plan(32, 24, 24, 1280, 1280, 1, 0, 5, ncu) == 2134
    assert lib.md_gemm_plan(294912, 320, 640, 0, 0, 5, ncu) == 135 and lib.md_gemm_plan(294912, 320, 960, 0, 0, 5, ncu) == 135
    # argument errors are reported, not guessed around
    assert lib.md_gemm_plan(128, 320, 100, 0, 0, 0, ncu) < 0 and lib.md_conv3x3_plan(1, 8, 8, 60, 320, 1, 0, 0, ncu) < 0
    # configs[4]: 983 040 tokens.  K = 1280 makes A 2.5 GB, beyond the sp kernel's 2^31-byte reach: planned (and launched) in row blocks
    assert lib.md_gemm_plan(983040, 320, 1280, 0, 0, 5, ncu) == 2135 and lib.md_gemm_plan(983040, 320, 320, 0, 0, 5, ncu) == 210
    assert lib.md_conv3x3_plan(60, 128, 128, 960, 320, 1, 0, 4, ncu) == 135
    # a smaller chip changes the rounds, hence the tile: the model is per device
    assert lib.md_gemm_plan(18432, 1280, 1280, 0, 0, 5, 192) in (2134, 2135, 2124)


def _gemm_and_conv_plans_over_the_grid(lib):
    """Every code md_gemm_plan / md_conv3x3_plan return over the grid below, one flat list per query in iteration order."""
    from itertools import product
    from mikudance_amd import ops
    ncus = (256, 192, 64)
    gemm = [lib.md_gemm_plan(M_, N, K, act, tr, epi, ncu)
            for M_, N, K, act, tr, epi, ncu in product(
                (4608, 18432, 294912, 983040), (4, 128, 320, 1280, 10240),
                (64, 100, 128, 320, 640, 1280, 2560, 5120), (ops.ACT_NONE, ops.ACT_GEGLU), (0, 1), range(8), ncus)]
    pairs = ((320, 320), (640, 320), (960, 320), (640, 640), (1920, 640), (1280, 1280), (2560, 1280), (320, 4), (64, 320), (64, 128),
             (128, 128), (128, 256), (256, 256), (60, 320))
    conv = [lib.md_conv3x3_plan(B, H, H, cin, cout, st, up, epi, ncu)
            for B, H, (cin, cout), st, up, epi, ncu in product(
                (2, 32), (12, 24, 96, 768), pairs, (1, 2), (0, 1), (0, 4, 5, 7), ncus)]
    return {"gemm": gemm, "conv": conv}


def test_gemm_and_conv_dispatch_over_a_grid_matches_the_recording(golden_dir):
    """The decisions of the GEMM / 3x3-conv dispatch (gemm.hip gemm_choose, through md_gemm_plan / md_conv3x3_plan: no device touched) over a
    grid of 15 360 GEMM and 5 376 conv problems on 256, 192 and 64 compute units: every K, activation, output form, epilogue and (Cin, Cout)
    pair of the wider grid that profiles/gemm_dispatch_refactor.log compared once (10 M x 13 N; 5 B x 8 H), with M, N, B and H thinned to
    the levels of the clip (12 x 12, 24 x 24, 96 x 96, the 983 040-token matrix that runs in row blocks) so that the recording stays
    readable in a diff.  The recording was taken at the last commit whose dispatcher decided and launched in one function (the one before gemm_choose), with

        from mikudance_amd import _lib; from tests.test_host_cpu import _gemm_and_conv_plans_over_the_grid as grid
        g = grid(_lib.load()); rows = lambda v, n: ",\n".join(",".join(map(str, v[i:i + n])) for i in range(0, len(v), n))
        open("tests/golden/gemm_plans.json", "w").write('{"gemm":[\n%s],\n"conv":[\n%s]}\n' % (rows(g["gemm"], 96), rows(g["conv"], 96)))

    and holds every code the table above names plus 302 and the argument error: a change of a rule, a tie-break or a tile's row shows here
    as the first problem that moved.  Record again only with a measurement that justifies the new decision."""
    from mikudance_amd import _lib
    want = json.load(open(os.path.join(golden_dir, "gemm_plans.json")))
    got = _gemm_and_conv_plans_over_the_grid(_lib.load())
    assert len(want["gemm"]) == 15360 and len(want["conv"]) == 5376
    for q in ("gemm", "conv"):
        assert len(got[q]) == len(want[q])
        moved = [i for i, (g, w) in enumerate(zip(got[q], want[q])) if g != w]
        assert not moved, (q, len(moved), "first at flat index", moved[0], "got", got[q][moved[0]], "recorded", want[q][moved[0]])
    seen = set(want["gemm"]) | set(want["conv"])
    assert {135, 134, 124, 132, 142, 144, 1124, 1134, 2135, 2134, 2132, 210, 220, 230, 301, 302, 303} <= seen and min(seen) < 0


class _PlanCall:
    """md_gemm_plan_call / md_conv_plan_call on made-up operand ADDRESSES (the queries read pointer values and pitches, never memory): every
    operand 2^40 bytes from the next, so none overlaps another at any size of the grid."""
    A, W, C, BIAS, RES, RADD = (i << 40 for i in range(1, 7))

    def __init__(self):
        from mikudance_amd import _lib
        self.lib = _lib.load()
        assert self.lib.md_set_cu_limit(0) == 0
        assert not os.environ.get("MD_GEMM_SP") and not os.environ.get("MD_GEMM_SP_NT"), "the dispatch tests assume the default knobs"

    def gemm(self, M, N, K, act=0, tr=0, epi=0, A=None, lda=None, C=None, ldc=None, res=None, ldr=None, radd=None, ldra=None, rpg=None, blocks=None):
        ldc = ldc if ldc is not None else (M if tr else (N // 2 if act == 3 else N))
        return self.lib.md_gemm_plan_call(A or self.A, K if lda is None else lda, self.W, C or self.C, ldc, M, N, K, self.BIAS if epi & 4 else None,
                                          res or (self.RES if epi & 1 else None), N if ldr is None else ldr,
                                          radd or (self.RADD if epi & 2 else None), N if ldra is None else ldra, M if rpg is None else rpg, act, tr,
                                          blocks[0] if blocks else None, blocks[1] if blocks else None)

    def conv(self, B, H, cin, cout, st=1, up=0, epi=0, act=0, kw=3, pad_lo=1, ldx=None, Y=None, ldy=None, res=None, ldr=None, Wd=None):
        Wd = Wd or H
        return self.lib.md_conv_plan_call(self.A, cin if ldx is None else ldx, self.W, Y or self.C, cout if ldy is None else ldy, B, H, Wd, cin, cout, kw,
                                          st, up, pad_lo, self.BIAS if epi & 4 else None, res or (self.RES if epi & 1 else None),
                                          cout if ldr is None else ldr, self.RADD if epi & 2 else None, cout, ((H << up) // st) * ((Wd << up) // st), act)


def test_plan_of_the_call_agrees_with_the_table_query_on_dense_aligned_operands(golden_dir):
    """md_gemm_plan_call / md_conv_plan_call run launch_gemm's own checks, knobs and gemm_choose (gemm.hip gemm_plan_checked).  On dense,
    16-byte aligned operands with the default knobs they answer what md_gemm_plan / md_conv3x3_plan answer over the grid of
    tests/golden/gemm_plans.json at 256 compute units (the count without a device, and the MI355X's own) -- except where the LAUNCH refuses the
    call, which the table query never modelled: GEGLU with N % 64, a residual, a row term or a transposed store; a transposed store with a
    residual or a row term.  There the call query is negative."""
    from itertools import product
    from mikudance_amd import ops
    q = _PlanCall()
    lib, G = q.lib, ops.ACT_GEGLU
    want = json.load(open(os.path.join(golden_dir, "gemm_plans.json")))
    n = refused = 0
    for i, (M_, N, K, act, tr, epi, ncu) in enumerate(product((4608, 18432, 294912, 983040), (4, 128, 320, 1280, 10240),
                                                              (64, 100, 128, 320, 640, 1280, 2560, 5120), (ops.ACT_NONE, G), (0, 1), range(8), (256, 192, 64))):
        if ncu != 256:
            continue
        got = q.gemm(M_, N, K, act, tr, epi)
        refuse = K % 64 != 0 or (act == G and (N % 64 != 0 or tr or epi & 3)) or (tr and epi & 3)
        if refuse:
            assert got < 0, ((M_, N, K, act, tr, epi), got)
            refused += 1
        else:
            assert got == want["gemm"][i] == lib.md_gemm_plan(M_, N, K, act, tr, epi, 256), ((M_, N, K, act, tr, epi), got, want["gemm"][i])
        n += 1
    assert n == 5120 and 0 < refused < n
    pairs = ((320, 320), (640, 320), (960, 320), (640, 640), (1920, 640), (1280, 1280), (2560, 1280), (320, 4), (64, 320), (64, 128),
             (128, 128), (128, 256), (256, 256), (60, 320))
    n = 0
    for i, (B, H, (cin, cout), st, up, epi, ncu) in enumerate(product((2, 32), (12, 24, 96, 768), pairs, (1, 2), (0, 1), (0, 4, 5, 7), (256, 192, 64))):
        if ncu != 256:
            continue
        got = q.conv(B, H, cin, cout, st, up, epi)
        assert got == want["conv"][i], ((B, H, cin, cout, st, up, epi), got, want["conv"][i])
        n += 1
    assert n == 1792
    # row blocks: 983 040 x 1280 fp16 is beyond the sp kernel's 2^31-byte reach
    import ctypes
    nb, tail = ctypes.c_int(0), ctypes.c_int(0)
    assert q.gemm(983040, 320, 1280, epi=5, blocks=(ctypes.byref(nb), ctypes.byref(tail))) == 2135 and nb.value == 2 and tail.value == 2135
    assert q.gemm(4608, 1280, 1280, epi=5, blocks=(ctypes.byref(nb), ctypes.byref(tail))) == 2132 and nb.value == 1 and tail.value == 2132


def test_plan_of_the_call_sees_alignment_pitches_activation_and_the_cu_limit():
    """One reason at a time moves an sp-eligible problem to gemm_kernel (30x): what md_gemm_plan cannot be asked."""
    q = _PlanCall()
    assert q.gemm(18432, 1280, 1280, epi=5) == 2134 and q.gemm(18432, 1280, 640, epi=4) == 134
    assert q.gemm(18432, 1280, 1280, epi=5, C=q.C + 8) == 303                      # output base 8 bytes off a 16-byte boundary
    assert q.gemm(18432, 1280, 1280, epi=5, ldc=1284) == 303                       # ldc % 8 == 4
    assert q.gemm(18432, 1280, 1280, epi=5, res=q.RES + 8) == 303                  # misaligned residual
    assert q.gemm(18432, 1280, 1280, epi=5, ldr=1284) == 303                       # residual pitch
    assert q.gemm(18432, 1280, 1280, epi=6, radd=q.RADD + 8) == 303                # misaligned row term
    assert q.gemm(18432, 1280, 1280, epi=4, act=1) == 303 and q.gemm(18432, 1280, 1280, epi=4, act=2) == 303      # SiLU / ReLU
    assert q.gemm(18432, 1280, 1280, epi=4, lda=1280 + 64) == 134 and q.gemm(18432, 1280, 1280, epi=5, C=q.RES, ldr=1280) == 2134    # slices and in place stay
    assert q.gemm(294912, 320, 320, epi=5) == 210 and q.gemm(294912, 320, 320, epi=5, C=q.C + 8) == 303
    assert q.gemm(294912 + 8, 320, 320, epi=5) == 303                              # M % 16: not the streaming kernel, K < 640: not sp
    assert q.conv(32, 96, 320, 320, epi=5) == 2135 and q.conv(32, 96, 320, 320, epi=4) == 135
    assert q.conv(32, 96, 320, 320, epi=4, act=1) == 302 and q.conv(32, 96, 320, 320, epi=4, act=2) == 302       # an activation on a conv
    assert q.conv(32, 24, 1280, 1280, epi=4, act=1) == 303
    assert q.conv(32, 96, 320, 320, epi=4, ldy=321) == 302 and q.conv(32, 96, 320, 320, epi=4, Y=q.C + 8) == 302  # odd output pitch / base
    assert q.conv(32, 96, 320, 320, epi=5, res=q.RES + 8) == 302
    assert q.conv(32, 96, 320, 320, epi=4, ldx=640) == 135 and q.conv(32, 96, 320, 320, st=2, pad_lo=0, epi=4) == 135
    assert q.conv(2, 16, 128, 128, kw=1, epi=4, Wd=4096) == 142
    # md_set_cu_limit is honoured: on 8 CUs the 480 tiles of 192 x 256 are 60 rounds of 29.6 us, the 384 of 192 x 320 are 48 of 35.2 us
    try:
        assert q.lib.md_set_cu_limit(8) == 0
        assert q.gemm(18432, 1280, 1280, epi=5) == 2135
    finally:
        assert q.lib.md_set_cu_limit(0) == 0
    assert q.gemm(18432, 1280, 1280, epi=5) == 2134


def test_plan_of_the_call_returns_every_refusal_of_the_launch():
    q = _PlanCall()
    G = 3
    assert q.gemm(18432, 1280, 1280) > 0
    assert q.gemm(18432, 1280, 1200) < 0 and q.gemm(18432, 1280, 0) < 0 and q.gemm(0, 1280, 1280) < 0            # bad K, empty problem
    assert q.gemm(18432, 1280, 1280, A=q.A + 8) < 0 and q.gemm(18432, 1280, 1280, lda=1284) < 0                   # A alignment / pitch
    assert q.gemm(18432, 2560, 1280, act=G, epi=4) == 144
    assert q.gemm(18432, 2560, 1280, act=G, epi=5) < 0 and q.gemm(18432, 2560, 1280, act=G, epi=6) < 0            # GEGLU with a residual / row term
    assert q.gemm(18432, 2560, 1280, act=G, tr=1) < 0 and q.gemm(18432, 2528, 1280, act=G) < 0                    # GEGLU transposed / N % 64
    assert q.gemm(18432, 2560, 1280, act=G, C=q.C + 8) < 0 and q.gemm(18432, 2560, 1280, act=G, ldc=1284) < 0
    assert q.gemm(18432, 1280, 1280, tr=1, epi=4) == 1134
    assert q.gemm(18432, 1280, 1280, tr=1, epi=6) < 0 and q.gemm(18432, 1280, 1280, tr=1, epi=5) < 0              # transposed with a row term / residual
    assert q.gemm(18432, 1280, 1280, tr=1, act=1) < 0
    assert q.gemm(18432, 1280, 1280, epi=2, rpg=0) < 0                                                            # row term without rows_per_group
    # an activation the kernels do not know would run as "none": 4 (QuickGELU) is the last one, GEGLU has no conv form
    assert q.gemm(18432, 1280, 1280, epi=4, act=4) == 303 and q.gemm(18432, 1280, 1280, epi=5, act=4) == 303
    assert q.gemm(18432, 1280, 1280, act=5) == -1 and q.gemm(18432, 1280, 1280, act=-1) == -1 and q.gemm(18432, 1280, 1280, act=1 << 16) == -1
    assert b"act=" in q.lib.md_last_error()
    assert q.conv(32, 96, 320, 320, epi=4, act=4) == 302 and q.conv(32, 96, 320, 320, act=5) == -1 and q.conv(32, 96, 320, 320, act=-1) == -1
    assert q.conv(32, 96, 320, 320, act=G) == -1 and b"act=3" in q.lib.md_last_error()
    assert q.gemm(18432, 1280, 1280, epi=1, res=q.C + 2 * 1280 * 10) < 0                                          # residual ten rows into the output
    assert q.gemm(18432, 1280, 1280, epi=1, res=q.C + 2 * 640, ldc=2560, ldr=2560) < 0                            # sibling slices that share columns
    assert q.gemm(18432, 1280, 1280, epi=1, res=q.C + 2 * 1280, ldc=2560, ldr=2560) == 2134                       # sibling slices that do not
    assert q.gemm(18432, 1280, 1280, epi=1, C=q.RES, ldc=1280, ldr=1288) < 0                                      # in place with another pitch
    assert q.conv(32, 96, 60, 320) < 0 and q.conv(32, 96, 64, 320, ldx=60) < 0 and q.conv(32, 96, 64, 320, ldx=68) < 0
    assert q.conv(32, 96, 64, 320, st=3) < 0 and q.conv(32, 96, 64, 320, st=2, up=1) < 0 and q.conv(32, 96, 64, 320, pad_lo=0) < 0
    assert q.conv(32, 96, 64, 320, kw=1, st=2) < 0 and q.conv(32, 96, 64, 320, kw=2) < 0
    assert q.conv(1, 4096, 64, 320, Wd=4096) < 0                                                                  # 2^24 pixels: the tap arithmetic
    assert q.conv(32, 96, 320, 320, epi=1, res=q.C + 2 * 320 * 10) < 0
    assert b"overlaps" in q.lib.md_last_error()


def test_attention_dispatch_table():
    """md_attention_plan runs the decision code of md_attention_fwd_f16 (launch_attn / launch_attn2 / attn2s_eligible) without touching a
    device: 400 = generic attn_kernel, 414 / 418 = attn2 DMA ring with 4 / 8 waves, 420 = attn2s (K / V^T resident in LDS).  Pinned: the
    shapes of BASELINE configs[1] (profiles/r02_ab_attention_*.log, r03_ab_attention_small.log) and both sides of every threshold, so that a
    change of a threshold shows here and in the flavour each case of tests/test_attention_flavours_gpu.py states."""
    from mikudance_amd import _lib
    plan = _lib.load().md_attention_plan
    GENERIC, RING4, RING8, RESIDENT = 400, 414, 418, 420
    table = {  # (D, Lq, Lk, kv_stride, ldvt, vt_align16)
        # configs[1], 32-frame batches: self-attention at the 96 x 96 / 48 x 48 / 24 x 24 levels (ldvt = every token of the batch)
        (40, 9216, 9216, 9216, 32 * 9216, 1): RING8, (80, 2304, 2304, 2304, 32 * 2304, 1): RING4, (160, 576, 576, 576, 32 * 576, 1): RING4,
        # cross-attention: 257 CLIP tokens, two context batches padded to a stride of 264
        (40, 9216, 257, 264, 528, 1): RESIDENT, (80, 2304, 257, 264, 528, 1): RING4, (160, 576, 257, 264, 528, 1): RING4,
        # Lq 1023 | 1024: 8 waves from 1024 on at D <= 40 only
        (40, 1023, 1024, 1024, 1024, 1): RING4, (40, 1024, 1024, 1024, 1024, 1): RING8,
        (80, 1023, 1024, 1024, 1024, 1): RING4, (80, 1024, 1024, 1024, 1024, 1): RING4,
        (8, 1024, 1024, 1024, 1024, 1): RING8, (16, 1023, 1024, 1024, 1024, 1): RING4, (32, 1024, 64, 64, 64, 1): RING8, (64, 4096, 64, 64, 64, 1): RING4,
        # Lq 2047 | 2048 with the cross-attention keys: residency needs the long query side
        (40, 2047, 257, 264, 528, 1): RING8, (40, 2048, 257, 264, 528, 1): RESIDENT,
        # Lk 320 | 328: a key tile of attn2s is STAGE = 64 * 40 * 2 + 2 * 32 * 128 = 13312 bytes of LDS; five tiles + the 2576 bytes of the folded
        # constants are 69136 <= 72 KiB, six are 82448: at most 5 tiles = 320 keys stay resident
        (40, 2048, 320, 320, 320, 1): RESIDENT, (40, 2048, 321, 328, 328, 1): RING8, (40, 2048, 328, 328, 328, 1): RING8,
        (40, 9216, 384, 384, 384, 1): RING8,
        # Lk = 8 | Lk < 8: the clamped V^T load of attn2s needs one whole 8-key chunk
        (40, 2048, 8, 8, 8, 1): RESIDENT, (40, 2048, 7, 8, 8, 1): RING8, (40, 2048, 1, 8, 8, 1): RING8,
        # resident at D = 40 only
        (8, 4096, 257, 264, 528, 1): RING8, (32, 4096, 257, 264, 528, 1): RING8, (80, 4096, 257, 264, 528, 1): RING4,
        # not "fast", one reason at a time: ldvt % 8, kv_stride % 8 (Lk = 256 keeps roundup8(Lk) <= kv_stride), V^T not 16-byte aligned
        (40, 2048, 257, 264, 532, 1): GENERIC, (40, 2048, 256, 260, 520, 1): GENERIC, (40, 2048, 257, 264, 528, 0): GENERIC,
        (80, 100, 257, 264, 532, 1): GENERIC, (160, 1024, 256, 260, 520, 1): GENERIC, (8, 2048, 257, 264, 528, 0): GENERIC,
        # the fourth, roundup8(Lk) > kv_stride, cannot stand alone: kv_stride % 8 == 0 and kv_stride >= Lk (checked before) imply
        # kv_stride >= roundup8(Lk).  With the smallest stride that misses the pad it comes with kv_stride % 8:
        (40, 2048, 257, 260, 520, 1): GENERIC, (40, 2048, 257, 257, 520, 1): GENERIC, (40, 200, 333, 333, 666, 1): GENERIC,
    }
    for args, want in table.items():
        assert plan(*args) == want, (args, plan(*args), want)
    # errors are reported, not guessed around: unsupported head dims, empty problems, kv_stride < Lk
    for args in [(24, 2048, 257, 264, 528, 1), (48, 64, 64, 64, 64, 1), (0, 64, 64, 64, 64, 1), (320, 64, 64, 64, 64, 1),
                 (40, 0, 64, 64, 64, 1), (40, 64, 0, 64, 64, 1), (40, 2048, 257, 256, 528, 1)]:
        assert plan(*args) < 0, (args, plan(*args))


def test_fused_normalisation_plans_are_the_measured_table():
    """md_gemm_ln_plan / md_gemm_affine_plan (no device touched): the fused normalisations exist exactly where they won their same-box A/B
    (profiles/r05_ab_fused_norms*.log) -- K = 320, plain epilogue, N a multiple of 320, >= 32768 rows in whole 16-row tiles -- and nowhere
    else; the host (blocks.ln_linear / gn_linear) runs the literal operator pair wherever a plan says no."""
    from mikudance_amd import _lib
    lib = _lib.load()
    ACT_NONE, ACT_GEGLU = 0, 3
    yes = [(294912, 960, 320, 2), (294912, 320, 320, 0), (147456, 320, 320, 0), (983040, 960, 320, 2), (32768, 640, 320, 0), (32784, 320, 320, 0)]
    for M, N, K, epi in yes:
        assert lib.md_gemm_ln_plan(M, N, K, ACT_NONE, epi) == 1, (M, N, K, epi)
    no = [(294912, 2560, 320, ACT_GEGLU, 0),          # GEGLU: memory waves VALU bound (and the fold costs the consumer its warm input)
          (73728, 1920, 640, ACT_NONE, 2), (73728, 640, 640, ACT_NONE, 0),    # K = 640: loader waves' work redone per column group
          (18432, 1280, 1280, ACT_NONE, 0), (4608, 1280, 1280, ACT_NONE, 0),  # not streaming-kernel shapes
          (16384, 320, 320, ACT_NONE, 0), (32776, 320, 320, ACT_NONE, 0),     # too few rows / not whole tiles
          (294912, 320, 320, ACT_NONE, 1), (294912, 256, 320, ACT_NONE, 0), (294912, 2880, 320, ACT_NONE, 0)]   # residual; N not k x 320; > 8 groups
    for M, N, K, act, epi in no:
        assert lib.md_gemm_ln_plan(M, N, K, act, epi) == 0, (M, N, K, act, epi)
    assert lib.md_gemm_affine_plan(294912, 320, 320, 9216) == 1 and lib.md_gemm_affine_plan(983040, 320, 320, 16384) == 1
    assert lib.md_gemm_affine_plan(73728, 640, 320, 9216) == 1                      # two column groups
    for M, N, K, rpi in [(73728, 640, 640, 2304), (294912, 320, 320, 9216 + 8), (294912, 320, 320, 9000), (294912, 320, 320, 0), (16384, 320, 320, 1024),
                         (18432, 1280, 1280, 576)]:
        assert lib.md_gemm_affine_plan(M, N, K, rpi) == 0, (M, N, K, rpi)


def test_ln_fold_algebra_and_row_mean_insensitivity():
    """packing.ln_fold: LN(x) @ W^T + bias == rstd * (x @ Wf^T - mu * s) + c.  With the fp16-rounded Wf the identity holds to the rounding
    of gamma * W (2^-11 per weight); with s summed from the ROUNDED Wf the mean term cancels exactly, so shifting every row by 1000 sigma
    changes nothing but fp64 noise -- and the GEGLU row interleave commutes with the fold."""
    import torch
    from mikudance_amd import packing
    g = torch.Generator().manual_seed(3)
    M, N, K = 64, 96, 320
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    bias = (torch.randn(N, generator=g) * 0.2).half()
    gamma = (1 + 0.2 * torch.randn(K, generator=g)).half()
    beta = (0.3 * torch.randn(K, generator=g)).half()
    wf, sc = packing.ln_fold(w, bias, gamma, beta)
    assert wf.dtype == torch.float16 and sc.dtype == torch.float32 and sc.shape == (2, N)
    assert torch.equal(sc[0].double(), wf.double().sum(1).float().double())                      # s is the sum of the ROUNDED weights
    def folded(xx):
        mu = xx.mean(1, keepdim=True)
        rstd = torch.rsqrt(((xx - mu) ** 2).mean(1, keepdim=True) + 1e-5)
        return rstd * (xx @ wf.double().t() - mu * wf.double().sum(1)) + sc[1].double()
    ref = torch.nn.functional.layer_norm(x, (K,), gamma.double(), beta.double(), 1e-5) @ w.double().t() + bias.double()
    assert (folded(x) - ref).abs().max() < 2e-3 * ref.abs().max()                                # rounding of gamma * W to fp16
    assert (folded(x + 1000.0) - folded(x)).abs().max() < 1e-7 * ref.abs().max()                 # (x - mu) . Wf: the mean never reaches the sum
    wp2, bp2 = packing.geglu_weight(torch.cat([w, w[:32]]), torch.cat([bias, bias[:32]]), "cpu")
    wf2, sc2 = packing.ln_fold(wp2, bp2, gamma, beta)
    wf3, sc3 = packing.ln_fold(torch.cat([w, w[:32]]), torch.cat([bias, bias[:32]]), gamma, beta)
    wp3, cp3 = packing.geglu_weight(wf3, sc3[1], "cpu")
    assert torch.equal(wf2, wp3) and torch.allclose(sc2[1], cp3.float(), atol=1e-3)              # interleave(fold) == fold(interleave)
