"""GPU: smoothed-energy guidance on the MI355X -- ops.token_blur (md_token_blur_f16 / md_token_mean_f16) against the float64 definition of
tests/seg_ref.py, its exact cases and safety properties, one TransformerBlock with blurred queries, the loop against the restated loop at reduced
width, and the drop-in script with --seg_scale.  Bounds: per element half an fp16 ulp of the reference + 4 x the largest error of the float32
restatement (the rule of tests/test_free_init_gpu.py), the operator bound of tests/test_blocks_gpu.py, the loop bound rel-L2 <= 3e-2 and
cosine >= 0.999.  profiles/seg_tests.log holds every printed figure of a run on an MI355X."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, blocks, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

import dpmpp_ref as R  # noqa: E402
import seg_ref as S  # noqa: E402
import todo_ref as T  # noqa: E402

DEV = torch.device("cuda:0")
INF = math.inf
G = 3.5

# the issue's table, and one case with several position groups per lane slot, two channel chunks and a ragged last chunk (C = 72)
SHAPES = [(1, 1, 1, 8, 1.0), (2, 2, 2, 8, 100.0), (2, 5, 7, 24, 0.8), (2, 5, 7, 24, 100.0), (1, 8, 8, 320, 1.5), (3, 12, 12, 64, 100.0),
          (1, 9, 23, 8, 3.0), (1, 16, 16, 8, 2.0), (2, 150, 37, 72, 9.0)]
CASES = SHAPES + [s[:4] + (INF,) for s in SHAPES]


def _x(B, Hh, Ww, C, seed):
    return torch.randn((B * Hh * Ww, C), generator=torch.Generator().manual_seed(seed)).half()


# ---- 1. the kernel against float64
@pytest.mark.parametrize("B,Hh,Ww,C,sigma", CASES)
def test_token_blur_matches_float64(B, Hh, Ww, C, sigma):
    x = _x(B, Hh, Ww, C, seed=B * 1000 + Hh * 31 + Ww + C)
    ref, bound = S.bound(x, B, Hh, Ww, sigma)
    rows = x.shape[0]
    buf = torch.full((rows + 16, C), 7.0, dtype=torch.float16, device=DEV)  # 8 guard rows on either side
    out = buf[8:8 + rows]
    got = ops.token_blur(x.to(DEV), B, Hh, Ww, sigma, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    err = (got.cpu().double() - ref).abs()
    print(f"\nSEG_BLUR ({B},{Hh},{Ww},{C}) sigma {sigma}: k {S.kernel_size(sigma, Hh) if sigma != INF else '-'}x"
          f"{S.kernel_size(sigma, Ww) if sigma != INF else '-'} max err {float(err.max()):.3e}, worst excess over the bound {float((err - bound).max()):.3e}")
    assert torch.isfinite(got).all() and (err <= bound).all()
    assert (buf[:8] == 7.0).all() and (buf[8 + rows:] == 7.0).all()         # nothing written in front of or behind y
    again = ops.token_blur(x.to(DEV), B, Hh, Ww, sigma)
    torch.cuda.synchronize()
    assert torch.equal(again, got)                                          # the same bits twice


def test_one_tap_returns_x_bit_for_bit_and_a_constant_stays():
    B, Hh, Ww, C = 2, 5, 7, 24
    x = _x(B, Hh, Ww, C, 3)
    x[0, :4] = torch.tensor([-0.0, 0.0, 6e-8, 65504.0]).half()
    assert S.kernel_size(0.1, Hh) == 1 and S.kernel_size(0.1, Ww) == 1
    got = ops.token_blur(x.to(DEV), B, Hh, Ww, 0.1).cpu()
    assert torch.equal(got.view(torch.int16), x.view(torch.int16))
    for sigma in (1.5, 100.0, INF):
        c = torch.full((B * Hh * Ww, C), 0.3337, dtype=torch.float16)
        ref, bound = S.bound(c, B, Hh, Ww, sigma)
        err = (ops.token_blur(c.to(DEV), B, Hh, Ww, sigma).cpu().double() - ref).abs()
        print(f"\nSEG_CONSTANT sigma {sigma}: max err {float(err.max()):.3e}")
        assert (err <= bound).all() and float((ref - 0.3337).abs().max()) < 1e-3


def test_refused_arguments_leave_y_alone():
    B, Hh, Ww, C = 2, 4, 6, 16
    x = _x(B, Hh, Ww, C, 5).to(DEV)
    y = torch.full_like(x, 7.0)
    ws = torch.empty(B * Hh * Ww * C + 8, dtype=torch.float32, device=DEV)
    w5, w7, w3 = (torch.tensor(S.taps(1.0, n).float().tolist(), device=DEV) for n in (4, 6, 2))
    assert (w5.numel(), w7.numel(), w3.numel()) == (5, 7, 3)
    X, Y, W, A, Bx = x.data_ptr(), y.data_ptr(), ws.data_ptr(), w5.data_ptr(), w7.data_ptr()
    blur = lambda x_=X, y_=Y, b=B, h=Hh, w=Ww, c=C, wy=A, ky=5, wx=Bx, kx=7, ws_=W: _lib.call(
        "md_token_blur_f16", x_, y_, b, h, w, c, wy, ky, wx, kx, ws_, ops._st())
    mean = lambda x_=X, y_=Y, b=B, l=Hh * Ww, c=C, ws_=W: _lib.call("md_token_mean_f16", x_, y_, b, l, c, ws_, ops._st())
    shared = (dict(x_=0), dict(y_=0), dict(ws_=0), dict(x_=X + 2), dict(y_=Y + 8), dict(ws_=W + 4), dict(c=12), dict(c=0), dict(b=0), dict(y_=X),
              dict(y_=X + 32), dict(ws_=X), dict(ws_=Y))
    table = ((blur, shared + (dict(h=0), dict(w=-1), dict(wy=0), dict(wx=0), dict(ky=4), dict(ky=0), dict(ky=7), dict(kx=6), dict(kx=9), dict(kx=-1),
                              dict(h=225, ky=1))),
             (mean, shared + (dict(l=0), dict(l=-3))))
    for call, cases in table:
        for kw in cases:
            with pytest.raises(_lib.MdanceHipError):
                call(**kw)
            torch.cuda.synchronize()
            assert (y == 7.0).all(), kw                                     # nothing was launched
    blur()
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and not (y == 7.0).all()
    for bad in (0.0, -1.0, float("nan"), "1", None, True):
        with pytest.raises(_lib.MdanceHipError):
            ops.token_blur(x, B, Hh, Ww, bad)
    with pytest.raises(_lib.MdanceHipError):
        ops.token_blur(x, B, Hh + 1, Ww, 1.0)


# ---- 2. one TransformerBlock in read mode
def _close(got, ref, what):
    """The operator bound of tests/test_blocks_gpu.py."""
    got, ref = got.float().cpu(), ref.float()
    err, bound = (got - ref).abs().max().item(), 1e-2 * ref.abs().max().item() + 1e-3
    print(f"\nSEG_BLOCK {what}: max err {err:.4g} (bound {bound:.4g})")
    assert got.shape == ref.shape and err <= bound, f"{what}: max err {err:.4g} > {bound:.4g}"
    return bound


@pytest.mark.parametrize("Hh,Ww", [(8, 8), (5, 7)])
@pytest.mark.parametrize("sigma", [1.5, INF])
def test_transformer_block_blurred_queries(Hh, Ww, sigma):
    st = T.block_setup(320, 64, Hh, Ww, 2, DEV, seed=21)
    blk, f, L, dim = st.blk, st.f, st.L, st.dim
    x, bank, ctx = st.x[f:].float(), st.bank.float(), st.ctx_f[f:]          # the conditional frames
    blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [st.bank.to(DEV)]
    cross = st.cross.rows(f, 2 * f)
    try:
        with torch.no_grad():
            h = st.x[f:].reshape(f * L, dim).to(DEV)
            got = blk(h.clone(), f, L, cross, sa=blocks.SelfAttnCall(blur=((blk,), sigma)), grid=(Hh, Ww))
            want = S.block_read(st.sd, "", x, ctx, bank, Hh, Ww, sigma)
            bound = _close(got.view(f, L, dim), want, f"{Hh}x{Ww} sigma {sigma}: selected vs seg_ref")
            plain = S.O.transformer_block_read(st.sd, "", x, ctx, bank, cfg=False)
            moved = float((plain - want).abs().max())
            print(f"\nSEG_BLOCK {Hh}x{Ww} sigma {sigma}: restated perturbed vs unperturbed {moved:.4g} = {moved / bound:.1f} x the bound")
            assert moved > 10 * bound                                       # of the references alone: the perturbation is far above the bound
            # unselected: the conditional half of a normal CFG call on the same rows, bitwise (same kernel flavours at these sizes, as PAG's test)
            un = blk(h.clone(), f, L, cross, sa=blocks.SelfAttnCall(blur=((), sigma)), grid=(Hh, Ww))
            both = blk(st.x.reshape(2 * f * L, dim).to(DEV), 2 * f, L, st.cross)
            torch.cuda.synchronize()
            assert torch.equal(un, both[f * L:])
            _close(un.view(f, L, dim), plain, f"{Hh}x{Ww}: unselected vs the oracle's conditional read")
            # with K / V token downsampling the selected block still attends: blurred q, pooled k / v
            got = blk(h.clone(), f, L, cross, sa=blocks.SelfAttnCall(blur=((blk,), sigma), pool={blk: (2, "mean")}), grid=(Hh, Ww))
            _close(got.view(f, L, dim), S.block_read(st.sd, "", x, ctx, bank, Hh, Ww, sigma, kv_pool=(2, "mean")),
                   f"{Hh}x{Ww} sigma {sigma}: selected with kv_pool (2, mean)")
            for kw in (dict(identity=(blk,)),):
                with pytest.raises(ValueError):
                    blk(h.clone(), f, L, cross, sa=blocks.SelfAttnCall(blur=((blk,), sigma), **kw), grid=(Hh, Ww))
    finally:
        blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []


# ---- 3. the loop
@pytest.fixture(scope="module")
def small():
    return build_models()


def _sched():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


def _loop(sch, models, inputs, steps, guidance=G, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, guidance, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_scale_zero_is_bitwise_the_plain_loop(small, monkeypatch, sampler):
    inputs = synth_inputs(4, 16, 16, ctx_len=5, ctx_dim=64, seed=91)
    mk = lambda: M.DDIMScheduler(**SCHED_KWARGS) if sampler == "ddim" else _sched()
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    a = _loop(mk(), small, inputs, 4, seg_scale=0.0, seg_blur_sigma=2.0, seg_applied_layers=("up_blocks.1",))
    seen_a = list(names)
    del names[:]
    b = _loop(mk(), small, inputs, 4)
    step = "md_cfg_ddim_step" if sampler == "ddim" else "md_cfg_multistep_step"
    assert torch.equal(a, b) and seen_a == names and [n for n in names if n.startswith("md_cfg")] == [step] * 4      # launch for launch
    assert not any("token_blur" in n or "token_mean" in n for n in names)
    del names[:]
    c = _loop(mk(), small, inputs, 4, seg_scale=3.0, seg_applied_layers=("mid",))
    assert [n for n in names if n.startswith("md_cfg")] == [step + "_pag"] * 4 and names.count("md_token_blur_f16") == 4
    d = rel_l2(c, b)
    print(f"\nSEG_EFFECT {sampler} rel_l2(seg_scale 3 on mid, plain) {d:.3e}")
    assert d > 3e-2, d                                                     # the keywords are not silently ignored


WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)
LOOPS = {"ddim": dict(), "2m": dict(sampler="2m"), "no-cfg": dict(guidance=1.0), "two-windows": dict(frames=8, win=dict(context_frames=6, context_stride=1, context_overlap=2)),
         "kv-downsample-2": dict(kv=2)}


@pytest.mark.parametrize("sigma", [100.0, INF])
@pytest.mark.parametrize("case", list(LOOPS))
def test_loop_vs_restatement_reduced_width(small, case, sigma):
    cfg = LOOPS[case]
    frames, steps, g, win = cfg.get("frames", 4), 4, cfg.get("guidance", G), cfg.get("win", {})
    lat, rl, emb = (t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=500 + frames))
    if g <= 1.0:
        emb = emb[1:]
    two_m = cfg.get("sampler") == "2m"
    mk = (lambda: _sched()) if two_m else (lambda: M.DDIMScheduler(**SCHED_KWARGS))
    mk_rs = lambda: R.Restated(2, "dpmsolver++", "midpoint") if two_m else None
    kv = cfg.get("kv", 1)
    _, _, ref_sd, den_sd = small
    with torch.no_grad():
        want = S.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, seg_scale=3.0, seg_blur_sigma=sigma, seg_layers=("mid",), kv_downsample=kv,
                              scheduler=mk_rs(), guidance_scale=g, **win)
        plain_want = S.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, seg_scale=0.0, kv_downsample=kv, scheduler=mk_rs(), guidance_scale=g, **win)
    if win:
        assert len(S.P.FR.make_windows("uniform", frames, **win)) == 2
    out = _loop(mk(), small, (lat, rl, emb), steps, guidance=g, seg_scale=3.0, seg_blur_sigma=sigma, seg_applied_layers=("mid",), kv_downsample=kv, **win)
    e, c, d = rel_l2(out, want), cosine(out, want), rel_l2(plain_want, want)
    print(f"\nSEG_LOOP {case} sigma {sigma} {steps} steps rel_l2 {e:.3e} cos {c:.7f} (restated seg_scale 0 vs 3: {d:.3e})")
    assert torch.isfinite(out).all() and e <= 3e-2 and c >= 0.999, (e, c)
    assert d > 3e-2, d                                                     # of the restatement alone: SEG moves the result beyond the bound


def test_script_seg(tmp_path, golden_dir):
    """The drop-in script end to end, with and without --seg_scale 3 --seg_blur_sigma inf (128 x 128 pixels: the mid block sees 2 x 2 tokens)."""
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir, width=128, height=128)
    base = ["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "3", "--seed", "7"]
    on = U.read_frames(inference_video.main(base + ["--seg_scale", "3", "--seg_blur_sigma", "inf", "--output_dir", str(tmp_path / "on")]))
    off = U.read_frames(inference_video.main(base + ["--output_dir", str(tmp_path / "off")]))
    a, b = (np.stack([np.asarray(fr, dtype=np.float32) for fr in frames]) for frames in (on, off))
    assert len(on) == len(off) == F_ and np.isfinite(a).all() and a[:, :, 2 * (W + 2):].std() > 0
    print(f"\nSEG_SCRIPT mean |on - off| over the generated panel {float(np.abs(a - b)[:, :, 2 * (W + 2):].mean()):.3f} (of 255)")
    assert not np.array_equal(a, b)
