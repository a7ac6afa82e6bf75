"""CPU: open-ended windows (context_schedule="uniform_open") and pyramid window fusion (context_fuse="pyramid") -- the layout against its
rule restated in tests/fusion_ref.py plus its properties, the weights against diffusers' list and their per-frame normalisation, the argument
checks, and the host loop of MikuDanceVideoPipeline.denoise() on emulated operators against the restated loop (one rank, three gloo ranks)."""
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd.context import get_context_scheduler
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import fake_ops
import fusion_ref as FR
import rescale_ref as RR
import v2v_ref as V
from loop_helpers import (CountingUNet, cosine, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401 (small_cpu: fixture)
                          worker_setup)

WIN12 = dict(context_frames=8, context_stride=1, context_overlap=4)        # f = 12: three windows (one wrapping) closed, two open


# ---- 1. the layout
GRID = [(F, s, o, lv) for s, o in ((8, 4), (8, 2), (16, 4), (30, 8), (30, 0), (5, 1), (3, 2))
        for F in sorted({1, s - 1, s, s + 1, s + 2, 2 * s - 1, 2 * s, 2 * s + 1, 3 * s + 1, 48, 64, 100, 300}) for lv in (1, 2, 3, 5)]


@pytest.mark.parametrize("F,s,o,lv", GRID)
def test_open_layout_matches_the_rule_and_its_properties(F, s, o, lv):
    got = [list(w) for w in get_context_scheduler("uniform_open")(0, 30, F, s, lv, o)]
    assert got == FR.open_windows(F, s, o, lv)
    assert got == [list(w) for w in get_context_scheduler("uniform_open")(7, 30, F, s, lv, o)]       # the step is ignored
    assert sorted({fr for w in got for fr in w}) == list(range(F))                                      # every frame covered
    assert len({tuple(w) for w in got}) == len(got)                                                     # no duplicates
    if F <= s:
        assert got == [list(range(F))]
        return
    by_d = {}
    for w in got:
        assert len(w) == s and all(0 <= fr < F for fr in w)
        steps = {b - a for a, b in zip(w, w[1:])}
        d = steps.pop() if s > 1 else 1
        assert not steps and d >= 1 and d & (d - 1) == 0                                                 # constant, a power of two
        by_d.setdefault(d, []).append(w)
    assert sorted(by_d) == [2 ** k for k in range(len(by_d))] and len(by_d) <= lv
    for d, ws in by_d.items():
        # the level's last begin is F - span; a duplicate of an earlier level's window is dropped, which for s >= 2 cannot happen
        assert max(w[-1] for w in ws) == F - 1
        assert ws[0][0] == 0
    one = by_d[1]
    for a, b in zip(one, one[1:]):
        assert b[0] > a[0] and len(set(a) & set(b)) >= o


def test_open_layout_worked_examples():
    sch = get_context_scheduler("uniform_open")
    starts = lambda F, s, o, lv: [(w[0], w[1] - w[0]) for w in sch(0, 30, F, s, lv, o)]
    assert [list(w) for w in sch(0, 30, 48, 30, 1, 8)] == [list(range(0, 30)), list(range(18, 48))]
    assert starts(100, 30, 8, 1) == [(0, 1), (22, 1), (44, 1), (66, 1), (70, 1)]
    assert [list(w) for w in sch(0, 30, 12, 8, 1, 4)] == [list(range(0, 8)), list(range(4, 12))]
    assert starts(64, 16, 4, 3) == [(0, 1), (12, 1), (24, 1), (36, 1), (48, 1), (0, 2), (28, 2), (33, 2), (0, 4), (3, 4)]
    closed = [list(w) for w in get_context_scheduler("uniform")(0, 30, 48, 30, 1, 8)]
    assert len(closed) == 3 and sum(1 for w in closed if w != sorted(w)) == 2                           # what the open layout replaces


def test_scheduler_names_and_errors():
    for bad in ("pyramid", "uniform_closed", "", None):
        with pytest.raises(ValueError, match="Unknown context_overlap policy"):
            get_context_scheduler(bad)
    for name in ("uniform", "uniform_open"):
        with pytest.raises(ValueError, match="context_overlap"):
            list(get_context_scheduler(name)(0, 30, 20, 8, 1, 8))
        assert [list(w) for w in get_context_scheduler(name)(0, 30, 6, 8, 1, 8)] == [list(range(6))]  # F <= s: no check needed


# ---- 2. the weights
def test_pyramid_is_diffusers_list():
    from mikudance_amd import windows as W
    for L in range(1, 65):
        assert W.pyramid(L) == FR.diffusers_pyramid(L) == FR.pyramid(L)


WEIGHT_CASES = [("uniform", 12, 8, 1, 4), ("uniform_open", 12, 8, 1, 4), ("uniform", 48, 30, 1, 8), ("uniform_open", 48, 30, 1, 8),
                ("uniform", 12, 8, 2, 4), ("uniform", 20, 16, 3, 4), ("uniform_open", 64, 16, 3, 4), ("uniform_open", 300, 30, 4, 8),
                ("uniform", 5, 8, 1, 4)]


@pytest.mark.parametrize("name,F,s,lv,o", WEIGHT_CASES)
def test_shares_sum_to_one_per_frame(name, F, s, lv, o):
    from mikudance_amd import windows as W
    wins = [list(w) for w in get_context_scheduler(name)(0, 30, F, s, lv, o)]
    got = W.fuse_weights(wins, F, "pyramid")
    want = FR.shares(wins, F)
    tot = np.zeros(F)
    for win, g, w in zip(wins, got, want):
        assert len(g) == len(win) and np.allclose(np.asarray(g), w.numpy(), rtol=1e-15, atol=0)
        sl = W.accumulate_slots(win)
        assert sl == FR.slots(win)
        for fr, x in zip(sl, g):
            assert (x == 0.0) == (fr < 0)
            if fr >= 0:
                tot[fr] += x
    assert np.abs(tot - 1.0).max() <= 1e-12
    if len(wins) == 1:
        assert all(x == 1.0 for x in got[0])


def test_a_wrapped_dilated_window_names_a_frame_twice():
    wins = [list(w) for w in get_context_scheduler("uniform")(0, 30, 12, 8, 2, 4)]
    assert any(len(set(w)) < len(w) for w in wins)                         # the case the -1 slots exist for is in WEIGHT_CASES


# ---- 3. argument checks
def _weighted():
    """(f, ftot, hw, halves) of every weighted accumulate so far."""
    return [(d["f"], d["ftot"], d["hw"], d["halves"]) for _, d in fake_ops.tail_calls("window_accumulate_weighted")]


@pytest.mark.parametrize("bad", ["Pyramid", "triangle", "", None, 1])
def test_bad_fuse_raises_before_any_model(monkeypatch, bad):
    fake_ops.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, M.DDIMScheduler(**SCHED_KWARGS))
    lat, rl, emb = torch.zeros(1, 4, 2, 2, 2, dtype=torch.float16), torch.zeros(1, 2, 22, 2, 2, dtype=torch.float16), torch.zeros(2, 5, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="context_fuse"):
        pipe.denoise(lat, rl, emb, 4, 3.5, context_fuse=bad)
    assert refu.calls == 0 and den.calls == 0 and fake_ops.tail_calls() == []
    # __call__: before the CLIP tower and the VAE as well
    from PIL import Image
    vae, clip = CountingUNet(), CountingUNet()
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        pipe = cls(vae=vae, image_encoder=clip, reference_unet=refu, denoising_unet=den, scheduler=M.DDIMScheduler(**SCHED_KWARGS))
        args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5)
        with pytest.raises(ValueError, match="context_fuse"):
            pipe(*args, context_fuse=bad)
        with pytest.raises(ValueError, match="Unknown context_overlap policy"):
            pipe(*args, context_schedule="open")
    assert refu.calls == 0 and den.calls == 0 and vae.calls == 0 and clip.calls == 0


def test_call_forwards_both_keywords(monkeypatch):
    from PIL import Image
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append((a[4] if len(a) > 4 else kw.get("context_schedule"), kw.get("context_fuse")))
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        pipe = cls(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=None, denoising_unet=types.SimpleNamespace(in_channels=4),
                   scheduler=M.DDIMScheduler(**SCHED_KWARGS))
        args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5)
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), context_schedule="uniform_open", context_fuse="pyramid")
    assert seen == [("uniform", "flat"), ("uniform_open", "pyramid")] * 2


def test_script_flags_parse():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.context_schedule, a.context_fuse, a.context_frames, a.context_overlap) == ("uniform", "flat", None, 8)
    a = IV.parse_args(["--context_schedule", "uniform_open", "--context_fuse", "pyramid", "--context_frames", "16", "--context_overlap", "4"])
    assert (a.context_schedule, a.context_fuse, a.context_frames, a.context_overlap) == ("uniform_open", "pyramid", 16, 4)
    for argv in (["--context_fuse", "triangle"], ["--context_schedule", "open"], ["--context_frames", "many"]):
        with pytest.raises(SystemExit):
            IV.parse_args(argv)


def test_script_flags_reach_the_call(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    seen = []

    def spy(self, latents, ref_latents, embeds, steps, guidance, schedule, frames, stride, overlap, *a, **kw):
        seen.append((schedule, frames, stride, overlap, kw["context_fuse"]))
        return latents

    monkeypatch.setattr(IV, "build_pipeline", fake_pipeline_builder(IV))
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base)
    IV.main(base + ["--context_schedule", "uniform_open", "--context_fuse", "pyramid", "--context_frames", "16", "--context_overlap", "4"])
    assert seen == [("uniform", None, 1, 8, "flat"), ("uniform_open", 16, 1, 4, "pyramid")]


# ---- 4. the restated loop is the oracle's at uniform + flat
@pytest.mark.parametrize("g", [3.5, 1.0], ids=["cfg", "nocfg"])
def test_restatement_equals_rescale_ref_at_uniform_flat(small_cpu, g):
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(12, 52)
    emb = emb if g > 1 else emb[1:]
    with torch.no_grad():
        want = RR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=g, reduced=True, **WIN12)
        got = FR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=g, reduced=True, schedule="uniform", fuse="flat", **WIN12)
        pyr = FR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=g, reduced=True, schedule="uniform", fuse="pyramid", **WIN12)
    assert torch.equal(got, want) and not torch.equal(pyr, want)


# ---- 5. the host loop on the emulated operators
@pytest.mark.parametrize("g", [3.5, 1.0], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("fuse", ["flat", "pyramid"])
@pytest.mark.parametrize("schedule", ["uniform", "uniform_open"])
def test_host_loop_matches_restatement(monkeypatch, small_cpu, schedule, fuse, g):
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(12, 61)
    emb = emb if g > 1 else emb[1:]
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 3, g, context_schedule=schedule, context_fuse=fuse, **WIN12)
    nb = 2 if g > 1 else 1
    n_win = {"uniform": 3, "uniform_open": 2}[schedule]
    assert _weighted() == ([(8, 12, 256, nb)] * (3 * n_win) if fuse == "pyramid" else [])
    with torch.no_grad():
        want = FR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 3, guidance_scale=g, reduced=True, schedule=schedule, fuse=fuse, **WIN12)
    r, c = rel_l2(out.float(), want), cosine(out.float(), want)
    print(f"\nFUSION_HOST_LOOP {schedule} {fuse} g={g} rel_l2 {r:.3e} cos {c:.7f}")
    assert torch.isfinite(out).all() and r <= 3e-2 and c >= 0.999, (r, c)


def test_defaults_never_call_the_weighted_op_and_keep_the_bits(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(12, 63))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    a = pipe.denoise(lat, rl, emb, 2, 3.5, context_schedule="uniform", context_fuse="flat", **WIN12)
    b = pipe.denoise(lat, rl, emb, 2, 3.5, **WIN12)
    assert torch.equal(a, b) and _weighted() == []
    c = pipe.denoise(lat, rl, emb, 2, 3.5, context_fuse="pyramid", **WIN12)
    assert not torch.equal(a, c) and len(_weighted()) == 6          # the keyword is not silently ignored


@pytest.mark.parametrize("g", [3.5, 1.0], ids=["cfg", "nocfg"])
def test_single_window_pyramid_is_bitwise_flat(monkeypatch, small_cpu, g):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 65))
    emb = emb if g > 1 else emb[1:]
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    a = pipe.denoise(lat, rl, emb, 2, g)
    b = pipe.denoise(lat, rl, emb, 2, g, context_fuse="pyramid", context_schedule="uniform_open")
    assert torch.equal(a, b) and len(_weighted()) == 2


def _check_combined(tag, out, want):
    r, c = rel_l2(out.float(), want), cosine(out.float(), want)
    print(f"\nFUSION_HOST_LOOP {tag} rel_l2 {r:.3e} cos {c:.7f}")
    assert torch.isfinite(out).all() and r <= 3e-2 and c >= 0.999, (r, c)


def test_loop_with_guidance_rescale(monkeypatch, small_cpu):
    """Pyramid fusion on open windows feeding guidance rescale and the scaled DDIM step: the CPU counterpart of the GPU test of this name."""
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(12, 330)
    kw = dict(guidance_rescale=0.7, **WIN12)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 3, 3.5, context_schedule="uniform_open", context_fuse="pyramid", **kw)
    tail = fake_ops.tail_calls()
    assert [(n, d["keywords"]) for n, d in tail] == ([("window_accumulate_weighted", ())] * 2 + [("cfg_guidance_rescale", ()), ("cfg_ddim_step", ("vscale",))]) * 3
    assert _weighted() == [(8, 12, 256, 2)] * 6 and all(d["phi"] == 0.7 for _, d in fake_ops.tail_calls("cfg_guidance_rescale"))
    with torch.no_grad():
        want = FR.denoise_loop(ref_sd, den_sd, lat, rl, emb, 3, guidance_scale=3.5, reduced=True, schedule="uniform_open", fuse="pyramid", **kw)
    _check_combined("rescale 0.7 ddim uniform_open pyramid", out, want)


def test_loop_with_video_to_video(monkeypatch, small_cpu):
    """Pyramid fusion on open windows inside a truncated, pre-noised DPM-Solver++ 2M schedule: the CPU counterpart of the GPU test of this name."""
    from oracle import cpu_ref as O
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(12, 340)
    x0 = (torch.randn(lat.shape, generator=torch.Generator().manual_seed(341)) * 0.8).half().float()
    strength, kept = 0.7, 2
    assert V.kept_steps(3, strength) == kept
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DPMSolverMultistepScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 3, 3.5, init_latents=x0.half(), strength=strength, context_schedule="uniform_open",
                       context_fuse="pyramid", **WIN12)
    tail = fake_ops.tail_calls()
    assert [(n, d["keywords"]) for n, d in tail] == [("add_noise", ())] + ([("window_accumulate_weighted", ())] * 2 + [("cfg_multistep_step", ())]) * kept
    assert _weighted() == [(8, 12, 256, 2)] * (2 * kept) and fake_ops.tail_calls("cfg_multistep_step")[0][1]["c_m1"] == 0.0
    start = V.noised(x0, lat, O.DDIM().set_timesteps(3)[3 - kept])
    with torch.no_grad():
        want = FR.denoise_loop(ref_sd, den_sd, start, rl, emb, 3, guidance_scale=3.5, reduced=True, schedule="uniform_open", fuse="pyramid",
                               scheduler=V.Truncated(R.Restated(2, "dpmsolver++", "midpoint"), strength), **WIN12)
    _check_combined(f"2m strength {strength} uniform_open pyramid", out, want)


# ---- 6. window parallelism: three gloo ranks
def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=321))
    # F = 16, s = 8, o = 2, open: [0..7], [6..13], [8..15] -- three windows, one per rank, no frame in more than two of them... frames 8..13
    # lie in windows 1 and 2 only, 6..7 in 0 and 1: every fp32 sum has at most two non-zero terms and is commutative
    kw = dict(context_frames=8, context_stride=1, context_overlap=2, context_schedule="uniform_open", context_fuse="pyramid")
    pipe = MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    out = pipe.denoise(lat, rl, emb, 3, 3.5, window_parallel=dp.WindowParallel(), **kw)
    got = dp.gather_latents(out)
    if rank == 0:
        one = pipe.denoise(lat, rl, emb, 3, 3.5, **kw)
        flat = pipe.denoise(lat, rl, emb, 3, 3.5, **dict(kw, context_fuse="flat"))
        q.put(dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                   finite=bool(torch.isfinite(out).all()), weighted=not torch.equal(out, flat)))
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    assert len(FR.open_windows(16, 8, 2, 1)) == 3
    res = run_world(3, _wp_worker)
    assert all(res.values()), res
