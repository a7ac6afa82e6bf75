"""GPU: open-ended windows and pyramid window fusion on the MI355X -- md_window_accumulate_weighted against float64 on its own inputs, its
bitwise equality with md_window_accumulate at weight 1, determinism and refusals; the defaults bitwise the loop without the keywords; the
loop at reduced width against tests/fusion_ref.py for every schedule / fuse pair, both samplers, with and without CFG, with guidance rescale
and video-to-video; two ranks under WindowParallel; the drop-in script with the four new flags.

Kernel bound (derived, not tuned): fp16 inputs are exact in fp32; each contribution costs one rounding of the product w * p and one of the
sum, each at most 2^-24 relative.  The k products together err by at most 2^-24 sum|w p|, each of the k sums by at most 2^-24 times the
magnitude it holds, itself at most S = |initial| + sum|w p|: |error| <= (k + 1) 2^-24 S to first order."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

import dpmpp_ref as R  # noqa: E402
import fusion_ref as FR  # noqa: E402
from loop_helpers import free_port  # noqa: E402
import v2v_ref as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
WIN12 = dict(context_frames=8, context_stride=1, context_overlap=4)        # F = 12: three windows closed (one wraps), two open
WIN16 = dict(context_frames=8, context_stride=1, context_overlap=2)        # F = 16: three windows under both schedules
PAIRS = [("uniform_open", "flat"), ("uniform", "pyramid"), ("uniform_open", "pyramid")]


# ---- 1. the kernel
def _kernel_case(hw, halves, f, ftot, seed, launches=3, ones=False):
    """`launches` windows of f slots over ftot frames: random distinct frames per window, some slots -1, random positive weights."""
    g = torch.Generator().manual_seed(seed)
    ns0 = torch.randn((halves, ftot, hw, 4), generator=g) * 3.0
    cnt0 = torch.rand((ftot,), generator=g)
    wins, wts, preds = [], [], []
    for _ in range(launches):
        win = torch.randperm(ftot, generator=g)[:f].to(torch.int32)
        if f > 2:
            win[torch.randint(0, f, (1,), generator=g)] = -1
        wins.append(win)
        wts.append(torch.ones(f) if ones else (torch.rand((f,), generator=g) * 0.9 + 0.05))
        preds.append((torch.randn((halves * f, hw, 4), generator=g) * 2.0).half())
    return ns0, cnt0, wins, wts, preds


KERNEL_CASES = [(hw, halves) for hw in (1, 2, 3, 5, 63, 64, 143, 255, 256, 257, 1023, 4096, 9216, 16383, 16384) for halves in (1, 2)]


@pytest.mark.parametrize("hw,halves", KERNEL_CASES)
def test_weighted_accumulate_matches_float64(hw, halves):
    f, ftot = 5, 7
    ns0, cnt0, wins, wts, preds = _kernel_case(hw, halves, f, ftot, seed=hw * 2 + halves)
    want, mag, k = ns0.double().clone(), ns0.double().abs().clone(), torch.zeros(ftot)
    cwant = cnt0.double().clone()
    ns, cnt = ns0.to(DEV), cnt0.to(DEV)
    for win, w, p in zip(wins, wts, preds):
        ops.window_accumulate_weighted(p.to(DEV), ns, cnt, win.to(DEV), w.to(DEV), f, ftot, hw, halves=halves)
        p64 = p.double().view(halves, f, hw, 4)
        for i, fr in enumerate(win.tolist()):
            if fr < 0:
                continue
            want[:, fr] += float(w[i]) * p64[:, i]                           # float(w[i]): the fp32 weight the kernel read, exactly
            mag[:, fr] += (float(w[i]) * p64[:, i]).abs()
            k[fr] += 1
            cwant[fr] += float(w[i])
    torch.cuda.synchronize()
    err = (ns.cpu().double() - want).abs()
    bound = (k.double().view(1, -1, 1, 1) + 1.0) * 2.0 ** -24 * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"\nWEIGHTED_KERNEL hw {hw} halves {halves}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}, k up to {int(k.max())}")
    assert (err <= bound).all(), worst
    assert torch.equal(ns.cpu()[:, k == 0], ns0[:, k == 0])                   # frames no window named are untouched
    assert ((cnt.cpu().double() - cwant).abs() <= (k.double() + 1.0) * 2.0 ** -24 * cwant).all()


@pytest.mark.parametrize("hw,halves", [(1, 1), (143, 2), (257, 1), (4096, 2), (16384, 2), (16383, 1)])
def test_weight_one_is_bitwise_window_accumulate(hw, halves):
    f, ftot = 6, 9
    ns0, cnt0, wins, wts, preds = _kernel_case(hw, halves, f, ftot, seed=hw + 11, ones=True)
    a, ca, b, cb = ns0.to(DEV), cnt0.to(DEV), ns0.to(DEV), cnt0.to(DEV)
    for win, w, p in zip(wins, wts, preds):
        ops.window_accumulate(p.to(DEV), a, ca, win.to(DEV), f, ftot, hw, halves=halves)
        ops.window_accumulate_weighted(p.to(DEV), b, cb, win.to(DEV), w.to(DEV), f, ftot, hw, halves=halves)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(ca, cb) and not torch.equal(a.cpu(), ns0)


def test_two_identical_launches_are_bitwise_equal():
    hw, halves, f, ftot = 16384, 2, 30, 48
    ns0, cnt0, wins, wts, preds = _kernel_case(hw, halves, f, ftot, seed=5, launches=2)
    outs = []
    for _ in range(2):
        ns, cnt = ns0.to(DEV), cnt0.to(DEV)
        for win, w, p in zip(wins, wts, preds):
            ops.window_accumulate_weighted(p.to(DEV), ns, cnt, win.to(DEV), w.to(DEV), f, ftot, hw, halves=halves)
        torch.cuda.synchronize()
        outs.append((ns.cpu(), cnt.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_refusals():
    f, ftot, hw = 4, 6, 8
    pred = torch.zeros((2 * f, hw, 4), device=DEV, dtype=torch.float16)
    ns, cnt = torch.zeros((2, ftot, hw, 4), device=DEV), torch.zeros((ftot,), device=DEV)
    win = torch.arange(f, dtype=torch.int32, device=DEV)
    wts = torch.ones((f + 1,), device=DEV)
    base = dict(pred=pred.data_ptr(), ns=ns.data_ptr(), cnt=cnt.data_ptr(), win=win.data_ptr(), w=wts.data_ptr(), f=f, ftot=ftot, hw=hw, halves=2)

    def call(**kw):
        a = dict(base, **kw)
        _lib.call("md_window_accumulate_weighted", a["pred"], a["ns"], a["cnt"], a["win"], a["w"], a["f"], a["ftot"], a["hw"], a["halves"], ops._st())

    call()                                                                 # the valid call
    call(w=wts.data_ptr() + 4)                                             # any 4-byte aligned weights
    for kw in (dict(pred=0), dict(ns=0), dict(cnt=0), dict(win=0), dict(w=0), dict(w=wts.data_ptr() + 2), dict(w=wts.data_ptr() + 1),
               dict(halves=0), dict(halves=3), dict(f=0), dict(f=-1), dict(ftot=f - 1)):
        with pytest.raises(_lib.MdanceHipError):
            call(**kw)
    torch.cuda.synchronize()
    assert float(cnt.sum().cpu()) == 2.0 * f                               # the two valid calls only
    with pytest.raises(_lib.MdanceHipError):                               # the wrapper: a CPU tensor
        ops.window_accumulate_weighted(pred, ns, cnt, win, wts[:f].cpu(), f, ftot, hw)


# ---- 2. the loop
@pytest.fixture(scope="module")
def small():
    return build_models()


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


def _loop(sch, models, inputs, steps, g=3.5, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    lat, rl, emb = (t.half().to(DEV) for t in inputs)
    out = pipe.denoise(lat, rl, emb if g > 1 else emb[1:], steps, g, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _want(models, inputs, steps, g=3.5, scheduler=None, **kw):
    _, _, ref_sd, den_sd = models
    lat, rl, emb = inputs
    with torch.no_grad():
        return FR.denoise_loop(ref_sd, den_sd, lat, rl, emb if g > 1 else emb[1:], steps, guidance_scale=g, reduced=True, scheduler=scheduler, **kw)


def _inputs(frames, seed):
    return tuple(t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=seed))


@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_defaults_are_bitwise_the_loop_without_the_keywords(small, monkeypatch, sampler):
    inputs = _inputs(12, 81)
    mk = _ddim if sampler == "ddim" else _dpm
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    a = _loop(mk(), small, inputs, 4, context_schedule="uniform", context_fuse="flat", **WIN12)
    assert "md_window_accumulate_weighted" not in names and names.count("md_window_accumulate") == 4 * 3
    del names[:]
    b = _loop(mk(), small, inputs, 4, **WIN12)
    assert torch.equal(a, b) and "md_window_accumulate_weighted" not in names
    del names[:]
    c = _loop(mk(), small, inputs, 4, context_schedule="uniform_open", context_fuse="pyramid", **WIN12)
    assert names.count("md_window_accumulate_weighted") == 4 * 2 and "md_window_accumulate" not in names
    d = rel_l2(c, b)
    print(f"\nFUSION_EFFECT {sampler} rel_l2(uniform_open + pyramid, defaults) {d:.3e}")
    assert d > 1e-3, d                                                     # the keywords are not silently ignored


def test_single_window_pyramid_is_bitwise_flat(small):
    inputs = _inputs(4, 83)
    for g in (3.5, 1.0):
        a = _loop(_ddim(), small, inputs, 3, g=g)
        b = _loop(_ddim(), small, inputs, 3, g=g, context_fuse="pyramid", context_schedule="uniform_open")
        assert torch.equal(a, b)


def _check(tag, out, want, base_err):
    r, c = rel_l2(out, want), cosine(out, want)
    print(f"\nFUSION_LOOP {tag} rel_l2 {r:.3e} cos {c:.7f} (uniform + flat, same clip and settings: {base_err:.3e})")
    assert r <= 3e-2 and c >= 0.999 and r <= 2.0 * base_err, (tag, r, c, base_err)


@pytest.mark.parametrize("g", [3.5, 1.0], ids=["cfg", "nocfg"])
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_loop_vs_restatement_f12(small, sampler, g):
    inputs = _inputs(12, 300)
    mk = _ddim if sampler == "ddim" else _dpm
    rs = (lambda: None) if sampler == "ddim" else (lambda: R.Restated(2, "dpmsolver++", "midpoint"))
    base = rel_l2(_loop(mk(), small, inputs, 8, g=g, **WIN12), _want(small, inputs, 8, g=g, scheduler=rs(), **WIN12))
    for schedule, fuse in PAIRS:
        out = _loop(mk(), small, inputs, 8, g=g, context_schedule=schedule, context_fuse=fuse, **WIN12)
        want = _want(small, inputs, 8, g=g, scheduler=rs(), schedule=schedule, fuse=fuse, **WIN12)
        _check(f"f12 {sampler} g={g} {schedule}+{fuse}", out, want, base)


def test_loop_vs_restatement_f16_three_windows(small):
    inputs = _inputs(16, 316)
    assert len(FR.make_windows("uniform_open", 16, 8, 1, 2)) == 3 and len(FR.make_windows("uniform", 16, 8, 1, 2)) == 3
    base = rel_l2(_loop(_ddim(), small, inputs, 8, **WIN16), _want(small, inputs, 8, **WIN16))
    for schedule, fuse in PAIRS:
        out = _loop(_ddim(), small, inputs, 8, context_schedule=schedule, context_fuse=fuse, **WIN16)
        _check(f"f16 ddim g=3.5 {schedule}+{fuse}", out, _want(small, inputs, 8, schedule=schedule, fuse=fuse, **WIN16), base)


def test_loop_with_guidance_rescale(small):
    inputs = _inputs(12, 330)
    kw = dict(guidance_rescale=0.7, **WIN12)
    base = rel_l2(_loop(_ddim(), small, inputs, 8, **kw), _want(small, inputs, 8, **kw))
    out = _loop(_ddim(), small, inputs, 8, context_schedule="uniform_open", context_fuse="pyramid", **kw)
    _check("f12 ddim rescale 0.7 uniform_open+pyramid", out, _want(small, inputs, 8, schedule="uniform_open", fuse="pyramid", **kw), base)


def test_loop_with_video_to_video(small):
    lat, rl, emb = _inputs(12, 340)
    x0 = (torch.randn(lat.shape, generator=torch.Generator().manual_seed(341)) * 0.8).half().float()
    t0 = O.DDIM().set_timesteps(8)[8 - V.kept_steps(8, 0.5)]
    start = V.noised(x0, lat, t0)
    run = lambda **kw: _loop(_dpm(), small, (lat, rl, emb), 8, init_latents=x0.half().to(DEV), strength=0.5, **WIN12, **kw)
    ref = lambda **kw: _want(small, (start, rl, emb), 8, scheduler=V.Truncated(R.Restated(2, "dpmsolver++", "midpoint"), 0.5), **WIN12, **kw)
    base = rel_l2(run(), ref())
    out = run(context_schedule="uniform_open", context_fuse="pyramid")
    _check("f12 2m strength 0.5 uniform_open+pyramid", out, ref(schedule="uniform_open", fuse="pyramid"), base)


# ---- 3. two ranks on one GPU
def _wp_worker(rank, world, port, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MD_DIST_BACKEND="gloo")
        torch.set_num_threads(max(1, min(16, (os.cpu_count() or 2) // world)))
        import torch.distributed as dist
        from mikudance_amd import DDIMScheduler, MikuDanceVideoPipeline, dp
        dp.init()
        dev = torch.device("cuda", 0)
        ref, den, _, _ = build_models(device=dev, keep_state_dicts=False)
        pipe = MikuDanceVideoPipeline(None, None, ref, den, DDIMScheduler(**SCHED_KWARGS))
        lat, rl, emb = (t.half().to(dev) for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=77))
        kw = dict(context_schedule="uniform_open", context_fuse="pyramid", **WIN16)   # [0..7] [6..13] [8..15]: no frame in three windows
        out = pipe.denoise(lat, rl, emb, 3, 3.5, window_parallel=dp.WindowParallel(), **kw)
        torch.cuda.synchronize()
        got = dp.gather_latents(out)
        res = {"rank": rank}
        if rank == 0:
            one = pipe.denoise(lat, rl, emb, 3, 3.5, **kw)
            flat = pipe.denoise(lat, rl, emb, 3, 3.5, **dict(kw, context_fuse="flat"))
            res.update(same_on_both_ranks=torch.equal(got[0], got[1]), equals_one_rank=torch.equal(out, one),
                       finite=bool(torch.isfinite(out).all()), weighted=not torch.equal(out, flat))
        dist.destroy_process_group()
        q.put(res)
    except Exception as e:
        import traceback
        q.put({"rank": rank, "error": f"{e!r}\n{traceback.format_exc()}"})


def test_window_parallel_two_ranks_equal_one_rank():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_wp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = []
    try:
        for _ in range(world):
            res = q.get(timeout=900)
            results.append(res)
            if "error" in res:
                break
        for p in procs:
            if not any("error" in r for r in results):
                p.join(timeout=120)
    finally:
        for p in procs:                             # never leave a rank holding cuda:0 for the following tests
            if p.is_alive():
                p.terminate()
            p.join(timeout=30)
    for res in results:
        assert "error" not in res, res["error"]
        if res["rank"] == 0:
            assert res["same_on_both_ranks"] and res["equals_one_rank"] and res["finite"] and res["weighted"], res
    assert len(results) == world and all(p.exitcode == 0 for p in procs)


# ---- 4. the script
def test_script_window_flags(tmp_path, golden_dir):
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir, frames=6)
    base = ["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "3", "--seed", "7"]
    win = ["--context_frames", "4", "--context_overlap", "2"]              # 6 frames: [0..3] [2..5] open, three windows closed
    new = inference_video.main(base + win + ["--context_schedule", "uniform_open", "--context_fuse", "pyramid", "--output_dir", str(tmp_path / "o1")])
    frames = U.read_frames(new)
    a = np.asarray(frames[0], dtype=np.float32)
    assert len(frames) == F_ and np.isfinite(a).all() and a[:, 2 * (W + 2):].std() > 0
    plain = inference_video.main(base + win + ["--output_dir", str(tmp_path / "o2")])
    named = inference_video.main(base + win + ["--context_fuse", "flat", "--context_schedule", "uniform", "--output_dir", str(tmp_path / "o3")])
    assert open(plain, "rb").read() == open(named, "rb").read()
    assert open(plain, "rb").read() != open(new, "rb").read()
