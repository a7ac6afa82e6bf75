"""CPU: adaptive DeepCache (deep_cache_threshold=; forward_nhwc(deep_cache=slot.auto(threshold, max_run))) on the emulated operator layer
(tests/fake_ops.py with the twin of ops.rel_l1 from tests/deepcache_adaptive_ref.py): the default path is untouched, the two ends of the threshold
are the fixed rule and the plain loop bit for bit, the accumulate / reset / cap / zero-denominator / NaN rules against scripted distances, every
refusal before any operator call, the first step of every pass, per-window decisions."""
import math

import pytest
import torch

import deepcache_adaptive_ref as AR
import deepcache_ref as DR
import fake_ops
import hires_ref
import mikudance_amd as M
from loop_helpers import CountingUNet, small_cpu, small_inputs, zero_inputs  # noqa: F401
from mikudance_amd import DeepCacheSlot
from mikudance_amd.selftest import SCHED_KWARGS
from test_deep_cache_cpu import _Spy, _modes                              # the helpers of the fixed rule's tests, as they are

G = 3.5


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _install(monkeypatch, fn=AR.rel_l1):
    fake_ops.install(monkeypatch)
    AR.install(monkeypatch, fn)


def _pipe(small_cpu):
    ref, den, _, _ = small_cpu
    return M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())


def _kinds(trace, window=None, plane=0):
    return [k for _, w, p, k, _ in trace if p == plane and (window is None or w == window)]


# ---- 1. the default path
def test_threshold_none_is_the_fixed_rule_call_for_call(monkeypatch, small_cpu):
    _install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 31))
    pipe = _pipe(small_cpu)
    spy = _Spy(small_cpu[1], monkeypatch)
    a = pipe.denoise(lat, rl, emb, 5, G, deep_cache_interval=2)
    calls_a, modes_a, trace_a = list(fake_ops.CALLS), _modes(spy), pipe.last_deep_cache_trace
    del fake_ops.CALLS[:], spy.calls[:]
    b = pipe.denoise(lat, rl, emb, 5, G, deep_cache_interval=2, deep_cache_threshold=None)
    assert torch.equal(a, b) and calls_a == fake_ops.CALLS and modes_a == _modes(spy)
    assert modes_a == [["fill"], ["reuse"], ["fill"], ["reuse"], ["fill"]]     # fill / reuse slots only: no auto call, so no decision
    assert not [c for c in calls_a if c[0] == "rel_l1"]
    # the fixed rule's trace carries no distance; without DeepCache there is no trace
    assert trace_a == [(k, 0, 0, "key" if k % 2 == 0 else "shallow", None) for k in range(5)] == pipe.last_deep_cache_trace
    pipe.denoise(lat, rl, emb, 2, G)
    assert pipe.last_deep_cache_trace is None
    plan = pipe.sampling_plan(2, G, False, (2, 16, 16), guidance_rescale=0.0, strength=1.0, context_fuse="flat", free_init_iters=1,
                              free_init_filter="butterworth", free_init_order=4, free_init_spatial_stop=0.25, free_init_temporal_stop=0.25,
                              free_init_fast=False, apg=False, apg_eta=0.0, apg_norm_threshold=0.0, apg_momentum=0.0, pag_scale=0.0,
                              pag_adaptive_scale=0.0, pag_applied_layers=("mid",), kv_downsample=1, kv_downsample_mode="nearest", seg_scale=0.0,
                              seg_blur_sigma=100.0, seg_applied_layers=("mid",), deep_cache_interval=3)
    assert plan.deep == (3, 3) and plan.deep_threshold is None


# ---- 2. the two ends of the threshold
@pytest.mark.parametrize("n,d", [(2, 3), (3, 3), (3, 1), (2, 4)])
def test_threshold_inf_is_the_cap_rule_bitwise(monkeypatch, small_cpu, n, d):
    _install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 41))
    pipe = _pipe(small_cpu)
    fixed = pipe.denoise(lat, rl, emb, 5, G, deep_cache_interval=n, deep_cache_depth=d)
    got = pipe.denoise(lat, rl, emb, 5, G, deep_cache_interval=n, deep_cache_depth=d, deep_cache_threshold=math.inf)
    trace = pipe.last_deep_cache_trace
    assert _kinds(trace) == ["key" if k % n == 0 else "shallow" for k in range(5)]
    assert torch.equal(got, fixed)
    assert trace[0][4] is None and all(math.isfinite(r) and r > 0 for *_, r in trace[1:])
    assert len([c for c in fake_ops.CALLS if c[0] == "rel_l1"]) == 4       # one distance per call behind the first


@pytest.mark.parametrize("d", [1, 3])
def test_tiny_threshold_is_the_plain_loop_bitwise(monkeypatch, small_cpu, d):
    _install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 42))
    pipe = _pipe(small_cpu)
    plain = pipe.denoise(lat, rl, emb, 4, G)
    got = pipe.denoise(lat, rl, emb, 4, G, deep_cache_interval=3, deep_cache_depth=d, deep_cache_threshold=1e-30)
    assert _kinds(pipe.last_deep_cache_trace) == ["key"] * 4 and torch.equal(got, plain)


def test_the_new_skip_does_not_overwrite_the_kept_one_before_the_decision(monkeypatch, small_cpu):
    """The distance is taken between two buffers: the kept skip slice still holds the step before when rel_l1 reads it."""
    seen = []

    def rel_l1(a, b, out=None):
        seen.append((a.data_ptr() != b.data_ptr(), bool((a != b).any())))
        return AR.rel_l1(a, b, out)

    _install(monkeypatch, rel_l1)
    lat, rl, emb = (t.half() for t in small_inputs(2, 43))
    _pipe(small_cpu).denoise(lat, rl, emb, 3, G, deep_cache_interval=2, deep_cache_threshold=math.inf)
    assert seen == [(True, True)] * 2


# ---- 3. the rules, step by step, against scripted distances
def _scripted(script):
    """ops.rel_l1 returning the (numerator, denominator) pairs of `script`, one per call."""
    left = list(script)

    def rel_l1(a, b, out=None):
        fake_ops.CALLS.append(("rel_l1", None))
        r = torch.tensor(left.pop(0), dtype=torch.float32)
        if out is None:
            return r
        out.copy_(r)
        return out
    return rel_l1, left


def test_planted_distances(monkeypatch, small_cpu):
    nan = float("nan")
    # threshold 1.0, cap 4; r = 2^-2 and 2^-1 add up exactly in binary floating point
    #  step  distance      accumulator      run   rule
    #   0    (fill)                                the first step of the pass
    #   1    0.25          0.25             1     below
    #   2    0.5           0.75             2     below
    #   3    0.25          1.0              3     acc >= threshold (equality fires) -> key, reset
    #   4    0.5           0.5              1     below: the accumulator started over
    #   5    0.25          0.75             2     below
    #   6    0.125         0.875            3     below
    #   7    0.0           0.875            4     run >= cap -> key, reset
    #   8    0 / 0                                zero denominator -> key (r = inf)
    #   9    nan / 1                               r not finite -> key
    #  10    0.5           0.5              1     below
    #  11    1 / 0                                zero denominator -> key
    script = [(0.25, 1.0), (1.0, 2.0), (0.5, 2.0), (0.5, 1.0), (0.25, 1.0), (0.125, 1.0), (0.0, 1.0), (0.0, 0.0), (nan, 1.0), (0.5, 1.0), (1.0, 0.0)]
    want = [("key", None), ("shallow", 0.25), ("shallow", 0.5), ("key", 0.25), ("shallow", 0.5), ("shallow", 0.25), ("shallow", 0.125), ("key", 0.0),
            ("key", math.inf), ("key", nan), ("shallow", 0.5), ("key", math.inf)]
    fn, left = _scripted(script)
    _install(monkeypatch, fn)
    lat, rl, emb = (t.half() for t in small_inputs(2, 44))
    pipe = _pipe(small_cpu)
    spy = _Spy(small_cpu[1], monkeypatch)
    out = pipe.denoise(lat, rl, emb, 12, G, deep_cache_interval=4, deep_cache_threshold=1.0)
    assert not left and torch.isfinite(out).all()
    trace = pipe.last_deep_cache_trace
    assert [(s, w, p) for s, w, p, _, _ in trace] == [(k, 0, 0) for k in range(12)]
    for (_, _, _, kind, r), (wkind, wr) in zip(trace, want):
        assert kind == wkind and (r == wr or (wr is not None and math.isnan(wr) and math.isnan(r))), (trace, want)
    # every evaluation is an auto call (the first one finds an empty slot and fills it)
    assert [c["mode"] for c in spy.calls] == ["auto"] * 12
    # and the same decisions forced through fill / reuse give the same latents: the hand-over leaves the buffers as a fill / reuse pair does
    kinds = [k for k, _ in want]
    den = small_cpu[1]
    real = den.forward_nhwc
    it = iter(kinds)

    def forced(x, nb, f, t, cross, **kw):
        slot = kw["deep_cache"]
        kw["deep_cache"] = slot.fill() if next(it) == "key" else slot.reuse()
        return real(x, nb, f, t, cross, **kw)

    fn, _ = _scripted(script)
    AR.install(monkeypatch, fn)
    monkeypatch.setattr(den, "forward_nhwc", forced, raising=False)
    assert torch.equal(pipe.denoise(lat, rl, emb, 12, G, deep_cache_interval=4, deep_cache_threshold=1.0), out)


def test_slot_level_rules_and_report(monkeypatch, small_cpu):
    """forward_nhwc(deep_cache=slot.auto(...)) on its own: an empty slot fills; the slot reports; acc / run live in the store."""
    ref, den, _, _ = small_cpu
    fn, left = _scripted([(1.0, 4.0), (1.0, 4.0), (3.0, 4.0)])
    _install(monkeypatch, fn)
    from mikudance_amd.synth import synth_inputs
    lat, rl, emb = (t.half().float() for t in synth_inputs(2, 16, 16, ctx_len=5, ctx_dim=64, seed=5))
    writer, reader = DR.write_banks(ref, den, rl, emb, 2, 16, 16)
    try:
        x = lat.repeat(2, 1, 1, 1, 1).half()
        slot = DeepCacheSlot(3)
        assert slot.last is None and slot.last_distance is None
        full = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True)
        a = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.auto(1.0, 9))
        assert torch.equal(a, full) and (slot.last, slot.last_distance) == ("key", None) and len(left) == 3
        b = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.auto(1.0, 9))      # the same inputs: replay
        assert torch.equal(b, full) and (slot.last, slot.last_distance, slot.store["acc"], slot.store["run"]) == ("shallow", 0.25, 0.25, 1)
        c = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.auto(1.0, 2))      # the cap of THIS call
        assert torch.equal(c, full) and (slot.last, slot.last_distance, slot.store["acc"], slot.store["run"]) == ("key", 0.25, 0.0, 0)
        d = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.auto(0.75, 9))
        assert torch.equal(d, full) and (slot.last, slot.last_distance) == ("key", 0.75) and not left
        e = DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.reuse())           # a key step leaves a slot reuse can take
        assert torch.equal(e, full)
    finally:
        reader.clear(); writer.clear(); den.clear_context_cache(); ref.clear_context_cache()


# ---- 4. refusals
THR = [(0, "got 0"), (0.0, "got 0.0"), (-1.0, "got -1.0"), (float("nan"), "got nan"), (-math.inf, "got -inf"), ("0.1", "got '0.1'"), (True, "got True")]


@pytest.mark.parametrize("value,msg", THR)
def test_bad_thresholds_are_refused_before_any_unet(value, msg):
    ref, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    with pytest.raises(ValueError, match="deep_cache_threshold must be a number > 0.*" + msg):
        pipe.denoise(*zero_inputs(), 2, G, deep_cache_interval=2, deep_cache_threshold=value)
    assert ref.calls == den.calls == 0


@pytest.mark.parametrize("kw,msg", [(dict(deep_cache_threshold=0.1), "deep_cache_threshold=0.1 needs deep_cache_interval >= 2"),
                                    (dict(deep_cache_threshold=0.1, deep_cache_interval=1), "needs deep_cache_interval >= 2"),
                                    (dict(deep_cache_threshold=0.1, deep_cache_interval=2, guidance_interval=(0.0, 0.5)),
                                     "guidance_interval / uncond_cache_interval cannot be combined with deep_cache"),
                                    (dict(deep_cache_threshold=0.1, deep_cache_interval=2, uncond_cache_interval=2),
                                     "guidance_interval / uncond_cache_interval cannot be combined with deep_cache"),
                                    (dict(deep_cache_threshold=0.1, uncond_cache_interval=2),
                                     "guidance_interval / uncond_cache_interval cannot be combined with deep_cache_threshold"),
                                    (dict(deep_cache_threshold=0.1, deep_cache_interval=0), "deep_cache_interval must be an integer >= 1, got 0")])
def test_loop_refusals_come_before_any_unet(kw, msg):
    ref, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 2, G, **kw)
    assert ref.calls == den.calls == 0


def test_call_refuses_before_clip_and_vae(monkeypatch):
    import numpy as np
    from PIL import Image
    fake_ops.install(monkeypatch)
    ref, den = CountingUNet(), CountingUNet()
    den.in_channels = 4
    vae, clip = fake_ops.FakeVAE(), fake_ops.FakeCLIP()
    ran = []
    monkeypatch.setattr(vae, "encode", lambda x: ran.append("vae"))
    monkeypatch.setattr(clip, "forward", lambda x: ran.append("clip"))
    pipe = M.MikuDanceVideoPipeline(vae=vae, image_encoder=clip, reference_unet=ref, denoising_unet=den, scheduler=_ddim())
    pipe._device = torch.device("cpu")
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 4, G)
    for kw, msg in ((dict(deep_cache_threshold=-0.5, deep_cache_interval=2), "deep_cache_threshold must be a number > 0"),
                    (dict(deep_cache_threshold=0.5), "needs deep_cache_interval >= 2")):
        with pytest.raises(ValueError, match=msg):
            pipe(*args, **kw)
    assert not ran and ref.calls == 0


def test_forward_refusals_of_an_auto_call_come_before_the_first_launch(monkeypatch, small_cpu):
    """Everything _deep_cache_begin refuses for a reuse call, for an auto call on a filled slot."""
    ref, den, _, _ = small_cpu
    _install(monkeypatch)
    from mikudance_amd.synth import synth_inputs
    lat, rl, emb = (t.half().float() for t in synth_inputs(2, 16, 16, ctx_len=5, ctx_dim=64, seed=5))
    writer, reader = DR.write_banks(ref, den, rl, emb, 2, 16, 16)
    try:
        x = lat.repeat(2, 1, 1, 1, 1).half()
        for bad in (0, -1.0, float("nan"), "1", None, True):
            with pytest.raises(ValueError, match="threshold must be a number > 0"):
                DeepCacheSlot(3).auto(bad, 2)
        for bad in (0, -1, 2.0, True, None):
            with pytest.raises(ValueError, match="max_run must be an integer >= 1"):
                DeepCacheSlot(3).auto(0.5, bad)
        slot = DeepCacheSlot(3)
        DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.auto(0.5, 3))
        n = len(fake_ops.CALLS)
        auto = lambda s=slot, d=3: DeepCacheSlot(d, "auto", s.store, 0.5, 3)
        with pytest.raises(ValueError, match="deep_cache_depth.*got 12"):
            DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=auto(d=12))
        with pytest.raises(ValueError, match=r"halves_identical\) = \(2, 2, False, False\), the fill call had \(2, 2, False, True\)"):
            DR.call_nhwc(den, x, 601, emb.half(), deep_cache=auto())
        with pytest.raises(ValueError, match=r"= \(2, 2, True, True\), the fill call had"):
            DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, two_queues=True, deep_cache=auto())
        with pytest.raises(ValueError, match=r"= \(1, 2, False, False\), the fill call had"):
            DR.call_nhwc(den, lat.half(), 601, emb[1:].half(), deep_cache=auto())
        with pytest.raises(ValueError, match=r"the kept buffer \(4, 16, 16, 192\) torch.float16 on cpu does not fit this call, which needs \(4, 8, 8, 192\)"):
            DR.call_nhwc(den, x[..., :8, :8], 601, emb.half(), halves_identical=True, deep_cache=auto())
        with pytest.raises(ValueError, match="does not fit this call"):
            DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=auto(d=4))
        good = slot.store["bufs"][0]
        slot.store["bufs"][0] = good.float()
        with pytest.raises(ValueError, match="torch.float32 on cpu does not fit"):
            DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=auto())
        slot.store["bufs"][0] = good
        with pytest.raises(ValueError, match="an auto slot comes from DeepCacheSlot.auto"):
            DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=DeepCacheSlot(3, "auto", slot.store))
        assert len([c for c in fake_ops.CALLS[n:] if c[0] in ("gemm", "conv", "rel_l1")]) == 0      # every refusal came before the first launch
        DR.call_nhwc(den, x, 601, emb.half(), halves_identical=True, deep_cache=slot.auto(0.5, 3))
        assert slot.last == "shallow"
    finally:
        reader.clear(); writer.clear(); den.clear_context_cache(); ref.clear_context_cache()


# ---- 5. passes and windows
def test_every_free_init_pass_starts_with_a_key_step(monkeypatch, small_cpu):
    _install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 45))
    pipe = _pipe(small_cpu)
    pipe.denoise(lat, rl, emb, 3, G, deep_cache_interval=3, deep_cache_threshold=math.inf, free_init_iters=2, generator=torch.Generator().manual_seed(1))
    trace = pipe.last_deep_cache_trace
    assert [(s, k) for s, _, _, k, _ in trace] == [(0, "key"), (1, "shallow"), (2, "shallow")] * 2
    assert [r is None for *_, r in trace] == [True, False, False] * 2      # an empty slot per pass: its first call measures nothing


def test_every_hires_pass_starts_with_a_key_step(monkeypatch, small_cpu):
    import numpy as np
    from PIL import Image
    hires_ref.install(monkeypatch)
    AR.install(monkeypatch)
    ref, den, _, _ = small_cpu
    pipe = M.MikuDanceVideoPipeline(vae=fake_ops.FakeVAE(), image_encoder=fake_ops.FakeCLIP(), reference_unet=ref, denoising_unet=den, scheduler=_ddim())
    pipe._device = torch.device("cpu")
    pipe.hires_min_side = 48
    traces = []
    real = pipe.denoise

    def denoise(*a, **kw):
        out = real(*a, **kw)
        traces.append(pipe.last_deep_cache_trace)
        return out

    monkeypatch.setattr(pipe, "denoise", denoise, raising=False)
    rng = np.random.default_rng(3)
    img = lambda: Image.fromarray(rng.integers(0, 255, (40, 56, 3), dtype=np.uint8))
    pipe(img(), img(), [img(), img()], [img(), img()], [img(), img()], rng.uniform(-0.5, 0.5, (2, 2, 12, 16)), 128, 96, 2, 4, G,
         generator=torch.Generator().manual_seed(11), hires_scale=2, hires_strength=0.75, deep_cache_interval=2, deep_cache_threshold=math.inf)
    assert [_kinds(t) for t in traces] == [["key", "shallow", "key", "shallow"], ["key", "shallow", "key"]]
    assert [t[0][0] for t in traces] == [0, 0]


def test_a_two_window_clip_has_a_trace_per_window(monkeypatch, small_cpu):
    """Window 1 is scripted to move twice as far as window 0: with threshold 1 it takes its key step one step earlier."""
    calls = [0]

    def rel_l1(a, b, out=None):
        fake_ops.CALLS.append(("rel_l1", None))
        r = torch.tensor((0.5 if calls[0] % 2 == 0 else 1.0, 1.0), dtype=torch.float32)     # windows alternate inside a step
        calls[0] += 1
        if out is None:
            return r
        out.copy_(r)
        return out

    _install(monkeypatch, rel_l1)
    lat, rl, emb = (t.half() for t in small_inputs(4, 46))
    pipe = _pipe(small_cpu)
    pipe.denoise(lat, rl, emb, 4, G, deep_cache_interval=4, deep_cache_threshold=1.0, context_frames=3, context_stride=1, context_overlap=1)
    trace = pipe.last_deep_cache_trace
    assert sorted({w for _, w, _, _, _ in trace}) == [0, 1] and len(trace) == 8
    assert [(s, w) for s, w, _, _, _ in trace] == [(k, w) for k in range(4) for w in (0, 1)]
    assert _kinds(trace, window=0) == ["key", "shallow", "key", "shallow"]      # 0.5, then 1.0 >= 1 -> key, then 0.5
    assert _kinds(trace, window=1) == ["key", "key", "key", "key"]              # 1.0 >= 1 at every step


def test_the_perturbed_plane_decides_on_its_own(monkeypatch, small_cpu):
    calls = [0]

    def rel_l1(a, b, out=None):
        r = torch.tensor((0.25 if calls[0] % 2 == 0 else 1.0, 1.0), dtype=torch.float32)     # main, perturbed, main, ...
        calls[0] += 1
        if out is None:
            return r
        out.copy_(r)
        return out

    _install(monkeypatch, rel_l1)
    lat, rl, emb = (t.half() for t in small_inputs(2, 47))
    pipe = _pipe(small_cpu)
    pipe.denoise(lat, rl, emb, 4, G, deep_cache_interval=4, deep_cache_threshold=1.0, pag_scale=2.0, pag_applied_layers=("down_blocks.0",))
    trace = pipe.last_deep_cache_trace
    assert _kinds(trace, plane=0) == ["key", "shallow", "shallow", "shallow"] and _kinds(trace, plane=1) == ["key"] * 4


def test_script_flag():
    from mikudance_amd import inference_video as IV
    assert IV.parse_args([]).deep_cache_threshold is None
    assert IV.parse_args(["--deep_cache_interval", "5", "--deep_cache_threshold", "0.15"]).deep_cache_threshold == 0.15
    with pytest.raises(SystemExit):
        IV.parse_args(["--deep_cache_threshold", "much"])
    assert "deep_cache_threshold=--deep_cache_threshold" in IV.__doc__
