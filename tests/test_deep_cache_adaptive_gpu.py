"""GPU: adaptive DeepCache (deep_cache_threshold=) on the MI355X, on the small UNets and the 16 x 16 latents of tests/test_deep_cache_gpu.py,
4 frames in 2 windows, 4 steps.  Every comparison is BITWISE: an auto call launches the kernels of a fill or of a reuse call at the same
shapes, plus md_rel_l1_f16 and one copy, so the two ends of the threshold are the fixed rule and the plain loop, and a run in between is the
run in which the same key / shallow pattern is forced through the fill / reuse modes -- which pins the buffer hand-over and the single copy."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

DEV = torch.device("cuda:0")
G, FRAMES, STEPS, CAP = 3.5, 4, 4, 4
WINDOWS = dict(context_frames=3, context_stride=1, context_overlap=1)      # 4 frames: 2 windows


@pytest.fixture(scope="module")
def small():
    return build_models()


@pytest.fixture(scope="module")
def inputs():
    return tuple(t.half().to(DEV) for t in synth_inputs(FRAMES, 16, 16, ctx_len=5, ctx_dim=64, seed=504))


def _run(small, inputs, two_queues=False, forced=None, **kw):
    """denoise() -> (latents on the host, the trace).  forced: the (step, window) -> "key" | "shallow" pattern to push through the fill / reuse
    modes, whatever slot the loop hands to forward_nhwc."""
    ref, den = small[:2]
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    pipe.two_queues = two_queues
    real = den.forward_nhwc
    if forced is not None:
        todo = list(forced)

        def forward_nhwc(x, nb, f, t, cross, **k):
            slot = k["deep_cache"]
            k["deep_cache"] = slot.fill() if todo.pop(0) == "key" else slot.reuse()
            return real(x, nb, f, t, cross, **k)

        den.forward_nhwc = forward_nhwc
    try:
        out = pipe.denoise(*inputs, STEPS, G, **WINDOWS, **kw)
    finally:
        if forced is not None:
            del den.forward_nhwc
    torch.cuda.synchronize()
    return out.float().cpu(), pipe.last_deep_cache_trace


def _mid_threshold(trace):
    """A threshold between window 0's first distance and the sum of its first two, read from a run whose first three steps are key, shallow,
    shallow (threshold inf, cap 4): a run under it measures the same two distances (its steps 0 and 1 are the same evaluations), so window 0's
    step 1 stays shallow (r1 < T) and its step 2 becomes a key step (r1 + r2 >= T)."""
    r = {(s, w): d for s, w, _, _, d in trace}
    r1, r2 = r[(1, 0)], r[(2, 0)]
    assert math.isfinite(r1) and math.isfinite(r2) and r1 > 0 and r2 > 0, (r1, r2)
    return r1 + 0.5 * r2


@pytest.mark.parametrize("two_queues", [False, True], ids=["one-queue", "two-queues"])
def test_adaptive_runs_are_bitwise_their_forced_twins(small, inputs, two_queues):
    kw = dict(two_queues=two_queues)
    plain, none = _run(small, inputs, **kw)
    assert none is None
    # threshold inf: the cap rule, bitwise the fixed rule
    fixed, tf = _run(small, inputs, deep_cache_interval=2, **kw)
    got, ti = _run(small, inputs, deep_cache_interval=2, deep_cache_threshold=math.inf, **kw)
    assert [(s, w, p, k) for s, w, p, k, _ in ti] == [(s, w, p, k) for s, w, p, k, _ in tf] == [(s, w, 0, "key" if s % 2 == 0 else "shallow")
                                                                                                 for s in range(STEPS) for w in (0, 1)]
    assert torch.isfinite(got).all() and torch.equal(got, fixed) and not torch.equal(got, plain)
    # a tiny threshold: every step a key step, bitwise the plain loop
    got, tt = _run(small, inputs, deep_cache_interval=CAP, deep_cache_threshold=1e-30, **kw)
    assert [k for *_, k, _ in tt] == ["key"] * (2 * STEPS) and torch.equal(got, plain)
    # a threshold in between, from the distances the cap-only run reports
    _, tc = _run(small, inputs, deep_cache_interval=CAP, deep_cache_threshold=math.inf, **kw)
    thr = _mid_threshold(tc)
    mid, tm = _run(small, inputs, deep_cache_interval=CAP, deep_cache_threshold=thr, **kw)
    kinds = [k for *_, k, _ in tm]
    print(f"\nDEEPCACHE_ADAPTIVE two_queues {two_queues}: threshold {thr:.4f}; " + " ".join(f"{s}/{w}:{k[0]}:{'-' if d is None else format(d, '.4f')}"
                                                                                            for s, w, _, k, d in tm))
    assert "shallow" in kinds and "key" in kinds[2:], tm                   # both kinds behind the first step
    assert [k for s, w, _, k, _ in tm if w == 0][:3] == ["key", "shallow", "key"]
    forced, _ = _run(small, inputs, deep_cache_interval=CAP, forced=kinds, **kw)
    assert torch.isfinite(mid).all() and torch.equal(mid, forced)
    # run to run: the same trace, the same bits
    again, ta = _run(small, inputs, deep_cache_interval=CAP, deep_cache_threshold=thr, **kw)
    assert ta == tm and torch.equal(again, mid)
