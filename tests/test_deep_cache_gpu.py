"""GPU: DeepCache (deep_cache_interval=, deep_cache_depth=; forward_nhwc(deep_cache=)) on the MI355X.  A shallow step launches only kernels that
the full step launches at the same shapes, so what is tested is the host graph on the device: which buffer is kept, what is read from it, on which
stream.

Bounds.  Replay (fill, then reuse on the same inputs): bitwise the full call of the same path, run to run bitwise.  Reuse on other inputs against
tests/deepcache_ref.py (fp32): rel-L2 <= 3e-2 and cosine >= 0.999, the project's UNet bound, AND rel-L2 <= 2 x the error the plain full forward has
against the oracle on the same (x2, t2), measured in the same test (the margin rule of tests/golden/parity_budget.json).  Loops against the CPU
emulation of the same loop (the pipeline on tests/fake_ops.py): rel-L2 <= 3e-2 and cosine >= 0.999, the loop bound of the other option tests.
profiles/deep_cache_tests.log holds every printed figure of a run on an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import DeepCacheSlot  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

import deepcache_ref as DR  # noqa: E402
import fake_ops  # noqa: E402

DEV = torch.device("cuda:0")
G, F_, STEPS = 3.5, 2, 4


@pytest.fixture(scope="module")
def small():
    return build_models()


@pytest.fixture(scope="module")
def small_host():
    return build_models(device="cpu", keep_state_dicts=False)


def _inputs(seed, f=F_, h=16, w=16):
    return tuple(t.half().float() for t in synth_inputs(f, h, w, ctx_len=5, ctx_dim=64, seed=seed))


def _two(lat):
    return lat.repeat(2, 1, 1, 1, 1).half().to(DEV)


class _Banks:
    """The reference banks of (rl, emb) in the denoising UNet's blocks for the duration of a with block."""

    def __init__(self, models, rl, emb, h, w):
        self.models, self.args = models, (rl, emb, F_, h, w)

    def __enter__(self):
        ref, den = self.models[:2]
        self.wr = DR.write_banks(ref, den, *self.args, device=DEV)

    def __exit__(self, *exc):
        ref, den = self.models[:2]
        for c in self.wr:
            c.clear()
        den.clear_context_cache()
        ref.clear_context_cache()


# ---- 1. replay
@pytest.mark.parametrize("two_queues", [False, True])
@pytest.mark.parametrize("d", [1, 3, 4])
def test_replay_is_bitwise_the_full_call_and_repeatable(small, d, two_queues):
    den = small[1]
    lat, rl, emb = _inputs(5)
    x, e = _two(lat), emb.half().to(DEV)
    kw = dict(halves_identical=True, two_queues=two_queues)
    with _Banks(small, rl, emb, 16, 16):
        DR.call_nhwc(den, x, 601, e, **kw)                                 # (the first two-queue call of a shape runs its queues one after the other)
        full = DR.call_nhwc(den, x, 601, e, **kw)
        runs = []
        for _ in range(2):
            slot = DeepCacheSlot(d)
            a = DR.call_nhwc(den, x, 601, e, deep_cache=slot, **kw)
            b = DR.call_nhwc(den, x, 601, e, deep_cache=slot.reuse(), **kw)
            c = DR.call_nhwc(den, x, 601, e, deep_cache=slot.reuse(), **kw)
            assert sorted(slot.store["bufs"]) == ([0, 1] if two_queues else [0])
            runs.append((a, b, c))
            slot.drop()
    assert torch.isfinite(full).all()
    for a, b, c in runs:
        assert torch.equal(a, full) and torch.equal(b, full) and torch.equal(c, full)


# ---- 2. reuse on other inputs against the fp32 restatement
@pytest.mark.parametrize("hw,d,two_queues", [((16, 16), 3, False), ((16, 16), 3, True), ((16, 16), 1, False), ((16, 16), 4, False), ((12, 20), 7, False),
                                             ((12, 20), 4, True)])
def test_shallow_step_matches_the_literal_reference(small, hw, d, two_queues):
    ref, den, ref_sd, den_sd = small
    h, w = hw
    lat1, rl, emb = _inputs(5, h=h, w=w)
    lat2 = _inputs(6, h=h, w=w)[0]
    t1, t2 = 601, 401
    e = emb.half().to(DEV)
    kw = dict(halves_identical=True, two_queues=two_queues)
    with _Banks(small, rl, emb, h, w):
        slot = DeepCacheSlot(d)
        DR.call_nhwc(den, _two(lat1), t1, e, deep_cache=slot, **kw)
        got = DR.call_nhwc(den, _two(lat2), t2, e, deep_cache=slot.reuse(), **kw)
        plain = DR.call_nhwc(den, _two(lat2), t2, e, **kw)
    banks = DR.oracle_banks(ref_sd, rl, emb, F_, h, w)
    with torch.no_grad():
        _, hidden = DR.full(den_sd, lat1.repeat(2, 1, 1, 1, 1), torch.tensor(t1), emb, banks)
        want = DR.shallow(den_sd, lat2.repeat(2, 1, 1, 1, 1), torch.tensor(t2), emb, banks, True, d, hidden[d - 1])
        want_full, _ = DR.full(den_sd, lat2.repeat(2, 1, 1, 1, 1), torch.tensor(t2), emb, banks)
    r, c, r0 = rel_l2(got, want), cosine(got, want), rel_l2(plain, want_full)
    print(f"\nDEEPCACHE_UNET {h}x{w} d{d} two_queues {two_queues}: rel_l2 {r:.3e} cos {c:.7f} (plain full forward vs oracle {r0:.3e}, ratio {r / r0:.2f}; "
          f"shallow vs full reference {rel_l2(want, want_full):.3e})")
    assert torch.isfinite(got).all() and r <= 3e-2 and c >= 0.999, (r, c)
    assert r <= 2.0 * r0, (r, r0)


# ---- 3-5. the loop
def _make(sampler):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS) if sampler == "2m" else M.DDIMScheduler(**SCHED_KWARGS)


def _loop(models, inputs, sampler="ddim", device=DEV, **kw):
    ref, den = models[:2]
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _make(sampler))
    out = pipe.denoise(*(t.half().to(device) for t in inputs), STEPS, G, **kw)
    if device != "cpu":
        torch.cuda.synchronize()
    return out.float().cpu()


def _emulated(small_host, inputs, sampler, **kw):
    """The same loop on the emulated operators on the host."""
    import tile_ref
    with pytest.MonkeyPatch.context() as mp:
        fake_ops.install(mp)
        tile_ref.install(mp)
        return _loop(small_host, inputs, sampler, device="cpu", **kw)


def test_interval_one_is_bitwise_the_plain_loop(small):
    inputs = _inputs(504)
    a = _loop(small, inputs)
    b = _loop(small, inputs, deep_cache_interval=1)
    c = _loop(small, inputs, deep_cache_interval=1, deep_cache_depth=6)
    d = _loop(small, inputs, deep_cache_interval=2)
    assert torch.equal(a, b) and torch.equal(a, c) and not torch.equal(a, d)
    print(f"\nDEEPCACHE_EFFECT rel_l2(N 2 d 3, plain) {rel_l2(d, a):.3e}")


CASES = {"ddim": ("ddim", {}), "2m": ("2m", {}), "kv2-tile2": ("ddim", dict(kv_downsample=2, tile_attention=2)),
         "seg": ("ddim", dict(seg_scale=2.0, seg_blur_sigma=1.5, seg_applied_layers=("down_blocks.0", "mid"))),
         "two-windows": ("ddim", dict(context_frames=3, context_stride=1, context_overlap=1))}


@pytest.mark.parametrize("case", list(CASES))
def test_loop_matches_the_emulated_loop(small, small_host, case):
    sampler, kw = CASES[case]
    inputs = _inputs(504, f=4 if case == "two-windows" else F_)
    kw = dict(kw, deep_cache_interval=2, deep_cache_depth=3)
    want = _emulated(small_host, inputs, sampler, **kw)
    got = _loop(small, inputs, sampler, **kw)
    e, c = rel_l2(got, want), cosine(got, want)
    print(f"\nDEEPCACHE_LOOP {case} {STEPS} steps N 2 d 3: rel_l2 {e:.3e} cos {c:.7f}")
    assert torch.isfinite(got).all() and e <= 3e-2 and c >= 0.999, (e, c)


def test_loop_on_two_queues_matches_the_emulated_loop(small, small_host):
    inputs = _inputs(504)
    kw = dict(deep_cache_interval=2, deep_cache_depth=3)
    want = _emulated(small_host, inputs, "ddim", **kw)
    ref, den = small[:2]
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _make("ddim"))
    pipe.two_queues = True
    outs = []
    for _ in range(2):
        outs.append(pipe.denoise(*(t.half().to(DEV) for t in inputs), STEPS, G, **kw).float().cpu())
    e, c = rel_l2(outs[0], want), cosine(outs[0], want)
    print(f"\nDEEPCACHE_LOOP two-queues {STEPS} steps N 2 d 3: rel_l2 {e:.3e} cos {c:.7f}")
    assert torch.equal(outs[0], outs[1]) and e <= 3e-2 and c >= 0.999, (e, c)
