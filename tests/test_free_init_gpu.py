"""GPU: FreeInit noise re-initialisation on the MI355X -- md_free_init_mix_f16 against diffusers' literal form in float64
(tests/free_init_ref.py: mix_literal) on a random symmetric table and on the three real filters, its exact cases (a table of zeros, a table
of ones, out aliasing x0, a == 0, run to run), its argument checks, and the loop at reduced width with free_init_iters=2 against the CPU
oracle composed with the literal mix.

Bound of the kernel tests, per element: half an fp16 ulp of the reference value (the one rounding on the way out) plus A, where A is
4 x the largest error of the dense per-axis DFT restated in float32 (mix_dense) against mix_literal on that very case -- computed here from
the references alone; the factor 4 allows for another summation order.  profiles/free_init_tests.log: measured maximum over bound per case."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import free_init as FI  # noqa: E402
from mikudance_amd import ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

import free_init_ref as FR  # noqa: E402

DEV = torch.device("cuda:0")
AB = (math.sqrt(0.0047), math.sqrt(1.0 - 0.0047))     # abar_999 of SD's plain scaled-linear table; the zero-SNR table of this model has a = 0
# distinct lengths per axis (an axis mix-up fails); 65, 130, 33 cross wave and tile boundaries; 256 is the cap; one clip of bench size
SHAPES = [(1, 8, 8), (2, 2, 2), (5, 6, 9), (3, 7, 10), (16, 12, 12), (7, 65, 3), (2, 3, 130), (33, 20, 5), (256, 2, 3), (2, 3, 256), (2, 256, 3),
          (16, 96, 96)]
_REF = {}


def _case(shape, table, ab=AB):
    """(x0, noise0, z, lpf, want, A) of a case, computed once: table = "random" | "ones" | a filter name."""
    key = (shape, table, ab)
    if key not in _REF:
        x0, n0, z = FR.random_case(*shape, seed=sum(shape))
        if table == "random":
            lpf = FR.random_symmetric_table(*shape, seed=sum(shape) + 1)
        elif table == "ones":
            lpf = np.ones(shape, dtype=np.float32)
        else:
            lpf = FI.freq_filter(*shape, table, 4, 0.25, 0.25).numpy()
        want = FR.mix_literal(x0, n0, z, *ab, FR.shifted(lpf))
        dense = FR.mix_dense(x0.numpy(), n0.numpy(), z.numpy(), *ab, lpf, np.float32)
        _REF[key] = (x0, n0, z, torch.from_numpy(lpf), want, 4.0 * float(np.abs(dense - want.numpy()).max()))
    return _REF[key]


def _mix(x0, n0, z, lpf, a, b, alias=False):
    xd = x0.to(DEV)
    out = xd if alias else torch.full_like(xd, float("nan"))
    ops.free_init_mix(out, xd, n0.to(DEV), z.to(DEV), lpf.to(DEV), a, b)
    torch.cuda.synchronize()
    return out.cpu()


def _check(tag, got, want, A):
    err = (got.double() - want).abs()
    bound = FR.half_ulp_f16(want) + A
    worst = float((err / bound).max())
    over = float(((err - FR.half_ulp_f16(want)) / A).max())             # the share of A in use: <= 1 passes, <= 0 is the rounding alone
    print(f"\nFREE_INIT_KERNEL {tag}: max |err| {float(err.max()):.3e}  A {A:.3e}  max err / bound {worst:.3f}  max (err - half ulp) / A {over:.3f}")
    assert torch.isfinite(got).all() and got.shape == want.shape and bool((err <= bound).all()), worst


# ---- 1. the kernel against the literal form
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_literal_on_a_random_table(shape):
    x0, n0, z, lpf, want, A = _case(shape, "random")
    _check(f"random table {shape}", _mix(x0, n0, z, lpf, *AB), want, A)


def test_kernel_matches_literal_with_a_large_a():
    ab = (0.6, 0.8)
    x0, n0, z, lpf, want, A = _case((5, 6, 9), "random", ab)
    _check("random table (5, 6, 9) a = 0.6", _mix(x0, n0, z, lpf, *ab), want, A)


@pytest.mark.parametrize("kind", ["butterworth", "gaussian", "ideal"])
@pytest.mark.parametrize("shape", [(16, 12, 12), (5, 6, 9)], ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_literal_on_the_real_filters(shape, kind):
    x0, n0, z, lpf, _, A = _case(shape, kind)
    want = FR.mix_literal(x0, n0, z, *AB, FR.lpf_literal(*shape, kind, 4, 0.25, 0.25))       # diffusers' own, unsymmetrised table
    _check(f"{kind} {shape}", _mix(x0, n0, z, lpf, *AB), want, A)


# ---- 2. exact cases
def test_a_table_of_zeros_returns_z_bit_for_bit():
    for shape in [(5, 6, 9), (16, 12, 12), (2, 3, 130)]:
        x0, n0, z, _, _, _ = _case(shape, "random")
        assert torch.equal(_mix(x0, n0, z, torch.zeros(shape), *AB), z)


@pytest.mark.parametrize("shape", [(5, 6, 9), (16, 12, 12)], ids=lambda s: "x".join(map(str, s)))
def test_a_table_of_ones_returns_the_renoised_sample(shape):
    x0, n0, z, lpf, want, A = _case(shape, "ones")
    direct = AB[0] * x0.double() + AB[1] * n0.double()                     # z drops out
    assert float((want - direct).abs().max()) < 1e-12
    _check(f"ones {shape}", _mix(x0, n0, z, lpf, *AB), direct, A)


def test_out_may_alias_x0_and_runs_are_bitwise_equal():
    for shape in [(3, 7, 10), (33, 20, 5)]:
        x0, n0, z, lpf, _, _ = _case(shape, "random")
        first = _mix(x0, n0, z, lpf, *AB)
        assert torch.equal(first, _mix(x0, n0, z, lpf, *AB))
        assert torch.equal(first, _mix(x0, n0, z, lpf, *AB, alias=True))


def test_a_zero_never_reads_x0():
    shape = (5, 6, 9)
    x0, n0, z, lpf, _, A = _case(shape, "random", (0.0, 1.0))
    bad = torch.full_like(x0, float("nan"))
    bad[::2] = float("inf")
    got = _mix(bad, n0, z, lpf, 0.0, 1.0)
    want = FR.mix_literal(bad, n0, z, 0.0, 1.0, FR.shifted(lpf.numpy()))
    _check("a = 0, NaN / Inf in x0", got, want, A)
    assert not torch.isfinite(_mix(bad, n0, z, lpf, 0.5, 0.5)).any()       # a != 0: x0 is read, and one NaN reaches every frequency


# ---- 3. argument checks
def test_plan_is_zero_exactly_outside_the_range():
    plan = M._lib.load().md_free_init_plan
    for v, ok in [(-1, 0), (0, 0), (1, 1), (2, 1), (255, 1), (256, 1), (257, 0), (1 << 20, 0)]:
        assert plan(v, 4, 4) == ok and plan(4, v, 4) == ok and plan(4, 4, v) == ok, v
    assert M._lib.load().md_free_init_workspace_bytes(257, 4, 4) == 0
    assert M._lib.load().md_free_init_workspace_bytes(2, 3, 5) >= 2 * 3 * 5 * 4 * 8


def test_kernel_refuses_bad_arguments():
    F, H, W = 2, 3, 5
    lib = M._lib.load()
    t = [torch.zeros((F, H, W, 4), device=DEV, dtype=torch.float16) for _ in range(4)]
    lpf = torch.zeros((F, H, W), device=DEV, dtype=torch.float32)
    need = lib.md_free_init_workspace_bytes(F, H, W)
    ws = torch.zeros((need + 64) // 4, device=DEV, dtype=torch.float32)
    o, x, n, z = (v.data_ptr() for v in t)
    l, w, st = lpf.data_ptr(), ws.data_ptr(), ops._st()
    good = (o, x, n, z, l, F, H, W, 0.5, 0.5, w, need, st)
    assert lib.md_free_init_mix_f16(*good) == 0

    def with_(**kw):
        names = ("out", "x0", "noise0", "z", "lpf", "F", "H", "W", "a", "b", "ws", "bytes", "st")
        return tuple(kw.get(k, v) for k, v in zip(names, good))

    for args in (with_(F=257), with_(H=0), with_(W=-3), with_(bytes=need - 1), with_(bytes=0), with_(out=o + 2), with_(x0=x + 4), with_(noise0=n + 2),
                 with_(z=z + 6), with_(lpf=l + 2), with_(ws=w + 8), with_(out=0), with_(x0=0), with_(noise0=0), with_(z=0), with_(lpf=0), with_(ws=0),
                 with_(a=float("nan")), with_(b=float("inf")), with_(a=-0.5), with_(b=-0.5)):
        with pytest.raises(M._lib.MdanceHipError, match="md_free_init_mix_f16"):
            M._lib.call("md_free_init_mix_f16", *args)
        assert lib.md_free_init_mix_f16(*args) == -1                        # MD_ERR_ARG
    torch.cuda.synchronize()
    big = torch.zeros((257, 1, 1, 4), device=DEV, dtype=torch.float16)
    with pytest.raises(M._lib.MdanceHipError, match="no kernel"):
        ops.free_init_mix(big, big, big, big, torch.zeros((257, 1, 1), device=DEV), 0.5, 0.5)
    with pytest.raises(M._lib.MdanceHipError):
        ops.free_init_mix(t[0], t[1], t[2], t[3], lpf.half(), 0.5, 0.5)


# ---- 4. the loop
@pytest.fixture(scope="module")
def small():
    return build_models()


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _inputs(frames, seed):
    return tuple(t.half().float() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=seed))


def _loop(sch, models, inputs, steps, seed=None, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    gen = torch.Generator().manual_seed(seed) if seed is not None else None
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, 3.5, generator=gen, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def test_loop_vs_cpu_oracle_reduced_width(small):
    _, _, ref_sd, den_sd = small
    inputs = _inputs(4, 91)
    out = _loop(_ddim(), small, inputs, 4, seed=23, free_init_iters=2)
    one = _loop(_ddim(), small, inputs, 4, seed=23)
    with torch.no_grad():
        want = FR.denoise_loop(ref_sd, den_sd, *inputs, 4, 2, torch.Generator().manual_seed(23), guidance_scale=3.5, reduced=True)
    r, c = rel_l2(out, want), cosine(out, want)
    print(f"\nFREE_INIT_LOOP ddim 2 passes of 4 steps, 4 frames 16x16: rel_l2 {r:.3e} cos {c:.7f} (iters=2 from iters=1: {rel_l2(out, one):.3e})")
    assert torch.isfinite(out).all() and r <= 3e-2 and c >= 0.999, (r, c)
    assert rel_l2(out, one) > 0.3                                        # ten times the bound: the second pass is not a no-op


@pytest.mark.parametrize("sampler", ["ddim", "ddim-eta", "2m", "2m-sde"])
def test_one_iteration_is_bitwise_the_plain_loop(small, sampler):
    make = _ddim if sampler.startswith("ddim") else (lambda: _dpm(algorithm_type="sde-dpmsolver++" if sampler == "2m-sde" else "dpmsolver++"))
    kw = dict(eta=0.5) if sampler == "ddim-eta" else {}
    inputs = _inputs(4, 92)
    a = _loop(make(), small, inputs, 3, seed=29, **kw)
    b = _loop(make(), small, inputs, 3, seed=29, free_init_iters=1, free_init_filter="ideal", free_init_order=2, free_init_spatial_stop=0.5,
              free_init_temporal_stop=0.1, free_init_fast=True, **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_two_iterations_with_dpm_solver_run_and_differ(small):
    inputs = _inputs(4, 93)
    a = _loop(_dpm(), small, inputs, 3, seed=31)
    b = _loop(_dpm(), small, inputs, 3, seed=31, free_init_iters=2, free_init_fast=True)
    assert torch.isfinite(b).all() and rel_l2(b, a) > 0.3
