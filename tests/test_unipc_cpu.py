"""CPU: UniPC sampling (mikudance_amd.UniPCMultistepScheduler, sampler "unipc") without a GPU -- the coefficient rows against the independent
float64 restatement tests/unipc_ref.py, two identities that need no reference (order 1 is DDIM, order 2 without the corrector is DPM-Solver++
2M midpoint), convergence on a problem with a closed-form solution, the rule by which the kernel moves its history planes, what the loop asks
of the operators (tests/fake_ops.py and the three emulations of tests/unipc_ref.py), the refusals, and the emulated loop against the oracle."""
import math

import numpy as np
import pytest
import torch

import mikudance_amd as M
from mikudance_amd.selftest import SCHED_KWARGS

import fake_ops
import unipc_ref as R
from loop_helpers import CountingUNet, rel_l2, small_cpu, small_inputs, zero_inputs  # noqa: F401
from test_sampling_loop_calls_cpu import GUIDES, LOOPS, _inputs8, assert_same, trace_loops

NS = [1, 2, 3, 5, 10, 20, 50]


def _sched(zero_snr=True, **kw):
    return M.UniPCMultistepScheduler(**dict(SCHED_KWARGS, rescale_betas_zero_snr=zero_snr), **kw)


def _rows(n, begin=0, **kw):
    s = _sched(**kw)
    s.set_timesteps(n)
    if begin:
        s.set_begin_index(begin)
    return [s.unipc_coefficients(i) for i in range(n)]


def _close(a, b, rel):
    return (a == 0.0 and b == 0.0) or (a != 0.0 and b != 0.0 and abs(a - b) <= rel * max(abs(a), abs(b)))


# ---- 1. the tables
@pytest.mark.parametrize("zero_snr", [True, False], ids=["zsnr", "finite"])
@pytest.mark.parametrize("solver", ["bh1", "bh2"])
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("n", NS)
def test_rows_match_the_restatement(n, order, solver, zero_snr):
    """<= 1e-10 relative per entry, 0 against 0 exactly, the corrector flag the same, everything finite; begin_index 0, 1, n - 1 and a
    disable_corrector list."""
    worst = 0.0
    for begin in sorted({0, min(1, n - 1), n - 1}):
        for off in ((), (1, 2, n - 1)):
            got = _rows(n, begin, zero_snr=zero_snr, solver_order=order, solver_type=solver, disable_corrector=off)
            want = R.coefficients(n, order, solver, zero_snr, begin, off)
            assert len(got) == len(want) == n
            for i, (g, w) in enumerate(zip(got, want)):
                assert len(g) == len(w) == 12 and g[11] is w[11], (begin, off, i, g, w)
                assert all(isinstance(v, float) and math.isfinite(v) for v in g[:11]), (i, g)
                for k in range(11):
                    assert _close(g[k], w[k], 1e-10), (begin, off, i, k, g[k], w[k])
                    if g[k]:
                        worst = max(worst, abs(g[k] - w[k]) / abs(w[k]))
                if not g[11]:
                    assert g[2:7] == (0.0,) * 5
    print(f"\nUNIPC_TABLE n={n} order={order} {solver} zero_snr={zero_snr}: worst relative difference {worst:.3e}")


def test_the_rules_of_the_table():
    """No corrector at step 0, at begin_index, on a disabled step; the corrector's order is the previous predictor's; the last step is first
    order and lands on m_t; t = 999 under zero terminal SNR is no history point; bh1 has no corrector out of it, bh2 has."""
    n = 10
    rows = _rows(n, solver_order=3, disable_corrector=(4,))
    on = [r[11] for r in rows]
    assert on == [False, True, True, True, False, True, True, True, True, True]
    po = [1 + (r[9] != 0.0) + (r[10] != 0.0) for r in rows]
    assert po == R.orders(n, 3) == [1, 1, 2, 3, 3, 3, 3, 3, 2, 1]                     # step 1: its only history is the lambda = -inf point
    co = [(r[4] != 0.0) + (r[5] != 0.0) + (r[6] != 0.0) for r in rows]
    assert [c for c, o in zip(co, on) if o] == [po[i - 1] for i in range(n) if on[i]]
    assert rows[-1][7:11] == (0.0, 1.0, 0.0, 0.0)
    assert _rows(n, solver_order=3, solver_type="bh1")[1][11] is False and _rows(n, solver_order=3, solver_type="bh2")[1][11] is True
    assert R.orders(n, 3, zero_snr=False) == [1, 2, 3, 3, 3, 3, 3, 3, 2, 1]
    b = _rows(n, 5, solver_order=3)                                          # a start at step 5: up by one a step, down with the steps left
    assert b[5][11] is False and [1 + (r[9] != 0.0) + (r[10] != 0.0) for r in b[5:]] == [1, 2, 3, 2, 1] and all(r[11] for r in b[6:])


@pytest.mark.parametrize("zero_snr", [True, False], ids=["zsnr", "finite"])
@pytest.mark.parametrize("solver", ["bh1", "bh2"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_every_plane_a_row_reads_holds_the_right_step(order, solver, zero_snr):
    """The kernel reads a plane only where a weight is non-zero and moves down only what it read (tests/unipc_ref.row_update states the rule).
    Followed with labels instead of data: whenever a row gives H_k a weight, H_k holds the data prediction of step i - 1 - k, and x_last the
    corrected sample of step i - 1, from an empty state, for every n, start and disable_corrector list."""
    for n in NS:
        for begin in sorted({0, min(1, n - 1), n // 2, n - 1}):
            for off in ((), (1, 2, n - 1), tuple(range(n))):
                rows = _rows(n, begin, zero_snr=zero_snr, solver_order=order, solver_type=solver, disable_corrector=off)
                xl, H = None, [None, None, None]
                for i in range(begin, n):
                    r = rows[i]
                    if r[11]:
                        assert xl == i - 1, (n, begin, off, i)
                    for k, (cw, pw) in enumerate(((r[4], r[9]), (r[5], r[10]), (r[6], 0.0))):
                        if cw != 0.0 or pw != 0.0:
                            assert H[k] == i - 1 - k, (n, begin, off, i, k, H)
                    rd0, rd1 = r[4] != 0.0 or r[9] != 0.0, r[5] != 0.0 or r[10] != 0.0
                    xl, H = i, [i, H[0] if rd0 else H[1], H[1] if rd1 else H[2]]


# ---- 2. identities that need no reference
@pytest.mark.parametrize("n", [1, 2, 5, 10, 20, 50])
def test_order_1_predictor_is_ddim(n):
    """Order 1, bh2, no corrector: x' = pc_x x + pc_m m_t is DDIM's eta = 0 update, which in (x, m_t = x0) reads
    sqrt(1 - a_prev) / sqrt(1 - a_t) x + (sqrt(a_prev) - sqrt(1 - a_prev) sqrt(a_t) / sqrt(1 - a_t)) x0.  n divides 1000: DDIM's prev_t = t - 1000 // n
    is then the next entry of the trailing list."""
    d = M.DDIMScheduler(**SCHED_KWARGS)
    d.set_timesteps(n)
    rows = _rows(n, solver_order=1, disable_corrector=tuple(range(n)))
    for i, t in enumerate(d.timesteps.tolist()):
        a_t, a_p = d.step_coefficients(t)
        sa, sb, sap, sdir = math.sqrt(a_t), math.sqrt(1.0 - a_t), math.sqrt(a_p), math.sqrt(1.0 - a_p)
        r = rows[i]
        assert not r[11] and r[9] == r[10] == 0.0
        assert _close(r[7], sdir / sb, 1e-12) and _close(r[8], sap - sdir * sa / sb, 1e-12), (i, r[7:9], sdir / sb, sap - sdir * sa / sb)


@pytest.mark.parametrize("zero_snr", [True, False], ids=["zsnr", "finite"])
@pytest.mark.parametrize("n", NS)
def test_order_2_predictor_is_dpm_solver_2m_midpoint(n, zero_snr):
    kw = dict(SCHED_KWARGS, rescale_betas_zero_snr=zero_snr)
    d = M.DPMSolverMultistepScheduler(**kw, solver_type="midpoint")
    d.set_timesteps(n)
    rows = _rows(n, zero_snr=zero_snr, solver_order=2, disable_corrector=tuple(range(n)))
    for i in range(n):
        a_s, s_s, c_x, c_m0, c_m1, c_z = d.multistep_coefficients(i)
        r = rows[i]
        assert c_z == 0.0 and r[10] == 0.0 and not r[11]
        for g, w in zip((r[0], r[1], r[7], r[8], r[9]), (a_s, s_s, c_x, c_m0, c_m1)):
            assert _close(g, w, 1e-12), (i, g, w)


# ---- 3. a problem with a closed-form solution
def _gaussian_error(n, order, corrector, solver="bh2", mu=0.7, s=0.5):
    """x0 ~ N(mu, s^2) per element: E[x0 | x_t] = mu + alpha s^2 / (alpha^2 s^2 + sigma^2) (x_t - alpha mu), the optimal v is
    alpha eps_hat - sigma x0_hat with eps_hat = (x_t - alpha x0_hat) / sigma, and the probability-flow ODE has the solution
    x_t = alpha_t mu + sqrt(alpha_t^2 s^2 + sigma_t^2) / sqrt(alpha_T^2 s^2 + sigma_T^2) (x_T - alpha_T mu) -> relative L2 of the sampler's end."""
    sch = R.Restated(order, solver, zero_snr=False, disable_corrector=() if corrector else tuple(range(n)))
    ts = sch.set_timesteps(n)
    x = xT = torch.randn((4, 64), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for i, t in enumerate(ts.tolist()):
        a, sg = float(sch.alpha[i]), float(sch.sigma[i])
        x0 = mu + a * s * s / (a * a * s * s + sg * sg) * (x - a * mu)
        x = sch.step(a * (x - a * x0) / sg - sg * x0, t, x)
    aT, sT = float(sch.alpha[0]), float(sch.sigma[0])
    want = mu + s / math.sqrt(aT * aT * s * s + sT * sT) * (xT - aT * mu)
    return rel_l2(x, want)


def test_convergence_on_the_gaussian_problem():
    ns = [5, 10, 20, 40]
    err = {(o, c): [_gaussian_error(n, o, c) for n in ns] for o in (1, 2, 3) for c in (True, False)}
    for (o, c), e in err.items():
        print(f"\nUNIPC_GAUSSIAN order {o} corrector {'on' if c else 'off'}: rel-L2 at n = {ns}: " + ", ".join(f"{v:.3e}" for v in e)
              + "; ratios " + ", ".join(f"{a / b:.2f}" for a, b in zip(e, e[1:])))
    for o in (1, 2, 3):
        e = err[(o, True)]
        assert all(a > b for a, b in zip(e, e[1:])), (o, e)                  # falls monotonically with n, corrector on
    for k in (1, 2):                                                         # n = 10, 20: UniPC-2 beats order 1 without corrector (DDIM)
        assert err[(2, True)][k] < err[(1, False)][k], (ns[k], err[(2, True)][k], err[(1, False)][k])


# ---- 4. what the loop asks of the operators
def _unipc_loop(monkeypatch, small, guidance=3.5, frames=2, steps=4, init=False, sched_kw=None, allocs=None, **kw):
    """One denoise() under UniPC on the emulated operators -> (the cfg_* records, the output)."""
    R.install(monkeypatch)
    ref, den, _, _ = small
    lat, rl, emb = _inputs8(frames, 300 + frames)
    if init:
        kw["init_latents"] = _inputs8(frames, 400 + frames)[0] * 0.18215
    if allocs is not None:
        real = torch.empty
        monkeypatch.setattr(torch, "empty", lambda *a, **k: (allocs.append((tuple(a[0]) if a and isinstance(a[0], (tuple, list)) else a, k.get("dtype"))), real(*a, **k))[1])
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _sched(**(sched_kw or {})))
    out = pipe.denoise(lat, rl, emb if guidance > 1.0 else emb[1:], steps, guidance, generator=torch.Generator().manual_seed(5), **kw)
    return [(n, d) for n, d in fake_ops.CALLS if n.startswith("cfg_")], out, pipe


@pytest.mark.parametrize("guide", ["plain", "rescale", "apg", "pag", "seg"])
@pytest.mark.parametrize("guidance", [3.5, 1.0], ids=["cfg", "nocfg"])
def test_one_step_call_of_the_guides_flavour(monkeypatch, small_cpu, guide, guidance):
    steps = 3                                                                # GUIDES' adaptive PAG scale reaches 0 at the last of 3 steps
    calls, out, pipe = _unipc_loop(monkeypatch, small_cpu, guidance, steps=steps, **GUIDES[guide])
    assert torch.isfinite(out).all()
    cfg = guidance > 1.0
    want = {"plain": "cfg_unipc_step", "rescale": "cfg_unipc_step", "apg": "cfg_unipc_step_apg" if cfg else "cfg_unipc_step",
            "pag": "cfg_unipc_step_pag", "seg": "cfg_unipc_step_pag"}[guide]
    names = [n for n, _ in calls if "_step" in n]
    assert names == ([want] * (steps - 1) + ["cfg_unipc_step"] if guide == "pag" else [want] * steps), names
    recs = [d for n, d in calls if "_step" in n]
    assert [d["scaled"] for d in recs if "scaled" in d] == ([guide == "rescale" and cfg] * steps if want == "cfg_unipc_step" else [False] * (guide == "pag"))
    rows = [pipe.scheduler.unipc_coefficients(i) for i in range(steps)]
    for d, row in zip(recs, rows):
        assert d["row"] == list(row[:11]) and d["correct"] is row[11] and d["halves"] == (2 if cfg else 1)
    if guide == "apg" and cfg:                                               # the statistics pass gets the row's alpha_s, sigma_s
        prep = [d for n, d in calls if n == "cfg_apg_prepare"]
        assert [(d["alpha_s"], d["sigma_s"]) for d in prep] == [row[:2] for row in rows]
    assert len([n for n, _ in calls if n == "cfg_guidance_rescale"]) == (steps if guide == "rescale" and cfg else 0)
    assert not [n for n, _ in calls if "ddim" in n or "multistep" in n]


def test_state_starts_over_per_free_init_pass_and_at_a_strength_start(monkeypatch, small_cpu):
    allocs = []
    calls, out, pipe = _unipc_loop(monkeypatch, small_cpu, frames=4, steps=3, free_init_iters=2, allocs=allocs, sched_kw=dict(solver_order=3))
    recs = [d for n, d in calls if n == "cfg_unipc_step"]
    table = [pipe.scheduler.unipc_coefficients(i) for i in range(3)]
    assert len(recs) == 6 and [d["row"] for d in recs] == [list(r[:11]) for r in table] * 2
    for first in (recs[0], recs[3]):                                         # the first row of a pass reads nothing of the state
        assert first["correct"] is False and first["row"][2:7] == [0.0] * 5 and first["row"][9:11] == [0.0, 0.0]
    assert recs[1]["correct"] and recs[4]["correct"]
    assert len([a for a in allocs if a == ((4, 4, 64, 4), torch.float32)]) == 1           # one state per call, not per pass
    monkeypatch.undo()
    calls, out, pipe = _unipc_loop(monkeypatch, small_cpu, steps=5, init=True, strength=0.6, sched_kw=dict(solver_order=3))
    recs = [d for n, d in calls if n == "cfg_unipc_step"]
    assert pipe.scheduler.begin_index == 2 and len(recs) == 3
    assert [d["row"] for d in recs] == [list(pipe.scheduler.unipc_coefficients(i)[:11]) for i in (2, 3, 4)]
    assert recs[0]["correct"] is False and recs[0]["row"][9:11] == [0.0, 0.0] and recs[1]["correct"] and recs[1]["row"][5] == 0.0
    full = _rows(5, solver_order=3)
    assert full[2][11] and full[2][9] != 0.0                                 # where the full table would have read the state


@pytest.mark.parametrize("case", ["ddim/plain/cfg", "2m/plain/cfg", "2m/apg/cfg", "2m-sde/pag/nocfg", "free-init-fast-apg", "v2v-2m-seg"])
def test_other_samplers_issue_the_recorded_calls_and_allocate_no_state(monkeypatch, small_cpu, case):
    """With the new emulations installed beside the old ones, DDIM and DPM-Solver++ still do what tests/golden/sampling_loop_calls.json holds:
    no cfg_unipc_* call, and no (4, F, HW, 4) state."""
    import json
    from test_sampling_loop_calls_cpu import GOLDEN
    allocs, real = [], torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (allocs.append(tuple(a[0]) if a and isinstance(a[0], (tuple, list)) else a), real(*a, **k))[1])
    got, out = trace_loops(monkeypatch, small_cpu, install=R.install, cases=[case])
    with open(GOLDEN) as fh:
        assert_same(got[case], json.load(fh)["loops"][case], case)
    assert not [n for n, _ in fake_ops.CALLS if "unipc" in n]
    assert not [a for a in allocs if len(a) == 4 and a[0] == 4 and a[3] == 4 and a[2] == 64], allocs
    assert LOOPS[case]["sampler"] in ("ddim", "2m", "2m-sde")


# ---- 5. argument errors, before any operator call
def test_refusals_come_before_any_operator_call(monkeypatch):
    R.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, _sched())
    with pytest.raises(ValueError, match="eta=0.5 cannot be combined with UniPCMultistepScheduler"):
        pipe.denoise(*zero_inputs(), 4, 3.5, eta=0.5)
    with pytest.raises(ValueError, match="cannot be combined with UniPCMultistepScheduler"):
        M.MikuDanceVideoPipeline.sampling_plan(4, 3.5, False, (2, 2, 2), sampler="unipc", eta=1.0, **PLAN_KW)
    assert M.MikuDanceVideoPipeline.sampling_plan(4, 3.5, False, (2, 2, 2), sampler="unipc", **PLAN_KW).sampler == "unipc"
    assert M.MikuDanceVideoPipeline.sampling_plan(4, 3.5, False, (2, 2, 2), eta=0.5, **PLAN_KW).sampler == "ddim"
    with pytest.raises(NotImplementedError, match="solver_order=4"):
        _sched(solver_order=4)
    with pytest.raises(NotImplementedError, match="solver_type='bh3'"):
        _sched(solver_type="bh3")
    for bad in (dict(predict_x0=False), dict(lower_order_final=False), dict(use_karras_sigmas=True), dict(prediction_type="epsilon"),
                dict(final_sigmas_type="sigma_min"), dict(thresholding=True)):
        with pytest.raises(NotImplementedError):
            M.UniPCMultistepScheduler(**dict(SCHED_KWARGS, **bad))
    assert refu.calls == den.calls == 0 and fake_ops.CALLS == []


PLAN_KW = dict(guidance_rescale=0.0, strength=1.0, context_fuse="flat", free_init_iters=1, free_init_filter="butterworth", free_init_order=4,
               free_init_spatial_stop=0.25, free_init_temporal_stop=0.25, free_init_fast=False, apg=False, apg_eta=0.0, apg_norm_threshold=0.0,
               apg_momentum=0.0, pag_scale=0.0, pag_adaptive_scale=0.0, pag_applied_layers=("mid",), kv_downsample=1, kv_downsample_mode="nearest",
               seg_scale=0.0, seg_blur_sigma=100.0, seg_applied_layers=("mid",))


def test_script_builds_the_scheduler_from_its_flags():
    from types import SimpleNamespace
    from mikudance_amd import inference_video as IV
    cfg = SimpleNamespace(noise_scheduler_kwargs=dict(SCHED_KWARGS))
    s = IV.build_scheduler(cfg, "unipc", solver_order=3, solver_type="bh1")
    assert isinstance(s, M.UniPCMultistepScheduler) and s.config["solver_order"] == 3 and s.config["solver_type"] == "bh1"
    d = IV.build_scheduler(cfg, "unipc")
    assert d.config["solver_order"] == 2 and d.config["solver_type"] == "bh2" and d.config["disable_corrector"] == []
    with pytest.raises(NotImplementedError):
        IV.build_scheduler(cfg, "unipc", solver_order=4)
    with pytest.raises(ValueError, match="takes no solver keywords"):
        IV.build_scheduler(cfg, "ddim", solver_order=2)
    a = IV.parse_args(["--config", "x.yaml", "--sampler", "unipc", "--solver_order", "3", "--unipc_solver_type", "bh1"])
    assert (a.sampler, a.solver_order, a.unipc_solver_type) == ("unipc", 3, "bh1")
    a = IV.parse_args(["--config", "x.yaml"])
    assert (a.sampler, a.solver_order, a.unipc_solver_type) == ("ddim", 2, "bh2")
    for bad in (["--solver_order", "4"], ["--unipc_solver_type", "bh3"]):
        with pytest.raises(SystemExit):
            IV.parse_args(["--config", "x.yaml", "--sampler", "unipc"] + bad)


# ---- 6. the emulated step and the emulated loop against the restatement
@pytest.mark.parametrize("order,solver", [(1, "bh2"), (2, "bh2"), (3, "bh1"), (3, "bh2")])
def test_emulated_step_follows_the_restatement(order, solver):
    """3 frames, 5 steps of random v through the emulation of md_cfg_unipc_step (fp32, fp16 latents, one clip-half) against Restated in
    float64 from the same start.  Bound: five roundings of the latents to fp16, each <= 2^-11 relative, carried by weights whose absolute
    sum stays below 2 -> 5 x 2 x 2^-11 = 4.9e-3 relative L2."""
    g = torch.Generator().manual_seed(order)
    s = _sched(solver_order=order, solver_type=solver)
    s.set_timesteps(5)
    rs = R.Restated(order, solver)
    ts = rs.set_timesteps(5)
    lat = torch.randn((3, 35, 4), generator=g).half()
    x = lat.double()
    state = torch.full((4, 3, 35, 4), float("nan"))
    one = torch.ones(3)
    for i, t in enumerate(ts.tolist()):
        v = torch.randn((1, 3, 35, 4), generator=g)
        R.cfg_unipc_step(lat, v, one, state, 3, 35, 1.0, s.unipc_coefficients(i), halves=1)
        x = rs.step(v[0].double(), t, x)
        assert torch.isfinite(lat).all()
        r = rel_l2(lat, x)
        print(f"\nUNIPC_EMULATED_STEP order {order} {solver} step {i}: rel-L2 {r:.3e}")
        assert r <= 5 * 2 * 2.0 ** -11, (i, r)
    assert torch.isfinite(state[:2]).all()


def test_emulated_loop_matches_oracle(monkeypatch, small_cpu):
    from oracle import cpu_ref as O
    R.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(3, 7)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _sched(solver_order=3))
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 5, 3.5)
    with torch.no_grad():
        want = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 5, guidance_scale=3.5, reduced=True, scheduler=R.Restated(3, "bh2"))
    r = rel_l2(out.float(), want)
    print(f"\nUNIPC_HOST_LOOP order 3 bh2, 3 frames, 5 steps: rel_l2 {r:.3e}")
    assert torch.isfinite(out).all() and r < 2e-2, r                         # the bound of tests/test_dpmsolver_cpu.py's host loop
