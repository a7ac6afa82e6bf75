"""CPU: DPM-Solver++ multistep sampling (mikudance_amd.DPMSolverMultistepScheduler) -- timesteps, coefficients against the float64
restatement of tests/dpmpp_ref.py, the order-1 / DDIM identity, convergence on an analytic model, the host loop of
MikuDanceVideoPipeline.denoise() on an emulated operator layer (one rank and three gloo ranks) against the oracle, and the refusals."""
import math
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import fake_ops
from loop_helpers import CountingUNet, rel_l2, run_world, small_cpu, small_inputs, worker_setup, zero_inputs  # noqa: F401 (small_cpu: fixture)

MODES = [dict(solver_order=1), dict(solver_type="midpoint"), dict(solver_type="heun"),
         dict(algorithm_type="sde-dpmsolver++", solver_type="midpoint"), dict(algorithm_type="sde-dpmsolver++", solver_type="heun"),
         dict(solver_order=1, algorithm_type="sde-dpmsolver++")]


def _sched(**kw):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS, **kw)


def _ref_coeffs(n, kw):
    return R.coefficients(n, kw.get("solver_order", 2), kw.get("algorithm_type", "dpmsolver++"), kw.get("solver_type", "midpoint"))


# ---- 1. timesteps
@pytest.mark.parametrize("n", [10, 20, 25, 30, 50])
def test_timesteps_equal_ddim(n):
    s, d = _sched(), M.DDIMScheduler(**SCHED_KWARGS)
    s.set_timesteps(n)
    d.set_timesteps(n)
    assert s.timesteps.tolist() == d.timesteps.tolist()


# ---- 2. coefficients
@pytest.mark.parametrize("n", [4, 10, 20, 30])
@pytest.mark.parametrize("mode", MODES, ids=lambda m: "-".join(f"{v}" for v in m.values()))
def test_coefficients_match_float64_restatement(n, mode):
    s = _sched(**mode)
    s.set_timesteps(n)
    want = _ref_coeffs(n, mode)
    got = [s.multistep_coefficients(i) for i in range(n)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert all(isinstance(v, float) and math.isfinite(v) for v in g), (i, g)
        assert np.allclose(g, w, rtol=1e-12, atol=1e-12), (i, g, w)
    sde = mode.get("algorithm_type") == "sde-dpmsolver++"
    # step 0 and the last step are order 1; step 1 takes the rho = 0 limit (its previous point is lambda = -inf)
    for i in (0, 1, n - 1):
        assert got[i][4] == 0.0, (i, got[i])
    if mode.get("solver_order", 2) == 2 and n >= 4:
        assert all(g[4] != 0.0 for g in got[2:n - 1])
    a_s, s_s, c_x, c_m0, _, c_z = got[0]                           # first step: x' = sigma_1 x + alpha_1 m0 (ODE), alpha_1 m0 + sigma_1 z (SDE)
    assert a_s == 0.0 and s_s == 1.0
    a1, s1 = math.sqrt(float(s.alphas_cumprod[int(s.timesteps[1])])), math.sqrt(1 - float(s.alphas_cumprod[int(s.timesteps[1])]))
    assert np.allclose((c_x, c_m0, c_z), (0.0, a1, s1) if sde else (s1, a1, 0.0), rtol=1e-12, atol=0)
    assert got[-1][2:] == (0.0, 1.0, 0.0, 0.0)                     # the last step lands on m0 itself


def test_set_timesteps_resets_multistep_state():
    s = _sched()
    s.set_timesteps(10)
    s._history, s._last_index = torch.zeros(4), 3
    s.set_timesteps(10)
    assert s._history is None and s._last_index is None and len([s.multistep_coefficients(i) for i in range(10)]) == 10
    s.set_timesteps(4)
    with pytest.raises(IndexError):
        s.multistep_coefficients(4)


# ---- 3. order 1 == DDIM eta = 0 when N divides 1000
def _ddim64(d, t, x, v):
    a_t, a_p = d.step_coefficients(t)
    x0 = math.sqrt(a_t) * x - math.sqrt(1 - a_t) * v
    ep = math.sqrt(a_t) * v + math.sqrt(1 - a_t) * x
    return math.sqrt(a_p) * x0 + math.sqrt(1 - a_p) * ep


def _dpm64(co, x, v, m1=None):
    a_s, s_s, c_x, c_m0, c_m1, _ = co
    m0 = a_s * x - s_s * v
    return c_x * x + c_m0 * m0 + (c_m1 * m1 if c_m1 else 0.0)


def test_order1_equals_ddim_at_20_steps():
    g = np.random.default_rng(0)
    s, d = _sched(solver_order=1), M.DDIMScheduler(**SCHED_KWARGS)
    s.set_timesteps(20)
    d.set_timesteps(20)
    for i, t in enumerate(s.timesteps.tolist()):
        x, v = g.standard_normal(64), g.standard_normal(64)
        assert np.abs(_dpm64(s.multistep_coefficients(i), x, v) - _ddim64(d, t, x, v)).max() <= 1e-12, i


def test_order1_differs_from_ddim_where_ddim_skips_the_next_entry_at_30_steps():
    """DDIM steps to t - 1000 // N (N = 30: 966 -> 933); the solver always to the list's next entry (966 -> 932).  The updates agree on
    the steps where the two targets coincide and differ where they do not."""
    g = np.random.default_rng(1)
    s, d = _sched(solver_order=1), M.DDIMScheduler(**SCHED_KWARGS)
    s.set_timesteps(30)
    d.set_timesteps(30)
    ts = s.timesteps.tolist()
    assert ts[1] == 966 and ts[2] == 932 and ts[1] - 1000 // 30 == 933
    same = diff = 0
    for i, t in enumerate(ts):
        x, v = g.standard_normal(64), g.standard_normal(64)
        err = np.abs(_dpm64(s.multistep_coefficients(i), x, v) - _ddim64(d, t, x, v)).max()
        target = ts[i + 1] if i + 1 < len(ts) else -1
        if t - 1000 // 30 == target or (i + 1 == len(ts) and t - 1000 // 30 < 0):
            assert err <= 1e-12, (i, t, err)
            same += 1
        else:
            assert err > 1e-6, (i, t, err)
            diff += 1
    assert same > 0 and diff > 0


# ---- 4. convergence on an analytic model (fails without the solver)
MU, SD = 0.7, 0.5


def _solve(n, **mode):
    """x0 ~ N(mu, s^2), exact denoiser m = mu + alpha s^2 / (alpha^2 s^2 + sigma^2) (x - alpha mu); the probability-flow ODE from x_T at
    t = 999 (alpha = 0) ends at mu + s x_T.  Returns the max-abs error of the scheduler's own coefficients applied in float64."""
    s = _sched(**mode)
    s.set_timesteps(n)
    xT = np.linspace(-3, 3, 101)
    x, m1 = xT.copy(), None
    for i in range(n):
        a_s, s_s, c_x, c_m0, c_m1, c_z = s.multistep_coefficients(i)
        assert c_z == 0.0
        m0 = MU + a_s * SD ** 2 / (a_s ** 2 * SD ** 2 + s_s ** 2) * (x - a_s * MU)
        x = c_x * x + c_m0 * m0 + (c_m1 * m1 if c_m1 else 0.0)
        m1 = m0
    return float(np.abs(x - (MU + SD * xT)).max())


def test_second_order_converges_faster_on_an_analytic_model():
    ns = (10, 20, 40)
    e1 = [_solve(n, solver_order=1) for n in ns]
    em = [_solve(n, solver_type="midpoint") for n in ns]
    eh = [_solve(n, solver_type="heun") for n in ns]
    print(f"\nDPM_CONVERGENCE N={ns} order1={e1} midpoint={em} heun={eh}")
    for e in (e1, em, eh):
        assert e[0] > e[1] > e[2], e
    for a, b, c in zip(e1, em, eh):
        assert b <= 0.85 * a and c <= 0.85 * a, (a, b, c)
    # the float64 values the feature request quotes for this model
    assert np.allclose([e1, em, eh], [[0.4127, 0.2346, 0.1304], [0.3414, 0.1502, 0.0641], [0.3350, 0.1448, 0.0610]], atol=1e-4, rtol=0)


# ---- 5. the host loop of denoise() on the emulated operators, against the oracle
@pytest.mark.parametrize("mode", [dict(solver_type="midpoint"), dict(algorithm_type="sde-dpmsolver++")], ids=["2m", "2m-sde"])
def test_host_loop_matches_oracle(monkeypatch, small_cpu, mode):
    from oracle import cpu_ref as O
    fake_ops.install(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 7)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _sched(**mode))
    steps = []
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), 4, 3.5, generator=torch.Generator().manual_seed(11),
                       callback=lambda i, t, x: steps.append((i, t)))
    assert steps == [(i, t) for i, t in enumerate([999, 749, 499, 249])]
    rs = R.Restated(2, mode.get("algorithm_type", "dpmsolver++"), mode.get("solver_type", "midpoint"), generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        want = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 4, guidance_scale=3.5, reduced=True, scheduler=rs)
    r = rel_l2(out.float(), want)
    print(f"\nDPM_HOST_LOOP {mode} rel_l2 {r:.3e}")
    assert torch.isfinite(out).all() and r < 2e-2, r


def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=321))
    kw = dict(context_frames=8, context_stride=1, context_overlap=2)             # 3 windows, the last one wraps
    pipe = MikuDanceVideoPipeline(None, None, ref, den, _sched())
    out = pipe.denoise(lat, rl, emb, 4, 3.5, window_parallel=dp.WindowParallel(), **kw)
    got = dp.gather_latents(out)
    if rank == 0:
        one = pipe.denoise(lat, rl, emb, 4, 3.5, **kw)
        q.put(dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                   finite=bool(torch.isfinite(out).all())))
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    """Three gloo ranks, one window each per step, every rank keeping its own history: the 2M loop (4 steps, two of them second
    order) is bit-identical on every rank and to the one-rank loop."""
    res = run_world(3, _wp_worker)
    assert res["identical_on_all_ranks"] and res["equals_one_rank"] and res["finite"], res


# ---- 6. refusals
@pytest.mark.parametrize("kw", [dict(solver_order=3), dict(use_karras_sigmas=True), dict(use_lu_lambdas=True), dict(algorithm_type="dpmsolver"),
                                dict(algorithm_type="sde-dpmsolver"), dict(thresholding=True), dict(prediction_type="epsilon"),
                                dict(solver_type="bh2"), dict(final_sigmas_type="sigma_min"), dict(timestep_spacing="linspace"),
                                dict(beta_schedule="scaled_linear"), dict(variance_type="learned_range"), dict(lambda_min_clipped=-5.1)])
def test_unsupported_configurations_raise(kw):
    with pytest.raises(NotImplementedError):
        M.DPMSolverMultistepScheduler(**dict(SCHED_KWARGS, **kw))


def test_from_config_ignores_unknown_keys_and_defaults():
    s = M.DPMSolverMultistepScheduler.from_config(M.DDIMScheduler(**SCHED_KWARGS).config)
    assert s.config["solver_order"] == 2 and s.config["algorithm_type"] == "dpmsolver++" and s.config["rescale_betas_zero_snr"]
    s2 = M.DPMSolverMultistepScheduler.from_config(dict(SCHED_KWARGS, some_future_key=1), algorithm_type="sde-dpmsolver++")
    assert s2.is_sde and s2.order == 1 and s2.init_noise_sigma == 1.0
    x = torch.zeros(3)
    assert s2.scale_model_input(x, 5) is x
    with pytest.raises(NotImplementedError):
        M.DPMSolverMultistepScheduler()                             # epsilon / linspace defaults are not the MikuDance configuration


class _DuckScheduler:                                                 # has every method the DDIM path calls, but is neither class
    init_noise_sigma = 1.0

    def __init__(self):
        self._d = M.DDIMScheduler(**SCHED_KWARGS)

    def set_timesteps(self, n):
        self._d.set_timesteps(n)
        self.timesteps = self._d.timesteps

    def step_coefficients(self, t):
        return self._d.step_coefficients(t)


def _refusal_pipe(monkeypatch, sch):
    fake_ops.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    return M.MikuDanceVideoPipeline(None, None, refu, den, sch), refu, den


@pytest.mark.parametrize("sch", [_DuckScheduler(), types.SimpleNamespace(init_noise_sigma=1.0, order=1)], ids=["ddim-lookalike", "other"])
def test_foreign_scheduler_raises_type_error_before_any_unet(monkeypatch, sch):
    pipe, refu, den = _refusal_pipe(monkeypatch, sch)
    with pytest.raises(TypeError, match="DDIMScheduler.*DPMSolverMultistepScheduler"):
        pipe.denoise(*zero_inputs(), 4, 3.5)
    assert refu.calls == 0 and den.calls == 0


def test_eta_with_the_solver_raises_value_error(monkeypatch):
    pipe, refu, den = _refusal_pipe(monkeypatch, _sched())
    with pytest.raises(ValueError, match="sde-dpmsolver"):
        pipe.denoise(*zero_inputs(), 4, 3.5, eta=0.5)
    assert refu.calls == 0 and den.calls == 0


def test_step_refuses_out_of_order_and_cpu_tensors():
    s = _sched()
    s.set_timesteps(10)
    with pytest.raises(RuntimeError):
        s.step(torch.zeros(8), 999, torch.zeros(8))                 # no CPU path
    s2 = _sched()
    with pytest.raises(ValueError):
        s2.multistep_coefficients(0)                                # before set_timesteps


def test_sampler_switch_of_the_script():
    from mikudance_amd import inference_video as IV
    assert IV.parse_args([]).sampler == "ddim"
    assert IV.parse_args(["--sampler", "dpmpp_2m_sde"]).sampler == "dpmpp_2m_sde"
    with pytest.raises(SystemExit):
        IV.parse_args(["--sampler", "euler"])
    cfg = types.SimpleNamespace(noise_scheduler_kwargs=dict(SCHED_KWARGS))
    d = IV.build_scheduler(cfg)
    assert type(d) is M.DDIMScheduler and d.config == M.DDIMScheduler(**SCHED_KWARGS).config
    m = IV.build_scheduler(cfg, "dpmpp_2m")
    assert type(m) is M.DPMSolverMultistepScheduler and not m.is_sde and m.config["solver_order"] == 2
    assert IV.build_scheduler(cfg, "dpmpp_2m_sde").is_sde
