"""GPU: UniPC sampling on the MI355X -- the four md_cfg_unipc_step* entries against a float64 evaluation of the same row on the same inputs
(small sizes and past one grid round of the launch, corrector on and off, a first step on a NaN state), six steps of order 3 through
UniPCMultistepScheduler.step against tests/unipc_ref.Restated, the tiny-UNet loop against the CPU oracle carrying Restated (plain and under
guidance_rescale, apg, pag_scale, strength, FreeInit), and determinism.  profiles/unipc_kernel_tests.log holds the printed figures of a run.

Bounds of the kernel tests.  Latents: the project's step error model, |got - want| <= U16 |want| + 2e-6 scale + 2^-24 with scale the sum of the
absolute values of the terms (tests/test_elementwise_gpu.py).  State planes (fp32): a FLOOR computed from the float64 reference alone, the
standard forward bound of a sum of k rounded operations, 2^-24 k sum |terms|, with k counted from the kernel's documented arithmetic: the
guided v costs K_V roundings (CFG: 1 / cnt, two products, the difference, the multiply-add = 5; without CFG the window sum is taken as it is =
0; the rescale factor + 1; PAG's term + 4: its 1 / cnt, difference, scale product, multiply-add; APG's v_g = c - gs (S m - K (a x - s c)) + 7
over the conditional mean's 2), m_t = alpha_s x - sigma_s v two more, x^c one per term on top of its operands.  A plane passes at
|got - want| <= 1.25 x floor (the project's operator margin, parity_budget.KERNEL_FACTOR); a plane that only moves (H1 <- H0, H2 <- H1, x^c = x
with the corrector off) must be bit-exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

import apg_ref as A  # noqa: E402
import elementwise_ref as E  # noqa: E402
import free_init_ref as FR  # noqa: E402
import pag_ref as P  # noqa: E402
import rescale_ref as RR  # noqa: E402
import unipc_ref as R  # noqa: E402
import v2v_ref as V  # noqa: E402
from parity_budget import KERNEL_FACTOR  # noqa: E402

DEV = torch.device("cuda:0")
U16, U32 = 2.0 ** -11, 2.0 ** -24
ROUND = 4096 * 256                      # pixels of one grid round: cfg_unipc_launch caps the grid at 4096 workgroups of 256 threads
BIG = {1: 1048613, 3: 349537}           # HW past one round: 37 pixels (Ftot = 1) and 35 pixels (Ftot = 3, the boundary inside frame 2) loop twice
K_V = {("plain", 1): 0, ("plain", 2): 5, ("scaled", 2): 6, ("pag", 1): 4, ("pag", 2): 9, ("apg", 2): 9}


def _sched(**kw):
    return M.UniPCMultistepScheduler(**SCHED_KWARGS, **kw)


def _row(kind):
    """A row of the 10-step, order-3 table: "on" = step 4 (corrector of order 3: every plane read), "off" = the same step with the corrector
    disabled (predictor of order 3: H2 is not read), "first" = step 0 (nothing read)."""
    s = _sched(solver_order=3, disable_corrector=(4,) if kind == "off" else ())
    s.set_timesteps(10)
    row = s.unipc_coefficients(0 if kind == "first" else 4)
    if kind == "on":
        assert row[11] and all(v != 0.0 for v in row[2:11])
    elif kind == "off":
        assert not row[11] and row[9] != 0.0 and row[10] != 0.0 and row[2:7] == (0.0,) * 5
    else:
        assert not row[11] and row[9] == row[10] == 0.0
    return row


_CASES = {}


def _case(ftot, hw, halves):
    """One set of inputs per shape, shared by the flavours and rows: E.step_case (planes, counter, latents, APG's momentum) and a state."""
    key = (ftot, hw, halves)
    if key not in _CASES:
        _CASES.clear()                                                       # one big case at a time
        c = E.step_case("plain", ftot, hw, halves, E.step_seed("plain", ftot, hw, halves))
        c.state = torch.randn((4, ftot, hw, 4), generator=torch.Generator().manual_seed(hw % 1009 + ftot)) * torch.tensor([1.0, 0.8, 0.9, 1.1]).view(4, 1, 1, 1)
        _CASES[key] = c
    return _CASES[key]


def _kernel(flavour, case, row, state):
    """One call on the device -> (latents, state, extra) on the host; extra: for apg (coef, momentum) as cfg_apg_prepare left them."""
    ftot, hw, halves = case.ftot, case.hw, case.halves
    g = E.guidance(flavour)
    cnt = case.cnt if halves == 2 else torch.full_like(case.cnt, float("nan"))                  # without CFG the counter is not read
    ld, nd, cd, sd = case.lat.to(DEV), case.ns.to(DEV), cnt.to(DEV), state.to(DEV)
    extra = None
    if flavour == "plain":
        ops.cfg_unipc_step(ld, nd, cd, sd, ftot, hw, g, row, halves=halves)
    elif flavour == "scaled":
        ops.cfg_unipc_step(ld, nd, cd, sd, ftot, hw, g, row, halves=halves, vscale=torch.tensor([E.VSCALE], device=DEV))
    elif flavour == "pag":
        ops.cfg_unipc_step_pag(ld, nd, cd, sd, case.pp.to(DEV), ftot, hw, g, E.PAG_S, row, halves=halves)
    else:
        md, coef = case.mprev.to(DEV), torch.zeros((ftot, 2), device=DEV)
        ops.cfg_apg_prepare(ld, nd, cd, md, coef, ftot, hw, row[0], row[1], E.APG_BETA, E.APG_ETA, E.apg_threshold(case, row[0], row[1]))
        ops.cfg_unipc_step_apg(ld, nd, cd, sd, md, coef, ftot, hw, g, row)
        extra = (coef.cpu(), md.cpu())
    torch.cuda.synchronize()
    return ld.cpu(), sd.cpu(), extra


def _check(tag, flavour, case, row, state, got, st, extra, second_round_from=None):
    """float64 on the same inputs, then the bounds of the module docstring.  Returns the worst |err| / floor over the computed planes.
    The row is the one the kernel was given: the ABI takes floats, so its eleven weights are rounded to fp32 first (against the float64 row the
    data prediction of the plain entry measured 1.189 x its floor of two roundings on an MI355X: the third was alpha_s's and sigma_s's own)."""
    row = tuple(torch.tensor(row[:11], dtype=torch.float32).double().tolist()) + (row[11],)
    a_s, s_s = row[0], row[1]
    if flavour == "apg":
        v, vabs = E._vg64(case.ns, case.cnt, case.lat, extra[1], extra[0], a_s, s_s)
    else:
        v, vabs = E._v64(case.ns, case.pp, case.cnt, case.halves, E.PAG_S if flavour == "pag" else 0.0)
        if flavour == "scaled":
            v, vabs = v * E.VSCALE, vabs * E.VSCALE
    x = case.lat.double()
    s64 = [state[k].double() for k in range(4)]
    want, new = R.row_update(x, v, s64, row)
    kv = K_V[(flavour, case.halves)]
    mag_m = (a_s * x).abs() + s_s * vabs
    floor_m = U32 * (kv + 2) * mag_m
    cc, pc = row[2:7], row[7:11]
    if row[11]:
        mag_c = (cc[0] * s64[0]).abs() + abs(cc[1]) * mag_m + sum((cc[2 + k] * s64[1 + k]).abs() for k in range(3))
        floor_c = U32 * (kv + 2 + 5) * mag_c
    else:
        mag_c, floor_c = x.abs(), torch.zeros_like(x)
    scale = abs(pc[0]) * mag_c + abs(pc[1]) * mag_m + (pc[2] * s64[1]).abs() + (pc[3] * s64[2]).abs() + mag_m
    g64 = got.double()
    assert torch.isfinite(g64).all() and torch.isfinite(st).all()
    err = (g64 - want).abs()
    bound = U16 * want.abs() + 2e-6 * scale + U32
    ratios = {}
    for name, plane, ref, floor in (("x_last", st[0], new[0], floor_c), ("H0", st[1], new[1], floor_m)):
        e = (plane.double() - ref).abs()
        if float(floor.max()) == 0.0:
            assert torch.equal(plane.double(), ref), (tag, name)             # x^c = x: the fp16 latent, exactly
            ratios[name] = 0.0
        else:
            ratios[name] = float((e / floor).max())
            assert (e <= KERNEL_FACTOR * floor).all(), (tag, name, ratios[name])
    rd0, rd1 = row[4] != 0.0 or row[9] != 0.0, row[5] != 0.0 or row[10] != 0.0
    assert torch.equal(st[2], state[1] if rd0 else state[2]) and torch.equal(st[3], state[2] if rd1 else state[3]), (tag, "rotation")
    line = (f"\n{tag} {flavour} ({case.ftot},{case.hw}) halves {case.halves} corrector {'on' if row[11] else 'off'}: latents max |got - want| "
            f"{float(err.max()):.3e}, worst |err| / bound {float((err / bound).max()):.3f}; state |err| / floor: x_last {ratios['x_last']:.3f}, "
            f"H0 {ratios['H0']:.3f} (margin {KERNEL_FACTOR})")
    if second_round_from is not None:
        e2, b2 = err.reshape(-1)[second_round_from * 4:], bound.reshape(-1)[second_round_from * 4:]
        line += f"; second round ({e2.numel() // 4} pixels): worst |err| / bound {float((e2 / b2).max()):.3f}"
        assert e2.numel() > 0 and (e2 <= b2).all()
    print(line)
    assert (err <= bound).all(), (tag, float(err.max()), float((err - bound).max()))
    return max(ratios.values())


# ---- 1. the kernel against float64
@pytest.mark.parametrize("corrector", ["on", "off"])
@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("hw", [1, 37, "round2"])
@pytest.mark.parametrize("ftot", [1, 3])
def test_every_entry_matches_float64(ftot, hw, halves, corrector):
    big = hw == "round2"
    hw = BIG[ftot] if big else hw
    assert (ftot * hw > ROUND) == big
    case, row = _case(ftot, hw, halves), _row(corrector)
    for flavour in ("plain", "scaled", "apg", "pag") if halves == 2 else ("plain", "pag"):
        got, st, extra = _kernel(flavour, case, row, case.state)
        _check("UNIPC_KERNEL_ROUND2" if big else "UNIPC_KERNEL", flavour, case, row, case.state, got, st, extra, second_round_from=ROUND if big else None)


@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("ftot,hw", [(1, 1), (3, 37)])
def test_first_step_reads_nothing_of_a_nan_state(ftot, hw, halves):
    case, row = _case(ftot, hw, halves), _row("first")
    nan = torch.full((4, ftot, hw, 4), float("nan"))
    for flavour in ("plain", "scaled", "apg", "pag") if halves == 2 else ("plain", "pag"):
        got, st, extra = _kernel(flavour, case, row, nan)
        assert torch.isfinite(got).all() and torch.isfinite(st[:2]).all() and torch.isnan(st[2:]).all()      # H1, H2: not read, so not written
        _check("UNIPC_KERNEL_FIRST", flavour, case, row, torch.zeros_like(nan), got, torch.cat([st[:2], torch.zeros_like(st[2:])]), extra)


def test_kernel_refuses_bad_arguments():
    lat = torch.zeros((2, 8, 4), device=DEV, dtype=torch.float16)
    ns, cnt, st = torch.zeros((2, 2, 8, 4), device=DEV), torch.ones(2, device=DEV), torch.zeros((4, 2, 8, 4), device=DEV)
    row = _row("on")
    with pytest.raises(_lib.MdanceHipError, match="non-finite"):
        ops.cfg_unipc_step(lat, ns, cnt, st, 2, 8, 3.5, row[:3] + (float("nan"),) + row[4:])
    with pytest.raises(_lib.MdanceHipError, match="corrector flag"):
        ops.cfg_unipc_step(lat, ns, cnt, st, 2, 8, 3.5, row[:11] + (2.0,))
    with pytest.raises(_lib.MdanceHipError, match="null"):
        _lib.call("md_cfg_unipc_step", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), 0, 2, 8, 2, 3.5, ops._unipc_state_row(st, row, 2, 8)[1], ops._st())
    with pytest.raises(_lib.MdanceHipError, match="null"):
        _lib.call("md_cfg_unipc_step", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), st.data_ptr(), 2, 8, 2, 3.5, 0, ops._st())
    with pytest.raises(_lib.MdanceHipError, match="alignment"):
        _lib.call("md_cfg_unipc_step", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), st.data_ptr() + 4, 2, 8, 2, 3.5,
                  ops._unipc_state_row(st, row, 2, 8)[1], ops._st())
    with pytest.raises(_lib.MdanceHipError, match="halves == 2"):
        _lib.call("md_cfg_unipc_step_scaled", lat.data_ptr(), ns.data_ptr(), cnt.data_ptr(), st.data_ptr(), cnt.data_ptr(), 2, 8, 1, 3.5,
                  ops._unipc_state_row(st, row, 2, 8)[1], ops._st())
    with pytest.raises(AssertionError):
        ops.cfg_unipc_step(lat, ns, cnt, st[:3], 2, 8, 3.5, row)
    torch.cuda.synchronize()
    assert not lat.any() and not st.any()                                    # nothing was launched


# ---- 2. six steps through the scheduler's own step()
@pytest.mark.parametrize("solver", ["bh1", "bh2"])
def test_scheduler_step_sequence_order_3(solver):
    """History rotation, x_last carry-over, the order ramp 1, 1, 2, 3, 2, 1 (zero terminal SNR: t = 999 is no history point).  Bound: six
    roundings of the sample to fp16, each <= 2^-11 relative, carried by weights whose absolute sum stays below 2 -> 6 x 2 x 2^-11."""
    s = _sched(solver_order=3, solver_type=solver)
    s.set_timesteps(6)
    rs = R.Restated(3, solver)
    ts = rs.set_timesteps(6)
    g = torch.Generator().manual_seed(9)
    x16 = torch.randn((1, 4, 3, 13, 11), generator=g).half()
    xd, x64 = x16.to(DEV), x16.double()
    for i, t in enumerate(ts.tolist()):
        v = torch.randn((1, 4, 3, 13, 11), generator=g).half()
        xd = s.step(v.to(DEV), t, xd).prev_sample
        x64 = rs.step(v.double(), t, x64)
        r = rel_l2(xd.cpu(), x64)
        print(f"\nUNIPC_SEQUENCE {solver} step {i}: rel-L2 {r:.3e}")
        assert xd.dtype == torch.float16 and xd.shape == x16.shape and r <= 6 * 2 * U16, (i, r)
    s2 = _sched(solver_order=3)
    s2.set_timesteps(6)
    with pytest.raises(RuntimeError, match="reads the state of step 1"):
        s2.step(v.to(DEV), s2.timesteps[2], xd)


# ---- 3. the loop against the CPU oracle
@pytest.fixture(scope="module")
def small():
    return build_models()


STEPS, FRAMES, G = 6, 4, 3.5


def _inputs(seed):
    return tuple(t.half().float() for t in synth_inputs(FRAMES, 16, 16, ctx_len=5, ctx_dim=64, seed=seed))


def _loop(models, inputs, steps=STEPS, seed=None, order=2, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _sched(solver_order=order))
    gen = torch.Generator().manual_seed(seed) if seed is not None else None
    if "init_latents" in kw:
        kw["init_latents"] = kw["init_latents"].half().to(DEV)
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), steps, G, generator=gen, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _want(mode, models, inputs, x0):
    _, _, ref_sd, den_sd = models
    common = dict(guidance_scale=G, scheduler=R.Restated(2, "bh2"))
    with torch.no_grad():
        if mode == "plain":
            return O.denoise_loop(ref_sd, den_sd, *inputs, STEPS, reduced=True, **common)
        if mode == "rescale":
            return RR.denoise_loop(ref_sd, den_sd, *inputs, STEPS, reduced=True, guidance_rescale=0.7, **common)
        if mode == "apg":
            return A.denoise_loop(ref_sd, den_sd, *inputs, STEPS, reduced=True, apg_on=True, apg_eta=0.5, apg_norm_threshold=2.0, apg_momentum=-0.5, **common)
        if mode == "pag":
            return P.denoise_loop(ref_sd, den_sd, *inputs, STEPS, pag_scale=3.0, pag_layers=("mid",), **common)
        if mode == "strength":
            start = STEPS - V.kept_steps(STEPS, 0.6)
            t0 = R.schedule(STEPS)[0][start]
            return O.denoise_loop(ref_sd, den_sd, V.noised(x0, inputs[0], t0), *inputs[1:], STEPS, reduced=True, guidance_scale=G,
                                  scheduler=R.Restated(2, "bh2", begin=start))
        assert mode == "free_init"
        return FR.denoise_loop(ref_sd, den_sd, *inputs, STEPS, 2, torch.Generator().manual_seed(23), make_scheduler=lambda: R.Restated(2, "bh2"),
                               guidance_scale=G, reduced=True)


LOOP_KW = {"plain": {}, "rescale": dict(guidance_rescale=0.7), "apg": dict(apg=True, apg_eta=0.5, apg_norm_threshold=2.0, apg_momentum=-0.5),
           "pag": dict(pag_scale=3.0, pag_applied_layers=("mid",)), "strength": dict(strength=0.6), "free_init": dict(free_init_iters=2)}


@pytest.mark.parametrize("mode", list(LOOP_KW))
def test_loop_vs_cpu_oracle_reduced_width(small, mode):
    """The tiny-UNet loop, 4 frames 16 x 16, 6 steps of UniPC order 2 bh2, against the oracle's loop carrying tests/unipc_ref.Restated.
    The bound is tests/test_dpmsolver_gpu.py's loop bound: rel-L2 <= 3e-2, cosine >= 0.999."""
    inputs = _inputs(211)
    x0 = (_inputs(311)[0] * 0.18215).half().float()
    kw = dict(LOOP_KW[mode])
    if mode == "strength":
        kw["init_latents"] = x0
    out = _loop(small, inputs, seed=23, **kw)
    want = _want(mode, small, inputs, x0)
    r, c = rel_l2(out, want), cosine(out, want)
    print(f"\nUNIPC_LOOP {mode}: {FRAMES} frames 16x16, {STEPS} steps, order 2 bh2: rel_l2 {r:.3e} cos {c:.7f}")
    assert torch.isfinite(out).all() and r <= 3e-2 and c >= 0.999, (r, c)


# ---- 4. determinism
def test_two_runs_give_the_same_bits(small):
    inputs = _inputs(211)
    a = _loop(small, inputs, order=3)
    b = _loop(small, inputs, order=3)
    assert torch.isfinite(a).all() and torch.equal(a, b)
