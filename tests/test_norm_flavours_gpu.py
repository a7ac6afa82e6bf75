"""GPU: every kernel flavour of csrc/norm.hip -- GroupNorm's one-sweep instances, its two- and three-launch forms and the table, the four
LayerNorm instances and the C = 320 kernel, InstanceNorm-SPADE, the row softmax -- each at the smallest shapes that reach its code paths
(tests/norm_ref.py has the case tables and says why each shape).  Every case
  (a) asserts the full plan (md_groupnorm_plan: code, threads, R, slab, nslab; md_layernorm_plan) BEFORE launching, so that a change of
      the rule fails the case instead of silently moving it to another kernel;
  (b) holds every operand and the output in ONE device allocation: 64 elements of 7.0 between the slots, N(0, 50) garbage in the lead and
      tail columns of a channel-slice input, the output pre-filled with NaN.  A kernel that reads past its operand reads garbage, one that
      writes past its output writes into the 7.0 or an input -- it fails the case, it does not leave the allocation;
  (c) launches three times and requires identical bits; afterwards everything outside the output holds its initial bits (the inputs too,
      except where the case runs in place) and the output is finite;
  (d) compares with the float64 reference on the same fp16-rounded inputs: elementwise |err| <= 1e-2 max|ref| + 1e-3 (the project's kernel
      tolerance) and relative L2 <= FACTOR x the case's floor, the relative L2 of a plain PyTorch emulation of the documented arithmetic
      (computed from the reference alone; InstanceNorm at HW = 1 has a floor of 0: the output must be beta exactly).  Cases with planted
      elements (sentinels, the outlier at the pilot's position) are measured over each planted element's (image, group) separately.
profiles/norm_flavour_tests.log: plan, floor and measured value of every case on MI355X, and the mutations these cases catch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_ref as nr  # noqa: E402
from norm_ref import FACTOR, rel_l2  # noqa: E402

from mikudance_amd import _lib, ops  # noqa: E402

GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _garbage(*shape, seed):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 50.0).half()


def _sliced(t, lead, tail, seed):
    """t [..., C] -> the flat [rows, lead + C + tail] tensor that holds it as a channel slice, N(0, 50) around it."""
    C = t.shape[-1]
    wide = _garbage(t.numel() // C, lead + C + tail, seed=seed)
    wide[:, lead:lead + C] = t.reshape(-1, C)
    return wide


class Arena:
    """Named slots of one allocation, each 16-byte aligned, 64 x 7.0 in front of, between and behind them.  `out` names the slots the
    launch may write (NaN at the start unless the slot has contents: in place)."""

    def __init__(self, dev, slots, out):
        self.off, parts, pos = {}, [], 0
        for name, t in slots.items():
            pad = GUARD + (-(pos + GUARD + t.numel())) % 8
            parts += [torch.full((GUARD,), 7.0, dtype=torch.float16), t.reshape(-1).clone(), torch.full((pad - GUARD,), 7.0, dtype=torch.float16)]
            self.off[name] = (pos + GUARD, t.numel())
            pos += t.numel() + pad
        parts.append(torch.full((GUARD,), 7.0, dtype=torch.float16))
        self.host = torch.cat(parts)
        self.dev = self.host.to(dev)
        assert self.dev.data_ptr() % 16 == 0 and all(o % 8 == 0 for o, _ in self.off.values())
        self.out = out
        self.written = torch.zeros(self.host.numel(), dtype=torch.bool)
        for name in out:
            o, n = self.off[name]
            self.written[o:o + n] = True

    def view(self, name, *shape):
        o, n = self.off[name]
        return self.dev[o:o + n].view(*shape)

    def run(self, name, launch, runs=3):
        """launch() `runs` times from the initial contents; returns the output slots (CPU) of the first run."""
        results = []
        for _ in range(runs):
            self.dev.copy_(self.host)
            launch()
            results.append(self.dev.cpu())
        for got in results[1:]:
            assert torch.equal(got.view(torch.int16), results[0].view(torch.int16)), f"{name}: two runs on the same inputs differ"
        got, keep = results[0], ~self.written
        same = got.view(torch.int16)[keep] == self.host.view(torch.int16)[keep]
        assert bool(same.all()), f"{name}: {int((~same).sum())} elements outside the output were written (inputs or the 7.0 between the slots)"
        return {n: got[self.off[n][0]:self.off[n][0] + self.off[n][1]] for n in self.out}


def nan16(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float16)


def measure(tag, name, plan, out, ref, floor):
    """The checks (d) of the module docstring on one tensor (or one unit of it); prints the PARITY_MEASURE line first."""
    value = rel_l2(out, ref)
    ratio = value / floor if floor else float(value != 0)
    print(f"\nPARITY_MEASURE norm_flavour:{tag} {name} plan={plan} floor={floor:.6e} got={value:.6e} ratio={ratio:.3f}")
    assert bool(torch.isfinite(out.float()).all()), f"{name}: non-finite output (an element that was never written stays NaN)"
    err, bound = float((out.double() - ref).abs().max()), 1e-2 * float(ref.abs().max()) + 1e-3
    assert err <= bound, f"{name}: max err {err:.4g} > {bound:.4g}"
    assert value <= FACTOR * floor, f"{name}: relative L2 {value:.3e} > {FACTOR} x the floor {floor:.3e}"


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def gn_plan(case, table):
    out = [ctypes.c_int(0) for _ in range(4)]
    code = _lib.load().md_groupnorm_plan(case.B, case.HW, case.C, case.G, case.lead + case.C + case.tail, 1, int(table), *(ctypes.byref(o) for o in out))
    return (code,) + tuple(o.value for o in out)


def run_gn(dev, case):
    pr = nr.gn_problem(case)
    B, HW, C, G = case.B, case.HW, case.C, case.G
    want = (case.code, case.threads, case.R, case.slab, case.nslab)
    plan = gn_plan(case, case.table)
    assert plan == want, f"{case.name}: the plan is {plan}, the case is meant for {want}"
    ldx = case.lead + C + case.tail
    slots = {"x": _sliced(pr.x, case.lead, case.tail, seed=21), "gamma": pr.gamma, "beta": pr.beta}
    if not case.inplace:
        slots["y"] = nan16(B, HW, C)
    arena = Arena(dev, slots, out=["x" if case.inplace else "y"])
    x = arena.view("x", B, HW, ldx)[:, :, case.lead:case.lead + C]
    y = x if case.inplace else arena.view("y", B, HW, C)
    gamma, beta = arena.view("gamma", C), arena.view("beta", C)
    plan_s = "/".join(map(str, plan))
    if case.table:
        return run_table(dev, case, pr, arena, x, y, gamma, beta, plan_s)
    out = arena.run(case.name, lambda: ops.groupnorm(x, gamma, beta, G, case.eps, silu=case.silu, out=y))
    out = out["x" if case.inplace else "y"].view(B, HW, C)
    measure("gn", case.name, plan_s, out, pr.ref, pr.floor)
    for b, g, p, c, k in pr.marks:
        ref, emu = nr.unit(pr.ref, case, b, g), nr.unit(pr.emu, case, b, g)
        measure("gn", f"{case.name} unit ({b}, {g}) pixel {p}", plan_s, nr.unit(out, case, b, g), ref, rel_l2(emu, ref))


def run_table(dev, case, pr, arena, x, y, gamma, beta, plan_s):
    """md_groupnorm_table_f16 against the float64 table; fp16(fma(x, scale, shift)) from the RETURNED table against the float64 GroupNorm at
    the fp16 floor (whole tensor and planted units); and, where md_groupnorm_ld_nhwc_f16 runs the same two / three launches on the shape,
    its silu = 0 output equal to that fma bit for bit (the fma in float64 -- exact for an fp16 x fp32 product, one rounding of the sum --
    rounded through fp32: the double rounding can differ from the device's single one in about 2^-29 of the elements, none here)."""
    B, HW, C, G = case.B, case.HW, case.C, case.G
    tables = []
    for _ in range(3):
        tables.append(ops.groupnorm_table(x, gamma, beta, G, case.eps))
    torch.cuda.synchronize()
    assert all(torch.equal(t.view(torch.int32), tables[0].view(torch.int32)) for t in tables[1:]), f"{case.name}: two runs on the same inputs differ"
    keep = ~arena.written
    assert torch.equal(arena.dev.cpu().view(torch.int16)[keep], arena.host.view(torch.int16)[keep]), f"{case.name}: the table sweep wrote to its inputs"
    table = tables[0]
    assert table.shape == (B, 2, C) and bool(torch.isfinite(table).all())
    ref, floor = nr.table_problem(case)
    value = rel_l2(table, ref)
    print(f"\nPARITY_MEASURE norm_flavour:gn {case.name} table plan={plan_s} floor={floor:.6e} got={value:.6e} ratio={value / floor:.3f}")
    assert value <= FACTOR * floor, f"{case.name}: the table's relative L2 {value:.3e} > {FACTOR} x the fp32 floor {floor:.3e}"
    applied = torch.addcmul(table[:, 1:2].double(), x.double(), table[:, 0:1].double()).float().half()
    out = applied.cpu()
    measure("gn", f"{case.name} applied", plan_s, out, pr.ref, pr.floor)
    for b, g, p, c, k in pr.marks:
        ref_u, emu_u = nr.unit(pr.ref, case, b, g), nr.unit(pr.emu, case, b, g)
        measure("gn", f"{case.name} applied unit ({b}, {g}) pixel {p}", plan_s, nr.unit(out, case, b, g), ref_u, rel_l2(emu_u, ref_u))
    if gn_plan(case, False)[0] == case.code:
        got = arena.run(case.name, lambda: ops.groupnorm(x, gamma, beta, G, case.eps, silu=False, out=y))["y"].view(B, HW, C)
        differ = int((got.view(torch.int16) != out.view(torch.int16)).sum())
        print(f"PARITY_MEASURE norm_flavour:gn {case.name} groupnorm(silu=0) vs fp16(fma(x, scale, shift)): {differ} of {got.numel()} elements differ")
        assert differ == 0


def _ids(c):
    return c.name


@pytest.mark.parametrize("case", nr.GN_SMALL, ids=_ids)
def test_groupnorm_one_sweep_kernel(dev, case):
    """Every instance of gn_small_kernel at its template steps, cpg = 4 ... 80, both workgroup-to-group maps (G & 7), G = 64, a channel-slice
    input with and without a lead, in place, both SiLU settings, sentinels."""
    run_gn(dev, case)


@pytest.mark.parametrize("case", nr.GN_TWO, ids=_ids)
def test_groupnorm_two_launches(dev, case):
    """gn_stats_kernel + gn_apply_kernel at every cpg of the UNets (2 ... 80: both pilot branches, chunks that straddle two groups), HW < R,
    one slab, a ragged last slab of one pixel, 128 slabs, a channel slice, in place, sentinels, the outlier at the pilot's position."""
    run_gn(dev, case)


@pytest.mark.parametrize("case", nr.GN_THREE, ids=_ids)
def test_groupnorm_three_launches(dev, case):
    """gn_finalize_kernel in between: 129 slabs, 130 (no multiple of its 8 lanes per group), in place, sentinels, the outlier."""
    run_gn(dev, case)


@pytest.mark.parametrize("case", nr.GN_TABLE, ids=_ids)
def test_groupnorm_table(dev, case):
    run_gn(dev, case)


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("case", nr.LN_CASES, ids=_ids)
def test_layernorm(dev, case):
    """layernorm_kernel<1 .. 4> at both ends of each width range and layernorm320_kernel, M around the 4- (8-) row blocks of a wave and the
    16 (32) rows of a workgroup, add_mode 1 / 2 with y2 starting as NaN, eps = 1e-5 and 1e-3."""
    pr = nr.ln_problem(case)
    M, C = case.M, case.C
    code = _lib.load().md_layernorm_plan(M, C)
    assert code == case.code, f"{case.name}: the plan is {code}, the case is meant for {case.code}"
    slots = {"x": pr.x, "gamma": pr.gamma, "beta": pr.beta, "y": nan16(M, C)}
    if case.add_mode:
        slots.update(add=pr.add, y2=nan16(M, C))
    arena = Arena(dev, slots, out=["y", "y2"] if case.add_mode else ["y"])
    ptr = lambda n: arena.dev.data_ptr() + 2 * arena.off[n][0]  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    out = arena.run(case.name, lambda: _lib.call("md_layernorm_f16", ptr("x"), ptr("y"), ptr("y2") if case.add_mode else 0, ptr("gamma"), ptr("beta"),
                                                 ptr("add") if case.add_mode else 0, M, C, case.eps, case.add_mode, case.add_row_begin,
                                                 case.rows_per_frame, case.frames, st))
    y = out["y"].view(M, C)
    measure("ln", case.name, code, y, pr.ref, pr.floor)
    if case.add_mode:
        y2 = out["y2"].view(M, C)
        measure("ln", case.name + " y2", code, y2, pr.ref2, pr.floor2)
        idle = ~pr.got
        assert torch.equal(y2[idle].view(torch.int16), y[idle].view(torch.int16)), f"{case.name}: y2 != y on a row that receives nothing"


# ------------------------------------------------------------------------------------------------------------------ InstanceNorm-SPADE
@pytest.mark.parametrize("case", nr.IN_CASES, ids=_ids)
def test_instnorm_spade(dev, case):
    """instnorm_spade_kernel: one to three 64-channel blocks, HW around its 32 row lanes (HW = 1: y = beta exactly), B = 1 and 3, a channel
    slice, gamma | beta from a seed of their own, sentinels, the outlier at pixel 0."""
    pr = nr.in_problem(case)
    B, HW, C = case.B, case.HW, case.C
    ldx = case.lead + C + case.tail
    arena = Arena(dev, {"x": _sliced(pr.x, case.lead, case.tail, seed=22), "gb": pr.gb, "y": nan16(B, HW, C)}, out=["y"])
    ptr = lambda n: arena.dev.data_ptr() + 2 * arena.off[n][0]  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    out = arena.run(case.name, lambda: _lib.call("md_instnorm_spade_ld_f16", ptr("x") + 2 * case.lead, ldx, ptr("gb"), ptr("y"), B, HW, C, pr.eps, st))
    y = out["y"].view(B, HW, C)
    measure("in", case.name, "-", y, pr.ref, pr.floor)
    for b, c, p, k in pr.marks:
        measure("in", f"{case.name} unit ({b}, {c}) pixel {p}", "-", y[b, :, c], pr.ref[b, :, c], rel_l2(pr.emu[b, :, c], pr.ref[b, :, c]))


# ------------------------------------------------------------------------------------------------------------------ row softmax
@pytest.mark.parametrize("case", nr.SM_CASES, ids=_ids)
def test_softmax_rows(dev, case):
    """softmax_rows_kernel in place: 0 / 1 / 2 full vectors per thread and a ragged tail, ld > cols with the pad bits untouched, rows = 1
    and 33, a peaky row, scale = 0.37 and 1.0.  (scale <= 0 is refused without a launch: tests/test_norm_floor_cpu.py.)"""
    pr = nr.sm_problem(case)
    rows, cols, ld = case.rows, case.cols, case.cols + case.pad
    wide = _garbage(rows, ld, seed=23)
    wide[:, :cols] = pr.x
    arena = Arena(dev, {"x": wide}, out=["x"])
    o = arena.off["x"][0]
    arena.written[:] = False
    arena.written[o:o + rows * ld].view(rows, ld)[:, :cols] = True                     # the pad columns must keep their bits
    x = arena.view("x", rows, ld)[:, :cols]
    out = arena.run(case.name, lambda: ops.softmax_rows_(x, scale=case.scale))["x"].view(rows, ld)[:, :cols]
    measure("softmax", case.name, "-", out, pr.ref, pr.floor)
