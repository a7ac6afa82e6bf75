"""References and the case tables of the kernel-level normalisation tests (tests/test_norm_flavours_gpu.py,
tests/test_norm_floor_cpu.py); CPU only.  The kernels are those of mikudance_amd/csrc/norm.hip.

`*_reference`   float64 on the fp16-rounded inputs: GroupNorm [+ SiLU], the GroupNorm table (scale = rstd gamma, shift = beta - mean scale),
                LayerNorm (y, and y2 = y + add in float64, no rounding in between), InstanceNorm-SPADE, row softmax.
`*_emulation`   the documented arithmetic in plain PyTorch and nothing of the kernels' structure (no pilot, no slabs, no lanes): fp32
                statistics from x.float() (torch's own mean / var, accurate to a few fp32 ulp), the affine in fp32, ONE rounding to fp16;
                y2 = fp16(float(fp16 y) + float(add)), two roundings, as norm.hip states.  The table is fp32 and has no fp16 rounding to
                hide behind, so its emulation carries what fp32 ACCUMULATION costs: the two-pass statistics with one sequential fp32 chain
                per (image, group) (the pessimistic association), about sqrt(n) 2^-25; any
                order a kernel may choose is at least that good, and a sum that loses a pixel (1 / HW) is far outside.
`rel_l2`, `FACTOR`   from tests/attention_ref.py.

rel_l2(emulation) is the FLOOR of a case: what a correct kernel of this arithmetic costs on these very inputs.  It is computed from the
reference alone, never recorded from a build; a kernel passes with rel_l2 <= FACTOR x floor.  One family has a floor of exactly 0 by
arithmetic: InstanceNorm at HW = 1, where mean = x, x - mean = 0 and y = 0 * (1 + gamma) + beta = beta in any precision.

Cases with `mark` carry planted elements, each in an (image, group) -- InstanceNorm: (image, channel) -- of its own, and are measured over
each such unit separately (floor and value restricted to the unit): over the whole tensor one unit's wrong rstd would be diluted by
1 / sqrt(units).
    mark = "sentinel"   one element 40 sigma above its unit's mean at, one unit each: the last pixel; the first pixel of the last slab; the
                        last channel of a group (middle pixel); the pixel of the last row lane of the first slab.  A sweep that drops or
                        double-counts the element moves the unit's variance by 1600 / n.
    mark = "pilot"      the element every pilot scheme would look at, x[b, pixel 0, first channel of the group], 300 sigma above the mean.

Every case carries the plan it is meant for (md_groupnorm_plan: code, threads, R, slab, nslab; md_layernorm_plan: code), derived by hand
from the rule in norm.hip; tests/test_norm_floor_cpu.py compares them with the library.  `gn_problem` / `ln_problem` / `in_problem` /
`sm_problem` build the seeded inputs, the reference and the floor once per process; they are shared and never modified."""
import collections
import functools

import torch

from attention_ref import FACTOR, rel_l2  # noqa: F401  (re-exported)

TWO, THREE = 600, 601                       # md_groupnorm_plan: two launches, three (finalize); 61k / 62k the one-sweep kernel, k = N / 6
S6, S12, S24, W12, W24 = 611, 612, 614, 622, 624
LN320 = 720                                 # md_layernorm_plan: 700 + MAXC, 720 the C = 320 kernel


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------ GroupNorm
def _group_stats(x, G, dtype):
    B, HW, C = x.shape
    xg = x.to(dtype).view(B, HW, G, C // G)
    var, mean = torch.var_mean(xg, dim=(1, 3), unbiased=False)
    return mean, var                                                         # [B, G]


def _per_channel(t, C):                                                      # [B, G] -> [B, 1, C]
    return t.repeat_interleave(C // t.shape[1], dim=1).unsqueeze(1)


def groupnorm_reference(x, gamma, beta, G, eps, silu=False):
    """x [B, HW, C], gamma / beta [C] fp16 -> float64 [B, HW, C]."""
    mean, var = _group_stats(x, G, torch.float64)
    C = x.shape[-1]
    y = (x.double() - _per_channel(mean, C)) * _per_channel((var + eps).rsqrt(), C) * gamma.double() + beta.double()
    return y * torch.sigmoid(y) if silu else y


def groupnorm_emulation(x, gamma, beta, G, eps, silu=False, stats=None):
    """Same operands -> fp16; `stats` = (mean, var) fp32 [B, G] replaces the statistics (the mutations of test_norm_floor_cpu.py)."""
    mean, var = _group_stats(x, G, torch.float32) if stats is None else stats
    C = x.shape[-1]
    y = (x.float() - _per_channel(mean, C)) * _per_channel((var + eps).rsqrt(), C) * gamma.float() + beta.float()
    return (y * torch.sigmoid(y) if silu else y).half()


def table_reference(x, gamma, beta, G, eps):
    """float64 [B, 2, C]: scale = rstd gamma, shift = beta - mean scale."""
    mean, var = _group_stats(x, G, torch.float64)
    C = x.shape[-1]
    scale = _per_channel((var + eps).rsqrt(), C) * gamma.double()
    return torch.cat([scale, beta.double() - _per_channel(mean, C) * scale], dim=1)


def table_emulation(x, gamma, beta, G, eps):
    """fp32 [B, 2, C] from two-pass statistics accumulated as ONE sequential fp32 chain per (image, group)."""
    B, HW, C = x.shape
    xg = x.float().view(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    n = xg.shape[-1]
    cols = xg.permute(2, 0, 1).contiguous()                                  # [n, B, G]

    def chain(t):                                                            # a true fp32 chain (torch's CPU cumsum accumulates in double)
        acc = torch.zeros_like(t[0])
        for row in t:
            acc = acc + row
        return acc
    mean = chain(cols) / n
    d = cols - mean
    var = chain(d * d) / n
    scale = _per_channel((var + eps).rsqrt(), C) * gamma.float()
    return torch.cat([scale, beta.float() - _per_channel(mean, C) * scale], dim=1)


# form:  lead / tail  x is the channel slice [lead, lead + C) of a tensor of pitch lead + C + tail (N(0, 50) around it)
#        inplace      y is x
#        table        md_groupnorm_table_f16 (and, through the returned table, the apply arithmetic)
GN = collections.namedtuple("GN", "name B HW C G code threads R slab nslab lead tail inplace silu table mark eps",
                            defaults=(0, 0, False, False, False, None, 1e-5))

# gn_small_kernel<N, NT>: cpg % 4 == 0, cpg / 4 <= 64, B G >= 256, HW <= 1024.  cpr = cpg / 4 pieces per pixel; NT = 512 when
# cdiv(HW, 256 // cpr) > 24; R = NT // cpr pixel lanes; it = cdiv(HW, R) sweeps; N = 6 (NT = 256 only) / 12 / 24.
GN_SMALL = [
    GN("small <6,256> cpg 4, one sweep", 8, 37, 128, 32, S6, 256, 256, 37, 1),                         # 219 idle lanes
    GN("small <6,256> it 6", 8, 150, 1280, 32, S6, 256, 25, 150, 1, silu=True),                       # 256 // 10 = 25 lanes, 6 full sweeps
    GN("small <12,256> it 12", 8, 300, 1280, 32, S12, 256, 25, 300, 1),
    GN("small <24,256> it 24", 8, 577, 1280, 32, S24, 256, 25, 577, 1, silu=True),                    # 23 * 25 = 575: a last sweep of 2 pixels
    GN("small <12,512> it 12", 8, 607, 1280, 32, W12, 512, 51, 607, 1),                               # cdiv(607, 25) = 25 > 24; cdiv(607, 51) = 12
    GN("small <24,512> it 21", 8, 1024, 1280, 32, W24, 512, 51, 1024, 1, silu=True),
    GN("small <12,512> cpg 80", 8, 300, 2560, 32, W12, 512, 25, 300, 1),                              # 256 // 20 = 12: 25 sweeps; 512 // 20 = 25: 12
    GN("small <24,512> cpg 80", 8, 301, 2560, 32, W24, 512, 25, 301, 1),                              # ... and 13 with one more pixel
    GN("small cpg 20", 8, 150, 640, 32, S6, 256, 51, 150, 1),
    GN("small cpg 60", 8, 150, 1920, 32, S12, 256, 17, 150, 1, silu=True),                            # 256 // 15 = 17, cdiv(150, 17) = 9
    GN("small G=4 (G & 7)", 64, 20, 64, 4, S6, 256, 64, 20, 1),                                       # the plain workgroup -> group map
    GN("small G=64", 4, 33, 256, 64, S6, 256, 256, 33, 1, silu=True),
    GN("small slice lead 64 tail 32", 8, 150, 1280, 32, S6, 256, 25, 150, 1, lead=64, tail=32),
    GN("small slice lead 0 tail 320", 8, 150, 1280, 32, S6, 256, 25, 150, 1, tail=320, silu=True),
    GN("small in place", 8, 300, 1280, 32, S12, 256, 25, 300, 1, inplace=True, silu=True),
    GN("small sentinels", 8, 577, 1280, 32, S24, 256, 25, 577, 1, mark="sentinel"),
]

# Two launches: R = 512 // (C / 8) row lanes, rows = 32 halved (down to 8) while B cdiv(HW, R rows) < 512, slab = R rows.
GN_TWO = [
    GN("two cpg 2", 2, 100, 64, 32, TWO, 512, 64, 512, 1),                                            # cpg < 8: the eight-pilot branch; nslab = 1
    GN("two cpg 4", 2, 100, 128, 32, TWO, 512, 32, 256, 1, silu=True),                                # cpg % 4 == 0 but B G = 64 < 256
    GN("two cpg 10", 2, 100, 320, 32, TWO, 480, 12, 96, 2),                                           # chunks 1, 3, ... straddle two groups
    GN("two cpg 20", 2, 100, 640, 32, TWO, 480, 6, 48, 3, silu=True),
    GN("two cpg 30", 2, 100, 960, 32, TWO, 480, 4, 32, 4),                                            # chunks 3, 7, ... straddle two groups
    GN("two cpg 40", 2, 100, 1280, 32, TWO, 480, 3, 24, 5, silu=True),
    GN("two cpg 60", 2, 100, 1920, 32, TWO, 480, 2, 16, 7),
    GN("two cpg 80", 2, 100, 2560, 32, TWO, 320, 1, 8, 13, silu=True),
    GN("two HW < R", 2, 5, 64, 32, TWO, 512, 64, 512, 1),
    GN("two ragged last slab of 1", 2, 97, 1280, 32, TWO, 480, 3, 24, 5),                             # 4 * 24 + 1
    GN("two HW 1025 past the small kernel", 8, 1025, 1280, 32, TWO, 480, 3, 24, 43),
    GN("two G=16 cpg 8", 3, 70, 128, 16, TWO, 512, 32, 256, 1),                                       # cpg = 8: every chunk is one group
    GN("two slice lead 64 tail 8", 2, 100, 320, 32, TWO, 480, 12, 96, 2, lead=64, tail=8, silu=True),
    GN("two in place", 2, 97, 1280, 32, TWO, 480, 3, 24, 5, inplace=True),
    GN("two 128 slabs", 1, 1024, 2560, 32, TWO, 320, 1, 8, 128),                                      # the neighbour of the three-launch case
    GN("two sentinels", 2, 100, 1280, 32, TWO, 480, 3, 24, 5, mark="sentinel"),
    GN("two pilot outlier", 2, 1104, 1280, 32, TWO, 480, 3, 24, 46, mark="pilot"),
]

# Three launches: nslab > 128.
GN_THREE = [
    GN("three 129 slabs", 1, 1025, 2560, 32, THREE, 320, 1, 8, 129, silu=True),
    GN("three 130 slabs cpg 10", 2, 12400, 320, 32, THREE, 480, 12, 96, 130),                         # 130 % 8 = 2: finalize lanes 2 .. 7 one short
    GN("three in place", 1, 1025, 2560, 32, THREE, 320, 1, 8, 129, inplace=True),
    GN("three sentinels", 1, 1025, 2560, 32, THREE, 320, 1, 8, 129, mark="sentinel"),
    GN("three pilot outlier", 1, 1104, 2560, 32, THREE, 320, 1, 8, 138, mark="pilot"),
]

GN_TABLE = [
    GN("table two", 2, 100, 320, 32, TWO, 480, 12, 96, 2, table=True),
    GN("table two slice", 2, 100, 320, 32, TWO, 480, 12, 96, 2, lead=64, tail=8, table=True),
    GN("table two cpg 40", 2, 1104, 1280, 32, TWO, 480, 3, 24, 46, table=True),
    GN("table three", 1, 1025, 2560, 32, THREE, 320, 1, 8, 129, table=True),
    GN("table three slice", 1, 1025, 2560, 32, THREE, 320, 1, 8, 129, lead=64, tail=64, table=True),
    GN("table small-kernel shape", 8, 150, 1280, 32, TWO, 480, 3, 24, 7, table=True),                 # B G = 256, HW <= 1024: still two launches
    GN("table two sentinels", 2, 100, 1280, 32, TWO, 480, 3, 24, 5, table=True, mark="sentinel"),
    GN("table two pilot outlier", 2, 1104, 1280, 32, TWO, 480, 3, 24, 46, table=True, mark="pilot"),
    GN("table three pilot outlier", 1, 1104, 2560, 32, THREE, 320, 1, 8, 138, table=True, mark="pilot"),
]

GN_CASES = GN_SMALL + GN_TWO + GN_THREE + GN_TABLE


class Problem:
    pass


def _marks(kind, B, HW, G, cpg, R, slab, nslab):
    """[(b, g, pixel, channel in group, sigmas)]: one planted element per (image, group), see the module docstring."""
    if kind is None:
        return []
    b = B - 1
    if kind == "pilot":
        return [(b, 0, 0, 0, 300.0), (0, G - 1, 0, 0, 300.0)]
    return [(b, G - 1, HW - 1, cpg - 1, 40.0),                          # the last pixel (and the tensor's very last element)
            (b, 1, (nslab - 1) * slab if nslab > 1 else HW - R if HW > R else 0, 0, 40.0),   # first pixel of the last slab (one-sweep kernel: of the last sweep)
            (0, 2, HW // 2, cpg - 1, 40.0),                             # the last channel of a group
            (0, G // 2, min(R, HW) - 1, cpg // 2, 40.0)]               # the pixel of the last row lane


@functools.lru_cache(maxsize=None)
def _gn_problem(B, HW, C, G, silu, mark, eps, R, slab, nslab):
    pr = Problem()
    cpg = C // G
    g = _gen(7000 + C + HW + G)
    offs = 1.5 * torch.randn(B, 1, G, 1, generator=g)                   # every (image, group) its own mean and spread
    sig = 0.5 + 1.5 * torch.rand(B, 1, G, 1, generator=g)
    x = offs + sig * torch.randn(B, HW, G, cpg, generator=g)
    pr.marks = _marks(mark, B, HW, G, cpg, R, slab, nslab)
    for b, gi, p, c, k in pr.marks:
        x[b, p, gi, c] = offs[b, 0, gi, 0] + k * sig[b, 0, gi, 0]
    pr.x = x.view(B, HW, C).half()
    pr.gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).half()
    pr.beta = (0.5 * torch.randn(C, generator=g)).half()
    pr.ref = groupnorm_reference(pr.x, pr.gamma, pr.beta, G, eps, silu)
    pr.emu = groupnorm_emulation(pr.x, pr.gamma, pr.beta, G, eps, silu)
    pr.floor = rel_l2(pr.emu, pr.ref)
    return pr


def gn_problem(case):
    return _gn_problem(case.B, case.HW, case.C, case.G, case.silu and not case.table, case.mark, case.eps, case.R, case.slab, case.nslab)


@functools.lru_cache(maxsize=None)
def table_problem(case):
    """(float64 table, its fp32 floor) of a table case."""
    pr = gn_problem(case)
    ref = table_reference(pr.x, pr.gamma, pr.beta, case.G, case.eps)
    return ref, rel_l2(table_emulation(pr.x, pr.gamma, pr.beta, case.G, case.eps), ref)


def unit(t, case, b, g):
    """The (image, group) slice of a [B, HW, C] tensor."""
    cpg = case.C // case.G
    return t[b, :, g * cpg:(g + 1) * cpg]


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_reference(x, gamma, beta, eps):
    xd = x.double()
    var, mean = torch.var_mean(xd, dim=-1, unbiased=False, keepdim=True)
    return (xd - mean) * (var + eps).rsqrt() * gamma.double() + beta.double()


def layernorm_emulation(x, gamma, beta, eps):
    xf = x.float()
    var, mean = torch.var_mean(xf, dim=-1, unbiased=False, keepdim=True)
    return ((xf - mean) * (var + eps).rsqrt() * gamma.float() + beta.float()).half()


def add_rows(add, M, add_mode, add_row_begin, rows_per_frame, frames):
    """[M, C] of what each row receives (zeros where none) and the [M] mask of rows that receive something."""
    rows = torch.arange(M)
    out = torch.zeros(M, add.shape[1], dtype=add.dtype)
    if add_mode == 1:
        got = rows >= add_row_begin
        out[got] = add[rows[got] - add_row_begin]
    else:
        got = torch.ones(M, dtype=torch.bool)
        out[:] = add[(rows // rows_per_frame) % frames]
    return out, got


LN = collections.namedtuple("LN", "name M C code eps add_mode add_row_begin rows_per_frame frames", defaults=(1e-5, 0, 0, 0, 0))


def _ln_code(C):                            # by hand: <1> up to 512, <2> up to 1024, <3> up to 1536, <4> up to 2048; 320 has its own kernel
    return {8: 701, 64: 701, 512: 701, 520: 702, 640: 702, 1024: 702, 1032: 703, 1280: 703, 1536: 703, 1544: 704, 2048: 704, 320: LN320}[C]


LN_WIDTHS = (8, 64, 512, 520, 640, 1024, 1032, 1280, 1536, 1544, 2048, 320)
# M = 1, 15, 16, 17, 31, 33: a wave owns 4 rows (the 320 kernel: 8) and a workgroup 16 (32); rows past M are clamped for the loads
LN_PLAIN = [LN(f"C={C} M={M}", M, C, _ln_code(C)) for C in LN_WIDTHS for M in (1, 15, 16, 17, 31, 33)]
LN_EPS = [LN(f"C={C} M=17 eps 1e-3", 17, C, _ln_code(C), eps=1e-3) for C in (64, 640, 2048, 320)]
# add_mode 1: the bank rows begin at row 0, at row 1, in the middle of a wave's row block (row 6: second of rows 4 .. 7, seventh of 0 .. 7), and
# at row M (no row receives anything: y2 = y).  add_mode 2 at M = 33: rows_per_frame = 1, 3, 7 x frames = 1, 5 -- a wave's 4 (8) rows cross a
# frame boundary in every one, and (row / rpf) % frames wraps inside the tensor at 1 x 5 and 3 x 5
LN_ADD = ([LN(f"C={C} bank from row {a}", 33, C, _ln_code(C), add_mode=1, add_row_begin=a) for C in (640, 320, 1544) for a in (0, 1, 6, 33)] +
          [LN(f"C={C} pos rpf={r} frames={f}", 33, C, _ln_code(C), add_mode=2, rows_per_frame=r, frames=f)
           for C in (640, 320) for r in (1, 3, 7) for f in (1, 5)] +
          [LN("C=1280 pos rpf=3 frames=5 eps 1e-3", 33, 1280, 703, eps=1e-3, add_mode=2, rows_per_frame=3, frames=5)])
LN_CASES = LN_PLAIN + LN_EPS + LN_ADD


@functools.lru_cache(maxsize=None)
def ln_problem(case):
    pr = Problem()
    M, C = case.M, case.C
    g = _gen(8000 + 7 * C + M)
    pr.x = (torch.randn(M, 1, generator=g) + (0.5 + torch.rand(M, 1, generator=g)) * torch.randn(M, C, generator=g)).half()
    pr.gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).half()
    pr.beta = (0.5 * torch.randn(C, generator=g)).half()
    pr.ref = layernorm_reference(pr.x, pr.gamma, pr.beta, case.eps)
    pr.emu = layernorm_emulation(pr.x, pr.gamma, pr.beta, case.eps)
    pr.floor = rel_l2(pr.emu, pr.ref)
    pr.add = None
    if case.add_mode:
        nadd = max(M - case.add_row_begin, 1) if case.add_mode == 1 else case.frames
        pr.add = torch.randn(nadd, C, generator=g).half()
        rows, pr.got = add_rows(pr.add, M, case.add_mode, case.add_row_begin, case.rows_per_frame, case.frames)
        pr.ref2 = pr.ref + rows.double()
        pr.emu2 = torch.where(pr.got[:, None], (pr.emu.float() + rows.float()).half(), pr.emu)      # untouched rows: y2 = y, bit for bit
        pr.floor2 = rel_l2(pr.emu2, pr.ref2)
    return pr


# ------------------------------------------------------------------------------------------------------------------ InstanceNorm-SPADE
def instnorm_reference(x, gb, eps):
    """x [B, HW, C], gb [B, HW, 2C] = gamma | beta -> float64."""
    C = x.shape[-1]
    xd = x.double()
    var, mean = torch.var_mean(xd, dim=1, unbiased=False, keepdim=True)
    return (xd - mean) * (var + eps).rsqrt() * (1.0 + gb[..., :C].double()) + gb[..., C:].double()


def instnorm_emulation(x, gb, eps):
    C = x.shape[-1]
    xf = x.float()
    var, mean = torch.var_mean(xf, dim=1, unbiased=False, keepdim=True)
    return ((xf - mean) * (var + eps).rsqrt() * (1.0 + gb[..., :C].float()) + gb[..., C:].float()).half()


IN = collections.namedtuple("IN", "name B HW C lead tail mark", defaults=(0, 0, None))
IN_CASES = ([IN(f"B={B} HW={HW} C={C}", B, HW, C) for C in (64, 128, 192) for HW in (1, 31, 32, 33, 145) for B in (1, 3)] +
            [IN("slice lead 64 tail 8", 3, 33, 128, lead=64, tail=8), IN("slice lead 0 tail 64", 1, 145, 64, tail=64),
             IN("sentinels", 2, 145, 128, mark="sentinel"),
             IN("pilot outlier", 1, 36864, 64, mark="pilot")])                 # 192 x 192: n large enough for 300 sigma to stay an outlier


@functools.lru_cache(maxsize=None)
def in_problem(case):
    pr = Problem()
    B, HW, C = case.B, case.HW, case.C
    g = _gen(9000 + 3 * C + HW + B)
    offs, sig = 1.5 * torch.randn(B, 1, C, generator=g), 0.5 + 1.5 * torch.rand(B, 1, C, generator=g)
    x = offs + sig * torch.randn(B, HW, C, generator=g)
    # units are (image, channel): last pixel / first pixel of the last sweep of 32 / a pixel in the middle, last channel of a 64-block / the
    # last row lane (pixel 31); the pilot outlier at pixel 0 of the first and of the last channel
    pr.marks = {None: [], "pilot": [(B - 1, 0, 0, 300.0), (0, C - 1, 0, 300.0)],
                "sentinel": [(B - 1, C - 1, HW - 1, 40.0), (B - 1, 1, (HW - 1) // 32 * 32, 40.0), (0, 63, HW // 2, 40.0), (0, C // 2, 31, 40.0)]}[case.mark]
    for b, c, p, k in pr.marks:
        x[b, p, c] = offs[b, 0, c] + k * sig[b, 0, c]
    pr.x = x.half()
    pr.gb = (0.5 * torch.randn(B, HW, 2 * C, generator=_gen(9500 + C + HW))).half()      # a seed of its own
    pr.eps = 1e-5
    pr.ref = instnorm_reference(pr.x, pr.gb, pr.eps)
    pr.emu = instnorm_emulation(pr.x, pr.gb, pr.eps)
    pr.floor = rel_l2(pr.emu, pr.ref)
    return pr


# ------------------------------------------------------------------------------------------------------------------ row softmax
def softmax_reference(x, scale):
    return torch.softmax(x.double() * scale, dim=-1)


def softmax_emulation(x, scale):
    return torch.softmax(x.float() * scale, dim=-1).half()


# 256 threads x 8 columns = 2048 per sweep: cols = 8 (one live thread), 2048 (one vector each), 2056 (thread 0 a second one), 4104 (two each,
# thread 0 a third).  pad: ld = cols + pad.  peaky: one logit 30 / scale above the rest in rows 0 and rows - 1.
SM = collections.namedtuple("SM", "name rows cols pad scale peaky", defaults=(0, 1.0, False))
SM_CASES = ([SM(f"rows={r} cols={c} scale={s}", r, c, 0, s) for c in (8, 2048, 2056, 4104) for r, s in ((1, 0.37), (33, 1.0))] +
            [SM(f"cols={c} pad 24", 33, c, 24, 0.37) for c in (8, 2056)] +
            [SM("peaky cols=2056", 33, 2056, 24, 0.37, True), SM("peaky cols=4104 scale 1", 2, 4104, 0, 1.0, True)])


@functools.lru_cache(maxsize=None)
def sm_problem(case):
    pr = Problem()
    g = _gen(9900 + case.cols + case.rows)
    x = 2.0 * torch.randn(case.rows, case.cols, generator=g)
    if case.peaky:
        x[0, case.cols - 1] = x[0].max() + 30.0 / case.scale                 # the ragged tail's last column
        x[-1, min(case.cols - 1, 1000)] = x[-1].max() + 30.0 / case.scale
    pr.x = x.half()
    pr.ref = softmax_reference(pr.x, case.scale)
    pr.floor = rel_l2(softmax_emulation(pr.x, case.scale), pr.ref)
    return pr
