"""References and the case table of the kernel-level temporal-attention tests (tests/test_temporal_flavours_gpu.py,
tests/test_temporal_floor_cpu.py); CPU only.  Operands are token-major: row (b*F + frame)*HW + pixel, columns head*D + d.

`reference`   float64 softmax(scale * Q K^T) V over the F frames of every (clip-half, pixel, head), on the fp16-rounded inputs.
`emulation`   the arithmetic md_temporal_attention_fwd_f16 documents (csrc/temporal.hip), in plain PyTorch and nothing of the kernels'
              structure: scores in fp32, p = exp2((s - max) * scale * log2e) in fp32, the denominator summed from those fp32 p, one
              rounding of the output to fp16.  matrix_core=True (temporal_attn_mfma_kernel): P is rounded to fp16 for the P V product
              (the denominator still comes from the fp32 exponentials); matrix_core=False (temporal_attn_kernel): everything in fp32.
`rel_l2`, `FACTOR`   from tests/attention_ref.py.

rel_l2(emulation) is the FLOOR of a case: what a correct kernel of this arithmetic costs on these very inputs.  It is computed from the
reference alone, never recorded from a build; a kernel passes with rel_l2 <= FACTOR x floor.  One case family has a floor of exactly 0:
with F = 1 the softmax is 1.0 and the output IS the V row (1.0 * v / 1.0 in any precision), so there the kernel must return V bit for bit.

`CASES` is the table both test files run; `problem(case)` builds the seeded inputs, the reference and the floor once per process."""
import collections
import functools

import torch

from attention_ref import FACTOR, rel_l2, rnd  # noqa: F401  (re-exported)

LOG2E = 1.4426950408889634
LANE, MFMA1, MFMA2 = 500, 511, 512          # md_temporal_attention_plan: lane-per-query kernel, matrix-core kernel with QB = 1 / 2


def _fold(t, NB, F, HW, H, D):             # [(b f) pixel, H*D] -> [b, pixel, head, f, D]
    return t.view(NB, F, HW, H, D).permute(0, 2, 3, 1, 4)


def _unfold(o, NB, F, HW, H, D):           # back to token-major rows
    return o.permute(0, 3, 1, 2, 4).reshape(NB * F * HW, H * D)


def reference(q, k, v, NB, F, HW, H, D, scale=None):
    """q / k / v [NB*F*HW, H*D] fp16 -> float64 [NB*F*HW, H*D]."""
    scale = D ** -0.5 if scale is None else scale
    qh, kh, vh = (_fold(t.double(), NB, F, HW, H, D) for t in (q, k, v))
    a = torch.softmax((qh @ kh.transpose(-1, -2)) * scale, dim=-1)
    return _unfold(a @ vh, NB, F, HW, H, D).contiguous()


def emulation(q, k, v, NB, F, HW, H, D, scale=None, matrix_core=True):
    """Same operands -> fp16 [NB*F*HW, H*D] by the documented arithmetic (see the module docstring)."""
    scale = D ** -0.5 if scale is None else scale
    sc2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)      # fp32 product, as the library forms it
    qh, kh, vh = (_fold(t.float(), NB, F, HW, H, D) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2)                                                                  # fp32
    p = torch.exp2((s - s.max(dim=-1, keepdim=True).values) * sc2)
    den = p.sum(dim=-1, keepdim=True)                                                              # from the fp32 exponentials in both forms
    if matrix_core:
        p = p.half().float()                                                                       # P rounded to fp16 for the matrix core
    return _unfold(((p @ vh) / den).half(), NB, F, HW, H, D).contiguous()


# ------------------------------------------------------------------------------------------------------------------ the cases
# form:  dense    q, k, v, o four dense [M, C] tensors, o starts as NaN
#        qkv      production (blocks.py: the motion module's attention): q | k | v the column thirds of one [M, 3C] buffer, o dense (NaN)
#        pitches  four different pitches: q at columns 32.. of [M, C+64], k the second half of [M, 2C], v at columns 8.. of [M, C+8],
#                 o at columns 16.. of [M, C+32]; N(0, 50) garbage around q / k / v, 7.0 around o
# peaky: dominant keys (k[frame j] = 4 q[frame i], logits ~ 4 sqrt(D) >= 25) for a few (pixel, head) units, see problem()
# mult:  scale = mult * D ** -0.5
Case = collections.namedtuple("Case", "name NB F HW H D code hg pb form peaky mult", defaults=("dense", False, 1.0))

# One per row of the plan table of tests/test_temporal_floor_cpu.py (511 / 512), NB * HW % pb != 0 wherever pb > 1, plus two H = 4 rows.
GEOMETRIES = [
    Case("geom H=8 D=40 F=16", 2, 16, 9, 8, 40, MFMA1, 8, 1),
    Case("geom H=8 D=80 F=16", 1, 16, 5, 8, 80, MFMA1, 4, 1),
    Case("geom H=8 D=160 F=16", 2, 16, 3, 8, 160, MFMA1, 2, 1),
    Case("geom H=8 D=40 F=30", 1, 30, 7, 8, 40, MFMA2, 4, 1),
    Case("geom H=8 D=80 F=30", 2, 30, 4, 8, 80, MFMA2, 2, 1),
    Case("geom H=8 D=160 F=32", 1, 32, 3, 8, 160, MFMA2, 1, 1),
    Case("geom H=8 D=40 F=7", 3, 7, 3, 8, 40, MFMA1, 8, 2),            # 9 pixels in pairs: O through LDS, the write-back's gp >= npix guard
    Case("geom H=2 D=40 F=16", 2, 16, 7, 2, 40, MFMA1, 2, 6),          # 14 pixels in sixes: a last workgroup of 2 pixels, 12 units on 4 waves
    Case("geom H=1 D=40 F=17", 2, 17, 5, 1, 40, MFMA2, 1, 8),          # 10 pixels in eights: 8 units, two per wave
    Case("geom H=8 D=40 F=17", 2, 17, 3, 8, 40, MFMA2, 8, 1),
    Case("geom H=8 D=160 F=3", 3, 3, 5, 8, 160, MFMA1, 8, 2),          # 15 pixels in pairs: direct stores, `break` on gp >= npix
    Case("geom H=4 D=40 F=8", 1, 8, 11, 4, 40, MFMA1, 4, 4),           # 11 pixels in fours: a last workgroup of 3
    Case("geom H=4 D=80 F=16", 2, 16, 3, 4, 80, MFMA1, 4, 1),
]


def _edge_plan(F, D):                      # H = 8; by hand from lds = 3 F (pb hg D 2 + 16) <= 49152, 16 / 8 units
    if F <= 16:
        hg, pb = {40: 8, 80: 4, 160: 2}[D], 1
        if F <= 2:                         # F = 1, 2: all 8 heads fit at every D (3 * 2 * 2576 bytes), and two pixels of them
            hg, pb = 8, 2
        if F == 15 and D == 40:            # 45 * 1296 = 58320 > 49152: one pixel
            hg, pb = 8, 1
        return MFMA1, hg, pb
    if F == 17:
        return MFMA2, {40: 8, 80: 4, 160: 2}[D], 1          # 51 * (hg D 2 + 16) <= 49152: hg D <= 473
    return MFMA2, {40: 4, 80: 2, 160: 1}[D], 1              # F = 31, 32: hg D <= 256 / 248


FRAME_EDGES = [Case(f"edge F={F} D={D}", 2, F, 3, 8, D, *_edge_plan(F, D)) for D in (40, 80, 160) for F in (1, 2, 15, 16, 17, 31, 32)]

# temporal_attn_kernel<FMAX>: one F from each bucket (4 / 8 / 16 / 32), HG * F lanes per pixel, PB = min(256 / (HG F), 48 KiB / (4 F HG D))
LANE_CASES = [
    Case("lane D=8 F=3 H=8", 1, 3, 11, 8, 8, LANE, 8, 10),             # 11 pixels in tens
    Case("lane D=16 F=5 H=2", 3, 5, 9, 2, 16, LANE, 2, 25),            # 27 pixels in 25s
    Case("lane D=32 F=9 H=8", 1, 9, 7, 8, 32, LANE, 8, 3),             # 7 pixels in threes, 216 of 256 lanes live
    Case("lane D=64 F=17 H=8", 2, 17, 3, 8, 64, LANE, 8, 1),
    Case("lane D=32 F=17 H=2", 2, 17, 5, 2, 32, LANE, 2, 7),           # 10 pixels in sevens
    Case("lane D=64 F=32 H=2", 1, 32, 5, 2, 64, LANE, 2, 3),           # PB capped by LDS (3 x 16 KiB), 5 pixels in threes
]

_FORM_BASES = [("H=8 D=40 F=16", 2, 16, 9, 8, 40, MFMA1, 8, 1), ("H=8 D=160 F=30", 1, 30, 5, 8, 160, MFMA2, 1, 1),
               ("lane D=32 F=9", 1, 9, 7, 8, 32, LANE, 8, 3)]
OPERAND_FORMS = [Case(f"{form} {b[0]}", *b[1:], form=form) for b in _FORM_BASES for form in ("qkv", "pitches")]

PEAKY = [
    Case("peaky D=40 F=16", 2, 16, 9, 8, 40, MFMA1, 8, 1, peaky=True),
    Case("peaky D=80 F=30", 2, 30, 4, 8, 80, MFMA2, 2, 1, peaky=True),
    Case("peaky D=160 F=16", 2, 16, 3, 8, 160, MFMA1, 2, 1, peaky=True),
    Case("peaky lane D=32 F=9", 1, 9, 7, 8, 32, LANE, 8, 3, peaky=True),
]

SCALES = [Case(f"scale x{m} {b[0]}", *b[1:], mult=m) for b in (_FORM_BASES[0], _FORM_BASES[2]) for m in (0.5, 3.0)]

CASES = GEOMETRIES + FRAME_EDGES + LANE_CASES + OPERAND_FORMS + PEAKY + SCALES


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def _problem(NB, F, HW, H, D, code, pb, peaky, mult):
    pr = Problem()
    M, C = NB * F * HW, H * D
    seed = 9000 + 10 * D + F
    pr.q, pr.k, pr.v = rnd(M, C, seed=seed), rnd(M, C, seed=seed + 1), rnd(M, C, seed=seed + 2)
    if peaky:
        # (pixel, head) units of the first and of the last wave: head 0 of the first pixel is unit 0 of its workgroup (wave 0, and wave 0
        # of the lane-per-query kernel); the last head of the first workgroup's last pixel is that workgroup's last unit (its last live
        # wave; lane 207 of 216 at D = 32, F = 9: wave 3); the same of the last pixel, in the partial last workgroup; a pixel in the
        # middle with an inner head.  Query 1 meets its key in frame 3 (the first 16-block), query F - 2 in the last frame.
        npix = NB * HW
        for pix, head in ((0, 0), (pb - 1, H - 1), (npix - 1, H - 1), (npix // 2, H // 2)):
            b, px = divmod(pix, HW)
            row = lambda f: (b * F + f) * HW + px
            cols = slice(head * D, (head + 1) * D)
            pr.k[row(3), cols] = 4 * pr.q[row(1), cols]
            pr.k[row(F - 1), cols] = 4 * pr.q[row(F - 2), cols]
    pr.scale = mult * D ** -0.5
    pr.ref = reference(pr.q, pr.k, pr.v, NB, F, HW, H, D, pr.scale)
    pr.floor = rel_l2(emulation(pr.q, pr.k, pr.v, NB, F, HW, H, D, pr.scale, matrix_core=code != LANE), pr.ref)
    return pr


def problem(case):
    """Seeded inputs (Q, K and V from different seeds), float64 reference and floor of a case; shared and never modified."""
    return _problem(case.NB, case.F, case.HW, case.H, case.D, case.code, case.pb, case.peaky, case.mult)
