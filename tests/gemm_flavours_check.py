"""The cases of tests/test_gemm_flavours_gpu.py (its docstring has the map from plan code to case).  Imported by that file for the automatic
dispatch; run as a script -- `gemm_flavours_check.py pin` under MD_GEMM_SP=1 MD_GEMM_SP_NT=5|4|2|42|32, `gemm_flavours_check.py off` under
MD_GEMM_SP=0 -- for the dispatch knobs, which the library reads once per process.  The script stops at the first failing case (an
exception) and launches nothing after it.

Every case, in this order: (a) ops.gemm_plan / ops.conv_plan on the very tensors of the call must equal the code the case is written for;
(b) three launches into an output pre-filled with NaN (a slice: into a wider buffer pre-filled with 7.0, whose other columns must stay
exactly 7.0) must give identical bits; (c) the pass rule of tests/gemm_ref.py against the float64 reference, with the floor computed for the
case from the reference's own emulation.  References are evaluated with torch in float64 on the device (plain matmul on operands built by
torch indexing).  A, W, bias, row term and residual use different seeds."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemm_ref as R  # noqa: E402
from mikudance_amd import _lib, ops, packing  # noqa: E402

NONE, SILU, RELU, GEGLU, QGELU = ops.ACT_NONE, ops.ACT_SILU, ops.ACT_RELU, ops.ACT_GEGLU, ops.ACT_QUICKGELU
# plan code -> (MT, NT, MD_GEMM_SP_NT pin): gemm.hip sp_tiles; the tile is 64 MT rows x 64 NT columns
TILES = {135: (3, 5, 5), 134: (3, 4, 4), 124: (2, 4, 2), 142: (4, 2, 42), 132: (3, 2, 32)}
PIN_TO_CODE = {pin: code for code, (_, _, pin) in TILES.items()}
CU_LIMIT = 8
FLOOR_MAX = 2.4e-4          # as tests/test_gemm_floor_cpu.py bounds the floor of every epilogue
_count = [0]


def cdiv(a, b):
    return -(-a // b)


class cu_limit:
    """md_set_cu_limit(n) for the block, md_set_cu_limit(0) whatever happens inside (process-wide; mikudance_amd/dp.py is the product's user)."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        assert _lib.load().md_set_cu_limit(self.n) == 0

    def __exit__(self, *exc):
        assert _lib.load().md_set_cu_limit(0) == 0


def _out_buffer(rows, cols, form, dev):
    """(buffer, view the kernel writes).  dense: NaN.  Otherwise 7.0 around the view: slice = [:, 32:32+cols] of cols + 64; mis8 = [:, 4:4+cols]
    of cols + 8 (base 8 bytes off a 16-byte boundary, pitch % 8 == 0); ld4 = [:, :cols] of cols + 4 (pitch % 8 == 4); odd = [:, :cols] of
    cols + 3; wide8 = [:, :cols] of cols + 8 (the transposed store with ldc_t = M + 8); pad8 = [:, :cols] of roundup8(cols), cols % 8 != 0
    (the transposed store as the CLIP vision tower asks for it, ldc_t = pad_to(M, 8): every row 16-byte aligned, a ragged tail in each)."""
    if form == "dense":
        buf = torch.full((rows, cols), float("nan"), dtype=torch.float16, device=dev)
        return buf, buf
    lo, extra = {"slice": (32, 64), "mis8": (4, 8), "ld4": (0, 4), "odd": (0, 3), "wide8": (0, 8), "pad8": (0, -cols % 8)}[form]
    buf = torch.full((rows, cols + extra), 7.0, dtype=torch.float16, device=dev)
    view = buf[:, lo:lo + cols]
    if form == "pad8":
        assert extra > 0 and view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0
    if form == "mis8":
        assert view.data_ptr() % 16 == 8 and view.stride(0) % 8 == 0
    if form in ("ld4", "odd"):
        assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == extra
    return buf, view


def _guard_ok(buf, view, form):
    if form == "dense":
        return True
    lo = view.storage_offset() % buf.stride(0)
    return bool((buf[:, :lo] == 7.0).all()) and bool((buf[:, lo + view.shape[1]:] == 7.0).all())


def _sliced(t, dev, lo, extra, seed):
    """t as the columns [lo, lo + n) of a wider buffer of loud garbage."""
    wide = R.rnd(t.shape[0], t.shape[1] + extra, seed=seed, scale=50.0)
    wide[:, lo:lo + t.shape[1]] = t
    return wide.to(dev)[:, lo:lo + t.shape[1]]


def _run(name, code, plan_fn, launch_fn, rows, cols, out_form, inplace_from, ref, floor, dev):
    buf0, view0 = _out_buffer(rows, cols, out_form, dev)
    got = plan_fn(view0)
    assert got == code, f"{name}: the plan query says {got}, the case is written for {code}"
    outs = []
    # the floor is one fp16 rounding of the output (2.07e-4, tests/test_gemm_floor_cpu.py; 1.9e-4 .. 2.1e-4 over these cases), or exactly 0 on
    # the identity screen: an emulation whose fp32 matmul ran at reduced precision would raise it and loosen the rule unnoticed
    assert floor < FLOOR_MAX, f"{name}: the emulation's own relative L2 {floor:.3e} is not the one-rounding floor (< {FLOOR_MAX})"
    for _ in range(3):
        buf, view = _out_buffer(rows, cols, out_form, dev)
        if inplace_from is not None:
            view.copy_(inplace_from)
        launch_fn(view)
        outs.append((buf, view))
    torch.cuda.synchronize()
    for buf, _ in outs[1:]:
        assert torch.equal(buf.view(torch.int16), outs[0][0].view(torch.int16)), f"{name}: two runs on the same inputs differ"
    assert _guard_ok(*outs[0], out_form), f"{name}: columns outside the output slice were written"
    _count[0] += 1
    R.pass_rule(f"{name} [{code}]", outs[0][1], ref, floor)
    return outs[0][1]


def gemm_case(dev, name, code, M, N, K, bias=True, res=None, rowadd=False, rpg=97, act=NONE, tr=False, a_form="dense", out_form="dense",
              exact=None, seed=0):
    """res: None | dense | inplace | slice (ldr = N + 64) | mis8 (base 8 bytes off).  a_form: dense | slice (lda = K + 64) | zero | eye.
    exact='bias+res': A = 0 must give fp16(bias + residual) bit for bit; exact='w': A = I must give W^T exactly."""
    s = 100 * seed
    a, w = R.rnd(M, K, seed=s + 1), R.rnd(N, K, seed=s + 2, scale=K ** -0.5)
    if a_form == "zero":
        a.zero_()
    elif a_form == "eye":
        a, w = torch.eye(K).half(), ((torch.arange(N * K).reshape(N, K) % 97).half() / 16)
    No = N // 2 if act == GEGLU else N
    b = R.rnd(N, seed=s + 3) if bias else None
    r = R.rnd(M, No, seed=s + 4) if res else None
    ra = R.rnd(cdiv(M, rpg), N, seed=s + 5) if rowadd else None
    d = lambda t: None if t is None else t.to(dev)
    ad, wd, bd, rd, rad = d(a), d(w), d(b), d(r), d(ra)
    epi = dict(bias=bd, rowadd=rad, rows_per_group=rpg if rowadd else 0, residual=rd, act=act, transpose_out=tr)
    ref = R.reference(ad, wd, **epi)
    floor = R.rel_l2(R.emulation(ad, wd, **epi), ref)
    if act == GEGLU:
        wk, bk = packing.geglu_weight(w, b if bias else torch.zeros(N), dev)
        bk = bk if bias else None
    else:
        wk, bk = wd, bd
    ak = _sliced(a, dev, 32, 64, s + 6) if a_form == "slice" else ad
    rk = {None: None, "dense": rd, "inplace": None, "slice": None, "mis8": None}[res]
    if res == "slice":
        rk = _sliced(r, dev, 64, 64, s + 7)
    elif res == "mis8":
        rk = _sliced(r, dev, 4, 8, s + 7)
        assert rk.data_ptr() % 16 == 8
    kw = dict(bias=bk, rowadd=rad, rows_per_group=rpg if rowadd else 0, act=act, transpose_out=tr)
    resid = (lambda view: view) if res == "inplace" else (lambda view: rk)
    rows, cols = (N, M) if tr else (M, No)
    out = _run(name, code, lambda v: ops.gemm_plan(ak, wk, residual=resid(v), out=v, **kw), lambda v: ops.gemm(ak, wk, residual=resid(v), out=v, **kw),
               rows, cols, out_form, rd if res == "inplace" else None, ref, floor, dev)
    if exact == "bias+res":
        assert torch.equal(out, (bd.float() + rd.float()).half()), f"{name}: A = 0 must leave fp16(bias + residual) bit for bit"
    elif exact == "w":
        assert torch.equal(out.float(), wd.float().t() + (bd.float() if bias else 0)), f"{name}: A = I must leave W^T exactly"


def conv_case(dev, name, code, B, H, W, cin, cout, bias=True, res=None, rowadd=False, act=NONE, stride=1, up=False, pad_lo=1, kw=3,
              x_form="dense", out_form="dense", seed=0):
    """x (B, H, W, cin); kw = 1: (clips, frames, pixels, cin).  res: None | dense | inplace.  The row term is one row per image
    (rows_per_group = Hout Wout).  x_form slice: ldx = cin + 192; out_form as gemm_case, on the (pixels, cout) matrix."""
    s = 100 * seed + 50
    x, wpk = R.rnd(B, H, W, cin, seed=s + 1), R.rnd(cout, 3 * kw * cin, seed=s + 2, scale=(3 * kw * cin) ** -0.5)
    xd, wd = x.to(dev), wpk.to(dev)
    A, (Ho, Wo) = R.conv_patches(xd, kw, stride, up, pad_lo)
    M = B * Ho * Wo
    b = R.rnd(cout, seed=s + 3).to(dev) if bias else None
    r = R.rnd(M, cout, seed=s + 4).to(dev) if res else None
    ra = R.rnd(B, cout, seed=s + 5).to(dev) if rowadd else None
    epi = dict(bias=b, rowadd=ra, rows_per_group=Ho * Wo if rowadd else 0, residual=r, act=act)
    ref = R.reference(A, wd, **epi)
    floor = R.rel_l2(R.emulation(A, wd, **epi), ref)
    del A
    xk = _sliced(x.reshape(-1, cin), dev, 192, 192, s + 6).unflatten(0, (B, H, W)) if x_form == "slice" else xd
    kwargs = dict(bias=b, rowadd=ra, rows_per_group=Ho * Wo if rowadd else 0, act=act, stride=stride, upsample=up, pad_lo=pad_lo, kw=kw)
    o4 = lambda v: v.unflatten(0, (B, Ho, Wo))
    resid = (lambda v: o4(v)) if res == "inplace" else (lambda v: None if r is None else r.view(B, Ho, Wo, cout))
    _run(name, code, lambda v: ops.conv_plan(xk, wd, cout, residual=resid(v), out=o4(v), **kwargs),
         lambda v: ops.conv3x3(xk, wd, cout, residual=resid(v), out=o4(v), **kwargs), M, cout, out_form, r if res == "inplace" else None, ref, floor, dev)


# ------------------------------------------------------------------------------------------------ gemm_sp_kernel, one tile under its pin
def sp_gemm_cases(dev, code):
    MT, NT, _ = TILES[code]
    BM, BN, kres = 64 * MT, 64 * NT, 64 * MT * NT
    t = f"sp{code}"
    for K in (128, 192, 256):                                 # two, three, four K tiles against the A ring of three and the W ring of two
        gemm_case(dev, f"{t} ragged tile K={K}", code, 77, BN, K, bias=False, seed=1)
    # the RESM switch: K / 64 >= MT NT + 1 (gemm_sp.h sp_resm); M = BM + 77: a full and a ragged row tile
    M = BM + 77
    gemm_case(dev, f"{t} residual below the switch K={kres}", code, M, BN, kres, res="dense", seed=2)
    K = kres + 64
    gemm_case(dev, f"{t} resm K={K}", 2000 + code, M, BN, K, res="dense", seed=3)
    gemm_case(dev, f"{t} resm no bias", 2000 + code, M, BN, K, bias=False, res="dense", seed=3)
    gemm_case(dev, f"{t} resm residual + row term", 2000 + code, M, BN, K, res="dense", rowadd=True, seed=3)
    gemm_case(dev, f"{t} resm in place", 2000 + code, M, BN, K, res="inplace", seed=3)
    gemm_case(dev, f"{t} resm strided residual", 2000 + code, M, BN, K, res="slice", seed=3)
    gemm_case(dev, f"{t} resm exact screen A=0", 2000 + code, M, BN, K, res="dense", a_form="zero", exact="bias+res", seed=3)
    # tile order: 11 row tiles (no multiple of group_m = 8) x 3 column tiles, the last row tile ragged
    gemm_case(dev, f"{t} tile order 11x3", code, 10 * BM + 50, 3 * BN, 128, seed=4)
    # the persistent grid wraps: 19 tiles on 8 workgroups (2 or 3 each), the last row tile ragged; the plan is asked UNDER the limit
    with cu_limit(CU_LIMIT):
        gemm_case(dev, f"{t} wrapped under the CU limit", code, 18 * BM + 33, BN, 192, seed=5)
        gemm_case(dev, f"{t} resm wrapped under the CU limit", 2000 + code, 18 * BM + 33, BN, K, res="dense", seed=5)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    gemm_case(dev, f"{t} wrapped at the device's count ({ncu} + 44 tiles)", code, (ncu + 43) * BM + 40, BN, 128, seed=6)
    # epilogues at one shape (K = 256: below the RESM switch of every tile but 192 x 128, whose switch is at 448)
    M, K = 300, 256
    gemm_case(dev, f"{t} bias", code, M, BN, K, seed=7)
    gemm_case(dev, f"{t} SiLU leaves the sp kernel", 303, M, BN, K, act=SILU, seed=7)
    gemm_case(dev, f"{t} ReLU leaves the sp kernel", 303, M, BN, K, act=RELU, seed=7)
    gemm_case(dev, f"{t} row term rpg=97", code, M, BN, K, rowadd=True, seed=7)
    gemm_case(dev, f"{t} row term, no bias", code, M, BN, K, bias=False, rowadd=True, seed=7)
    gemm_case(dev, f"{t} bias + residual + row term", code, M, BN, K, res="dense", rowadd=True, seed=7)
    gemm_case(dev, f"{t} residual in place (epilogue form)", code, M, BN, K, res="inplace", seed=7)
    # operand forms
    gemm_case(dev, f"{t} A a column slice", code, M, BN, K, a_form="slice", seed=8)
    gemm_case(dev, f"{t} output a column slice", code, M, BN, K, out_form="slice", seed=8)
    gemm_case(dev, f"{t} residual a slice", code, M, BN, K, res="slice", seed=8)
    gemm_case(dev, f"{t} identity A", code, BN, BN, BN, bias=False, a_form="eye", exact="w", seed=9)


def sp_conv_cases(dev, code):
    MT, NT, _ = TILES[code]
    BN, sub = 64 * NT, MT * NT
    t = f"spconv{code}"
    B, H, W = 3, 13, 11                                       # 429 pixels: ragged against every tile
    resm = lambda ktiles: 2000 + code if ktiles >= sub + 1 else code
    conv_case(dev, f"{t} stride 1", code, B, H, W, 64, BN, seed=1)
    conv_case(dev, f"{t} stride 2 odd side", code, B, H, W, 64, BN, stride=2, seed=1)
    conv_case(dev, f"{t} stride 2 pad_lo=0 odd side", code, B, H, W, 64, BN, stride=2, pad_lo=0, seed=1)
    conv_case(dev, f"{t} stride 2 pad_lo=0 even side", code, B, 12, 10, 64, BN, stride=2, pad_lo=0, seed=2)
    conv_case(dev, f"{t} folded upsample", code, B, H, W, 64, BN, up=True, seed=1)
    conv_case(dev, f"{t} kw=1 frames=1", code, 2, 1, 50, 128, BN, kw=1, seed=3)
    conv_case(dev, f"{t} kw=1 frames=5", code, 2, 5, 50, 128, BN, kw=1, seed=4)
    conv_case(dev, f"{t} input a channel slice", code, B, H, W, 64, BN, x_form="slice", seed=1)
    conv_case(dev, f"{t} output a channel slice", code, B, H, W, 64, BN, out_form="slice", seed=1)
    # residual + one row of the row term per image; and RESM either side of its switch (K tiles: 6 = kw 1 x 128, 9 = 3 x 3 x 64, 18 = 3 x 3 x 128)
    lo, hi = (9, 18) if sub + 1 > 9 else (6, 9)
    shape = {6: dict(kw=1, cin=128), 9: dict(kw=3, cin=64), 18: dict(kw=3, cin=128)}
    for kt in (lo, hi):
        sh = shape[kt]
        conv_case(dev, f"{t} residual + row term, {kt} K tiles", resm(kt), B, H, W, sh["cin"], BN, res="dense", rowadd=True, kw=sh["kw"], seed=5)
        conv_case(dev, f"{t} residual in place, {kt} K tiles", resm(kt), B, H, W, sh["cin"], BN, res="inplace", kw=sh["kw"], seed=5)
    with cu_limit(CU_LIMIT):                                  # 8 x 24 x 24 = 4608 pixels: 18 / 24 / 36 row tiles on 8 workgroups
        conv_case(dev, f"{t} wrapped under the CU limit", code, 8, 24, 24, 64, BN, seed=6)
        conv_case(dev, f"{t} resm wrapped under the CU limit", resm(18), 8, 24, 24, 128, BN, res="dense", seed=6)


def transposed_pinned_cases(dev, code):
    """MD_GEMM_SP=1 with the 192 x 256 (1134) or 128 x 256 (1124) tile pinned: the swapped problem has N = 320 ROWS, ragged against both."""
    for M in (256, 512):
        gemm_case(dev, f"transposed M={M} bias", 1000 + code, M, 320, 128, tr=True, seed=11)
        gemm_case(dev, f"transposed M={M}", 1000 + code, M, 320, 128, bias=False, tr=True, seed=11)
        gemm_case(dev, f"transposed M={M} ldc_t=M+8", 1000 + code, M, 320, 192, tr=True, out_form="wide8", seed=12)
    # M = 257 (the CLIP tower's token count) is the swapped problem's N and no multiple of the 256-column tile: sp_eligible turns the
    # swapped problem down under either pin (md_gemm_plan_call on the CPU: 303), so the ragged transposed store of gemm_kernel runs here too
    gemm_case(dev, "transposed M=257 ldc_t=264 leaves the sp kernel", 303, 257, 320, 128, tr=True, out_form="pad8", seed=13)
    gemm_case(dev, "transposed M=257 ldc_t=257 leaves the sp kernel", 303, 257, 320, 128, tr=True, seed=13)


def geglu_sp_cases(dev):
    """MD_GEMM_SP=1: the 256 x 256 GEGLU tile at every K (the automatic dispatch takes it from K = 640 on)."""
    gemm_case(dev, "geglu sp K=128 ragged M=200", 144, 200, 512, 128, act=GEGLU, seed=21)
    gemm_case(dev, "geglu sp K=640 ragged M=200", 144, 200, 512, 640, act=GEGLU, seed=22)
    gemm_case(dev, "geglu sp no bias", 144, 200, 512, 128, bias=False, act=GEGLU, seed=21)
    gemm_case(dev, "geglu sp output a slice", 144, 200, 512, 128, act=GEGLU, out_form="slice", seed=21)
    with cu_limit(CU_LIMIT):                                  # 10 x 2 tiles on 8 workgroups, the last row tile ragged
        gemm_case(dev, "geglu sp wrapped under the CU limit", 144, 9 * 256 + 40, 512, 128, act=GEGLU, seed=23)


# ------------------------------------------------------------------------------------------------ automatic dispatch (in process)
def transposed_auto_cases(dev):
    """MD_GEMM_SP=2: the swapped sp kernel needs tiles >= 112 && K >= 256 (gemm.hip gemm_choose_kernel); N = 1280 rows of the swapped problem
    are 10 tiles of 128 x 256, M / 256 column tiles."""
    gemm_case(dev, "transposed auto 120 tiles K=256", 1124, 3072, 1280, 256, tr=True, seed=31)
    gemm_case(dev, "transposed auto 110 tiles K=256", 303, 2816, 1280, 256, tr=True, seed=32)
    gemm_case(dev, "transposed auto 120 tiles K=192", 303, 3072, 1280, 192, tr=True, seed=33)
    gemm_case(dev, "transposed auto 303 ldc_t=M+8", 303, 256, 320, 128, tr=True, out_form="wide8", seed=34)


def transposed_ragged_cases(dev):
    """gemm_kernel's transposed epilogue stores 8 rows m .. m + 7 of one column n as one 16-byte piece of C^T[n]; M % 8 != 0 leaves a last
    piece of M % 8 elements for the scalar branch (`m + 8 <= p.M` fails), and a row of C^T that is not 16-byte aligned takes the scalar
    branch for every piece.  M = 257 (ViT-L/14's token count: a tail of ONE element, in the second 256-row tile) and 261 (a tail of five);
    pitch roundup8(M) as the tower asks for it (ldc_t = pad_to(L, 8); columns [M, pitch) start as 7.0 and must stay 7.0: the epilogue does
    not write them) and pitch M (odd: only every eighth row of C^T is aligned)."""
    for M in (257, 261):
        gemm_case(dev, f"transposed ragged M={M} ldc_t={M + -M % 8}", 303, M, 128, 128, tr=True, out_form="pad8", seed=35)
        gemm_case(dev, f"transposed ragged M={M} ldc_t={M}", 303, M, 128, 128, tr=True, seed=35)


M_STREAM = 32768 + 16 * 7


def streaming_cases(dev, N, K):
    """wsgemm_kernel<KS = K / 32, TPR = 1 (one column group) | 2, RES, RA>: the four (residual, row term) instantiations of one
    (K depth, tiles per round) pair; rows_per_group = 5000 is no multiple of the 16-row tile."""
    code, M, t = (210 if K == 320 else 220), M_STREAM, f"ws N={N} K={K}"
    gemm_case(dev, f"{t} plain", code, M, N, K, seed=41)
    gemm_case(dev, f"{t} residual", code, M, N, K, res="dense", seed=41)
    gemm_case(dev, f"{t} row term only", code, M, N, K, rowadd=True, rpg=5000, seed=41)
    gemm_case(dev, f"{t} row term only, no bias", code, M, N, K, bias=False, rowadd=True, rpg=5000, seed=41)
    gemm_case(dev, f"{t} residual + row term", code, M, N, K, res="dense", rowadd=True, rpg=5000, seed=41)
    gemm_case(dev, f"{t} residual in place", code, M, N, K, res="inplace", seed=41)
    gemm_case(dev, f"{t} A and C column slices", code, M, N, K, a_form="slice", out_form="slice", seed=42)


def streaming_edge_cases(dev):
    gemm_case(dev, "ws M % 16 = 8 leaves the streaming kernel", 303, 32768 + 8, 320, 320, res="dense", seed=43)
    gemm_case(dev, "ws geglu", 230, M_STREAM, 512, 320, act=GEGLU, seed=44)
    gemm_case(dev, "ws geglu output a slice", 230, M_STREAM, 512, 320, act=GEGLU, out_form="slice", seed=44)


def geglu_auto_cases(dev):
    gemm_case(dev, "geglu auto K=640", 144, 200, 512, 640, act=GEGLU, seed=22)
    gemm_case(dev, "geglu 303 K=128", 303, 200, 512, 128, act=GEGLU, seed=21)
    gemm_case(dev, "geglu 302 K=128 packed N=1024", 302, 32768 + 5, 1024, 128, act=GEGLU, seed=45)


def occupancy_small_cases(dev):
    for N in (4, 64):
        gemm_case(dev, f"301 gemm N={N}", 301, 300, N, 128, res="dense", rowadd=True, seed=51)
        conv_case(dev, f"301 conv Cout={N}", 301, 3, 13, 11, 64, N, res="dense", rowadd=True, seed=51)
        conv_case(dev, f"301 conv Cout={N} stride 2 pad_lo=0", 301, 3, 13, 11, 64, N, stride=2, pad_lo=0, seed=51)
    for N in (200, 1288):
        gemm_case(dev, f"303 gemm N={N}", 303, 300, N, 128, res="dense", rowadd=True, seed=52)
        gemm_case(dev, f"303 gemm N={N} SiLU", 303, 300, N, 128, act=SILU, seed=52)
    conv_case(dev, "303 conv Cout=200 stride 2 pad_lo=0", 303, 3, 13, 11, 64, 200, stride=2, pad_lo=0, res="dense", seed=53)
    conv_case(dev, "303 conv Cout=200 upsample", 303, 3, 13, 11, 64, 200, up=True, rowadd=True, seed=53)


def occupancy_302_conv(dev):
    conv_case(dev, "302 conv Cout=192, 131072 pixels", 302, 8, 128, 128, 64, 192, res="dense", rowadd=True, seed=54)


def occupancy_302_gemm(dev):
    gemm_case(dev, "302 gemm K=2048 N=1288", 302, 24064 + 5, 1288, 2048, res="dense", seed=55)


def alignment_cases(dev):
    """M = 4608, N = 1280, K = 640 takes an sp tile by itself; each misalignment ALONE sends it to gemm_kernel, which must cope with it."""
    M, N, K = 4608, 1280, 640
    gemm_case(dev, "aligned base case", 2132, M, N, K, res="dense", seed=61)
    gemm_case(dev, "output base 8 bytes off", 303, M, N, K, res="dense", out_form="mis8", seed=61)
    gemm_case(dev, "output pitch % 8 = 4", 303, M, N, K, res="dense", out_form="ld4", seed=61)
    gemm_case(dev, "residual base 8 bytes off", 303, M, N, K, res="mis8", seed=61)
    # 8 x 48 x 48 pixels, 64 -> 256 channels: 192 tiles of 192 x 128
    conv_case(dev, "conv aligned base case", 132, 8, 48, 48, 64, 256, seed=62)
    conv_case(dev, "conv output through an odd pitch", 303, 8, 48, 48, 64, 256, out_form="odd", seed=62)
    conv_case(dev, "conv SiLU", 303, 8, 48, 48, 64, 256, act=SILU, seed=62)
    conv_case(dev, "conv ReLU", 303, 8, 48, 48, 64, 256, act=RELU, rowadd=True, seed=62)


def quickgelu_cases(dev):
    """MD_ACT_QUICKGELU (fc1 of the CLIP vision tower's MLP): like SiLU / ReLU it leaves the sp and the streaming kernels, so the automatic
    dispatch reaches every flavour of gemm_kernel that can carry it.  M = 257 is ragged against the 128-row tile; N = 200: the last group
    of 8 columns of a row is the scalar path (nv < 8).  The residual must enter AFTER the activation (tests/gemm_ref.py _epilogue), the
    row term before it."""
    M, N, K = 257, 200, 128
    gemm_case(dev, "quickgelu bias", 303, M, N, K, act=QGELU, seed=81)
    gemm_case(dev, "quickgelu no bias", 303, M, N, K, bias=False, act=QGELU, seed=81)
    gemm_case(dev, "quickgelu bias + residual", 303, M, N, K, res="dense", act=QGELU, seed=81)
    gemm_case(dev, "quickgelu bias + row term rpg=97", 303, M, N, K, rowadd=True, act=QGELU, seed=81)
    gemm_case(dev, "quickgelu output a column slice", 303, M, N, K, act=QGELU, out_form="slice", seed=81)
    gemm_case(dev, "quickgelu output pitch % 8 = 4", 303, M, N, K, act=QGELU, out_form="ld4", seed=81)
    gemm_case(dev, "quickgelu 301 bias + residual", 301, 300, 64, 128, res="dense", act=QGELU, seed=82)
    # 302 takes a plain GEMM from K = 2048 on (gemm_choose_kernel: conv || geglu || K >= 2048): at the shape of `geglu 302` (K = 128) the
    # call query answers 303 for this activation, at the shape of `302 gemm K=2048 N=1288` it answers 302
    gemm_case(dev, "quickgelu M=32768+5 N=1024 K=128", 303, 32768 + 5, 1024, 128, act=QGELU, seed=83)
    gemm_case(dev, "quickgelu 302 K=2048 N=1288", 302, 24064 + 5, 1288, 2048, act=QGELU, seed=83)
    conv_case(dev, "quickgelu conv Cout=200", 303, 3, 13, 11, 64, 200, act=QGELU, seed=84)


QUICKGELU_SCREEN = (-65504.0, -1000.0, -100.0, -60.0, -20.0, -1.0, -0.0, 0.0, 1.0, 20.0, 100.0, 65504.0)


def _ordered(t):
    """fp16 -> integers in the order of the values (both zeros 0): neighbours in fp16 differ by 1."""
    bits = t.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(bits < 0x8000, bits, 0x8000 - bits)


def quickgelu_screen(dev, code, M, N, K):
    """A = 0: every output element is quickgelu(bias[n]).  The kernel forms v / (1 + exp(-1.702 v)); from v <= -52.2 on the exponential is
    beyond fp32 (exp(88.7)) and must come out as +Inf so that the quotient is a ZERO -- a NaN (Inf / Inf, 0 x Inf) or a flush of the
    denominator would show here and in no random case (|pre-activation| < 6 there).  Finite everywhere, within one fp16 ulp of
    fp16(float64 x sigmoid(1.702 x)), magnitude 0 for every bias <= -60; three launches with identical bits."""
    a = torch.zeros(M, K, dtype=torch.float16, device=dev)
    w = R.rnd(N, K, seed=8501, scale=K ** -0.5).to(dev)
    bias = torch.tensor([QUICKGELU_SCREEN[n % len(QUICKGELU_SCREEN)] for n in range(N)], dtype=torch.float16, device=dev)
    name = f"quickgelu exact screen {M}x{N} [{code}]"
    outs = []
    for _ in range(3):
        out = torch.full((M, N), float("nan"), dtype=torch.float16, device=dev)
        got = ops.gemm_plan(a, w, bias=bias, act=QGELU, out=out)
        assert got == code, f"{name}: the plan query says {got}, the case is written for {code}"
        ops.gemm(a, w, bias=bias, act=QGELU, out=out)
        outs.append(out)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{name}: two runs on the same inputs differ"
    out = outs[0]
    b64 = bias.double()
    want = (b64 * torch.sigmoid(1.702 * b64)).half()
    ulps = (_ordered(out) - _ordered(want)[None, :]).abs()
    print(f"PARITY_MEASURE gemm_flavour:{name} floor=1ulp got={int(ulps.max())}ulp nonfinite={int((~torch.isfinite(out)).sum())}", flush=True)
    assert bool(torch.isfinite(out).all()), f"{name}: non-finite output in columns {sorted(set((~torch.isfinite(out)).nonzero()[:, 1].tolist()))[:12]}"
    assert int(ulps.max()) <= 1, f"{name}: {int(ulps.max())} fp16 ulps from quickgelu(bias)"
    assert bool((out[:, bias <= -60.0] == 0).all()), f"{name}: a bias <= -60 must give a zero"
    assert torch.equal(out[:, bias == 65504.0], torch.full_like(out[:, bias == 65504.0], 65504.0)), f"{name}: quickgelu(65504) is 65504"
    _count[0] += 1


def quickgelu_screen_cases(dev):
    quickgelu_screen(dev, 303, 257, 200, 128)
    quickgelu_screen(dev, 301, 300, 64, 128)


def refused_act_case(dev):
    """An `act` that is none of MD_ACT_*: MD_ERR_ARG from the launch and from both call queries, nothing launched, the output untouched
    (before the check existed such a value ran as MD_ACT_NONE).  MD_ACT_GEGLU on a conv likewise."""
    lib = _lib.load()
    M, N, K = 257, 200, 128
    a, w, b = R.rnd(M, K, seed=8601).to(dev), R.rnd(N, K, seed=8602).to(dev), R.rnd(N, seed=8603).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    for act in (5, -1, 255):
        out = torch.full((M, N), 7.0, dtype=torch.float16, device=dev)
        args = (a.data_ptr(), K, w.data_ptr(), out.data_ptr(), N, M, N, K, b.data_ptr(), None, 0, None, 0, 0, act, 0)
        assert lib.md_gemm_plan_call(*args, None, None) == -1, act                     # MD_ERR_ARG
        assert lib.md_gemm_f16(*args, st) == -1 and b"act=" in lib.md_last_error(), act
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), f"act={act}: refused, but the output was written"
    x, wc = R.rnd(3, 13, 11, 64, seed=8604).to(dev), R.rnd(200, 576, seed=8605).to(dev)
    for act in (5, GEGLU):
        y = torch.full((3, 13, 11, 200), 7.0, dtype=torch.float16, device=dev)
        args = (x.data_ptr(), 64, wc.data_ptr(), y.data_ptr(), 200, 3, 13, 11, 64, 200, 3, 1, 0, 1, b.data_ptr(), None, 0, None, 0, 0, act)
        assert lib.md_conv_plan_call(*args) == -1, act
        assert lib.md_conv_nhwc_f16(*args, st) == -1 and b"act=" in lib.md_last_error(), act
        torch.cuda.synchronize()
        assert bool((y == 7.0).all()), f"conv act={act}: refused, but the output was written"
    _count[0] += 1


def sp_off_cases(dev):
    """MD_GEMM_SP=0, the baseline of tests/test_full_size_gpu.py: the same problems on gemm_kernel."""
    gemm_case(dev, "sp off: the RESM-depth GEMM", 303, 4608, 1280, 1024, res="dense", seed=71)
    conv_case(dev, "sp off: conv 8 x 128 x 128, 64 -> 256", 302, 8, 128, 128, 64, 256, seed=72)
    conv_case(dev, "sp off: conv stride 2 pad_lo=0", 303, 3, 13, 11, 64, 256, stride=2, pad_lo=0, res="dense", seed=73)


def main(mode):
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda:0")
    sp, nt = os.environ.get("MD_GEMM_SP"), int(os.environ.get("MD_GEMM_SP_NT", "0"))
    if mode == "pin":
        assert sp == "1" and nt in PIN_TO_CODE, "run with MD_GEMM_SP=1 and MD_GEMM_SP_NT=5|4|2|42|32"
        code = PIN_TO_CODE[nt]
        sp_gemm_cases(dev, code)
        sp_conv_cases(dev, code)
        if code in (134, 124):
            transposed_pinned_cases(dev, code)
        if code == 135:
            geglu_sp_cases(dev)
    else:
        assert mode == "off" and sp == "0", "run with MD_GEMM_SP=0"
        sp_off_cases(dev)
    print(f"ALL OK {_count[0]} cases")


if __name__ == "__main__":
    main(sys.argv[1])
