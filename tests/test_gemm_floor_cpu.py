"""CPU: the yardstick of tests/test_gemm_flavours_gpu.py.  That file requires rel_l2(kernel) <= 1.25 x rel_l2(emulation), both against the
float64 reference of tests/gemm_ref.py.  Here: the conv reference (written out from shifted slices) agrees with F.conv2d / F.conv3d in
float64 on small cases of every form; the floor of a plain case is the fp16 output rounding and nothing else; and two degradations that
every elementwise bound of the suite lets through land above the factor, so the rule has teeth.

Measured here (relative L2 against float64 A W^T, fp16-rounded N(0,1) / N(0,1/K) operands):
    M x N x K            floor       fp16 partial sums per 64-deep K tile
    900 x 640 x 256      2.074e-4    3.275e-4 (1.58 x)
    900 x 320 x 640      2.073e-4    4.866e-4 (2.35 x)
    1152 x 1280 x 1280   2.074e-4    6.721e-4 (3.24 x)
and the tanh GELU in a GEGLU epilogue: 1.39 x (K = 128) and 1.40 x (K = 640) its case's floor."""
import pytest
import torch
import torch.nn.functional as F

from gemm_ref import (ACT_GEGLU, ACT_NONE, ACT_QUICKGELU, ACT_RELU, ACT_SILU, KERNEL_FACTOR, conv_emulation, conv_patches, conv_reference,
                      emulation, reference, rel_l2, rnd)


def _unpack3x3(wpk, cin):                              # [Cout, (ky, kx, c)] -> [Cout, Cin, 3, 3]
    return wpk.reshape(wpk.shape[0], 3, 3, cin).permute(0, 3, 1, 2)


@pytest.mark.parametrize("h,wd,stride,up,pad_lo", [(13, 11, 1, False, 1), (13, 11, 2, False, 1), (12, 10, 2, False, 1), (13, 11, 2, False, 0),
                                                   (12, 10, 2, False, 0), (7, 5, 1, True, 1), (1, 1, 1, False, 1), (2, 2, 2, False, 0)])
def test_conv_reference_is_conv2d(h, wd, stride, up, pad_lo):
    B, cin, cout = 2, 8, 5
    x, wpk = rnd(B, h, wd, cin, seed=1), rnd(cout, 9 * cin, seed=2, scale=(9 * cin) ** -0.5)
    bias = rnd(cout, seed=3)
    xin = x.double().permute(0, 3, 1, 2)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    if pad_lo == 0:
        want = F.conv2d(F.pad(xin, (0, 1, 0, 1)), _unpack3x3(wpk, cin).double(), bias.double(), stride=stride, padding=0)
    else:
        want = F.conv2d(xin, _unpack3x3(wpk, cin).double(), bias.double(), stride=stride, padding=1)
    got = conv_reference(x, wpk, stride=stride, upsample=up, pad_lo=pad_lo, bias=bias)
    assert got.dtype == torch.float64 and got.shape == want.permute(0, 2, 3, 1).shape
    assert float((got - want.permute(0, 2, 3, 1)).abs().max()) < 1e-12


@pytest.mark.parametrize("frames", [1, 5])
def test_conv_reference_kw1_is_conv3d_3x1x1(frames):
    clips, hw, c, cout = 2, 6, 8, 5
    x, w3 = rnd(clips, frames, hw, c, seed=4), rnd(cout, c, 3, seed=5)
    wpk = w3.permute(0, 2, 1).reshape(cout, 3 * c).contiguous()               # (ky, c)
    want = F.conv3d(x.double().permute(0, 3, 1, 2)[..., None], w3.double()[..., None, None], padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1)
    got = conv_reference(x, wpk, kw=1)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12


def test_conv_reference_epilogue_and_patch_order():
    """Row term per image, residual last; the patch matrix of a one-hot image puts channel c of tap (ky, kx) in column (3 ky + kx) Cin + c."""
    B, h, wd, cin, cout = 3, 4, 5, 8, 6
    x, wpk = rnd(B, h, wd, cin, seed=6), rnd(cout, 9 * cin, seed=7)
    bias, temb, res = rnd(cout, seed=8), rnd(B, cout, seed=9), rnd(B, h, wd, cout, seed=10)
    base = conv_reference(x, wpk)
    got = conv_reference(x, wpk, bias=bias, rowadd=temb, rows_per_group=h * wd, residual=res)
    want = base + bias.double() + temb.double()[:, None, None, :] + res.double()
    assert float((got - want).abs().max()) < 1e-12
    one = torch.zeros(1, 3, 3, cin, dtype=torch.float16)
    one[0, 0, 2, 5] = 1.0                                                     # pixel (y = 0, x = 2), channel 5
    A, (ho, wo) = conv_patches(one)
    row = 1 * wo + 1                                                          # output pixel (1, 1) sees it through tap (ky = 0, kx = 2)
    assert (ho, wo) == (3, 3) and A[row].nonzero().flatten().tolist() == [(3 * 0 + 2) * cin + 5]


def test_reference_epilogues():
    M, N, K = 50, 16, 64
    a, w = rnd(M, K, seed=11), rnd(N, K, seed=12, scale=K ** -0.5)
    bias, radd, res = rnd(N, seed=13), rnd(8, N, seed=14), rnd(M, N, seed=15)
    base = a.double() @ w.double().t()
    full = base + bias.double() + radd.double().repeat_interleave(7, 0)[:M]
    assert torch.equal(reference(a, w, bias=bias, rowadd=radd, rows_per_group=7, residual=res), full + res.double())
    assert torch.equal(reference(a, w, bias=bias, act=ACT_SILU), F.silu(base + bias.double()))
    assert torch.equal(reference(a, w, bias=bias, act=ACT_RELU), F.relu(base + bias.double()))
    assert torch.equal(reference(a, w, bias=bias, transpose_out=True), (base + bias.double()).t())
    # QuickGELU x sigmoid(1.702 x), written here the other way (x / (1 + exp(-1.702 x))); bias and row term before it, the residual after it
    qg = lambda x: x / (1.0 + torch.exp(-1.702 * x))
    assert float((reference(a, w, bias=bias, act=ACT_QUICKGELU) - qg(base + bias.double())).abs().max()) < 1e-14
    got = reference(a, w, bias=bias, rowadd=radd, rows_per_group=7, residual=res, act=ACT_QUICKGELU)
    assert float((got - (qg(full) + res.double())).abs().max()) < 1e-14
    assert float((got - qg(full + res.double())).abs().max()) > 0.1              # the other order is another function
    assert emulation(a, w, bias=bias, act=ACT_QUICKGELU).dtype == torch.float16
    hg = base + bias.double()
    assert float((reference(a, w, bias=bias, act=ACT_GEGLU) - hg[:, :8] * F.gelu(hg[:, 8:])).abs().max()) < 1e-14
    assert emulation(a, w, bias=bias, residual=res).dtype == torch.float16


def _plain(M, N, K):
    return rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)


def test_floor_of_a_plain_case_is_one_fp16_rounding():
    a, w = _plain(900, 640, 256)
    ref = reference(a, w)
    floor = rel_l2(emulation(a, w), ref)
    print(f"\nPARITY_MEASURE gemm_floor_cpu:plain floor={floor:.6e} one_rounding={rel_l2(ref.half(), ref):.6e}")
    assert abs(floor - 2.07e-4) <= 0.05 * 2.07e-4, floor
    assert abs(rel_l2(ref.half(), ref) - floor) <= 1e-3 * floor                # fp32 accumulation costs nothing visible next to the rounding
    x, wpk = rnd(3, 13, 11, 64, seed=3), rnd(128, 576, seed=4, scale=576 ** -0.5)
    cfloor = rel_l2(conv_emulation(x, wpk), conv_reference(x, wpk))
    assert abs(cfloor - 2.07e-4) <= 0.05 * 2.07e-4, cfloor


def _fp16_partial_sums(a, w, tile=64):
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float16)
    for k in range(0, a.shape[1], tile):
        acc = (acc.float() + a[:, k:k + tile].float() @ w[:, k:k + tile].float().t()).half()
    return acc


@pytest.mark.parametrize("M,N,K", [(900, 320, 640), (1152, 1280, 1280)])
def test_fp16_partial_sums_per_k_tile_land_above_the_factor(M, N, K):
    """A kernel that loses its fp32 accumulation (the accumulators rounded to fp16 once per 64-deep K tile) passes |err| <= 1e-2 max|ref| +
    1e-3 with a margin of 50 x; against the floor it sits at 2.3 x (K = 640) and 3.2 x (K = 1280)."""
    a, w = _plain(M, N, K)
    ref = reference(a, w)
    floor, bad = rel_l2(emulation(a, w), ref), rel_l2(_fp16_partial_sums(a, w), ref)
    print(f"\nPARITY_MEASURE gemm_floor_cpu:fp16_partials K={K} floor={floor:.6e} degraded={bad:.6e} ({bad / floor:.2f} x)")
    assert float((_fp16_partial_sums(a, w).double() - ref).abs().max()) <= 1e-2 * float(ref.abs().max()) + 1e-3      # the old bound lets it through
    assert bad > KERNEL_FACTOR * floor, (bad, floor)


def _gelu_tanh(x):
    x = x.float()
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608 * (x + 0.044715 * x * x * x)))


@pytest.mark.parametrize("K,inner", [(128, 256), (640, 256)])
def test_tanh_gelu_in_geglu_lands_above_the_factor(K, inner):
    a, w, b = rnd(600, K, seed=11), rnd(2 * inner, K, seed=12, scale=K ** -0.5), rnd(2 * inner, seed=13)
    ref = reference(a, w, bias=b, act=ACT_GEGLU)
    floor = rel_l2(emulation(a, w, bias=b, act=ACT_GEGLU), ref)
    bad = rel_l2(emulation(a, w, bias=b, act=ACT_GEGLU, gelu=_gelu_tanh), ref)
    print(f"\nPARITY_MEASURE gemm_floor_cpu:geglu_tanh K={K} floor={floor:.6e} degraded={bad:.6e} ({bad / floor:.2f} x)")
    assert 1.5e-4 < floor < 3e-4, floor
    assert bad > KERNEL_FACTOR * floor, (bad, floor)


def test_emulation_of_every_epilogue_sits_at_one_rounding():
    """Bias, row term, residual, SiLU / ReLU / QuickGELU in fp32 and one rounding: the floor stays the output rounding (1.9e-4 .. 2.3e-4) for
    every form (QuickGELU measured: 2.05e-4 alone or with a bias, 2.08e-4 / 2.09e-4 with a residual / a row term; the printed lines say so)."""
    M, N, K = 400, 128, 192
    a, w = rnd(M, K, seed=21), rnd(N, K, seed=22, scale=K ** -0.5)
    bias, radd, res = rnd(N, seed=23), rnd(5, N, seed=24), rnd(M, N, seed=25)
    for kw in (dict(bias=bias), dict(bias=bias, residual=res), dict(rowadd=radd, rows_per_group=97), dict(bias=bias, act=ACT_SILU),
               dict(bias=bias, act=ACT_RELU), dict(bias=bias, rowadd=radd, rows_per_group=97, residual=res), dict(transpose_out=True),
               dict(act=ACT_NONE), dict(bias=bias, act=ACT_QUICKGELU), dict(act=ACT_QUICKGELU),
               dict(bias=bias, residual=res, act=ACT_QUICKGELU), dict(bias=bias, rowadd=radd, rows_per_group=97, act=ACT_QUICKGELU)):
        floor = rel_l2(emulation(a, w, **kw), reference(a, w, **kw))
        if kw.get("act") == ACT_QUICKGELU:
            print(f"\nPARITY_MEASURE gemm_floor_cpu:quickgelu {'+'.join(sorted(k for k in kw if k not in ('act', 'rows_per_group')))} floor={floor:.6e}")
        assert 1.8e-4 < floor < 2.4e-4, (sorted(kw), floor)
