"""GPU: the CLIP vision tower (mikudance_amd/clip_vision.py) one step above its kernels -- ONE encoder layer and the embeddings against a
float64 restatement (tests/clip_ref.py) -- where tests/test_clip_gpu.py holds the final embeddings, 24 layers and two LayerNorms later, to
relative L2 < 2e-2.  The kernels themselves are in tests/test_gemm_flavours_gpu.py (QuickGELU, the ragged transposed store) and
tests/test_attention_flavours_gpu.py (the tower's plan-400 call).  As there: the plan of every call is asserted before anything is
launched, three runs must give identical bits, outputs start as NaN, floors come from the references' own emulation per case.

Layer: |err| <= 1e-2 max|ref| + 1e-3 (the operator bound of tests/test_blocks_gpu.py) and relative L2 <= parity_budget.FACTOR (2.0: the
constant for composed paths, as tests/attention_ref.py uses it for accumulation-order noise) x the floor, the relative L2 of the
restatement built from the fp32 emulations against the one built from the float64 references.  Both round to fp16 where the product
materialises a tensor (tests/clip_ref.py says why), so value and floor are both made of the elements whose LAST rounding fell the other
way because an input differed upstream: 37 - 40 % of them for the emulation, one fp16 ulp each (floor 3.0e-4 at dim 1024, 3.2e-4 at dim
128; tests/test_clip_ref_cpu.py).
Embeddings: row 0 bit for bit; rows 1.. under the GEMM pass rule (tests/gemm_ref.py) against float64 patches . W^T + pos[1:].
profiles/clip_kernel_tests.log has every figure measured on the MI355X."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import attention_ref  # noqa: E402
import clip_ref  # noqa: E402
import gemm_ref as R  # noqa: E402
from norm_ref import LN, ln_problem  # noqa: E402
from parity_budget import FACTOR  # noqa: E402

from mikudance_amd import _lib, ops, packing  # noqa: E402
from mikudance_amd.clip_vision import CLIPVisionTransformer, _ClipLayer  # noqa: E402

EPS = 1e-5
GEMM_KERNEL_128, GENERIC_ATTENTION = 303, 400


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _layer_module(w, dim, inner, heads, dev):
    m = _ClipLayer(dim, inner, heads, EPS)
    a = m.self_attn
    pairs = dict(n1=m.layer_norm1, n2=m.layer_norm2, q=a.q_proj, k=a.k_proj, v=a.v_proj, o=a.out_proj, f1=m.mlp.fc1, f2=m.mlp.fc2)
    with torch.no_grad():
        for name, mod in pairs.items():
            mod.weight.copy_(w[name + "w"])
            mod.bias.copy_(w[name + "b"])
    return m.to(device=dev, dtype=torch.float16)


def _assert_layer_plans(x, dim, inner, heads, L):
    """The seven launches of _ClipLayer.forward on tensors of the very shapes and pitches it uses: gemm_kernel's 128 x 128 flavour for every
    GEMM (M = L is far too short for the sp and the streaming kernels) and the generic attention kernel (roundup8(L) > kv_stride = L)."""
    dev = x.device
    e = lambda *s: torch.empty(s, dtype=torch.float16, device=dev)
    assert ops.gemm_plan(x, e(2 * dim, dim), bias=e(2 * dim)) == GEMM_KERNEL_128
    vt = e(dim, packing.pad_to(L, 8))
    assert ops.gemm_plan(x, e(dim, dim), bias=e(dim), transpose_out=True, out=vt[:, :L]) == GEMM_KERNEL_128
    assert ops.gemm_plan(x, e(dim, dim), bias=e(dim), residual=e(L, dim)) == GEMM_KERNEL_128
    assert ops.gemm_plan(x, e(inner, dim), bias=e(inner), act=ops.ACT_QUICKGELU) == GEMM_KERNEL_128
    assert ops.gemm_plan(e(L, inner), e(dim, inner), bias=e(dim), residual=e(L, dim)) == GEMM_KERNEL_128
    assert _lib.load().md_layernorm_plan(L, dim) > 0
    assert _lib.load().md_attention_plan(dim // heads, L, L, L, vt.stride(0), int(vt.data_ptr() % 16 == 0)) == GENERIC_ATTENTION


@pytest.mark.parametrize("dim,inner,heads,L", [(128, 256, 4, 17),            # the reduced tower of tests/test_clip_gpu.py
                                               (1024, 4096, 16, 257)])       # ViT-L/14
def test_one_encoder_layer_against_float64(dev, dim, inner, heads, L):
    w = clip_ref.layer_weights(dim, inner, seed=9100 + dim)
    x = ln_problem(LN("clip layer input", L, dim, 0, EPS)).x          # per-row mean ~ N(0, 1), spread 0.5 .. 1.5
    ref = clip_ref.layer(x, w, heads, EPS, exact=True)
    floor = attention_ref.rel_l2(clip_ref.layer(x, w, heads, EPS, exact=False), ref)
    m = _layer_module(w, dim, inner, heads, dev)
    xd = x.to(dev)
    _assert_layer_plans(xd, dim, inner, heads, L)
    with torch.no_grad():
        outs = [m(xd, L) for _ in range(3)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), "two runs on the same inputs differ"
    assert torch.equal(xd.cpu(), x), "the layer wrote into its input"
    got = outs[0].cpu().double()
    value = attention_ref.rel_l2(got, ref)
    print(f"\nPARITY_MEASURE clip_kernels:layer dim={dim} inner={inner} heads={heads} L={L} floor={floor:.6e} got={value:.6e} "
          f"factor=parity_budget.FACTOR={FACTOR}")
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err, bound = float((got - ref).abs().max()), 1e-2 * float(ref.abs().max()) + 1e-3
    assert err <= bound, f"max err {err:.4g} > {bound:.4g}"
    assert floor > 0 and value <= FACTOR * floor, f"relative L2 {value:.3e} > {FACTOR} x the floor {floor:.3e}"


@pytest.mark.parametrize("image,patch,dim", [(56, 14, 128),                  # the reduced tower: 16 patches, 17 tokens
                                             (224, 14, 1024)])               # ViT-L/14: 256 patches, 257 tokens
def test_embeddings_against_float64(dev, image, patch, dim):
    """ops.gemm(a, wp, residual=pos, out=x[1:]): K = 588 zero-padded to 640, the output the rows below row 0 of a taller buffer whose row 0
    holds fp16(class + pos[0]) -- written BEFORE the launch, so it must survive it bit for bit."""
    cfg = SimpleNamespace(hidden_size=dim, patch_size=patch, image_size=image, intermediate_size=2 * dim, num_attention_heads=dim // 64 or 1,
                          num_hidden_layers=0, layer_norm_eps=EPS)
    tower = CLIPVisionTransformer(cfg)
    n, k = tower.n_tokens, 3 * patch * patch
    g = torch.Generator().manual_seed(9200 + dim)
    wconv = (torch.randn(dim, 3, patch, patch, generator=g) * k ** -0.5).half()
    cls, pos = torch.randn(dim, generator=g).half(), torch.randn(n, dim, generator=g).half()
    px = torch.randn(1, 3, image, image, generator=g).half()
    with torch.no_grad():
        for p_ in tower.parameters():
            p_.zero_()                                                          # the LayerNorms are not run here
        tower.embeddings.patch_embedding.weight.copy_(wconv)
        tower.embeddings.class_embedding.copy_(cls)
        tower.embeddings.position_embedding.weight.copy_(pos)
    tower = tower.to(device=dev, dtype=torch.float16)
    a, wmat = clip_ref.patches(px, patch), wconv.reshape(dim, k)
    ref = R.reference(a, wmat, residual=pos[1:])
    floor = R.rel_l2(R.emulation(a, wmat, residual=pos[1:]), ref)
    assert floor < 2.4e-4, floor                                                # the one-rounding floor, as tests/test_gemm_floor_cpu.py bounds it
    pk = tower.packed()
    assert pk["kp"] == 640 and tuple(pk["wp"].shape) == (dim, 640) and not bool(pk["wp"][:, k:].any())
    probe = torch.empty((n, dim), dtype=torch.float16, device=dev)
    plan = ops.gemm_plan(torch.empty((n - 1, 640), dtype=torch.float16, device=dev), pk["wp"], residual=pk["pos"], out=probe[1:])
    assert plan == GEMM_KERNEL_128, plan
    outs = []
    for _ in range(3):
        buf = torch.full((n, dim), float("nan"), dtype=torch.float16, device=dev)
        got = tower.embed_tokens(px.to(dev), out=buf)
        assert got.data_ptr() == buf.data_ptr()
        outs.append(buf)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), "two runs on the same inputs differ"
    out = outs[0].cpu()
    assert torch.equal(out[0].view(torch.int16), (cls.float() + pos[0].float()).half().view(torch.int16)), "row 0 is not fp16(class + pos[0])"
    R.pass_rule(f"embeddings image={image} patch={patch} dim={dim} [{plan}]", out[1:], ref, floor, prefix="clip_kernels")
