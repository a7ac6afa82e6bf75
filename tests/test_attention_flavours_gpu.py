"""GPU: every kernel flavour behind md_attention_fwd_f16, each at the smallest shapes that reach its code paths, in the operand forms the
pipeline uses.  md_attention_fwd_f16 chooses between four kernels (csrc/attention.hip launch_attn, attention_v2.h launch_attn2,
attention_v2s.h attn2s_eligible); md_attention_plan answers which one, and every case here
  (a) asserts the plan BEFORE launching, so a change of a dispatch threshold fails the case instead of silently moving it to another kernel;
  (b) runs the kernel three times and requires identical bits (attn2s has no barrier inside its walk over the q-blocks, the ring kernels
      share K / V^T tiles between waves: a race shows as run-to-run drift);
  (c) compares with float64 softmax(scale Q K^T) V on the same fp16-rounded inputs (kv_index gather applied in the reference):
      elementwise |err| <= 1e-2 max|ref| + 1e-3 (the project's kernel tolerance) and relative L2 <= 2 x the case's floor, the relative L2
      of a plain PyTorch emulation of the documented arithmetic (tests/attention_ref.py: computed from the reference alone, not recorded).
Dense outputs start as NaN, so a row no workgroup wrote fails (c).  K and V use other seeds than Q.
profiles/attention_flavour_tests.log: floor and measured value of every case on MI355X (kernels at 1.00-1.07 x their floor), and the
mutations of attn2s (a q-block skipped, the key mask off by one, P cut to 8 bits) that these cases catch and the older tests do not.
profiles/clip_kernel_tests.log: the same for the call of the CLIP vision tower (plan 400 at D = 64 with an unwritten V^T slack)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from attention_ref import FACTOR, emulation, reference, rel_l2, rnd  # noqa: E402

from mikudance_amd import _lib, ops  # noqa: E402

GENERIC, RING4, RING8, RESIDENT = 400, 414, 418, 420
PAD_MAGNITUDE = 60000.0            # finite, next to the largest fp16 (65504)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def problem(B, H, D, Lq, Lk, kv_index=None, peaky=False, fold=False):
    """Seeded inputs, float64 reference and floor of one logical problem; shared by every test that runs it (never modified)."""
    pr = Problem()
    C, nkv = H * D, (B if kv_index is None else max(kv_index) + 1)
    seed = 7000 + 10 * D
    pr.q, pr.k, pr.v = rnd(B, Lq, C, seed=seed), rnd(nkv, Lk, C, seed=seed + 1), rnd(nkv, Lk, C, seed=seed + 2)
    if peaky:           # one dominant key in tile 0, one in the last tile, for a query of the first and of the last wave: the lazy rescale fires
        for b in range(B):
            kb = b if kv_index is None else kv_index[b]
            pr.k[kb, 300 % Lk] = 4 * pr.q[b, 5]
            pr.k[kb, Lk - 1] = 5 * pr.q[b, Lq - 8]
    pr.B, pr.H, pr.D, pr.Lq, pr.Lk, pr.nkv, pr.kv_index = B, H, D, Lq, Lk, nkv, kv_index
    pr.ref = reference(pr.q, pr.k, pr.v, H, D, kv_index)
    pr.floor = rel_l2(emulation(pr.q, pr.k, pr.v, H, D, kv_index, fold=fold), pr.ref)
    return pr


def _checker(rows, cols):
    return 1.0 - 2.0 * ((torch.arange(rows)[:, None] + torch.arange(cols)[None, :]) % 2).float()


def launch(dev, pr, flavour, stride, pad=0.0, form="dense", vt_form="dense", runs=3, vt_slack=0.0):
    """Builds the operands of `pr` in the requested form, asserts the plan, launches `runs` times; returns the outputs (CPU).
    form: dense | slices (Q, K, O column slices of wider buffers: garbage around Q and K, 7.0 around O) | halves (Q | K the two column
    halves of one [B*L, 2C] buffer, O a slice).  vt_form: dense | misaligned (base 8 bytes off a 16-byte boundary) | odd_ld (ldvt % 8 = 4) |
    pitch8 (row pitch roundup8(nkv * stride) > nkv * stride, base 16-byte aligned: V^T as md_gemm_f16's transposed store leaves it for the
    CLIP vision tower; the columns behind the last batch, which that store does not write, hold `vt_slack`).
    pad: rows [Lk, stride) of every K batch and the same columns of V^T hold +/-pad in a checkerboard."""
    B, H, D, Lq, Lk, nkv = pr.B, pr.H, pr.D, pr.Lq, pr.Lk, pr.nkv
    C, n = H * D, nkv * stride
    kp, vp = torch.zeros(nkv, stride, C, dtype=torch.float16), torch.zeros(nkv, stride, C, dtype=torch.float16)
    kp[:, :Lk], vp[:, :Lk] = pr.k, pr.v
    if stride > Lk:
        kp[:, Lk:] = (pad * _checker(stride - Lk, C)).half()
        vp[:, Lk:] = (pad * _checker(stride - Lk, C)).half()
    q2, k2, vt = pr.q.reshape(B * Lq, C), kp.reshape(n, C), vp.reshape(n, C).t().contiguous()
    if form == "dense":
        qd, kd = q2.to(dev), k2.to(dev)
    elif form == "slices":
        qb, kb_ = rnd(B * Lq, C + 64, seed=1, scale=50.0), rnd(n, C + 64, seed=2, scale=50.0)
        qb[:, 32:32 + C], kb_[:, 16:16 + C] = q2, k2
        qd, kd = qb.to(dev)[:, 32:32 + C], kb_.to(dev)[:, 16:16 + C]
    else:
        assert form == "halves" and B * Lq == n
        qk = torch.cat([q2, k2], dim=1).to(dev)
        qd, kd = qk[:, :C], qk[:, C:]
    if vt_form == "dense":
        vtd = vt.to(dev)
    elif vt_form == "misaligned":
        wide = rnd(C, n + 8, seed=3, scale=50.0)
        wide[:, 4:4 + n] = vt
        vtd = wide.to(dev)[:, 4:4 + n]
        assert vtd.data_ptr() % 16 == 8 and vtd.stride(0) % 8 == 0
    elif vt_form == "pitch8":
        assert n % 8 != 0
        wide = torch.full((C, n + -n % 8), vt_slack, dtype=torch.float16)
        wide[:, :n] = vt
        vtd = wide.to(dev)[:, :n]
        assert vtd.data_ptr() % 16 == 0 and vtd.stride(0) % 8 == 0 and vtd.stride(0) == n + -n % 8
    else:
        assert vt_form == "odd_ld"
        wide = rnd(C, n + 4, seed=3, scale=50.0)
        wide[:, :n] = vt
        vtd = wide.to(dev)[:, :n]
        assert vtd.data_ptr() % 16 == 0 and vtd.stride(0) % 8 == 4
    idx = None if pr.kv_index is None else torch.tensor(pr.kv_index, dtype=torch.int32, device=dev)
    got = _lib.load().md_attention_plan(D, Lq, Lk, stride, vtd.stride(0), int(vtd.data_ptr() % 16 == 0))
    assert got == flavour, f"md_attention_plan says {got}, the case is meant for {flavour}: D={D} Lq={Lq} Lk={Lk} stride={stride}"
    outs = []
    for _ in range(runs):
        if form == "dense":
            obuf = torch.full((B * Lq, C), float("nan"), dtype=torch.float16, device=dev)
            out = obuf
        else:
            obuf = torch.full((B * Lq, C + 64), 7.0, dtype=torch.float16, device=dev)
            out = obuf[:, 32:32 + C]
        ops.attention(qd, kd, vtd, B, H, D, Lq, Lk, kv_stride=stride, kv_index=idx, out=out)
        outs.append(obuf.cpu())
    for o in outs[1:]:
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), "two runs on the same inputs differ"
    if form != "dense":
        for o in outs:
            assert bool((o[:, :32] == 7.0).all()) and bool((o[:, 32 + C:] == 7.0).all()), "columns outside the O slice were written"
        outs = [o[:, 32:32 + C].contiguous() for o in outs]
    return outs


def check(name, pr, out):
    got, ref = out.double(), pr.ref
    err, bound = float((got - ref).abs().max()), 1e-2 * float(ref.abs().max()) + 1e-3
    value = rel_l2(out, ref)
    print(f"\nPARITY_MEASURE attn_flavour:{name} floor={pr.floor:.6e} got={value:.6e}")
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output (a row that was never written stays NaN)"
    assert err <= bound, f"{name}: max err {err:.4g} > {bound:.4g}"
    assert value <= FACTOR * pr.floor, f"{name}: relative L2 {value:.3e} > {FACTOR} x the floor {pr.floor:.3e}"


def run_case(dev, name, flavour, B, H, D, Lq, Lk, stride=None, kv_index=None, peaky=False, **forms):
    fold = flavour != GENERIC and D % 16 == 8          # attention_v2.h: head dims 8 and 40 pre-scale Q (tests/attention_ref.py)
    pr = problem(B, H, D, Lq, Lk, kv_index, peaky, fold)
    out = launch(dev, pr, flavour, Lk if stride is None else stride, **forms)[0]
    check(name, pr, out)
    return pr, out


# --------------------------------------------------------------------------------------------- attn2s: K / V^T resident in LDS (420)
# 256 queries per q-block (8 waves x 32), qsplit = min(ceil(512 / npair), nqb / 4) workgroups per (batch, head) pair, workgroup `slice`
# walks q-blocks slice, slice + qsplit, ...
@pytest.mark.parametrize("Lq", [2048,       # nqb = 8, qsplit = 2: even slices
                                2085,       # nqb = 9: slices of 5 and 4 blocks; the last block has one partial wave (5 rows), six waves past Lq
                                4100])      # nqb = 17, qsplit = 4: slices of 5 / 4 / 4 / 4 blocks, 4 rows in the last one
def test_resident_cross_attention_q_slicing(dev, Lq):
    """The production form of the 96 x 96 level: 257 CLIP tokens padded to a stride of 264, query batches mapped through kv_index."""
    run_case(dev, f"resident Lq={Lq}", RESIDENT, 2, 8, 40, Lq, 257, stride=264, kv_index=(1, 0))


@pytest.mark.parametrize("Lk", [8,          # one tile, 56 of its 64 keys masked, V^T chunks clamped to column 0
                                64,         # exactly one full tile: no mask branch
                                72,         # a full tile + 8 keys
                                320])       # five tiles: the residency limit (69136 of 73728 bytes of LDS)
def test_resident_key_tile_edges(dev, Lk):
    run_case(dev, f"resident Lk={Lk}", RESIDENT, 2, 8, 40, 2048, Lk)


def test_resident_pair_decode_with_fifteen_pairs(dev):
    """(pair / H, pair % H) with H = 5, B = 3: npair = 15 is neither a power of two nor a multiple of 8."""
    run_case(dev, "resident B=3 H=5", RESIDENT, 3, 5, 40, 2048, 257, stride=264, kv_index=(1, 0, 1))


def test_resident_peaky_rows_fire_the_lazy_rescale(dev):
    """A dominant key in tile 0 and one in the last tile (for rows of the first and the last wave): the reference set from tile 0 has to
    move after it (P >= 2 in the OR test), with four tiles of O^T already accumulated."""
    run_case(dev, "resident peaky", RESIDENT, 2, 8, 40, 2048, 257, stride=264, kv_index=(1, 0), peaky=True)


# --------------------------------------------------------------------------------------------- attn2 ring, 8 waves (418)
@pytest.mark.parametrize("B,H,D,Lq,Lk", [(2, 8, 8, 1029, 1000),      # ragged last q-block (5 of 256 rows) and last key tile (40 of 64), FOLD at d = 8
                                         (2, 8, 16, 1024, 72),       # exactly four q-blocks, a full key tile + 8 keys
                                         (2, 8, 32, 1300, 136),      # 20 rows in the last q-block; D % 32 == 0: no ones row, denominator from l_run
                                         (2, 8, 40, 2048, 328),      # just past residency: what a threshold change would swap for attn2s
                                         (3, 5, 32, 1300, 136)])     # 15 pairs: the (pair, q-block) decode without the XCD mapping
def test_ring_eight_waves(dev, B, H, D, Lq, Lk):
    run_case(dev, f"ring8 B={B} H={H} D={D} Lq={Lq} Lk={Lk}", RING8, B, H, D, Lq, Lk)


# --------------------------------------------------------------------------------------------- attn2 ring, 4 waves (414)
@pytest.mark.parametrize("B,D,Lq,kv_index", [(4, 80, 1029, (1, 0, 0, 1)),      # Lq >= 1024 stays on 4 waves at d = 80; two context batches
                                             (2, 160, 576, (1, 0)),            # the 24 x 24 level
                                             (2, 64, 130, (1, 0))])            # D % 32 == 0: denominator from l_run, not the ones row
def test_ring_four_waves_cross_attention(dev, B, D, Lq, kv_index):
    run_case(dev, f"ring4 cross D={D} Lq={Lq}", RING4, B, 8, D, Lq, 257, stride=264, kv_index=kv_index)


def test_ring_four_waves_self_attention_past_1024(dev):
    run_case(dev, "ring4 self D=80 Lq=1100", RING4, 2, 8, 80, 1100, 1096)


# --------------------------------------------------------------------------------------------- generic attn_kernel (400)
@pytest.mark.parametrize("D", [8, 16, 32, 40, 64, 80, 160])
def test_generic_kernel_every_head_dim(dev, D):
    """Lk = 77 = kv_stride is no multiple of 8; Lq = 130 is ragged against the kernel's 128-row block."""
    run_case(dev, f"generic D={D}", GENERIC, 2, 8, D, 130, 77)


@pytest.mark.parametrize("vt_form", ["misaligned", "odd_ld"])
def test_generic_kernel_is_taken_for_an_unaligned_vt_alone(dev, vt_form):
    """Everything else qualifies for the DMA kernels (stride 264, Lk = 257): only the V^T base (a [:, 4:] view of a wider buffer) or only
    ldvt % 8 sends the call to the generic kernel, whose element-wise V^T loads must then cope with it."""
    run_case(dev, f"generic vt {vt_form}", GENERIC, 2, 8, 40, 130, 257, stride=264, kv_index=(1, 0), vt_form=vt_form)


@pytest.mark.parametrize("H,D,L", [(16, 64, 257),       # ViT-L/14: 16 heads of 64, 257 tokens, ldvt = 264
                                   (4, 32, 17)])        # the reduced tower of tests/test_clip_gpu.py: ldvt = 24
def test_clip_tower_call_never_reads_the_vt_slack(dev, H, D, L):
    """mikudance_amd/clip_vision.py _ClipLayer.forward: ops.attention(qk[:, :C], qk[:, C:], vt, 1, H, C // H, L, L) -- one batch, Q | K the
    halves of one GEMM output, kv_stride = Lk = L, and V^T from a transposed store with ldc_t = pad_to(L, 8) into a torch.empty buffer: its
    columns [L, ldvt) are never written.  roundup8(L) > kv_stride makes this plan 400, and include/mdance_hip.h promises that the generic
    kernel reads no V^T column >= Lk.  So NaN there must give the bits of zeros there (and both must pass the float64 rule): a whole
    16-byte chunk loaded across Lk turns the NaN run non-finite (0 x NaN in the matrix core), whatever the key mask does."""
    name = f"clip tower H={H} D={D} L={L}"
    pr, zero = run_case(dev, f"{name} zero slack", GENERIC, 1, H, D, L, L, form="halves", vt_form="pitch8")
    loud = launch(dev, pr, GENERIC, L, form="halves", vt_form="pitch8", vt_slack=float("nan"))[0]
    check(f"{name} NaN slack", pr, loud)
    assert torch.equal(loud.view(torch.int16), zero.view(torch.int16)), "the contents of V^T columns [Lk, ldvt) moved the output"


# --------------------------------------------------------------------------------------------- operand forms of the pipeline
@pytest.mark.parametrize("flavour,B,H,D,Lq,Lk,stride,kv_index,form", [
    (RESIDENT, 3, 5, 40, 2048, 257, 264, (1, 0, 1), "slices"),
    (RING8, 2, 8, 40, 1096, 1096, 1096, None, "halves"),           # blocks.TransformerBlock: q, k = qk[:, :C], qk[:, C:]  (ldq = ldk = 2C)
    (RING4, 2, 8, 80, 328, 328, 328, None, "halves"),
    (RING4, 2, 8, 160, 576, 257, 264, (1, 0), "slices")])
def test_operand_forms(dev, flavour, B, H, D, Lq, Lk, stride, kv_index, form):
    """Q and K as column slices (ld > H*D, K's base offset), O a column slice [:, 32:32 + C] of a buffer pre-filled with 7.0 (ldo > H*D):
    the columns outside the slice must still be exactly 7.0."""
    run_case(dev, f"{form} flavour={flavour} D={D}", flavour, B, H, D, Lq, Lk, stride=stride, kv_index=kv_index, form=form)


# --------------------------------------------------------------------------------------------- the pad of K / V^T
@pytest.mark.parametrize("flavour,B,D,Lq,kv_index", [(RESIDENT, 2, 40, 2048, (1, 0)), (RING8, 2, 40, 1029, (1, 0)), (RING4, 4, 80, 1029, (1, 0, 0, 1))])
def test_pad_contents_do_not_reach_the_result(dev, flavour, B, D, Lq, kv_index):
    """include/mdance_hip.h: the pad rows of K and pad columns of V^T ([257, 264) of every batch) may hold any finite values.  The DMA
    kernels fetch the V^T pad columns and rely on P == +0 for keys >= Lk (masked score -1e30 -> exp2 -> +0, 0 x finite = 0): +/-60000 in
    the pad must give the bits of the zero pad.  A masking slip or a chunk fetched from beyond Lk shows here and nowhere else."""
    pr, zero = run_case(dev, f"pad flavour={flavour}", flavour, B, 8, D, Lq, 257, stride=264, kv_index=kv_index)
    loud = launch(dev, pr, flavour, 264, pad=PAD_MAGNITUDE, runs=1)[0]
    assert bool(torch.isfinite(loud.float()).all())
    diff = (loud.float() - zero.float()).abs()
    assert torch.equal(loud.view(torch.int16), zero.view(torch.int16)), f"pad contents moved the output: max |diff| {float(diff.max()):.4g} in {int((diff > 0).sum())} elements"
