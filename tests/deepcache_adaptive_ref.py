"""TEST INFRASTRUCTURE for adaptive DeepCache (deep_cache_threshold=): the CPU twin of ops.rel_l1 for the emulated operator layer
(tests/fake_ops.py, which this file leaves as it is: install() below adds the twin after fake_ops.install), the float64 statement of
md_rel_l1_f16 and the depth of the kernel's summation order as mikudance_amd/csrc/rel_l1.hip states it."""
import torch

import fake_ops

RL_THREADS, RL_MAX_BLOCKS = 256, 2048                                      # rel_l1.hip: threads per workgroup, the cap on the grid
ROUND = RL_THREADS * RL_MAX_BLOCKS                                         # units of one full grid round


def rel_l1(a, b, out=None):
    """(sum |a - b|, sum |b|) as 2 fp32: float32 sums of the fp16 values (the order of the sums is torch's, not the kernel's)."""
    assert a.dtype == b.dtype == torch.float16 and a.shape == b.shape and a.stride(-1) == b.stride(-1) == 1, (a.shape, b.shape)
    fake_ops.CALLS.append(("rel_l1", (tuple(a.shape), tuple(a.stride()), tuple(b.stride()))))
    r = torch.stack([(a.float() - b.float()).abs().sum(), b.float().abs().sum()])
    if out is None:
        return r
    out.copy_(r)
    return out


def install(monkeypatch, fn=rel_l1):
    """After fake_ops.install(monkeypatch): the twin (or `fn`, a scripted stand-in) over mikudance_amd.ops.rel_l1."""
    from mikudance_amd import ops
    monkeypatch.setattr(ops, "rel_l1", fn)


def rel_l1_f64(a, b):
    """(sum |a - b|, sum |b|) in float64 over the same fp16 values: every term exact, the sums to ~1e-16."""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().sum()), float(b.abs().sum())


def vector_path(a, b):
    """Whether md_rel_l1_f16 takes 16-byte loads for these two (..., C) views: C and both row pitches multiples of 8, both bases 16-byte aligned."""
    return all(t.shape[-1] % 8 == 0 and t.stride(-2) % 8 == 0 and t.data_ptr() % 16 == 0 for t in (a, b))


def rel_l1_depth(rows, C, vector):
    """The largest number of fp32 additions a term passes through (rel_l1.hip, THE SUMMATION ORDER)."""
    units = rows * (C // 8 if vector else C)
    P = min(-(-units // RL_THREADS), RL_MAX_BLOCKS)
    iters = -(-units // (RL_THREADS * P))
    return (7 if vector else 0) + iters + -(-P // RL_THREADS) + 18
