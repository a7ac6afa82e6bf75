"""TEST INFRASTRUCTURE of colour matching (color_match=, md_color_moments / md_color_apply): the references the kernels are held to, and the
emulations of the two operators for the CPU tests of the host side.

    display32(x)               s = clamp(0.5 v + 0.5, 0, 1) in numpy float32, product and sum rounded separately, NaN kept -- the kernels' s
    sums_f64(x)                the nine sums per frame in float64, from the SAME source values: s and every product formed in float64 -> (B, 9)
    moments_depth(H, W)        the kernel's depth d restated: the largest number of fp32 additions a term passes through
    apply_ref(x, coef, bytes)  md_color_apply in numpy float32, the same operations in the same order -> (B, H, W, 3) uint8 or (B, 3, H, W) fp32
    color_moments / color_apply  the operators' emulations (float64 sums of the float32 s; apply_ref), logged in fake_ops.CALLS
"""
import numpy as np
import torch

F32 = np.float32
ORDER = ((0,), (1,), (2,), (0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def _np(x):
    """(B, 3, H, W) torch tensor, any strides / device -> numpy of its own dtype widened exactly to float32."""
    assert x.dim() == 4 and x.shape[1] == 3 and x.dtype in (torch.float16, torch.float32)
    return x.detach().cpu().float().contiguous().numpy()


def _clamp(s):
    return np.where(s < 0, s.dtype.type(0), np.where(s > 1, s.dtype.type(1), s))        # a NaN fails both comparisons and stays


def display32(x):
    v = _np(x)
    with np.errstate(all="ignore"):
        return _clamp(F32(0.5) * v + F32(0.5))


def sums_f64(x):
    v = _np(x).astype(np.float64)
    with np.errstate(all="ignore"):
        s = _clamp(0.5 * v + 0.5)
        return np.stack([np.prod([s[:, c] for c in idx], axis=0).reshape(s.shape[0], -1).sum(1) for idx in ORDER], axis=1)


def moments_depth(H, W):
    """csrc/color_match.hip, THE SUMMATION ORDER: 7 (the 8 pixels of a unit) + iters (a thread's units) + 6 (butterfly) + 3 (4 waves)."""
    U = H * ((W + 7) // 8)
    P = (U + 1023) // 1024
    iters = (U + 256 * P - 1) // (256 * P)
    assert 1 <= iters <= 4
    return iters + 16


def apply_ref(x, coef, as_bytes):
    s = display32(x)                                                             # (B, 3, H, W) float32
    m = np.asarray(coef.detach().cpu().numpy() if isinstance(coef, torch.Tensor) else coef)
    assert m.dtype == F32 and m.shape == (s.shape[0], 12)
    k = lambda j: m[:, j][:, None, None]
    with np.errstate(all="ignore"):
        y = np.stack([((k(9 + c) + k(3 * c) * s[:, 0]) + k(3 * c + 1) * s[:, 1]) + k(3 * c + 2) * s[:, 2] for c in range(3)], axis=1)
        assert y.dtype == F32
        y = _clamp(y)
        if not as_bytes:
            return y
        q = np.where(np.isnan(y), F32(0), y) * F32(255)
        return np.ascontiguousarray(q.astype(np.uint8).transpose(0, 2, 3, 1))


def color_moments(src, out=None):
    """The emulation of mikudance_amd.ops.color_moments: the float64 sums of the float32 s (what the device's sums round)."""
    import fake_ops
    B, _, H, W = src.shape
    s = display32(src).astype(np.float64)
    sums = np.stack([np.prod([s[:, c] for c in idx], axis=0).reshape(B, -1).sum(1) for idx in ORDER], axis=1)
    fake_ops.CALLS.append(("color_moments", dict(B=B, H=H, W=W, src=str(src.dtype).split(".")[-1], strides=tuple(src.stride()))))
    res = torch.from_numpy(sums)
    if out is not None:
        out.copy_(res)
        return out
    return res


def color_apply(src, coef, out=None, *, dtype=torch.uint8):
    """The emulation of mikudance_amd.ops.color_apply: apply_ref, into `out`."""
    import fake_ops
    B, _, H, W = src.shape
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (B, 12) and dtype in (torch.uint8, torch.float32)
    res = torch.from_numpy(apply_ref(src, coef, dtype == torch.uint8))
    if out is None:
        out = torch.empty(tuple(res.shape), dtype=dtype)
    assert out.dtype == dtype and tuple(out.shape) == tuple(res.shape)
    fake_ops.CALLS.append(("color_apply", dict(B=B, H=H, W=W, src=str(src.dtype).split(".")[-1], dst=str(dtype).split(".")[-1], strides=tuple(src.stride()))))
    out.copy_(res)
    return out


def install(monkeypatch):
    """frames_ref.install (fake_ops + tile_blend + frames_u8) and the two operators on top of it."""
    import frames_ref
    from mikudance_amd import ops
    frames_ref.install(monkeypatch)
    monkeypatch.setattr(ops, "color_moments", color_moments, raising=False)
    monkeypatch.setattr(ops, "color_apply", color_apply, raising=False)
