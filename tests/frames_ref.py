"""TEST INFRASTRUCTURE of uint8 frame output (output_type="uint8" / "pil", md_frames_u8): the reference the kernel must equal bit for bit, and the
emulation of ops.frames_u8 for the CPU tests of the host side.

    u8_ref(x, f32_math)        torch on the CPU, LITERALLY today's expression ((x / 2 + 0.5).clamp(0, 1).float() * 255).numpy().astype(np.uint8)
                               in fp16 (f32_math False: x must be fp16) or fp32 (True: x converted first, exactly), NaN positions set to 0 --
                               same shape as x
    one_expression(x)          trunc(clamp(127.5 x + 127.5, 0, 255)) in fp32: what the chain is NOT (it differs from the fp16 chain at 544 fp16
                               inputs and agrees with the fp32 chain on all of them); the tests use it to guard u8_ref itself
    all_fp16()                 the 65 536 fp16 bit patterns in order
    frames_u8(...)             the operator's emulation on u8_ref, logged in fake_ops.CALLS
"""
import numpy as np
import torch

F16 = torch.float16


def u8_ref(x, f32_math):
    x = x.detach().cpu()
    assert x.dtype in (torch.float16, torch.float32) and (f32_math or x.dtype == F16)
    v = x.float() if f32_math else x
    s = (v / 2 + 0.5).clamp(0, 1).float()
    nan = torch.isnan(s)
    out = (torch.where(nan, torch.zeros_like(s), s) * 255).numpy().astype(np.uint8)
    return torch.from_numpy(out)


def one_expression(x):
    v = x.detach().cpu().float()
    q = (127.5 * v + 127.5).clamp(0, 255)
    return torch.from_numpy(torch.where(torch.isnan(q), torch.zeros_like(q), q).numpy().astype(np.uint8))


def all_fp16():
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(F16)


def frames_u8(src, out=None, *, f32_math=None):
    """The emulation of mikudance_amd.ops.frames_u8: same argument meaning, u8_ref's bytes."""
    import fake_ops
    assert src.dim() == 4 and src.dtype in (torch.float16, torch.float32) and 1 <= src.shape[1] <= 4
    B, C, H, W = src.shape
    if f32_math is None:
        f32_math = src.dtype == torch.float32
    assert isinstance(f32_math, bool) and (f32_math or src.dtype == F16)
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.uint8)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, H, W, C) and out.stride(3) == 1 and out.stride(2) == C
    fake_ops.CALLS.append(("frames_u8", dict(B=B, C=C, H=H, W=W, src=str(src.dtype).split(".")[-1], f32_math=f32_math, strides=tuple(src.stride()))))
    out.copy_(u8_ref(src, f32_math).permute(0, 2, 3, 1))
    return out


def install(monkeypatch):
    """vae_tiling_ref.install (fake_ops + tile_blend) and this operator on top of it."""
    import vae_tiling_ref
    from mikudance_amd import ops
    vae_tiling_ref.install(monkeypatch)
    monkeypatch.setattr(ops, "frames_u8", frames_u8, raising=False)
