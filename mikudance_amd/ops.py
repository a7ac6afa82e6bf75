"""Thin tensor-level wrappers over the C ABI (include/mdance_hip.h).  PyTorch supplies device memory and the
stream; all arithmetic happens in the HIP kernels.  Every function requires CUDA(ROCm) fp16 tensors and raises
otherwise -- there is no eager/CPU fallback."""
import ctypes

import torch

from . import _lib

ACT_NONE, ACT_SILU, ACT_RELU, ACT_GEGLU, ACT_QUICKGELU = 0, 1, 2, 3, 4
F16 = torch.float16


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _chk(t, name, dtype=F16):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.MdanceHipError(f"{name} must live on the GPU: mikudance_amd has no CPU path")
    if t.dtype != dtype:
        raise _lib.MdanceHipError(f"{name} must be {dtype}, got {t.dtype}")


def require_gpu(t, who):
    """Entry check of the host-side loops: there is no CPU path behind them (the operators below check again, per tensor)."""
    if not t.is_cuda:
        raise RuntimeError(f"{who}: tensors must live on the MI355X; there is no CPU path")


def _rowmajor(t, name):
    _chk(t, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise _lib.MdanceHipError(f"{name} must be a 2-D row-major matrix (stride(1) == 1)")
    return t.stride(0)


def _pixel_pitch(x, name, align=8):
    """x: (B, H, W, C) or (B, HW, C) fp16 NHWC, contiguous or a channel slice of a wider contiguous NHWC tensor (a skip connection
    living inside the concat buffer of the up-block resnet that will consume it).  Returns the pixel pitch in elements.
    align: inputs are fetched in 16-byte pieces (pitch and base multiples of 8 elements); outputs (align = 1) may have any pitch."""
    _chk(x, name)
    C = x.shape[-1]
    ld = x.stride(-2)
    ok = x.stride(-1) == 1 and ld >= C and ld % align == 0 and x.data_ptr() % (2 * align) == 0
    n = 1
    for d in range(x.dim() - 2, -1, -1):                       # every outer dimension walks whole pixels: one uniform pitch
        ok = ok and (x.shape[d] == 1 or x.stride(d) == ld * n)
        n *= x.shape[d]
    if not ok:
        raise _lib.MdanceHipError(f"{name} must be NHWC with one uniform pixel pitch (contiguous, or a channel slice of a contiguous tensor): "
                                  f"shape {tuple(x.shape)} strides {tuple(x.stride())}")
    return ld


def _gemm_args(a, w, bias, residual, rowadd, rows_per_group, act, transpose_out, out, ldc_t):
    """The argument list of md_gemm_f16 up to the stream (md_gemm_plan_call takes the same one) and the output tensor."""
    lda = _rowmajor(a, "a")
    _chk(w, "w")
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous(), (w.shape, K)
    if out is None:
        if transpose_out:
            out = torch.empty((N, ldc_t or M), device=a.device, dtype=F16)
        else:
            out = torch.empty((M, N // 2 if act == ACT_GEGLU else N), device=a.device, dtype=F16)
    ldc = _rowmajor(out, "out")
    ldr = _rowmajor(residual, "residual") if residual is not None else 0
    ldra = _rowmajor(rowadd, "rowadd") if rowadd is not None else 0
    _chk(bias, "bias")
    return (a.data_ptr(), lda, w.data_ptr(), out.data_ptr(), ldc, M, N, K, _p(bias), _p(residual), ldr, _p(rowadd), ldra, rows_per_group,
            act, int(transpose_out)), out


def gemm(a, w, bias=None, residual=None, rowadd=None, rows_per_group=0, act=ACT_NONE, transpose_out=False, out=None,
         ldc_t=None):
    """out[M, N] = epi(a[M, K] @ w[N, K]^T).  transpose_out: out is [N, ldc_t] (V^T for attention)."""
    args, out = _gemm_args(a, w, bias, residual, rowadd, rows_per_group, act, transpose_out, out, ldc_t)
    M, N, K = args[5:8]
    _lib.call("md_gemm_f16", *args, _st(),
              meta=(f"gemm M={M} N={N} K={K}" + (" geglu" if act == ACT_GEGLU else "") + (" T" if transpose_out else ""),
                    2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)))
    return out


def gemm_plan(a, w, bias=None, residual=None, rowadd=None, rows_per_group=0, act=ACT_NONE, transpose_out=False, out=None,
              ldc_t=None, blocks=False):
    """The plan code (include/mdance_hip.h: md_gemm_plan) of the kernel ops.gemm would run for these very tensors and keywords, under the
    process's MD_GEMM_SP / MD_GEMM_SP_NT and CU limit; nothing is launched.  A negative code is the error the call would raise with.
    blocks=True: (code, row blocks, code of the last block)."""
    args, _ = _gemm_args(a, w, bias, residual, rowadd, rows_per_group, act, transpose_out, out, ldc_t)
    nb, tail = ctypes.c_int(1), ctypes.c_int(0)
    code = _lib.load().md_gemm_plan_call(*args, ctypes.byref(nb), ctypes.byref(tail))
    return (code, nb.value, tail.value) if blocks else code


def _conv_args(x, w, cout, bias, residual, rowadd, rows_per_group, act, stride, upsample, out, pad_lo, kw):
    """The argument list of md_conv_nhwc_f16 up to the stream (md_conv_plan_call takes the same one), the output tensor and (Ho, Wo)."""
    _chk(w, "w")
    assert x.dim() == 4
    ldx = _pixel_pitch(x, "x")
    B, H, W, Cin = x.shape
    assert w.shape == (cout, 3 * kw * Cin) and w.is_contiguous(), (w.shape, cout, Cin)
    hup, wup = (H * 2, W * 2) if upsample else (H, W)
    Ho, Wo = (hup + pad_lo - 2) // stride + 1, ((wup + pad_lo - 2) // stride + 1 if kw == 3 else W)
    if out is None:
        out = torch.empty((B, Ho, Wo, cout), device=x.device, dtype=F16)
    assert tuple(out.shape) == (B, Ho, Wo, cout), (tuple(out.shape), (B, Ho, Wo, cout))
    ldy = _pixel_pitch(out, "out", align=1)
    r2 = residual.flatten(0, -2) if residual is not None else None
    ldr = _rowmajor(r2, "residual") if r2 is not None else 0
    ldra = _rowmajor(rowadd, "rowadd") if rowadd is not None else 0
    _chk(bias, "bias")
    return (x.data_ptr(), ldx, w.data_ptr(), out.data_ptr(), ldy, B, H, W, Cin, cout, kw, stride, int(upsample), int(pad_lo), _p(bias),
            _p(r2), ldr, _p(rowadd), ldra, rows_per_group, act), out, (Ho, Wo)


def conv3x3(x, w, cout, bias=None, residual=None, rowadd=None, rows_per_group=0, act=ACT_NONE, stride=1, upsample=False,
            out=None, pad_lo=1, kw=3):
    """x: (B, H, W, Cin) NHWC (contiguous or a channel slice: see _pixel_pitch); w: [Cout, 3*kw*Cin] packed (ky, kx, cin);
    returns (B, Ho, Wo, Cout).
    pad_lo=0 (stride 2 only): zero padding (0,1,0,1) instead of 1 all round (the AutoencoderKL downsampler).
    kw=1: a 3 x 1 filter (taps along H only; Conv3d (3,1,1) of the temporal VAE decoder with H = frames, W = pixels).
    `out` may be a channel slice of a wider NHWC tensor (row pitch = its last-dim stride)."""
    args, out, (Ho, Wo) = _conv_args(x, w, cout, bias, residual, rowadd, rows_per_group, act, stride, upsample, out, pad_lo, kw)
    B, H, W, Cin = x.shape
    _lib.call("md_conv_nhwc_f16", *args, _st(),
              meta=(f"conv3x{kw} B={B} {H}x{W} Cin={Cin} Cout={cout} s={stride} up={int(upsample)}",
                    2.0 * B * Ho * Wo * cout * 3 * kw * Cin, 2.0 * (B * H * W * Cin + cout * 3 * kw * Cin + B * Ho * Wo * cout)))
    return out


def conv_plan(x, w, cout, bias=None, residual=None, rowadd=None, rows_per_group=0, act=ACT_NONE, stride=1, upsample=False,
              out=None, pad_lo=1, kw=3):
    """The plan code of the kernel ops.conv3x3 would run for these very tensors and keywords (see gemm_plan); nothing is launched."""
    args, _, _ = _conv_args(x, w, cout, bias, residual, rowadd, rows_per_group, act, stride, upsample, out, pad_lo, kw)
    return _lib.load().md_conv_plan_call(*args)


def _dense16(t):
    """The fused streaming kernels fetch whole 16-byte pieces of every row: base 16-byte aligned, row pitch a multiple of 8 elements."""
    return t is None or (t.data_ptr() % 16 == 0 and t.stride(-2) % 8 == 0 and t.stride(-1) == 1)


def gemm_ln_plan(M, N, K, act=ACT_NONE, rowadd=False, a=None):
    """True when md_gemm_ln_f16 has a kernel for the problem (else: layernorm + gemm on the unfolded weights).  The C-side query answers
    for dense, 16-byte aligned operands; `a` (the token matrix about to be passed) adds the pointer / pitch check, so that a channel- or
    row-sliced operand with an odd offset takes the literal pair instead of failing with MD_ERR_ARG."""
    return _dense16(a) and bool(_lib.load().md_gemm_ln_plan(M, N, K, act, 2 if rowadd else 0))


def gemm_ln(a, wf, sc, eps=1e-5, rowadd=None, rows_per_group=0, act=ACT_NONE, out=None):
    """out[M, N] = epi(LayerNorm(a) @ w^T + bias) from the RAW rows of a, with (wf, sc) = packing.ln_fold(w, bias, gamma, beta)."""
    lda = _rowmajor(a, "a")
    _chk(wf, "wf"); _chk(sc, "sc", torch.float32); _chk(rowadd, "rowadd")
    M, K = a.shape
    N = wf.shape[0]
    assert wf.shape[1] == K and wf.is_contiguous() and sc.shape == (2, N) and sc.is_contiguous(), (wf.shape, sc.shape, K)
    if out is None:
        out = torch.empty((M, N // 2 if act == ACT_GEGLU else N), device=a.device, dtype=F16)
    ldc = _rowmajor(out, "out")
    ldra = _rowmajor(rowadd, "rowadd") if rowadd is not None else 0
    if rowadd is not None and (rows_per_group <= 0 or rowadd.shape[0] * rows_per_group < M or rowadd.shape[1] < N):
        raise _lib.MdanceHipError(f"gemm_ln: row term {tuple(rowadd.shape)} does not cover M={M} rows in groups of {rows_per_group} x N={N}")
    _lib.call("md_gemm_ln_f16", a.data_ptr(), lda, wf.data_ptr(), sc.data_ptr(), out.data_ptr(), ldc, M, N, K, float(eps), _p(rowadd), ldra,
              rows_per_group, act, _st(),
              meta=(f"gemm M={M} N={N} K={K}" + (" geglu" if act == ACT_GEGLU else "") + " ln", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)))
    return out


_workspaces = {}


def _workspace(who, device, need, dtype=torch.float32, floor=0):
    """The workspace of entry point `who` on this (device, current stream): one cache per entry point, so that no two ever share a buffer;
    kept until it is too small for `need` bytes, then replaced by one of max(need, floor) bytes rounded up to whole elements of `dtype`."""
    cache = _workspaces.setdefault(who, {})
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() * dtype.itemsize < need:
        ws = cache[key] = torch.empty((max(need, floor) + dtype.itemsize - 1) // dtype.itemsize, device=device, dtype=dtype)
    return ws


def _gn_workspace(x, B, HW, C, groups):
    return _workspace("groupnorm", x.device, _lib.load().md_groupnorm_workspace_bytes(B, HW, C, groups), floor=1 << 20)


def gemm_affine_plan(M, N, K, rows_per_image, x=None):
    """As gemm_ln_plan: `x` (the NHWC tensor or channel slice about to be passed) adds the alignment check the C-side query cannot make."""
    return _dense16(x) and bool(_lib.load().md_gemm_affine_plan(M, N, K, rows_per_image))


def groupnorm_table(x, gamma, beta, groups, eps):
    """Statistics sweep of GroupNorm only: fp32 (B, 2, C) = [rstd * gamma, beta - mean * rstd * gamma] for gemm_affine."""
    _chk(gamma, "gamma"); _chk(beta, "beta")
    ldx = _pixel_pitch(x, "x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    ws = _gn_workspace(x, B, HW, C, groups)
    table = torch.empty((B, 2, C), device=x.device, dtype=torch.float32)
    _lib.call("md_groupnorm_table_f16", x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), B, HW, C, groups, float(eps), table.data_ptr(),
              ws.data_ptr(), ws.numel() * 4, _st(), meta=(f"groupnorm B={B} HW={HW} C={C} stats", 0.0, 2.0 * B * HW * C))
    return table


def gemm_affine(x, table, w, bias=None, out=None):
    """out[B*HW, N] = fp16(x * scale[image] + shift[image]) @ w^T + bias; x (B, HW, C) / (B, H, W, C) NHWC (a channel slice is fine)."""
    lda = _pixel_pitch(x, "x")
    _chk(w, "w"); _chk(bias, "bias"); _chk(table, "table", torch.float32)
    B, K = x.shape[0], x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    assert w.shape[1] == K and w.is_contiguous() and table.shape == (B, 2, K) and table.is_contiguous()
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=F16)
    ldc = _rowmajor(out, "out")
    _lib.call("md_gemm_affine_f16", x.data_ptr(), lda, table.data_ptr(), M // B, w.data_ptr(), out.data_ptr(), ldc, M, N, K, _p(bias), _st(),
              meta=(f"gemm M={M} N={N} K={K} gn", 2.0 * M * N * K, 2.0 * (M * K + N * K + M * N)))
    return out


def groupnorm(x, gamma, beta, groups, eps, silu=False, out=None):
    """x: (B, HW, C) or (B, H, W, C) NHWC, contiguous or a channel slice (see _pixel_pitch); the output is contiguous."""
    _chk(gamma, "gamma"); _chk(beta, "beta")
    ldx = _pixel_pitch(x, "x")
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    ws = _gn_workspace(x, B, HW, C, groups)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=F16)
    assert out.is_contiguous() and out.shape == x.shape
    _lib.call("md_groupnorm_ld_nhwc_f16", x.data_ptr(), ldx, out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), B, HW, C, groups,
              float(eps), int(silu), ws.data_ptr(), ws.numel() * 4, _st(),
              meta=(f"groupnorm B={B} HW={HW} C={C}", 0.0, 6.0 * B * HW * C))
    return out


def layernorm(x, gamma, beta, eps=1e-5, add=None, add_mode=0, add_row_begin=0, rows_per_frame=0, frames=0):
    """x: [M, C].  Returns y (add_mode 0) or (y, y2)."""
    _chk(x, "x"); _chk(gamma, "gamma"); _chk(beta, "beta"); _chk(add, "add")
    assert x.dim() == 2 and x.is_contiguous()
    M, C = x.shape
    y = torch.empty_like(x)
    y2 = torch.empty_like(x) if add_mode else None
    _lib.call("md_layernorm_f16", x.data_ptr(), y.data_ptr(), _p(y2), gamma.data_ptr(), beta.data_ptr(), _p(add), M, C,
              float(eps), add_mode, add_row_begin, rows_per_frame, frames, _st(),
              meta=(f"layernorm M={M} C={C} mode={add_mode}", 0.0, 2.0 * M * C * (2 + (2 if add_mode else 0))))
    return (y, y2) if add_mode else y


def instnorm_spade(x, gamma_beta, eps=1e-5):
    """x: (B, HW, C); gamma_beta: (B, HW, 2C)."""
    _chk(gamma_beta, "gamma_beta")
    ldx = _pixel_pitch(x, "x")
    assert gamma_beta.is_contiguous()
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    y = torch.empty(x.shape, device=x.device, dtype=F16)
    _lib.call("md_instnorm_spade_ld_f16", x.data_ptr(), ldx, gamma_beta.data_ptr(), y.data_ptr(), B, HW, C, float(eps), _st())
    return y


def attention(q, k, vt, B, H, D, Lq, Lk, kv_stride=None, kv_index=None, scale=None, out=None):
    """q [B*Lq, >=H*D], k [nkv*kv_stride, >=H*D], vt [H*D, >=nkv*kv_stride] (V transposed) -> out [B*Lq, H*D]."""
    ldq = _rowmajor(q, "q"); ldk = _rowmajor(k, "k"); ldvt = _rowmajor(vt, "vt")
    if kv_index is not None:
        _chk(kv_index, "kv_index", torch.int32)
    if out is None:
        out = torch.empty((B * Lq, H * D), device=q.device, dtype=F16)
    ldo = _rowmajor(out, "out")
    _lib.call("md_attention_fwd_f16", q.data_ptr(), ldq, k.data_ptr(), ldk, vt.data_ptr(), ldvt, out.data_ptr(), ldo,
              _p(kv_index), B, H, D, Lq, Lk, kv_stride if kv_stride is not None else Lk,
              float(scale if scale is not None else D ** -0.5), _st(),
              meta=(f"attention B={B} H={H} D={D} Lq={Lq} Lk={Lk}", 4.0 * B * H * Lq * Lk * D, 2.0 * B * H * D * (2 * Lq + 2 * Lk)))
    return out


def softmax_rows_(x, scale=1.0):
    """In-place softmax(scale * x) over the rows of a 2-D row-major fp16 matrix."""
    ld = _rowmajor(x, "x")
    rows, cols = x.shape
    _lib.call("md_softmax_rows_f16", x.data_ptr(), ld, rows, cols, float(scale), _st(),
              meta=(f"softmax_rows {rows}x{cols}", 0.0, 4.0 * rows * cols))
    return x


def temporal_attention(q, k, v, NB, F, HW, H, D, out=None, scale=None):
    """q/k/v: [(NB*F)*HW, >=H*D] token-major (frame-major rows).  Attention across the F frames of every pixel; scale defaults to D ** -0.5."""
    ldq = _rowmajor(q, "q"); ldk = _rowmajor(k, "k"); ldv = _rowmajor(v, "v")
    if out is None:
        out = torch.empty((NB * F * HW, H * D), device=q.device, dtype=F16)
    ldo = _rowmajor(out, "out")
    _lib.call("md_temporal_attention_fwd_f16", q.data_ptr(), ldq, k.data_ptr(), ldk, v.data_ptr(), ldv, out.data_ptr(), ldo,
              NB, F, HW, H, D, float(D ** -0.5 if scale is None else scale), _st(),
              meta=(f"temporal_attention NB={NB} F={F} HW={HW} D={D}", 4.0 * NB * HW * H * F * F * D, 8.0 * NB * F * HW * H * D))
    return out


def pack_nhwc(src, n, f, strides, c_begin, c_count, cpad, ho, wo, hin=None, win=None):
    """Strided gather into a fresh (n, ho, wo, cpad) fp16 NHWC tensor.  strides = (sB, sF, sC, sY, sX) in elements.
    (hin, win) != (ho, wo) applies PyTorch's nearest-neighbour resize rule."""
    if not src.is_cuda or src.dtype not in (torch.float16, torch.float32):
        raise _lib.MdanceHipError("pack_nhwc: source must be a CUDA fp16/fp32 tensor")
    dst = torch.empty((n, ho, wo, cpad), device=src.device, dtype=F16)
    sB, sF, sC, sY, sX = strides
    _lib.call("md_pack_nhwc_f16", src.data_ptr(), int(src.dtype == torch.float32), dst.data_ptr(), n, f, sB, sF, sC, sY, sX,
              c_begin, c_count, cpad, ho, wo, hin or ho, win or wo, _st())
    return dst


def unpack_nhwc(src, dst, n, f, strides, c, ho, wo):
    """Scatter NHWC fp16 `src` (n, ho, wo, ldc>=c) into the strided fp16/fp32 tensor `dst`."""
    _chk(src, "src")
    sB, sF, sC, sY, sX = strides
    _lib.call("md_unpack_nhwc_f16", src.data_ptr(), src.shape[-1], dst.data_ptr(), int(dst.dtype == torch.float32), n, f, sB,
              sF, sC, sY, sX, c, ho, wo, _st())
    return dst


def concat_channels(a, b):
    _chk(a, "a"); _chk(b, "b")
    assert a.is_contiguous() and b.is_contiguous() and a.shape[:-1] == b.shape[:-1]
    out = torch.empty(a.shape[:-1] + (a.shape[-1] + b.shape[-1],), device=a.device, dtype=F16)
    _lib.call("md_concat_channels_f16", a.data_ptr(), a.shape[-1], b.data_ptr(), b.shape[-1], out.data_ptr(),
              a.numel() // a.shape[-1], _st())
    return out


def window_accumulate(pred, noise_sum, counter, window, f, ftot, hw, halves=2):
    _chk(pred, "pred"); _chk(noise_sum, "noise_sum", torch.float32); _chk(counter, "counter", torch.float32)
    _chk(window, "window", torch.int32)
    _lib.call("md_window_accumulate", pred.data_ptr(), noise_sum.data_ptr(), counter.data_ptr(), window.data_ptr(), f, ftot,
              hw, halves, _st())


def window_accumulate_weighted(pred, noise_sum, counter, window, weights, f, ftot, hw, halves=2):
    """noise_sum[:, window[i]] += weights[i] * pred[:, i]; counter[window[i]] += weights[i] (md_window_accumulate_weighted).  `weights`:
    fp32 (f,) on the device, the normalised per-slot weights of windows.fuse_weights; the other arguments as window_accumulate."""
    _chk(pred, "pred"); _chk(noise_sum, "noise_sum", torch.float32); _chk(counter, "counter", torch.float32)
    _chk(window, "window", torch.int32); _chk(weights, "weights", torch.float32)
    assert halves in (1, 2) and pred.is_contiguous() and pred.numel() == halves * f * hw * 4
    assert noise_sum.is_contiguous() and noise_sum.numel() == halves * ftot * hw * 4 and counter.numel() >= ftot
    assert window.is_contiguous() and weights.is_contiguous() and window.numel() == f and weights.numel() == f
    _lib.call("md_window_accumulate_weighted", pred.data_ptr(), noise_sum.data_ptr(), counter.data_ptr(), window.data_ptr(),
              weights.data_ptr(), f, ftot, hw, halves, _st())


def cfg_guidance_rescale(noise_sum, counter, ftot, hw, guidance, phi, out=None):
    """Guidance rescale factor (md_cfg_guidance_rescale): fp32 (1,) device tensor 1 - phi + phi std(c) / std(v) of the guided output
    v = u + guidance (c - u) of a CFG noise_sum (2, ftot, hw, 4); 1 when std(v) == 0.  Stays on the device: pass it as `vscale=` to
    cfg_ddim_step / cfg_multistep_step.  The workspace is kept per (device, stream) and reused."""
    _chk(noise_sum, "noise_sum", torch.float32); _chk(counter, "counter", torch.float32)
    assert noise_sum.is_contiguous() and noise_sum.numel() == 2 * ftot * hw * 4 and counter.numel() >= ftot
    ws = _workspace("cfg_guidance_rescale", noise_sum.device, _lib.load().md_cfg_rescale_workspace_bytes(ftot, hw), torch.float64, 1 << 14)
    if out is None:
        out = torch.empty((1,), device=noise_sum.device, dtype=torch.float32)
    _chk(out, "out", torch.float32)
    _lib.call("md_cfg_guidance_rescale", noise_sum.data_ptr(), counter.data_ptr(), ftot, hw, 2, float(guidance), float(phi), ws.data_ptr(),
              ws.numel() * 8, out.data_ptr(), _st(), meta=(f"cfg_guidance_rescale F={ftot} HW={hw}", 0.0, 8.0 * ftot * hw * 4))
    return out


def add_noise(latents, x0, a, b):
    """In place: latents = fp16(a * x0 + b * latents) (md_add_noise_f16), both contiguous fp16 tensors of the same size; a = sqrt(abar_t),
    b = sqrt(1 - abar_t).  a == 0 leaves exactly b * latents, whatever x0 holds."""
    _chk(latents, "latents"); _chk(x0, "x0")
    assert latents.is_contiguous() and x0.is_contiguous() and latents.numel() == x0.numel() and latents.numel() > 0
    _lib.call("md_add_noise_f16", latents.data_ptr(), x0.data_ptr(), latents.numel(), float(a), float(b), _st())
    return latents


def _fp32_buffer(t, name, numel):
    """A contiguous fp32 device buffer of `numel` elements -> its pointer."""
    _chk(t, name, torch.float32)
    assert t.is_contiguous() and t.numel() == numel
    return t.data_ptr()


def _step_buffers(latents, noise_sum, counter, ftot, hw, halves):
    """The buffers every entry of the step tail takes -> their three pointers."""
    _chk(latents, "latents"); _chk(noise_sum, "noise_sum", torch.float32); _chk(counter, "counter", torch.float32)
    n = ftot * hw * 4
    assert halves in (1, 2) and latents.is_contiguous() and latents.numel() == n
    assert noise_sum.is_contiguous() and noise_sum.numel() == halves * n and counter.numel() >= ftot
    return latents.data_ptr(), noise_sum.data_ptr(), counter.data_ptr()


def _unipc_state_row(state, row, ftot, hw):
    """The checks the cfg_unipc_step* wrappers share -> (state pointer, the row as 12 C floats in host memory)."""
    assert len(row) == 12
    return _fp32_buffer(state, "state", 4 * ftot * hw * 4), (ctypes.c_float * 12)(*(float(v) for v in row))


def _cfg_step(sampler, latents, noise_sum, counter, ftot, hw, halves, guidance, coeffs, *, history=None, state=None, noise_coeff=0.0,
              variance_noise=None, vscale=None, apg=None, pag=None, meta=None):
    """The one call behind the cfg_*_step* wrappers:
        md_cfg_<sampler>_step<guide>(latents, noise_sum, counter, <the sampler's buffers>, <the guide's buffers>, ftot, hw, halves, guidance,
                                     <the guide's scalar>, <the sampler's coefficients>, stream)
    sampler  "ddim": no buffer of its own; coeffs (alpha_t, alpha_prev), noise_coeff = eta, which follows them.  The plain entry at
             eta == 0 (md_cfg_ddim_step) takes neither variance_noise nor eta; at eta != 0 it is md_cfg_ddim_step_eta.
             "multistep": history, variance_noise; the six coeffs, noise_coeff = c_z, the last of them.
             "unipc": state; coeffs is the row of 12, handed over as host floats.
    guide    at most one of vscale (_scaled: the fp32 device factor), apg = (momentum_buf, coef) (_apg) and
             pag = (perturbed_sum, pag_scale) (_pag)."""
    n = ftot * hw * 4
    bufs = _step_buffers(latents, noise_sum, counter, ftot, hw, halves)
    z = 0
    if noise_coeff:
        _chk(variance_noise, "variance_noise")
        assert variance_noise is not None and variance_noise.is_contiguous() and variance_noise.numel() == n
        z = variance_noise.data_ptr()
    if sampler == "unipc":
        sp, rp = _unipc_state_row(state, coeffs, ftot, hw)
        mid, tail = (sp,), (rp,)
    else:
        mid, tail = (_fp32_buffer(history, "history", n), z) if sampler == "multistep" else (z,), tuple(float(c) for c in coeffs)
    guide, ptrs, scalar = "", (), ()
    if vscale is not None:
        _chk(vscale, "vscale", torch.float32)
        guide, ptrs = "_scaled", (vscale.data_ptr(),)
    elif apg is not None:
        guide, ptrs = "_apg", (_fp32_buffer(apg[0], "momentum_buf", n), _fp32_buffer(apg[1], "coef", ftot * 2))
    elif pag is not None:
        guide, ptrs, scalar = "_pag", (_fp32_buffer(pag[0], "perturbed_sum", n),), (float(pag[1]),)
    if sampler == "ddim":
        if guide or noise_coeff:
            guide, tail = guide or "_eta", tail + (float(noise_coeff),)
        else:
            mid = ()
    _lib.call(f"md_cfg_{sampler}_step{guide}", *bufs, *mid, *ptrs, ftot, hw, halves, float(guidance), *scalar, *tail, _st(), meta=meta)


def cfg_ddim_step(latents, noise_sum, counter, ftot, hw, guidance, alpha_t, alpha_prev, halves=2, eta=0.0, variance_noise=None, vscale=None):
    """eta > 0: `variance_noise` is the caller's N(0, 1) draw, fp16, laid out like `latents` (ftot, hw, 4).
    vscale: the fp32 device factor of cfg_guidance_rescale (md_cfg_ddim_step_scaled, any eta); None: the unscaled entry points."""
    _cfg_step("ddim", latents, noise_sum, counter, ftot, hw, halves, guidance, (alpha_t, alpha_prev), noise_coeff=eta,
              variance_noise=variance_noise, vscale=vscale)


def cfg_multistep_step(latents, noise_sum, counter, history, ftot, hw, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z, halves=2,
                       variance_noise=None, vscale=None):
    """DPM-Solver++ multistep update (md_cfg_multistep_step): `history` is the fp32 (ftot, hw, 4) data-prediction buffer the caller keeps
    between steps; the coefficients are DPMSolverMultistepScheduler.multistep_coefficients(step_index).  c_z != 0: `variance_noise` is
    the caller's N(0, 1) draw, fp16, laid out like `latents`.  vscale: as in cfg_ddim_step (md_cfg_multistep_step_scaled)."""
    _cfg_step("multistep", latents, noise_sum, counter, ftot, hw, halves, guidance, (alpha_s, sigma_s, c_x, c_m0, c_m1, c_z), history=history,
              noise_coeff=c_z, variance_noise=variance_noise, vscale=vscale)


def cfg_apg_prepare(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, alpha_s, sigma_s, momentum, eta, norm_threshold):
    """Adaptive projected guidance, the statistics pass of one step (md_cfg_apg_prepare; arXiv 2410.02416 Algorithm 1 on the data prediction,
    PER FRAME): updates the fp32 (ftot, hw, 4) `momentum_buf` in place, m = sigma_s (u - c) + momentum m (momentum == 0 never reads it), and
    writes the fp32 (ftot, 2) `coef` = (S, (1 - eta) S proj) per frame.  Both stay on the device: hand them to cfg_ddim_step_apg /
    cfg_multistep_step_apg with the same alpha / sigma.  The workspace is kept per (device, stream) and reused."""
    n = ftot * hw * 4
    bufs = _step_buffers(latents, noise_sum, counter, ftot, hw, 2)
    mp, cp = _fp32_buffer(momentum_buf, "momentum_buf", n), _fp32_buffer(coef, "coef", ftot * 2)
    ws = _workspace("cfg_apg_prepare", noise_sum.device, _lib.load().md_cfg_apg_workspace_bytes(ftot, hw), torch.float64, 1 << 14)
    _lib.call("md_cfg_apg_prepare", *bufs, mp, ftot, hw, 2, float(alpha_s), float(sigma_s), float(momentum), float(eta), float(norm_threshold),
              ws.data_ptr(), ws.numel() * 8, cp, _st(), meta=(f"cfg_apg_prepare F={ftot} HW={hw}", 0.0, (2.0 + 8.0 + 8.0) * n))
    return coef


def cfg_ddim_step_apg(latents, noise_sum, counter, momentum_buf, coef, ftot, hw, guidance, alpha_t, alpha_prev, eta=0.0, variance_noise=None):
    """cfg_ddim_step under CFG with APG's guided output (md_cfg_ddim_step_apg): `momentum_buf` and `coef` as cfg_apg_prepare left them for this
    step at alpha_s = sqrt(alpha_t), sigma_s = sqrt(1 - alpha_t).  eta / variance_noise as in cfg_ddim_step."""
    _cfg_step("ddim", latents, noise_sum, counter, ftot, hw, 2, guidance, (alpha_t, alpha_prev), noise_coeff=eta, variance_noise=variance_noise,
              apg=(momentum_buf, coef))


def cfg_multistep_step_apg(latents, noise_sum, counter, history, momentum_buf, coef, ftot, hw, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                           variance_noise=None):
    """cfg_multistep_step under CFG with APG's guided output (md_cfg_multistep_step_apg): `momentum_buf` and `coef` as cfg_apg_prepare left them
    for this step at the same alpha_s, sigma_s; `history` receives alpha_s x - sigma_s v_g.  The rest as in cfg_multistep_step."""
    _cfg_step("multistep", latents, noise_sum, counter, ftot, hw, 2, guidance, (alpha_s, sigma_s, c_x, c_m0, c_m1, c_z), history=history,
              noise_coeff=c_z, variance_noise=variance_noise, apg=(momentum_buf, coef))


def cfg_ddim_step_pag(latents, noise_sum, counter, perturbed_sum, ftot, hw, guidance, pag_scale, alpha_t, alpha_prev, halves=2, eta=0.0,
                      variance_noise=None):
    """cfg_ddim_step with perturbed-attention guidance (md_cfg_ddim_step_pag; arXiv 2403.17377): v + pag_scale inv (sum_c - perturbed_sum) in place
    of the guided v, with or without CFG.  `perturbed_sum`: fp32 (ftot, hw, 4), the perturbed evaluation accumulated over the windows like one
    plane of `noise_sum` (halves planes).  eta / variance_noise as in cfg_ddim_step."""
    _cfg_step("ddim", latents, noise_sum, counter, ftot, hw, halves, guidance, (alpha_t, alpha_prev), noise_coeff=eta,
              variance_noise=variance_noise, pag=(perturbed_sum, pag_scale))


def cfg_multistep_step_pag(latents, noise_sum, counter, history, perturbed_sum, ftot, hw, guidance, pag_scale, alpha_s, sigma_s, c_x, c_m0, c_m1,
                           c_z, halves=2, variance_noise=None):
    """cfg_multistep_step with perturbed-attention guidance (md_cfg_multistep_step_pag): `perturbed_sum` and pag_scale as in cfg_ddim_step_pag;
    `history` receives alpha_s x - sigma_s v of the PAG-guided v.  The rest as in cfg_multistep_step."""
    _cfg_step("multistep", latents, noise_sum, counter, ftot, hw, halves, guidance, (alpha_s, sigma_s, c_x, c_m0, c_m1, c_z), history=history,
              noise_coeff=c_z, variance_noise=variance_noise, pag=(perturbed_sum, pag_scale))


def cfg_unipc_step(latents, noise_sum, counter, state, ftot, hw, guidance, row, halves=2, vscale=None):
    """UniPC correct-then-predict update (md_cfg_unipc_step): `state` is the fp32 (4, ftot, hw, 4) buffer (x_last and the data predictions of
    the last three steps) the caller keeps between steps, uninitialised before the first; `row` is
    UniPCMultistepScheduler.unipc_coefficients(step_index).  vscale: as in cfg_ddim_step (md_cfg_unipc_step_scaled)."""
    _cfg_step("unipc", latents, noise_sum, counter, ftot, hw, halves, guidance, row, state=state, vscale=vscale,
              meta=(f"cfg_unipc_step F={ftot} HW={hw}", 0.0, (4.0 + 4.0 * halves + 32.0) * ftot * hw * 4))


def cfg_unipc_step_apg(latents, noise_sum, counter, state, momentum_buf, coef, ftot, hw, guidance, row):
    """cfg_unipc_step under CFG with APG's guided output (md_cfg_unipc_step_apg): `momentum_buf` and `coef` as cfg_apg_prepare left them for
    this step at the row's alpha_s, sigma_s; the data prediction kept in `state` is alpha_s x - sigma_s v_g."""
    _cfg_step("unipc", latents, noise_sum, counter, ftot, hw, 2, guidance, row, state=state, apg=(momentum_buf, coef))


def cfg_unipc_step_pag(latents, noise_sum, counter, state, perturbed_sum, ftot, hw, guidance, pag_scale, row, halves=2):
    """cfg_unipc_step with perturbed-attention guidance (md_cfg_unipc_step_pag): `perturbed_sum` and pag_scale as in cfg_ddim_step_pag."""
    _cfg_step("unipc", latents, noise_sum, counter, ftot, hw, halves, guidance, row, state=state, pag=(perturbed_sum, pag_scale))


def cfg_uncond_cache(noise_sum, counter, delta, ftot, hw, mode, scale=1.0):
    """The unconditional plane of a step that evaluated the conditional half only (md_cfg_uncond_cache).  noise_sum: fp32 (2, ftot, hw, 4),
    planes [u, c]; counter: fp32 (ftot,); delta: fp32 (ftot, hw, 4).  mode 0 stores delta = c_sum / cnt - u_sum / cnt; mode 1 restores
    u_sum = c_sum - scale * delta * cnt in place.  With mode 1 and scale == 0 (no guidance at this step) delta is not read and may be None:
    u_sum = c_sum bit for bit."""
    _chk(noise_sum, "noise_sum", torch.float32); _chk(counter, "counter", torch.float32); _chk(delta, "delta", torch.float32)
    n = ftot * hw * 4
    assert noise_sum.is_contiguous() and noise_sum.numel() == 2 * n and counter.numel() >= ftot
    assert delta is None or (delta.is_contiguous() and delta.numel() == n)
    _lib.call("md_cfg_uncond_cache", noise_sum.data_ptr(), counter.data_ptr(), _p(delta), ftot, hw, int(mode), float(scale), _st(),
              meta=(f"cfg_uncond_cache F={ftot} HW={hw} mode={int(mode)}", 0.0, 4.0 * n * (2 if mode == 1 and not scale else 3)))


def free_init_mix(out, x0, noise0, z, lpf, a, b):
    """FreeInit's frequency mix (md_free_init_mix_f16): out = fp16(z + IDFT3(lpf * DFT3(a x0 + b noise0 - z))) per channel over (F, H, W).
    out / x0 / noise0 / z: contiguous (F, H, W, 4) fp16, out may be x0; lpf: contiguous (F, H, W) fp32, unshifted order
    (free_init.freq_filter).  a == 0 never reads x0.  A shape without a kernel raises; the workspace is kept per (device, stream)."""
    for t, name in ((out, "out"), (x0, "x0"), (noise0, "noise0"), (z, "z")):
        _chk(t, name)
    _chk(lpf, "lpf", torch.float32)
    if out.dim() != 4 or out.shape[-1] != 4:
        raise _lib.MdanceHipError(f"free_init_mix: latents must be (F, H, W, 4), got {tuple(out.shape)}")
    F, H, W, _ = out.shape
    if not _lib.load().md_free_init_plan(F, H, W):
        raise _lib.MdanceHipError(f"free_init_mix: no kernel for a clip of F={F} H={H} W={W} (every axis must be 1..256)")
    assert all(t.is_contiguous() and t.shape == out.shape for t in (out, x0, noise0, z)), [tuple(t.shape) for t in (out, x0, noise0, z)]
    assert lpf.is_contiguous() and tuple(lpf.shape) == (F, H, W), (tuple(lpf.shape), (F, H, W))
    ws = _workspace("free_init_mix", out.device, _lib.load().md_free_init_workspace_bytes(F, H, W))
    n = F * H * W * 4
    _lib.call("md_free_init_mix_f16", out.data_ptr(), x0.data_ptr(), noise0.data_ptr(), z.data_ptr(), lpf.data_ptr(), F, H, W, float(a), float(b),
              ws.data_ptr(), ws.numel() * 4, _st(),
              meta=(f"free_init_mix F={F} H={H} W={W}", 16.0 * n * (F + H + W), 2.0 * n * 4 + 1.0 * n + 12 * 8.0 * n))
    return out


POOL_MODES = {"nearest": 0, "mean": 1}


def token_pool(x, B, Hh, Ww, s, mode="nearest", out=None):
    """Token downsampling of a K / V source (md_token_pool_f16; ToDo, arXiv 2402.13573): x [B*Hh*Ww, C] contiguous, the tokens of B frames ->
    (y, Lk, stride): y [B*stride, C], frame b in rows [b*stride, b*stride + Lk), Lk = (Hh // s) * (Ww // s), stride = roundup8(Lk), the rows
    behind Lk exact zeros (the pad of `attention`: pass kv_stride=stride).  mode "nearest": the token at (oy*s, ox*s); "mean": the mean of the
    s x s block, fp32, one rounding.  `out`: a contiguous [B*stride, C] destination."""
    _chk(x, "x"); _chk(out, "out")
    if mode not in POOL_MODES:
        raise _lib.MdanceHipError(f"token_pool: mode must be one of {sorted(POOL_MODES)}, got {mode!r}")
    if x.dim() != 2 or not x.is_contiguous() or x.shape[0] != B * Hh * Ww:
        raise _lib.MdanceHipError(f"token_pool: x must be a contiguous [B*Hh*Ww, C] matrix, got {tuple(x.shape)} for B={B} Hh={Hh} Ww={Ww}")
    C = x.shape[1]
    Ho, Wo = Hh // s, Ww // s
    Lk = Ho * Wo
    stride = (Lk + 7) // 8 * 8
    if out is None:
        out = torch.empty((B * stride, C), device=x.device, dtype=F16)
    assert out.is_contiguous() and tuple(out.shape) == (B * stride, C), (tuple(out.shape), (B * stride, C))
    taps = s * s if mode == "mean" else 1
    _lib.call("md_token_pool_f16", x.data_ptr(), out.data_ptr(), B, Hh, Ww, C, s, POOL_MODES[mode], stride, _st(),
              meta=(f"token_pool B={B} {Hh}x{Ww} C={C} s={s} {mode}", 1.0 * B * Lk * C * (taps if taps > 1 else 0), 2.0 * B * C * (Lk * taps + stride)))
    return out, Lk, stride


def _tile_call(who, x, B, Hh, Ww, t, shift, tile_stride, out, inverse):
    """The argument checks the two wrappers share and the one launch of md_token_tile_f16 -> (out, Lt, tile_stride)."""
    _chk(x, "x"); _chk(out, "out")
    sy, sx = shift
    if t < 1 or Hh % t or Ww % t:
        raise _lib.MdanceHipError(f"{who}: t = {t} does not divide the {Hh} x {Ww} grid")
    Lt = (Hh // t) * (Ww // t)
    tile_stride = Lt if tile_stride is None else tile_stride
    rows_tile, rows_frame = B * t * t * tile_stride, B * Hh * Ww
    rows_in, rows_out = (rows_tile, rows_frame) if inverse else (rows_frame, rows_tile)
    if x.dim() != 2 or not x.is_contiguous() or x.shape[0] != rows_in:
        raise _lib.MdanceHipError(f"{who}: x must be a contiguous [{rows_in}, C] matrix, got {tuple(x.shape)} for B={B} Hh={Hh} Ww={Ww} t={t} "
                                  f"tile_stride={tile_stride}")
    C = x.shape[1]
    if out is None:
        out = torch.empty((rows_out, C), device=x.device, dtype=F16)
    assert out.is_contiguous() and tuple(out.shape) == (rows_out, C), (tuple(out.shape), (rows_out, C))
    rows_read = B * t * t * Lt                                     # either direction reads the B*Hh*Ww tokens (the inverse skips the pad rows) and writes rows_out
    _lib.call("md_token_tile_f16", x.data_ptr(), out.data_ptr(), B, Hh, Ww, C, t, sy, sx, tile_stride, int(inverse), _st(),
              meta=(f"{who} B={B} {Hh}x{Ww} C={C} t={t}", 0.0, 2.0 * C * (rows_read + rows_out)))
    return out, Lt, tile_stride


def token_tile(x, B, Hh, Ww, t, shift=(0, 0), tile_stride=None, out=None):
    """Frame order -> tile-major order for tiled self-attention (md_token_tile_f16; MSW-MSA of HiDiffusion, arXiv 2311.17528): x [B*Hh*Ww, C]
    contiguous, the tokens of B frames -> (y, Lt, tile_stride): y [B*t*t*tile_stride, C], tile (b, j, i) = batch item (b*t + j)*t + i holding the
    th x tw = (Hh // t) x (Ww // t) tokens of torch.roll(grid, (-sy, -sx), (1, 2)) at (j*th.., i*tw..), Lt = th*tw, the rows behind Lt exact
    zeros.  shift = (sy, sx), 0 <= sy < Hh, 0 <= sx < Ww; tile_stride: rows per tile, default Lt (a Q operand; pass roundup8(Lt) for K / V and
    kv_stride=tile_stride to `attention`).  `out`: a contiguous [B*t*t*tile_stride, C] destination."""
    return _tile_call("token_tile", x, B, Hh, Ww, t, shift, tile_stride, out, False)


def token_untile(x, B, Hh, Ww, t, shift=(0, 0), tile_stride=None, out=None):
    """The inverse of token_tile with the same arguments: x [B*t*t*tile_stride, C] tile-major -> y [B*Hh*Ww, C] in frame order.  The pad rows
    of x are not read."""
    return _tile_call("token_untile", x, B, Hh, Ww, t, shift, tile_stride, out, True)[0]


RESIZE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}
RESIZE_TAPS = {"nearest": 1, "bilinear": 4, "bicubic": 16}


def latent_resize(x, F, hi, wi, ho, wo, mode="bicubic", out=None):
    """Resampling of packed latents (md_latent_resize_f16; two-pass high-resolution sampling): x contiguous fp16 of F*hi*wi*4 elements, the
    loop's (F, hi, wi, 4) layout -> y (F, ho, wo, 4).  mode "nearest" (nearest-exact), "bilinear" or "bicubic", each as F.interpolate(size=(ho, wo),
    align_corners=False, antialias=False); any ratio, no antialiasing on the way down.  `out`: a contiguous destination of F*ho*wo*4 elements
    that does not overlap x."""
    _chk(x, "x"); _chk(out, "out")
    if mode not in RESIZE_MODES:
        raise _lib.MdanceHipError(f"latent_resize: mode must be one of {sorted(RESIZE_MODES)}, got {mode!r}")
    if min(F, hi, wi, ho, wo) < 1:
        raise _lib.MdanceHipError(f"latent_resize: F, hi, wi, ho, wo must be positive, got {(F, hi, wi, ho, wo)}")
    if not x.is_contiguous() or x.numel() != F * hi * wi * 4:
        raise _lib.MdanceHipError(f"latent_resize: x must be contiguous with F*hi*wi*4 = {F * hi * wi * 4} elements, got shape {tuple(x.shape)} "
                                  f"strides {tuple(x.stride())}")
    if out is None:
        out = torch.empty((F, ho, wo, 4), device=x.device, dtype=F16)
    if not out.is_contiguous() or out.numel() != F * ho * wo * 4:
        raise _lib.MdanceHipError(f"latent_resize: out must be contiguous with F*ho*wo*4 = {F * ho * wo * 4} elements, got shape {tuple(out.shape)}")
    n_out = F * ho * wo
    taps = RESIZE_TAPS[mode]
    _lib.call("md_latent_resize_f16", x.data_ptr(), out.data_ptr(), F, hi, wi, ho, wo, RESIZE_MODES[mode], _st(),
              meta=(f"latent_resize F={F} {hi}x{wi}->{ho}x{wo} {mode}", 8.0 * n_out * taps if taps > 1 else 0.0, 8.0 * (F * hi * wi + n_out)))
    return out


def tile_blend(cur, dst, c, above=None, left=None, extent=(0, 0)):
    """Seam blending of one tile of a tiled VAE pass (md_tile_blend_f16): cur (B, Th, Tw, ldc) contiguous NHWC fp16 with c <= ldc valid channels is
    blended IN PLACE over its first extent[0] rows with the last rows of `above` (B, Ah, Tw, ldc) and then over its first extent[1] columns with
    the last columns of `left` (B, Th, Lw, ldc), both as they stand after their own calls (the extents clamped to the tiles' sizes), and its
    top-left keep_h x keep_w corner is written to dst: a (B, c, keep_h, keep_w) fp16 / fp32 VIEW of the final NCHW tensor at the tile's place, any
    strides.  Returns cur."""
    _chk(cur, "cur"); _chk(above, "above"); _chk(left, "left")
    if cur.dim() != 4 or not cur.is_contiguous():
        raise _lib.MdanceHipError(f"tile_blend: cur must be a contiguous (B, Th, Tw, ldc) tensor, got shape {tuple(cur.shape)} strides {tuple(cur.stride())}")
    B, Th, Tw, ldc = cur.shape
    if above is not None and (above.dim() != 4 or not above.is_contiguous() or (above.shape[0], above.shape[2], above.shape[3]) != (B, Tw, ldc)):
        raise _lib.MdanceHipError(f"tile_blend: above must be contiguous (B, Ah, Tw, ldc) = ({B}, *, {Tw}, {ldc}), got {tuple(above.shape)}")
    if left is not None and (left.dim() != 4 or not left.is_contiguous() or (left.shape[0], left.shape[1], left.shape[3]) != (B, Th, ldc)):
        raise _lib.MdanceHipError(f"tile_blend: left must be contiguous (B, Th, Lw, ldc) = ({B}, {Th}, *, {ldc}), got {tuple(left.shape)}")
    if not dst.is_cuda or dst.dtype not in (torch.float16, torch.float32):
        raise _lib.MdanceHipError("tile_blend: dst must be a CUDA fp16/fp32 tensor")
    if dst.dim() != 4 or dst.shape[0] != B or dst.shape[1] != c or not (1 <= dst.shape[2] <= Th and 1 <= dst.shape[3] <= Tw):
        raise _lib.MdanceHipError(f"tile_blend: dst must be a (B, c, keep_h <= Th, keep_w <= Tw) = ({B}, {c}, <= {Th}, <= {Tw}) view, got {tuple(dst.shape)}")
    sB, sC, sY, sX = dst.stride()
    keep_h, keep_w = dst.shape[2:]
    ev, eh = extent
    n = B * Th * Tw * c
    _lib.call("md_tile_blend_f16", cur.data_ptr(), ldc, _p(above), 0 if above is None else above.shape[1], _p(left),
              0 if left is None else left.shape[2], dst.data_ptr(), int(dst.dtype == torch.float32), B, Th, Tw, c, int(ev), int(eh), keep_h, keep_w,
              sB, sC, sY, sX, _st(),
              meta=(f"tile_blend B={B} {Th}x{Tw} C={c}", 0.0, 4.0 * n + dst.element_size() * B * c * keep_h * keep_w))
    return cur


def frames_u8(src, out=None, *, f32_math=None):
    """Decoded frames -> the bytes the writers take (md_frames_u8): src (B, C, H, W)-shaped fp16 / fp32 with ANY strides, C in 1..4 -- an NHWC
    buffer is passed as its permuted view, the strides say what it is -- -> out (B, H, W, C) uint8, the reference's
    ((x / 2 + 0.5).clamp(0, 1).float() * 255) truncated, operation by operation: in fp16 with f32_math=False, in fp32 with f32_math=True;
    None: as the source dtype.  An fp32 source needs fp32 arithmetic.  NaN gives 0.  `out`: a uint8 (B, H, W, C) tensor or VIEW whose last two
    dimensions are packed (stride C and 1); the row and frame pitches are free, so a frame can land inside a larger canvas.  Returns out."""
    B, C, H, W = _frame_src("frames_u8", src, range(1, 5))
    if f32_math is None:
        f32_math = src.dtype == torch.float32
    if not isinstance(f32_math, bool):
        raise _lib.MdanceHipError(f"frames_u8: f32_math must be True, False or None, got {f32_math!r}")
    if src.dtype == torch.float32 and not f32_math:
        raise _lib.MdanceHipError("frames_u8: an fp32 source needs f32_math=True")
    out, dB, dY = _byte_dst("frames_u8", out, B, H, W, C, src.device)
    n = B * H * W * C
    _lib.call("md_frames_u8", src.data_ptr(), int(src.dtype == torch.float32), int(f32_math), out.data_ptr(), B, H, W, C, *src.stride(), dB, dY, _st(),
              meta=(f"frames_u8 B={B} {H}x{W} C={C} {'f32' if f32_math else 'f16'}", 0.0, float(src.element_size() * n + n)))
    return out


def blur_kernel_size(sigma, n):
    """Taps of SEG's Gaussian along a grid axis of n tokens: the official gaussian_blur_2d's ceil(6 sigma) + 1 - ceil(6 sigma) % 2, clamped to
    the largest odd number a reflect-padded axis of n allows (n if n is odd, else n + 1); 1 for n = 1."""
    import math
    c = math.ceil(6.0 * sigma)
    return int(min(c + 1 - c % 2, n if n % 2 else n + 1))


def blur_taps(sigma, n):
    """The normalised Gaussian taps w_j ~ exp(-(j / sigma)^2 / 2), j = -r..r, r = blur_kernel_size(sigma, n) // 2, in float64 (a list)."""
    import math
    r = blur_kernel_size(sigma, n) // 2
    w = [math.exp(-0.5 * (j / sigma) ** 2) for j in range(-r, r + 1)]
    tot = math.fsum(w)
    return [v / tot for v in w]


_blur_tables = {}


def token_blur(x, B, Hh, Ww, sigma, out=None):
    """The query blur of smoothed-energy guidance (SEG, arXiv 2408.00760; md_token_blur_f16 / md_token_mean_f16): x [B*Hh*Ww, C] contiguous,
    the tokens of B frames on an Hh x Ww grid -> y of the same shape, every channel filtered on its own.  sigma: a finite float > 0 -- the
    separable Gaussian with reflect padding, taps per axis as blur_taps (float64 on the host, rounded once to fp32, kept on the device per
    (sigma, n)) -- or math.inf: every token becomes its frame's mean.  fp32 throughout, one rounding; `out`: a contiguous destination of x's
    shape that does not overlap x.  The fp32 workspace is kept per (device, stream)."""
    import math
    _chk(x, "x"); _chk(out, "out")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or math.isnan(sigma) or not sigma > 0:
        raise _lib.MdanceHipError(f"token_blur: sigma must be a positive float or math.inf, got {sigma!r}")
    if x.dim() != 2 or not x.is_contiguous() or B < 1 or Hh < 1 or Ww < 1 or x.shape[0] != B * Hh * Ww:
        raise _lib.MdanceHipError(f"token_blur: x must be a contiguous [B*Hh*Ww, C] matrix, got {tuple(x.shape)} for B={B} Hh={Hh} Ww={Ww}")
    C = x.shape[1]
    if out is None:
        out = torch.empty_like(x)
    assert out.is_contiguous() and out.shape == x.shape, (tuple(out.shape), tuple(x.shape))
    ws = _workspace("token_blur", x.device, _lib.load().md_token_blur_workspace_bytes(B, Hh, Ww, C))
    n = B * Hh * Ww * C
    if math.isinf(sigma):
        _lib.call("md_token_mean_f16", x.data_ptr(), out.data_ptr(), B, Hh * Ww, C, ws.data_ptr(), _st(),
                  meta=(f"token_blur B={B} {Hh}x{Ww} C={C} mean", 1.0 * n, 4.0 * n))
        return out
    tabs = []
    for ax in (Hh, Ww):
        tkey = (x.device, float(sigma), ax)
        t = _blur_tables.get(tkey)
        if t is None:
            t = _blur_tables[tkey] = torch.tensor(blur_taps(float(sigma), ax), dtype=torch.float64).to(torch.float32).to(x.device)
        tabs.append(t)
    wy, wx = tabs
    _lib.call("md_token_blur_f16", x.data_ptr(), out.data_ptr(), B, Hh, Ww, C, wy.data_ptr(), wy.numel(), wx.data_ptr(), wx.numel(), ws.data_ptr(),
              _st(), meta=(f"token_blur B={B} {Hh}x{Ww} C={C} k={wy.numel()}x{wx.numel()}", 2.0 * n * (wy.numel() + wx.numel()), 12.0 * n))
    return out


def rel_l1(a, b, out=None):
    """The distance of adaptive DeepCache (md_rel_l1_f16): a, b fp16 of one shape (..., C), each contiguous or a channel slice of a wider
    contiguous tensor (one uniform row pitch each, see _pixel_pitch; the two pitches may differ) -> 2 fp32 on the device,
    (sum |a - b|, sum |b|), fp32 terms and sums in a fixed order: the same inputs give the same bits.  Nothing is read back: the caller does.
    `out`: a contiguous fp32 destination of 2 elements.  The 16 KiB workspace is kept per (device, stream)."""
    lda, ldb = _pixel_pitch(a, "a", align=1), _pixel_pitch(b, "b", align=1)
    if a.shape != b.shape or a.numel() == 0 or a.device != b.device:
        raise _lib.MdanceHipError(f"rel_l1: a and b must be non-empty, of one shape and on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    C = a.shape[-1]
    rows = a.numel() // C
    if rows >= 1 << 31 or max(lda, ldb) >= 1 << 31:
        raise _lib.MdanceHipError(f"rel_l1: {rows} rows of pitch {lda} / {ldb} exceed the entry point's int arguments")
    if out is None:
        out = torch.empty((2,), device=a.device, dtype=torch.float32)
    _chk(out, "out", torch.float32)
    if out.shape != (2,) or not out.is_contiguous() or out.device != a.device:
        raise _lib.MdanceHipError(f"rel_l1: out must be 2 contiguous fp32 on a's device, got {tuple(out.shape)}")
    ws = _workspace("rel_l1", a.device, _lib.load().md_rel_l1_workspace_bytes(rows, C), floor=1 << 14)
    _lib.call("md_rel_l1_f16", a.data_ptr(), lda, b.data_ptr(), ldb, rows, C, ws.data_ptr(), ws.numel() * 4, out.data_ptr(), _st(),
              meta=(f"rel_l1 rows={rows} C={C}", 2.0 * rows * C, 4.0 * rows * C))
    return out


def _frame_src(who, src, channels):
    """The source refusals frames_u8 and both colour-matching operators share; channels: the counts taken, a range -> (B, C, H, W)."""
    if not src.is_cuda or src.dtype not in (torch.float16, torch.float32):
        raise _lib.MdanceHipError(f"{who}: src must be a CUDA fp16/fp32 tensor")
    if src.dim() != 4 or src.shape[1] not in channels or min(src.shape) < 1:
        lo, hi = channels[0], channels[-1]
        form = f"(B, {lo}, H, W)-shaped with" if lo == hi else f"(B, C, H, W)-shaped with C in {lo}..{hi} and"
        raise _lib.MdanceHipError(f"{who}: src must be {form} no empty dimension, got {tuple(src.shape)}")
    B, C, H, W = src.shape
    if B * H * W >= 1 << 31:
        raise _lib.MdanceHipError(f"{who}: B*H*W = {B * H * W} exceeds the entry point's int arguments")
    return B, C, H, W


def _byte_dst(who, out, B, H, W, C, device):
    """The byte destination of frames_u8 and color_apply: a uint8 (B, H, W, C) tensor or VIEW with packed pixels (a new tensor for None) ->
    (out, dB, dY), the frame and row pitches the entry points take."""
    if out is None:
        out = torch.empty((B, H, W, C), device=device, dtype=torch.uint8)
    if not out.is_cuda or out.dtype != torch.uint8 or out.device != device:
        raise _lib.MdanceHipError(f"{who}: out must be a CUDA uint8 tensor on src's device")
    if tuple(out.shape) != (B, H, W, C) or out.stride(3) != 1 or out.stride(2) != C:
        raise _lib.MdanceHipError(f"{who}: out must be a (B, H, W, C) = ({B}, {H}, {W}, {C}) view with packed pixels (strides (*, *, {C}, 1)), got shape "
                                  f"{tuple(out.shape)} strides {tuple(out.stride())}")
    dY = out.stride(1) if H > 1 else max(out.stride(1), W * C)           # the stride of a dimension of size 1 says nothing
    dB = out.stride(0) if B > 1 else max(out.stride(0), (H - 1) * dY + W * C)
    return out, dB, dY


def color_moments(src, out=None):
    """The colour moments of decoded frames (md_color_moments): src (B, 3, H, W)-shaped fp16 / fp32 with ANY strides, as frames_u8 takes it ->
    (B, 9) float64 on the device, per frame the sums over its pixels of s0, s1, s2, s0^2, s1^2, s2^2, s0 s1, s0 s2, s1 s2 with
    s = clamp(0.5 v + 0.5, 0, 1) in fp32 (NaN kept): fp32 terms, fp32 sums per workgroup, fp64 across workgroups, all in a fixed order
    (csrc/color_match.hip), so the same input gives the same bits.  Nothing is read back: the caller does.  `out`: a contiguous float64
    (B, 9) destination.  The workspace (36 bytes per 8192 pixels) is kept per (device, stream)."""
    B, _, H, W = _frame_src("color_moments", src, range(3, 4))
    if out is None:
        out = torch.empty((B, 9), device=src.device, dtype=torch.float64)
    _chk(out, "out", torch.float64)
    if tuple(out.shape) != (B, 9) or not out.is_contiguous() or out.device != src.device:
        raise _lib.MdanceHipError(f"color_moments: out must be ({B}, 9) contiguous float64 on src's device, got {tuple(out.shape)}")
    ws = _workspace("color_moments", src.device, _lib.load().md_color_moments_workspace_bytes(B, H, W), floor=1 << 16)
    sB, sC, sY, sX = src.stride()
    n = B * H * W * 3
    _lib.call("md_color_moments", src.data_ptr(), int(src.dtype == torch.float32), B, H, W, sB, sC, sY, sX, ws.data_ptr(), ws.numel() * 4,
              out.data_ptr(), _st(), meta=(f"color_moments B={B} {H}x{W}", 5.0 * n, float(src.element_size() * n + 72 * B)))
    return out


def color_apply(src, coef, out=None, *, dtype=torch.uint8):
    """The affine colour map in front of the output quantisation (md_color_apply): src as color_moments takes it, coef (B, 12) contiguous
    fp32 on the device, frame b's row-major 3 x 3 matrix M then its offset t -> y = clamp(M s + t, 0, 1), every operation rounded in fp32.
    dtype torch.uint8: out (B, H, W, 3) bytes, fp32(y * 255) truncated, NaN -> 0, `out` as frames_u8 takes it (packed pixels, free row and
    frame pitches); dtype torch.float32: out (B, 3, H, W) fp32 with any positive strides, y itself, NaN kept.  Returns out."""
    B, _, H, W = _frame_src("color_apply", src, range(3, 4))
    _chk(coef, "coef", torch.float32)
    if tuple(coef.shape) != (B, 12) or not coef.is_contiguous() or coef.device != src.device:
        raise _lib.MdanceHipError(f"color_apply: coef must be ({B}, 12) contiguous fp32 on src's device, got {tuple(coef.shape)}")
    if dtype not in (torch.uint8, torch.float32):
        raise _lib.MdanceHipError(f"color_apply: dtype must be torch.uint8 or torch.float32, got {dtype!r}")
    sB, sC, sY, sX = src.stride()
    n = B * H * W * 3
    if dtype == torch.uint8:
        out, dB, dY = _byte_dst("color_apply", out, B, H, W, 3, src.device)
        dst = (dB, 1, dY, 3)
    else:
        if out is None:
            out = torch.empty((B, 3, H, W), device=src.device, dtype=torch.float32)
        if not out.is_cuda or out.dtype != torch.float32 or out.device != src.device:
            raise _lib.MdanceHipError("color_apply: out must be a CUDA float32 tensor on src's device")
        if tuple(out.shape) != (B, 3, H, W):
            raise _lib.MdanceHipError(f"color_apply: out must be (B, 3, H, W) = ({B}, 3, {H}, {W}), got {tuple(out.shape)}")
        dst = tuple(max(s, 1) if d == 1 else s for s, d in zip(out.stride(), out.shape))     # (dB, dC, dY, dX)
        if min(dst) < 1:
            raise _lib.MdanceHipError(f"color_apply: out must not be an expanded view, got strides {tuple(out.stride())}")
    _lib.call("md_color_apply", src.data_ptr(), int(src.dtype == torch.float32), coef.data_ptr(), out.data_ptr(), int(dtype == torch.float32), B, H, W,
              sB, sC, sY, sX, *dst, _st(),
              meta=(f"color_apply B={B} {H}x{W} {'f32' if dtype == torch.float32 else 'u8'}", 7.0 * n, float((src.element_size() + out.element_size()) * n + 48 * B)))
    return out
