"""AutoencoderKL on the MI355X kernels (the row after the denoising loop).

The reference pipeline calls a third-party diffusers==0.24.0 `AutoencoderKL` (sd-vae-ft-mse) for 3F+2 encodes and F decodes
per clip (src/pipelines/pipeline_mikudance.py:115-130 decode_latents, :456-549 `self.vae.encode(...).latent_dist.mean`;
built at scripts/inference_video.py:72-79).  This module keeps that interface -- `from_pretrained`, `.encode(x).latent_dist`
(`.mean`, `.sample()`), `.decode(z).sample`, `.dtype`, `.device`, `.config.scaling_factor` -- and the diffusers state-dict
key layout (incl. the legacy `query/key/value/proj_attn` attention names of the published checkpoint), and runs on the
same C-ABI kernels as the UNets: NHWC 3x3 convs (the encoder's downsampler pads (0,1,0,1): `pad_lo = 0`), GroupNorm(+SiLU),
GEMMs.  The mid-block attention has ONE head of 512 channels -- too wide for the flash kernel's register tile -- so it runs
per frame as QK^T GEMM -> row softmax (md_softmax_rows_f16) -> PV GEMM.

Tiling and slicing (`enable_tiling` / `enable_slicing`, `tiled_encode` / `tiled_decode`; off by default): diffusers 0.24's names and rules, restated
from the published algorithm -- overlapping tiles of `tile_sample_min_size` pixels / `tile_latent_min_size` latents, each through the whole
encoder + quant_conv or post_quant_conv + decoder, the seams blended over `tile_overlap_factor` of a tile, vertical then horizontal, on the
neighbour as blended.  One md_tile_blend_f16 launch per tile blends, crops and writes into the final NCHW tensor (`tile_grid` is the geometry).
A tiled result DIFFERS from the untiled one by design: every tile's GroupNorm and attention see that tile only.

Parity: the oracle's restatement (oracle/cpu_ref.py vae_*) follows the published diffusers semantics; diffusers is not in
/root/reference, so this row -- tiling and slicing included -- is PARITY UNPINNED."""
import json
import os
from types import SimpleNamespace

import torch
from torch import nn

from . import ops, packing
from .blocks import GROUPS, Affine, Conv, Linear, _Packed, tokens

EPS = 1e-6


class VaeResnet(_Packed):
    """diffusers ResnetBlock2D with temb_channels=None: GN+SiLU -> conv -> GN+SiLU -> conv (+1x1 shortcut), eps 1e-6."""

    def __init__(self, cin, cout):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.norm1 = Affine(cin)
        self.conv1 = Conv(cin, cout, 3)
        self.norm2 = Affine(cout)
        self.conv2 = Conv(cout, cout, 3)
        self.conv_shortcut = Conv(cin, cout, 1) if cin != cout else None

    def _pack(self, dev):
        pk = dict(n1w=packing.vec(self.norm1.weight, dev), n1b=packing.vec(self.norm1.bias, dev),
                  n2w=packing.vec(self.norm2.weight, dev), n2b=packing.vec(self.norm2.bias, dev),
                  c1=packing.conv3x3_weight(self.conv1.weight, dev), c1b=packing.vec(self.conv1.bias, dev),
                  c2=packing.conv3x3_weight(self.conv2.weight, dev), c2b=packing.vec(self.conv2.bias, dev))
        if self.conv_shortcut is not None:
            pk["sc"] = packing.conv1x1_weight(self.conv_shortcut.weight, dev)
            pk["scb"] = packing.vec(self.conv_shortcut.bias, dev)
        return pk

    def forward(self, x):
        pk = self.packed()
        h = ops.groupnorm(x, pk["n1w"], pk["n1b"], GROUPS, EPS, silu=True)
        h = ops.conv3x3(h, pk["c1"], self.cout, bias=pk["c1b"])
        h = ops.groupnorm(h, pk["n2w"], pk["n2b"], GROUPS, EPS, silu=True)
        sc = x if self.conv_shortcut is None else ops.gemm(tokens(x), pk["sc"], bias=pk["scb"]).view(x.shape[:-1] + (self.cout,))
        return ops.conv3x3(h, pk["c2"], self.cout, bias=pk["c2b"], residual=sc)


class VaeSampler(_Packed):
    """Downsample2D(padding=0): F.pad (0,1,0,1) + 3x3 stride-2 conv, or Upsample2D: nearest 2x + 3x3 conv (folded)."""

    def __init__(self, c, up):
        super().__init__()
        self.c, self.up = c, up
        self.conv = Conv(c, c, 3)

    def _pack(self, dev):
        return dict(w=packing.conv3x3_weight(self.conv.weight, dev), b=packing.vec(self.conv.bias, dev))

    def forward(self, x):
        pk = self.packed()
        if self.up:
            return ops.conv3x3(x, pk["w"], self.c, bias=pk["b"], upsample=True)
        return ops.conv3x3(x, pk["w"], self.c, bias=pk["b"], stride=2, pad_lo=0)


class VaeAttention(_Packed):
    """diffusers Attention(heads=1, dim_head=C, bias=True, norm_num_groups=32, residual_connection=True) on a feature map."""

    def __init__(self, c):
        super().__init__()
        self.c = c
        self.group_norm = Affine(c)
        self.to_q, self.to_k, self.to_v = Linear(c, c), Linear(c, c), Linear(c, c)
        self.to_out = nn.ModuleList([Linear(c, c)])

    def _pack(self, dev):
        L, V = packing.linear_weight, packing.vec
        return dict(nw=V(self.group_norm.weight, dev), nb=V(self.group_norm.bias, dev),
                    q=L(self.to_q.weight, dev), qb=V(self.to_q.bias, dev), k=L(self.to_k.weight, dev), kb=V(self.to_k.bias, dev),
                    v=L(self.to_v.weight, dev), vb=V(self.to_v.bias, dev),
                    o=L(self.to_out[0].weight, dev), ob=V(self.to_out[0].bias, dev))

    def forward(self, x):
        pk = self.packed()
        B, Hh, Ww, C = x.shape
        L = Hh * Ww
        if L % 8:
            raise ValueError(f"AutoencoderKL mid attention: {Hh}x{Ww} tokens must be a multiple of 8")
        Lp = packing.pad_to(L, 64)                                       # K of the PV GEMM
        n = tokens(ops.groupnorm(x, pk["nw"], pk["nb"], GROUPS, EPS))
        q = ops.gemm(n, pk["q"], bias=pk["qb"])
        k = ops.gemm(n, pk["k"], bias=pk["kb"])
        a = torch.empty((B * L, C), device=x.device, dtype=torch.float16)
        s = torch.zeros((L, Lp), device=x.device, dtype=torch.float16)    # score matrix of one frame (padding columns stay 0)
        vt = torch.zeros((C, Lp), device=x.device, dtype=torch.float16)
        for b in range(B):
            rows = slice(b * L, (b + 1) * L)
            ops.gemm(n[rows], pk["v"], bias=pk["vb"], transpose_out=True, out=vt)      # V^T [C][Lp], columns >= L stay zero
            ops.gemm(q[rows], k[rows], out=s[:, :L])
            ops.softmax_rows_(s[:, :L], scale=C ** -0.5)
            ops.gemm(s, vt, out=a[rows])
        return ops.gemm(a, pk["o"], bias=pk["ob"], residual=tokens(x)).view(x.shape)


class VaeMid(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnet(c, c), VaeResnet(c, c)])
        self.attentions = nn.ModuleList([VaeAttention(c)])

    def forward(self, x):
        return self.resnets[1](self.attentions[0](self.resnets[0](x)))


class _DownBlock(nn.Module):
    def __init__(self, cin, cout, down):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnet(cin, cout), VaeResnet(cout, cout)])
        if down:
            self.downsamplers = nn.ModuleList([VaeSampler(cout, up=False)])
        self.down = down

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.downsamplers[0](x) if self.down else x


class _UpBlock(nn.Module):
    def __init__(self, cin, cout, up):
        super().__init__()
        self.resnets = nn.ModuleList([VaeResnet(cin if i == 0 else cout, cout) for i in range(3)])
        if up:
            self.upsamplers = nn.ModuleList([VaeSampler(cout, up=True)])
        self.up = up

    def forward(self, x):
        for r in self.resnets:
            x = r(x)
        return self.upsamplers[0](x) if self.up else x


class Encoder(_Packed):
    def __init__(self, in_channels, latent_channels, chans):
        super().__init__()
        self.in_channels, self.zc = in_channels, 2 * latent_channels
        self.conv_in = Conv(in_channels, chans[0], 3)
        self.down_blocks = nn.ModuleList([_DownBlock(chans[max(i - 1, 0)], c, i < len(chans) - 1) for i, c in enumerate(chans)])
        self.mid_block = VaeMid(chans[-1])
        self.conv_norm_out = Affine(chans[-1])
        self.conv_out = Conv(chans[-1], self.zc, 3)
        self.c0 = chans[0]

    def _pack(self, dev):
        return dict(ci=packing.conv3x3_weight(self.conv_in.weight, dev), cib=packing.vec(self.conv_in.bias, dev),
                    nw=packing.vec(self.conv_norm_out.weight, dev), nb=packing.vec(self.conv_norm_out.bias, dev),
                    co=packing.conv3x3_weight(self.conv_out.weight, dev), cob=packing.vec(self.conv_out.bias, dev))

    def forward(self, x64):
        """x64: (B, H, W, 64) fp16, image channels first, zero padded.  Returns (B, H/8, W/8, 64) with 2*latent valid channels."""
        pk = self.packed()
        h = ops.conv3x3(x64, pk["ci"], self.c0, bias=pk["cib"])
        for blk in self.down_blocks:
            h = blk(h)
        h = self.mid_block(h)
        h = ops.groupnorm(h, pk["nw"], pk["nb"], GROUPS, EPS, silu=True)
        out = torch.zeros(h.shape[:3] + (64,), device=h.device, dtype=torch.float16)
        ops.conv3x3(h, pk["co"], self.zc, bias=pk["cob"], out=out[..., :self.zc])
        return out


class Decoder(_Packed):
    def __init__(self, latent_channels, out_channels, chans):
        super().__init__()
        self.out_channels = out_channels
        rev = list(reversed(chans))
        self.conv_in = Conv(latent_channels, rev[0], 3)
        self.mid_block = VaeMid(rev[0])
        self.up_blocks = nn.ModuleList([_UpBlock(rev[max(i - 1, 0)], c, i < len(rev) - 1) for i, c in enumerate(rev)])
        self.conv_norm_out = Affine(rev[-1])
        self.conv_out = Conv(rev[-1], out_channels, 3)
        self.c0 = rev[0]

    def _pack(self, dev):
        return dict(ci=packing.conv3x3_weight(self.conv_in.weight, dev), cib=packing.vec(self.conv_in.bias, dev),
                    nw=packing.vec(self.conv_norm_out.weight, dev), nb=packing.vec(self.conv_norm_out.bias, dev),
                    co=packing.conv3x3_weight(self.conv_out.weight, dev), cob=packing.vec(self.conv_out.bias, dev))

    def forward(self, z64):
        """z64: (B, h, w, 64) fp16 (post_quant_conv output, zero padded).  Returns (B, 8h, 8w, out_channels) fp16."""
        pk = self.packed()
        h = ops.conv3x3(z64, pk["ci"], self.c0, bias=pk["cib"])
        h = self.mid_block(h)
        for blk in self.up_blocks:
            h = blk(h)
        h = ops.groupnorm(h, pk["nw"], pk["nb"], GROUPS, EPS, silu=True)
        return ops.conv3x3(h, pk["co"], self.out_channels, bias=pk["cob"])


class DiagonalGaussian:
    """diffusers DiagonalGaussianDistribution: moments (B, 2z, h, w) -> mean | logvar (clamped to [-30, 20])."""

    def __init__(self, moments):
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)

    def sample(self, generator=None):
        noise = torch.randn(self.mean.shape, generator=generator, device="cpu" if generator is not None and generator.device.type == "cpu"
                            else self.mean.device, dtype=torch.float32).to(self.mean.device, self.mean.dtype)
        return self.mean + self.std * noise

    def mode(self):
        return self.mean


class AutoencoderKL(_Packed):
    def __init__(self, in_channels=3, out_channels=3, block_out_channels=(128, 256, 512, 512), latent_channels=4, layers_per_block=2,
                 norm_num_groups=32, act_fn="silu", scaling_factor=0.18215, sample_size=512, down_block_types=None, up_block_types=None,
                 force_upcast=True, **unused):
        super().__init__()
        if layers_per_block != 2 or norm_num_groups != GROUPS or act_fn != "silu":
            raise ValueError("AutoencoderKL: only the sd-vae-ft-mse family (2 layers per block, 32 groups, SiLU) is built")
        chans = tuple(block_out_channels)
        if any(c % 64 for c in chans):
            raise ValueError(f"AutoencoderKL (MI355X): block_out_channels {chans} must be multiples of 64 (the conv / GEMM kernels tile "
                             "the channel dimension by 64; sd-vae-ft-mse is (128, 256, 512, 512))")
        self.config = SimpleNamespace(in_channels=in_channels, out_channels=out_channels, block_out_channels=chans,
                                      latent_channels=latent_channels, layers_per_block=2, norm_num_groups=GROUPS, act_fn="silu",
                                      scaling_factor=scaling_factor, sample_size=sample_size)
        self.zc = latent_channels
        self.use_tiling = self.use_slicing = False
        self.tile_sample_min_size = sample_size
        self.tile_latent_min_size = int(sample_size / 2 ** (len(chans) - 1))
        self.tile_overlap_factor = 0.25
        self.encoder = Encoder(in_channels, latent_channels, chans)
        self.decoder = Decoder(latent_channels, out_channels, chans)
        self.quant_conv = Conv(2 * latent_channels, 2 * latent_channels, 1)
        self.post_quant_conv = Conv(latent_channels, latent_channels, 1)

    dtype = property(lambda self: self.quant_conv.weight.dtype)
    device = property(lambda self: self.quant_conv.weight.device)

    def _pack(self, dev):
        def pad_k(w):                       # 1x1 conv weight (N, K, 1, 1) -> [N][64]
            out = torch.zeros((w.shape[0], 64), dtype=torch.float16, device=dev)
            out[:, :w.shape[1]] = w.detach().reshape(w.shape[0], w.shape[1]).to(dev, torch.float16)
            return out
        return dict(q=pad_k(self.quant_conv.weight), qb=packing.vec(self.quant_conv.bias, dev),
                    pq=pad_k(self.post_quant_conv.weight), pqb=packing.vec(self.post_quant_conv.bias, dev))

    # ---- reference-facing interface (NCHW tensors in / out, like diffusers)
    def _moments_nhwc(self, x):
        """x (B, C, H, W), any strides (a tile is a view) -> encoder + quant_conv -> (B, H/f, W/f, 64) fp16 NHWC, 2z valid channels."""
        pk = self.packed()
        B, C, H, W = x.shape
        st = x.stride()
        x64 = ops.pack_nhwc(x, B, 1, (st[0], 0, st[1], st[2], st[3]), 0, C, 64, H, W)
        h = self.encoder(x64)                                                            # (B, h, w, 64), 2z valid
        m64 = torch.zeros_like(h)
        ops.gemm(tokens(h), pk["q"], bias=pk["qb"], out=tokens(m64)[:, :2 * self.zc])
        return m64

    def _image_nhwc(self, z):
        """z (B, z, h, w), any strides -> post_quant_conv + decoder -> (B, f h, f w, out_channels) fp16 NHWC."""
        pk = self.packed()
        B, C, h, w = z.shape
        st = z.stride()
        z64 = ops.pack_nhwc(z, B, 1, (st[0], 0, st[1], st[2], st[3]), 0, C, 64, h, w)
        p64 = torch.zeros_like(z64)
        ops.gemm(tokens(z64), pk["pq"], bias=pk["pqb"], out=tokens(p64)[:, :self.zc])
        return self.decoder(p64)                                                         # (B, 8h, 8w, 3)

    @staticmethod
    def _out_dtype(t):
        return t.dtype if t.dtype != torch.float64 else torch.float32

    def _run(self, x, out, encode, tiled):
        """One untiled or tiled pass of x into `out` (a view of the final NCHW tensor), image by image under enable_slicing()."""
        B = x.shape[0]
        for sl in ([slice(b, b + 1) for b in range(B)] if self.use_slicing and B > 1 else [slice(0, B)]):
            xs, os_ = x[sl], out[sl]
            so = os_.stride()
            n, strides, size = xs.shape[0], (so[0], 0, so[1], so[2], so[3]), tuple(out.shape[1:])
            if tiled:
                self._tiled(xs, os_, encode)
            elif encode:
                ops.unpack_nhwc(self._moments_nhwc(xs), os_, n, 1, strides, *size)          # 2z of 64 channels
            else:
                ops.unpack_nhwc(self._image_nhwc(xs), os_, n, 1, strides, *size)            # the image, pitch out_channels

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        if x.dim() != 4 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"AutoencoderKL.encode expects (B, C, H, W) with H, W multiples of 8, got {tuple(x.shape)}")
        B, C, H, W = x.shape
        tiled = self.use_tiling and max(H, W) > self.tile_sample_min_size
        if tiled:
            self.tile_grid(H, W, encode=True)                                            # every refusal before the first launch
        moments = torch.empty((B, 2 * self.zc, H // 8, W // 8), device=x.device, dtype=self._out_dtype(x))
        self._run(x, moments, True, tiled)
        out = SimpleNamespace(latent_dist=DiagonalGaussian(moments))
        return out if return_dict else (out.latent_dist,)

    @torch.no_grad()
    def decode(self, z, return_dict=True):
        if z.dim() != 4 or z.shape[1] != self.zc:
            raise ValueError(f"AutoencoderKL.decode expects (B, {self.zc}, h, w), got {tuple(z.shape)}")
        B, C, h, w = z.shape
        tiled = self.use_tiling and max(h, w) > self.tile_latent_min_size
        if tiled:
            self.tile_grid(h, w, encode=False)
        img = torch.empty((B, self.config.out_channels, 8 * h, 8 * w), device=z.device, dtype=self._out_dtype(z))
        self._run(z, img, False, tiled)
        out = SimpleNamespace(sample=img)
        return out if return_dict else (img,)

    @torch.no_grad()
    def decode_u8(self, z, out=None):
        """decode(z) as the bytes a writer takes: (B, 8h, 8w, out_channels) uint8 on the device, bit for bit
        ((decode(z).sample / 2 + 0.5).clamp(0, 1).float() * 255) truncated, in the arithmetic of the dtype decode would have returned (fp16
        chain for fp16 latents, fp32 chain for fp32).  Untiled, the decoder's NHWC image goes into ops.frames_u8 (md_frames_u8) directly: no
        NCHW tensor, no elementwise pass.  With tiling or slicing on, decode runs as it stands and one frames_u8 reads its NCHW result.
        `out`: a destination view as ops.frames_u8 takes it."""
        return ops.frames_u8(self.decode_image_view(z), out, f32_math=self._out_dtype(z) == torch.float32)

    @torch.no_grad()
    def decode_image_view(self, z):
        """decode(z)'s image where the decoder left it, as the strided (B, out_channels, 8h, 8w) view decode_u8 hands to ops.frames_u8: the
        decoder's own NHWC buffer, permuted (fp16, no NCHW tensor, no elementwise pass), or decode's NCHW result with tiling or slicing on.
        The values are decode(z).sample's.  For the operators that read an image once at the output boundary (ops.color_moments /
        ops.color_apply)."""
        if z.dim() != 4 or z.shape[1] != self.zc:
            raise ValueError(f"AutoencoderKL.decode_image_view expects (B, {self.zc}, h, w), got {tuple(z.shape)}")
        tiled = self.use_tiling and max(z.shape[2:]) > self.tile_latent_min_size
        if tiled or (self.use_slicing and z.shape[0] > 1):
            return self.decode(z).sample
        return self._image_nhwc(z).permute(0, 3, 1, 2)

    # ---- tiling and slicing (diffusers 0.24: enable_tiling / enable_slicing, tiled_encode / tiled_decode)
    def enable_tiling(self, use_tiling=True):
        """encode / decode of an input with a side above tile_sample_min_size pixels / tile_latent_min_size latents run tile by tile."""
        self.use_tiling = bool(use_tiling)

    def disable_tiling(self):
        self.enable_tiling(False)

    def enable_slicing(self):
        """encode / decode of a batch run one image per encoder / decoder call (per-image arithmetic: the VAE never mixes samples)."""
        self.use_slicing = True

    def disable_slicing(self):
        self.use_slicing = False

    def set_tile_size(self, pixels):
        """Both tile sizes from one number of image pixels: tile_sample_min_size = pixels, tile_latent_min_size = pixels / f.  A multiple of 4 f
        (32 for the 8x VAE), so that the overlap and the blend extent are whole latents."""
        f = 2 ** (len(self.config.block_out_channels) - 1)
        if isinstance(pixels, bool) or not isinstance(pixels, int) or pixels < 4 * f or pixels % (4 * f):
            raise ValueError(f"AutoencoderKL: the tile size must be a positive multiple of {4 * f} image pixels, got {pixels!r}")
        self.tile_sample_min_size, self.tile_latent_min_size = pixels, pixels // f

    def tile_grid(self, n_rows, n_cols, encode):
        """The tile geometry of tiled_encode (an image of n_rows x n_cols pixels) or tiled_decode (latents): (rows, cols, extent), rows / cols
        lists of (start, size, out_start, keep) per tile along the axis -- the tile reads input [start, start + size), its output is
        blended over `extent` output elements with the tile before it and its first `keep` output elements land at out_start.
        Tiles start every overlap = int(tile (1 - tile_overlap_factor)) inputs and are `tile` long, shorter at the far edge; extent =
        int(out_tile tile_overlap_factor) and keep <= limit = out_tile - extent, out_tile the other space's tile size (diffusers 0.24).
        ValueError for a grid the operators cannot run, naming the first such tile and input sizes that work: an image tile's sides must be
        multiples of f = 8 and every tile's latent map h x w a multiple of 8 tokens (the mid-block attention's row softmax and GEMMs; the
        convolutions and GroupNorms take any non-empty map, down to 1 x 1), and the kept parts must fill the output exactly."""
        f = 2 ** (len(self.config.block_out_channels) - 1)
        tile, out_tile = (self.tile_sample_min_size, self.tile_latent_min_size) if encode else (self.tile_latent_min_size, self.tile_sample_min_size)
        what = "tiled_encode" if encode else "tiled_decode"
        fac = self.tile_overlap_factor
        if not (isinstance(tile, int) and isinstance(out_tile, int) and tile > 0 and out_tile > 0 and 0.0 <= fac < 1.0):
            raise ValueError(f"AutoencoderKL.{what}: tile sizes must be positive integers and tile_overlap_factor in [0, 1), got "
                             f"{self.tile_sample_min_size!r}, {self.tile_latent_min_size!r}, {fac!r}")
        overlap, extent = int(tile * (1 - fac)), int(out_tile * fac)
        limit = out_tile - extent
        if overlap < 1 or (limit * f != overlap if encode else overlap * f != limit):
            raise ValueError(f"AutoencoderKL.{what}: tile_sample_min_size {self.tile_sample_min_size}, tile_latent_min_size {self.tile_latent_min_size} and "
                             f"tile_overlap_factor {fac} do not agree (a tile step of {overlap} against a kept part of {limit}, factor {f}); "
                             f"set_tile_size(a multiple of {4 * f}) gives sizes that do")

        def axis(n):
            out, tiles = 0, []
            for start in range(0, n, overlap):
                size = min(tile, n - start)
                keep = min(limit, size // f if encode else size * f)
                tiles.append((start, size, out, keep))
                out += keep
            return tiles

        def bad(rows, cols):
            for i, (_, th, _, _) in enumerate(rows):
                for j, (_, tw, _, _) in enumerate(cols):
                    if encode and (th % f or tw % f):
                        return i, j, th, tw, f"its sides must be multiples of {f}"
                    lh, lw = (th // f, tw // f) if encode else (th, tw)
                    if lh < 1 or lw < 1 or (lh * lw) % 8:
                        return i, j, th, tw, f"its {lh} x {lw} latent map must be a multiple of 8 tokens"
            return None

        rows, cols = axis(n_rows), axis(n_cols)
        first = bad(rows, cols)
        if first is not None:
            i, j, th, tw, why = first
            step = f if encode else 1
            near = lambda n, ok: [m for m in (next((m for m in range(n, 0, -step) if ok(m)), None),
                                               next((m for m in range(n, n + 2 * tile + 1, step) if ok(m)), None)) if m is not None]
            good_r = near(n_rows, lambda m: bad(axis(m), cols) is None)
            good_c = near(n_cols, lambda m: bad(rows, axis(m)) is None)
            unit = "pixels" if encode else "latents"
            raise ValueError(f"AutoencoderKL.{what}: tile (row {i}, column {j}) of the {n_rows} x {n_cols} input is {th} x {tw} {unit}: {why}.  "
                             f"With {n_cols} columns, {good_r or 'no nearby number of'} rows work; with {n_rows} rows, {good_c or 'no nearby number of'} "
                             f"columns work (tiles of {tile} every {overlap} {unit}).")
        return rows, cols, extent

    def _tiled(self, x, out, encode):
        """x -> out tile by tile.  Alive at any time: the row of blended tiles above (one entry per column, replaced as the row below is
        made) -- its entry to the left of the current tile is the left neighbour."""
        rows, cols, extent = self.tile_grid(x.shape[2], x.shape[3], encode)
        c = out.shape[1]
        line = [None] * len(cols)
        for i, (y0, th, oy, kh) in enumerate(rows):
            for j, (x0, tw, ox, kw) in enumerate(cols):
                view = x[:, :, y0:y0 + th, x0:x0 + tw]
                cur = self._moments_nhwc(view) if encode else self._image_nhwc(view)
                ops.tile_blend(cur, out[:, :, oy:oy + kh, ox:ox + kw], c, above=line[j] if i else None, left=line[j - 1] if j else None,
                               extent=(extent, extent))
                line[j] = cur

    @torch.no_grad()
    def tiled_encode(self, x, return_dict=True):
        """encode tile by tile, whatever the size of x (diffusers' tiled_encode): the blend runs on the 2z moments."""
        if x.dim() != 4 or x.shape[2] % 8 or x.shape[3] % 8:
            raise ValueError(f"AutoencoderKL.tiled_encode expects (B, C, H, W) with H, W multiples of 8, got {tuple(x.shape)}")
        B, C, H, W = x.shape
        rows, cols, _ = self.tile_grid(H, W, encode=True)
        moments = torch.empty((B, 2 * self.zc, rows[-1][2] + rows[-1][3], cols[-1][2] + cols[-1][3]), device=x.device, dtype=self._out_dtype(x))
        self._run(x, moments, True, True)
        out = SimpleNamespace(latent_dist=DiagonalGaussian(moments))
        return out if return_dict else (out.latent_dist,)

    @torch.no_grad()
    def tiled_decode(self, z, return_dict=True):
        """decode tile by tile, whatever the size of z (diffusers' tiled_decode)."""
        if z.dim() != 4 or z.shape[1] != self.zc:
            raise ValueError(f"AutoencoderKL.tiled_decode expects (B, {self.zc}, h, w), got {tuple(z.shape)}")
        rows, cols, _ = self.tile_grid(z.shape[2], z.shape[3], encode=False)
        img = torch.empty((z.shape[0], self.config.out_channels, rows[-1][2] + rows[-1][3], cols[-1][2] + cols[-1][3]), device=z.device,
                          dtype=self._out_dtype(z))
        self._run(z, img, False, True)
        out = SimpleNamespace(sample=img)
        return out if return_dict else (img,)

    def forward(self, sample, sample_posterior=False, generator=None):
        post = self.encode(sample).latent_dist
        return self.decode(post.sample(generator) if sample_posterior else post.mode())

    # ---- checkpoint loading (diffusers layout; the published sd-vae-ft-mse file uses the legacy attention names)
    LEGACY = {".query.": ".to_q.", ".key.": ".to_k.", ".value.": ".to_v.", ".proj_attn.": ".to_out.0."}

    @classmethod
    def convert_legacy_keys(cls, sd):
        out = {}
        for k, v in sd.items():
            for a, b in cls.LEGACY.items():
                if ".attentions." in k and a in k:
                    k = k.replace(a, b)
                    if v.dim() == 4:
                        v = v.reshape(v.shape[0], v.shape[1])
            out[k] = v
        return out

    @classmethod
    def from_pretrained(cls, pretrained_model_path, subfolder=None, **kw):
        path = os.path.join(pretrained_model_path, subfolder) if subfolder else str(pretrained_model_path)
        cfg_file = os.path.join(path, "config.json")
        if not os.path.isfile(cfg_file):
            raise RuntimeError(f"{cfg_file} does not exist or is not a file")
        cfg = {k: v for k, v in json.load(open(cfg_file)).items() if not k.startswith("_")}
        model = cls(**cfg)
        st = os.path.join(path, "diffusion_pytorch_model.safetensors")
        bn = os.path.join(path, "diffusion_pytorch_model.bin")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st, device="cpu")
        elif os.path.exists(bn):
            sd = torch.load(bn, map_location="cpu", weights_only=True)
        else:
            raise FileNotFoundError(f"no weights file found in {path}")
        model.load_state_dict(cls.convert_legacy_keys(sd), strict=True)
        return model
