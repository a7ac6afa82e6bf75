"""TEST INFRASTRUCTURE: DeepCache (arXiv 2312.00858, the idea only) restated in fp32 from the block functions of oracle/cpu_ref.py, and the helpers
the DeepCache tests share.

The restatement walks the denoising UNet as flat lists -- the skip-producing operators of the down path in production order (conv_in is skip 0,
then every down layer and every downsampler) and the up layers in evaluation order -- and never looks at the product's code:
  full(...)     the whole UNet (oracle.cpu_ref.denoising_unet_forward, restated so that it can hand out what DeepCache keeps) -> (prediction,
                hidden), hidden[k] = the hidden state that meets skip k on the up path (what is concatenated in front of skip k)
  shallow(...)  a shallow evaluation of depth d on OTHER inputs: conv_in and the first d - 1 down operators on (x2, t2), then hidden[d - 1] of
                a full evaluation in place of everything deeper, then the last d up layers (and an upsampler where one lies between them),
                conv_norm_out, conv_out.
"""
import torch
import torch.nn.functional as F

from oracle import cpu_ref as O


def _down_ops(sd):
    out = []
    for i in range(O._n_levels(sd)):
        out += [("layer", i, 0), ("layer", i, 1)]
        if f"down_blocks.{i}.downsamplers.0.conv.weight" in sd:
            out.append(("down", i, None))
    return out


def _layer(sd, p, j, x, emb_f, ctx_f, bank, cfg, f, gf):
    x = O.resnet(sd, p + f"resnets.{j}.", x, emb_f, gn_frames=gf)
    if (p + "attentions.0.norm.weight") in sd:
        x = O.transformer_3d(sd, p + f"attentions.{j}.", x, ctx_f, bank(p + f"attentions.{j}."), cfg)
    if (p + f"motion_modules.{j}.temporal_transformer.norm.weight") in sd:
        x = O.motion_module(sd, p + f"motion_modules.{j}.", x, f)
    return x


def _walk(sd, sample, t, ctx, banks, cfg, depth=None, deep=None):
    nl = O._n_levels(sd)
    b, _, f, hh, ww = sample.shape
    gf = 1
    emb_f = O.time_embedding(sd, t, b).repeat_interleave(f, dim=0)
    ctx_f = ctx.repeat_interleave(f, dim=0)
    bank = (lambda p: banks.get(p + "transformer_blocks.0.")) if banks is not None else (lambda p: None)
    x = sample.permute(0, 2, 1, 3, 4).reshape(b * f, -1, hh, ww)
    x = F.conv2d(x, sd["conv_in.weight"], sd["conv_in.bias"], padding=1)
    skips = [x]
    ops = _down_ops(sd)
    for kind, i, j in ops if depth is None else ops[:depth - 1]:
        p = f"down_blocks.{i}."
        x = O.downsample(sd, p + "downsamplers.0.", x) if kind == "down" else _layer(sd, p, j, x, emb_f, ctx_f, bank, cfg, f, gf)
        skips.append(x)
    force_size = any(s_ % 2 ** (nl - 1) for s_ in (hh, ww))
    hidden = {}
    if depth is None:
        x = O.resnet(sd, "mid_block.resnets.0.", x, emb_f, gn_frames=gf)
        x = O.transformer_3d(sd, "mid_block.attentions.0.", x, ctx_f, bank("mid_block.attentions.0."), cfg)
        if "mid_block.motion_modules.0.temporal_transformer.norm.weight" in sd:
            x = O.motion_module(sd, "mid_block.motion_modules.0.", x, f)
        x = O.resnet(sd, "mid_block.resnets.1.", x, emb_f, gn_frames=gf)
    else:
        assert len(skips) == depth and deep.shape[2:] == skips[-1].shape[2:]
        x = deep
    ups = [(i, j) for i in range(nl) for j in range(3)]
    skipped = 0 if depth is None else len(ups) - depth
    for n, (i, j) in enumerate(ups):
        p = f"up_blocks.{i}."
        if n >= skipped:
            hidden[len(skips) - 1] = x
            x = torch.cat([x, skips.pop()], dim=1)
            x = _layer(sd, p, j, x, emb_f, ctx_f, bank, cfg, f, gf)
            if j == 2 and (p + "upsamplers.0.conv.weight") in sd:
                x = O.upsample(sd, p + "upsamplers.0.", x, skips[-1].shape[2:] if force_size else None)
    x = O.group_norm_frames(x, sd["conv_norm_out.weight"], sd["conv_norm_out.bias"], 1e-5, gf)
    x = F.conv2d(F.silu(x), sd["conv_out.weight"], sd["conv_out.bias"], padding=1)
    return x.reshape(b, f, -1, hh, ww).permute(0, 2, 1, 3, 4), hidden


def full(sd, sample, t, ctx, banks=None, cfg=True):
    return _walk(sd, sample, t, ctx, banks, cfg)


def shallow(sd, sample, t, ctx, banks, cfg, depth, deep):
    return _walk(sd, sample, t, ctx, banks, cfg, depth=depth, deep=deep)[0]


# ---- helpers shared by the CPU and the GPU tests
def call_nhwc(den, sample, t, emb, **kw):
    """UNet3DConditionModel.forward's packing round forward_nhwc, with forward_nhwc's keywords: sample (b, 4, f, h, w) fp16, emb (b, L, D) ->
    the prediction (b, 4, f, h, w) fp32 on the host."""
    from mikudance_amd import ops
    b, c, f, hh, ww = sample.shape
    st = sample.stride()
    x = ops.pack_nhwc(sample, b * f, f, (st[0], st[2], st[1], st[3], st[4]), 0, c, 64, hh, ww)
    cross = den._cross(emb, [i // f for i in range(b * f)], sample.device)
    pred = den.forward_nhwc(x, b, f, torch.full((b,), float(t)), cross, **kw)
    out = torch.empty((b, 4, f, hh, ww), device=sample.device, dtype=torch.float16)
    so = out.stride()
    ops.unpack_nhwc(pred.view(b * f, hh, ww, 4), out, b * f, f, (so[0], so[2], so[1], so[3], so[4]), 4, hh, ww)
    return out.float().cpu()


def write_banks(ref, den, rl, emb, f, h, w, device="cpu"):
    """One write pass of the reference UNet on both clip-halves -> (writer, reader) with the banks in the denoising UNet's blocks (clear both when
    done) -- the setting of tests/test_host_graph_cpu.py::_pair."""
    from mikudance_amd import ReferenceAttentionControl
    writer = ReferenceAttentionControl(ref, do_classifier_free_guidance=True, mode="write", batch_size=1, fusion_blocks="full")
    reader = ReferenceAttentionControl(den, do_classifier_free_guidance=True, mode="read", batch_size=1, fusion_blocks="full")
    g = rl.repeat(2, 1, 1, 1, 1).reshape(2 * f, 22, h, w).half().to(device)
    ref(g, torch.zeros((), dtype=torch.long), encoder_hidden_states=emb.repeat((f, 1, 1)).half().to(device), return_dict=False)
    reader.update(writer)
    return writer, reader


def oracle_banks(ref_sd, rl, emb, f, h, w):
    with torch.no_grad():
        g = rl.repeat(2, 1, 1, 1, 1).reshape(2 * f, 22, h, w)
        banks, _ = O.reference_unet_forward(ref_sd, g, emb.repeat((f, 1, 1)))
    return {k: v.half().float() for k, v in banks.items()}
