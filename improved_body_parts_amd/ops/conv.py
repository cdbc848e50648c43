"""Fused conv + BatchNorm + LeakyReLU (+ residual) on the HIP path.

The convolution itself goes through :mod:`.conv_kernels` (hand-written MFMA
implicit-GEMM for the supported shapes); BN statistics, the scale/shift+act
epilogue and the whole BN backward run as the fused CDNA4 kernels of
bn_act.hip. Tensors stay NHWC (torch channels_last) end to end.

Replaces: nn.Conv2d -> nn.BatchNorm2d -> nn.LeakyReLU chains
(reference models/layers_transposed.py:90-120) and their autograd.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import conv_kernels
from ._backend import hip_extension
from ._cache import versioned

LEAKY_SLOPE = 0.01
_CL = torch.channels_last


def _to_cl(t):
    return t.contiguous(memory_format=_CL)


def _conv_forward(x, weight, bias, stride, padding, dilation):
    """Convolution forward dispatch: MFMA implicit-GEMM kernel when the shape is
    supported, library fallback otherwise (first iterations / odd shapes)."""
    y = conv_kernels.conv_fwd(x, weight, stride, padding, dilation)
    if y is None:
        y = F.conv2d(x, weight, None, stride, padding, dilation)
        y = _to_cl(y)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return y


def _conv_dgrad(dy, weight, x_shape, stride, padding, dilation):
    dx = conv_kernels.conv_dgrad(dy, weight, x_shape, stride, padding, dilation)
    if dx is None:
        dx = torch.nn.grad.conv2d_input(x_shape, weight, dy, stride, padding,
                                        dilation)
        dx = _to_cl(dx)
    return dx


def _conv_wgrad(x, dy, w_shape, stride, padding, dilation):
    dw = conv_kernels.conv_wgrad(x, dy, w_shape, stride, padding, dilation)
    if dw is None:
        dw = torch.nn.grad.conv2d_weight(x, w_shape, dy, stride, padding,
                                         dilation)
    return dw


def _on_inference_path(x, bn, training):
    """The bf16 inference path (the conv kernel's epilogue does the whole
    module): bf16 input, BN (if any) in eval mode, grad disabled — read here,
    outside ``Function.apply``; inside ``forward`` it is always off."""
    return not _bn_training(bn, training) and not torch.is_grad_enabled() \
        and x.dtype == torch.bfloat16


def _bn_training(bn, training):
    return training and bn is not None and bn.training


def _inference_epilogue(conv, bn):
    """(scale, shift) of the conv kernel's fused epilogue on the inference
    path: the folded eval-mode BN, else the bias-only pair (ones, bias), else
    (None, None). Cached against parameter versions (``bn.bias`` is not in the
    key): fresh tensors per call were ~60 fill/copy launches per step."""
    gamma = bn.weight if bn is not None else None
    if gamma is not None:
        # owned by the module's own running_var, so one entry per BN module
        var = bn.running_var
        return versioned(var, "bn-fold",
                         (gamma._version, bn.running_mean._version,
                          var._version), _fold_bn, bn)
    bias = conv.bias
    if bias is not None:
        return versioned(bias, "bias-fold", (bias._version,), _fold_bias, bias)
    return None, None


def _fold_bn(_, bn):
    invstd = torch.rsqrt(bn.running_var.float() + bn.eps)
    scale = bn.weight.float() * invstd
    return scale, bn.bias.float() - bn.running_mean.float() * scale


def _fold_bias(_, bias):
    return (torch.ones(bias.shape[0], device=bias.device, dtype=torch.float32),
            bias.detach().float())


def _tick_running_stats(bn_mod):
    """The finalize kernel updates running stats in place without going
    through ATen — tick their version counters so the eval-path folded-BN
    cache (keyed on them) does not serve stale scale/shift."""
    torch.autograd.graph.increment_version(bn_mod.running_mean)
    torch.autograd.graph.increment_version(bn_mod.running_var)


class ConvBnActFn(torch.autograd.Function):
    """y = leaky( bn( conv(x, w) ) (+ residual) ) (+ residual_post [+2]),
    all fused on device. ``residual`` joins BEFORE the activation (bottleneck
    skip); ``residual_post``/``residual_post2`` join AFTER it (hourglass
    up1+deconv1, cross-stack feature-cache) — their backward is identity."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, residual,
                residual_post, residual_post2,
                stride, padding, dilation, act, training, bn_mod, inference):
        ext = hip_extension()
        x = _to_cl(x)

        # inference fast path: fold BN into the conv epilogue -> ONE kernel.
        # `inference`, decided OUTSIDE apply(): None or the (scale, shift)
        if inference is not None:
            scale, shift = inference
            if scale is not None or act or residual is not None \
                    or residual_post is not None:
                y = conv_kernels.conv_fwd(x, weight, stride, padding, dilation,
                                          scale=scale, shift=shift,
                                          residual=residual, act=act,
                                          residual_post=residual_post,
                                          residual_post2=residual_post2)
                if y is not None:
                    ctx.conf = None
                    return y

        y_conv = _conv_forward(x, weight, bias if gamma is None else None,
                               stride, padding, dilation)
        C = y_conv.shape[1]

        sync_group, sync_world = _sync_info(bn_mod, training)
        if gamma is not None:
            if training:
                mom = bn_mod.momentum if bn_mod.momentum is not None else 0.1
                if sync_world > 1:
                    # SyncBN: all-reduce (sums, sumsq) so the fused path keeps
                    # cross-rank statistics (module forward is bypassed here)
                    import torch.distributed as dist
                    sums, sumsq = ext.bn_stats(y_conv, C)
                    flat = torch.cat([sums, sumsq])
                    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=sync_group)
                    M = (y_conv.numel() // C) * sync_world
                    mean, invstd, scale, shift = ext.bn_finalize(
                        flat[:C], flat[C:], M, gamma.float(), beta.float(),
                        bn_mod.running_mean, bn_mod.running_var,
                        bn_mod.num_batches_tracked, mom, bn_mod.eps)
                    _tick_running_stats(bn_mod)
                else:
                    # single fused kernel chain: stats + colsum + per-channel
                    # epilogue + running-stat update (the Python mean/var/rsqrt
                    # chain was ~6 tiny launches per conv layer)
                    mean, invstd, scale, shift = ext.bn_stats_finalize(
                        y_conv, C, gamma.float(), beta.float(),
                        bn_mod.running_mean, bn_mod.running_var,
                        bn_mod.num_batches_tracked, mom, bn_mod.eps)
                    _tick_running_stats(bn_mod)
            else:
                mean = bn_mod.running_mean.float()
                var = bn_mod.running_var.float()
                invstd = torch.rsqrt(var + bn_mod.eps)
                scale = (gamma.float() * invstd)
                shift = (beta.float() - mean * scale)
        elif act or residual is not None:
            mean = invstd = None
            scale = torch.ones(C, device=x.device, dtype=torch.float32)
            shift = torch.zeros(C, device=x.device, dtype=torch.float32)
        else:
            # plain conv (the 1x1 heads): no epilogue pass needed
            mean = invstd = scale = shift = None

        if scale is not None:
            res_cl = _to_cl(residual) if residual is not None else None
            y = ext.bn_act_fwd(y_conv, scale, shift, res_cl, LEAKY_SLOPE, act)
        else:
            y = y_conv

        # y (pre post-add) is what backward needs to reconstruct the act region
        ctx.save_for_backward(x, weight, gamma, y_conv, y, mean, invstd)
        ctx.conf = (stride, padding, dilation, act, training,
                    residual is not None, bias is not None and gamma is None,
                    residual_post is not None, residual_post2 is not None)
        ctx.sync = (sync_group, sync_world)
        if residual_post is not None:
            y = y + _to_cl(residual_post)
        if residual_post2 is not None:
            y = y + _to_cl(residual_post2)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = hip_extension()
        x, weight, gamma, y_conv, y, mean, invstd = ctx.saved_tensors
        (stride, padding, dilation, act, training, has_res, has_bias,
         has_post, has_post2) = ctx.conf
        C = y_conv.shape[1]
        dy = _to_cl(dy)
        has_bn = gamma is not None
        # post-act residuals are pure adds: their gradient is dy itself
        dpost = dy if has_post else None
        dpost2 = dy if has_post2 else None

        if not has_bn and not act and not has_res and not has_bias:
            # plain conv fast path (the 1x1 heads without bias)
            dx = _conv_dgrad(dy, weight, x.shape, stride, padding, dilation) \
                if ctx.needs_input_grad[0] else None
            dw = _conv_wgrad(x, dy, weight.shape, stride, padding, dilation) \
                if ctx.needs_input_grad[1] else None
            return (dx, dw, None, None, None, None, dpost, dpost2,
                    None, None, None, None, None, None, None)

        dpre, sum_dpre, sum_dxhat = ext.bn_act_bwd(
            dy, y, y_conv, mean if has_bn else None, invstd if has_bn else None,
            LEAKY_SLOPE, act, has_bn, C)

        sync_group, sync_world = getattr(ctx, "sync", (None, 1))
        if has_bn and training and sync_world > 1:
            # SyncBN backward: dx needs GLOBAL sum_dpre/sum_dxhat over the
            # global count; averaging (sum / world) makes the local-M division
            # inside bn_act_bwd_apply equal the global-M division, and the
            # per-rank dgamma/dbeta then DDP-average to the correct value.
            import torch.distributed as dist
            flat = torch.cat([sum_dpre, sum_dxhat])
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=sync_group)
            flat = flat / sync_world
            sum_dpre, sum_dxhat = flat[:C], flat[C:]

        dres = dpre if has_res else None
        if has_bn:
            if training:
                dconv = ext.bn_act_bwd_apply(dpre, y_conv, mean, invstd,
                                             gamma.float(), sum_dpre, sum_dxhat, C)
            else:
                dconv = ext.bn_act_bwd_apply(dpre, y_conv, mean, invstd,
                                             gamma.float(), None, None, C)
            dgamma = sum_dxhat.to(gamma.dtype)
            dbeta = sum_dpre.to(gamma.dtype)
        else:
            dconv = dpre
            dgamma = dbeta = None

        dbias = sum_dpre.to(weight.dtype) if has_bias else None
        dx = _conv_dgrad(dconv, weight, x.shape, stride, padding, dilation) \
            if ctx.needs_input_grad[0] else None
        dw = _conv_wgrad(x, dconv, weight.shape, stride, padding, dilation) \
            if ctx.needs_input_grad[1] else None
        return (dx, dw, dbias, dgamma, dbeta, dres, dpost, dpost2,
                None, None, None, None, None, None, None)


def _sync_info(bn_mod, training):
    """(process_group, world_size) when bn_mod is a SyncBatchNorm2d in a
    multi-rank training run; (None, 1) otherwise."""
    if not training or bn_mod is None or not hasattr(bn_mod, "process_group"):
        return None, 1
    import torch.distributed as dist
    if not dist.is_initialized():
        return None, 1
    group = bn_mod.process_group
    world = dist.get_world_size(group)
    return group, world


def conv_bn_act_hip(x, conv, bn, act: bool, residual=None, training: bool = False,
                    residual_post=None, residual_post2=None):
    """Module-level entry used by models.layers: pulls parameters out of the
    nn.Conv2d / nn.BatchNorm2d containers and runs the fused function."""
    gamma = bn.weight if bn is not None else None
    beta = bn.bias if bn is not None else None
    bn_training = _bn_training(bn, training)
    inference = _inference_epilogue(conv, bn) \
        if _on_inference_path(x, bn, training) else None
    return ConvBnActFn.apply(
        x, conv.weight, conv.bias, gamma, beta, residual,
        residual_post, residual_post2,
        conv.stride, conv.padding, conv.dilation, act,
        bn_training, bn, inference)


def upconv_fold_enabled() -> bool:
    """``IBP_UPCONV_FOLD=0`` (read at call time) restores the separate
    upsample kernel and the 3x3 conv over the upsampled map for A/B runs."""
    return os.environ.get("IBP_UPCONV_FOLD", "1") != "0"


def upsample_conv_bn_act_hip(low, conv, bn, act: bool, training: bool = False,
                             residual_post=None, residual_post2=None):
    """``conv_bn_act_hip(upsample2x_nearest(low), ...)``. On the bf16
    inference path (grad disabled, BN in eval mode) a 3x3 stride-1 pad-1 conv
    with Cin % 64 == 0 and Cout % 8 == 0 runs as four parity 2x2 convs over
    ``low`` itself (``conv_kernels.upfold_fwd``); everything else runs the
    upsample kernel and the conv as two calls."""
    if _on_inference_path(low, bn, training) and upconv_fold_enabled():
        if conv_kernels.upfold_supported(low, conv.weight, conv.stride,
                                         conv.padding, conv.dilation):
            scale, shift = _inference_epilogue(conv, bn)
            return conv_kernels.upfold_fwd(
                _to_cl(low), conv.weight, scale=scale, shift=shift, act=act,
                residual_post=residual_post, residual_post2=residual_post2)
    from . import spatial
    return conv_bn_act_hip(spatial.upsample2x_hip(low), conv, bn, act=act,
                           training=training, residual_post=residual_post,
                           residual_post2=residual_post2)


def skip_fold_enabled() -> bool:
    """``IBP_SKIP_FOLD=0`` (read at call time) restores the projection
    shortcut as a conv of its own for A/B runs."""
    return os.environ.get("IBP_SKIP_FOLD", "1") != "0"


def _branch_fold(conv, bn):
    """(scale, shift) of one branch, computed afresh: eval-mode BN fold, else
    (None, bias), else (None, None)."""
    if bn is not None and bn.weight is not None:
        return _fold_bn(None, bn)
    return None, (conv.bias.detach().float() if conv.bias is not None else None)


def _fold_versions(conv, bn):
    if bn is not None and bn.weight is not None:
        return (conv.weight._version, bn.weight._version, bn.bias._version,
                bn.running_mean._version, bn.running_var._version)
    bias = conv.bias
    return (conv.weight._version, bias._version if bias is not None else -1)


def cat_fold(conv_a, bn_a, conv_b, bn_b):
    """``(pack, ones, shift)`` of the two-source conv that computes
    ``bn_a(conv_a(.)) + bn_b(conv_b(.))`` in eval mode: both folded scales
    ride the weight rows, the shifts add up. One pack launch per version of
    anything that enters either fold — both weights, each BN's weight, bias,
    running mean and running var, or the conv bias without BN. Cached on the
    first conv's weight, one entry per partner."""
    wb = conv_b.weight
    return versioned(conv_a.weight, ("cat", id(wb), id(bn_a), id(bn_b)),
                     _fold_versions(conv_a, bn_a) + _fold_versions(conv_b, bn_b),
                     _cat_build, conv_a, bn_a, conv_b, bn_b)[0]


def _cat_build(prev, conv_a, bn_a, conv_b, bn_b):
    scale_a, shift_a = _branch_fold(conv_a, bn_a)
    scale_b, shift_b = _branch_fold(conv_b, bn_b)
    packed = conv_kernels.cat_pack(prev[0] if prev is not None else None,
                                   conv_a.weight, conv_b.weight, scale_a,
                                   scale_b, shift_a, shift_b)
    # the partners stay alive with the entry, so their ids (in the tag)
    # cannot be handed to other objects
    return packed, (conv_b.weight, bn_a, bn_b)


def _plain_1x1(conv):
    return (conv.kernel_size == (1, 1) and conv.stride == (1, 1)
            and conv.padding == (0, 0) and conv.dilation == (1, 1)
            and conv.groups == 1)


def conv_bn_add_conv_bn_act_hip(y, conv_a, bn_a, x, conv_b, bn_b, act: bool,
                                training: bool = False):
    """``act(bn_a(conv_a(y)) + bn_b(conv_b(x)))`` — the tail of a Residual
    block with a projection shortcut. On the bf16 inference path (grad
    disabled, both BNs in eval mode) two plain 1x1 convs with equal Cout and
    ``conv_a.in_channels % 64 == 0`` run as ONE conv over both inputs
    (``conv_kernels.conv_cat_fwd``); everything else runs the two calls:
    ``conv_b`` on its own, its output the pre-act residual of ``conv_a``."""
    if skip_fold_enabled() and _on_inference_path(y, bn_a, training) \
            and _on_inference_path(x, bn_b, training) \
            and _plain_1x1(conv_a) and _plain_1x1(conv_b) \
            and conv_kernels.cat_supported(y, conv_a.weight, x, conv_b.weight):
        pack, ones, shift = cat_fold(conv_a, bn_a, conv_b, bn_b)
        return conv_kernels.conv_cat_fwd(y, conv_a.weight, x, conv_b.weight,
                                         pack, scale=ones, shift=shift,
                                         act=act)
    residual = conv_bn_act_hip(x, conv_b, bn_b, act=False, training=training)
    return conv_bn_act_hip(y, conv_a, bn_a, act=act, residual=residual,
                           training=training)


def conv_group_enabled() -> bool:
    """``IBP_CONV_GROUP=0`` (read at call time) restores one launch per conv
    for A/B runs."""
    return os.environ.get("IBP_CONV_GROUP", "1") != "0"


def conv_bn_act_group_hip(items):
    """Independent Conv(+BN)(+LeakyReLU)(+residuals) modules in one grouped
    launch per 8 members. ``items`` is a list of dicts with keys ``x conv bn
    act`` and optionally ``residual residual_post residual_post2 training``.

    Only the bf16 inference fast path is grouped (grad disabled, BN in eval
    mode, every member inside the MFMA envelope); otherwise every member goes
    through :func:`conv_bn_act_hip` on its own. Outputs are bit-identical
    either way: a grouped member runs the plan it would get alone."""
    if len(items) > 1 and conv_group_enabled() and all(
            _on_inference_path(it["x"], it["bn"], it.get("training", False))
            for it in items):
        members = []
        for it in items:
            conv = it["conv"]
            scale, shift = _inference_epilogue(conv, it["bn"])
            members.append(dict(
                x=_to_cl(it["x"]), weight=conv.weight, stride=conv.stride,
                padding=conv.padding, dilation=conv.dilation, scale=scale,
                shift=shift, residual=it.get("residual"), act=it["act"],
                residual_post=it.get("residual_post"),
                residual_post2=it.get("residual_post2")))
        ys = conv_kernels.conv_fwd_group(members)
        if ys is not None:
            return ys
    return [conv_bn_act_hip(it["x"], it["conv"], it["bn"], it["act"],
                            residual=it.get("residual"),
                            training=it.get("training", False),
                            residual_post=it.get("residual_post"),
                            residual_post2=it.get("residual_post2"))
            for it in items]
