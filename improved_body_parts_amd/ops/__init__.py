"""Operator layer: every hot op of the framework goes through here.

Two backends:

  * ``hip``   — hand-written CDNA4 (gfx950) kernels in ``csrc/`` compiled into the
    in-tree extension ``_ibp_hip``: MFMA implicit-GEMM convolution (fwd/dgrad/wgrad,
    NHWC bf16), fused BN+LeakyReLU, fused pool/upsample, fused SE, fused focal-L2
    loss fwd+bwd, fused multi-tensor SGD, on-device heatmap GT generation and
    keypoint post-processing. This is THE compute path on MI355X.
  * ``eager`` — plain PyTorch composition. Used on CPU (tests, plumbing config)
    and as the fp32 numerics oracle each kernel is validated against.

Policy: on a CUDA (ROCm) device the HIP extension is REQUIRED — a missing
extension raises rather than silently falling back (set ``IBP_AMD_ALLOW_EAGER=1``
to override for debugging). This replaces the reference's reliance on
cuDNN/Apex with first-party kernels.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import _backend
from ._backend import (
    hip_available,
    hip_extension,
    require_hip,
    use_hip_for,
)

LEAKY_SLOPE = 0.01


# ---------------------------------------------------------------------------
# conv + bn + activation
# ---------------------------------------------------------------------------

def conv_bn_act(x, conv, bn, act: bool, training: bool,
                residual_post=None, residual_post2=None):
    """conv -> (bn) -> (leaky_relu) (+ residual_post [+ residual_post2]).
    ``conv``/``bn`` are the parameter-holding nn.Conv2d / nn.BatchNorm2d
    modules (or bn None). The post-act residuals ride the conv epilogue on
    the HIP inference path (hourglass skip join, feature-cache add)."""
    if use_hip_for(x):
        from . import conv as _conv
        return _conv.conv_bn_act_hip(x, conv, bn, act=act, residual=None,
                                     training=training,
                                     residual_post=residual_post,
                                     residual_post2=residual_post2)
    y = conv(x)
    if bn is not None:
        y = bn(y)
    if act:
        y = F.leaky_relu(y, LEAKY_SLOPE, inplace=True)
    if residual_post is not None:
        y = y + residual_post
    if residual_post2 is not None:
        y = y + residual_post2
    return y


def upsample_conv_bn_act(low, conv, bn, act: bool, residual_post=None,
                         residual_post2=None, training: bool = False):
    """``conv_bn_act(upsample2x_nearest(low), ...)`` — the hourglass refine
    layer. On the HIP bf16 inference path an eligible 3x3 conv runs as four
    2x2 convs over ``low`` itself, one per output parity, and the upsampled
    map is never written (see ``conv.upsample_conv_bn_act_hip``; switch off
    with ``IBP_UPCONV_FOLD=0``). Elsewhere it is the two calls."""
    if use_hip_for(low):
        from . import conv as _conv
        return _conv.upsample_conv_bn_act_hip(
            low, conv, bn, act=act, training=training,
            residual_post=residual_post, residual_post2=residual_post2)
    return conv_bn_act(upsample2x_nearest(low), conv, bn, act=act,
                       training=training, residual_post=residual_post,
                       residual_post2=residual_post2)


def conv_bn_add_act(x, conv, bn, residual, act: bool, training: bool,
                    residual_post=None):
    """conv -> (bn) -> += residual -> (leaky_relu); the fused tail of a Residual block."""
    if use_hip_for(x):
        from . import conv as _conv
        return _conv.conv_bn_act_hip(x, conv, bn, act=act, residual=residual,
                                     training=training,
                                     residual_post=residual_post)
    y = conv(x)
    if bn is not None:
        y = bn(y)
    y = y + residual
    if act:
        y = F.leaky_relu(y, LEAKY_SLOPE, inplace=True)
    if residual_post is not None:
        y = y + residual_post
    return y


def conv_bn_add_conv_bn_act(y, conv_a, bn_a, x, conv_b, bn_b, act: bool,
                            training: bool):
    """``conv_bn_add_act(y, conv_a, bn_a, conv_bn_act(x, conv_b, bn_b,
    act=False), act)`` — a Residual block's last conv with its projection
    shortcut. On the HIP bf16 inference path two plain 1x1 convs run as one
    conv over K = Ca + Cb that reads both inputs, and the shortcut's output
    is never written (see ``conv.conv_bn_add_conv_bn_act_hip``; switch off
    with ``IBP_SKIP_FOLD=0``). Elsewhere it is the two calls."""
    if use_hip_for(y):
        from . import conv as _conv
        return _conv.conv_bn_add_conv_bn_act_hip(
            y, conv_a, bn_a, x, conv_b, bn_b, act=act, training=training)
    residual = conv_bn_act(x, conv_b, bn_b, act=False, training=training)
    return conv_bn_add_act(y, conv_a, bn_a, residual, act=act,
                           training=training)


def conv_bn_act_group(items):
    """Several INDEPENDENT :func:`conv_bn_act` / :func:`conv_bn_add_act`
    calls — ``items`` is a list of dicts with keys ``x conv bn act`` and
    optionally ``residual residual_post residual_post2 training`` — returning
    their outputs in order. On the HIP bf16 inference path the members share
    one grouped kernel launch per 8 (see ``conv.conv_bn_act_group_hip``);
    elsewhere they run one by one. Results never depend on the grouping."""
    if items and all(use_hip_for(it["x"]) for it in items):
        from . import conv as _conv
        return _conv.conv_bn_act_group_hip(items)
    out = []
    for it in items:
        if it.get("residual") is not None:
            y = conv_bn_add_act(
                it["x"], it["conv"], it["bn"], it["residual"], act=it["act"],
                training=it.get("training", False),
                residual_post=it.get("residual_post"))
            if it.get("residual_post2") is not None:
                y = y + it["residual_post2"]
            out.append(y)
        else:
            out.append(conv_bn_act(
                it["x"], it["conv"], it["bn"], act=it["act"],
                training=it.get("training", False),
                residual_post=it.get("residual_post"),
                residual_post2=it.get("residual_post2")))
    return out


def grouped_heads_enabled(x) -> bool:
    """True when the per-scale head layers may be issued as grouped launches:
    HIP backend, bf16, grad disabled, ``IBP_CONV_GROUP`` not ``0`` (read at
    call time)."""
    if not (use_hip_for(x) and x.dtype == torch.bfloat16
            and not torch.is_grad_enabled()):
        return False
    from . import conv as _conv
    return _conv.conv_group_enabled()


# ---------------------------------------------------------------------------
# pooling / upsampling / concat
# ---------------------------------------------------------------------------

def maxpool2x2(x):
    if use_hip_for(x):
        from . import spatial
        return spatial.maxpool2x2_hip(x)
    return F.max_pool2d(x, 2, 2)


def upsample2x_nearest(x):
    if use_hip_for(x):
        from . import spatial
        return spatial.upsample2x_hip(x)
    return F.interpolate(x, scale_factor=2, mode="nearest")


def channel_concat(a, b):
    if a.is_cuda:
        return torch.cat([a, b], dim=1).contiguous(memory_format=torch.channels_last)
    return torch.cat([a, b], dim=1)


# ---------------------------------------------------------------------------
# squeeze-excitation
# ---------------------------------------------------------------------------

def se_layer(x, fc1, fc2):
    """Global-avg-pool -> fc1 -> leaky_relu -> fc2 -> sigmoid -> channel scale."""
    if use_hip_for(x):
        from . import spatial
        return spatial.se_layer_hip(x, fc1, fc2)
    n, c = x.shape[:2]
    y = x.float().mean(dim=(2, 3))
    y = F.leaky_relu(fc1(y.to(x.dtype)), LEAKY_SLOPE)
    y = torch.sigmoid(fc2(y))
    return x * y.view(n, c, 1, 1)


def se_layer_group(items):
    """:func:`se_layer` over independent maps — ``items`` is a list of
    ``(x, fc1, fc2)``; one grouped launch per SE stage on the HIP inference
    path, per-member calls elsewhere."""
    if items and all(use_hip_for(x) for x, _, _ in items):
        from . import spatial
        return spatial.se_layer_group_hip(items)
    return [se_layer(x, fc1, fc2) for x, fc1, fc2 in items]


# ---------------------------------------------------------------------------
# focal L2 loss (fused fwd/bwd on HIP)
# ---------------------------------------------------------------------------

def focal_l2_loss(pred, gt, mask, *, heat_start, bkg_start, gamma=1,
                  multi_task_weight=0.1, keypoint_task_weight=3.0,
                  nstack_weight=(1, 1, 1, 1), alpha=0.0, beta=0.0):
    """Focal L2 over (nstack, N, C, H, W) predictions.

    ``gt`` (N, C, H0, W0) and ``mask`` (N, 1, H0, W0) may be at an integer
    multiple of the prediction resolution: the HIP kernel average-pools GT
    windows and bilinearly samples mask_miss ON THE FLY (the supervision
    pyramid never materialises — reference loss_model.py:52-56 builds it
    per scale with adaptive_avg_pool2d / interpolate). Mask semantics
    everywhere: bilinear value kept where >= 0.5, else 0. Per-channel task
    weights: person-mask channel (C-2) gets multi_task_weight, keypoint
    channels [heat_start, bkg_start) get keypoint_task_weight
    (reference loss_model.py:146-156).
    """
    if use_hip_for(pred):
        from . import loss as _loss
        h0, w0 = gt.shape[-2:]
        h, w = pred.shape[-2:]
        if h0 % h or w0 % w or h0 // h != w0 // w:
            # non-integer pyramid ratio (odd input sizes): pre-pool eagerly,
            # kernel runs with r = 1
            gt = F.adaptive_avg_pool2d(gt.float(), (h, w)).to(pred.dtype)
            m = F.interpolate(mask.float(), size=(h, w), mode="bilinear",
                              align_corners=False)
            mask = ((m >= 0.5).float() * m).to(pred.dtype)
        # the kernels read gt and mask with pred's element type
        if gt.dtype != pred.dtype:
            gt = gt.to(pred.dtype)
        if mask.dtype != pred.dtype:
            mask = mask.to(pred.dtype)
        return _loss.focal_l2_loss_hip(pred, gt, mask, heat_start=heat_start,
                                       bkg_start=bkg_start, gamma=gamma,
                                       multi_task_weight=multi_task_weight,
                                       keypoint_task_weight=keypoint_task_weight,
                                       nstack_weight=nstack_weight,
                                       alpha=alpha, beta=beta)
    nstack = pred.shape[0]
    C = pred.shape[2]
    size = pred.shape[-2:]
    if gt.shape[-2:] != size:
        gt = F.adaptive_avg_pool2d(gt.float(), size).to(pred.dtype)
    m = mask.float()
    if m.shape[-2:] != size:
        m = F.interpolate(m, size=size, mode="bilinear", align_corners=False)
    mask = ((m >= 0.5).float() * m).to(pred.dtype)
    cw = torch.ones(C, dtype=pred.dtype, device=pred.device)
    cw[heat_start:bkg_start] = keypoint_task_weight
    cw[C - 2] = multi_task_weight
    gt_b = gt.unsqueeze(0)
    mask_b = (mask.unsqueeze(0) * cw.view(1, 1, C, 1, 1))
    st = torch.where(gt_b >= 0.01, pred - alpha, 1.0 - pred - beta)
    if gamma == 1:
        factor = torch.abs(1.0 - st)
    else:
        factor = (1.0 - st) ** gamma
    out = (pred - gt_b) ** 2 * factor * mask_b
    loss_nstack = out.sum(dim=(1, 2, 3, 4))
    w = [loss_nstack[i] * nstack_weight[i] for i in range(nstack)]
    return sum(w) / sum(nstack_weight)
