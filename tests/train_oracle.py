"""fp64 oracle for the training-step kernels ``conv_wgrad.hip``, ``loss.hip``
and ``sgd.hip``.

Plain torch in float64, on whatever device the inputs live on (the large
weight-gradient cases evaluate it on the GPU: any correct fp64 matmul of their
small integers is exact). Tensors are LOGICAL (NCHW); memory format does not
matter. ``test_train_oracle.py`` validates this file on the CPU against
``torch.nn.grad.conv2d_weight``, the eager focal loss through autograd and
``torch.optim.SGD``, all in fp64.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from bn_spatial_oracle import rne_bf16, bf16_ulp  # noqa: F401  (re-exported)

F64 = torch.float64


# ---------------------------------------------------------------------------
# convolution weight gradient
# ---------------------------------------------------------------------------

def wgrad(x, dy, w_shape, stride, pad, dil):
    """dW[co][ci][kh][kw] = sum over (n, ho, wo) of
    x[n][ci][ho*s - ph + kh*dh][wo*s - pw + kw*dw] * dy[n][co][ho][wo].

    One ``x_tap^T @ dy`` matmul per filter tap over the zero-padded input.
    ``x`` is [N, Cin, H, W], ``dy`` [N, Cout, Ho, Wo]; returns fp64
    [Cout, Cin, KH, KW] on the inputs' device."""
    cout, cin, kh, kw = w_shape
    x = x.detach().to(F64)
    dy = dy.detach().to(F64)
    n, _, ho, wo = dy.shape
    assert x.shape[1] == cin and dy.shape[1] == cout and x.shape[0] == n
    ph, pw = pad
    dh, dw_ = dil
    # pad far enough that every tap slice is in range whatever the geometry
    eh = max((ho - 1) * stride + (kh - 1) * dh + 1 - (x.shape[2] + ph), 0)
    ew = max((wo - 1) * stride + (kw - 1) * dw_ + 1 - (x.shape[3] + pw), 0)
    xp = F.pad(x, (pw, ew, ph, eh))
    dy_m = dy.permute(0, 2, 3, 1).reshape(n * ho * wo, cout)
    out = torch.empty(cout, cin, kh, kw, dtype=F64, device=x.device)
    for a in range(kh):
        for b in range(kw):
            tap = xp[:, :, a * dh: a * dh + (ho - 1) * stride + 1: stride,
                     b * dw_: b * dw_ + (wo - 1) * stride + 1: stride]
            tap_m = tap.permute(0, 2, 3, 1).reshape(n * ho * wo, cin)
            out[:, :, a, b] = (tap_m.t() @ dy_m).t()
    return out


def wgrad_abs(x, dy, w_shape, stride, pad, dil):
    """Sum of |addends| of every element of :func:`wgrad`."""
    return wgrad(x.detach().to(F64).abs(), dy.detach().to(F64).abs(),
                 w_shape, stride, pad, dil)


# ---------------------------------------------------------------------------
# focal L2 loss with the on-the-fly supervision pyramid
# ---------------------------------------------------------------------------

def _window_mean(gt, r):
    n, c, h0, w0 = gt.shape
    return gt.reshape(n, c, h0 // r, r, w0 // r, r).mean(dim=(3, 5))


def _bilinear_axis(size_out, r, size_in, device):
    """Source indices and weight of the upper neighbour along one axis for
    ``interpolate(..., mode='bilinear', align_corners=False)`` at an integer
    down-scale ``r`` (source coordinate (i + 1/2) r - 1/2, neighbours clamped
    into the map)."""
    src = (torch.arange(size_out, dtype=F64, device=device) + 0.5) * r - 0.5
    i0 = torch.floor(src)
    frac = src - i0
    i0 = i0.long()
    lo = i0.clamp(0, size_in - 1)
    hi = (i0 + 1).clamp(0, size_in - 1)
    return lo, hi, frac


def _mask_sample(mask, r):
    """Bilinear sample of the full-resolution mask at the low resolution, then
    the keep-value threshold: v where v >= 0.5, else 0."""
    n, one, h0, w0 = mask.shape
    if r == 1:
        v = mask
    else:
        ylo, yhi, fy = _bilinear_axis(h0 // r, r, h0, mask.device)
        xlo, xhi, fx = _bilinear_axis(w0 // r, r, w0, mask.device)
        top = mask[:, :, ylo, :]
        bot = mask[:, :, yhi, :]
        fx = fx.view(1, 1, 1, -1)
        fy = fy.view(1, 1, -1, 1)
        top = top[..., xlo] * (1 - fx) + top[..., xhi] * fx
        bot = bot[..., xlo] * (1 - fx) + bot[..., xhi] * fx
        v = top * (1 - fy) + bot * fy
    return torch.where(v >= 0.5, v, torch.zeros_like(v))


def channel_weights(C, heat_start, bkg_start, mtw, ktw, device="cpu"):
    cw = torch.ones(C, dtype=F64, device=device)
    cw[heat_start:bkg_start] = ktw
    cw[C - 2] = mtw              # the person-mask channel wins an overlap
    return cw


def focal_l2(pred, gt, mask, *, heat_start, bkg_start, gamma, mtw, ktw,
             alpha=0.0, beta=0.0, gscale=None):
    """``pred`` [S, N, C, H, W], ``gt`` [N, C, rH, rW], ``mask`` [N, 1, rH, rW].

    Returns a dict of fp64 tensors:
      sums      [S]   per-stack sum of (s-g)^2 * |1-st|^gamma * mask * w_c
      sums_abs  [S]   the same (every addend is non-negative)
      u         [S, N, C, H, W]   1 - st, the base of the focal factor
      dpred, dpred_abs   gradient of sum_j gscale[j] * sums[j] with respect to
                pred and the sum of the absolute values of its two terms
                w*gscale*(2 d factor) and w*gscale*(d^2 factor'); only with
                ``gscale`` ([S]). sign(0) = 0 for gamma = 1."""
    pred = pred.detach().to(F64)
    gt = gt.detach().to(F64)
    mask = mask.detach().to(F64)
    S, N, C, H, W = pred.shape
    r = gt.shape[2] // H
    assert gt.shape[2] == r * H and gt.shape[3] == r * W
    g = _window_mean(gt, r) if r > 1 else gt
    m = _mask_sample(mask, r)
    w = (m * channel_weights(C, heat_start, bkg_start, mtw, ktw,
                             pred.device).view(1, C, 1, 1)).unsqueeze(0)
    g = g.unsqueeze(0)
    pos = g >= 0.01
    st = torch.where(pos, pred - alpha, 1.0 - pred - beta)
    u = 1.0 - st
    factor = u.abs() if gamma == 1 else u * u
    d = pred - g
    addend = d * d * factor * w
    out = {"sums": addend.sum(dim=(1, 2, 3, 4)),
           "sums_abs": addend.abs().sum(dim=(1, 2, 3, 4)), "u": u}
    if gscale is not None:
        gs = gscale.detach().to(F64).to(pred.device).view(S, 1, 1, 1, 1)
        du = torch.where(pos, -torch.ones_like(u), torch.ones_like(u))
        dfac = (torch.sign(u) if gamma == 1 else 2.0 * u) * du
        t1 = w * gs * (2.0 * d * factor)
        t2 = w * gs * (d * d * dfac)
        out["dpred"] = t1 + t2
        out["dpred_abs"] = t1.abs() + t2.abs()
    return out


# ---------------------------------------------------------------------------
# SGD with momentum, weight decay and a bf16 copy of an fp32 master
# ---------------------------------------------------------------------------

def sgd_steps(w0, grads, lr, mu, wd, m0=None):
    """``g = grad + wd*w ; m = mu*m + g ; w -= lr*m`` for each gradient in
    ``grads`` (momentum starts at ``m0`` or zero). Returns a list with one
    ``(w, m, w_bf16)`` per step, fp64 / fp64 / bf16 = RNE(w)."""
    w = w0.detach().to("cpu", F64).clone()
    m = torch.zeros_like(w) if m0 is None else m0.detach().to("cpu", F64).clone()
    out = []
    for g in grads:
        gv = g.detach().to("cpu", F64) + wd * w
        m = mu * m + gv
        w = w - lr * m
        out.append((w.clone(), m.clone(), rne_bf16(w)))
    return out
