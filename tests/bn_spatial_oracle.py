"""fp64 CPU oracle for the kernels of ``bn_act.hip`` and ``spatial.hip``.

One function per extension op, with the argument list of the binding in
``bindings.cpp``. Every input is promoted to float64 on the CPU, every output
is float64 (argmax bytes are uint8). Activations are ``[M][C]`` / NHWC, like
the storage the kernels see. ``test_bn_spatial_oracle.py`` validates this file
against torch's own fp64 BatchNorm / max_pool2d / interpolate / SE chain.
"""
from __future__ import annotations

import torch

F64 = torch.float64


def _d(t):
    return None if t is None else t.detach().to("cpu", F64)


# ---------------------------------------------------------------------------
# bf16 helpers
# ---------------------------------------------------------------------------

def _pow2(k: torch.Tensor) -> torch.Tensor:
    """Exact 2**k in fp64 for an integer tensor, |k| < 1023 (built from the
    exponent bits: no library pow / ldexp rounding or dtype promotion)."""
    return ((k.to(torch.int64) + 1023) << 52).view(F64)


def rne_bf16(x64: torch.Tensor) -> torch.Tensor:
    """Round an fp64 tensor to the nearest bf16 (ties to even) in ONE rounding
    step (fp64 -> fp32 -> bf16 would round twice). Returns a bf16 tensor."""
    x = x64.detach().to("cpu", F64)
    m, e = torch.frexp(x)                       # x = m * 2**e, 0.5 <= |m| < 1
    # 8 significant bits; below 2**-126 the bf16 grid is the fixed 2**-133
    e = torch.clamp(e, min=-125)
    q = torch.round(x * _pow2(8 - e))           # torch.round is half-to-even
    r = q * _pow2(e - 8)
    r = torch.where(torch.isfinite(x), r, x)
    out = r.to(torch.bfloat16)                  # exact: r is on the bf16 grid
    big = torch.isfinite(x) & (r.abs() > 3.3895313892515355e38)
    return torch.where(big, torch.sign(x).to(torch.bfloat16) * float("inf"), out)


def bf16_ulp(x64: torch.Tensor) -> torch.Tensor:
    """Size of one bf16 ulp at |x| (fp64 tensor): 2**(floor(log2|x|) - 7)."""
    x = x64.detach().to("cpu", F64)
    _, e = torch.frexp(x)
    e = torch.where(x == 0, torch.full_like(e, -125), torch.clamp(e, min=-125))
    return _pow2(e - 8)


def _bf16_ordinal(t: torch.Tensor) -> torch.Tensor:
    assert t.dtype == torch.bfloat16
    i = t.detach().cpu().contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)   # -0.0 and +0.0 coincide


def bf16_ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance between two bf16 tensors counted in representable values."""
    return (_bf16_ordinal(a) - _bf16_ordinal(b)).abs()


# ---------------------------------------------------------------------------
# bn_act.hip
# ---------------------------------------------------------------------------

def bn_stats(x_mc, C):
    x = _d(x_mc).reshape(-1, C)
    return [x.sum(0), (x * x).sum(0)]


def bn_finalize(sums, sumsq, M, gamma, beta, running_mean, running_var,
                num_batches, momentum, eps):
    """[mean, invstd, scale, shift]; ``running_*`` (fp64) and ``num_batches``
    (int64) are updated in place when given, like the kernel does."""
    s, q, g, b = _d(sums), _d(sumsq), _d(gamma), _d(beta)
    mean = s / M
    var = torch.clamp(q / M - mean * mean, min=0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    if running_mean is not None:
        assert running_mean.dtype == F64 and running_var.dtype == F64
        unbiased = var * (M / (M - 1 if M > 1 else 1))
        running_mean.mul_(1.0 - momentum).add_(mean * momentum)
        running_var.mul_(1.0 - momentum).add_(unbiased * momentum)
    if num_batches is not None:
        num_batches += 1
    scale = g * invstd
    shift = b - mean * scale
    return [mean, invstd, scale, shift]


def bn_stats_finalize(x_mc, C, gamma, beta, running_mean, running_var,
                      num_batches, momentum, eps):
    x = _d(x_mc).reshape(-1, C)
    s, q = bn_stats(x, C)
    return bn_finalize(s, q, x.shape[0], gamma, beta, running_mean,
                       running_var, num_batches, momentum, eps)


def _leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


def bn_act_fwd(x, scale, shift, residual, slope, act):
    sc, sh = _d(scale), _d(shift)
    xd = _d(x)
    v = xd.reshape(-1, sc.numel()) * sc + sh
    if residual is not None:
        v = v + _d(residual).reshape(v.shape)
    return (_leaky(v, slope) if act else v).reshape(xd.shape)


def bn_act_fwd_terms(x, scale, shift, residual):
    """Sum of |addends| of the forward formula (for the elementwise bound)."""
    sc, sh = _d(scale), _d(shift)
    xd = _d(x)
    t = (xd.reshape(-1, sc.numel()) * sc).abs() + sh.abs()
    if residual is not None:
        t = t + _d(residual).reshape(t.shape).abs()
    return t.reshape(xd.shape)


def bn_act_bwd(dy, y, x, mean, invstd, slope, act, need_xhat, C):
    """[dpre, sum_dpre, sum_dxhat]; sum_dxhat is zero without ``need_xhat``."""
    g = _d(dy).reshape(-1, C)
    if act:
        g = torch.where(_d(y).reshape(-1, C) > 0, g, g * slope)
    sum_dpre = g.sum(0)
    if need_xhat:
        xhat = (_d(x).reshape(-1, C) - _d(mean)) * _d(invstd)
        sum_dxhat = (g * xhat).sum(0)
    else:
        sum_dxhat = torch.zeros(C, dtype=F64)
    return [g.reshape(dy.shape), sum_dpre, sum_dxhat]


def bn_act_bwd_apply_terms(dpre, x, mean, invstd, gamma, sum_dpre, sum_dxhat,
                           C):
    """The addends (P*dpre, Q*x, R) of dx = P[c]*dpre + Q[c]*x + R[c]; the eval
    form (sums None) has Q = R = 0."""
    g = _d(dpre).reshape(-1, C)
    xd = _d(x).reshape(-1, C)
    M = g.shape[0]
    A = _d(gamma) * _d(invstd)
    if sum_dpre is None:
        z = torch.zeros_like(g)
        return A * g, z, z
    Q = -A * _d(invstd) * _d(sum_dxhat) / M
    R = -A * _d(sum_dpre) / M - Q * _d(mean)
    return A * g, Q * xd, R.expand_as(g)


def bn_act_bwd_apply(dpre, x, mean, invstd, gamma, sum_dpre, sum_dxhat, C):
    """dx = gamma*invstd*(dpre - sum_dpre/M - xhat*sum_dxhat/M); eval form
    (sums None): dx = gamma*invstd*dpre."""
    g = _d(dpre).reshape(-1, C)
    M = g.shape[0]
    w = _d(gamma) * _d(invstd)
    if sum_dpre is not None:
        xhat = (_d(x).reshape(-1, C) - _d(mean)) * _d(invstd)
        g = g - _d(sum_dpre) / M - xhat * _d(sum_dxhat) / M
    return (w * g).reshape(dpre.shape)


# ---------------------------------------------------------------------------
# spatial.hip (NHWC)
# ---------------------------------------------------------------------------

def maxpool2x2_fwd(x, N, H, W, C):
    """[y, arg]: arg in 0..3 is the FIRST maximum of the window in row-major
    order (00, 01, 10, 11); an odd last row / column is never read."""
    xd = _d(x).reshape(N, H, W, C)
    Ho, Wo = H // 2, W // 2
    xd = xd[:, :2 * Ho, :2 * Wo]
    win = torch.stack([xd[:, 0::2, 0::2], xd[:, 0::2, 1::2],
                       xd[:, 1::2, 0::2], xd[:, 1::2, 1::2]], dim=0)
    y = win[0].clone()
    arg = torch.zeros(y.shape, dtype=torch.uint8)
    for k in (1, 2, 3):
        better = win[k] > y          # strict: an equal later value never wins
        y = torch.where(better, win[k], y)
        arg = torch.where(better, torch.full_like(arg, k), arg)
    return [y, arg]


def maxpool2x2_bwd(dy, arg, N, H, W, C):
    Ho, Wo = H // 2, W // 2
    g = _d(dy).reshape(N, Ho, Wo, C)
    a = arg.detach().cpu().reshape(N, Ho, Wo, C)
    dx = torch.zeros(N, H, W, C, dtype=F64)
    for k in range(4):
        dh, dw = k >> 1, k & 1
        dx[:, dh:2 * Ho:2, dw:2 * Wo:2] = torch.where(a == k, g,
                                                      torch.zeros_like(g))
    return dx


def upsample2x_fwd(x, N, H, W, C):
    xd = _d(x).reshape(N, H, W, C)
    return xd.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def upsample2x_bwd(dy, N, H, W, C):
    """(H, W) are the INPUT extents; dy is [N, 2H, 2W, C]."""
    g = _d(dy).reshape(N, 2 * H, 2 * W, C)
    return (g[:, 0::2, 0::2] + g[:, 0::2, 1::2]
            + g[:, 1::2, 0::2] + g[:, 1::2, 1::2])


def se_reduce(a, b, N, HW, C):
    v = _d(a).reshape(N, HW, C)
    if b is not None:
        v = v * _d(b).reshape(N, HW, C)
    return v.sum(1)


def se_scale(x, s, addc, N, HW, C):
    xd = _d(x)
    v = xd.reshape(N, HW, C) * _d(s).reshape(N, 1, C)
    if addc is not None:
        v = v + _d(addc).reshape(N, 1, C)
    return v.reshape(xd.shape)


def se_gate(pooled, w1, b1, w2, b2, slope, pool_scale=1.0):
    p = _d(pooled) * pool_scale
    h = _leaky(p @ _d(w1).t() + _d(b1), slope)
    return torch.sigmoid(h @ _d(w2).t() + _d(b2))


def se_layer_fwd_bwd(x, w1, b1, w2, b2, dy, slope):
    """The whole training SE layer on an NHWC map and its backward, from the
    ops above and the chain rule: [y, dx, dw1, db1, dw2, db2]."""
    xd, g = _d(x), _d(dy)
    N, H, W, C = xd.shape
    HW = H * W
    W1, B1, W2, B2 = _d(w1), _d(b1), _d(w2), _d(b2)
    p = se_reduce(xd, None, N, HW, C) / HW
    z1 = p @ W1.t() + B1
    h = _leaky(z1, slope)
    s = torch.sigmoid(h @ W2.t() + B2)
    y = se_scale(xd, s, None, N, HW, C)
    ds = se_reduce(g, xd, N, HW, C)
    dz2 = ds * s * (1.0 - s)
    dz1 = dz2 @ W2
    dz1 = torch.where(z1 > 0, dz1, dz1 * slope)
    dp = dz1 @ W1
    dx = se_scale(g, s, dp / HW, N, HW, C)
    return [y, dx, dz1.t() @ p, dz1.sum(0), dz2.t() @ h, dz2.sum(0)]
