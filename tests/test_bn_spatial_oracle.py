"""Validates ``bn_spatial_oracle`` (the fp64 reference of the GPU tests in
``test_bn_spatial_gpu.py``) against torch's own fp64 operators. CPU only."""
import pytest
import torch
import torch.nn.functional as F

import bn_spatial_oracle as O

F64 = torch.float64
SLOPE = 0.01


def _close(a, b, what, rtol=1e-11, atol=1e-12):
    assert a.shape == b.shape, f"{what}: {a.shape} vs {b.shape}"
    assert torch.allclose(a, b, rtol=rtol, atol=atol), \
        f"{what}: max |diff| {(a - b).abs().max().item():.3e}"


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------
# bf16 helpers
# ---------------------------------------------------------------------------

def test_rne_bf16_rounds_once_to_even():
    x = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40,
                      0.0, -2.5, 3.0e38, 3.4e38, 2.0 ** -133 * 1.5, 2.0 ** -134],
                     dtype=F64)
    want = torch.tensor([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 0.0, -2.5,
                         float(torch.tensor(3.0e38).bfloat16()), float("inf"),
                         2.0 ** -132, 0.0], dtype=F64)
    assert torch.equal(O.rne_bf16(x).double(), want)
    # a value just above a bf16 tie whose fp32 rounding lands ON the tie: two
    # roundings give 1.0, one rounding gives the next bf16
    assert float(O.rne_bf16(torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40],
                                         dtype=F64))) == 1 + 2.0 ** -7
    torch.manual_seed(0)
    r = torch.randn(20000, dtype=F64) * torch.exp2(
        torch.randint(-30, 30, (20000,)).double())
    # every fp32-representable value rounds like torch's own fp32 -> bf16 cast
    r32 = r.float()
    assert torch.equal(O.rne_bf16(r32.double()), r32.bfloat16())


def test_bf16_ulp_helpers():
    a = torch.tensor([1.0, -0.0, 2.0, -1.0, 1.0]).bfloat16()
    b = torch.tensor([1 + 2.0 ** -7, 0.0, 2.0 - 2.0 ** -7, -1.0, -1.0]).bfloat16()
    d = O.bf16_ulp_distance(a, b)
    assert d[:4].tolist() == [1, 0, 1, 0] and d[4] == 2 * 0x3F80
    u = O.bf16_ulp(torch.tensor([1.0, 1.99, 2.0, -3.0, 0.0], dtype=F64))
    assert u.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133]


# ---------------------------------------------------------------------------
# BatchNorm + leaky relu
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("act,res", [(True, False), (False, False), (True, True)],
                         ids=["act", "noact", "act-res"])
def test_bn_act_matches_batchnorm2d(training, act, res):
    torch.manual_seed(4)
    N, C, H, W = 3, 5, 4, 7
    M = N * H * W
    bn = torch.nn.BatchNorm2d(C, momentum=0.1, eps=1e-5).double()
    with torch.no_grad():
        bn.weight.copy_(torch.tensor([1.5, -0.7, 0.0, 0.3, 2.0]))
        bn.bias.copy_(torch.randn(C))
        bn.running_mean.copy_(torch.randn(C))
        bn.running_var.copy_(torch.rand(C) + 0.5)
    bn.train(training)
    x = (torch.randn(N, C, H, W, dtype=F64) * 2 + 1).requires_grad_(True)
    r = torch.randn(N, C, H, W, dtype=F64, requires_grad=True) if res else None
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    nb = bn.num_batches_tracked.clone()

    pre = bn(x) + r if res else bn(x)
    y = F.leaky_relu(pre, SLOPE) if act else pre
    dy = torch.randn_like(y)
    y.backward(dy)

    xm = _nhwc(x.detach()).reshape(M, C)
    g, b = bn.weight.detach(), bn.bias.detach()
    if training:
        s, q = O.bn_stats(xm, C)
        _close(s, xm.sum(0), "sums")
        _close(q, (xm * xm).sum(0), "sumsq")
        rm2, rv2, nb2 = rm.clone(), rv.clone(), nb.clone()
        mean, invstd, scale, shift = O.bn_stats_finalize(
            xm, C, g, b, rm, rv, nb, 0.1, 1e-5)
        split = O.bn_finalize(s, q, M, g, b, rm2, rv2, nb2, 0.1, 1e-5)
        for u, v in zip(split + [rm2, rv2], [mean, invstd, scale, shift, rm, rv]):
            assert torch.equal(u, v)
        _close(rm, bn.running_mean, "running_mean")
        _close(rv, bn.running_var, "running_var (unbiased factor)")
        assert int(nb) == int(bn.num_batches_tracked) == int(nb2) == 1
        _close(mean, xm.mean(0), "mean")
        _close(invstd, 1 / torch.sqrt(xm.var(0, unbiased=False) + 1e-5), "invstd")
    else:
        mean = rm
        invstd = 1 / torch.sqrt(rv + 1e-5)
        scale = g * invstd
        shift = b - mean * scale
        assert int(bn.num_batches_tracked) == 0

    rn = _nhwc(r.detach()).reshape(M, C) if res else None
    yo = O.bn_act_fwd(xm, scale, shift, rn, SLOPE, act)
    _close(yo, _nhwc(y.detach()).reshape(M, C), "y")
    terms = O.bn_act_fwd_terms(xm, scale, shift, rn)
    assert (terms >= yo.abs() - 1e-12).all()

    dym = _nhwc(dy).reshape(M, C)
    dpre, sd, sx = O.bn_act_bwd(dym, yo, xm, mean, invstd, SLOPE, act, True, C)
    _close(sd, bn.bias.grad, "dbeta = sum dpre")
    _close(sx, bn.weight.grad, "dgamma = sum dpre*xhat")
    if res:
        _close(dpre, _nhwc(r.grad).reshape(M, C), "dpre")
    dpre0, sd0, sx0 = O.bn_act_bwd(dym, yo, xm, None, None, SLOPE, act, False, C)
    assert torch.equal(dpre0, dpre) and torch.equal(sd0, sd)
    assert torch.equal(sx0, torch.zeros(C, dtype=F64))
    sums = (sd, sx) if training else (None, None)
    dx = O.bn_act_bwd_apply(dpre, xm, mean, invstd, g, *sums, C)
    _close(dx, _nhwc(x.grad).reshape(M, C), "dx")
    p, qx, rr = O.bn_act_bwd_apply_terms(dpre, xm, mean, invstd, g, *sums, C)
    _close(p + qx + rr, dx, "P*dpre + Q*x + R", atol=1e-10)


def test_bn_constant_channel_clamps_variance():
    x = torch.full((7, 3), 1.7, dtype=F64)
    mean, invstd, scale, shift = O.bn_stats_finalize(
        x, 3, torch.ones(3), torch.tensor([0.5, -1.0, 2.0]), None, None, None,
        0.1, 1e-5)
    assert torch.isfinite(invstd).all() and (invstd <= 1e-5 ** -0.5).all()
    y = O.bn_act_fwd(x, scale, shift, None, SLOPE, False)
    _close(y, torch.tensor([0.5, -1.0, 2.0], dtype=F64).expand(7, 3), "y=beta",
           atol=1e-9)


def test_bn_single_row_unbiased_factor():
    rm, rv = torch.zeros(2, dtype=F64), torch.ones(2, dtype=F64)
    O.bn_stats_finalize(torch.tensor([[1.0, 2.0]], dtype=F64), 2, torch.ones(2),
                        torch.zeros(2), rm, rv, None, 0.5, 1e-5)
    assert torch.equal(rm, torch.tensor([0.5, 1.0], dtype=F64))
    assert torch.equal(rv, torch.tensor([0.5, 0.5], dtype=F64))   # M-1 -> 1


# ---------------------------------------------------------------------------
# maxpool / upsample
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(2, 3, 2, 2), (1, 4, 6, 10), (2, 5, 7, 9),
                                   (1, 2, 5, 4)])
@pytest.mark.parametrize("levels", [0, 4, 1], ids=["randn", "ties4", "all-equal"])
def test_maxpool_matches_torch(shape, levels):
    torch.manual_seed(sum(shape) + levels)
    N, C, H, W = shape
    if levels == 0:
        x = torch.randn(shape, dtype=F64)
    else:
        x = torch.randint(0, levels, shape).double() - 1.0
    x.requires_grad_(True)
    y = F.max_pool2d(x, 2, 2)
    dy = torch.randn_like(y)
    y.backward(dy)
    yo, arg = O.maxpool2x2_fwd(_nhwc(x.detach()), N, H, W, C)
    assert arg.dtype == torch.uint8 and int(arg.max()) <= 3
    assert torch.equal(yo, _nhwc(y.detach()))
    dxo = O.maxpool2x2_bwd(_nhwc(dy), arg, N, H, W, C)
    # torch's CPU max_pool2d also keeps the first maximum in row-major order
    assert torch.equal(dxo, _nhwc(x.grad))
    if levels == 1:
        assert int(arg.max()) == 0
    # odd extents: the last row / column gets no gradient
    assert not dxo[:, 2 * (H // 2):].any() and not dxo[:, :, 2 * (W // 2):].any()


def test_maxpool_argmax_is_first_maximum():
    # one window per channel, every tie pattern of two values
    pats = torch.tensor([[(k >> b) & 1 for b in range(4)] for k in range(16)],
                        dtype=F64)                              # [16, 4]
    x = pats.t().reshape(1, 2, 2, 16)                           # NHWC
    _, arg = O.maxpool2x2_fwd(x, 1, 2, 2, 16)
    want = [0 if k == 0 else min(b for b in range(4) if (k >> b) & 1)
            for k in range(16)]
    assert arg.reshape(16).tolist() == want


@pytest.mark.parametrize("shape", [(2, 3, 2, 2), (1, 4, 3, 5)])
def test_upsample_matches_torch(shape):
    torch.manual_seed(1)
    N, C, H, W = shape
    x = torch.randn(shape, dtype=F64, requires_grad=True)
    y = F.interpolate(x, scale_factor=2, mode="nearest")
    dy = torch.randn_like(y)
    y.backward(dy)
    assert torch.equal(O.upsample2x_fwd(_nhwc(x.detach()), N, H, W, C),
                       _nhwc(y.detach()))
    _close(O.upsample2x_bwd(_nhwc(dy), N, H, W, C), _nhwc(x.grad), "upsample dx")


# ---------------------------------------------------------------------------
# squeeze-excitation
# ---------------------------------------------------------------------------

def test_se_chain_matches_eager():
    torch.manual_seed(2)
    N, C, CH, H, W = 3, 16, 4, 5, 6
    HW = H * W
    fc1 = torch.nn.Linear(C, CH).double()
    fc2 = torch.nn.Linear(CH, C).double()
    x = torch.randn(N, C, H, W, dtype=F64, requires_grad=True)
    pooled = x.mean(dim=(2, 3))
    s = torch.sigmoid(fc2(F.leaky_relu(fc1(pooled), SLOPE)))
    s.retain_grad()
    xs = x.detach().clone().requires_grad_(True)   # dx of the scale op alone
    y = xs * s.view(N, C, 1, 1)
    dy = torch.randn_like(y)
    y.backward(dy)

    xn = _nhwc(x.detach())
    sums = O.se_reduce(xn, None, N, HW, C)
    _close(sums / HW, pooled.detach(), "GAP")
    so = O.se_gate(sums, fc1.weight, fc1.bias, fc2.weight, fc2.bias, SLOPE,
                   1.0 / HW)
    _close(so, s.detach(), "gate")
    _close(O.se_gate(sums / HW, fc1.weight, fc1.bias, fc2.weight, fc2.bias,
                     SLOPE), so, "gate, pool_scale default")
    _close(O.se_scale(xn, so, None, N, HW, C), _nhwc(y.detach()), "scale")
    addc = torch.randn(N, C, dtype=F64)
    _close(O.se_scale(xn, so, addc, N, HW, C),
           _nhwc(y.detach() + addc.view(N, C, 1, 1)), "scale + addc")
    _close(O.se_reduce(_nhwc(dy), xn, N, HW, C), s.grad, "ds = <dy, x>")
    _close(O.se_scale(_nhwc(dy), so, None, N, HW, C), _nhwc(xs.grad), "scale dx")


def test_se_layer_fwd_bwd_matches_autograd():
    torch.manual_seed(5)
    N, C, CH, H, W = 2, 32, 2, 4, 3
    fc1 = torch.nn.Linear(C, CH).double()
    fc2 = torch.nn.Linear(CH, C).double()
    x = torch.randn(N, C, H, W, dtype=F64, requires_grad=True)
    s = torch.sigmoid(fc2(F.leaky_relu(fc1(x.mean(dim=(2, 3))), SLOPE)))
    y = x * s.view(N, C, 1, 1)
    dy = torch.randn_like(y)
    y.backward(dy)
    got = O.se_layer_fwd_bwd(_nhwc(x.detach()), fc1.weight, fc1.bias,
                             fc2.weight, fc2.bias, _nhwc(dy), SLOPE)
    want = [_nhwc(y.detach()), _nhwc(x.grad), fc1.weight.grad, fc1.bias.grad,
            fc2.weight.grad, fc2.bias.grad]
    for g, w, name in zip(got, want, ["y", "dx", "dw1", "db1", "dw2", "db2"]):
        _close(g, w, name)
