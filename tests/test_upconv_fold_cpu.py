"""Upsample-folded refine conv: the identity itself, on the CPU in float64.

``conv2d(interpolate(x, 2, 'nearest'), W, padding=1)`` equals, per output
parity (py, px), a 2x2 conv over the low-resolution map with the folded
weights of ``conv_kernels.upfold_weight_reference`` and zero reads outside the
map. In float64 with small-integer operands both sides are exact, so the
comparison has no tolerance; a random-operand case is held to a few ulps.
"""
import pytest
import torch
import torch.nn.functional as F

from improved_body_parts_amd.ops import conv_kernels


def _fold_apply(x, e):
    """x [N, Cin, H, W], e [4, Cout, 2, 2, Cin] -> [N, Cout, 2H, 2W] by the
    formula of the kernel: low-resolution row i + a - (1 - py), zero outside."""
    n, cin, h, w = x.shape
    cout = e.shape[1]
    y = x.new_zeros(n, cout, 2 * h, 2 * w)
    for py in range(2):
        for px in range(2):
            # pad (1 - py) rows on top / py at the bottom, likewise columns
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            k = e[py * 2 + px].permute(0, 3, 1, 2)      # [Cout, Cin, 2, 2]
            y[:, :, py::2, px::2] = F.conv2d(xp, k)
    return y


@pytest.mark.parametrize("h,w", [(5, 7), (8, 8)])
def test_fold_equals_upsample_then_conv_exactly_in_float64(h, w):
    gen = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randint(-3, 4, (2, 6, h, w), generator=gen).double()
    wt = torch.randint(-2, 3, (5, 6, 3, 3), generator=gen).double()
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt,
                    padding=1)
    e = conv_kernels.upfold_weight_reference(wt)
    assert e.shape == (4, 5, 2, 2, 6) and e.dtype == torch.float64
    got = _fold_apply(x, e)
    assert got.shape == want.shape
    for py in range(2):
        for px in range(2):
            assert torch.equal(got[:, :, py::2, px::2],
                               want[:, :, py::2, px::2]), f"parity {py},{px}"


@pytest.mark.parametrize("h,w", [(5, 7), (8, 8)])
def test_fold_on_random_float64_operands(h, w):
    gen = torch.Generator().manual_seed(h * 7 + w)
    x = torch.randn(1, 4, h, w, generator=gen, dtype=torch.float64)
    wt = torch.randn(3, 4, 3, 3, generator=gen, dtype=torch.float64)
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt,
                    padding=1)
    got = _fold_apply(x, conv_kernels.upfold_weight_reference(wt))
    # 36 products per output either way, regrouped: a few float64 ulps
    assert (got - want).abs().max() <= 64 * 2.0 ** -52 * want.abs().max()


def test_fold_sums_the_taps_the_issue_names():
    """E[py][px][a][b] = sum over kh in R(py,a), kw in R(px,b) with
    R(0,0)={0} R(0,1)={1,2} R(1,0)={0,1} R(1,1)={2}: checked with a weight
    whose entries are distinct powers of two (the sum names its terms)."""
    wt = (2.0 ** torch.arange(9, dtype=torch.float64)).reshape(1, 1, 3, 3)
    e = conv_kernels.upfold_weight_reference(wt)[:, 0, :, :, 0]
    rows = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    want = sum(2.0 ** (kh * 3 + kw) for kh in rows[(py, a)]
                               for kw in rows[(px, b)])
                    assert float(e[py * 2 + px, a, b]) == want


def test_bf16_fold_rounds_once_from_fp32():
    """bf16 weights: fp32 sum, one rounding; cancelling sums give exact 0."""
    wt = torch.tensor([1.0, -1.0, 0.00390625, 1.0, -1.0, 3.0, 2.0, 5.0, 7.0]
                      ).reshape(1, 1, 3, 3).bfloat16()
    e = conv_kernels.upfold_weight_reference(wt)
    assert e.dtype == torch.bfloat16
    # parity (1,1), tap (0,0): W[0][0]+W[0][1]+W[1][0]+W[1][1] = 1-1+1-1
    assert float(e[3, 0, 0, 0, 0]) == 0.0
    # parity (0,1), tap (0,0): W[0][0] + W[0][1] = 0; tap (1,1): W[1][2]+W[2][2]
    assert float(e[1, 0, 0, 0, 0]) == 0.0
    assert float(e[1, 0, 1, 1, 0]) == 10.0
    # parity (0,0), tap (0,1): W[0][1] + W[0][2] = -1 + 2^-8 -> bf16(-0.99609375)
    assert float(e[0, 0, 0, 1, 0]) == -0.99609375


def test_cpu_op_is_the_two_calls():
    """Off the GPU ``ops.upsample_conv_bn_act`` is upsample then conv."""
    from improved_body_parts_amd import ops
    torch.manual_seed(0)
    conv = torch.nn.Conv2d(8, 8, 3, 1, 1, bias=False)
    bn = torch.nn.BatchNorm2d(8).eval()
    low = torch.randn(1, 8, 5, 7)
    post = torch.randn(1, 8, 10, 14)
    with torch.no_grad():
        got = ops.upsample_conv_bn_act(low, conv, bn, act=True,
                                       residual_post=post)
        want = ops.conv_bn_act(ops.upsample2x_nearest(low), conv, bn,
                               act=True, training=False, residual_post=post)
    assert torch.equal(got, want)
