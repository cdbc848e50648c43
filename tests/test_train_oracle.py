"""CPU validation of ``train_oracle.py`` against torch's own fp64 results at
tiny shapes: ``torch.nn.grad.conv2d_weight``, the eager branch of
``ops.focal_l2_loss`` through autograd, and ``torch.optim.SGD``."""
import pytest
import torch

import train_oracle as O
from improved_body_parts_amd import ops

F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# N, Cin, Cout, H, W, KH, KW, stride, pad, dil
WGRAD_CASES = [
    (2, 3, 4, 7, 9, 3, 3, 1, (1, 1), (1, 1)),
    (1, 5, 2, 9, 8, 1, 1, 1, (0, 0), (1, 1)),
    (2, 3, 4, 11, 10, 3, 3, 2, (1, 1), (1, 1)),     # stride 2, odd and even
    (2, 2, 3, 13, 12, 7, 7, 2, (3, 3), (1, 1)),     # the stem's geometry
    (1, 4, 3, 10, 14, 3, 3, 1, (3, 5), (3, 5)),     # unequal pad / dilation
    (2, 3, 2, 8, 9, 1, 3, 1, (0, 1), (1, 1)),       # KH != KW
    (1, 2, 3, 9, 9, 3, 2, 2, (2, 0), (2, 1)),       # everything unequal
    (3, 2, 2, 3, 1, 3, 3, 1, (1, 1), (1, 1)),       # Wo = 1
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_wgrad_oracle_matches_conv2d_weight(case):
    N, Cin, Cout, H, W, KH, KW, s, pad, dil = case
    g = _gen(1)
    x = torch.randn(N, Cin, H, W, generator=g, dtype=F64)
    Ho = (H + 2 * pad[0] - dil[0] * (KH - 1) - 1) // s + 1
    Wo = (W + 2 * pad[1] - dil[1] * (KW - 1) - 1) // s + 1
    dy = torch.randn(N, Cout, Ho, Wo, generator=g, dtype=F64)
    shape = (Cout, Cin, KH, KW)
    want = torch.nn.grad.conv2d_weight(x, shape, dy, stride=s, padding=pad,
                                       dilation=dil)
    got = O.wgrad(x, dy, shape, s, pad, dil)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    want_abs = torch.nn.grad.conv2d_weight(x.abs(), shape, dy.abs(), stride=s,
                                           padding=pad, dilation=dil)
    torch.testing.assert_close(O.wgrad_abs(x, dy, shape, s, pad, dil),
                               want_abs, rtol=1e-12, atol=1e-12)
    assert (want_abs >= want.abs() - 1e-12).all()


@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("gamma", [1, 2])
@pytest.mark.parametrize("ab", [(0.0, 0.0), (0.1, 0.02)])
def test_focal_oracle_matches_eager_autograd(r, gamma, ab):
    g = _gen(10 * r + gamma)
    S, N, C, H, W = 3, 2, 6, 4, 6
    pred = torch.rand(S, N, C, H, W, generator=g, dtype=F64)
    # the eager branch pools gt and samples the mask in fp32: multiples of
    # 1/64 and 1/4 keep that exact, so fp64 agreement is not limited by it
    gt = torch.randint(0, 65, (N, C, r * H, r * W), generator=g).to(F64) / 64
    gt = gt * (torch.rand(gt.shape, generator=g) < 0.4)   # zeros: both branches
    mask = torch.randint(0, 5, (N, 1, r * H, r * W), generator=g).to(F64) / 4
    nw = (1, 2, 4)
    kw = dict(heat_start=2, bkg_start=4, gamma=gamma, multi_task_weight=0.1,
              keypoint_task_weight=3.0, alpha=ab[0], beta=ab[1])
    p = pred.clone().requires_grad_(True)
    loss = ops.focal_l2_loss(p, gt, mask, nstack_weight=nw, **kw)
    (3.0 * loss).backward()
    gscale = 3.0 * torch.tensor(nw, dtype=F64) / sum(nw)
    o = O.focal_l2(pred, gt, mask, heat_start=2, bkg_start=4, gamma=gamma,
                   mtw=0.1, ktw=3.0, alpha=ab[0], beta=ab[1], gscale=gscale)
    want_loss = (o["sums"] * torch.tensor(nw, dtype=F64)).sum() / sum(nw)
    torch.testing.assert_close(want_loss, loss.detach(), rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(o["dpred"], p.grad, rtol=1e-11, atol=1e-13)
    assert (o["dpred_abs"] >= o["dpred"].abs() - 1e-15).all()
    assert torch.equal(o["sums"], o["sums_abs"])
    # both sides of both switches are present at these shapes
    m = O._mask_sample(mask, r)
    assert (m == 0).any() and (m >= 0.5).any()


def test_focal_oracle_sign_of_zero():
    """gamma = 1 at u = 0 exactly: d|u|/ds is taken as 0 (as torch.abs does)."""
    pred = torch.tensor([1.0, 0.0], dtype=F64).view(1, 1, 2, 1, 1)
    gt = torch.tensor([0.5, 0.0], dtype=F64).view(1, 2, 1, 1)
    mask = torch.ones(1, 1, 1, 1, dtype=F64)
    o = O.focal_l2(pred, gt, mask, heat_start=0, bkg_start=0, gamma=1,
                   mtw=1.0, ktw=1.0, gscale=torch.ones(1, dtype=F64))
    assert torch.equal(o["u"].flatten(), torch.zeros(2, dtype=F64))
    assert torch.equal(o["dpred"].flatten(), torch.zeros(2, dtype=F64))
    p = pred.clone().requires_grad_(True)
    ops.focal_l2_loss(p, gt, mask, heat_start=0, bkg_start=0, gamma=1,
                      multi_task_weight=1.0, keypoint_task_weight=1.0,
                      nstack_weight=(1,)).backward()
    assert torch.equal(p.grad, o["dpred"])


def test_mask_sample_matches_interpolate():
    g = _gen(3)
    for r in (2, 3, 4, 16):
        mask = torch.rand(2, 1, 2 * r, 3 * r, generator=g, dtype=F64)
        want = torch.nn.functional.interpolate(
            mask, size=(2, 3), mode="bilinear", align_corners=False)
        want = torch.where(want >= 0.5, want, torch.zeros_like(want))
        torch.testing.assert_close(O._mask_sample(mask, r), want,
                                   rtol=1e-13, atol=1e-14)


@pytest.mark.parametrize("mu,wd", [(0.9, 1e-4), (0.0, 1e-4), (0.9, 0.0),
                                   (0.5, 0.25)])
def test_sgd_oracle_matches_torch_sgd(mu, wd):
    g = _gen(5)
    w0 = torch.randn(3, 5, generator=g, dtype=F64)
    grads = [torch.randn(3, 5, generator=g, dtype=F64) for _ in range(4)]
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.SGD([p], lr=0.05, momentum=mu, weight_decay=wd)
    steps = O.sgd_steps(w0, grads, 0.05, mu, wd)
    for gr, (w, m, wb) in zip(grads, steps):
        p.grad = gr.clone()
        opt.step()
        torch.testing.assert_close(w, p.detach(), rtol=1e-13, atol=1e-14)
        if mu:
            torch.testing.assert_close(m, opt.state[p]["momentum_buffer"],
                                       rtol=1e-13, atol=1e-14)
        assert wb.dtype == torch.bfloat16
        assert torch.equal(wb, w.to(torch.float32).to(torch.bfloat16)) or \
            (wb.double() - w).abs().le(
                (w.to(torch.float32).to(torch.bfloat16).double() - w).abs()).all()
