"""Nearest-x2 upsample folded into the hourglass refine conv (four 2x2 convs).

The oracle everywhere is the layer as the model defines it — upsample, 3x3
conv with the ORIGINAL weights, epilogue — in float64 on the CPU.

* pack: ``pack_upfold_weight`` equals the host fold bit for bit;
* plans: the shapes below reach the tile / split / epilogue paths they are
  named for (``conv_mfma_upfold_plan``);
* integers: x, W in {-1, 0, 1}, power-of-two scales, integer shifts and
  residuals, |y| <= 256: every value is exact whatever the order, so the
  output must EQUAL the oracle — folded weights are then small integers too;
* precision: random operands, relative L2 error at most twice the bf16
  output-rounding floor of the oracle (expected sqrt(2): the folded weight
  carries one more rounding of the same size as the output's);
* fallback and the model-level switch.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

# the integer cases and the plans they must land on: shared with the CPU
# planner test
from conv_plan_cases import (INT_CASES, UPFOLD_CASE_PLANS,
                             UPFOLD_CASE_PLANS_TARGET_1, UPFOLD_SHAPE_PLANS,
                             UPFOLD_SPLITS_BELOW_12)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd import ops
    from improved_body_parts_amd.ops import _backend, conv_kernels

CL = torch.channels_last


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"


def _dirty_pool():
    junk = torch.full((64 << 20,), float("nan"), device="cuda")
    del junk


def _draw(gen, shape, values, probs):
    idx = torch.multinomial(torch.tensor(probs), int(torch.Size(shape).numel()),
                            replacement=True, generator=gen)
    return torch.tensor(values, dtype=torch.float32)[idx].reshape(shape)


def _plan(n, cin, cout, h, w):
    return tuple(_backend.hip_extension().conv_mfma_upfold_plan(
        n * h * w, cout, cin))


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


# ---------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("cout,cin", [(40, 64), (7, 24)])
def test_pack_equals_host_fold_bit_for_bit(cout, cin):
    gen = torch.Generator().manual_seed(cout * 1000 + cin)
    w = torch.randn(cout, cin, 3, 3, generator=gen)
    # cancelling sums: neighbours that add to zero exactly, or to a value
    # far below either term (the fp32 sum keeps it, the order matters)
    w[0::3, :, :, 1] = -w[0::3, :, :, 0]
    w[1::3, :, 1, :] = -w[1::3, :, 0, :] * (1 + 2.0 ** -7)
    w[2::3, :, 2, 2] = 2.0 ** -12
    w = w.bfloat16()
    want = conv_kernels.upfold_weight_reference(w).reshape(4, cout, 4 * cin)
    _dirty_pool()
    out = torch.empty(4, cout, 4 * cin, dtype=torch.bfloat16, device="cuda")
    _backend.hip_extension().pack_upfold_weight(w.cuda(), out)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    # the cached entry point returns the same pack, once per weight version
    wc = w.cuda()
    p1 = conv_kernels.upfold_packed_weight(wc)
    assert torch.equal(p1.cpu().view(torch.int16), want.view(torch.int16))
    assert conv_kernels.upfold_packed_weight(wc) is p1
    wc.mul_(2)
    p2 = conv_kernels.upfold_packed_weight(wc)
    assert p2 is not p1 and torch.equal(p2.float(), p1.float() * 2)


# ---------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------

def test_cases_hit_the_paths_they_are_named_for(monkeypatch):
    monkeypatch.delenv("IBP_SPLITK_TARGET", raising=False)
    monkeypatch.delenv("IBP_CONV_BM", raising=False)
    # the workload's four refine convs, batch 4: one plan for all parities,
    # from M = 4 * M_low rows and 4 * ntiles tiles
    # ... and the precision shape: 2 x 256 -> 256 at 16 x 16, non-DEEP split
    assert len(UPFOLD_SHAPE_PLANS) == 5
    for shape, want in UPFOLD_SHAPE_PLANS:
        assert _plan(*shape) == want, shape
    by_name = {c[0]: c for c in INT_CASES}

    def plan_of(name):
        _, n, cin, cout, h, w, *_ = by_name[name]
        return _plan(n, cin, cout, h, w)

    assert set(UPFOLD_CASE_PLANS) == {
        "5x7-split", "8x8-split", "16x24-cout72", "32x32-unsplit",
        "8x8-res-off8"}
    for name, want in UPFOLD_CASE_PLANS.items():
        assert plan_of(name) == want, name
    assert _plan(*UPFOLD_SPLITS_BELOW_12)[2] > 1  # one image fewer splits
    monkeypatch.setenv("IBP_SPLITK_TARGET", "1")
    assert set(UPFOLD_CASE_PLANS_TARGET_1) == {"5x7-unsplit",
                                               "5x7-cout33-unsplit"}
    for name, want in UPFOLD_CASE_PLANS_TARGET_1.items():
        assert plan_of(name) == want, name


# ---------------------------------------------------------------------------
# integer cases: exact equality with the float64 oracle
# ---------------------------------------------------------------------------

def _offset_copy(t_cl_nchw, offset_bytes):
    """The same NCHW-shaped channels_last values at a data pointer moved by
    ``offset_bytes`` from a fresh (256-byte aligned) allocation."""
    if not offset_bytes:
        return t_cl_nchw
    n, c, h, w = t_cl_nchw.shape
    k = offset_bytes // 2
    buf = torch.empty(n * h * w * c + k, dtype=t_cl_nchw.dtype, device="cuda")
    view = buf[k:].view(n, h, w, c)
    view.copy_(t_cl_nchw.permute(0, 2, 3, 1))
    out = view.permute(0, 3, 1, 2)
    assert out.data_ptr() % 16 == offset_bytes % 16
    return out


@pytest.mark.parametrize("case", INT_CASES, ids=[c[0] for c in INT_CASES])
def test_exact_integers_vs_float64(case, monkeypatch):
    name, n, cin, cout, h, w, res_off, sk_target, full = case
    if sk_target is None:
        monkeypatch.delenv("IBP_SPLITK_TARGET", raising=False)
    else:
        monkeypatch.setenv("IBP_SPLITK_TARGET", sk_target)
    gen = torch.Generator().manual_seed(len(name) * 977 + cout)
    x = _draw(gen, (n, cin, h, w), [-1., 0., 1.], [0.15, 0.6, 0.25])
    wt = _draw(gen, (cout, cin, 3, 3), [-1., 0., 1.], [0.15, 0.6, 0.25])
    acc = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"),
                   wt.double(), padding=1)
    kw = {}
    want = acc
    if full:
        scale = _draw(gen, (cout,), [-2., -1., -.5, .5, 1., 2.],
                      [0.05, 0.10, 0.15, 0.20, 0.20, 0.30])
        shift = torch.randint(-8, 9, (cout,), generator=gen).float()
        res = [_draw(gen, (n, cout, 2 * h, 2 * w),
                     [-4., -3., -2., -1., 0., 1., 2., 3., 4.],
                     [0.02, 0.04, 0.06, 0.08, 0.10, 0.15, 0.15, 0.20, 0.20])
               for _ in range(2)]
        # acc * scale + shift is exact (integers, power-of-two scales); from
        # the activation on, the kernel's fp32 formula in the kernel's order
        v = (acc * scale.double().view(1, -1, 1, 1)
             + shift.double().view(1, -1, 1, 1)).float()
        v = torch.where(v > 0, v, v * torch.tensor(0.01, dtype=torch.float32))
        want = (v + res[0]) + res[1]
        rd = [_offset_copy(r.cuda().bfloat16().contiguous(memory_format=CL),
                           res_off) for r in res]
        kw = dict(scale=scale.cuda(), shift=shift.cuda(), act=True,
                  residual_post=rd[0], residual_post2=rd[1])
    # exactness premise: small integers, far inside fp32 and bf16
    assert float(acc.abs().max()) <= 256 and float(want.abs().max()) <= 256
    want = want.float().bfloat16()
    _dirty_pool()
    y = conv_kernels.upfold_fwd(
        x.cuda().bfloat16().contiguous(memory_format=CL),
        wt.cuda().bfloat16(), **kw)
    torch.cuda.synchronize()
    assert y.shape == (n, cout, 2 * h, 2 * w)
    y = y.cpu()
    bad = y.float() != want.float()
    assert torch.equal(y, want), \
        f"{name}: {int(bad.sum())} of {bad.numel()} differ, " \
        f"first at {bad.nonzero()[:1].tolist()}"
    # and the two-call path computes the same values on these operands
    two = conv_kernels.conv_fwd(
        ops.upsample2x_nearest(
            x.cuda().bfloat16().contiguous(memory_format=CL)),
        wt.cuda().bfloat16(), (1, 1), (1, 1), (1, 1), **kw)
    assert torch.equal(two.cpu(), want)


# ---------------------------------------------------------------------------
# precision: random operands
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 256, 256, 16, 16),
                                            (1, 64, 40, 5, 7)])
def test_precision_within_twice_the_bf16_floor(n, cin, cout, h, w):
    gen = torch.Generator().manual_seed(n * 31 + cin)
    x = torch.randn(n, cin, h, w, generator=gen).bfloat16()
    wt = (0.05 * torch.randn(cout, cin, 3, 3, generator=gen)).bfloat16()
    oracle = F.conv2d(F.interpolate(x.double(), scale_factor=2,
                                    mode="nearest"), wt.double(), padding=1)
    floor = _rel_l2(oracle.float().bfloat16(), oracle)
    _dirty_pool()
    xd = x.cuda().contiguous(memory_format=CL)
    y = conv_kernels.upfold_fwd(xd, wt.cuda())
    two = conv_kernels.conv_fwd(ops.upsample2x_nearest(xd), wt.cuda(),
                                (1, 1), (1, 1), (1, 1))
    err = _rel_l2(y.cpu(), oracle)
    err_two = _rel_l2(two.cpu(), oracle)
    print(f"\nupfold precision {n}x{cin}->{cout} @{h}x{w}: floor {floor:.3e}, "
          f"two-call {err_two:.3e} ({err_two / floor:.3f}x), "
          f"folded {err:.3e} ({err / floor:.3f}x)")
    assert err <= 2.0 * floor


# ---------------------------------------------------------------------------
# op-level gate and fallback
# ---------------------------------------------------------------------------

def _conv_bn(cin, cout, seed):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1, bias=False)
    bn = torch.nn.BatchNorm2d(cout)
    bn.running_mean.normal_(0, 0.1)
    bn.running_var.uniform_(0.5, 1.5)
    return conv.cuda().bfloat16().eval(), bn.cuda().eval()


def _spy(monkeypatch):
    calls = []
    real = conv_kernels.upfold_fwd
    monkeypatch.setattr(conv_kernels, "upfold_fwd",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.parametrize("cin,cout", [(64, 50), (48, 64)])
def test_outside_the_envelope_runs_the_two_calls(cin, cout, monkeypatch):
    monkeypatch.delenv("IBP_UPCONV_FOLD", raising=False)
    conv, bn = _conv_bn(cin, cout, 3)
    calls = _spy(monkeypatch)
    low = torch.randn(2, cin, 6, 5, device="cuda").bfloat16() \
        .contiguous(memory_format=CL)
    post = torch.randn(2, cout, 12, 10, device="cuda").bfloat16() \
        .contiguous(memory_format=CL)
    with torch.no_grad():
        got = ops.upsample_conv_bn_act(low, conv, bn, act=True,
                                       residual_post=post)
        want = ops.conv_bn_act(ops.upsample2x_nearest(low), conv, bn,
                               act=True, training=False, residual_post=post)
    assert not calls
    assert torch.equal(got, want)


def test_gate_switch_grad_and_training(monkeypatch):
    monkeypatch.delenv("IBP_UPCONV_FOLD", raising=False)
    conv, bn = _conv_bn(64, 64, 5)
    calls = _spy(monkeypatch)
    low = torch.randn(1, 64, 6, 5, device="cuda").bfloat16() \
        .contiguous(memory_format=CL)
    with torch.no_grad():
        want = ops.conv_bn_act(ops.upsample2x_nearest(low), conv, bn,
                               act=True, training=False)
        folded = ops.upsample_conv_bn_act(low, conv, bn, act=True)
        assert len(calls) == 1
        assert _rel_l2(folded, want) < 2e-2 and not torch.isnan(folded).any()
        monkeypatch.setenv("IBP_UPCONV_FOLD", "0")
        off = ops.upsample_conv_bn_act(low, conv, bn, act=True)
        assert len(calls) == 1 and torch.equal(off, want)
        monkeypatch.setenv("IBP_UPCONV_FOLD", "1")
    # grad enabled: the autograd path, two calls
    with_grad = ops.upsample_conv_bn_act(low, conv, bn, act=True)
    assert len(calls) == 1 and with_grad.shape == want.shape


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def posenet():
    from improved_body_parts_amd.models.posenet import PoseNet
    torch.manual_seed(7)
    model = PoseNet(2, 64, 50, bn=True, increase=32, init_weights=False)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    model = model.cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.float()
    model.eval()
    # the same (bf16-rounded) parameters in fp32, eager on the CPU
    ref = copy.deepcopy(model).float().cpu().eval()
    img = torch.rand(1, 64, 64, 3, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        ref_out = ref(img.float().cpu())
    return model, img, ref_out


def test_fold_off_is_the_two_calls_on_one_hourglass_level(posenet, monkeypatch):
    model, _, _ = posenet
    hg = model.hourglass[0]
    calls = _spy(monkeypatch)
    x = torch.randn(1, 64, 16, 16, device="cuda").bfloat16() \
        .contiguous(memory_format=CL)
    post = torch.randn(1, 64, 16, 16, device="cuda").bfloat16() \
        .contiguous(memory_format=CL)
    monkeypatch.setenv("IBP_UPCONV_FOLD", "0")
    with torch.no_grad():
        got = hg._forward(0, x, [], post)
        # the level by hand, as it was before the fold existed
        up1 = hg.hg[0][0](x)
        low1 = hg.hg[0][1](ops.maxpool2x2(x))
        low2 = hg._forward(1, low1, [])
        low3 = hg.hg[0][2](low2)
        up2 = ops.upsample2x_nearest(low3)
        want = hg.hg[0][3](up2, residual_post=up1, residual_post2=post)
    assert not calls
    assert torch.equal(got, want)


def test_posenet_fold_on_within_twice_the_fold_off_error(posenet, monkeypatch):
    model, img, ref_out = posenet
    calls = _spy(monkeypatch)
    with torch.no_grad():
        monkeypatch.setenv("IBP_UPCONV_FOLD", "0")
        off = model(img)
        assert not calls
        monkeypatch.setenv("IBP_UPCONV_FOLD", "1")
        _dirty_pool()
        on = model(img)
    # channels 64 / 96 / 128 / 160: levels 0 and 2 of both stacks fold
    assert len(calls) == 4
    for i in range(2):
        for j in range(5):
            e_off = _rel_l2(off[i][j].cpu(), ref_out[i][j])
            e_on = _rel_l2(on[i][j].cpu(), ref_out[i][j])
            print(f"\nstack {i} scale {j}: fold off {e_off:.3e}, "
                  f"on {e_on:.3e} ({e_on / e_off:.3f}x)")
            assert not torch.isnan(on[i][j].float()).any()
            assert e_on <= 2.0 * e_off, f"stack {i} scale {j}"
