"""Two-source 1x1 conv: a Residual block's last conv with its projection
shortcut as one conv over K = mid + ins that reads both inputs.

The oracle everywhere is the two-branch layer as the model defines it —
``act(bn_a(conv_a(y)) + bn_b(conv_b(x)))`` with the ORIGINAL weights — in
float64 on the CPU.

* pack: ``pack_cat_weight`` equals the host reference bit for bit; one pack
  per version of anything that enters either fold;
* exact cases: operands in {-1, 0, 1}, power-of-two scales, integer shifts:
  every partial sum is exact whatever the order, so the output must EQUAL the
  oracle rounded to bf16, on every tile / split / depth the planner can pick
  and with the source boundary in each position of the K loop;
* precision: random operands, relative L2 error at most twice the bf16
  output-rounding floor of the oracle (expected sqrt(2): the scaled weight
  carries one more rounding of the same size as the output's);
* gates: everything outside the envelope runs the two calls, bit for bit;
* the model: errors against the fp32 run and the number of fused calls.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from test_cat_conv_cpu import CAT_PLANS

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd import ops
    from improved_body_parts_amd.ops import _backend, conv, conv_kernels

CL = torch.channels_last


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"


@pytest.fixture(autouse=True)
def _default_plans(monkeypatch):
    for k in ("IBP_CONV_BM", "IBP_SPLITK_TARGET", "IBP_SKIP_FOLD"):
        monkeypatch.delenv(k, raising=False)


def _dirty_pool():
    junk = torch.full((64 << 20,), float("nan"), device="cuda")
    del junk


def _draw(gen, shape, values, probs):
    idx = torch.multinomial(torch.tensor(probs), int(torch.Size(shape).numel()),
                            replacement=True, generator=gen)
    return torch.tensor(values, dtype=torch.float32)[idx].reshape(shape)


def _rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _cl_cuda(t):
    return t.cuda().bfloat16().contiguous(memory_format=CL)


# ---------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------

def _modules(cout, ca, cb, seed, bn=True):
    torch.manual_seed(seed)
    conv_a = torch.nn.Conv2d(ca, cout, 1, bias=not bn)
    conv_b = torch.nn.Conv2d(cb, cout, 1, bias=not bn)
    bns = []
    for _ in range(2):
        m = None
        if bn:
            m = torch.nn.BatchNorm2d(cout)
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 2.0)
            m.bias.data.normal_(0, 0.5)
            m = m.cuda().eval()
        bns.append(m)
    return (conv_a.cuda().bfloat16().eval(), bns[0],
            conv_b.cuda().bfloat16().eval(), bns[1])


def _bits(t):
    return t.cpu().view(torch.int16 if t.dtype == torch.bfloat16
                        else torch.int32)


@pytest.mark.parametrize("scales", [True, False], ids=["scales", "plain"])
@pytest.mark.parametrize("cout,ca,cb", [(40, 64, 64), (50, 256, 50)])
def test_pack_equals_reference_bit_for_bit(cout, ca, cb, scales):
    gen = torch.Generator().manual_seed(cout + ca + cb)
    wa = torch.randn(cout, ca, 1, 1, generator=gen).bfloat16()
    wb = torch.randn(cout, cb, 1, 1, generator=gen).bfloat16()
    vecs = [None] * 4
    if scales:
        vecs = [torch.rand(cout, generator=gen) * 1.5 + 0.25,
                -(torch.rand(cout, generator=gen) + 0.5),
                torch.randn(cout, generator=gen),
                torch.randn(cout, generator=gen)]
        vecs[3][::3] = -vecs[2][::3]          # shifts that cancel
    want_pack, want_shift = conv_kernels.cat_weight_reference(wa, wb, *vecs)
    _dirty_pool()
    pack, ones, shift = conv_kernels.cat_pack(
        None, wa.cuda(), wb.cuda(),
        *[None if v is None else v.cuda() for v in vecs])
    assert pack.shape == (cout, ca + cb)
    assert torch.equal(_bits(pack), _bits(want_pack))
    assert torch.equal(_bits(shift), _bits(want_shift))
    assert torch.equal(ones.cpu(), torch.ones(cout))


@pytest.mark.parametrize("bn", [True, False], ids=["bn", "bias"])
def test_fold_is_cached_per_version_of_everything_it_reads(bn):
    conv_a, bn_a, conv_b, bn_b = _modules(40, 64, 64, 11, bn=bn)

    def reference():
        fa = conv._branch_fold(conv_a, bn_a)
        fb = conv._branch_fold(conv_b, bn_b)
        return conv_kernels.cat_weight_reference(
            conv_a.weight.cpu(), conv_b.weight.cpu(),
            *[None if t is None else t.cpu()
              for t in (fa[0], fb[0], fa[1], fb[1])])

    first = conv.cat_fold(conv_a, bn_a, conv_b, bn_b)
    assert conv.cat_fold(conv_a, bn_a, conv_b, bn_b) is first
    want = reference()
    assert torch.equal(_bits(first[0]), _bits(want[0]))
    assert torch.equal(_bits(first[2]), _bits(want[1]))
    keyed = [conv_a.weight, conv_b.weight]
    for m, c in ((bn_a, conv_a), (bn_b, conv_b)):
        keyed += [m.weight, m.bias, m.running_mean, m.running_var] if bn \
            else [c.bias]
    assert len(keyed) == (10 if bn else 4)
    prev = first
    for t in keyed:
        with torch.no_grad():
            t.mul_(1.25)
        now = conv.cat_fold(conv_a, bn_a, conv_b, bn_b)
        assert now is not prev
        assert conv.cat_fold(conv_a, bn_a, conv_b, bn_b) is now
        want = reference()
        assert torch.equal(_bits(now[0]), _bits(want[0]))
        assert torch.equal(_bits(now[2]), _bits(want[1]))
        prev = now


# ---------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------

# (N, H, W), Ca, Cb, Cout, plan or None, full epilogue, residual_post
EXACT = [(nhw, ca, cb, cout, plan, i % 2 == 0, False)
         for i, (nhw, ca, cb, cout, plan, _) in enumerate(CAT_PLANS)]
EXACT[1] = EXACT[1][:5] + (True, True)      # split 3, boundary in slice 0
EXACT += [((1, 5, 7), 64, 50, 50, None, True, False),    # pair epilogue
          ((1, 5, 7), 256, 50, 384, None, False, False)]  # merge shape


@pytest.mark.parametrize(
    "case", EXACT, ids=[f"{c[0][0]}x{c[0][1]}x{c[0][2]}-{c[1]}+{c[2]}-{c[3]}"
                        for c in EXACT])
def test_exact_integers_vs_float64(case):
    (n, h, w), ca, cb, cout, plan, full, post = case
    if plan is not None:
        got = tuple(_backend.hip_extension().conv_mfma_tile_plan(
            n * h * w, cout, ca + cb))
        assert got == plan
    gen = torch.Generator().manual_seed(ca * 7 + cb + cout)
    vals, probs = [-1., 0., 1.], [0.15, 0.6, 0.25]
    a = _draw(gen, (n, ca, h, w), vals, probs)
    b = _draw(gen, (n, cb, h, w), vals, probs)
    wa = _draw(gen, (cout, ca, 1, 1), vals, probs)
    wb = _draw(gen, (cout, cb, 1, 1), [-2., -1., 0., 1., 2.],
               [0.05, 0.15, 0.5, 0.2, 0.1])
    acc_a = F.conv2d(a.double(), wa.double())
    acc_b = F.conv2d(b.double(), wb.double())
    vecs = [None] * 4
    want = acc_a + acc_b
    res = None
    if full:
        pows = [-2., -1., -.5, .5, 1., 2.]
        pp = [0.05, 0.10, 0.15, 0.20, 0.20, 0.30]
        vecs = [_draw(gen, (cout,), pows, pp), _draw(gen, (cout,), pows, pp),
                torch.randint(-8, 9, (cout,), generator=gen).float(),
                torch.randint(-8, 9, (cout,), generator=gen).float()]
        v = lambda t: t.double().view(1, -1, 1, 1)
        # exact up to here (integers and halves); from the activation on, the
        # kernel's fp32 formula in the kernel's order
        pre = (acc_a * v(vecs[0]) + v(vecs[2])
               + acc_b * v(vecs[1]) + v(vecs[3])).float()
        want = torch.where(pre > 0, pre,
                           pre * torch.tensor(0.01, dtype=torch.float32))
        if post:
            res = _draw(gen, (n, cout, h, w), [-4., -2., -1., 0., 1., 2., 3.],
                        [0.05, 0.1, 0.15, 0.3, 0.2, 0.1, 0.1])
            want = want + res
    # exactness premise: every partial sum is a multiple of 1/2 far inside
    # fp32's 24 bits, in any order and across split-K slabs
    assert float((acc_a.abs() + acc_b.abs()).max()) <= 1024
    assert float(want.abs().max()) <= 4096
    want = want.float().bfloat16()
    _dirty_pool()
    pack, ones, shift = conv_kernels.cat_pack(
        None, wa.cuda().bfloat16(), wb.cuda().bfloat16(),
        *[None if t is None else t.cuda() for t in vecs])
    y = conv_kernels.conv_cat_fwd(
        _cl_cuda(a), wa, _cl_cuda(b), wb, pack, scale=ones, shift=shift,
        act=full, residual_post=None if res is None else _cl_cuda(res))
    torch.cuda.synchronize()
    assert y.shape == (n, cout, h, w)
    y = y.cpu()
    bad = y.float() != want.float()
    assert torch.equal(y, want), \
        f"{int(bad.sum())} of {bad.numel()} differ, " \
        f"first at {bad.nonzero()[:1].tolist()}"


# ---------------------------------------------------------------------------
# precision: random operands, the op against the float64 layer
# ---------------------------------------------------------------------------

def _two_calls(y, conv_a, bn_a, x, conv_b, bn_b, act, training=False):
    """The layer as it ran before the fused op existed."""
    residual = ops.conv_bn_act(x, conv_b, bn_b, act=False, training=training)
    return ops.conv_bn_add_act(y, conv_a, bn_a, residual, act=act,
                               training=training)


def _layer_f64(y, conv_a, bn_a, x, conv_b, bn_b, act):
    def branch(t, c, m):
        out = F.conv2d(t.double().cpu(), c.weight.double().cpu())
        return F.batch_norm(out, m.running_mean.double().cpu(),
                            m.running_var.double().cpu(),
                            m.weight.double().cpu(), m.bias.double().cpu(),
                            False, 0.0, m.eps)
    out = branch(y, conv_a, bn_a) + branch(x, conv_b, bn_b)
    return F.leaky_relu(out, 0.01) if act else out


def _spy(monkeypatch):
    calls = []
    real = conv_kernels.conv_cat_fwd
    monkeypatch.setattr(conv_kernels, "conv_cat_fwd",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.parametrize("n,h,w,ca,cb,cout", [(2, 16, 16, 320, 512, 640),
                                              (1, 5, 7, 64, 64, 40)])
def test_precision_within_twice_the_bf16_floor(n, h, w, ca, cb, cout,
                                               monkeypatch):
    conv_a, bn_a, conv_b, bn_b = _modules(cout, ca, cb, n * 31 + ca)
    gen = torch.Generator().manual_seed(ca + cb)
    y = _cl_cuda(torch.randn(n, ca, h, w, generator=gen))
    x = _cl_cuda(torch.randn(n, cb, h, w, generator=gen))
    oracle = _layer_f64(y, conv_a, bn_a, x, conv_b, bn_b, True)
    floor = _rel_l2(oracle.float().bfloat16(), oracle)
    calls = _spy(monkeypatch)
    _dirty_pool()
    with torch.no_grad():
        fused = ops.conv_bn_add_conv_bn_act(y, conv_a, bn_a, x, conv_b, bn_b,
                                            act=True, training=False)
        assert len(calls) == 1
        two = _two_calls(y, conv_a, bn_a, x, conv_b, bn_b, True)
    err, err_two = _rel_l2(fused.cpu(), oracle), _rel_l2(two.cpu(), oracle)
    print(f"\ncat precision {n}x{h}x{w} {ca}+{cb}->{cout}: floor {floor:.3e}, "
          f"two-call {err_two:.3e} ({err_two / floor:.3f}x), "
          f"fused {err:.3e} ({err / floor:.3f}x)")
    assert not torch.isnan(fused.float()).any()
    assert err <= 2.0 * floor


# ---------------------------------------------------------------------------
# gates: outside the envelope it is the two calls
# ---------------------------------------------------------------------------

def _inputs(ca, cb, dtype=torch.bfloat16, nhw=(2, 6, 5)):
    gen = torch.Generator().manual_seed(ca + cb)
    n, h, w = nhw
    return [torch.randn(n, c, h, w, generator=gen).cuda().to(dtype)
            .contiguous(memory_format=CL) for c in (ca, cb)]


def test_gates_run_the_two_calls(monkeypatch):
    calls = _spy(monkeypatch)
    mods = _modules(64, 64, 64, 5)
    y, x = _inputs(64, 64)
    with torch.no_grad():
        want = _two_calls(y, *mods[:2], x, *mods[2:], True)
        fused = ops.conv_bn_add_conv_bn_act(y, *mods[:2], x, *mods[2:],
                                            act=True, training=False)
        assert len(calls) == 1 and _rel_l2(fused, want) < 2e-2
        # the switch, read at call time
        monkeypatch.setenv("IBP_SKIP_FOLD", "0")
        off = ops.conv_bn_add_conv_bn_act(y, *mods[:2], x, *mods[2:],
                                          act=True, training=False)
        assert len(calls) == 1 and torch.equal(off, want)
        monkeypatch.delenv("IBP_SKIP_FOLD")
        # Cin % 64 != 0 (48 + 64)
        m48 = _modules(64, 48, 64, 6)
        y48, x48 = _inputs(48, 64)
        got = ops.conv_bn_add_conv_bn_act(y48, *m48[:2], x48, *m48[2:],
                                          act=True, training=False)
        assert len(calls) == 1
        assert torch.equal(got, _two_calls(y48, *m48[:2], x48, *m48[2:], True))
        # training-mode BN: batch statistics, whatever the running ones
        # are. Two rows: the statistics kernel adds per-block partial sums
        # with atomics, and two terms give the same sum in either order.
        for m in (mods[1], mods[3]):
            m.train()
        y2, x2 = _inputs(64, 64, nhw=(1, 1, 2))
        got = ops.conv_bn_add_conv_bn_act(y2, *mods[:2], x2, *mods[2:],
                                          act=True, training=True)
        assert len(calls) == 1
        assert torch.equal(got, _two_calls(y2, *mods[:2], x2, *mods[2:], True,
                                           training=True))
        for m in (mods[1], mods[3]):
            m.eval()
        # fp32 input
        f32 = [None if m is None else copy.deepcopy(m).float() for m in mods]
        yf, xf = _inputs(64, 64, torch.float32)
        got = ops.conv_bn_add_conv_bn_act(yf, *f32[:2], xf, *f32[2:],
                                          act=True, training=False)
        assert len(calls) == 1
        assert torch.equal(got, _two_calls(yf, *f32[:2], xf, *f32[2:], True))
    # grad enabled: the autograd path
    got = ops.conv_bn_add_conv_bn_act(y, *mods[:2], x, *mods[2:], act=True,
                                      training=False)
    assert len(calls) == 1 and got.requires_grad
    assert torch.equal(got.detach(),
                       _two_calls(y, *mods[:2], x, *mods[2:], True).detach())


def test_unequal_cout_is_outside_the_envelope():
    """Decided on the shapes alone: with unequal Cout the two calls have no
    defined result either (the shortcut would not fit the add), so nothing
    is launched here."""
    y, x = _inputs(64, 64)
    wa = torch.empty(64, 64, 1, 1, device="cuda", dtype=torch.bfloat16)
    wb = torch.empty(32, 64, 1, 1, device="cuda", dtype=torch.bfloat16)
    assert conv_kernels.cat_supported(y, wa, x, wa)
    assert not conv_kernels.cat_supported(y, wa, x, wb)
    assert not conv_kernels.cat_supported(y, wa, x[:, :, :3], wa)
    assert not conv_kernels.cat_supported(y.float(), wa, x, wa)


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def posenet():
    from improved_body_parts_amd.models.posenet import PoseNet
    torch.manual_seed(7)
    model = PoseNet(2, 128, 50, bn=True, increase=128, init_weights=False)
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
    img = torch.rand(1, 128, 128, 3, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        ref_out = ref(img.float().cpu())
    return model, img, ref_out


def test_posenet_fold_on_within_twice_the_fold_off_error(posenet, monkeypatch):
    model, img, ref_out = posenet
    calls = _spy(monkeypatch)
    with torch.no_grad():
        monkeypatch.setenv("IBP_SKIP_FOLD", "0")
        off = model(img)
        assert not calls
        monkeypatch.setenv("IBP_SKIP_FOLD", "1")
        _dirty_pool()
        on = model(img)
    # hg[d][1] and hg[d][2], four depths, two stacks: their mids 64 .. 320 are
    # multiples of 64; pre.res1 (32 -> 64, mid 32) keeps its two calls
    assert len(calls) == 16
    for i in range(2):
        for j in range(5):
            e_off = _rel_l2(off[i][j].cpu(), ref_out[i][j])
            e_on = _rel_l2(on[i][j].cpu(), ref_out[i][j])
            print(f"\nstack {i} scale {j}: fold off {e_off:.3e}, "
                  f"on {e_on:.3e} ({e_on / e_off:.3f}x)")
            assert not torch.isnan(on[i][j].float()).any()
            assert e_on <= 2.0 * e_off, f"stack {i} scale {j}"
