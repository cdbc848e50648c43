"""Tap-uniform gather of the MFMA conv (``ConvParams::gather``).

The gather only changes how the A and B tiles reach LDS: chunk boundaries,
the LDS image, the MFMA order, split-K slicing and the epilogues are the
generic kernel's, so every output must EQUAL the generic gather's bit for bit.
Every case therefore runs the op twice — ``IBP_CONV_GATHER`` unset and ``=0``
— and requires ``torch.equal``; and once against a CPU float64 conv on
small-integer operands (bf16 products and fp32 sums are exact, the one
rounding is float -> bf16 of an exactly known value), also ``torch.equal``.

The plan each case lands on (split, prefetch depth, gather) is asserted
through ``conv_mfma_conv_plan``, so a case keeps testing the path it is named
for: both main loops (DEEP and single-stage), slices that begin at a tap
boundary and inside a tap, all four tiles, the upfold bodies, the grouped
kernel's per-member choice, and the ineligible inputs that must stay on the
generic gather.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd.ops import _backend, conv_kernels

CL = torch.channels_last


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("IBP_CONV_GATHER", "IBP_CONV_BM", "IBP_SPLITK_TARGET"):
        monkeypatch.delenv(k, raising=False)


def _dirty_pool():
    junk = torch.full((64 << 20,), float("nan"), device="cuda")
    del junk


def _draw(gen, shape, values, probs):
    idx = torch.multinomial(torch.tensor(probs), int(torch.Size(shape).numel()),
                            replacement=True, generator=gen)
    return torch.tensor(values, dtype=torch.float32)[idx].reshape(shape)


def _ints(gen, shape):
    return _draw(gen, shape, [-2., -1., 0., 1., 2.],
                 [0.10, 0.15, 0.20, 0.25, 0.30])


def _signs(gen, shape):
    return _draw(gen, shape, [-1., 0., 1.], [0.2, 0.3, 0.5])


def _dev(t):
    return t.cuda().bfloat16().contiguous(memory_format=CL)


def _plan(x, weight, stride, padding, dilation):
    """[BM, BN, splitk, deep, gather] of conv_fwd(x, weight, ...) now."""
    args = conv_kernels._conv_args(x, conv_kernels.packed_weight(weight),
                                   weight.shape, stride, padding, dilation)
    return list(_backend.hip_extension().conv_mfma_conv_plan(*args[:3]))


def _both(monkeypatch, run):
    """run() with the planner's choice and with IBP_CONV_GATHER=0."""
    monkeypatch.delenv("IBP_CONV_GATHER", raising=False)
    _dirty_pool()
    on = run()
    monkeypatch.setenv("IBP_CONV_GATHER", "0")
    _dirty_pool()
    off = run()
    monkeypatch.delenv("IBP_CONV_GATHER", raising=False)
    torch.cuda.synchronize()
    return on, off


def _assert_equal(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape, what
    bad = got.float() != want.float()
    assert torch.equal(got, want), \
        f"{what}: {int(bad.sum())} of {bad.numel()} differ, " \
        f"first at {bad.nonzero()[:1].tolist()}"


def _check_conv(monkeypatch, seed, n, h, w, cin, cout, k, stride=1, dil=1,
                want_plan=None, want_gather=1, epi=False):
    gen = torch.Generator().manual_seed(seed)
    pad = dil * (k - 1) // 2
    x = _ints(gen, (n, cin, h, w))
    wt = _signs(gen, (cout, cin, k, k))
    acc = F.conv2d(x.double(), wt.double(), stride=stride, padding=pad,
                   dilation=dil).float()
    kw = {}
    want = acc
    if epi:
        # power-of-two scales, integer shifts and residuals: exact until the
        # activation; from there the kernel's fp32 formula in its order
        scale = _draw(gen, (cout,), [-2., -1., -.5, .5, 1., 2.],
                      [0.05, 0.10, 0.15, 0.20, 0.20, 0.30])
        shift = torch.randint(-8, 9, (cout,), generator=gen).float()
        res = [_draw(gen, tuple(acc.shape),
                     [-4., -3., -2., -1., 0., 1., 2., 3., 4.],
                     [0.02, 0.04, 0.06, 0.08, 0.10, 0.15, 0.15, 0.20, 0.20])
               for _ in range(3)]
        v = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        v = v + res[0]
        v = torch.where(v > 0, v, v * torch.tensor(0.01, dtype=torch.float32))
        want = (v + res[1]) + res[2]
        kw = dict(scale=scale.cuda(), shift=shift.cuda(), act=True,
                  residual=_dev(res[0]), residual_post=_dev(res[1]),
                  residual_post2=_dev(res[2]))
    want = want.bfloat16()
    xd, wd = _dev(x), wt.cuda().bfloat16()
    geo = ((stride, stride), (pad, pad), (dil, dil))
    plan = _plan(xd, wd, *geo)
    assert plan[4] == want_gather, plan
    if want_plan is not None:
        assert tuple(plan[:4]) == want_plan, plan
    monkeypatch.setenv("IBP_CONV_GATHER", "0")
    assert _plan(xd, wd, *geo) == plan[:4] + [0]
    on, off = _both(monkeypatch,
                    lambda: conv_kernels.conv_fwd(xd, wd, *geo, **kw))
    what = f"{n}x{cin}x{h}x{w} -> {cout} k{k} s{stride} d{dil} plan {plan}"
    _assert_equal(on, off, what + " (switch on vs off)")
    _assert_equal(on, want, what + " (vs float64)")
    return plan


# ---------------------------------------------------------------------------
# eligible convs
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("target,want", [(None, (32, 64, 9, 1)),
                                         ("1", (32, 64, 1, 0))])
def test_3x3_tile_larger_than_the_image(monkeypatch, target, want):
    """M = 35 is below every BM: rows past M, and every row has padding
    taps. Split 9 ways (one chunk per slice, DEEP) and unsplit (nk = 9,
    single-stage loop)."""
    if target:
        monkeypatch.setenv("IBP_SPLITK_TARGET", target)
    _check_conv(monkeypatch, 11, 1, 5, 7, 64, 64, 3, want_plan=want)


# nk_total = 18, 8 tiles. Slices of 5 chunks begin at k = 0, 320 (tap 2,
# second half), 640 (tap 5, its start), 960; slices of 9 at 0 and 576 (tap 4,
# second half).
NINE = [(None, (32, 64, 18, 1)), ("32", (32, 64, 4, 1)),
        ("16", (32, 64, 2, 0)), ("1", (32, 64, 1, 0))]


@pytest.mark.parametrize("target,want", NINE)
def test_3x3_tiles_span_images_cout_tail_two_chunks_per_tap(monkeypatch,
                                                            target, want):
    """N=3, 9x9: n changes inside a tile, Cout 40 has a tail, Cin 128 is two
    chunks per tap; the tap state starts at k_begin != 0 in the split runs."""
    if target:
        monkeypatch.setenv("IBP_SPLITK_TARGET", target)
    _check_conv(monkeypatch, 12, 3, 9, 9, 128, 40, 3, want_plan=want)


@pytest.mark.parametrize("target", [None, "1"])
@pytest.mark.parametrize("bm,cout,tile", [("32", 40, (32, 64)),
                                          ("64", 40, (64, 64)),
                                          ("128", 40, (128, 64)),
                                          ("128", 128, (128, 128))])
def test_every_tiles_staging_map(monkeypatch, bm, cout, tile, target):
    monkeypatch.setenv("IBP_CONV_BM", bm)
    if target:
        monkeypatch.setenv("IBP_SPLITK_TARGET", target)
    plan = _check_conv(monkeypatch, 13, 3, 9, 9, 128, cout, 3)
    assert tuple(plan[:2]) == tile
    assert plan[3] == (0 if target else 1)     # single-stage loop / DEEP


@pytest.mark.parametrize("target", [None, "1"])
def test_3x3_stride_2(monkeypatch, target):
    if target:
        monkeypatch.setenv("IBP_SPLITK_TARGET", target)
    _check_conv(monkeypatch, 14, 2, 10, 10, 64, 64, 3, stride=2)


@pytest.mark.parametrize("target", [None, "1"])
@pytest.mark.parametrize("dil", [3, 5])
def test_3x3_dilated(monkeypatch, dil, target):
    if target:
        monkeypatch.setenv("IBP_SPLITK_TARGET", target)
    _check_conv(monkeypatch, 15 + dil, 1, 12, 12, 64, 64, 3, dil=dil)


@pytest.mark.parametrize("epi", [False, True])
def test_1x1_deep(monkeypatch, epi):
    """One tap. nk_total = 3: DEEP; with a pre-activation residual and two
    post-activation residuals."""
    plan = _check_conv(monkeypatch, 21, 2, 6, 6, 192, 384, 1, epi=epi)
    assert plan[3] == 1
    monkeypatch.setenv("IBP_SPLITK_TARGET", "1")
    plan = _check_conv(monkeypatch, 22, 2, 6, 6, 192, 384, 1, epi=epi)
    assert plan[2:4] == [1, 1]


@pytest.mark.parametrize("cin,target,deep", [(64, None, 1), (128, "1", 0)])
def test_upfold(monkeypatch, cin, target, deep):
    """Four parity 2x2 convs with their own pad_h / pad_w and the scatter;
    Cin 128 unsplit runs the single-stage loop (nk = 8)."""
    if target:
        monkeypatch.setenv("IBP_SPLITK_TARGET", target)
    n, cout, h, w = 2, 64, 4, 6
    gen = torch.Generator().manual_seed(31 + cin)
    x = _draw(gen, (n, cin, h, w), [-1., 0., 1.], [0.15, 0.6, 0.25])
    wt = _draw(gen, (cout, cin, 3, 3), [-1., 0., 1.], [0.15, 0.6, 0.25])
    want = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"),
                    wt.double(), padding=1).float().bfloat16()
    xd, wd = _dev(x), wt.cuda().bfloat16()
    ext = _backend.hip_extension()
    tile = list(ext.conv_mfma_upfold_plan(n * h * w, cout, cin))
    assert tile[3] == deep
    # a parity as the planner sees it: 2x2 over the low-resolution map
    parity = [n, h, w, cin, cout, 2, 2, 1, 1, 1, 1, 1, h, w, 1]
    pack = conv_kernels.upfold_packed_weight(wd)
    assert list(ext.conv_mfma_conv_plan(xd, pack, parity))[4] == 1
    on, off = _both(monkeypatch, lambda: conv_kernels.upfold_fwd(xd, wd))
    _assert_equal(on, off, f"upfold Cin {cin} (switch on vs off)")
    _assert_equal(on, want, f"upfold Cin {cin} (vs float64)")


# ---------------------------------------------------------------------------
# ineligible inputs stay on the generic gather
# ---------------------------------------------------------------------------

def test_cin16_7x7_stride2_is_generic(monkeypatch):
    _check_conv(monkeypatch, 41, 2, 12, 12, 16, 64, 7, stride=2, want_gather=0)


def test_1x1_cin50_is_generic(monkeypatch):
    _check_conv(monkeypatch, 42, 2, 6, 6, 50, 64, 1, want_gather=0)


def test_dgrad_zs2_is_generic(monkeypatch):
    gen = torch.Generator().manual_seed(43)
    n, cin, cout, h, w = 2, 64, 64, 10, 10
    dy = _ints(gen, (n, cout, 5, 5))
    wt = _signs(gen, (cout, cin, 3, 3))
    want = torch.nn.grad.conv2d_input((n, cin, h, w), wt.double(), dy.double(),
                                      stride=2, padding=1).float().bfloat16()
    dyd, wd = _dev(dy), wt.cuda().bfloat16()
    args = conv_kernels._conv_args(
        dyd, conv_kernels.packed_weight_dgrad(wd), (cin, cout, 3, 3), (1, 1),
        (1, 1), (1, 1), zs=2, out_hw=(h, w))
    assert args[2][14] == 2
    plan = list(_backend.hip_extension().conv_mfma_conv_plan(*args[:3]))
    assert plan[4] == 0, plan
    on, off = _both(monkeypatch, lambda: conv_kernels.conv_dgrad(
        dyd, wd, (n, cin, h, w), (2, 2), (1, 1), (1, 1)))
    _assert_equal(on, off, "dgrad (switch on vs off)")
    _assert_equal(on, want, "dgrad (vs float64)")


def test_x_at_an_8_byte_aligned_pointer_is_generic(monkeypatch):
    """The data pointer of a channel slice that starts at channel 4: 8-byte
    but not 16-byte aligned. (Dense rows here; only the address matters.)"""
    gen = torch.Generator().manual_seed(44)
    n, cin, cout, h, w = 2, 64, 64, 6, 6
    x = _ints(gen, (n, cin, h, w))
    wt = _signs(gen, (cout, cin, 3, 3))
    want = F.conv2d(x.double(), wt.double(), padding=1).float().bfloat16()
    buf = torch.empty(n * h * w * cin + 4, dtype=torch.bfloat16, device="cuda")
    xd = buf[4:].view(n, h, w, cin)
    xd.copy_(x.permute(0, 2, 3, 1))
    xd = xd.permute(0, 3, 1, 2)
    assert xd.data_ptr() % 16 == 8 and xd.is_contiguous(memory_format=CL)
    wd = wt.cuda().bfloat16()
    geo = ((1, 1), (1, 1), (1, 1))
    assert _plan(xd, wd, *geo)[4] == 0
    assert _plan(_dev(x), wd, *geo)[4] == 1     # the aligned copy is eligible
    on, off = _both(monkeypatch, lambda: conv_kernels.conv_fwd(xd, wd, *geo))
    _assert_equal(on, off, "misaligned x (switch on vs off)")
    _assert_equal(on, want, "misaligned x (vs float64)")


# ---------------------------------------------------------------------------
# grouped launch: the kernel chooses per member
# ---------------------------------------------------------------------------

def test_group_mixes_eligible_and_ineligible_members(monkeypatch):
    """outs (Cin 64) beside merge_preds (Cin 50) at 8x8 ... 1x1 maps, and one
    3x3 member: each member equals its single launch and the oracle."""
    gen = torch.Generator().manual_seed(51)
    specs = [(8, 64, 50, 1), (8, 50, 64, 1), (4, 64, 64, 3), (2, 50, 64, 1),
             (1, 64, 50, 1)]
    members, wants, gathers = [], [], []
    for size, cin, cout, k in specs:
        x = _ints(gen, (1, cin, size, size))
        wt = _signs(gen, (cout, cin, k, k))
        wants.append(F.conv2d(x.double(), wt.double(),
                              padding=(k - 1) // 2).float().bfloat16())
        m = dict(x=_dev(x), weight=wt.cuda().bfloat16(), stride=(1, 1),
                 padding=((k - 1) // 2,) * 2, dilation=(1, 1))
        gathers.append(_plan(m["x"], m["weight"], m["stride"], m["padding"],
                             m["dilation"])[4])
        members.append(m)
    assert gathers == [1, 0, 1, 0, 1]
    singles = [conv_kernels.conv_fwd(**m) for m in members]
    on, off = _both(monkeypatch, lambda: conv_kernels.conv_fwd_group(members))
    assert on is not None and len(on) == len(off) == len(members)
    for i, spec in enumerate(specs):
        _assert_equal(on[i], singles[i], f"member {i} {spec} (vs single)")
        _assert_equal(on[i], off[i], f"member {i} {spec} (switch on vs off)")
        _assert_equal(on[i], wants[i], f"member {i} {spec} (vs float64)")


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------

def test_two_stack_model_outputs_equal_with_the_switch(monkeypatch,
                                                       small_config,
                                                       small_opt):
    from improved_body_parts_amd.models.posenet import PoseNet
    torch.manual_seed(7)
    model = PoseNet(small_opt.nstack, small_opt.hourglass_inp_dim,
                    small_config.num_layers, bn=True,
                    increase=small_opt.increase, init_weights=False)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    model = model.cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.float()
    model.eval()
    img = torch.rand(1, 64, 64, 3, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        on, off = _both(monkeypatch, lambda: model(img))
    assert len(on) == len(off) == 2 and all(len(s) == 5 for s in on)
    for i in range(2):
        for j in range(5):
            assert on[i][j].float().abs().max() > 0
            _assert_equal(on[i][j], off[i][j], f"stack {i} scale {j}")
