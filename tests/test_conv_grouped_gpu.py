"""Grouped conv launch: every member must equal its single call bit for bit.

A grouped member runs the plan it would get alone (same tile, split-K factor,
epilogue path and summation order), so the comparisons are ``torch.equal``
against ``conv_kernels.conv_fwd`` on random bf16 data. The five member sizes
are the five scales of a head layer shrunk to N=1: M = 9216 (BM=128), 2304
(BM=64), 576, 144 and 36 (BM=32; the last has rows past M inside its tile);
the tile, split and prefetch depth each member lands on are asserted through
the ``conv_mfma_tile_plan`` binding.
Before every grouped call a large allocation is filled with NaN and freed, so
an uninitialised or overlapping workspace sub-allocation shows up as NaN.

One mixed group is also checked against a CPU float64 conv with small-integer
operands (exact in fp32 whatever the summation order), which covers a bug
shared by the grouped and the single path.
"""
import pytest
import torch
import torch.nn.functional as F

# the member lists and the plans they must land on: shared with the CPU
# planner test
from conv_plan_cases import (EXACT_PLANS, EXACT_SPECS, G1, G1_BM, G3, G3_BM,
                             GL, GL_TILE_DEEP, GROUPS, TILE_CONFIGS)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd.ops import _backend, conv_kernels

CL = torch.channels_last


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"


def _dirty_pool():
    junk = torch.full((64 << 20,), float("nan"), device="cuda")
    del junk


def _member(gen, size, cin, cout, k, epi):
    """One conv problem on random bf16 data; ``epi`` is a subset of
    {scale, act, res, post, post2} ('scale' means scale AND shift)."""
    def rnd(*shape):
        return torch.randn(*shape, generator=gen)

    def act_map(c):
        return rnd(1, c, size, size).cuda().bfloat16().contiguous(
            memory_format=CL)

    m = dict(x=act_map(cin), weight=(rnd(cout, cin, k, k) * 0.1).cuda().bfloat16(),
             stride=(1, 1), padding=((k - 1) // 2,) * 2, dilation=(1, 1))
    if "scale" in epi:
        m["scale"] = (rnd(cout) * 0.5 + 1.0).cuda()
        m["shift"] = rnd(cout).cuda()
    if "act" in epi:
        m["act"] = True
    if "res" in epi:
        m["residual"] = act_map(cout)
    if "post" in epi:
        m["residual_post"] = act_map(cout)
    if "post2" in epi:
        m["residual_post2"] = act_map(cout)
    return m


def _plan(size, cin, cout, k, _epi=None):
    """(BM, BN, splitk, deep) the host plans for a member (N = 1)."""
    ext = _backend.hip_extension()
    return tuple(ext.conv_mfma_tile_plan(size * size, cout, k * k * cin))


def test_member_shapes_land_on_the_plans_the_groups_are_meant_to_mix():
    """The groups above only test what their names say while the planner
    keeps putting their members on these tiles and splits."""
    assert [_plan(*m)[0] for m in G3] == G3_BM == [128, 64, 32, 32, 32]
    assert [_plan(*m)[0] for m in G1] == G1_BM == [128, 64, 32, 32, 32]
    assert all(_plan(*m)[2] > 1 for m in G3)
    # 1x1 with Cin = 64 is a single K-chunk: unsplit beside split members
    assert [_plan(*m)[2] == 1 for m in G1] == [m[1] == 64 for m in G1]
    assert all(_plan(*m)[3] == 1 for m in G1)
    assert [_plan(*m)[:2] + _plan(*m)[3:] for m in GL] == GL_TILE_DEEP
    # every tile configuration of the grouped kernel's switch is exercised
    seen = {_plan(*m)[:2] + _plan(*m)[3:] for m in G3 + G1 + GL}
    assert seen == TILE_CONFIGS and len(TILE_CONFIGS) == 8
    # the exact-integer group: one unsplit non-DEEP member, split and
    # unsplit DEEP ones
    assert [_plan(s, ci, co, k) for s, ci, co, k, _ in EXACT_SPECS] \
        == EXACT_PLANS


@pytest.mark.parametrize("name", list(GROUPS))
def test_group_equals_single_calls(name):
    gen = torch.Generator().manual_seed(len(name) * 131 + 5)
    members = [_member(gen, *spec) for spec in GROUPS[name]]
    singles = []
    for m in members:
        y = conv_kernels.conv_fwd(**m)
        assert y is not None
        singles.append(y)
    for _ in range(2):
        _dirty_pool()
        ys = conv_kernels.conv_fwd_group(members)
        assert ys is not None and len(ys) == len(members)
        torch.cuda.synchronize()
        for i, (y, want) in enumerate(zip(ys, singles)):
            assert y.shape == want.shape
            assert not torch.isnan(y.float()).any(), f"{name}[{i}]: NaN"
            assert torch.equal(y, want), \
                f"{name}[{i}] {GROUPS[name][i]}: " \
                f"{int((y != want).sum())} of {y.numel()} differ"


def test_group_outputs_do_not_depend_on_list_order():
    """The grid orders problems by K-chunks per block; results must not."""
    gen = torch.Generator().manual_seed(99)
    members = [_member(gen, *spec) for spec in G3 + G1[:3]]
    _dirty_pool()
    fwd = conv_kernels.conv_fwd_group(members)
    _dirty_pool()
    rev = conv_kernels.conv_fwd_group(members[::-1])[::-1]
    for a, b in zip(fwd, rev):
        assert torch.equal(a, b)


def _draw(gen, shape, values, probs):
    idx = torch.multinomial(torch.tensor(probs), int(torch.Size(shape).numel()),
                            replacement=True, generator=gen)
    return torch.tensor(values, dtype=torch.float32)[idx].reshape(shape)


def test_group_exact_integers_vs_float64():
    """x in -2..2, w in -1..1, K <= 9*64 = 576, power-of-two scales, integer
    shifts and residuals: every partial sum and ``acc*scale + shift`` is exact
    in fp32, so the expected output is a CPU float64 conv through the fp32
    epilogue formula, compared without tolerance."""
    gen = torch.Generator().manual_seed(4242)
    specs = EXACT_SPECS
    members, wants = [], []
    for size, cin, cout, k, full in specs:
        x = _draw(gen, (1, cin, size, size), [-2., -1., 0., 1., 2.],
                  [0.10, 0.15, 0.20, 0.25, 0.30])
        w = _draw(gen, (cout, cin, k, k), [-1., 0., 1.], [0.2, 0.3, 0.5])
        acc = F.conv2d(x.double(), w.double(), padding=(k - 1) // 2).float()
        m = dict(x=x.cuda().bfloat16().contiguous(memory_format=CL),
                 weight=w.cuda().bfloat16(), stride=(1, 1),
                 padding=((k - 1) // 2,) * 2, dilation=(1, 1))
        if full:
            scale = _draw(gen, (cout,), [-2., -1., -.5, .5, 1., 2.],
                          [0.05, 0.10, 0.15, 0.20, 0.20, 0.30])
            shift = torch.randint(-8, 9, (cout,), generator=gen).float()
            res = [_draw(gen, (1, cout, size, size),
                         [-4., -3., -2., -1., 0., 1., 2., 3., 4.],
                         [0.02, 0.04, 0.06, 0.08, 0.10, 0.15, 0.15, 0.20, 0.20])
                   for _ in range(3)]
            rd = [r.cuda().bfloat16().contiguous(memory_format=CL) for r in res]
            m.update(scale=scale.cuda(), shift=shift.cuda(), residual=rd[0],
                     act=True, residual_post=rd[1], residual_post2=rd[2])
            v = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
            v = v + res[0]
            v = torch.where(v > 0, v,
                            v * torch.tensor(0.01, dtype=torch.float32))
            v = v + res[1]
            v = v + res[2]
            wants.append(v.bfloat16())
        else:
            wants.append(acc.bfloat16())
        members.append(m)
    _dirty_pool()
    ys = conv_kernels.conv_fwd_group(members)
    for spec, y, want in zip(specs, ys, wants):
        y = y.cpu()
        bad = y.float() != want.float()
        assert torch.equal(y, want), \
            f"{spec}: {int(bad.sum())} of {bad.numel()} differ, " \
            f"first at {bad.nonzero()[:1].tolist()}"


def test_posenet_grouped_heads_equal_per_conv_launches(monkeypatch):
    """nstack=2 also runs the merge_preds residual and the feature-cache
    adds. All 2 x 5 outputs must be bit-identical with IBP_CONV_GROUP=0."""
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
    img = torch.rand(1, 64, 64, 3, device="cuda", dtype=torch.bfloat16)
    calls = []
    real = conv_kernels.conv_fwd_group
    monkeypatch.setattr(conv_kernels, "conv_fwd_group",
                        lambda members: calls.append(len(members)) or
                        real(members))
    with torch.no_grad():
        monkeypatch.setenv("IBP_CONV_GROUP", "0")
        want = model(img)
        assert not calls, "IBP_CONV_GROUP=0 must not reach the grouped launch"
        monkeypatch.setenv("IBP_CONV_GROUP", "1")
        _dirty_pool()
        got = model(img)
    # head layers are groups of five — stack 0: conv1, conv2, outs,
    # merge_features, merge_preds; stack 1: conv1, conv2, outs
    assert [c for c in calls if c == 5] == [5] * 8
    assert len(got) == 2 and all(len(s) == 5 for s in got)
    for i in range(2):
        for j in range(5):
            assert got[i][j].shape == want[i][j].shape
            assert got[i][j].float().abs().max() > 0
            assert torch.equal(got[i][j], want[i][j]), f"stack {i} scale {j}"
