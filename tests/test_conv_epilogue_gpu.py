"""Exact-integer tests of the conv_mfma epilogue and the split-K combine.

All operands are small integers (x in -2..2, w in -1..1, K <= 576, scale a
power of two, integer shift and residuals), so every partial sum and every
``acc*scale + shift`` is exact in fp32 whatever the summation order. The
expected output is a CPU float64 conv cast to fp32, the same fp32 epilogue
formula, then ``.bfloat16()`` — compared with ``torch.equal``, no tolerance.

x, w and the residuals come from skewed (non-symmetric) distributions and
most cases have Cin != Cout, so a transposed accumulator map cannot pass.
"""
import functools

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


def _draw(gen, shape, values, probs):
    idx = torch.multinomial(torch.tensor(probs), int(torch.Size(shape).numel()),
                            replacement=True, generator=gen)
    return torch.tensor(values, dtype=torch.float32)[idx].reshape(shape)


@functools.lru_cache(maxsize=None)
def _case(n, h, w_, cin, cout, k):
    """CPU inputs + the float64 conv reference (as fp32), computed once per
    shape and shared by every test that uses the shape. Treat as read-only."""
    gen = torch.Generator().manual_seed(1000 * cin + cout + 7 * h + k)
    x = _draw(gen, (n, cin, h, w_), [-2., -1., 0., 1., 2.],
              [0.10, 0.15, 0.20, 0.25, 0.30])
    w = _draw(gen, (cout, cin, k, k), [-1., 0., 1.], [0.2, 0.3, 0.5])
    acc = F.conv2d(x.double(), w.double(), padding=(k - 1) // 2).float()
    scale = _draw(gen, (cout,), [-2., -1., -.5, .5, 1., 2.],
                  [0.05, 0.10, 0.15, 0.20, 0.20, 0.30])
    shift = torch.randint(-8, 9, (cout,), generator=gen).float()
    res = [_draw(gen, (n, cout, h, w_),
                 [-4., -3., -2., -1., 0., 1., 2., 3., 4.],
                 [0.02, 0.04, 0.06, 0.08, 0.10, 0.15, 0.15, 0.20, 0.20])
           for _ in range(3)]
    return x, w, acc, scale, shift, res


def _expected(acc, scale, shift, res, full):
    if not full:
        return acc.bfloat16()
    v = acc * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    v = v + res[0]
    v = torch.where(v > 0, v, v * torch.tensor(0.01, dtype=torch.float32))
    v = v + res[1]
    v = v + res[2]
    return v.bfloat16()


def _offset_cl(t, offset_elems):
    """Device bf16 copy of NCHW ``t`` in channels_last storage that starts
    ``offset_elems`` elements into its allocation."""
    n, c, h, w_ = t.shape
    buf = torch.empty(t.numel() + offset_elems, device="cuda",
                      dtype=torch.bfloat16)
    view = buf[offset_elems:].view(n, h, w_, c).permute(0, 3, 1, 2)
    view.copy_(t)
    assert view.is_contiguous(memory_format=CL)
    return view


def _run(shape, full, dirty=False, res_offset=0):
    n, h, w_, cin, cout, k = shape
    x, w, acc, scale, shift, res = _case(*shape)
    xd = x.cuda().bfloat16().contiguous(memory_format=CL)
    wd = w.cuda().bfloat16()
    pad = (k - 1) // 2
    kwargs = {}
    if full:
        rd = [_offset_cl(r, res_offset) for r in res]
        if res_offset:
            assert all(r.data_ptr() % 16 == 2 * res_offset for r in rd)
        kwargs = dict(scale=scale.cuda(), shift=shift.cuda(), residual=rd[0],
                      act=True, residual_post=rd[1], residual_post2=rd[2])
    want = _expected(acc, scale, shift, res, full)
    outs = []
    for _ in range(2 if dirty else 1):
        if dirty:
            # dirty the allocator pool so empty() workspaces are non-zero
            junk = torch.full((64 << 20,), 3.3e7, device="cuda")
            del junk
        y = conv_kernels.conv_fwd(xd, wd, (1, 1), (pad, pad), (1, 1), **kwargs)
        assert y is not None and y.shape == want.shape
        outs.append(y.cpu())
    for y in outs:
        bad = (y.float() != want.float())
        assert torch.equal(y, want), \
            f"{shape} full={full}: {int(bad.sum())} of {bad.numel()} differ, " \
            f"first at {bad.nonzero()[:1].tolist()}"
    if dirty:
        assert torch.equal(outs[0], outs[1]), f"{shape}: runs differ"


# (n, h, w, cin, cout, k), split?  — M = n*h*w picks the tile
TILE_CASES = [
    pytest.param((1, 16, 16, 64, 64, 3), True, id="bm32-3x3-split9"),
    pytest.param((1, 16, 16, 64, 64, 1), False, id="bm32-1x1"),
    pytest.param((1, 64, 64, 128, 128, 1), True, id="bm64-1x1-split"),
    pytest.param((1, 64, 64, 64, 128, 1), False, id="bm64-1x1"),
    pytest.param((2, 112, 112, 64, 256, 1), False, id="128x128-392tiles"),
    pytest.param((1, 96, 96, 128, 256, 1), True, id="128x128-split"),
    pytest.param((2, 112, 112, 64, 192, 1), False, id="128x64"),
]


@pytest.mark.parametrize("full", [False, True], ids=["bare", "full"])
@pytest.mark.parametrize("shape,split", TILE_CASES)
def test_epilogue_tiles(shape, split, full):
    _run(shape, full, dirty=split)


@pytest.mark.parametrize("full", [False, True], ids=["bare", "full"])
@pytest.mark.parametrize("cout", [50, 52, 68, 77])
@pytest.mark.parametrize("split", [True, False], ids=["split", "unsplit"])
def test_epilogue_cout_tails(split, cout, full):
    shape = (1, 16, 16, 64, cout, 3) if split else (1, 64, 64, 64, cout, 1)
    _run(shape, full, dirty=split)


@pytest.mark.parametrize("full", [False, True], ids=["bare", "full"])
@pytest.mark.parametrize("cout", [40, 72])
def test_epilogue_cout_tails_lane_exchange(cout, full):
    """Cout % 8 == 0 but no multiple of 32: the last 8-channel groups of the
    16-byte-store path have no second fragment to trade for."""
    _run((1, 64, 64, 64, cout, 1), full)


@pytest.mark.parametrize("full", [False, True], ids=["bare", "full"])
@pytest.mark.parametrize("cout,k", [(64, 3), (128, 1), (50, 1)])
def test_epilogue_m_tail(cout, k, full):
    """M = 3*15*15 = 675 is no multiple of any tile height."""
    _run((3, 15, 15, 64, cout, k), full, dirty=(k == 3))


@pytest.mark.parametrize("shape,split", [
    pytest.param((1, 64, 64, 64, 128, 1), False, id="unsplit"),
    pytest.param((1, 64, 64, 128, 128, 1), True, id="split"),
])
def test_epilogue_residuals_offset_8_bytes(shape, split):
    """Residuals 8 bytes past a 16-byte boundary: legal for 8-byte accesses,
    not for 16-byte ones."""
    _run(shape, True, dirty=split, res_offset=4)


@pytest.mark.parametrize("stride", [1, 2])
def test_dgrad_exact(stride):
    """conv_dgrad runs the same kernel (zs = stride); K = 9*64 = 576."""
    gen = torch.Generator().manual_seed(77 + stride)
    cout, cin, hx = 64, 128, 16
    ho = hx // stride
    dy = _draw(gen, (1, cout, ho, ho), [-2., -1., 0., 1., 2.],
               [0.10, 0.15, 0.20, 0.25, 0.30])
    w = _draw(gen, (cout, cin, 3, 3), [-1., 0., 1.], [0.2, 0.3, 0.5])
    want = F.conv_transpose2d(dy.double(), w.double(), stride=stride, padding=1,
                              output_padding=stride - 1).float().bfloat16()
    dyd = dy.cuda().bfloat16().contiguous(memory_format=CL)
    wd = w.cuda().bfloat16()
    outs = []
    for _ in range(2):
        junk = torch.full((64 << 20,), 3.3e7, device="cuda")
        del junk
        dx = conv_kernels.conv_dgrad(dyd, wd, (1, cin, hx, hx),
                                     (stride, stride), (1, 1), (1, 1))
        assert dx is not None and dx.shape == want.shape
        outs.append(dx.cpu())
    assert torch.equal(outs[0], want)
    assert torch.equal(outs[0], outs[1])
