"""Direct tests of ``conv_wgrad.hip`` against the fp64 oracle
``train_oracle.wgrad`` (validated on the CPU by ``test_train_oracle.py``).

* Coverage cases use x in {-1, 0, 1} and dy in {-1, 0, 1} with a non-zero in
  every row m, sized so that the fp64 ``max|dW| <= 256``: every partial sum
  is then a small integer, exact in fp32 in any order and exact in the bf16
  output, so dW must EQUAL the oracle. One dropped or doubled row m, a stage
  that is not consumed, a workspace slice that is not written or a mis-reduced
  tree group changes at least one element.
* Every case is pinned to the launch plan it is built for through the debug
  op ``conv_wgrad_plan`` (run with the ``IBP_WGRAD_*`` variables unset).
* Precision cases use randn-based bf16 data and bound every element from the
  kernel's fp32 accumulation (u = 2**-24).
"""
import os

import pytest
import torch

import train_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd.ops import _backend, conv_kernels

BF16, F64 = torch.bfloat16, torch.float64
U = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"
    set_ = [k for k in os.environ if k.startswith("IBP_WGRAD_")]
    assert not set_, f"these tests pin the default plans; unset {set_}"


def _ext():
    return _backend.hip_extension()


def _dirty():
    """Leave junk in the caching allocator's free blocks (large and small
    pool) so that an ``empty()`` workspace is not zero by luck."""
    junk = [torch.full((16 << 20,), 3.3e7, device="cuda")]
    junk += [torch.full((1 << 20,), 3.3e7, device="cuda") for _ in range(4)]
    junk += [torch.full((n,), 3.3e7, device="cuda")
             for n in (64, 512, 4096, 1 << 15, 1 << 17) for _ in range(4)]
    del junk


class Case:
    def __init__(self, name, N, Cin, Cout, H, W, KH, KW, s, pad, dil, plan,
                 dy_nnz=0):
        self.name = name
        self.N, self.Cin, self.Cout, self.H, self.W = N, Cin, Cout, H, W
        self.KH, self.KW, self.s, self.pad, self.dil = KH, KW, s, pad, dil
        self.Ho = (H + 2 * pad[0] - dil[0] * (KH - 1) - 1) // s + 1
        self.Wo = (W + 2 * pad[1] - dil[1] * (KW - 1) - 1) // s + 1
        self.M = N * self.Ho * self.Wo
        self.KD = KH * KW * Cin
        # [TKD, TCO, waves, elem, kd_cb, chunks, chunk_len, tree groups...]
        self.plan = plan
        # 0: dense {-1, 0, 1} dy rows; 1 / 2: at most that many +-1 per row
        self.dy_nnz = dy_nnz
        self.w_shape = (Cout, Cin, KH, KW)


# chunk_len = 64 * stages; the last chunk of 67x63 holds 2109 rows, of
# 257x256 and 256x257 320 rows
CASES = [
    Case("m35-partial-stage", 1, 16, 16, 5, 7, 3, 3, 1, (1, 1), (1, 1),
         [64, 64, 4, 1, 0, 1, 64]),
    Case("1x1-2chunks-even-stages", 1, 16, 16, 64, 64, 1, 1, 1, (0, 0), (1, 1),
         [64, 64, 4, 1, 0, 2, 2048]),
    Case("67x63-odd-stages-ragged", 1, 32, 24, 67, 63, 3, 3, 1, (1, 1), (1, 1),
         [64, 64, 4, 1, 0, 2, 2112]),
    Case("clean-reorder-kdcb2", 2, 128, 64, 16, 16, 3, 3, 1, (1, 1), (1, 1),
         [64, 64, 4, 0, 2, 1, 512]),
    Case("1x3-unequal-pad-cout40", 2, 64, 40, 12, 20, 1, 3, 1, (0, 1), (1, 1),
         [64, 64, 4, 0, 1, 1, 512]),
    Case("head-cout50", 2, 256, 50, 32, 32, 1, 1, 1, (0, 0), (1, 1),
         [64, 64, 4, 0, 0, 1, 2048]),
    Case("cin50-3x3-tap-walk", 2, 50, 50, 24, 16, 3, 3, 1, (1, 1), (1, 1),
         [64, 64, 4, 1, 0, 1, 768]),
    Case("cin3-7x7-s2-odd-h", 2, 3, 64, 37, 45, 7, 7, 2, (3, 3), (1, 1),
         [64, 64, 4, 1, 0, 1, 896]),
    Case("3x3-s2", 2, 16, 32, 33, 30, 3, 3, 2, (1, 1), (1, 1),
         [64, 64, 4, 1, 0, 1, 512]),
    Case("dil35-pad35-wo72", 1, 32, 16, 40, 72, 3, 3, 1, (3, 5), (3, 5),
         [64, 64, 4, 1, 0, 1, 2880]),
    Case("wo100-step-dho0", 1, 16, 16, 9, 100, 3, 3, 1, (1, 1), (1, 1),
         [64, 64, 4, 1, 0, 1, 960]),
    Case("wo1-stage-spans-21-images", 70, 16, 16, 3, 1, 3, 3, 1, (1, 1), (1, 1),
         [64, 64, 4, 1, 0, 1, 256]),
    Case("tree-ragged-group", 2, 16, 16, 136, 136, 1, 1, 1, (0, 0), (1, 1),
         [64, 64, 4, 1, 0, 18, 2112, 3], dy_nnz=1),
    Case("two-tree-stages", 1, 16, 128, 520, 512, 1, 1, 1, (0, 0), (1, 1),
         [64, 128, 4, 1, 0, 130, 2048, 17, 3], dy_nnz=1),
    Case("wide-clean-cout136", 1, 64, 136, 257, 256, 1, 1, 1, (0, 0), (1, 1),
         [64, 128, 4, 0, 0, 32, 2112, 4], dy_nnz=2),
    Case("wide-elem-cin50-cout130", 1, 50, 130, 256, 256, 1, 1, 1, (0, 0),
         (1, 1), [64, 128, 4, 1, 0, 32, 2048, 4], dy_nnz=2),
    Case("mid-clean-reorder", 1, 256, 128, 256, 256, 3, 3, 1, (1, 1), (1, 1),
         [128, 128, 8, 0, 2, 32, 2048, 4], dy_nnz=2),
    Case("mid-elem-cin120-cout136", 1, 120, 136, 256, 257, 3, 3, 1, (1, 1),
         (1, 1), [128, 128, 8, 1, 0, 32, 2112, 4], dy_nnz=2),
    Case("mid-elem-last-kd-tile", 1, 144, 128, 256, 256, 3, 3, 1, (2, 2),
         (2, 2), [128, 128, 8, 1, 0, 32, 2048, 4], dy_nnz=2),
    # the tap-crossing walk with KH != KW: wrapping kw at KH goes wrong here
    # (Cin = 5: every 16-row piece runs through three or four taps and so
    # through the kw = KW - 1 -> next kh wrap)
    Case("kh3-kw2-cin5-tap-walk", 2, 5, 24, 11, 13, 3, 2, 1, (1, 0), (1, 1),
         [64, 64, 4, 1, 0, 1, 320]),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]

# the space-to-depth stem (even H and W): runs through conv_kernels.conv_wgrad
STEM = Case("stem-s2d", 2, 3, 64, 40, 56, 7, 7, 2, (3, 3), (1, 1), None)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_plan_of_the_cases(case):
    """The cases are chosen for the plan they hit; a planner change must show
    up here rather than silently move them elsewhere."""
    got = list(_ext().conv_wgrad_plan(case.M, case.Cin, case.Cout, case.KH,
                                      case.KW))
    assert got == case.plan, f"M={case.M} KD={case.KD}"
    tkd, tco, waves, elem, kd_cb, chunks, chunk_len = got[:7]
    assert chunk_len % 64 == 0
    assert (chunks - 1) * chunk_len < case.M <= chunks * chunk_len
    assert elem == int(case.Cin % 16 != 0 or case.KD % tkd != 0)
    tree, left = [], chunks
    while left > 16:
        left = -(-left // 8)
        tree.append(left)
    assert got[7:] == tree


def _exact_inputs(case, seed):
    """x in {-1, 0, 1} [N, Cin, H, W]; dy in {-1, 0, 1} [N, Cout, Ho, Wo] with
    a non-zero in every row m. Both bf16, channels_last, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (case.N, case.H, case.W, case.Cin), generator=g,
                      dtype=torch.int8)
    M, Cout = case.M, case.Cout
    if case.dy_nnz == 0:
        dy = torch.randint(-1, 2, (M, Cout), generator=g, dtype=torch.int8)
        # rows that came out all zero get one entry
        empty = (dy != 0).sum(dim=1) == 0
        dy[empty, torch.randint(0, Cout, (int(empty.sum()),), generator=g)] = 1
    else:
        dy = torch.zeros(M, Cout, dtype=torch.int8)
        rows = torch.arange(M)
        c1 = torch.randint(0, Cout, (M,), generator=g)
        dy[rows, c1] = (torch.randint(0, 2, (M,), generator=g) * 2 - 1).to(
            torch.int8)
        if case.dy_nnz == 2:
            # a second, different channel in about half of the rows
            c2 = (c1 + 1 + torch.randint(0, Cout - 1, (M,), generator=g)) % Cout
            s2 = (torch.randint(0, 2, (M,), generator=g) * 2 - 1).to(torch.int8)
            on = torch.rand(M, generator=g) < 0.5
            dy[rows[on], c2[on]] = s2[on]
    x = x.to(BF16).permute(0, 3, 1, 2)
    dy = dy.view(case.N, case.Ho, case.Wo, Cout).to(BF16).permute(0, 3, 1, 2)
    return x, dy


def _check_exact_design(case, dy, ref):
    """The conditions of the design, on the reference alone."""
    rows = dy.permute(0, 2, 3, 1).reshape(case.M, case.Cout)
    assert bool((rows != 0).any(dim=1).all()), "a dy row m is all zero"
    peak = float(ref.abs().max())
    assert peak <= 256, f"max|dW_ref| = {peak} is not exact in bf16"
    assert peak >= 4, "degenerate data"


def _launch(case, x, dy):
    """The raw binding on NHWC buffers (what ops/conv_kernels.py passes)."""
    xn = x.cuda().contiguous(memory_format=torch.channels_last)
    dyn = dy.cuda().contiguous(memory_format=torch.channels_last)
    _dirty()
    dw = _ext().conv_mfma_wgrad(xn, dyn, case.N, case.H, case.W, case.Cin,
                                case.Cout, case.KH, case.KW, case.s,
                                case.pad[0], case.pad[1], case.dil[0],
                                case.dil[1], case.Ho, case.Wo)
    torch.cuda.synchronize()
    assert dw.dtype == BF16 and tuple(dw.shape) == case.w_shape
    return dw


def _oracle(case, x, dy, fn=O.wgrad):
    # the large cases evaluate the fp64 oracle on the GPU (exact on integers)
    big = case.M * case.KD * case.Cout > 2e9
    dev = "cuda" if big else "cpu"
    return fn(x.to(dev), dy.to(dev), case.w_shape, case.s, case.pad,
              case.dil).cpu()


def _assert_equal(case, got, ref, plan=None):
    g = got.detach().cpu().to(F64)
    bad = g != ref
    if bad.any():
        idx = bad.nonzero()
        co, ci, kh, kw = idx[0].tolist()
        kd = (kh * case.KW + kw) * case.Cin + ci
        raise AssertionError(
            f"{case.name}: {int(bad.sum())} of {bad.numel()} elements differ; "
            f"first dW[co={co}][ci={ci}][kh={kh}][kw={kw}] (row kd={kd}) got "
            f"{g[bad][0].item()} want {ref[bad][0].item()}; kd rows affected "
            f"{sorted(set(((i[2] * case.KW + i[3]) * case.Cin + i[1]).item() for i in idx[:4096]))[:24]}"
            f"; plan {plan or case.plan}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_vs_fp64_oracle(case):
    x, dy = _exact_inputs(case, seed=1000 + CASES.index(case))
    ref = _oracle(case, x, dy)
    _check_exact_design(case, dy, ref)
    got = _launch(case, x, dy)
    _assert_equal(case, got, ref)


def test_stem_space_to_depth_vs_direct_7x7_oracle():
    """Even H and W: ``conv_kernels.conv_wgrad`` takes the space-to-depth
    route (4x4 conv over 16 channels, asymmetric effective pad, weight LUT);
    the oracle is the direct 7x7 stride-2 sum."""
    case = STEM
    x, dy = _exact_inputs(case, seed=77)
    ref = _oracle(case, x, dy)
    _check_exact_design(case, dy, ref)
    _dirty()
    got = conv_kernels.conv_wgrad(
        x.cuda().contiguous(memory_format=torch.channels_last),
        dy.cuda().contiguous(memory_format=torch.channels_last),
        case.w_shape, (2, 2), (3, 3), (1, 1))
    assert got is not None and tuple(got.shape) == case.w_shape
    _assert_equal(case, got, ref, plan="space-to-depth stem")


def test_exact_result_does_not_depend_on_workspace_contents():
    """Two launches of a multi-chunk, tree-reduced case around different
    allocator junk give the same bits (plain stores into an ``empty()``
    workspace; fixed reduction order)."""
    case = BY_NAME["tree-ragged-group"]
    x, dy = _exact_inputs(case, seed=5)
    a = _launch(case, x, dy)
    junk = torch.full((8 << 20,), -7.7e8, device="cuda")
    del junk
    b = _launch(case, x, dy)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# precision: real mantissas
# ---------------------------------------------------------------------------

PRECISION = ["67x63-odd-stages-ragged", "cin50-3x3-tap-walk",
             "cin3-7x7-s2-odd-h"]


@pytest.mark.parametrize("name", PRECISION)
def test_precision_vs_fp64_oracle(name):
    """randn bf16 x, 0.1*randn bf16 dy. fp32 accumulation over at most
    chunk_len rows per chunk, ``chunks`` slices and the 8-wide MFMA inner sum,
    then ONE bf16 rounding: each element within
        1/2 ulp_bf16(ref) (1 + 2**-7) + (chunk_len + chunks + 8) u sum|addends|
    of the fp64 value, and the relative L2 error of dW at most twice that of
    the reference's own bf16 rounding."""
    case = BY_NAME[name]
    g = torch.Generator().manual_seed(4321 + PRECISION.index(name))
    x = torch.randn(case.N, case.H, case.W, case.Cin, generator=g).to(BF16) \
        .permute(0, 3, 1, 2)
    dy = (0.1 * torch.randn(case.N, case.Ho, case.Wo, case.Cout, generator=g)) \
        .to(BF16).permute(0, 3, 1, 2)
    ref = _oracle(case, x, dy)
    mag = _oracle(case, x, dy, O.wgrad_abs)
    got = _launch(case, x, dy).cpu().to(F64)
    chunks, chunk_len = case.plan[5], case.plan[6]
    bound = 0.5 * O.bf16_ulp(ref) * (1 + 2.0 ** -7) \
        + (chunk_len + chunks + 8) * U * mag
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    rel = float((got - ref).norm() / ref.norm())
    floor = float((O.rne_bf16(ref).to(F64) - ref).norm() / ref.norm())
    print(f"\n[wgrad precision] {name}: max err/bound {ratio:.3f}, "
          f"rel L2 {rel:.3e}, bf16 rounding of the reference {floor:.3e}")
    assert ratio <= 1.0, f"{name}: element error {ratio:.3f} x bound"
    assert rel <= 2.0 * floor, f"{name}: rel L2 {rel:.3e} > 2 x {floor:.3e}"
