"""Direct tests of the ``bn_act.hip`` and ``spatial.hip`` extension ops against
the fp64 oracle in ``bn_spatial_oracle.py`` (validated on the CPU by
``test_bn_spatial_oracle.py``).

Two kinds of input:

* coverage tests draw small integers, so every fp32 partial sum is exact in
  any summation order and the kernels must EQUAL the oracle — a skipped or
  doubled row / channel cannot hide behind a tolerance;
* precision tests draw randn-based bf16 data and bound the error from the
  fp32 formula of the kernel (u = 2**-24 is the fp32 unit roundoff).
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

import bn_spatial_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd import ops
    from improved_body_parts_amd.ops import _backend

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CL = torch.channels_last
U = 2.0 ** -24                                    # fp32 unit roundoff
SLOPE32 = float(torch.tensor(0.01, dtype=F32))    # the model's slope, as the
#                                                   kernels see it: (float)0.01
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"


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


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _eq(got, want64, what):
    """``got`` (device, any float dtype) equals the fp64 oracle value exactly."""
    g = got.detach().cpu().to(F64).reshape(want64.shape)
    bad = g != want64
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.numel()} differ, first at "
        f"{bad.nonzero()[0].tolist()}: got {g[bad][0].item()} "
        f"want {want64[bad][0].item()}")


# ---------------------------------------------------------------------------
# coverage: exact integer data, equality
# ---------------------------------------------------------------------------

# (M, C) -> [cpb, rpb, rows, grid_y] of the bf16 v8 launch
V8_CASES = {
    (512, 32): [4, 64, 1, 1],       # one row-block, M a multiple of the step
    (37, 8): [1, 256, 1, 1],        # most threads own no row
    (2, 8): [1, 256, 1, 1],         # smallest legal training batch
    (1000, 48): [6, 42, 3, 1],      # 252 of 256 threads work; ragged M
    (4099, 768): [96, 2, 257, 1],   # 192 threads; colsum takes 3 trips; prime M
    (8209, 768): [96, 2, 512, 1],   # ceil(M/16) = 514 > 512: the row cap binds
    (64, 2056): [256, 1, 8, 2],     # C8 = 257: one live lane in grid.y = 1
}
SCALAR_CASES = [(BF16, 1000, 50),   # the head width, C % 8 != 0
                (F32, 1000, 32),    # fp32 scalar path
                (F32, 100, 300)]    # grid.y = 2
ALL_CASES = [pytest.param(BF16, m, c, id=f"bf16v8-{m}x{c}")
             for (m, c) in V8_CASES] + \
            [pytest.param(dt, m, c, id=f"{'bf16' if dt == BF16 else 'fp32'}"
                                       f"-scalar-{m}x{c}")
             for dt, m, c in SCALAR_CASES]


def _v8_formula(M, C):
    C8 = C // 8
    cpb = min(C8, 256)
    rpb = 256 // cpb
    rows = max(min(-(-M // (rpb * 8)), 512), 1)
    return [cpb, rpb, rows, -(-C8 // cpb)]


@pytest.mark.parametrize("M,C", list(V8_CASES))
def test_v8_geometry_of_the_cases(M, C):
    """The cases below are chosen for the launch geometry they hit; a planner
    change must show up here rather than silently move them elsewhere."""
    assert _v8_formula(M, C) == V8_CASES[(M, C)]
    assert list(_ext().bn_v8_geometry(M, C)) == V8_CASES[(M, C)]
    cpb, rpb, rows, _ = V8_CASES[(M, C)]
    assert cpb * rpb <= 256 and rows <= 512


@functools.lru_cache(maxsize=None)
def _int_case(dtype, M, C):
    """Exactly representable inputs: x in [-8, 8], dy even in [-8, 8], y in
    [-8, 8] (zeros included: act'(0) is the slope), integer mean in [-4, 4],
    invstd in {1/4, 1/2}. With slope 1/2 every addend of every sum is a
    multiple of 1/8 below 2**7 and every sum is far below 2**24 * 1/8, so
    fp32 accumulation is exact in any order."""
    g = _gen(1000 * C + M)
    c = types.SimpleNamespace(M=M, C=C, dtype=dtype)
    c.x = _ints(g, (M, C), -8, 8)
    c.dy = _ints(g, (M, C), -4, 4) * 2
    c.y = _ints(g, (M, C), -8, 8)
    c.mean = _ints(g, (C,), -4, 4)
    c.invstd = 0.25 * (1 + _ints(g, (C,), 0, 1))
    c.gamma = _ints(g, (C,), -3, 3)
    c.beta = _ints(g, (C,), -3, 3)
    for k in ("x", "dy", "y"):
        setattr(c, k + "g", getattr(c, k).to(dtype).cuda())
    for k in ("mean", "invstd", "gamma", "beta"):
        setattr(c, k + "g", getattr(c, k).to(F32).cuda())
    c.sums, c.sumsq = O.bn_stats(c.x, C)
    assert float(c.sumsq.max()) < 2 ** 24
    return c


@pytest.mark.parametrize("dtype,M,C", ALL_CASES)
def test_bn_stats_exact(dtype, M, C):
    c = _int_case(dtype, M, C)
    for _ in range(2):                      # second call: recycled workspace
        _dirty()
        s, q = _ext().bn_stats(c.xg, C)
        _eq(s, c.sums, "sums")
        _eq(q, c.sumsq, "sumsq")


@pytest.mark.parametrize("dtype,M,C", ALL_CASES)
def test_bn_stats_finalize_exact_mean_and_split_path(dtype, M, C):
    """Fused stats+finalize: the mean is exact up to the one ``* (1/M)``
    (replayed here in IEEE fp32). The split SyncBN path bn_stats ->
    bn_finalize must reproduce the fused op on all four outputs and on the
    running statistics: same exact sums, same fp32 epilogue."""
    c = _int_case(dtype, M, C)
    ext = _ext()
    rm0 = torch.linspace(-1, 1, C)
    rv0 = torch.linspace(0.5, 2, C)

    def state():
        return rm0.clone().cuda(), rv0.clone().cuda(), \
            torch.tensor(7, dtype=torch.int64, device="cuda")

    rm, rv, nb = state()
    ptrs = (rm.data_ptr(), rv.data_ptr(), nb.data_ptr())
    _dirty()
    fused = ext.bn_stats_finalize(c.xg, C, c.gammag, c.betag, rm, rv, nb,
                                  MOM, EPS)
    inv_m = torch.tensor(1.0, dtype=F32) / torch.tensor(float(M), dtype=F32)
    _eq(fused[0], (c.sums.to(F32) * inv_m).to(F64), "mean = sum * (1/M)")
    assert (rm.data_ptr(), rv.data_ptr(), nb.data_ptr()) == ptrs
    assert int(nb) == 8
    assert not torch.equal(rm.cpu(), rm0) and not torch.equal(rv.cpu(), rv0)

    rm2, rv2, nb2 = state()
    _dirty()
    s, q = ext.bn_stats(c.xg, C)
    split = ext.bn_finalize(s, q, M, c.gammag, c.betag, rm2, rv2, nb2, MOM, EPS)
    for a, b, name in zip(split, fused, ("mean", "invstd", "scale", "shift")):
        assert torch.equal(a, b), f"split vs fused {name}"
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv) and int(nb2) == 8
    for t in fused:
        assert torch.isfinite(t).all()
    # against the oracle: sums are exact, the epilogue is a handful of fp32 ops
    want = O.bn_stats_finalize(c.x, C, c.gamma, c.beta, None, None, None, MOM, EPS)
    for a, w, name in zip(fused, want, ("mean", "invstd", "scale", "shift")):
        err = (a.cpu().to(F64) - w).abs()
        # ~6 fp32 roundings of 2**-24 around E[x^2] - mean^2, where E[x^2]
        # <= 64 + 16 and var of the 17 uniform integers is ~24 (M = 2: exact):
        # <= 6 u * 80 / 24 ~ 1.2e-6 relative in var, half of it in invstd
        assert (err <= 1e-5 * w.abs() + 1e-5).all(), f"{name}: {err.max():.3e}"


@pytest.mark.parametrize("act", [True, False], ids=["act", "noact"])
@pytest.mark.parametrize("need_xhat", [True, False], ids=["xhat", "noxhat"])
@pytest.mark.parametrize("dtype,M,C", ALL_CASES)
def test_bn_act_bwd_exact(dtype, M, C, need_xhat, act):
    c = _int_case(dtype, M, C)
    want = O.bn_act_bwd(c.dy, c.y, c.x, c.mean, c.invstd, 0.5, act, need_xhat, C)
    assert float(want[2].abs().max()) < 2 ** 21       # exact in fp32 (1/8 grid)
    _dirty()
    got = _ext().bn_act_bwd(c.dyg, c.yg, c.xg,
                            c.meang if need_xhat else None,
                            c.invstdg if need_xhat else None,
                            0.5, act, need_xhat, C)
    assert got[0].dtype == dtype and got[0].shape == c.dyg.shape
    _eq(got[0], want[0], "dpre")
    _eq(got[1], want[1], "sum dpre")
    _eq(got[2], want[2], "sum dpre*xhat" if need_xhat else "zero xhat plane")


# ---------------------------------------------------------------------------
# precision: randn-based bf16 data, bounds from the fp32 formula
# ---------------------------------------------------------------------------

def _report(what, text):
    print(f"[bn_spatial] {what}: {text}")


def _assert_elementwise(got, ref64, terms64, what):
    """Elementwise bf16 output of an fp32 formula.

    The kernel evaluates the formula in fp32 (each of its <= 4 roundings is
    at most u times the running magnitude, which the sum of the |addends|
    dominates) and rounds once more to bf16, so

        |got - RNE_bf16(ref64)| <= 1 bf16 ulp(ref64) + 4 u sum|addends|.

    On top of it, at most 1e-3 of the elements may differ from the correctly
    rounded reference at all (an fp32 evaluation lands on the other side of
    a bf16 rounding boundary for ~4e-5 of realistic elements).
    fp32 outputs: |got - ref64| <= 2 u |ref64| + 4 u sum|addends|."""
    g = got.detach().cpu()
    ref64 = ref64.reshape(g.shape)
    terms64 = terms64.reshape(g.shape).abs()
    assert torch.isfinite(g.float()).all(), f"{what}: non-finite output"
    if g.dtype == BF16:
        diff = (g.to(F64) - O.rne_bf16(ref64).to(F64)).abs()
        bound = O.bf16_ulp(ref64) + 4 * U * terms64
    else:
        diff = (g.to(F64) - ref64).abs()
        bound = 2 * U * ref64.abs() + 4 * U * terms64
    worst = float((diff / bound).max())
    frac = float((diff != 0).to(F64).mean()) if g.dtype == BF16 else 0.0
    _report(what, f"max err/bound {worst:.3f}, fraction != RNE(ref) {frac:.2e}")
    assert worst <= 1.0, f"{what}: error {worst:.3f}x the bound"
    assert frac <= 1e-3, f"{what}: {frac:.2e} of the elements differ from RNE"


def _assert_reduction(got, ref64, abs_sum64, n, what):
    """fp32 sum of n addends in ANY order: |got - ref| <= n u sum|addends|
    (worst case, loose on purpose: the exact-integer tests carry the
    sharpness)."""
    g = got.detach().cpu().to(F64).reshape(ref64.shape)
    assert torch.isfinite(g).all(), f"{what}: non-finite"
    bound = n * U * abs_sum64 + 1e-30
    worst = float(((g - ref64).abs() / bound).max())
    _report(what, f"max err/bound {worst:.4f}")
    assert worst <= 1.0, f"{what}: error {worst:.3f}x the bound"


RATIOS = (0.0, 4.0, 32.0)
PRECISION_CASES = [(1000, 48), (4099, 768), (1000, 50)]


@functools.lru_cache(maxsize=None)
def _real_case(M, C):
    """randn-based bf16 activations: channel c has std sigma_c in {1/2, 1, 2}
    and mean RATIOS[c % 3] * sigma_c; channel 0 is constant. gamma has a zero
    and negative entries. The GPU statistics are computed once and shared."""
    g = _gen(77 * C + M)
    c = types.SimpleNamespace(M=M, C=C)
    sigma = 2.0 ** torch.randint(-1, 2, (C,), generator=g).to(F64)
    c.ratio = torch.tensor([RATIOS[i % 3] for i in range(C)], dtype=F64)
    x = torch.randn(M, C, generator=g, dtype=F64) * sigma + c.ratio * sigma
    x[:, 0] = 1.5                                  # constant: var clamps at 0
    c.xg = x.to(BF16).cuda()
    c.x = c.xg.cpu().to(F64)                       # the values the kernel sees
    c.gamma = torch.randn(C, generator=g).to(F32)
    c.gamma[1] = 0.0
    c.gamma[2] = -c.gamma[2].abs() - 0.5
    c.gamma[0] = 1.25
    c.beta = torch.randn(C, generator=g).to(F32)
    c.res = torch.randn(M, C, generator=g).to(BF16)
    c.dy = torch.randn(M, C, generator=g).to(BF16)
    c.rm0 = torch.randn(C, generator=g).to(F32)
    c.rv0 = (torch.rand(C, generator=g) + 0.5).to(F32)
    c.rm, c.rv = c.rm0.clone().cuda(), c.rv0.clone().cuda()
    c.nb = torch.tensor(3, dtype=torch.int64, device="cuda")
    c.ptrs = (c.rm.data_ptr(), c.rv.data_ptr(), c.nb.data_ptr())
    _dirty()
    c.stats = _ext().bn_stats_finalize(c.xg, C, c.gamma.cuda(), c.beta.cuda(),
                                       c.rm, c.rv, c.nb, MOM, EPS)
    torch.cuda.synchronize()
    return c


@pytest.mark.parametrize("M,C", PRECISION_CASES)
def test_bn_stats_precision(M, C):
    c = _real_case(M, C)
    _dirty()
    s, q = _ext().bn_stats(c.xg, C)
    rs, rq = O.bn_stats(c.x, C)
    _assert_reduction(s, rs, c.x.abs().sum(0), M, "sums")
    _assert_reduction(q, rq, rq, M, "sumsq")


@pytest.mark.parametrize("M,C", PRECISION_CASES)
def test_bn_finalize_precision(M, C):
    """One-pass variance E[x^2] - mean^2 in fp32. With e_S = n u sum|x| and
    e_Q = n u sum x^2 the reduction bounds (n = M rows):

      e_mean = e_S / M + 2 u |mu|                     (1/M rounding, product)
      e_var  = e_Q / M + 2 |mu| e_mean + 4 u (E[x^2] + mu^2)
            <= (3 n + 12) u (sigma^2 + mu^2)          (|mu| E|x| <= E[x^2])
             = (3 n + 12) u sigma^2 (1 + mu^2 / sigma^2)

    i.e. the relative error of var grows like 1 + (mean/std)^2. invstd is
    monotone in var, so it lies between rsqrt(var + e_var + eps) and
    rsqrt(max(var - e_var, 0) + eps), widened by 4 u for the add and the
    hardware rsqrt. scale, shift and the running statistics follow by the
    product rule (e_scale, e_shift, e_rm, e_rv below)."""
    c = _real_case(M, C)
    mean, invstd, scale, shift = [t.cpu().to(F64) for t in c.stats]
    for t in (mean, invstd, scale, shift):
        assert torch.isfinite(t).all()
    rm_ref, rv_ref = c.rm0.to(F64), c.rv0.to(F64)
    nb_ref = torch.tensor(3)
    gam, bet = c.gamma.to(F64), c.beta.to(F64)
    rmean, rinv, rscale, rshift = O.bn_stats_finalize(
        c.x, C, gam, bet, rm_ref, rv_ref, nb_ref, MOM, EPS)
    ex2 = (c.x * c.x).mean(0)
    var = torch.clamp(ex2 - rmean * rmean, min=0.0)

    e_mean = U * c.x.abs().sum(0) + 2 * U * rmean.abs()   # (n u sum|x|) / n
    e_var = (3 * M + 12) * U * (var + rmean * rmean)
    lo = (1 - 4 * U) / torch.sqrt(var + e_var + EPS)
    hi = (1 + 4 * U) / torch.sqrt(torch.clamp(var - e_var, min=0.0) + EPS)
    e_inv = torch.maximum(hi - rinv, rinv - lo)
    e_scale = gam.abs() * e_inv + U * gam.abs() * hi
    e_shift = rmean.abs() * e_scale + e_mean * (rscale.abs() + e_scale) \
        + 2 * U * (bet.abs() + (rmean.abs() + e_mean) * (rscale.abs() + e_scale))
    unb = M / (M - 1)
    e_rm = MOM * e_mean + 4 * U * ((1 - MOM) * c.rm0.to(F64).abs()
                                   + MOM * rmean.abs())
    e_rv = MOM * unb * e_var + 6 * U * ((1 - MOM) * c.rv0.to(F64).abs()
                                        + MOM * unb * var)

    def check(got, ref, err, name):
        worst = float(((got - ref).abs() / (err + 1e-30)).max())
        _report(f"finalize {M}x{C} {name}", f"max err/bound {worst:.4f}")
        assert worst <= 1.0, f"{name}: error {worst:.3f}x the bound"

    check(mean, rmean, e_mean, "mean")
    assert (invstd >= lo).all() and (invstd <= hi).all(), "invstd interval"
    check(invstd, rinv, e_inv, "invstd")
    check(scale, rscale, e_scale, "scale")
    check(shift, rshift, e_shift, "shift")
    # running statistics: updated IN PLACE, num_batches_tracked + 1 per call
    assert (c.rm.data_ptr(), c.rv.data_ptr(), c.nb.data_ptr()) == c.ptrs
    assert int(c.nb) == 4 == int(nb_ref)
    check(c.rm.cpu().to(F64), rm_ref, e_rm, "running_mean")
    check(c.rv.cpu().to(F64), rv_ref, e_rv, "running_var")
    assert float(invstd[0]) <= EPS ** -0.5 * (1 + 4 * U)   # constant channel

    # how far the one-pass variance can be trusted (docs/KERNELS.md): the
    # kernel's var, recovered from invstd, against the bound per mean/std ratio
    var_got = 1.0 / (invstd * invstd) - EPS
    for r in RATIOS:
        sel = (c.ratio == r)
        sel[0] = False
        ratio = ((var_got - var).abs() / e_var)[sel].max()
        rel = ((var_got - var).abs() / var)[sel].max()
        _report(f"finalize {M}x{C} mean/std={r:g}",
                f"var err/bound {float(ratio):.2e}, relative {float(rel):.2e}")


@pytest.mark.parametrize("M,C", PRECISION_CASES)
def test_bn_act_fwd_precision(M, C):
    c = _real_case(M, C)
    ext = _ext()
    _, _, scale, shift = c.stats
    resg = c.res.cuda()
    for res, act in ((None, False), (None, True), (resg, True), (resg, False)):
        y = ext.bn_act_fwd(c.xg, scale, shift, res, SLOPE32, act)
        assert y.dtype == BF16 and y.shape == c.xg.shape
        ref = O.bn_act_fwd(c.x, scale, shift, res, SLOPE32, act)
        terms = O.bn_act_fwd_terms(c.x, scale, shift, res)
        _assert_elementwise(y, ref, terms,
                            f"bn_act_fwd {M}x{C} res={res is not None} act={act}")
        if res is None and not act:
            # the constant channel sits at beta (same elementwise bound)
            beta0 = c.beta[:1].to(F64)
            t0 = abs(1.5 * float(scale[0])) + abs(float(shift[0]))
            d0 = (y[:, 0].cpu().to(F64) - O.rne_bf16(beta0).to(F64)).abs().max()
            b0 = float(O.bf16_ulp(beta0)) + 4 * U * t0
            _report(f"bn_act_fwd {M}x{C} constant channel at beta",
                    f"err/bound {float(d0) / b0:.3f}")
            assert float(d0) <= b0


@pytest.mark.parametrize("M,C", PRECISION_CASES)
def test_bn_act_bwd_precision(M, C):
    c = _real_case(M, C)
    ext = _ext()
    mean, invstd, scale, shift = c.stats
    gam = c.gamma.cuda()
    y = ext.bn_act_fwd(c.xg, scale, shift, None, SLOPE32, True)
    dyg = c.dy.cuda()
    _dirty()
    dpre, sd, sx = ext.bn_act_bwd(dyg, y, c.xg, mean, invstd, SLOPE32, True,
                                  True, C)
    rdpre, rsd, rsx = O.bn_act_bwd(c.dy, y, c.x, mean, invstd, SLOPE32, True,
                                   True, C)
    _assert_elementwise(dpre, rdpre, rdpre, f"dpre {M}x{C}")
    xhat = (c.x - mean.cpu().to(F64)) * invstd.cpu().to(F64)
    _assert_reduction(sd, rsd, rdpre.abs().sum(0), M, f"sum dpre {M}x{C}")
    _assert_reduction(sx, rsx, (rdpre * xhat).abs().sum(0), M,
                      f"sum dpre*xhat {M}x{C}")
    # apply: the oracle takes the SAME dpre / sums the kernel is given
    for training in (True, False):
        sums = (sd, sx) if training else (None, None)
        dx = ext.bn_act_bwd_apply(dpre, c.xg, mean, invstd, gam, *sums, C)
        assert dx.dtype == BF16 and dx.shape == dpre.shape
        ref = O.bn_act_bwd_apply(dpre, c.x, mean, invstd, gam, *sums, C)
        p, qx, r = O.bn_act_bwd_apply_terms(dpre, c.x, mean, invstd, gam,
                                            *sums, C)
        _assert_elementwise(dx, ref, p.abs() + qx.abs() + r.abs(),
                            f"bn_act_bwd_apply {M}x{C} training={training}")


# ---------------------------------------------------------------------------
# se_gate
# ---------------------------------------------------------------------------

# Maximum |gate - fp64 gate| measured on an MI355X over the six cases below
# (fast exponential + fp32 dot products; not derivable from the source):
#   C=8   CH=1 : 5.1e-8 (fp32 params), 5.9e-8 (bf16 params)
#   C=256 CH=16: 5.7e-7, 9.4e-7
#   C=768 CH=64: 1.40e-6, 1.91e-6
# The assertion allows 4x the largest of them for other seeds.
SE_GATE_MEASURED = 1.91e-6


@pytest.mark.parametrize("pdtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C,CH", [(8, 1), (256, 16), (768, 64)])
def test_se_gate_direct(C, CH, pdtype):
    g = _gen(C + CH)
    N, pool_scale = 3, 1.0 / 37.0
    pooled = (torch.randn(N, C, generator=g) * 37.0).to(F32)
    w1 = (torch.randn(CH, C, generator=g) * (2.0 / C ** 0.5)).to(pdtype)
    b1 = torch.randn(CH, generator=g).to(pdtype)
    w2 = (torch.randn(C, CH, generator=g) * (2.0 / CH ** 0.5)).to(pdtype)
    b2 = torch.randn(C, generator=g).to(pdtype)
    s = _ext().se_gate(pooled.cuda(), w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda(),
                       SLOPE32, pool_scale)
    assert s.dtype == F32 and tuple(s.shape) == (N, C)
    ref = O.se_gate(pooled, w1, b1, w2, b2, SLOPE32, pool_scale)
    err = float((s.cpu().to(F64) - ref).abs().max())
    _report(f"se_gate C={C} CH={CH} {pdtype}", f"max abs err {err:.3e}")
    assert err <= 4 * SE_GATE_MEASURED


# ---------------------------------------------------------------------------
# spatial ops
# ---------------------------------------------------------------------------

SPATIAL = [pytest.param(BF16, 2, 8, 2, 2, id="bf16-2x8x2x2"),
           pytest.param(BF16, 1, 24, 6, 10, id="bf16-1x24x6x10"),
           pytest.param(BF16, 3, 40, 16, 4, id="bf16-3x40x16x4"),
           pytest.param(BF16, 1, 50, 6, 6, id="bf16-scalar-1x50x6x6"),
           pytest.param(F32, 2, 12, 6, 4, id="fp32-2x12x6x4")]
ODD = [pytest.param(BF16, 2, 64, 7, 9, id="bf16-odd-2x64x7x9"),
       pytest.param(F32, 1, 12, 5, 7, id="fp32-odd-1x12x5x7")]


def _spatial_input(kind, dtype, shape, seed):
    g = _gen(seed)
    if kind == "ties4":      # four distinct values: every window holds ties
        x = torch.randint(0, 4, shape, generator=g).to(F64) - 1.5
    elif kind == "eighths":  # multiples of 1/8 in [-4, 4]
        x = torch.randint(-32, 33, shape, generator=g).to(F64) / 8
    else:
        x = torch.randn(shape, generator=g, dtype=F64)
    x = x.to(dtype)
    return x, x.to(F64)


def _first_max_position(x64, N, H, W, C):
    """Window position (0..3, row-major) of the first maximum, from x alone."""
    Ho, Wo = H // 2, W // 2
    v = x64.reshape(N, H, W, C)[:, :2 * Ho, :2 * Wo]
    win = torch.stack([v[:, 0::2, 0::2], v[:, 0::2, 1::2],
                       v[:, 1::2, 0::2], v[:, 1::2, 1::2]])
    is_max = win == win.max(0).values
    first = is_max & (is_max.cumsum(0) == 1)
    return (first * torch.arange(4).view(4, 1, 1, 1, 1)).sum(0), \
        is_max.sum(0) > 1


@pytest.mark.parametrize("kind", ["randn", "ties4"])
@pytest.mark.parametrize("dtype,N,C,H,W", SPATIAL + ODD)
def test_maxpool_direct(dtype, N, C, H, W, kind):
    ext = _ext()
    x, x64 = _spatial_input(kind, dtype, (N, H, W, C), N + C + H + W)
    Ho, Wo = H // 2, W // 2
    y, arg = ext.maxpool2x2_fwd(x.cuda(), N, H, W, C)
    ry, rarg = O.maxpool2x2_fwd(x64, N, H, W, C)
    assert y.dtype == dtype and arg.dtype == torch.uint8
    assert tuple(y.shape) == (N, Ho, Wo, C) == tuple(arg.shape)
    _eq(y, ry, "maxpool y")
    assert torch.equal(arg.cpu(), rarg), "argmax byte"
    first, tied = _first_max_position(x64, N, H, W, C)
    assert torch.equal(arg.cpu().long(), first), "argmax is not the first maximum"
    if kind == "ties4":
        assert float(tied.double().mean()) > 0.25          # ties do happen

    g = _gen(5)
    dy = torch.randn(N, Ho, Wo, C, generator=g)
    dy = torch.where(dy == 0, torch.ones_like(dy), dy).to(dtype)
    dy = torch.where(dy == 0, torch.ones_like(dy), dy)
    _dirty()
    dx = ext.maxpool2x2_bwd(dy.cuda(), arg, N, H, W, C)
    assert dx.dtype == dtype and tuple(dx.shape) == (N, H, W, C)
    _eq(dx, O.maxpool2x2_bwd(dy, rarg, N, H, W, C), "maxpool dx")
    d = dx.cpu().to(F64)
    assert not d[:, 2 * Ho:].any() and not d[:, :, 2 * Wo:].any()
    d = d[:, :2 * Ho, :2 * Wo]
    hit = torch.stack([d[:, 0::2, 0::2], d[:, 0::2, 1::2],
                       d[:, 1::2, 0::2], d[:, 1::2, 1::2]]) != 0
    assert (hit.sum(0) == 1).all(), "one position per window gets the gradient"
    assert torch.equal((hit * torch.arange(4).view(4, 1, 1, 1, 1)).sum(0), first)


@pytest.mark.parametrize("N,C,H,W", [(2, 64, 7, 9), (1, 24, 6, 10)])
def test_maxpool_autograd_ties_match_cpu_max_pool2d(N, C, H, W):
    """Through ops.maxpool2x2(...).backward in bf16, on tied inputs, against
    F.max_pool2d on the CPU (which also keeps the first maximum)."""
    x, x64 = _spatial_input("ties4", BF16, (N, C, H, W), 11)
    xg = x.cuda().contiguous(memory_format=CL).requires_grad_(True)
    y = ops.maxpool2x2(xg)
    dy = torch.randn(y.shape, generator=_gen(6)).to(BF16)
    y.backward(dy.cuda())
    xr = x64.clone().requires_grad_(True)
    yr = F.max_pool2d(xr, 2, 2)
    yr.backward(dy.to(F64))
    assert torch.equal(y.detach().cpu().to(F64), yr.detach())
    assert torch.equal(xg.grad.cpu().to(F64), xr.grad)


@pytest.mark.parametrize("dtype,N,C,H,W", SPATIAL)
def test_upsample_direct(dtype, N, C, H, W):
    ext = _ext()
    x, x64 = _spatial_input("randn", dtype, (N, H, W, C), 3 * N + C + H + W)
    y = ext.upsample2x_fwd(x.cuda(), N, H, W, C)
    assert y.dtype == dtype and tuple(y.shape) == (N, 2 * H, 2 * W, C)
    _eq(y, O.upsample2x_fwd(x64, N, H, W, C), "upsample y")

    # 4-to-1 sum of multiples of 1/8 in [-4, 4]: |sum| <= 16 on a 1/8 grid is
    # exact in fp32, so the result is the correctly rounded fp64 sum
    dy, dy64 = _spatial_input("eighths", dtype, (N, 2 * H, 2 * W, C), 9)
    dx = ext.upsample2x_bwd(dy.cuda(), N, H, W, C)
    assert dx.dtype == dtype and tuple(dx.shape) == (N, H, W, C)
    ref = O.upsample2x_bwd(dy64, N, H, W, C)
    _eq(dx, O.rne_bf16(ref).to(F64) if dtype == BF16 else ref, "upsample dx")

    dy, dy64 = _spatial_input("randn", dtype, (N, 2 * H, 2 * W, C), 10)
    dx = ext.upsample2x_bwd(dy.cuda(), N, H, W, C)
    terms = O.upsample2x_bwd(dy64.abs(), N, H, W, C)
    _assert_elementwise(dx, O.upsample2x_bwd(dy64, N, H, W, C), terms,
                        "upsample dx randn")


SE_REDUCE = [pytest.param(BF16, 64, 24, 1, id="bf16-hw64-1row"),
             pytest.param(BF16, 33 * 33, 40, 18, id="bf16-hw1089-18rows"),
             pytest.param(BF16, 33 * 33, 264, 18, id="bf16-hw1089-c264-gridy2"),
             pytest.param(F32, 33 * 33, 12, 18, id="fp32-hw1089-18rows")]


def _se_reduce_check(dtype, N, HW, C, rows):
    assert min(-(-HW // 64), 512) == rows        # workspace rows of the launch
    g = _gen(HW + C + N)
    a = _ints(g, (N, HW, C), -8, 8)
    b = _ints(g, (N, HW, C), -8, 8)
    ag, bg = a.to(dtype).cuda(), b.to(dtype).cuda()
    for prod in (False, True):
        _dirty()
        out = _ext().se_reduce(ag, bg if prod else None, N, HW, C)
        assert out.dtype == F32 and tuple(out.shape) == (N, C)
        _eq(out, O.se_reduce(a, b if prod else None, N, HW, C),
            f"se_reduce prod={prod}")


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("dtype,HW,C,rows", SE_REDUCE)
def test_se_reduce_exact(dtype, HW, C, rows, N):
    _se_reduce_check(dtype, N, HW, C, rows)


def test_se_reduce_exact_row_cap():
    _se_reduce_check(BF16, 1, 182 * 182, 8, 512)   # ceil(HW/64) = 518 > 512


def test_se_reduce_precision():
    N, HW, C = 3, 33 * 33, 40
    g = _gen(21)
    a = torch.randn(N, HW, C, generator=g).to(BF16)
    b = (torch.randn(N, HW, C, generator=g) + 1).to(BF16)
    a64, b64 = a.to(F64), b.to(F64)
    _dirty()
    _assert_reduction(_ext().se_reduce(a.cuda(), None, N, HW, C),
                      O.se_reduce(a64, None, N, HW, C), a64.abs().sum(1), HW,
                      "se_reduce")
    _assert_reduction(_ext().se_reduce(a.cuda(), b.cuda(), N, HW, C),
                      O.se_reduce(a64, b64, N, HW, C), (a64 * b64).abs().sum(1),
                      HW, "se_reduce prod")


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "addc"])
@pytest.mark.parametrize("dtype,C", [(BF16, 24), (BF16, 50), (F32, 12)],
                         ids=["bf16v8-c24", "bf16-scalar-c50", "fp32-c12"])
def test_se_scale_direct(dtype, C, with_add):
    N, HW = 3, 35                      # i / (HW * C8) crosses images
    g = _gen(C)
    x = torch.randn(N, HW, C, generator=g).to(dtype)
    s = torch.rand(N, C, generator=g).to(F32)
    addc = torch.randn(N, C, generator=g).to(F32) if with_add else None
    y = _ext().se_scale(x.cuda(), s.cuda(), addc.cuda() if with_add else None,
                        N, HW, C)
    assert y.dtype == dtype and y.shape == x.shape
    ref = O.se_scale(x, s, addc, N, HW, C)
    terms = O.se_scale(x.abs(), s, addc.abs() if with_add else None, N, HW, C)
    _assert_elementwise(y, ref, terms, f"se_scale C={C} addc={with_add}")


def test_se_layer_bf16_autograd():
    """ops.se_layer in bf16 through autograd against the fp64 layer evaluated
    on the same bf16 parameters. Between the HIP reduce / scale kernels the
    training path rounds to bf16 after the pooled cast, fc1, leaky, fc2 and
    the sigmoid, and once more for y: <= 6 roundings of 2**-9 relative on the
    way to y and to the se_scale part of dx, hence 2**-6 on their relative
    L2 error. The FC gradients pass through about twice as many roundings
    (ds, the sigmoid and leaky backward, the two GEMM outputs on top of the
    forward ones): 2**-5."""
    g = _gen(12)
    N, C, H, W = 2, 32, 12, 12
    fc1 = torch.nn.Linear(C, C // 16)
    fc2 = torch.nn.Linear(C // 16, C)
    with torch.no_grad():
        for p in (fc1.weight, fc1.bias, fc2.weight, fc2.bias):
            p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    fc1, fc2 = fc1.cuda().bfloat16(), fc2.cuda().bfloat16()
    x = torch.randn(N, C, H, W, generator=g).to(BF16)
    dy = torch.randn(N, C, H, W, generator=g).to(BF16)
    xg = x.cuda().contiguous(memory_format=CL).requires_grad_(True)
    y = ops.se_layer(xg, fc1, fc2)
    assert y.dtype == BF16
    y.backward(dy.cuda().contiguous(memory_format=CL))
    want = O.se_layer_fwd_bwd(x.permute(0, 2, 3, 1), fc1.weight, fc1.bias,
                              fc2.weight, fc2.bias, dy.permute(0, 2, 3, 1),
                              0.01)
    got = [y.detach().permute(0, 2, 3, 1), xg.grad.permute(0, 2, 3, 1),
           fc1.weight.grad, fc1.bias.grad, fc2.weight.grad, fc2.bias.grad]
    tols = [2.0 ** -6, 2.0 ** -6] + [2.0 ** -5] * 4
    for a, w, tol, name in zip(got, want, tols,
                               ("y", "dx", "dw1", "db1", "dw2", "db2")):
        a = a.detach().cpu().to(F64)
        assert a.shape == w.shape, name
        rel = float((a - w).norm() / w.norm())
        _report(f"se_layer bf16 {name}", f"relative L2 {rel:.3e}")
        assert rel <= tol, f"{name}: relative L2 {rel:.3e} > {tol:.3e}"
