"""Direct tests of ``loss.hip`` and ``sgd.hip`` against the fp64 oracles in
``train_oracle.py`` (validated on the CPU by ``test_train_oracle.py``).

Focal loss: ``gt`` holds multiples of 1/64 and ``mask`` is binary (one case:
multiples of 1/4), so window means and bilinear samples are exact in fp32 as
in fp64 and no element can sit on the wrong side of the 0.01 / 0.5 switches.
Bounds follow the kernel's fp32 formula, u = 2**-24:

* per-stack sums within ``n u sum|addends|``, n = per-thread trips + 8 +
  number of blocks (serial accumulation, wave + block reduction, one atomic
  per block);
* fp32 ``dpred`` within ``16 u (|w g 2 d factor| + |w g d^2 factor'|)``;
* bf16 ``dpred`` within one bf16 ulp of the reference plus that.

Fused SGD: multiples of 1/8 with lr = mu = 1/2, wd = 1/4 keep every fp32
operation exact (equality); randn data with the trainer's hyper-parameters is
bounded by one fp32 rounding per operation, propagated through the steps.
"""
import functools

import pytest
import torch

import train_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd import ops
    from improved_body_parts_amd.ops import _backend
    from improved_body_parts_amd.ops import optim as fused_optim

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
CL = torch.channels_last
U = 2.0 ** -24


def f32(v):
    """The value a ``(float)`` cast of a Python double gives the kernels."""
    return float(torch.tensor(v, dtype=F32))


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"


def _ext():
    return _backend.hip_extension()


# ===========================================================================
# focal L2
# ===========================================================================

MTW, KTW = f32(0.1), 3.0
AB = {"ab0": (0.0, 0.0), "ab1": (f32(0.1), f32(0.02))}


class Geo:
    def __init__(self, S, N, C, hs, bs, H, W):
        self.S, self.N, self.C, self.hs, self.bs, self.H, self.W = \
            S, N, C, hs, bs, H, W


SMALL = Geo(2, 2, 6, 2, 4, 8, 24)       # C - 2 coincides with bkg_start
HEAD = Geo(3, 1, 50, 30, 48, 16, 16)    # the model's channel layout
LARGE = Geo(1, 1, 50, 30, 48, 128, 128)  # per_stack = 819 200 > 2048 * 256
TINY = Geo(2, 1, 6, 2, 4, 4, 8)         # per_stack = 192: one block per stack


def _plant_window(gt, n, c, y, x, r, units):
    """Zero the r x r window (y, x) of plane (n, c) and give it a total of
    ``units``/64, at most 64/64 per element."""
    win = gt[n, c, y * r:(y + 1) * r, x * r:(x + 1) * r]
    win.zero_()
    flat = torch.zeros(r * r, dtype=gt.dtype)
    k = 0
    while units > 0:
        flat[k] = min(units, 64) / 64.0
        units -= min(units, 64)
        k += 1
    win.copy_(flat.view(r, r))


@functools.lru_cache(maxsize=None)
def _focal_case(geo_name, r, ab_name, quarter_mask, seed):
    """fp32-valued inputs that are also exact in bf16 where they have to be
    (gt, mask), the planted positions, for ab = (0, 0)."""
    geo = {"small": SMALL, "head": HEAD, "large": LARGE,
           "tiny": TINY}[geo_name]
    S, N, C, H, W = geo.S, geo.N, geo.C, geo.H, geo.W
    g = torch.Generator().manual_seed(seed)
    # gt: multiples of 1/64; half of the windows empty, 80 % of the other
    # elements set -> about 60 % zeros
    win_on = (torch.rand(N, C, H, 1, W, 1, generator=g) < 0.5)
    win_on = win_on.expand(N, C, H, r, W, r).reshape(N, C, H * r, W * r)
    el_on = torch.rand(N, C, H * r, W * r, generator=g) < 0.8
    gt = torch.randint(1, 65, (N, C, H * r, W * r), generator=g).to(F32) / 64
    gt = gt * win_on * el_on
    # windows that average 1/128 (negative side of the 0.01 switch; r > 1)
    # and 1/64 (positive side)
    for c in range(C):
        if r > 1:
            _plant_window(gt, 0, c, 1, 2, r, r * r // 2)
        _plant_window(gt, 0, c, 2, 3, r, r * r)
    if quarter_mask:
        mask = torch.randint(0, 5, (N, 1, H * r, W * r), generator=g).to(F32) / 4
    else:
        mask = (torch.rand(N, 1, H * r, W * r, generator=g) < 0.8).to(F32)
    # pred: uniform on the 2**-24 grid torch.rand draws from, kept inside
    # [2**-13, 1 - 2**-8] so that no |u| < 1e-5 arises by chance, also after
    # rounding to bf16 (1 - 2**-8 is the largest bf16 below 1)
    pred = torch.randint(1 << 11, (1 << 24) - (1 << 16) + 1, (S, N, C, H, W),
                         generator=g).to(F32) / float(1 << 24)
    planted = None
    if ab_name == "ab0":
        gl = gt.reshape(N, C, H, r, W, r).mean(dim=(3, 5))
        pos = (gl >= 0.01).nonzero()
        neg = (gl < 0.01).nonzero()
        assert len(pos) >= 8 and len(neg) >= 8
        ip = pos[torch.randperm(len(pos), generator=g)[:8]].tolist()
        ineg = neg[torch.randperm(len(neg), generator=g)[:8]].tolist()
        zero_u = torch.zeros(S, N, C, H, W, dtype=torch.bool)
        for k in range(4):
            # u = 0: pred = 1 on the positive branch, 0 on the negative one
            pred[k % S][tuple(ip[k])] = 1.0
            zero_u[k % S][tuple(ip[k])] = True
            pred[k % S][tuple(ineg[k])] = 0.0
            zero_u[k % S][tuple(ineg[k])] = True
            # and the other way round: u = 1
            pred[k % S][tuple(ip[4 + k])] = 0.0
            pred[k % S][tuple(ineg[4 + k])] = 1.0
        planted = zero_u
    return geo, pred, gt, mask, planted


@functools.lru_cache(maxsize=None)
def _focal_ref(geo_name, r, gamma, ab_name, quarter_mask, seed, dtype_name,
               gscale):
    """Inputs rounded to the tested dtype and the fp64 oracle on them."""
    geo, pred, gt, mask, planted = _focal_case(geo_name, r, ab_name,
                                               quarter_mask, seed)
    dt = BF16 if dtype_name == "bf16" else F32
    pred, gt_d, mask_d = pred.to(dt), gt.to(dt), mask.to(dt)
    assert torch.equal(gt_d.float(), gt) and torch.equal(mask_d.float(), mask)
    alpha, beta = AB[ab_name]
    gs = torch.tensor(gscale, dtype=F32)
    o = O.focal_l2(pred, gt_d, mask_d, heat_start=geo.hs, bkg_start=geo.bs,
                   gamma=gamma, mtw=MTW, ktw=KTW, alpha=alpha, beta=beta,
                   gscale=gs)
    # condition on the reference alone: |u| >= 1e-5 except the planted zeros
    small = o["u"].abs() < 1e-5
    if planted is None:
        assert not small.any()
    else:
        assert torch.equal(small, planted)
        assert bool((o["u"][planted] == 0).all())
    # both sides of both switches occur
    gl = O._window_mean(gt.double(), r) if r > 1 else gt.double()
    assert (gl >= 0.01).any() and (gl < 0.01).any()
    if r > 1:
        assert (gl == 1 / 128).any()
    assert (gl == 1 / 64).any()
    m = O._mask_sample(mask.double(), r)
    assert (m == 0).any() and (m >= 0.5).any()
    if quarter_mask:
        assert (m == 0.5).any()
    return geo, pred, gt_d, mask_d, gs, o


def _sum_n(per_stack):
    blocks = min(-(-per_stack // 256), 2048)
    trips = -(-per_stack // (blocks * 256))
    return trips + 8 + blocks, trips


def _check_sums(sums, o, per_stack, what, extra=0):
    n, _ = _sum_n(per_stack)
    err = (sums.detach().cpu().to(F64) - o["sums"]).abs()
    bound = (n + extra) * U * o["sums_abs"]
    ratio = float((err / bound).max())
    print(f"\n[focal sums] {what}: max err/bound {ratio:.3f} (n = {n})")
    assert ratio <= 1.0, f"{what}: per-stack sums off by {ratio:.3f} x bound"


def _check_dpred(dpred, o, dtype_name, what, factor=16):
    got = dpred.detach().cpu().to(F64)
    bound = factor * U * o["dpred_abs"]
    if dtype_name == "bf16":
        bound = bound + O.bf16_ulp(o["dpred"])
    err = (got - o["dpred"]).abs()
    bad = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"\n[focal dpred] {what}: max err/bound {worst:.3f}")
    assert not bad.any(), (
        f"{what}: {int(bad.sum())} of {bad.numel()} dpred elements outside the "
        f"bound, worst {worst:.3f} x, first at {bad.nonzero()[0].tolist()}")


def _raw(geo, pred, gt, mask, gs, gamma, alpha, beta):
    ext = _ext()
    args = (geo.hs, geo.bs, gamma, MTW, KTW, alpha, beta)
    p, g_, m = pred.cuda(), gt.cuda(), mask.cuda()
    sums = ext.focal_l2_fwd(p, g_, m, *args)
    dpred = ext.focal_l2_bwd(p, g_, m, gs.cuda(), *args)
    torch.cuda.synchronize()
    assert sums.dtype == F32 and dpred.dtype == pred.dtype
    return sums, dpred


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
@pytest.mark.parametrize("ab_name", ["ab0", "ab1"])
@pytest.mark.parametrize("gamma", [1, 2])
@pytest.mark.parametrize("r", [1, 2, 4, 16])
def test_focal_kernels_vs_oracle(r, gamma, ab_name, dtype_name):
    """Raw bindings on a non-square 8 x 24 map with C = 6, heat_start = 2,
    bkg_start = 4, two stacks with different upstream scales."""
    geo, pred, gt, mask, gs, o = _focal_ref(
        "small", r, gamma, ab_name, False, 100 + r, dtype_name, (0.75, -1.5))
    alpha, beta = AB[ab_name]
    sums, dpred = _raw(geo, pred, gt, mask, gs, gamma, alpha, beta)
    what = f"r={r} gamma={gamma} {ab_name} {dtype_name}"
    _check_sums(sums, o, pred[0].numel(), what)
    _check_dpred(dpred, o, dtype_name, what)


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
@pytest.mark.parametrize("gamma", [1, 2])
def test_focal_quarter_mask_bilinear_lands_on_threshold(gamma, dtype_name):
    """A mask of multiples of 1/4 at r = 2: bilinear values are exact
    multiples of 1/16 and some equal 0.5, which is kept."""
    geo, pred, gt, mask, gs, o = _focal_ref(
        "small", 2, gamma, "ab0", True, 7, dtype_name, (1.0, 1.0))
    sums, dpred = _raw(geo, pred, gt, mask, gs, gamma, 0.0, 0.0)
    what = f"quarter mask gamma={gamma} {dtype_name}"
    _check_sums(sums, o, pred[0].numel(), what)
    _check_dpred(dpred, o, dtype_name, what)


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
@pytest.mark.parametrize("gamma", [1, 2])
def test_focal_loss_autograd_three_weighted_stacks(gamma, dtype_name):
    """``ops.focal_l2_loss`` at C = 50 (heat_start 30, bkg_start 48), S = 3
    with nstack_weight (1, 2, 4), r = 4, and the loss multiplied by 3 before
    backward: the per-stack scale 3 w_j / 7 reaches dpred."""
    nw = (1, 2, 4)
    # what ops/loss.py hands the kernel: fp32 (3 * nw) / 7
    gs32 = (torch.tensor(3.0, dtype=F32) * torch.tensor(nw, dtype=F32)
            / torch.tensor(nw, dtype=F32).sum())
    geo, pred, gt, mask, gs, o = _focal_ref(
        "head", 4, gamma, "ab0", False, 11, dtype_name,
        tuple(float(v) for v in gs32))
    p = pred.cuda().requires_grad_(True)
    loss = ops.focal_l2_loss(p, gt.cuda(), mask.cuda(), heat_start=geo.hs,
                             bkg_start=geo.bs, gamma=gamma,
                             multi_task_weight=0.1, keypoint_task_weight=3.0,
                             nstack_weight=nw)
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    what = f"autograd S=3 gamma={gamma} {dtype_name}"
    _check_dpred(p.grad, o, dtype_name, what)
    # loss = sum_j nw_j sums_j / 7: the sums' bound plus the 3 products, 2
    # additions and the division of the fp32 host expression
    n, _ = _sum_n(pred[0].numel())
    nw64 = torch.tensor(nw, dtype=F64)
    want = float((o["sums"] * nw64).sum() / 7)
    bound = (n + 6) * U * float((o["sums_abs"] * nw64).sum() / 7)
    err = abs(float(loss.detach().double()) - want)
    print(f"\n[focal loss] {what}: err/bound {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16"])
def test_focal_grid_stride_second_trip(dtype_name):
    """One 1 x 50 x 128 x 128 stack: per_stack = 819 200 exceeds the 2048 x 256
    threads of the capped grid, so the grid-stride loops take a second trip."""
    geo, pred, gt, mask, gs, o = _focal_ref(
        "large", 2, 2, "ab1", False, 21, dtype_name, (1.0,))
    per_stack = pred[0].numel()
    n, trips = _sum_n(per_stack)
    assert per_stack == 819200 and trips == 2 and n == 2 + 8 + 2048
    alpha, beta = AB["ab1"]
    sums, dpred = _raw(geo, pred, gt, mask, gs, 2, alpha, beta)
    what = f"large {dtype_name}"
    _check_sums(sums, o, per_stack, what)
    _check_dpred(dpred, o, dtype_name, what)


def test_focal_planted_zero_u_gives_zero_gradient():
    """gamma = 1 at u = 0 exactly (pred = 1 on a positive element, pred = 0 on
    a negative one): factor = 0 and sign(0) = 0, so dpred is exactly 0."""
    geo, pred, gt, mask, gs, o = _focal_ref(
        "small", 2, 1, "ab0", False, 102, "fp32", (0.75, -1.5))
    _, _, _, _, planted = _focal_case("small", 2, "ab0", False, 102)
    assert int(planted.sum()) == 8
    _, dpred = _raw(geo, pred, gt, mask, gs, 1, 0.0, 0.0)
    assert bool((dpred.cpu()[planted] == 0).all())
    assert bool((o["dpred"][planted] == 0).all())


def test_focal_mixed_dtypes_are_cast_not_reinterpreted():
    """bf16 pred with fp32 gt / mask through the public op equals the all-bf16
    call bit for bit, loss and gradient (the kernels read gt and mask with
    pred's element type). 192 elements per stack: one block and one atomicAdd
    per stack, so the forward sum is repeatable too."""
    geo, pred, gt, mask, gs, o = _focal_ref(
        "tiny", 2, 2, "ab1", False, 41, "bf16", (1.0 / 3, 2.0 / 3))
    assert pred[0].numel() <= 256
    kw = dict(heat_start=geo.hs, bkg_start=geo.bs, gamma=2,
              multi_task_weight=0.1, keypoint_task_weight=3.0,
              nstack_weight=(1, 2), alpha=0.1, beta=0.02)
    pa = pred.cuda().requires_grad_(True)
    la = ops.focal_l2_loss(pa, gt.cuda(), mask.cuda(), **kw)
    la.backward()
    pb = pred.cuda().requires_grad_(True)
    lb = ops.focal_l2_loss(pb, gt.float().cuda(), mask.float().cuda(), **kw)
    lb.backward()
    torch.cuda.synchronize()
    assert torch.equal(la.detach(), lb.detach())
    assert torch.equal(pa.grad, pb.grad)
    _check_dpred(pb.grad, o, "bf16", "mixed dtypes")
    _check_sums(torch.stack([la.detach() * 3]), {
        "sums": (o["sums"] * torch.tensor([1.0, 2.0], dtype=F64)).sum().view(1),
        "sums_abs": (o["sums_abs"] * torch.tensor([1.0, 2.0], dtype=F64))
        .sum().view(1)}, pred[0].numel(), "mixed dtypes loss", extra=6)


def test_focal_bindings_reject_mismatched_inputs():
    ext = _ext()
    S, N, C, H, W = 2, 2, 6, 8, 24
    pred = torch.rand(S, N, C, H, W, device="cuda")
    gt = torch.rand(N, C, 2 * H, 2 * W, device="cuda")
    mask = torch.ones(N, 1, 2 * H, 2 * W, device="cuda")
    gs = torch.ones(S, device="cuda")
    args = (2, 4, 2, 0.1, 3.0, 0.0, 0.0)
    bad = [
        (pred.bfloat16(), gt, mask),                 # would read garbage
        (pred, gt.bfloat16(), mask),                 # would read past the end
        (pred, gt, mask.bfloat16()),
        (pred, gt[:, :5].contiguous(), mask),        # gt with another C
        (pred, gt[:1].contiguous(), mask[:1].contiguous()),   # another N
        (pred, gt, mask.expand(N, C, 2 * H, 2 * W).contiguous()),
        (pred, gt, torch.ones(N, 1, H, W, device="cuda")),    # mask at low res
        (pred, gt, mask[:, 0]),                      # 3-D mask
    ]
    for p, g_, m in bad:
        with pytest.raises(RuntimeError, match="focal_l2"):
            ext.focal_l2_fwd(p, g_, m, *args)
        with pytest.raises(RuntimeError, match="focal_l2"):
            ext.focal_l2_bwd(p, g_, m, gs, *args)
    with pytest.raises(RuntimeError, match="stack_gscale"):
        ext.focal_l2_bwd(pred, gt, mask, gs[:1].contiguous(), *args)
    with pytest.raises(RuntimeError, match="stack_gscale"):
        ext.focal_l2_bwd(pred, gt, mask, gs.double(), *args)
    # and the well-formed call still runs
    ext.focal_l2_fwd(pred, gt, mask, *args)
    ext.focal_l2_bwd(pred, gt, mask, gs, *args)
    torch.cuda.synchronize()


# ===========================================================================
# fused SGD
# ===========================================================================

# (dtype, shape): fp32 BN-style parameters sit between bf16 ones; numel
# brackets the 65 536-element chunk; one 4-D bf16 weight
SGD_PARAMS = [(BF16, (1,)), (F32, (7,)), (BF16, (65535,)), (BF16, (65536,)),
              (F32, (65537,)), (BF16, (65537,)), (BF16, (196613,)),
              (BF16, (8, 4, 3, 3))]


def _eighths(g, shape):
    return torch.randint(-16, 17, shape, generator=g).to(F32) / 8


def _make_batch(w0s):
    """Device parameters with zero momentum and, for bf16, an fp32 master."""
    batch = []
    for (dt, _), w0 in zip(SGD_PARAMS, w0s):
        p = w0.to(dt).cuda()
        m = torch.zeros(w0.shape, dtype=F32, device="cuda")
        master = w0.to(F32).cuda() if dt == BF16 else None
        batch.append([p, None, m, master])
    return batch


def _step(batch, grads, lr, mu, wd):
    for row, g in zip(batch, grads):
        row[1] = g.to(row[0].dtype).cuda()
    fused_optim.fused_sgd_step([tuple(r) for r in batch], lr, mu, wd)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mu,wd", [(0.5, 0.25), (0.0, 0.25), (0.5, 0.0)],
                         ids=["mu-wd", "no-momentum", "no-decay"])
def test_sgd_exact_three_steps(mu, wd):
    """Multiples of 1/8 in [-2, 2], lr = 1/2: after three steps every value is
    a multiple of 2**-12 below 16, so each fp32 operation is exact with or
    without FMA contraction. Momentum, master and fp32 parameters equal the
    oracle; bf16 parameters equal bf16(master)."""
    g = torch.Generator().manual_seed(31)
    lr = 0.5
    w0s = [_eighths(g, shape) for _, shape in SGD_PARAMS]
    grads = [[_eighths(g, shape) for _, shape in SGD_PARAMS] for _ in range(3)]
    batch = _make_batch(w0s)
    want = [O.sgd_steps(w0, [gr[i] for gr in grads], lr, mu, wd)
            for i, w0 in enumerate(w0s)]
    for t in range(3):
        _step(batch, grads[t], lr, mu, wd)
        for i, ((dt, shape), (p, _, m, master)) in enumerate(
                zip(SGD_PARAMS, batch)):
            w64, m64, wb = want[i][t]
            what = f"step {t} param {i} {dt} {shape}"
            assert torch.equal(m.cpu().to(F64), m64), what + " momentum"
            if dt == BF16:
                assert torch.equal(master.cpu().to(F64), w64), what + " master"
                assert torch.equal(p.cpu(), wb), what + " bf16 copy"
            else:
                assert torch.equal(p.cpu().to(F64), w64), what + " fp32 param"


def _sgd_bound(w0, grads, lr, mu, wd):
    """fp64 trajectory and the propagated bound of an fp32 evaluation with one
    rounding per operation (t = wd w, g + t, mu m, + , lr m, w - .):
        Eg = wd Ew + u (|wd w| + |gv|)
        Em = mu Em + Eg + u (|mu m| + |m'|)
        Ew = Ew + lr Em + u (|lr m'| + |w'|)
    Magnitudes are the oracle's; the factor 1 + 2**-10 covers their own error."""
    steps = O.sgd_steps(w0, grads, lr, mu, wd)
    w, m = w0.to(F64), torch.zeros_like(w0, dtype=F64)
    Ew, Em = torch.zeros_like(w), torch.zeros_like(w)
    out = []
    for g, (w1, m1, _) in zip(grads, steps):
        gv = g.to(F64) + wd * w
        Eg = wd * Ew + U * ((wd * w).abs() + gv.abs())
        Em = mu * Em + Eg + U * ((mu * m).abs() + m1.abs())
        Ew = Ew + lr * Em + U * ((lr * m1).abs() + w1.abs())
        w, m = w1, m1
        out.append((w1, m1, Ew * (1 + 2.0 ** -10), Em * (1 + 2.0 ** -10)))
    return out


def test_sgd_precision_five_steps():
    """randn data with the trainer's hyper-parameters (as the kernel sees
    them: cast to fp32)."""
    from improved_body_parts_amd.config import TrainingOpt
    opt = TrainingOpt()
    lr, mu, wd = f32(opt.learning_rate), f32(opt.momentum), f32(opt.weight_decay)
    assert (opt.learning_rate, opt.momentum, opt.weight_decay) == \
        (2.5e-5, 0.9, 2e-4)
    g = torch.Generator().manual_seed(32)
    w0s = [torch.randn(shape, generator=g).to(dt).to(F32)
           for dt, shape in SGD_PARAMS]
    grads = [[torch.randn(shape, generator=g).to(dt).to(F32)
              for dt, shape in SGD_PARAMS] for _ in range(5)]
    batch = _make_batch(w0s)
    want = [_sgd_bound(w0, [gr[i] for gr in grads], lr, mu, wd)
            for i, w0 in enumerate(w0s)]
    worst = 0.0
    for t in range(5):
        _step(batch, grads[t], lr, mu, wd)
        for i, ((dt, shape), (p, _, m, master)) in enumerate(
                zip(SGD_PARAMS, batch)):
            w64, m64, Ew, Em = want[i][t]
            what = f"step {t} param {i} {dt} {shape}"
            em = (m.cpu().to(F64) - m64).abs()
            wk = (master if dt == BF16 else p).cpu()
            ew = (wk.to(F64) - w64).abs()
            assert bool((em <= Em).all()), what + " momentum"
            assert bool((ew <= Ew).all()), what + " weights"
            worst = max(worst, float((em / Em).max()), float((ew / Ew).max()))
            if dt == BF16:
                assert torch.equal(p.cpu(), wk.to(BF16)), \
                    what + ": bf16 copy is not RNE(master)"
    print(f"\n[sgd precision] worst err/bound over 5 steps {worst:.3f}")


def test_sgd_table_is_rebuilt_when_gradients_move(monkeypatch):
    """Same tensors: the cached table is reused. Gradients replaced by new
    tensors (set_to_none): the table is rebuilt, not just re-run, and the
    step uses the new gradients. Every step ticks every ``_version``."""
    builds = []
    real = fused_optim._build_table
    monkeypatch.setattr(fused_optim, "_build_table",
                        lambda b, d: builds.append(1) or real(b, d))
    g = torch.Generator().manual_seed(33)
    lr, mu, wd = 0.5, 0.5, 0.25
    shapes = [(BF16, (65537,)), (F32, (7,)), (BF16, (8, 4, 3, 3))]
    w0s = [_eighths(g, s) for _, s in shapes]
    grads = [[_eighths(g, s) for _, s in shapes] for _ in range(3)]
    ps = [w.to(dt).cuda() for (dt, _), w in zip(shapes, w0s)]
    ms = [torch.zeros(w.shape, device="cuda") for w in w0s]
    masters = [w.cuda() if dt == BF16 else None
               for (dt, _), w in zip(shapes, w0s)]
    gbuf = [gr.to(dt).cuda() for (dt, _), gr in zip(shapes, grads[0])]
    versions = [p._version for p in ps]

    def step():
        fused_optim.fused_sgd_step(list(zip(ps, gbuf, ms, masters)), lr, mu, wd)
        torch.cuda.synchronize()
        for i, p in enumerate(ps):
            assert p._version > versions[i]
            versions[i] = p._version

    step()
    assert len(builds) == 1
    for b, gr in zip(gbuf, grads[1]):      # same storage, new values
        b.copy_(gr)
    step()
    assert len(builds) == 1, "an unchanged batch must reuse its table"
    old = gbuf                              # kept alive: the new ones must move
    gbuf = [gr.to(dt).cuda() for (dt, _), gr in zip(shapes, grads[2])]
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(old, gbuf))
    step()
    assert len(builds) == 2, "moved gradients must rebuild the table"
    for i, ((dt, _), w0) in enumerate(zip(shapes, w0s)):
        w64, m64, wb = O.sgd_steps(w0, [gr[i] for gr in grads], lr, mu, wd)[-1]
        assert torch.equal(ms[i].cpu().to(F64), m64)
        if dt == BF16:
            assert torch.equal(masters[i].cpu().to(F64), w64)
            assert torch.equal(ps[i].cpu(), wb)
        else:
            assert torch.equal(ps[i].cpu().to(F64), w64)


def test_sgd_channels_last_parameter_with_contiguous_gradient():
    """The kernel pairs param / grad / momentum / master by linear memory
    offset. A channels-last parameter handed a contiguous gradient must still
    be updated element by element like ``torch.optim.SGD`` on the same
    logical tensors."""
    from improved_body_parts_amd.config import TrainingOpt
    from improved_body_parts_amd.engine import FusedSGD
    opt = TrainingOpt()
    # a learning rate at which a permuted gradient cannot hide in rounding
    lr, mu, wd = f32(0.05), f32(opt.momentum), f32(opt.weight_decay)
    g = torch.Generator().manual_seed(34)
    w0 = torch.randn(8, 4, 3, 3, generator=g).to(BF16)
    grads = [torch.randn(8, 4, 3, 3, generator=g).to(BF16) for _ in range(3)]
    p = torch.nn.Parameter(w0.cuda().contiguous(memory_format=CL))
    assert p.is_contiguous(memory_format=CL) and not p.is_contiguous()
    sgd = FusedSGD([p], lr=lr, momentum=mu, weight_decay=wd)
    ref_p = torch.nn.Parameter(w0.to(F64))
    ref = torch.optim.SGD([ref_p], lr=lr, momentum=mu, weight_decay=wd)
    want = _sgd_bound(w0.to(F32), [gr.to(F32) for gr in grads], lr, mu, wd)
    for t, gr in enumerate(grads):
        p.grad = gr.cuda().contiguous()
        assert p.grad.is_contiguous() and p.grad.stride() != p.stride()
        sgd.step()
        ref_p.grad = gr.to(F64)
        ref.step()
        torch.cuda.synchronize()
        w64, m64, Ew, Em = want[t]
        torch.testing.assert_close(w64, ref_p.detach(), rtol=1e-13, atol=1e-14)
        master = sgd.state[p]["master"].cpu().to(F64)
        mom = sgd.state[p]["momentum_buffer"].cpu().to(F64)
        assert bool(((master - ref_p.detach()).abs() <= Ew).all()), \
            f"step {t}: master differs from torch.optim.SGD"
        assert bool(((mom - ref.state[ref_p]["momentum_buffer"]).abs()
                     <= Em).all()), f"step {t}: momentum"
        assert torch.equal(p.detach().cpu(),
                           sgd.state[p]["master"].cpu().to(BF16))
        assert p.is_contiguous(memory_format=CL)


def test_sgd_step_rejects_rows_with_different_layouts():
    fused_optim._table_cache.clear()
    w = torch.randn(8, 4, 3, 3).to(BF16).cuda()
    p = w.contiguous(memory_format=CL)
    ok = (p, torch.zeros_like(p), torch.zeros_like(p, dtype=F32), p.float())
    assert ok[2].stride() == p.stride() and ok[3].stride() == p.stride()
    fused_optim.fused_sgd_step([ok], 0.1, 0.9, 0.0)     # well-formed: runs
    rows = [
        (p, torch.zeros_like(w), ok[2], ok[3]),                  # grad
        (p, ok[1], torch.zeros_like(w, dtype=F32), ok[3]),       # momentum
        (p, ok[1], ok[2], w.float()),                            # master
        (p[:, ::2], ok[1][:, ::2], ok[2][:, ::2], ok[3][:, ::2]),  # not dense
        (p, ok[1].float(), ok[2], ok[3]),                        # grad dtype
        (p, ok[1], ok[2].to(BF16), ok[3]),                       # momentum dtype
    ]
    for row in rows:
        fused_optim._table_cache.clear()
        with pytest.raises(ValueError, match="fused_sgd_step"):
            fused_optim.fused_sgd_step([row], 0.1, 0.9, 0.0)
    torch.cuda.synchronize()
    # a 1x1 conv weight: the strides of length-1 dimensions do not matter
    q = torch.zeros(16, 4, 1, 1, device="cuda")
    qg = torch.zeros(64, device="cuda").as_strided((16, 4, 1, 1), (4, 1, 4, 4))
    assert q.stride() != qg.stride()
    fused_optim._table_cache.clear()
    fused_optim.fused_sgd_step([(q, qg, torch.zeros_like(q), None)],
                               0.1, 0.9, 0.0)
    torch.cuda.synchronize()
