"""Two-source 1x1 conv on the CPU: the identity, the reference pack, the planner.

``bn_a(conv_a(y)) + bn_b(conv_b(x))`` in eval mode is one 1x1 conv over the
channel-concatenated inputs whose weight rows carry the folded BN scales and
whose shift is the sum of the folded shifts. ``tests/csrc/cat_plan_check.cpp``
drives ``plan_conv`` / ``assemble_group`` for the two-source guards, compiled
with the host compiler under AddressSanitizer and UBSan and run as a child
process (as ``test_conv_plan_cpu.py`` does for the rest of the planner).
"""
import json
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from improved_body_parts_amd.ops import conv_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "improved_body_parts_amd", "ops", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all"]

# (M as N, H, W), Cin, Cin2, Cout -> (BM, BN, splitk, deep), K-chunks per slice
# By hand from pick_tile / pick_split (target 384): BM 32 up to M 2048, 64 up
# to 8192, else 128; BN 128 only with BM 128 where it pads no more than 64;
# split = ceil(384 / ntiles) normalised so that every slice has chunks; deep
# when a slice has at most 6 chunks. The GPU test runs these very cases.
CAT_PLANS = [
    ((1, 5, 7), 64, 64, 40, (32, 64, 2, 1), 1),      # 2 tiles, 2 chunks
    ((2, 16, 16), 192, 512, 640, (32, 64, 3, 1), 4),  # 160 tiles, 11 chunks
    ((1, 64, 64), 64, 128, 384, (64, 64, 1, 1), 3),   # 384 tiles
    ((1, 64, 64), 192, 512, 384, (64, 64, 1, 0), 11),
    ((1, 96, 96), 64, 128, 768, (128, 128, 1, 1), 3),  # 72 x 6 = 432 tiles
    ((1, 96, 96), 192, 256, 768, (128, 128, 1, 0), 7),
    ((1, 96, 96), 64, 64, 192, (128, 64, 2, 1), 1),   # 72 x 3 = 216 tiles
]


def _folded(gen, c):
    """eval-mode BN as (scale, shift) in float64."""
    gamma = torch.rand(c, generator=gen, dtype=torch.float64) * 1.5 + 0.5
    beta = torch.randn(c, generator=gen, dtype=torch.float64)
    mean = torch.randn(c, generator=gen, dtype=torch.float64) * 0.1
    var = torch.rand(c, generator=gen, dtype=torch.float64) + 0.5
    scale = gamma / torch.sqrt(var + 1e-5)
    return scale, beta - mean * scale


@pytest.mark.parametrize("ca,cb,cout", [(64, 64, 40), (256, 50, 384)])
def test_identity_in_float64(ca, cb, cout):
    gen = torch.Generator().manual_seed(ca + cb)
    a = torch.randn(2, ca, 5, 7, generator=gen, dtype=torch.float64)
    b = torch.randn(2, cb, 5, 7, generator=gen, dtype=torch.float64)
    wa = torch.randn(cout, ca, 1, 1, generator=gen, dtype=torch.float64)
    wb = torch.randn(cout, cb, 1, 1, generator=gen, dtype=torch.float64)
    (sa, ta), (sb, tb) = _folded(gen, cout), _folded(gen, cout)
    v = lambda t: t.view(1, -1, 1, 1)
    ref = F.leaky_relu(F.conv2d(a, wa) * v(sa) + v(ta)
                       + F.conv2d(b, wb) * v(sb) + v(tb), 0.01)
    wcat = torch.cat([wa * sa.view(-1, 1, 1, 1), wb * sb.view(-1, 1, 1, 1)],
                     dim=1)
    cat = F.leaky_relu(F.conv2d(torch.cat([a, b], dim=1), wcat)
                       + v(ta + tb), 0.01)
    assert float((cat - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_reference_pack_layout_and_rounding():
    gen = torch.Generator().manual_seed(3)
    cout, ca, cb = 6, 64, 10
    wa = torch.randn(cout, ca, 1, 1, generator=gen).bfloat16()
    wb = torch.randn(cout, cb, 1, 1, generator=gen).bfloat16()
    sa = torch.rand(cout, generator=gen) + 0.5
    ta = torch.randn(cout, generator=gen)
    tb = torch.randn(cout, generator=gen)
    pack, shift = conv_kernels.cat_weight_reference(wa, wb, sa, None, ta, tb)
    assert pack.shape == (cout, ca + cb) and pack.dtype == torch.bfloat16
    assert pack.is_contiguous() and shift.dtype == torch.float32
    # source a first, scaled in fp32 and rounded once; b unscaled = unchanged
    want_a = (wa.float().view(cout, ca) * sa.view(-1, 1)).bfloat16()
    assert torch.equal(pack[:, :ca], want_a)
    assert torch.equal(pack[:, ca:], wb.view(cout, cb))
    assert torch.equal(shift, ta + tb)
    pack0, shift0 = conv_kernels.cat_weight_reference(wa, wb)
    assert torch.equal(pack0, torch.cat([wa.view(cout, ca),
                                         wb.view(cout, cb)], dim=1))
    assert torch.equal(shift0, torch.zeros(cout))


# ---------------------------------------------------------------------------
# planner
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler (c++) on this machine")
    exe = str(tmp_path_factory.mktemp("cat_plan") / "cat_plan_check")
    cmd = [cxx, *FLAGS, "-I", CSRC,
           os.path.join(ROOT, "tests", "csrc", "cat_plan_check.cpp"),
           "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"],
                      capture_output=True).returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
        assert built.returncode == 0, built.stderr[-4000:]

    def run(lines):
        env = {k: v for k, v in os.environ.items()
               if k not in ("IBP_CONV_BM", "IBP_SPLITK_TARGET")}
        out = subprocess.run([exe], input="\n".join(lines) + "\n", text=True,
                             capture_output=True, env=env, timeout=120)
        assert out.returncode == 0, out.stderr[-4000:]
        assert not out.stderr, out.stderr[-4000:]
        res = [json.loads(l) for l in out.stdout.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


A = 1 << 24


def _conv(n, h, w, cin, cout, cin2, x2=2 * A, k=1, stride=1, pad=0, dil=1,
          zs=1, up=0, tile=0, push=0, ho=None, wo=None):
    geom = [n, h, w, cin, cout, k, k, stride, pad, pad, dil, dil,
            h if ho is None else ho, w if wo is None else wo, zs]
    return "conv " + " ".join(str(v) for v in (*geom, A, x2, cin2, up, tile,
                                               push))


def test_cat_plans_are_those_of_a_conv_over_the_summed_k(check):
    res = check([_conv(*nhw, cin, cout, cin2)
                 for nhw, cin, cin2, cout, _, _ in CAT_PLANS]
                + [_conv(*nhw, cin + cin2, cout, 0, x2=0)
                   for nhw, cin, cin2, cout, _, _ in CAT_PLANS])
    n = len(CAT_PLANS)
    for (nhw, cin, cin2, cout, plan, nk), r, plain in zip(CAT_PLANS, res[:n],
                                                          res[n:]):
        assert r["K"] == cin + cin2 and r["M"] == nhw[0] * nhw[1] * nhw[2]
        assert (r["Cin"], r["Cin2"], r["x2"]) == (cin, cin2, 2 * A)
        assert (r["BM"], r["BN"], r["splitk"], r["deep"]) == plan, (nhw, cin)
        assert r["nk_block"] == nk
        # tile, split and depth of the plain conv with K = Cin + Cin2
        for key in ("BM", "BN", "splitk", "deep", "nblocks", "ws_elems", "K"):
            assert r[key] == plain[key], key
        assert plain["Cin2"] == 0 and plain["x2"] == 0


def test_odd_second_source_plans(check):
    a, b = check([_conv(1, 5, 7, 64, 50, 50), _conv(1, 5, 7, 256, 384, 50)])
    assert a["K"] == 114 and a["vec_epi"] == 0
    assert b["K"] == 306 and b["nk_block"] * b["splitk"] >= 5


def test_guards(check):
    ok = _conv(1, 8, 8, 64, 64, 64)
    bad = {
        "Cin % 64": _conv(1, 8, 8, 48, 64, 64),
        "Cin 0": _conv(1, 8, 8, 0, 64, 64),
        "3x3": _conv(1, 8, 8, 64, 64, 64, k=3, pad=1),
        "stride": _conv(1, 8, 8, 64, 64, 64, stride=2, ho=4, wo=4),
        "pad": _conv(1, 8, 8, 64, 64, 64, pad=1, ho=10, wo=10),
        "dilation": _conv(1, 8, 8, 64, 64, 64, dil=2),
        "zs": _conv(1, 8, 8, 64, 64, 64, zs=2),
        "up": _conv(1, 8, 8, 64, 64, 64, up=1),
        "Cin2 0": _conv(1, 8, 8, 64, 64, 0),
        "Cin2 < 0": _conv(1, 8, 8, 64, 64, -8),
        "Cin2 without x2": _conv(1, 8, 8, 64, 64, 64, x2=0),
        "foreign tile": _conv(1, 8, 8, 64, 64, 64, tile=1),
    }
    res = check([ok] + list(bad.values()))
    assert "error" not in res[0] and res[0]["K"] == 128
    for name, r in zip(bad, res[1:]):
        assert "two-source conv" in r.get("error", ""), (name, r)


def test_group_refuses_a_two_source_member(check):
    plain = _conv(1, 8, 8, 64, 64, 0, x2=0, push=1)
    cat = _conv(1, 8, 8, 64, 64, 64, push=1)
    res = check([plain, plain, cat, "group 0 2 4096", "group 0 3 4096",
                 "group 2 3 4096"])
    assert res[3]["n"] == 2
    assert "two-source" in res[4]["error"]
    assert "two-source" in res[5]["error"]
