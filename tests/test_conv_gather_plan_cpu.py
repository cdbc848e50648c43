"""Which gather the MFMA conv's planner picks (ops/csrc/conv_plan.h), on the
CPU.

``tests/csrc/conv_gather_check.cpp`` is compiled once with the host compiler
under AddressSanitizer and UBSan and driven as a child process, like
``conv_plan_check.cpp``: commands on stdin, one JSON object per command.

The rule (``gather_eligible``): tap-uniform (1) when the conv has one source,
``zs == 1``, ``Cin % 64 == 0``, ``KH*KW <= 32``, 16-byte aligned ``x`` and
``w``, ``m32``, and both operands at most 2^31 - 1 bytes long (the kernel's
unsigned 32-bit byte offsets; 2^31 is its out-of-range offset); generic (0)
otherwise and whenever ``IBP_CONV_GATHER=0``.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "improved_body_parts_amd", "ops", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all"]
ENV_KEYS = ("IBP_CONV_BM", "IBP_SPLITK_TARGET", "IBP_CONV_GATHER")
A = 1 << 24          # made-up addresses, 256-byte aligned, far apart
X, W, X2 = A, 2 * A, 3 * A


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(lines, **env) -> list of dicts, one per command."""
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler (c++) on this machine")
    exe = str(tmp_path_factory.mktemp("conv_gather") / "conv_gather_check")
    cmd = [cxx, *FLAGS, "-I", CSRC,
           os.path.join(ROOT, "tests", "csrc", "conv_gather_check.cpp"),
           "-o", exe]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"],
                      capture_output=True).returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
        assert built.returncode == 0, built.stderr[-4000:]

    def run(lines, **env):
        child_env = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
        child_env.update(env)
        out = subprocess.run([exe], input="\n".join(lines) + "\n", text=True,
                             capture_output=True, env=child_env, timeout=120)
        assert out.returncode == 0, out.stderr[-4000:]
        assert not out.stderr, out.stderr[-4000:]
        res = [json.loads(l) for l in out.stdout.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


def _geom(n=2, h=9, w=9, cin=128, cout=40, k=3, stride=1, dil=1, zs=1,
          ho=None, wo=None):
    pad = dil * (k - 1) // 2
    ho = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1 if ho is None else ho
    wo = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1 if wo is None else wo
    return [n, h, w, cin, cout, k, k, stride, pad, pad, dil, dil, ho, wo, zs]


def _plan(geom, x=X, w=W, x2=0, cin2=0, push=0):
    assert len(geom) == 15
    return "plan " + " ".join(str(v) for v in (*geom, x, w, x2, cin2, push))


def test_eligible_shapes_of_the_model(check):
    cases = [
        _geom(),                                   # 3x3 Cin 128
        _geom(cin=64, cout=64, h=5, w=7, n=1),     # M below every tile
        _geom(cin=64, stride=2, h=10, w=10),       # strided
        _geom(cin=64, dil=3, h=12, w=12),          # the dilated block
        _geom(cin=64, dil=5, h=12, w=12),
        _geom(cin=192, cout=384, k=1, h=6, w=6),   # 1x1 (one tap)
        _geom(cin=64, k=5),                        # 25 taps
        [2, 4, 6, 64, 64, 2, 2, 1, 1, 0, 1, 1, 4, 6, 1],   # an upfold parity
    ]
    for g, r in zip(cases, check([_plan(g) for g in cases])):
        assert r["gather"] == 1 and r["m32"] == 1, g


def test_each_condition_failing_alone(check):
    base = _geom(cin=64, cout=64, k=1, h=8, w=8)
    assert len(base) == 15
    rows = {
        "base": _plan(base),
        # two sources (legal only as a plain 1x1 conv)
        "two sources": _plan(base, x2=X2, cin2=64),
        # zs = 2: the dgrad of a stride-2 conv
        "zs": _plan(_geom(cin=64, cout=64, k=3, h=5, w=5, zs=2, ho=9, wo=9)),
        "Cin % 64 (50)": _plan(_geom(cin=50, cout=64, k=1, h=8, w=8)),
        "Cin % 64 (16)": _plan(_geom(cin=16, cout=64, k=7, stride=2)),
        "Cin % 64 (96)": _plan(_geom(cin=96, cout=64, k=3)),
        "taps 36": _plan(_geom(cin=64, k=6, ho=9, wo=9)),
        "x + 8": _plan(base, x=X + 8),
        "x + 2": _plan(base, x=X + 2),
        "w + 8": _plan(base, w=W + 8),
        # M + BM reaches 2^31 over a tiny input (Ho, Wo are the caller's)
        "m32": _plan(_geom(n=1, cin=64, cout=64, k=1, h=1, w=1, ho=1,
                           wo=2**31 - 128)),
    }
    res = dict(zip(rows, check(list(rows.values()))))
    assert res["base"]["gather"] == 1
    for name, r in res.items():
        if name != "base":
            assert r["gather"] == 0, name
    assert res["m32"]["m32"] == 0
    assert all(r["m32"] == 1 for n, r in res.items() if n != "m32")
    # the neighbours of the failing values are eligible
    near = [_plan(_geom(cin=64, k=5)),               # 25 taps
            _plan(base, x=X + 16), _plan(base, w=W + 16),
            _plan(_geom(n=1, cin=64, cout=64, k=1, h=1, w=1, ho=1,
                        wo=2**31 - 129))]
    assert [r["gather"] for r in check(near)] == [1, 1, 1, 1]


def test_taps_bound_is_32(check):
    # 4 x 8 = 32 taps fit the row mask, 33 (3 x 11) do not
    def g(kh, kw):
        return [1, 16, 16, 64, 64, kh, kw, 1, 0, 0, 1, 1, 16 - kh + 1,
                16 - kw + 1, 1]
    r32, r33 = check([_plan(g(4, 8)), _plan(g(3, 11))])
    assert (r32["gather"], r33["gather"]) == (1, 0)


def test_address_width_bound_at_its_edge(check):
    """Offsets are unsigned 32-bit BYTE offsets and 2^31 is the out-of-range
    offset: an operand may be 2^31 - 1 bytes long. With Cin % 64 == 0 sizes
    are multiples of 128 bytes: 2^31 - 128 is in, 2^31 is out."""
    def x_of(pixels):     # 1x1 over a 1 x pixels map, Cin 64: 128 B / pixel
        return _plan([1, 1, pixels, 64, 64, 1, 1, 1, 0, 0, 1, 1, 1, pixels, 1])

    def w_of(cout):       # 1x1, Cin 64: 128 B per weight row
        return _plan([1, 8, 8, 64, cout, 1, 1, 1, 0, 0, 1, 1, 8, 8, 1])
    xin, xout, win, wout = check([x_of(2**24 - 1), x_of(2**24),
                                  w_of(2**24 - 1), w_of(2**24)])
    assert xin["M"] * 128 == 2**31 - 128 and xin["gather"] == 1
    assert xout["M"] * 128 == 2**31 and xout["gather"] == 0
    assert xin["m32"] == xout["m32"] == 1
    assert (win["gather"], wout["gather"]) == (1, 0)
    # the batch and the rows count as much as the columns
    big = [128, 512, 512, 64, 64, 3, 3, 1, 1, 1, 1, 1, 512, 512, 1]   # 4 GiB
    half = [32, 512, 512, 64, 64, 3, 3, 1, 1, 1, 1, 1, 512, 512, 1]   # 1 GiB
    assert [r["gather"] for r in check([_plan(big), _plan(half)])] == [0, 1]


def test_env_switch_forces_generic(check):
    cmds = [_plan(_geom()), _plan(_geom(cin=64, k=1)),
            _plan(_geom(cin=50, k=1))]
    assert [r["gather"] for r in check(cmds)] == [1, 1, 0]
    assert [r["gather"] for r in check(cmds, IBP_CONV_GATHER="0")] == [0, 0, 0]
    assert [r["gather"] for r in check(cmds, IBP_CONV_GATHER="1")] == [1, 1, 0]
    # the switch changes nothing else of the plan
    on, off = check(cmds), check(cmds, IBP_CONV_GATHER="0")
    for a, b in zip(on, off):
        assert {k: v for k, v in a.items() if k != "gather"} == \
            {k: v for k, v in b.items() if k != "gather"}


def test_group_table_carries_each_members_gather(check):
    """outs (Cin 64) beside merge_preds (Cin 50) at the five scales: every
    grid slot keeps its own member's gather, and cfg stays the tile index."""
    sizes = (8, 4, 2, 1)
    members = []
    for s in sizes:
        members.append(_geom(n=1, h=s, w=s, cin=64, cout=50, k=1))
        members.append(_geom(n=1, h=s, w=s, cin=50, cout=64, k=1))
    res = check([_plan(g, x=X + 4096 * i, w=W + 4096 * i, push=1)
                 for i, g in enumerate(members)] + ["group"])
    plans, g = res[:-1], res[-1]
    assert [p["gather"] for p in plans] == [1, 0] * len(sizes)
    assert g["n"] == len(members)
    assert g["gather"] == [plans[m]["gather"] for m in g["order"]]
    assert all(0 <= c < 8 for c in g["cfg"])
