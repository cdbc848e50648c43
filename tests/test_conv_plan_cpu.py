"""The MFMA conv's host planner (ops/csrc/conv_plan.h) on the CPU.

``tests/csrc/conv_plan_check.cpp`` is compiled once with the host compiler
under AddressSanitizer and UBSan and driven as a child process: commands on
stdin, one JSON object per command on stdout. Pointers are made-up integers;
the planner only compares and offsets them.

* plans: every ``(BM, BN, splitk, deep)`` the GPU tests assert through the
  extension's bindings (``conv_plan_cases.py``);
* split-K: no slice without work over 2.4 M ``(ntiles, nk_total, target)``;
* epilogue paths from pointer alignment, against a table written by hand from
  the rule above ``p.vec_epi`` in ``plan_conv``;
* group assembly for the member lists of the grouped-launch test;
* the 32-bit guards and the ``IBP_CONV_BM`` check.
"""
import json
import os
import shutil
import subprocess

import pytest

import conv_plan_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "improved_body_parts_amd", "ops", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all"]
K_MAX_GROUP = 8


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """run(lines, **env) -> list of dicts, one per command."""
    cxx = shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler (c++) on this machine")
    exe = str(tmp_path_factory.mktemp("conv_plan") / "conv_plan_check")
    cmd = [cxx, *FLAGS, "-I", CSRC,
           os.path.join(ROOT, "tests", "csrc", "conv_plan_check.cpp"),
           "-o", exe]
    # sanitizer runtimes inside the program where the toolchain has them as
    # archives, so the program does not depend on what else gets loaded
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"],
                      capture_output=True).returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
        assert built.returncode == 0, built.stderr[-4000:]

    def run(lines, **env):
        child_env = {k: v for k, v in os.environ.items()
                     if k not in ("IBP_CONV_BM", "IBP_SPLITK_TARGET")}
        child_env.update(env)
        out = subprocess.run([exe], input="\n".join(lines) + "\n", text=True,
                             capture_output=True, env=child_env, timeout=120)
        assert out.returncode == 0, out.stderr[-4000:]
        assert not out.stderr, out.stderr[-4000:]
        res = [json.loads(l) for l in out.stdout.splitlines()]
        assert len(res) == len(lines)
        return res

    return run


def _tuple(r):
    return (r["BM"], r["BN"], r["splitk"], r["deep"])


# ---------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------

def test_grouped_members_land_on_their_plans(check):
    def plans(specs):
        return [_tuple(r) for r in check(
            [f"tile {s[0] * s[0]} {s[2]} {s[3] * s[3] * s[1]}"
             for s in specs])]

    g3, g1, gl = plans(C.G3), plans(C.G1), plans(C.GL)
    assert [p[0] for p in g3] == C.G3_BM
    assert [p[0] for p in g1] == C.G1_BM
    assert all(p[2] > 1 for p in g3)
    assert [p[2] == 1 for p in g1] == [m[1] == 64 for m in C.G1]
    assert all(p[3] == 1 for p in g1)
    assert [p[:2] + p[3:] for p in gl] == C.GL_TILE_DEEP
    assert {p[:2] + p[3:] for p in g3 + g1 + gl} == C.TILE_CONFIGS
    assert plans(C.EXACT_SPECS) == C.EXACT_PLANS


def test_upfold_shapes_land_on_their_plans(check):
    by_name = {c[0]: c for c in C.INT_CASES}

    def cmd(n, cin, cout, h, w):
        return f"uptile {n * h * w} {cout} {cin}"

    def of(name):
        _, n, cin, cout, h, w, *_ = by_name[name]
        return cmd(n, cin, cout, h, w)

    shapes = [s for s, _ in C.UPFOLD_SHAPE_PLANS]
    names = list(C.UPFOLD_CASE_PLANS)
    res = check([cmd(*s) for s in shapes] + [of(n) for n in names]
                + [cmd(*C.UPFOLD_SPLITS_BELOW_12)])
    got = [_tuple(r) for r in res]
    assert got[:len(shapes)] == [p for _, p in C.UPFOLD_SHAPE_PLANS]
    assert got[len(shapes):-1] == [C.UPFOLD_CASE_PLANS[n] for n in names]
    assert got[-1][2] > 1
    names = list(C.UPFOLD_CASE_PLANS_TARGET_1)
    res = check([of(n) for n in names], IBP_SPLITK_TARGET="1")
    assert [_tuple(r) for r in res] == \
        [C.UPFOLD_CASE_PLANS_TARGET_1[n] for n in names]


# ---------------------------------------------------------------------------
# split-K: every slice has work
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("target", [1, 7, 64, 384, 1000])
def test_no_split_slice_without_work(check, target):
    """1 <= splitk <= nk_total and (splitk-1)*ceil(nk_total/splitk) < nk_total
    for ntiles 1..1200, nk_total 1..400: a slice without K-chunks returns
    early and the combine then sums its uninitialised workspace slab."""
    (r,) = check(["sweep 1200 400"], IBP_SPLITK_TARGET=str(target))
    assert r["cases"] == 1200 * 400
    assert r["bad"] == 0, f"first (ntiles, nk_total, splitk) {r['first_bad']}"


# ---------------------------------------------------------------------------
# one conv: command line and epilogue paths
# ---------------------------------------------------------------------------

PTRS = ("x", "w", "y", "scale", "shift", "res", "res_post", "res_post2")
A = 1 << 24          # made-up addresses, 256-byte aligned, far apart


def _conv(geom, ptrs, act=1, up=0, py=0, px=0, ws=0, push=0):
    assert len(geom) == 15
    return "conv " + " ".join(str(v) for v in (
        *geom, *(ptrs.get(k, 0) for k in PTRS), act, up, py, px, ws, push))


def _geom(n, h, w, cin, cout, k, pad=None):
    """stride-1 conv with 'same' padding."""
    pad = (k - 1) // 2 if pad is None else pad
    return [n, h, w, cin, cout, k, k, 1, pad, pad, 1, 1, h, w, 1]


# Expected "vec_epi pair_epi vec_combine", by hand from the rule in plan_conv:
#   vec_epi  = Cout % 4 == 0 and (split or: scale, shift 16-byte aligned and
#              res, res_post, res_post2, y 8-byte aligned); 2 instead of 1
#              when also Cout % 8 == 0 and y is 16-byte aligned
#   pair_epi = Cout % 2 == 0 and res, res_post, res_post2, y 4-byte aligned
#   vec_combine = Cout % 8 == 0 and all six and the workspace 16-byte aligned
# Rows: the one pointer that is moved; columns: moved by 2, 4, 8, 16 bytes.
# "ws+8" is the workspace moved by 8 bytes (it exists only when split).
EPI_TABLE = {
    # Cout 64 and 72: Cout % 8 == 0
    ("cout%8", "unsplit"): {
        "none": "211",
        "scale": "010 010 010 211",
        "shift": "010 010 010 211",
        "res": "000 010 210 211",
        "res_post": "000 010 210 211",
        "res_post2": "000 010 210 211",
        "y": "000 010 110 211",
        "ws+8": "211",
    },
    ("cout%8", "split"): {
        "none": "211",
        "scale": "210 210 210 211",
        "shift": "210 210 210 211",
        "res": "200 210 210 211",
        "res_post": "200 210 210 211",
        "res_post2": "200 210 210 211",
        "y": "100 110 110 211",
        "ws+8": "210",
    },
    # Cout 50: only Cout % 2 == 0, split or not
    ("cout%2", "unsplit"): {
        "none": "010",
        "scale": "010 010 010 010",
        "shift": "010 010 010 010",
        "res": "000 010 010 010",
        "res_post": "000 010 010 010",
        "res_post2": "000 010 010 010",
        "y": "000 010 010 010",
        "ws+8": "010",
    },
    # Cout 33: per-element everywhere
    ("odd", "unsplit"): {
        "none": "000",
        "scale": "000 000 000 000",
        "shift": "000 000 000 000",
        "res": "000 000 000 000",
        "res_post": "000 000 000 000",
        "res_post2": "000 000 000 000",
        "y": "000 000 000 000",
        "ws+8": "000",
    },
}
EPI_TABLE[("cout%2", "split")] = EPI_TABLE[("cout%2", "unsplit")]
EPI_TABLE[("odd", "split")] = EPI_TABLE[("odd", "unsplit")]
COUT_CLASS = {64: "cout%8", 72: "cout%8", 50: "cout%2", 33: "odd"}
MOVED = ("scale", "shift", "res", "res_post", "res_post2", "y")


@pytest.mark.parametrize("cout", [64, 72, 50, 33])
@pytest.mark.parametrize("split", ["unsplit", "split"])
def test_epilogue_path_from_pointer_alignment(check, cout, split):
    # 1x1 over 8x8: one M-tile row; Cin 128 is two K-chunks (split 2), Cin 64
    # a single one (unsplit)
    geom = _geom(1, 8, 8, 128 if split == "split" else 64, cout, 1)
    base = {k: A * (i + 1) for i, k in enumerate(PTRS)}
    ws = A * 16
    table = EPI_TABLE[(COUT_CLASS[cout], split)]
    cases = [("none", 0, _conv(geom, base, ws=ws), table["none"]),
             ("ws+8", 8, _conv(geom, base, ws=ws + 8), table["ws+8"])]
    for name in MOVED:
        for off, want in zip((2, 4, 8, 16), table[name].split()):
            cases.append((name, off,
                          _conv(geom, {**base, name: base[name] + off}, ws=ws),
                          want))
    assert len(cases) == 2 + 6 * 4
    for (name, off, _, want), r in zip(cases, check([c[2] for c in cases])):
        assert (r["splitk"] > 1) == (split == "split")
        got = f"{r['vec_epi']}{r['pair_epi']}{r['vec_combine']}"
        assert got == want, f"Cout {cout} {split}: {name} moved by {off}"


# ---------------------------------------------------------------------------
# group assembly
# ---------------------------------------------------------------------------

def _tile_cfg(bm, bn, deep):
    return {(128, 128): 0, (128, 64): 2, (64, 64): 4, (32, 64): 6}[bm, bn] \
        + deep


def _member_cmd(i, spec):
    size, cin, cout, k, epi = spec
    ptrs = {"x": A * (16 * i + 1), "w": A * (16 * i + 2),
            "y": A * (16 * i + 3)}
    if "scale" in epi:
        ptrs.update(scale=A * (16 * i + 4), shift=A * (16 * i + 5))
    for j, key in enumerate(("res", "post", "post2")):
        if key in epi:
            ptrs[PTRS[5 + j]] = A * (16 * i + 6 + j)
    return _conv(_geom(1, size, size, cin, cout, k), ptrs,
                 act=int("act" in epi), push=1), ptrs["y"]


def _combine_blocks(total, vec):
    work = total // 8 if vec else total
    return min(max((work + 255) // 256, 1), 4096)


@pytest.mark.parametrize("name", list(C.GROUPS))
def test_group_assembly(check, name):
    specs = C.GROUPS[name]
    chunks = [(f, min(f + K_MAX_GROUP, len(specs)))
              for f in range(0, len(specs), K_MAX_GROUP)]
    if name == "list-of-9":
        assert chunks == [(0, 8), (8, 9)]
    ws_base = A * 4096 + 64       # 16-byte aligned, not more
    cmds, ys = zip(*[_member_cmd(i, s) for i, s in enumerate(specs)])
    res = check(list(cmds) + [f"group {f} {l} {ws_base}" for f, l in chunks])
    plans, groups = res[:len(specs)], res[len(specs):]
    for (first, last), g in zip(chunks, groups):
        mem = plans[first:last]
        my = ys[first:last]
        n = last - first
        assert g["n"] == n and g["up"] == 0
        # stable, most K-chunks per block first
        order = sorted(range(n), key=lambda i: -mem[i]["nk_block"])
        assert g["order"] == order
        # block prefix sums in grid order; the last one is the grid size
        run, ends = 0, []
        for i in order:
            run += mem[i]["nblocks"]
            ends.append(run)
        assert g["block_end"][:n] == ends and g["blocks"] == ends[-1]
        assert [g["y"][i] for i in range(n)] == [my[i] for i in order]
        for i, m in enumerate(order):
            assert g["cfg"][i] == mem[m]["cfg"] == _tile_cfg(
                mem[m]["BM"], mem[m]["BN"], mem[m]["deep"])
            assert g["splitk"][i] == mem[m]["splitk"]
        # entries past n repeat the last member
        for i in range(n, K_MAX_GROUP):
            assert g["block_end"][i] == ends[-1]
            assert g["cfg"][i] == g["cfg"][n - 1]
            assert g["y"][i] == g["y"][n - 1] and g["ws"][i] == g["ws"][n - 1]
        # workspace: known before the pointer, 16-byte aligned, disjoint,
        # each slice long enough for splitk slabs of M x Cout floats
        off = g["ws_off"] + [g["ws_total"]]
        for i in range(n):
            need = mem[i]["splitk"] * mem[i]["M"] * specs[first + i][2] \
                if mem[i]["splitk"] > 1 else 0
            assert mem[i]["ws_elems"] == need
            assert off[i] % 4 == 0 and off[i + 1] - off[i] >= need
            assert off[i + 1] - off[i] < need + 4
        for i, m in enumerate(order):
            assert g["ws"][i] == (ws_base + 4 * off[m]
                                  if mem[m]["splitk"] > 1 else 0)
        # combine table: exactly the split members, in grid order
        split = [m for m in order if mem[m]["splitk"] > 1]
        assert g["cn"] == len(split)
        run, cends = 0, []
        for j, m in enumerate(split):
            total = mem[m]["M"] * specs[first + m][2]
            assert g["c_y"][j] == my[m]
            assert g["c_ws"][j] == ws_base + 4 * off[m]
            assert g["c_total"][j] == total
            assert g["c_splitk"][j] == mem[m]["splitk"]
            assert g["c_up"][j] == 0
            # every pointer here is 16-byte aligned: vector combine exactly
            # where Cout % 8 == 0
            assert g["c_vec"][j] == mem[m]["vec_combine"] \
                == int(specs[first + m][2] % 8 == 0)
            run += _combine_blocks(total, g["c_vec"][j])
            cends.append(run)
        assert g["c_block_end"][:len(split)] == cends
        assert g["cblocks"] == (cends[-1] if cends else 0)
        for j in range(len(split), K_MAX_GROUP):
            assert g["c_block_end"][j] == g["cblocks"]
            assert g["c_y"][j] == (g["c_y"][len(split) - 1] if split else 0)


def test_group_of_upfold_parities_and_mixed_members(check):
    # 2 x 64 -> 64 at 8 x 8 low resolution ("8x8-split"): four parity 2x2 convs
    n, cin, cout, h, w = 2, 64, 64, 8, 8
    y = A * 3
    par = [_conv([n, h, w, cin, cout, 2, 2, 1, 1 - py, 1 - px, 1, 1, h, w, 1],
                 {"x": A, "w": A * 2 + (py * 2 + px) * cout * 4 * cin * 2,
                  "y": y}, up=1, py=py, px=px, push=1)
           for py in (0, 1) for px in (0, 1)]
    plain = _member_cmd(5, C.G3[0])[0]
    res = check(par + ["group 0 4 4096", plain, "group 0 5 4096",
                       "group 4 5 4096", "group 3 5 4096"])
    for r, (py, px) in zip(res[:4], [(0, 0), (0, 1), (1, 0), (1, 1)]):
        assert _tuple(r) == C.UPFOLD_CASE_PLANS["8x8-split"]
        assert (r["up"], r["py"], r["px"]) == (1, py, px)
        assert r["M"] == n * h * w and r["K"] == 4 * cin
    g = res[4]
    assert g["up"] == 1 and g["n"] == 4 and g["order"] == [0, 1, 2, 3]
    assert g["y"] == [y] * 8 and g["cn"] == 4 and g["c_up"] == [1] * 8
    assert g["block_end"][:4] == [res[0]["nblocks"] * (i + 1)
                                  for i in range(4)]
    assert "cannot mix" in res[6]["error"]
    assert res[7]["up"] == 0 and res[7]["n"] == 1
    assert "cannot mix" in res[8]["error"]


# ---------------------------------------------------------------------------
# guards
# ---------------------------------------------------------------------------

def test_m32_flips_where_rows_plus_tile_reach_2_31(check):
    def one_row(m):   # M = 1 * 1 * m rows, BM = 128
        return _conv([1, 1, m, 64, 64, 1, 1, 1, 0, 0, 1, 1, 1, m, 1],
                     {"x": A, "w": 2 * A, "y": 3 * A})
    lo, hi = check([one_row(2**31 - 129), one_row(2**31 - 128)])
    assert lo["BM"] == hi["BM"] == 128
    assert lo["M"] + 128 == 2**31 - 1 and lo["m32"] == 1
    assert hi["M"] + 128 == 2**31 and hi["m32"] == 0


def test_upfold_rejects_outputs_past_32_bit_rows(check):
    def parity(m_low):
        return _conv([1, 1, m_low, 64, 64, 2, 2, 1, 1, 1, 1, 1, 1, m_low, 1],
                     {"x": A, "w": 2 * A, "y": 3 * A}, up=1)
    ok, bad = check([parity(2**29 - 129), parity(2**29 - 128)])
    assert ok["BM"] == 128 and ok["up"] == 1 and ok["m32"] == 1
    assert 4 * ok["M"] + 4 * 128 == 2**31 - 4
    assert "32-bit row math" in bad["error"]


def test_conv_bm_override_is_validated(check):
    (r,) = check(["tile 9216 64 576"], IBP_CONV_BM="64")
    assert r["BM"] == 64 and r["n_mtiles"] == 144
    for bad in ("48", "256", "0", "big"):
        (r,) = check(["tile 9216 64 576"], IBP_CONV_BM=bad)
        assert "IBP_CONV_BM" in r["error"], bad
