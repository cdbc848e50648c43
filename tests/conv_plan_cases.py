"""Conv problems of the grouped-launch and upsample-fold tests and the plans
``(BM, BN, splitk, deep)`` the host planner must give them.

Shared by ``test_conv_grouped_gpu.py`` and ``test_upconv_fold_gpu.py`` (which
ask the extension's plan bindings) and ``test_conv_plan_cpu.py`` (which asks
the planner compiled for the CPU): the groups only test what their names say
while the planner keeps putting their members on these tiles and splits.
"""

FULL = ("scale", "act", "res", "post", "post2")

# ---------------------------------------------------------------------------
# grouped launch: (size, cin, cout, k, epilogue), N = 1, stride 1, same padding
# ---------------------------------------------------------------------------
G3 = [(96, 64, 64, 3, FULL), (48, 128, 128, 3, ()),
      (24, 192, 50, 3, ("scale", "act")), (12, 64, 72, 3, ("scale", "post")),
      (6, 128, 64, 3, FULL)]
# 1x1 (DEEP); Cin = 64 is a single K-chunk: unsplit members beside split
# ones, on the 16-byte-store lane exchange (Cout 64 and 72) and the pair path
G1 = [(96, 64, 64, 1, FULL), (48, 128, 128, 1, ("scale", "post")),
      (24, 64, 72, 1, ("scale", "act")), (12, 192, 50, 1, FULL),
      (6, 64, 50, 1, ())]
# long K (Cin 192/384) and wide Cout: few enough splits that a block keeps
# more than 6 K-chunks, i.e. the non-DEEP bodies of all four tiles, plus the
# 128x128 and 128x64 DEEP ones
GL = [(96, 192, 256, 3, FULL), (96, 192, 192, 3, ("scale", "act")),
      (48, 192, 256, 3, ()), (24, 384, 256, 3, ("scale", "post")),
      (6, 384, 64, 3, FULL), (96, 128, 256, 1, ("scale", "post2")),
      (96, 128, 192, 1, FULL)]
GROUPS = {
    "3x3-mixed": G3,
    "1x1-mixed": G1,
    "long-k-non-deep": GL,
    "group-of-1": G3[:1],
    "group-of-2-unsplit": [G1[0], G1[2]],
    "group-of-8": G3 + G1[:3],
    "list-of-9": G1 + G3[:4],
}

# (size, cin, cout, k, full epilogue); 226^2 = 399 * 128 + 4 rows fills the
# chip without split-K: 9 K-chunks per block, the non-DEEP body
EXACT_SPECS = [(226, 64, 64, 3, True), (48, 64, 128, 1, False),
               (24, 64, 50, 3, True), (12, 64, 72, 1, True),
               (6, 64, 64, 3, False)]

# BM of the members of G3 and of G1
G3_BM = [128, 64, 32, 32, 32]
G1_BM = [128, 64, 32, 32, 32]
# (BM, BN, deep) of the members of GL
GL_TILE_DEEP = [(128, 128, 0), (128, 64, 0), (64, 64, 0), (32, 64, 0),
                (32, 64, 1), (128, 128, 1), (128, 64, 1)]
# every tile configuration of the grouped kernel's switch, exercised by
# G3 + G1 + GL together
TILE_CONFIGS = {(bm, bn, d) for bm, bn in
                [(128, 128), (128, 64), (64, 64), (32, 64)] for d in (0, 1)}
# the exact-integer group: one unsplit non-DEEP member, split and unsplit
# DEEP ones
EXACT_PLANS = [(128, 64, 1, 0), (64, 64, 1, 1), (32, 64, 9, 1),
               (32, 64, 1, 1), (32, 64, 9, 1)]

# ---------------------------------------------------------------------------
# upsample fold
# ---------------------------------------------------------------------------
# (name, N, Cin, Cout, low H, low W, residual offset in bytes, IBP_SPLITK_TARGET,
#  full epilogue)
INT_CASES = [
    # odd sizes, borders dominate, M_low < one tile; split 4 over 4 K-chunks:
    # 16-byte slab stores past a half-empty column tile, vector combine
    ("5x7-split", 1, 64, 40, 5, 7, 0, None, True),
    # the same problem unsplit (the planner's documented override): the
    # vec_epi = 2 lane exchange with a half-empty 16-byte store pair
    ("5x7-unsplit", 1, 64, 40, 5, 7, 0, "1", True),
    # 32-row tile, split-K with scatter in slabs and vector combine
    ("8x8-split", 2, 64, 64, 8, 8, 0, None, True),
    # non-square, 64-row tile, Cout tail, split, vector combine
    ("16x24-cout72", 2, 128, 72, 16, 24, 0, None, True),
    # 128x128 tile, unsplit vec_epi = 2 lane exchange with scatter; N = 12
    # is the smallest batch at which 4 x 96 tiles fill the chip unsplit
    ("32x32-unsplit", 12, 64, 128, 32, 32, 0, None, True),
    # residuals 8-byte but not 16-byte aligned: the scalar combine body
    ("8x8-res-off8", 2, 64, 64, 8, 8, 8, None, True),
    # no activation, no residuals, no scale/shift
    ("8x8-plain", 2, 64, 64, 8, 8, 0, None, False),
    # Cout % 8 != 0 (outside the model's gate, inside the op's): the 8-byte
    # vec_epi = 1 stores, the 4-byte pair stores and the per-element path,
    # split (slab stores of each width, scalar combine) and unsplit
    ("5x7-cout36-split", 1, 64, 36, 5, 7, 0, None, True),
    ("5x7-cout36-unsplit", 1, 64, 36, 5, 7, 0, "1", True),
    ("5x7-cout34-split", 1, 64, 34, 5, 7, 0, None, True),
    ("5x7-cout34-unsplit", 1, 64, 34, 5, 7, 0, "1", True),
    ("5x7-cout33-unsplit", 1, 64, 33, 5, 7, 0, "1", True),
]

# ((N, Cin, Cout, low H, low W), plan). The workload's four refine convs,
# batch 4: one plan for all parities, from M = 4 * M_low rows and 4 * ntiles
# tiles; then the precision shape: 2 x 256 -> 256 at 16 x 16, non-DEEP split
UPFOLD_SHAPE_PLANS = [
    ((4, 256, 256, 64, 64), (128, 128, 1, 0)),
    ((4, 384, 384, 32, 32), (128, 128, 1, 0)),
    ((4, 512, 512, 16, 16), (64, 64, 1, 0)),
    ((4, 640, 640, 8, 8), (32, 64, 2, 0)),
    ((2, 256, 256, 16, 16), (32, 64, 2, 0)),
]
# INT_CASES name -> plan, IBP_SPLITK_TARGET unset
UPFOLD_CASE_PLANS = {
    "5x7-split": (32, 64, 4, 1),
    "8x8-split": (32, 64, 4, 1),
    "16x24-cout72": (64, 64, 4, 1),
    "32x32-unsplit": (128, 128, 1, 1),
    "8x8-res-off8": (32, 64, 4, 1),
}
# one image fewer than "32x32-unsplit" splits
UPFOLD_SPLITS_BELOW_12 = (11, 64, 128, 32, 32)
# INT_CASES name -> plan with IBP_SPLITK_TARGET=1
UPFOLD_CASE_PLANS_TARGET_1 = {
    "5x7-unsplit": (32, 64, 1, 1),
    "5x7-cout33-unsplit": (32, 64, 1, 1),
}
