"""Oracle and shared cases for the device-side augmentation tests.

``warp_rule`` is a numpy rendering of the rule ``ops/csrc/augment.hip`` is
written to (``scipy.ndimage.affine_transform(order=1, mode="constant")``):

    (sx, sy) = Mi . (ox, oy, 1)
    outside [0, Ws-1] x [0, Hs-1]  -> the constant
    otherwise                      -> bilinear blend of the in-range neighbours

In fp64 it is the oracle; in fp32 it is the yardstick of the tolerance: a GPU
result must lie within 10x the fp32 rendering's own error against the fp64 one
(the convention of test_ensemble_merge_gpu.py).
"""
from __future__ import annotations

import json

import numpy as np

from improved_body_parts_amd.config import CanonicalConfig, COCOSourceConfig
from improved_body_parts_amd.data.transformer import AugmentSelection
from improved_body_parts_amd.ops.augment import inverse_affine

CONFIGS = {128: CanonicalConfig(128, 128, 4), 64: CanonicalConfig(64, 64, 4)}
# (Hs, Ws): smaller and larger than the output, odd sizes, five samples
SOURCE_SIZES = [(97, 141), (50, 77), (200, 150), (33, 35), (128, 128)]
AUGS = {
    "unrandom": (False, 0.0, (0, 0), 1.0),
    "flip": (True, 0.0, (0, 0), 1.0),
    "rot33": (False, 33.0, (7, -5), 1.21),
    "flip_rot-40": (True, -40.0, (-11, 3), 0.7),
    "rot17.5": (False, 17.5, (3, 2), 1.3),
}
INTEGER_CASES = ("unrandom", "flip")
TINT = (np.array([1.1, 0.9, 1.05], np.float32), 0.04)   # gains, shift
BAND = 1e-3          # px
BAND_CAP = 0.005     # share of pixels / cells that may lie in the band
EXACT_ATOL = 1e-6    # integer-matrix cases, [0, 1] units


def make_aug(name, tint=False):
    flip, degree, crop, scale = AUGS[name]
    return AugmentSelection(flip, degree, crop, scale, tint)


def make_records(cfg, mask_dtype=np.uint8, seed=11):
    """Five raw records ``(img, mask_miss, mask_all, meta)`` of different sizes:
    white-noise images, step-edge masks, centre (Ws/2 + 3, Hs/2 - 2) and
    ``scale_provided = target_dist`` (so the base scale is exactly 1)."""
    rng = np.random.default_rng(seed)
    hi = 255 if mask_dtype == np.uint8 else 1
    records = []
    for n, (hs, ws) in enumerate(SOURCE_SIZES):
        img = rng.integers(0, 256, (hs, ws, 3), dtype=np.uint8)
        mask_miss = np.full((hs, ws), hi, mask_dtype)
        mask_miss[hs // 4:hs // 2, ws // 3:ws // 3 + ws // 4] = 0
        mask_all = np.zeros((hs, ws), mask_dtype)
        mask_all[hs // 3:hs - hs // 5, ws // 5:ws // 2 + 3] = hi
        people = 1 + n % 3
        joints = np.zeros((people, cfg.num_parts, 3), np.float32)
        joints[:, :, 0] = rng.uniform(0.2 * ws, 0.8 * ws, joints.shape[:2])
        joints[:, :, 1] = rng.uniform(0.2 * hs, 0.8 * hs, joints.shape[:2])
        joints[:, :, 2] = rng.integers(0, 3, joints.shape[:2])
        meta = {"objpos": [ws / 2 + 3, hs / 2 - 2],
                "scale_provided": cfg.transform_params.target_dist,
                "joints": joints}
        records.append((img, mask_miss, mask_all, meta))
    return records


def forward_matrix(record, aug, cfg):
    meta = record[3]
    center = np.asarray(meta["objpos"], dtype=np.float32).reshape(2)
    return aug.affine(center, meta.get("scale_provided", 1.0), cfg)


def source_coords(Mi, out_hw, dtype=np.float64):
    """Source coordinate of every output pixel, evaluated in ``dtype``."""
    H, W = out_hw
    Mi = np.asarray(Mi).astype(dtype)
    oy, ox = np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype),
                         indexing="ij")
    sx = (Mi[0, 0] * ox + Mi[0, 1] * oy) + Mi[0, 2]
    sy = (Mi[1, 0] * ox + Mi[1, 1] * oy) + Mi[1, 2]
    return sx, sy


def warp_rule(src, Mi, out_hw, cval, dtype=np.float64):
    """The warp rule on a (Hs, Ws) or (Hs, Ws, C) source, computed in ``dtype``."""
    src = np.asarray(src).astype(dtype)
    hs, ws = src.shape[:2]
    sx, sy = source_coords(Mi, out_hw, dtype)
    inside = (sx >= 0) & (sx <= ws - 1) & (sy >= 0) & (sy <= hs - 1)
    flx, fly = np.floor(sx), np.floor(sy)
    x0 = np.clip(flx.astype(np.int64), 0, ws - 1)
    y0 = np.clip(fly.astype(np.int64), 0, hs - 1)
    x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
    fx, fy = (sx - flx).astype(dtype), (sy - fly).astype(dtype)
    if src.ndim == 3:
        fx, fy, ins = fx[..., None], fy[..., None], inside[..., None]
    else:
        ins = inside
    one = dtype(1)
    top = (one - fx) * src[y0, x0] + fx * src[y0, x1]
    bot = (one - fx) * src[y1, x0] + fx * src[y1, x1]
    out = (one - fy) * top + fy * bot
    return np.where(ins, out, dtype(cval)).astype(dtype)


def band_mask(Mi, src_hw, out_hw, eps=BAND):
    """Output pixels whose fp64 source coordinate lies within ``eps`` of the
    source border rectangle without lying exactly on it."""
    hs, ws = src_hw
    sx, sy = source_coords(Mi, out_hw, np.float64)
    dx = np.minimum(np.abs(sx), np.abs(sx - (ws - 1)))
    dy = np.minimum(np.abs(sy), np.abs(sy - (hs - 1)))
    x_span = (sx >= -eps) & (sx <= ws - 1 + eps)
    y_span = (sy >= -eps) & (sy <= hs - 1 + eps)
    near = ((dx < eps) & y_span) | ((dy < eps) & x_span)
    on_x = ((sx == 0) | (sx == ws - 1)) & (sy >= 0) & (sy <= hs - 1)
    on_y = ((sy == 0) | (sy == hs - 1)) & (sx >= 0) & (sx <= ws - 1)
    return near & ~(on_x | on_y)


def pool(m, s):
    h, w = m.shape
    return m[:h - h % s, :w - w % s].reshape(h // s, s, w // s, s).mean(axis=(1, 3))


def cell_band(band, s):
    """Stride cells with any sample in the band."""
    return pool(band.astype(np.float64), s) > 0


def to_float01(m, dtype):
    """``Transformer._to_float01`` in ``dtype`` (the float32 division first)."""
    m = np.asarray(m, dtype=np.float32)
    if m.max() > 1.5:
        m = m / 255.0
    return m.astype(dtype)


def render(record, M, cfg, tint=None, dtype=np.float64):
    """(image [0,1] (H,W,3), mask_miss (h,w), mask_all (h,w)) by the rule."""
    img, mask_miss, mask_all, _ = record
    out_hw = (cfg.height, cfg.width)
    Mi = inverse_affine(M)
    im = warp_rule(img, Mi, out_hw, 128.0, dtype) / dtype(255)
    if tint is not None:
        gains, shift = tint
        im = np.clip(im * np.asarray(gains).astype(dtype) + dtype(shift),
                     dtype(0), dtype(1))
    mm = pool(warp_rule(to_float01(mask_miss, dtype), Mi, out_hw, 1.0, dtype),
              cfg.stride)
    ma = pool(warp_rule(to_float01(mask_all, dtype), Mi, out_hw, 0.0, dtype),
              cfg.stride)
    return im, mm, ma


class Expected:
    """fp64 oracle, band masks and the fp32-derived tolerances of one
    (record, matrix, tint) case."""

    def __init__(self, record, M, cfg, tint=None, exact=False):
        src_hw = record[0].shape[:2]
        self.img, self.miss, self.all = render(record, M, cfg, tint, np.float64)
        i32, m32, a32 = render(record, M, cfg, tint, np.float32)
        if exact:
            self.band = np.zeros((cfg.height, cfg.width), bool)
            self.cells = np.zeros(self.miss.shape, bool)
            self.img_tol = self.mask_tol = EXACT_ATOL
        else:
            self.band = band_mask(inverse_affine(M), src_hw,
                                  (cfg.height, cfg.width))
            self.cells = cell_band(self.band, cfg.stride)
            keep, ckeep = ~self.band, ~self.cells
            self.img_tol = 10.0 * float(np.abs(i32 - self.img)[keep].max())
            self.mask_tol = 10.0 * max(
                float(np.abs(m32 - self.miss)[ckeep].max()),
                float(np.abs(a32 - self.all)[ckeep].max()))

    def check_image(self, got, label, bf16=False, want=None):
        """``want``: another rendering of the same case (the host pipeline's)
        to compare with in place of the fp64 oracle."""
        want = self.img if want is None else np.asarray(want, dtype=np.float64)
        got = np.asarray(got, dtype=np.float64)
        err = np.abs(got - want)
        allow = self.img_tol + (2.0 ** -8 * np.abs(want) if bf16 else 0.0)
        keep = ~self.band
        worst = float((err - allow)[keep].max())
        print(f"{label}: image err {float(err[keep].max()):.3e} "
              f"tol {self.img_tol:.3e} band {self.band.mean():.5f}")
        assert self.band.mean() <= BAND_CAP
        assert worst <= 0.0, f"{label}: image off by {worst:.3e} beyond tol"

    def check_masks(self, miss, all_, label, want=None):
        keep = ~self.cells
        assert self.cells.mean() <= BAND_CAP
        want_miss, want_all = (self.miss, self.all) if want is None else want
        for name, got, want in (("mask_miss", miss, want_miss),
                                ("mask_all", all_, want_all)):
            want = np.asarray(want, dtype=np.float64)
            err = np.abs(np.asarray(got, dtype=np.float64) - want)[keep].max()
            print(f"{label}: {name} err {float(err):.3e} tol {self.mask_tol:.3e}")
            assert err <= self.mask_tol, f"{label}: {name} off by {err:.3e}"


# ---------------------------------------------------------------------------
# in-memory h5-layout fixture (own copy of the mapping the COCO reader expects)
# ---------------------------------------------------------------------------
class FakeDS:
    def __init__(self, v):
        self.v = v

    def __getitem__(self, idx):
        assert idx == ()
        return self.v


class FakeH5(dict):
    def get(self, k, default=None):
        return super().get(k, default)


def coco_fixture(cfg, n=4, seed=5):
    """``n`` records of different sizes in the reference's h5 layout: 2-person
    COCO-order annotations, a mask_miss hole, a mask_all box."""
    rng = np.random.default_rng(seed)
    dataset, images, masks = {}, {}, {}
    for k in range(n):
        H, W = 160 + 24 * k, 200 - 16 * k
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        people = []
        for pi in range(2):
            joints = np.zeros((17, 3), np.float32)
            cx, cy = 40 + 60 * pi, 50 + 20 * pi
            for j in range(17):
                joints[j] = (cx + (j % 4) * 9, cy + (j // 4) * 11, 1.0)
            people.append(joints.tolist())
        mask_miss = np.ones((H, W), np.float32)
        mask_miss[60:90, 30:80] = 0.0
        mask_all = np.zeros((H, W), np.float32)
        mask_all[30:120, 20:150] = 1.0
        name = f"img{k}.jpg"
        meta = {"image": name, "objpos": [70.0 + k, 80.0 - k],
                "scale_provided": 60.0 / cfg.height, "joints": people}
        dataset[str(k)] = FakeDS(json.dumps(meta))
        images[name] = FakeDS(img)
        masks[name] = FakeDS(np.stack([mask_miss, mask_all]))
    h5 = FakeH5({"dataset": dataset, "images": images, "masks": masks})
    return h5, COCOSourceConfig("unused.h5")
