"""Device-side augmentation, the parts that need no GPU: the warp rule the
kernel is written to, the batch packer, the CPU path of the op (the oracle by
construction), the loader's epoch logic and the border band of the GPU cases."""
import random

import numpy as np
import pytest
import torch

import augment_oracle as O
from improved_body_parts_amd.data import (DeviceAugmentLoader, DeviceTransformer,
                                          MyDataset, Transformer)
from improved_body_parts_amd.ops.augment import (DESC_DTYPE, FLAG_MASK_F32,
                                                 FLAG_TINT, augment_batch,
                                                 inverse_affine, pack_batch)

CASES = [(size, name) for size in O.CONFIGS for name in O.AUGS]


@pytest.mark.parametrize("size,name", CASES)
def test_warp_rule_equals_transformer_warp(size, name):
    """The fp64 rule equals scipy's order-1 constant-mode warp within 1e-5 of a
    0-255 unit on every pixel of every GPU case."""
    cfg = O.CONFIGS[size]
    aug = O.make_aug(name)
    worst = 0.0
    for rec in O.make_records(cfg):
        M = O.forward_matrix(rec, aug, cfg)
        want = Transformer._warp(rec[0], M, (cfg.height, cfg.width), order=1,
                                 cval=128.0)
        got = O.warp_rule(rec[0], inverse_affine(M), (cfg.height, cfg.width), 128.0)
        worst = max(worst, float(np.abs(got - want).max()))
        mask = O.to_float01(rec[1], np.float32)
        want_m = Transformer._warp(mask, M, (cfg.height, cfg.width), order=1,
                                   cval=1.0)
        got_m = O.warp_rule(mask, inverse_affine(M), (cfg.height, cfg.width), 1.0)
        assert np.abs(got_m - want_m).max() <= 1e-5 / 255 + 1e-7
    print(f"{size} {name}: rule vs scipy {worst:.3e} of a 0-255 unit")
    assert worst <= 1e-5


@pytest.mark.parametrize("size,name", CASES)
def test_border_band_is_thin(size, name):
    """At most 0.5 % of the pixels (and of the mask cells) of a GPU case may sit
    within 1e-3 px of the source border without lying exactly on it."""
    cfg = O.CONFIGS[size]
    aug = O.make_aug(name)
    for rec in O.make_records(cfg):
        Mi = inverse_affine(O.forward_matrix(rec, aug, cfg))
        band = O.band_mask(Mi, rec[0].shape[:2], (cfg.height, cfg.width))
        cells = O.cell_band(band, cfg.stride)
        print(f"{size} {name} {rec[0].shape[:2]}: band {band.mean():.5f} "
              f"cells {cells.mean():.5f}")
        assert band.mean() <= O.BAND_CAP
        assert cells.mean() <= O.BAND_CAP


def test_packer_round_trip():
    cfg = O.CONFIGS[128]
    rec_u8 = O.make_records(cfg, np.uint8)
    rec_f32 = O.make_records(cfg, np.float32)
    # mixed batch: uint8 and float32 mask pairs, tinted and plain samples
    recs = [rec_u8[0], rec_f32[1], rec_u8[2], rec_f32[3], rec_u8[4]]
    rng = np.random.default_rng(0)
    invs = [rng.normal(size=(2, 3)) for _ in recs]
    tints = [None, O.TINT, None, O.TINT, None]
    packed = pack_batch([r[0] for r in recs],
                        [np.stack([r[1], r[2]]) for r in recs], invs, tints)
    packed.validate()
    assert packed.desc.dtype == DESC_DTYPE and len(packed) == 5
    assert packed.buffer.dtype == torch.uint8 and packed.buffer.dim() == 1

    spans = []
    for d, r, inv, tint in zip(packed.desc, recs, invs, tints):
        hs, ws = r[0].shape[:2]
        assert (d["hs"], d["ws"]) == (hs, ws)
        np.testing.assert_array_equal(d["mi"], inv.astype(np.float32).reshape(6))
        is_f32 = r[1].dtype == np.float32
        assert bool(d["flags"] & FLAG_MASK_F32) == is_f32
        assert bool(d["flags"] & FLAG_TINT) == (tint is not None)
        np.testing.assert_array_equal(
            d["mask_scale"], np.float32([1.0, 1.0] if is_f32 else [1 / 255, 1 / 255]))
        if tint is not None:
            np.testing.assert_array_equal(d["gain"], tint[0])
            assert d["shift"] == np.float32(tint[1])
        assert d["img_off"] % 16 == 0 and d["mask_off"] % 16 == 0
        spans.append((int(d["img_off"]), hs * ws * 3))
        spans.append((int(d["mask_off"]), 2 * hs * ws * (4 if is_f32 else 1)))
    # sources do not overlap, each leaves the kernel's read-ahead free
    spans.sort()
    for (a, n), (b, _) in zip(spans, spans[1:]):
        assert a + n + 8 <= b
    assert spans[-1][0] + spans[-1][1] + 8 <= packed.buffer.numel()

    for (img, pair), r in zip(packed.unpack(), recs):
        np.testing.assert_array_equal(img, r[0])
        assert pair.dtype == r[1].dtype
        np.testing.assert_array_equal(pair[0], r[1])
        np.testing.assert_array_equal(pair[1], r[2])


def test_packer_rejects_bad_input():
    cfg = O.CONFIGS[64]
    img, mm, ma, _ = O.make_records(cfg)[0]
    eye = np.eye(3)[:2]
    pair = np.stack([mm, ma])
    with pytest.raises(ValueError):
        pack_batch([img.astype(np.float32)], [pair], [eye])
    with pytest.raises(ValueError):
        pack_batch([img[..., 0]], [pair], [eye])
    with pytest.raises(ValueError):
        pack_batch([img], [pair[:, :-1]], [eye])
    with pytest.raises(ValueError):
        augment_batch([img.astype(np.float32) / 255], [pair], [eye], None, cfg, "cpu")
    packed = pack_batch([img], [pair], [eye])
    packed.desc["img_off"][0] = packed.buffer.numel() - 16
    with pytest.raises(ValueError):
        packed.validate()


@pytest.mark.parametrize("mask_dtype", [np.uint8, np.float32])
def test_transform_batch_cpu_equals_transformer(mask_dtype):
    """CPU tensors: per-sample ``Transformer.transform``, bit for bit, the tint
    drawn from equal seeds."""
    cfg = O.CONFIGS[64]
    recs = O.make_records(cfg, mask_dtype)
    names = list(O.AUGS)
    augs = [O.make_aug(n, tint=(i % 2 == 0)) for i, n in enumerate(names)]
    dt = DeviceTransformer(cfg, device="cpu")
    img, miss, all_, joints = dt.transform_batch(recs, augs, rng=random.Random(3))
    assert img.shape == (5, 64, 64, 3) and img.dtype == torch.float32
    assert miss.shape == all_.shape == (5, 16, 16)

    rng = random.Random(3)
    tf = Transformer(cfg)
    for i, (rec, aug) in enumerate(zip(recs, augs)):
        wi, wm, wa, meta = tf.transform(*rec, aug=aug, rng=rng)
        np.testing.assert_array_equal(img[i].numpy(), wi)
        np.testing.assert_array_equal(miss[i].numpy(), wm)
        np.testing.assert_array_equal(all_[i].numpy(), wa)
        np.testing.assert_array_equal(joints[i], meta["joints"])

    # random selections come out of the rng in Transformer.transform's order
    img2, _, _, joints2 = dt.transform_batch(recs, None, rng=random.Random(9))
    rng = random.Random(9)
    for i, rec in enumerate(recs):
        wi, _, _, meta = tf.transform(*rec, rng=rng)
        np.testing.assert_array_equal(img2[i].numpy(), wi)
        np.testing.assert_array_equal(joints2[i], meta["joints"])


def _loader(cfg, **kw):
    h5, src = O.coco_fixture(cfg, n=6)
    ds = MyDataset(cfg, src, augment=True, h5_file=h5)
    return ds, DeviceAugmentLoader(ds, device="cpu", dtype=torch.float32, **kw)


def test_raw_is_first_half_of_gen():
    cfg = O.CONFIGS[64]
    h5, src = O.coco_fixture(cfg, n=2)
    ds = MyDataset(cfg, src, augment=False, h5_file=h5)
    img, mm, ma, meta = ds.iterator.raw(1)
    assert img.dtype == np.uint8 and img.shape == (184, 184, 3)
    assert mm.shape == ma.shape == img.shape[:2]
    assert np.asarray(meta["joints"]).shape[1:] == (cfg.num_parts, 3)
    from improved_body_parts_amd.data import AugmentSelection
    wi, wm, wa, wmeta = ds.iterator.transformer.transform(
        img, mm, ma, meta, aug=AugmentSelection.unrandom())
    gi, gm, _ = ds[1]
    np.testing.assert_array_equal(gi.numpy(), wi)
    np.testing.assert_array_equal(gm[0].numpy(), wm)


def test_loader_cpu_shapes_and_epoch_determinism():
    cfg = O.CONFIGS[64]
    ds, loader = _loader(cfg, batch_size=2, seed=4)
    assert len(loader) == 3
    loader.set_epoch(1)
    first = list(loader)
    assert len(first) == 3
    h, w = cfg.mask_shape
    for images, mask_miss, heatmaps in first:
        assert images.shape == (2, cfg.height, cfg.width, 3)
        assert mask_miss.shape == (2, 1, h, w)
        assert heatmaps.shape == (2, cfg.num_layers, h, w)
        assert images.dtype == mask_miss.dtype == heatmaps.dtype == torch.float32
        assert torch.isfinite(heatmaps).all()
        assert 0.0 <= float(images.min()) and float(images.max()) <= 1.0
    again = list(loader)
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    loader.set_epoch(2)
    other = list(loader)
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(first, other))


def test_loader_keeps_a_partial_batch_without_drop_last():
    cfg = O.CONFIGS[64]
    _, loader = _loader(cfg, batch_size=4, drop_last=False, augment=False,
                        shuffle=False)
    sizes = [b[0].shape[0] for b in loader]
    assert len(loader) == 2 and sizes == [4, 2]


def test_loader_ranks_split_the_dataset():
    cfg = O.CONFIGS[64]
    shares = []
    for rank in range(2):
        ds, loader = _loader(cfg, batch_size=1, seed=7, rank=rank, world_size=2)
        loader.set_epoch(3)
        shares.append(set(int(i) for i in loader.epoch_indices()))
        assert len(loader) == 3
    assert shares[0].isdisjoint(shares[1])
    assert shares[0] | shares[1] == set(range(len(ds)))
