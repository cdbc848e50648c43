"""Device-side augmentation on the GPU: the fused warp kernel against the fp64
rendering of its rule, the loader against the host pipeline, the trainer flag.

Tolerances: for the two integer-matrix augmentations the arithmetic is exact,
so every pixel is held to 1e-6; for the others a result must lie within 10x the
error of the fp32 numpy rendering of the same rule (computed per case), with the
pixels within 1e-3 px of the source border left out (their share is capped at
0.5 %, see test_device_augment_cpu.py).
"""
import functools

import numpy as np
import pytest
import torch

import augment_oracle as O
from improved_body_parts_amd.data import (AugmentSelection, DeviceAugmentLoader,
                                          Heatmapper, MyDataset, Transformer,
                                          transform_joints)
from improved_body_parts_amd.ops.augment import augment_batch

pytestmark = pytest.mark.gpu

SIZES = list(O.CONFIGS)
NAMES = list(O.AUGS)


@functools.lru_cache(maxsize=None)
def _records(size, mask_kind):
    return O.make_records(O.CONFIGS[size], np.uint8 if mask_kind == "u8" else np.float32)


@functools.lru_cache(maxsize=None)
def _mats(size, name):
    cfg = O.CONFIGS[size]
    return [O.forward_matrix(r, O.make_aug(name), cfg) for r in _records(size, "u8")]


@functools.lru_cache(maxsize=None)
def _expected(size, name, tint):
    """fp64 oracle + tolerances per sample (masks: the same for 0/255 uint8
    and 0/1 float32 inputs, which normalise to the same values)."""
    cfg = O.CONFIGS[size]
    return [O.Expected(r, M, cfg, O.TINT if tint else None,
                       exact=name in O.INTEGER_CASES)
            for r, M in zip(_records(size, "u8"), _mats(size, name))]


def _run(size, name, tint, mask_kind="u8", dtype=torch.float32, only=None):
    cfg = O.CONFIGS[size]
    recs, mats = _records(size, mask_kind), _mats(size, name)
    if only is not None:
        recs, mats = [recs[only]], [mats[only]]
    out = augment_batch([r[0] for r in recs],
                        [np.stack([r[1], r[2]]) for r in recs], mats,
                        [O.TINT if tint else None] * len(recs), cfg, "cuda", dtype)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("tint", [False, True], ids=["plain", "tint"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("size", SIZES)
def test_image_matches_fp64_oracle(size, name, tint, dtype):
    img, _, _ = _run(size, name, tint, dtype=dtype)
    cfg = O.CONFIGS[size]
    assert img.shape == (5, cfg.height, cfg.width, 3) and img.dtype == dtype
    got = img.float().cpu().numpy()
    for i, exp in enumerate(_expected(size, name, tint)):
        exp.check_image(got[i], f"{size} {name} tint={tint} sample {i}",
                        bf16=dtype == torch.bfloat16)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("size", SIZES)
def test_masks_match_fp64_oracle(size, name):
    _, miss8, all8 = _run(size, name, False, "u8")
    _, miss32, all32 = _run(size, name, False, "f32")
    h, w = O.CONFIGS[size].mask_shape
    for t in (miss8, all8, miss32, all32):
        assert t.shape == (5, h, w) and t.dtype == torch.float32
    for i, exp in enumerate(_expected(size, name, False)):
        label = f"{size} {name} sample {i}"
        exp.check_masks(miss8[i].cpu().numpy(), all8[i].cpu().numpy(), label + " u8")
        exp.check_masks(miss32[i].cpu().numpy(), all32[i].cpu().numpy(), label + " f32")
        # 0/255 uint8 and 0/1 float32 inputs agree with each other
        exp.check_masks(miss8[i].cpu().numpy(), all8[i].cpu().numpy(),
                        label + " u8 vs f32",
                        want=(miss32[i].cpu().numpy(), all32[i].cpu().numpy()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("size", SIZES)
def test_repeatable_and_rows_independent(size, dtype):
    first = _run(size, "rot33", True, "f32", dtype)
    second = _run(size, "rot33", True, "f32", dtype)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # a batch of one equals its row of the batch of five: descriptors and
    # offsets of the ragged sources are not mixed up
    for i in range(5):
        single = _run(size, "rot33", True, "f32", dtype, only=i)
        for a, b in zip(single, first):
            assert torch.equal(a[0], b[i]), f"sample {i}"


def test_loader_matches_host_pipeline(monkeypatch):
    from improved_body_parts_amd.config import CanonicalConfig
    cfg = CanonicalConfig(128, 128, 4)
    cfg.transform_params.tint_prob = 0.5
    h5, src = O.coco_fixture(cfg, n=4)
    ds = MyDataset(cfg, src, augment=True, h5_file=h5)

    # record what the loader draws, to replay it through the host pipeline
    drawn, tints = [], []
    draw = AugmentSelection.random.__func__
    draw_tint = Transformer._tint_params

    def recording_draw(cls, tp, rng=None):
        drawn.append(draw(cls, tp, rng))
        return drawn[-1]

    def recording_tint(rng=None):
        tints.append(draw_tint(rng))
        return tints[-1]

    monkeypatch.setattr(AugmentSelection, "random", classmethod(recording_draw))
    monkeypatch.setattr(Transformer, "_tint_params", staticmethod(recording_tint))
    loader = DeviceAugmentLoader(ds, batch_size=4, device="cuda",
                                 dtype=torch.float32, shuffle=False, seed=2)
    batches = list(loader)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(batches) == 1 and len(drawn) == 4
    images, mask_miss, heatmaps = (t.cpu().numpy() for t in batches[0])
    h, w = cfg.mask_shape
    assert images.shape == (4, 128, 128, 3) and mask_miss.shape == (4, 1, h, w)
    assert heatmaps.shape == (4, cfg.num_layers, h, w)

    tf, hm = Transformer(cfg), Heatmapper(cfg)
    tints = iter(tints)
    for i, aug in enumerate(drawn):
        rec = ds.iterator.raw(i)
        M = O.forward_matrix(rec, aug, cfg)
        tint = next(tints) if aug.tint else None
        want_img, want_miss, want_all = tf.warp(rec[0], rec[1], rec[2], M, tint)
        joints = transform_joints(rec[3]["joints"], M, aug.flip, cfg)
        want_heat = hm.create_heatmaps(joints, want_all)

        exp = O.Expected(rec, M, cfg, tint)
        label = f"loader sample {i}"
        exp.check_image(images[i], label, want=want_img)
        keep = ~exp.cells
        err = np.abs(mask_miss[i, 0].astype(np.float64) - want_miss)[keep].max()
        print(f"{label}: mask_miss err {err:.3e} tol {exp.mask_tol:.3e}")
        assert exp.cells.mean() <= O.BAND_CAP and err <= exp.mask_tol

        # GT: the existing device-GT tolerance; the eroded-mask background also
        # carries the mask's own tolerance, outside the 3x3 reach of band cells
        allow = 2e-5 + 1e-4 * np.abs(want_heat)
        err = np.abs(heatmaps[i].astype(np.float64) - want_heat)
        independent = [c for c in range(cfg.num_layers) if c != cfg.bkg_start]
        print(f"{label}: heatmap err {err[independent].max():.3e} "
              f"bkg err {err[cfg.bkg_start].max():.3e}")
        assert (err[independent] <= allow[independent]).all()
        pad = np.pad(exp.cells, 1, mode="edge")
        reach = np.zeros_like(exp.cells)
        for dy in range(3):
            for dx in range(3):
                reach |= pad[dy:dy + h, dx:dx + w]
        bkg_ok = err[cfg.bkg_start] <= allow[cfg.bkg_start] + exp.mask_tol
        assert (bkg_ok | reach).all()


def test_trainer_device_augment_takes_two_steps(small_opt, tmp_path):
    from improved_body_parts_amd.config import CanonicalConfig
    from improved_body_parts_amd.engine import Trainer
    cfg = CanonicalConfig(128, 128, 4)
    h5, src = O.coco_fixture(cfg, n=4)
    ds = MyDataset(cfg, src, augment=True, h5_file=h5)
    torch.manual_seed(0)
    tr = Trainer(small_opt, cfg, ds, rank=0, world_size=1, num_workers=0,
                 checkpoint_dir=str(tmp_path), device=torch.device("cuda", 0),
                 device_augment=True)
    assert isinstance(tr.train_loader, DeviceAugmentLoader)
    assert len(tr.train_loader) == 2
    losses = [tr.train_step(batch) for batch in tr.train_loader]
    assert len(losses) == 2
    assert all(l is not None and np.isfinite(l) for l in losses)

    # without the flag, or without a raw() reader, nothing changes
    plain = Trainer(small_opt, cfg, ds, rank=0, world_size=1, num_workers=0,
                    checkpoint_dir=str(tmp_path), device=torch.device("cuda", 0))
    assert not isinstance(plain.train_loader, DeviceAugmentLoader)
