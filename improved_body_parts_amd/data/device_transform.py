"""Batched augmentation with the pixel work on the device.

``DeviceTransformer`` is the batch twin of ``Transformer``: the host draws the
``AugmentSelection``, composes the affine, moves the joints (a few hundred
floats) and draws the tint; image and masks are warped by ``ops.augment`` —
the HIP kernel on a GPU, ``Transformer.warp`` per sample on the CPU.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops.augment import augment_batch, inverse_affine, pack_batch, warp_packed
from .transformer import AugmentSelection, Transformer, transform_joints


class PreparedBatch:
    """Host half of one batch, ready for ``DeviceTransformer.execute``."""

    def __init__(self, joints, packed=None, host_args=None):
        self.joints = joints        # list of (P_i, num_parts, 3) float32
        self.packed = packed        # PackedBatch (GPU path)
        self.host_args = host_args  # (images, mask_pairs, mats, tints) (CPU path)


class DeviceTransformer:
    def __init__(self, config, device="cuda", dtype=torch.float32):
        self.config = config
        self.device = torch.device(device)
        self.dtype = dtype

    def prepare(self, records, augs=None, rng=None) -> PreparedBatch:
        """Everything that needs no device: draws, matrices, joints, packing.

        records: list of ``(img, mask_miss, mask_all, meta)`` as
        ``RawDataIterator.raw`` returns them; augs: list of
        ``AugmentSelection`` (``None`` entries, or ``None`` for the list, are
        drawn from ``rng``). Per sample the draw order is that of
        ``Transformer.transform``: the selection, then three tint gains, then
        the tint shift.
        """
        cfg = self.config
        augs = augs if augs is not None else [None] * len(records)
        images, pairs, mats, tints, joints = [], [], [], [], []
        for (img, mask_miss, mask_all, meta), aug in zip(records, augs):
            aug = aug or AugmentSelection.random(cfg.transform_params, rng)
            scale_self = meta.get("scale_provided", 1.0)
            center = np.asarray(meta["objpos"], dtype=np.float32).reshape(2)
            M = aug.affine(center, scale_self, cfg)
            joints.append(transform_joints(meta["joints"], M, aug.flip, cfg))
            tints.append(Transformer._tint_params(rng) if aug.tint else None)
            images.append(img)
            pairs.append((mask_miss, mask_all))
            mats.append(M)
        if self.device.type == "cpu":
            return PreparedBatch(joints, host_args=(images, pairs, mats, tints))
        packed = pack_batch(images, [_stack_pair(p) for p in pairs],
                            [inverse_affine(M) for M in mats],
                            tints, pin=True)
        return PreparedBatch(joints, packed=packed)

    def execute(self, prepared: PreparedBatch):
        """The device half: H2D + warp. Returns ``(images (B,H,W,3),
        mask_miss (B,h,w), mask_all (B,h,w), joints)``."""
        if prepared.packed is not None:
            img, miss, all_ = warp_packed(prepared.packed, self.config,
                                          self.device, self.dtype)
        else:
            images, pairs, mats, tints = prepared.host_args
            img, miss, all_ = augment_batch(images, pairs, mats, tints,
                                            self.config, self.device, self.dtype)
        return img, miss, all_, prepared.joints

    def transform_batch(self, records, augs=None, rng=None):
        return self.execute(self.prepare(records, augs, rng))


def _stack_pair(pair):
    """(mask_miss, mask_all) -> one (2, H, W) array; a mixed uint8/float pair
    is carried as float32 in each mask's own value range."""
    a, b = (np.asarray(m) for m in pair)
    if a.dtype == np.uint8 and b.dtype == np.uint8:
        return np.stack([a, b])
    return np.stack([a.astype(np.float32, copy=False),
                     b.astype(np.float32, copy=False)])
