"""Batched training augmentation: packer + dispatch for csrc/augment.hip.

``augment_batch`` warps a batch of raw records of different sizes into the
network's input image and the two stride-grid masks. On a GPU it packs the
records into one pinned staging buffer and one descriptor table (one H2D copy
each) and runs the fused warp kernel; on the CPU it runs the host
``Transformer.warp`` per sample, which is therefore the oracle of the kernel.
"""
from __future__ import annotations

import numpy as np
import torch

from ._backend import require_hip

# one row per sample; mirrors ``struct AugDesc`` in csrc/augment.hip
DESC_DTYPE = np.dtype([
    ("img_off", "<i8"), ("mask_off", "<i8"),
    ("hs", "<i4"), ("ws", "<i4"),
    ("mi", "<f4", (6,)),
    ("mask_scale", "<f4", (2,)),
    ("gain", "<f4", (3,)), ("shift", "<f4"),
    ("flags", "<i4"), ("pad", "<i4"),
])
assert DESC_DTYPE.itemsize == 80
FLAG_TINT = 1
FLAG_MASK_F32 = 2
_ALIGN = 16    # every source starts on a 16-byte boundary ...
_SLACK = 8     # ... and is followed by at least this many readable bytes


def inverse_affine(M) -> np.ndarray:
    """fp64 inverse (destination -> source) of a 2x3 source -> destination
    affine: the matrix ``Transformer._warp`` hands to scipy."""
    full = np.vstack([np.asarray(M, dtype=np.float64), [0.0, 0.0, 1.0]])
    return np.linalg.inv(full)[:2]


def _check_image(img):
    if not (isinstance(img, np.ndarray) and img.dtype == np.uint8
            and img.ndim == 3 and img.shape[2] == 3):
        raise ValueError("augment: images must be uint8 (H, W, 3) arrays, got "
                         f"{getattr(img, 'dtype', type(img))} "
                         f"{getattr(img, 'shape', '')}")


def _mask_scale(m) -> float:
    """``Transformer._to_float01`` as a factor."""
    return 1.0 / 255.0 if float(np.max(m)) > 1.5 else 1.0


class PackedBatch:
    """Host side of one batch: ``buffer`` (1-D uint8 tensor, pinned when
    asked) holds every image and mask pair, ``desc`` (structured array of
    ``DESC_DTYPE``) says where and how each is warped."""

    def __init__(self, buffer: torch.Tensor, desc: np.ndarray):
        self.buffer = buffer
        self.desc = desc

    def __len__(self):
        return len(self.desc)

    def unpack(self):
        """Views of the packed sources: ``[(image, mask_pair), ...]``."""
        raw = self.buffer.numpy()
        out = []
        for d in self.desc:
            hs, ws = int(d["hs"]), int(d["ws"])
            io, mo = int(d["img_off"]), int(d["mask_off"])
            img = raw[io:io + hs * ws * 3].reshape(hs, ws, 3)
            if d["flags"] & FLAG_MASK_F32:
                pair = raw[mo:mo + 2 * hs * ws * 4].view(np.float32)
            else:
                pair = raw[mo:mo + 2 * hs * ws]
            out.append((img, pair.reshape(2, hs, ws)))
        return out

    def validate(self):
        """Every source, plus the kernel's read-ahead, lies inside the buffer."""
        n = self.buffer.numel()
        for d in self.desc:
            hs, ws = int(d["hs"]), int(d["ws"])
            esize = 4 if d["flags"] & FLAG_MASK_F32 else 1
            io, mo = int(d["img_off"]), int(d["mask_off"])
            ok = (hs >= 1 and ws >= 1 and io >= 0 and mo >= 0
                  and mo % esize == 0
                  and io + hs * ws * 3 + _SLACK <= n
                  and mo + 2 * hs * ws * esize + _SLACK <= n)
            if not ok:
                raise ValueError("augment: descriptor points outside the "
                                 "packed buffer")


def pack_batch(images, mask_pairs, inv_mats, tints=None, pin=False) -> PackedBatch:
    """Pack ragged records for the kernel.

    images: list of uint8 (Hs, Ws, 3); mask_pairs: list of (2, Hs, Ws) uint8 or
    float32 (mask_miss, mask_all); inv_mats: list of 2x3 destination -> source
    affines; tints: list of ``None`` or ``(gains[3], shift)``.
    """
    B = len(images)
    if not (len(mask_pairs) == B and len(inv_mats) == B):
        raise ValueError("augment: images, masks and matrices differ in length")
    tints = tints if tints is not None else [None] * B
    desc = np.zeros(B, dtype=DESC_DTYPE)
    pairs = []
    off = 0

    def take(nbytes):
        nonlocal off
        start = off
        off = (start + nbytes + _SLACK + _ALIGN - 1) // _ALIGN * _ALIGN
        return start

    for i, (img, pair, mi, tint) in enumerate(zip(images, mask_pairs, inv_mats, tints)):
        _check_image(img)
        pair = np.asarray(pair)
        if pair.dtype != np.uint8:
            pair = pair.astype(np.float32, copy=False)
        if pair.shape != (2,) + img.shape[:2]:
            raise ValueError("augment: mask pair must be (2, H, W) of its image")
        pairs.append(pair)
        d = desc[i]
        d["hs"], d["ws"] = img.shape[:2]
        d["img_off"] = take(img.size)
        d["mask_off"] = take(pair.nbytes)
        d["mi"] = np.asarray(mi, dtype=np.float64).reshape(6)
        d["mask_scale"] = (_mask_scale(pair[0]), _mask_scale(pair[1]))
        flags = FLAG_MASK_F32 if pair.dtype == np.float32 else 0
        if tint is not None:
            d["gain"], d["shift"] = tint
            flags |= FLAG_TINT
        else:
            d["gain"] = 1.0
        d["flags"] = flags

    buffer = torch.empty(max(off, _ALIGN), dtype=torch.uint8, pin_memory=pin)
    raw = buffer.numpy()
    for d, img, pair in zip(desc, images, pairs):
        io, mo = int(d["img_off"]), int(d["mask_off"])
        raw[io:io + img.size] = img.reshape(-1)
        raw[mo:mo + pair.nbytes] = np.ascontiguousarray(pair).reshape(-1).view(np.uint8)
    return PackedBatch(buffer, desc)


def warp_packed(packed: PackedBatch, config, device, dtype=torch.float32):
    """H2D copy of a packed batch (one for the sources, one for the
    descriptors) + the fused warp kernel."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("augment: image dtype must be float32 or bfloat16")
    ext = require_hip()
    packed.validate()
    desc_host = torch.from_numpy(packed.desc.view(np.uint8).reshape(len(packed), -1))
    if packed.buffer.is_pinned():
        desc_host = desc_host.pin_memory()
    src = packed.buffer.to(device, non_blocking=True)
    desc = desc_host.to(device, non_blocking=True)
    img, miss, all_ = ext.augment_warp(src, desc, config.height, config.width,
                                       config.stride, dtype == torch.bfloat16)
    return img, miss, all_


def augment_batch(images, mask_pairs, mats, tints, config, device,
                  dtype=torch.float32):
    """Warp one batch by the source -> destination affines ``mats``.

    Returns ``(images (B,H,W,3) dtype, mask_miss (B,h,w) fp32, mask_all
    (B,h,w) fp32)`` on ``device``.
    """
    device = torch.device(device)
    for img in images:
        _check_image(img)
    tints = tints if tints is not None else [None] * len(images)
    if device.type == "cpu":
        from ..data.transformer import Transformer
        tf = Transformer(config)
        outs = [tf.warp(img, pair[0], pair[1], np.asarray(M, np.float32), tint)
                for img, pair, M, tint in zip(images, mask_pairs, mats, tints)]
        img, miss, all_ = (torch.from_numpy(np.stack([o[k] for o in outs]))
                           for k in range(3))
        return img.to(dtype), miss, all_
    packed = pack_batch(images, mask_pairs, [inverse_affine(M) for M in mats],
                        tints, pin=True)
    return warp_packed(packed, config, device, dtype)
