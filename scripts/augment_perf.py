#!/usr/bin/env python
"""Input-pipeline rates at the training shape (512^2, batch 16) on COCO-like
640x480 records, three paths alternated round by round in one process:

  (a) host ``Transformer.transform`` alone (records already read);
  (b) host ``RawDataIterator.gen``: read + Transformer + numpy Heatmapper;
  (c) ``DeviceAugmentLoader``: read + draw + pack, H2D, HIP warp, HIP GT.

(c) is also split into its two halves, each timed alone: the producer (what
the loader's host thread does per batch) and the device side (H2D + warp + GT
of an already packed batch, ending in a synchronise), which shows which of the
two limits the overlapped stream.

The records are generated from a seed in the h5 layout (uint8 images, float32
mask pairs, as ``build_coco_h5`` writes them) and served from memory, so no
path pays for file decoding. Needs a GPU for (c); ``--host-only`` rehearses
(a) and (b) without one.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from improved_body_parts_amd.config import CanonicalConfig, COCOSourceConfig  # noqa: E402
from improved_body_parts_amd.data import (AugmentSelection, DeviceAugmentLoader,  # noqa: E402
                                          MyDataset)

TRAIN_STEP_IMG_S = 143.0   # measured training step, 512^2 batch 16, one MI355X


class _DS:
    def __init__(self, v):
        self.v = v

    def __getitem__(self, idx):
        return self.v


class _H5(dict):
    def get(self, k, default=None):
        return super().get(k, default)


def coco_like(cfg, n, seed=0, H=480, W=640):
    rng = np.random.default_rng(seed)
    dataset, images, masks = {}, {}, {}
    for k in range(n):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        mask_miss = np.ones((H, W), np.float32)
        mask_all = np.zeros((H, W), np.float32)
        people = []
        for _ in range(int(rng.integers(1, 5))):
            cx, cy = rng.uniform(120, W - 120), rng.uniform(120, H - 120)
            size = rng.uniform(80, 220)
            joints = np.zeros((17, 3), np.float32)
            joints[:, 0] = cx + rng.uniform(-0.3, 0.3, 17) * size
            joints[:, 1] = cy + rng.uniform(-0.5, 0.5, 17) * size
            joints[:, 2] = rng.integers(0, 3, 17)
            people.append(joints.tolist())
            x0, x1 = int(max(cx - size / 3, 0)), int(min(cx + size / 3, W))
            y0, y1 = int(max(cy - size / 2, 0)), int(min(cy + size / 2, H))
            mask_all[y0:y1, x0:x1] = 1.0
        mask_miss[40:120, 60:200] = 0.0
        first = np.asarray(people[0])
        name = f"{k:012d}.jpg"
        meta = {"image": name, "objpos": [float(first[:, 0].mean()),
                                          float(first[:, 1].mean())],
                "scale_provided": float(np.ptp(first[:, 1])) / cfg.height,
                "joints": people}
        dataset[str(k)] = _DS(json.dumps(meta))
        images[name] = _DS(img)
        masks[name] = _DS(np.stack([mask_miss, mask_all]))
    return _H5({"dataset": dataset, "images": images, "masks": masks})


class Repeated:
    """The dataset seen ``times`` over (the reader wraps indices itself)."""

    def __init__(self, ds, times):
        self.iterator = ds.iterator
        self.n = len(ds) * times

    def __len__(self):
        return self.n


def rate_host_transform(ds, cfg, samples, rng):
    it = ds.iterator
    recs = [it.raw(i) for i in range(samples)]
    t0 = time.perf_counter()
    for rec in recs:
        aug = AugmentSelection.random(cfg.transform_params, rng)
        it.transformer.transform(*rec, aug=aug, rng=rng)
    return samples / (time.perf_counter() - t0)


def rate_host_gen(ds, samples):
    t0 = time.perf_counter()
    for i in range(samples):
        ds.iterator.gen(i)
    return samples / (time.perf_counter() - t0)


def rate_loader(loader, epoch):
    loader.set_epoch(epoch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for images, _, _ in loader:
        n += images.shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def rate_producer(loader, steps, rng):
    share = loader.epoch_indices()
    B = loader.batch_size
    t0 = time.perf_counter()
    for s in range(steps):
        loader._host_batch(share[s * B:(s + 1) * B], rng)
    return steps * B / (time.perf_counter() - t0)


def rate_device_side(loader, steps, rng):
    B = loader.batch_size
    prepared = loader._host_batch(loader.epoch_indices()[:B], rng)
    loader._device_batch(prepared)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loader._device_batch(prepared)
    torch.cuda.synchronize()
    return steps * B / (time.perf_counter() - t0)


def summary(name, vals):
    med = statistics.median(vals)
    print(f"{name:<44s} median {med:9.1f}  min {min(vals):9.1f}  "
          f"max {max(vals):9.1f}  samples/s  rounds {['%.1f' % v for v in vals]}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--records", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-samples", type=int, default=64,
                    help="samples per round for the host paths")
    ap.add_argument("--steps", type=int, default=200,
                    help="batches per round for the device path")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--device-only", action="store_true",
                    help="only the device side of (c): for a profiler run")
    args = ap.parse_args()
    if not args.host_only and not torch.cuda.is_available():
        raise SystemExit("augment_perf: no GPU; the device path is not "
                         "measured elsewhere (use --host-only to rehearse)")

    cfg = CanonicalConfig(args.size, args.size, 4)
    ds = MyDataset(cfg, COCOSourceConfig("unused.h5"), augment=True,
                   h5_file=coco_like(cfg, args.records))
    rng = random.Random(0)
    random.seed(0)
    print(f"shape {args.size}^2 batch {args.batch}, {args.records} records of "
          f"640x480 uint8 + float32 mask pairs, image dtype {args.dtype}, "
          f"{args.rounds} rounds alternating the paths")
    loader = None
    if not args.host_only:
        print(f"device: {torch.cuda.get_device_name(0)}")
        times = -(-args.steps * args.batch // args.records)
        loader = DeviceAugmentLoader(
            Repeated(ds, times), args.batch, "cuda",
            torch.bfloat16 if args.dtype == "bf16" else torch.float32, seed=1)
        rate_device_side(loader, 3, rng)          # warm-up: code objects, pins
        if args.device_only:
            print(f"device side alone: "
                  f"{rate_device_side(loader, args.steps, rng):.1f} samples/s")
            return

    a, b, c, prod, dev = [], [], [], [], []
    for r in range(args.rounds):
        a.append(rate_host_transform(ds, cfg, args.host_samples, rng))
        b.append(rate_host_gen(ds, args.host_samples))
        if loader is not None:
            c.append(rate_loader(loader, r))
            prod.append(rate_producer(loader, max(args.steps // 4, 1), rng))
            dev.append(rate_device_side(loader, 5 * args.steps, rng))
    ma = summary("(a) host Transformer.transform", a)
    mb = summary("(b) host Transformer + Heatmapper (gen)", b)
    if loader is None:
        return
    mc = summary("(c) DeviceAugmentLoader (overlapped)", c)
    mp = summary("    (c) producer alone: read+draw+pack", prod)
    md = summary("    (c) device side alone: H2D+warp+GT", dev)
    spread = max(b) - min(b)
    faster = mc - mb > spread
    print(f"claim rule: (c) - (b) = {mc - mb:.1f} vs (b) max-min {spread:.1f} -> "
          f"(c) is {'faster than' if faster else 'NOT shown faster than'} (b)"
          + (f", {mc / mb:.1f}x" if faster else ""))
    print(f"(c) as a share of the {TRAIN_STEP_IMG_S:.0f} img/s training step: "
          f"{100 * mc / TRAIN_STEP_IMG_S:.0f} %")
    print(f"limit of (c): the {'producer thread' if mp < md else 'device side'} "
          f"(producer {mp:.0f} vs device {md:.0f} samples/s)")
    print(f"host processes needed to feed one GPU at {TRAIN_STEP_IMG_S:.0f} img/s: "
          f"(b) {TRAIN_STEP_IMG_S / mb:.1f}, (c) {TRAIN_STEP_IMG_S / mc:.2f}")


if __name__ == "__main__":
    main()
