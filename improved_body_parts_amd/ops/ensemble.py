"""Fused tail of the rotation-free ensemble forward.

``predict`` follows the network forward with a chain of eager ops per image:
mirror the flipped view back, permute its L/R channels, average the two views,
bicubic x-stride upsample to the padded size, crop the padding, bicubic resize
to the original size, scale by ``1 / n_runs`` and accumulate. The chain is a
separable linear map of the stride-resolution output, so on the GPU it is one
HIP kernel (``csrc/ensemble_merge.hip``) driven by per-axis tap tables composed
here; on the CPU ``ensemble_merge`` runs the torch chain itself, which is also
the oracle the kernel is tested against.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from ._backend import hip_extension, use_hip_for

TABLE_K = 8          # tap-table row pitch; must match kEmK in ensemble_merge.hip
_TILE_X = 64         # kEmTX
_TILE_Y = 16         # kEmTY
_WAVES = 4           # kEmWaves
_LDS_BUDGET = 48 * 1024
_MAX_CB = 25


# --------------------------------------------------------------------------
# composed per-axis operator
# --------------------------------------------------------------------------

def bicubic_matrix(n_in: int, n_out: int) -> np.ndarray:
    """(n_out, n_in) fp64 matrix of ``F.interpolate(mode="bicubic",
    align_corners=False)`` along one axis: cubic convolution with A = -0.75,
    source coordinate ``(i + 0.5) * n_in / n_out - 0.5`` and border taps
    clamped into the input."""
    A = -0.75
    m = np.zeros((n_out, n_in), dtype=np.float64)
    scale = n_in / n_out
    for i in range(n_out):
        src = (i + 0.5) * scale - 0.5
        i0 = int(np.floor(src))
        t = src - i0
        w = (((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A,
             ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1,
             ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A)
        for k in range(4):
            m[i, min(max(i0 - 1 + k, 0), n_in - 1)] += w[k]
    return m


def compose_axis_matrix(n_src: int, stride: int, n_crop: int, n_out: int) -> np.ndarray:
    """fp64 (n_out, n_src) operator of: bicubic upsample n_src -> n_src*stride,
    keep the first n_crop samples, bicubic resize n_crop -> n_out."""
    n_mid = n_src * stride
    if not 1 <= n_crop <= n_mid:
        raise ValueError(f"crop {n_crop} outside the upsampled extent {n_mid}")
    return bicubic_matrix(n_crop, n_out) @ bicubic_matrix(n_src, n_mid)[:n_crop]


@functools.lru_cache(maxsize=256)
def axis_table(n_src: int, stride: int, n_crop: int, n_out: int):
    """Tap table of the composed operator: ``(start int32[n_out],
    weights fp32[n_out, TABLE_K], span)``. Row ``i`` of the operator is
    ``weights[i, k]`` at source index ``start[i] + k``; unused taps are 0 and
    ``span`` is the widest run of taps any row really uses. Built in fp64,
    rounded once to fp32."""
    R = compose_axis_matrix(n_src, stride, n_crop, n_out)
    start = np.zeros(n_out, dtype=np.int32)
    weights = np.zeros((n_out, TABLE_K), dtype=np.float32)
    span = 1
    lo_next = n_src - 1
    for i in reversed(range(n_out)):
        nz = np.nonzero(R[i])[0]
        lo, hi = (int(nz[0]), int(nz[-1])) if len(nz) else (0, 0)
        # a tap whose weight is exactly 0 can shorten a row from the left; keep
        # the starts monotone (a tile's window begins at its first row's start)
        lo = lo_next = min(lo, lo_next)
        width = hi - lo + 1
        assert width <= TABLE_K, \
            f"composed bicubic row spans {width} source taps (> {TABLE_K})"
        span = max(span, width)
        start[i] = lo
        weights[i, :width] = R[i, lo:hi + 1]
    assert np.all(np.diff(start) >= 0)
    start.setflags(write=False)
    weights.setflags(write=False)
    return start, weights, span


def table_to_matrix(start, weights, n_src: int) -> np.ndarray:
    """Dense fp64 (n_out, n_src) matrix that a tap table encodes."""
    m = np.zeros((len(start), n_src), dtype=np.float64)
    for i, s in enumerate(start):
        for k in range(weights.shape[1]):
            if weights[i, k] != 0:
                m[i, s + k] += float(weights[i, k])
    return m


def _window(start, span: int, tile: int) -> int:
    """Source extent one output tile of ``tile`` samples reads."""
    n = len(start)
    first = start[0:n:tile].astype(np.int64)
    last = start[np.minimum(np.arange(0, n, tile) + tile - 1, n - 1)].astype(np.int64)
    return int((last - first).max()) + span


@functools.lru_cache(maxsize=64)
def _device_plan(device, C, h4, w4, stride, sh, sw, H, W):
    """Device copies of both tap tables plus the kernel's tile plan."""
    ys, yw, yspan = axis_table(h4, stride, sh, H)
    xs, xw, xspan = axis_table(w4, stride, sw, W)
    span = max(yspan, xspan)
    kt = 5 if span <= 5 else TABLE_K          # taps the kernel walks
    wr = _window(ys, kt, _TILE_Y)
    wc = _window(xs, kt, _TILE_X)
    cb = min(C, _MAX_CB)
    groups = -(-C // cb)
    cb = -(-C // groups)                      # even channel groups
    lds = lambda n: 4 * (n * ((wr * wc) | 1) + _WAVES * wr * _TILE_X)
    while cb > 1 and lds(cb) > _LDS_BUDGET:
        cb -= 1
    if lds(cb) > _LDS_BUDGET:
        raise RuntimeError(
            f"ensemble_merge: a {wr}x{wc} source window per output tile does "
            f"not fit the kernel's LDS budget (resize {h4}x{w4} -> {H}x{W})")
    dev = lambda a: torch.tensor(a, device=device)   # copies the read-only table
    return dict(ys=dev(ys), yw=dev(yw), xs=dev(xs), xw=dev(xw), span=span,
                wr=wr, wc=wc, cb=cb)


# --------------------------------------------------------------------------
# public op
# --------------------------------------------------------------------------

def merge_chain(out_lowres, flip_perm, stride, crop_hw, out_hw, scale=1.0,
                chan_order=None):
    """The eager torch chain (the tail of ``predict``), batched along N.
    Returns (N, C, H, W) fp32."""
    v = out_lowres.float()
    if chan_order is not None:
        v = v[:, torch.as_tensor(chan_order, dtype=torch.long, device=v.device)]
    perm = torch.as_tensor(flip_perm, dtype=torch.long, device=v.device)
    n = v.shape[0] // 2
    # flip ensemble: mirror the flipped copy back and permute L/R channels
    merged = (v[:n] + torch.flip(v[n:], dims=[-1])[:, perm]) * 0.5
    # x stride upsample, unpad, resize to original
    up = F.interpolate(merged, size=(v.shape[2] * stride, v.shape[3] * stride),
                       mode="bicubic", align_corners=False)
    up = up[:, :, :crop_hw[0], :crop_hw[1]]
    up = F.interpolate(up, size=tuple(out_hw), mode="bicubic", align_corners=False)
    return up * scale


def ensemble_merge(out_lowres, flip_perm, stride, crop_hw, out_hw, scale=1.0,
                   out=None, accumulate=False, chan_order=None):
    """Merge the ``[views | mirrored views]`` network output into full-size maps.

    ``out_lowres``: (2N, Cs, h4, w4) bf16/fp32, view ``n`` is image ``n`` and
    view ``N + n`` its horizontal mirror. ``chan_order`` (length C, default
    identity) picks the output channels out of the Cs network channels;
    ``flip_perm`` (length C) is the L/R permutation in that output order.
    The maps are upsampled x ``stride``, cropped to ``crop_hw`` and resized to
    ``out_hw``. Returns ``out`` (N, C, H, W) fp32 planar: written with
    ``scale * result`` or, if ``accumulate``, incremented by it.
    """
    if out_lowres.dim() != 4 or out_lowres.shape[0] % 2:
        raise ValueError("out_lowres must be (2N, C, h4, w4)")
    n, cs, h4, w4 = out_lowres.shape[0] // 2, *out_lowres.shape[1:]
    order = np.arange(cs) if chan_order is None else np.asarray(chan_order)
    perm = np.asarray(flip_perm.cpu() if torch.is_tensor(flip_perm) else flip_perm)
    C = len(order)
    if perm.shape != (C,) or sorted(perm.tolist()) != list(range(C)):
        raise ValueError("flip_perm must be a permutation of the output channels")
    if order.min() < 0 or order.max() >= cs:
        raise ValueError("chan_order outside the network's channels")
    H, W = int(out_hw[0]), int(out_hw[1])
    sh, sw = int(crop_hw[0]), int(crop_hw[1])
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs an existing `out`")
        out = torch.empty(n, C, H, W, device=out_lowres.device, dtype=torch.float32)
    if out.shape != (n, C, H, W) or out.dtype != torch.float32 \
            or not out.is_contiguous():
        raise ValueError("out must be contiguous fp32 (N, C, H, W)")

    if not use_hip_for(out_lowres):
        res = merge_chain(out_lowres, perm, stride, (sh, sw), (H, W), scale,
                          chan_order)
        if accumulate:
            out += res
        else:
            out.copy_(res)
        return out

    plan = _device_plan(out_lowres.device, C, h4, w4, int(stride), sh, sw, H, W)
    chan = _device_channels(out_lowres.device, tuple(order.tolist()),
                            tuple(perm.tolist()))
    src = out_lowres.permute(0, 2, 3, 1).contiguous()   # free for channels_last
    hip_extension().ensemble_merge(
        src, chan[0], chan[1], plan["ys"], plan["yw"], plan["xs"], plan["xw"],
        out, float(scale), bool(accumulate), plan["cb"], plan["wr"], plan["wc"],
        plan["span"])
    return out


@functools.lru_cache(maxsize=16)
def _device_channels(device, order, perm):
    order = np.asarray(order, dtype=np.int32)
    perm = np.asarray(perm, dtype=np.int64)
    return (torch.from_numpy(order).to(device),
            torch.from_numpy(np.ascontiguousarray(order[perm])).to(device))
