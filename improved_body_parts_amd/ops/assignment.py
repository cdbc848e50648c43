"""Device-side keypoint assignment: canonical peak order and limb matching.

``find_peaks_batch`` / ``find_connections_batch`` bring the peak buffer to the
host, enumerate every (limb, peakA, peakB) candidate in Python, upload the
list, score it on the device, copy the scores back and match on the host. The
two ops here keep all of that on the device (``csrc/limb_match.hip``):

  * ``canonical_peaks`` orders the buffer of ``peaks_batched`` as the host does
    (channel, refined y, refined x), so a peak's id is its row index, and
    returns per-channel offsets;
  * ``limb_match`` scores, filters and greedily matches all ``nA x nB``
    segments of every (image, limb type) and returns finished connection rows.

``decode_assignment`` turns host copies of their outputs into the structures
``find_people`` consumes. On CPU tensors both ops run the existing host
functions, which are also the oracle the kernels are tested against.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from ._backend import hip_extension, use_hip_for

MAX_PART = 64        # kMatchMaxPart in limb_match.hip: one 64-bit mask per side
MAX_PEAKS = 512      # kCanonMaxPeaks: rows peaks_canonical stages in LDS
OVERFLOW = -2        # count of a limb whose part has more than max_part peaks
NO_PEAKS = -1        # count of a limb with a part that has no peak (special_k)


def _buffer_counts(buf_np, max_peaks):
    """Per-image peak counts of a ``peaks_batched`` buffer, clamped to the cap
    (the device counter keeps counting past it)."""
    counts = np.ascontiguousarray(buf_np[:, 0, 0]).view(np.int32)
    return np.clip(counts, 0, max_peaks)


def canonical_peaks(buf, n_parts):
    """Order a ``peaks_batched`` buffer (N, 1 + max_peaks, 5) as the host does.

    Returns ``(peaks, offsets)``: fp32 (N, max_peaks, 5) rows
    ``[channel, x, y, score, peak]`` sorted by channel, then y, then x (exact
    ties keep arrival order), zero past the image's count, and int32
    (N, n_parts + 1) offsets: channel ``c`` owns rows
    ``[offsets[c], offsets[c + 1])`` and ``offsets[n_parts]`` is the count.
    """
    if buf.dim() != 3 or buf.shape[1] < 2 or buf.shape[2] != 5:
        raise ValueError("buf must be (N, 1 + max_peaks, 5)")
    n_parts = int(n_parts)
    if use_hip_for(buf):
        peaks, offsets = hip_extension().peaks_canonical(
            buf.contiguous().float(), n_parts)
        return peaks, offsets
    buf_np = buf.contiguous().float().numpy()
    N, max_peaks = buf_np.shape[0], buf_np.shape[1] - 1
    peaks = np.zeros((N, max_peaks, 5), dtype=np.float32)
    offsets = np.zeros((N, n_parts + 1), dtype=np.int32)
    for n, cnt in enumerate(_buffer_counts(buf_np, max_peaks)):
        rows = buf_np[n, 1:1 + cnt].copy()
        rows[:, 0] = np.clip(np.nan_to_num(rows[:, 0]), 0, n_parts - 1) \
            .astype(np.int32)
        rows = rows[np.lexsort((rows[:, 1], rows[:, 2], rows[:, 0]))]
        peaks[n, :cnt] = rows
        offsets[n] = np.searchsorted(rows[:, 0], np.arange(n_parts + 1))
    return torch.from_numpy(peaks), torch.from_numpy(offsets)


@functools.lru_cache(maxsize=16)
def _device_limbs(device, limbs):
    return torch.tensor(limbs, dtype=torch.int32, device=device).reshape(-1, 2)


def limb_match(maps, peaks, offsets, limbs, first_limb_plane, mid_num, thre2,
               connect_ration, max_part=MAX_PART):
    """Score and greedily match the limbs of every image on the device.

    ``maps``: planar fp32 (N, planes, H, W) whose limb planes start at
    ``first_limb_plane``; ``peaks`` / ``offsets`` as :func:`canonical_peaks`
    returns them; ``limbs``: (partA, partB) per limb type. Returns
    ``(rows, counts)``: fp32 (N, L, max_part, 6) connection rows
    ``[idA, idB, score, i, j, length]`` and int32 (N, L) counts. Only the first
    ``counts[n, k]`` rows of a limb are defined; ``NO_PEAKS`` marks a limb with
    an empty part and ``OVERFLOW`` one with more than ``max_part`` peaks in a
    part, which the caller has to redo on the host.
    """
    limbs = tuple((int(a), int(b)) for a, b in limbs)
    n_parts = offsets.shape[1] - 1
    max_part = int(max_part)
    if not 1 <= max_part <= MAX_PART:
        raise ValueError(f"max_part must be in [1, {MAX_PART}]")
    if not limbs or any(not (0 <= a < n_parts and 0 <= b < n_parts)
                        for a, b in limbs):
        raise ValueError("limbs must name parts in [0, n_parts)")
    if first_limb_plane < 0 or first_limb_plane + len(limbs) > maps.shape[1]:
        raise ValueError("limb planes outside maps")
    if use_hip_for(maps):
        rows, counts = hip_extension().limb_match(
            maps.contiguous().float(), peaks, offsets,
            _device_limbs(maps.device, limbs), int(first_limb_plane),
            int(mid_num), float(thre2), float(connect_ration), max_part)
        return rows, counts
    return _limb_match_host(maps, peaks, offsets, limbs, int(first_limb_plane),
                            int(mid_num), float(thre2), float(connect_ration),
                            max_part)


def _peak_lists(peaks_np, off_np):
    """``all_peaks`` of one image: per part a list of ``(x, y, score, id)``
    with the id equal to the row index."""
    vals = peaks_np[:, 1:4].astype(np.float64).tolist()
    bounds = np.clip(off_np, 0, len(vals)).tolist()
    return [[(*vals[r], r) for r in range(lo, hi)]
            for lo, hi in zip(bounds[:-1], bounds[1:])]


def _limb_match_host(maps, peaks, offsets, limbs, first_limb_plane, mid_num,
                     thre2, connect_ration, max_part):
    """CPU fallback of ``limb_match``: the host scoring and greedy matching of
    ``find_connections_batch``, limb by limb, written into the op's layout."""
    from types import SimpleNamespace
    from ..engine.inference import _greedy_match, _limb_scores_host

    maps_np = maps.contiguous().float().numpy()
    peaks_np, off_np = peaks.numpy(), offsets.numpy()
    N, L = maps_np.shape[0], len(limbs)
    rows = np.zeros((N, L, max_part, 6), dtype=np.float32)
    counts = np.zeros((N, L), dtype=np.int32)
    params = {"connect_ration": connect_ration}
    for n in range(N):
        all_peaks = _peak_lists(peaks_np[n], off_np[n])
        for k, (a, b) in enumerate(limbs):
            if max(len(all_peaks[a]), len(all_peaks[b])) > max_part:
                counts[n, k] = OVERFLOW
                continue
            plane = maps_np[n, first_limb_plane + k]
            meta = [(0, i, j) for i in range(len(all_peaks[a]))
                    for j in range(len(all_peaks[b]))]
            scores = np.array(
                [_limb_scores_host(plane, all_peaks[a][i], all_peaks[b][j],
                                   mid_num, thre2) for _, i, j in meta],
                dtype=np.float32).reshape(-1, 3)
            conns, special_k = _greedy_match(
                all_peaks, scores, meta, params,
                SimpleNamespace(limbs_conn=[(a, b)]))
            if special_k:
                counts[n, k] = NO_PEAKS
            else:
                counts[n, k] = len(conns[0])
                rows[n, k, :len(conns[0])] = conns[0]
    return torch.from_numpy(rows), torch.from_numpy(counts)


def decode_assignment(peaks, offsets, rows, counts):
    """Host copies of :func:`canonical_peaks` / :func:`limb_match` outputs
    (numpy arrays) -> one ``(all_peaks, connection_all, special_k)`` per image
    in the structures of ``find_peaks_batch`` / ``find_connections_batch``:
    ``all_peaks`` per part a list of ``(x, y, score, id)``; ``connection_all``
    per limb an (n, 6) float64 array, ``[]`` for a limb in ``special_k``, or
    ``None`` for a limb that overflowed ``max_part`` (to be redone on the
    host)."""
    peaks, offsets = np.asarray(peaks), np.asarray(offsets)
    rows, counts = np.asarray(rows), np.asarray(counts)
    out = []
    for n in range(peaks.shape[0]):
        all_peaks = _peak_lists(peaks[n], offsets[n])
        connection_all, special_k = [], []
        for k, cnt in enumerate(counts[n].tolist()):
            if cnt == NO_PEAKS:
                special_k.append(k)
                connection_all.append([])
            elif cnt < 0:
                connection_all.append(None)
            else:
                cnt = min(cnt, rows.shape[2])
                connection_all.append(rows[n, k, :cnt].astype(np.float64))
        out.append((all_peaks, connection_all, special_k))
    return out
