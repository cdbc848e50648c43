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
``find_people`` consumes. ``assemble_people`` (``csrc/people_assemble.hip``)
goes one stage further and runs ``find_people`` and ``subsets_to_keypoints`` on
those device outputs, bit-identically; ``decode_people`` turns host copies of
its outputs into the result format of ``process_batch``. On CPU tensors all
three ops run the existing host functions, which are also the oracle the
kernels are tested against.
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
MAX_PEOPLE = 128     # kAsmMaxPeople in people_assemble.hip: subset rows in LDS
N_PARTS = 18         # kAsmParts: part slots of a subset row
N_KEYPOINTS = 17     # kAsmKeypoints: COCO keypoints per person


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


# --------------------------------------------------------------------------
# person assembly (csrc/people_assemble.hip)
# --------------------------------------------------------------------------

def _mapping_table(dt_gt_mapping, n_parts):
    """``{part: COCO slot or None}`` (or a sequence) -> a tuple of ``n_parts``
    ints, -1 for a part without a COCO slot."""
    if isinstance(dt_gt_mapping, dict):
        # the last key mapped to a slot wins on the host; so does the highest
        # part index in the kernel
        if list(dt_gt_mapping) != sorted(dt_gt_mapping):
            raise ValueError("dt_gt_mapping keys must ascend")
        seq = [dt_gt_mapping.get(p) for p in range(n_parts)]
        if set(dt_gt_mapping) - set(range(n_parts)):
            raise ValueError("dt_gt_mapping names parts outside [0, n_parts)")
    else:
        seq = list(dt_gt_mapping)
    table = tuple(-1 if g is None else int(g) for g in seq)
    if len(table) != n_parts or any(not -1 <= g < N_KEYPOINTS for g in table):
        raise ValueError(f"dt_gt_mapping must give {n_parts} slots in "
                         f"[0, {N_KEYPOINTS}) or None")
    return table


@functools.lru_cache(maxsize=16)
def _device_mapping(device, table):
    return torch.tensor(table, dtype=torch.int32, device=device)


def assemble_people(peaks, offsets, rows, counts, limbs, dt_gt_mapping, len_rate,
                    connection_tole, remove_recon, max_people=MAX_PEOPLE):
    """Greedy person assembly (``find_people``) and ``subsets_to_keypoints`` of
    every image, on the device outputs of :func:`canonical_peaks` and
    :func:`limb_match`.

    ``limbs``: (partA, partB) per limb type; ``dt_gt_mapping``: COCO slot (or
    ``None``) per part, a dict or a sequence. Returns
    ``(n_people, subset, keypoints)``: int32 (N,), fp64
    (N, max_people, n_parts + 2, 2) subset rows in the layout and order of
    ``find_people``, and fp32 (N, max_people, 17, 2) COCO coordinates with
    ``(0, 0)`` for a missing keypoint. Only rows ``[0, n_people[n])`` of an
    image are defined. ``n_people[n] == OVERFLOW`` marks an image with an
    overflowed limb, a peak id outside the image's peaks, or more than
    ``max_people`` subset rows alive at once; the caller redoes it on the host.
    """
    limbs = tuple((int(a), int(b)) for a, b in limbs)
    max_people = int(max_people)
    if not 1 <= max_people <= MAX_PEOPLE:
        raise ValueError(f"max_people must be in [1, {MAX_PEOPLE}]")
    if peaks.dim() != 3 or peaks.shape[2] != 5 or peaks.shape[1] < 1 or \
            peaks.dtype != torch.float32:
        raise ValueError("peaks must be fp32 (N, max_peaks, 5)")
    N = peaks.shape[0]
    if offsets.dim() != 2 or offsets.shape[0] != N or \
            offsets.shape[1] != N_PARTS + 1 or offsets.dtype != torch.int32:
        raise ValueError(f"offsets must be int32 (N, {N_PARTS + 1})")
    if rows.dim() != 4 or rows.shape[0] != N or rows.shape[1] != len(limbs) or \
            not 1 <= rows.shape[2] <= MAX_PART or rows.shape[3] != 6 or \
            rows.dtype != torch.float32:
        raise ValueError(f"rows must be fp32 (N, L, max_part <= {MAX_PART}, 6)")
    if counts.shape != rows.shape[:2] or counts.dtype != torch.int32:
        raise ValueError("counts must be int32 (N, L)")
    if not limbs or any(not (0 <= a < N_PARTS and 0 <= b < N_PARTS)
                        for a, b in limbs):
        raise ValueError("limbs must name parts in [0, n_parts)")
    table = _mapping_table(dt_gt_mapping, N_PARTS)
    if use_hip_for(peaks):
        if peaks.shape[1] > MAX_PEAKS:
            raise ValueError(f"device assembly stages at most {MAX_PEAKS} peaks "
                             f"per image (max_peaks={peaks.shape[1]})")
        n_people, subset, keypoints = hip_extension().people_assemble(
            peaks.contiguous(), offsets.contiguous(), rows.contiguous(),
            counts.contiguous(), _device_limbs(peaks.device, limbs),
            _device_mapping(peaks.device, table), float(len_rate),
            float(connection_tole), int(remove_recon), max_people)
        return n_people, subset, keypoints
    return _assemble_host(peaks, offsets, rows, counts, limbs, table,
                          float(len_rate), float(connection_tole),
                          int(remove_recon), max_people)


def _assemble_host(peaks, offsets, rows, counts, limbs, table, len_rate,
                   connection_tole, remove_recon, max_people):
    """CPU fallback of ``assemble_people``: ``decode_assignment``, the host
    ``find_people`` and ``subsets_to_keypoints``, written into the op's
    layout."""
    from types import SimpleNamespace
    from ..engine.inference import find_people, subsets_to_keypoints

    config = SimpleNamespace(
        limbs_conn=list(limbs), heat_layers=N_PARTS,
        dt_gt_mapping={p: (None if g < 0 else g) for p, g in enumerate(table)})
    params = {"len_rate": len_rate, "connection_tole": connection_tole,
              "remove_recon": remove_recon}
    N = peaks.shape[0]
    n_people = np.zeros(N, dtype=np.int32)
    subset = np.zeros((N, max_people, N_PARTS + 2, 2), dtype=np.float64)
    keypoints = np.zeros((N, max_people, N_KEYPOINTS, 2), dtype=np.float32)
    decoded = decode_assignment(peaks.numpy(), offsets.numpy(), rows.numpy(),
                                counts.numpy())
    for n, (all_peaks, connection_all, special_k) in enumerate(decoded):
        n_cand = sum(len(sub) for sub in all_peaks)
        if any(c is None for c in connection_all) or any(
                len(c) and not ((c[:, :2] >= 0) & (c[:, :2] < n_cand)).all()
                for c in connection_all):
            n_people[n] = OVERFLOW
            continue
        stats = {}
        sub, candidate = find_people(connection_all, special_k, all_peaks,
                                     params, config, stats=stats)
        if stats["max_live"] > max_people:
            n_people[n] = OVERFLOW
            continue
        n_people[n] = len(sub)
        subset[n, :len(sub)] = sub
        for i, (coco, _) in enumerate(subsets_to_keypoints(sub, candidate, config)):
            keypoints[n, i] = [(0.0, 0.0) if pt is None else pt for pt in coco]
    return (torch.from_numpy(n_people), torch.from_numpy(subset),
            torch.from_numpy(keypoints))


def decode_people(n_people, keypoints, totals, dt_gt_mapping):
    """Host copies of :func:`assemble_people` outputs (numpy arrays) -> one
    list of ``(coco_keypoints, score)`` per image, the result format of
    ``process_batch``. ``totals``: fp64 (N, max_people), column 0 of subset row
    ``n_parts`` (the summed score). ``coco_keypoints`` holds 17 ``(x, y)``
    tuples, ``None`` for a COCO slot no part maps to; the score is
    ``1 - 1 / total``. An image flagged ``OVERFLOW`` gives ``None``."""
    n_people = np.asarray(n_people)
    totals = np.asarray(totals, dtype=np.float64)
    table = _mapping_table(dt_gt_mapping, N_PARTS)
    unmapped = [g for g in range(N_KEYPOINTS) if g not in table]
    # only rows below an image's count are defined: gather those, image by
    # image in order, and leave the rest of the buffers alone
    valid = np.arange(totals.shape[1])[None, :] < n_people[:, None]
    totals = totals[valid]
    with np.errstate(divide="ignore"):
        scores = np.where(totals > 0, 1 - 1.0 / totals, 0.0).tolist()
    points = np.asarray(keypoints)[valid].astype(np.float64).tolist()
    out, lo = [], 0
    for cnt in n_people.tolist():
        if cnt < 0:
            out.append(None)
            continue
        people = []
        for i in range(lo, lo + cnt):
            coco = [tuple(pt) for pt in points[i]]
            for g in unmapped:
                coco[g] = None
            people.append((coco, scores[i]))
        out.append(people)
        lo += cnt
    return out
