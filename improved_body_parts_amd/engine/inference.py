"""End-to-end inference + keypoint assignment pipeline.

Capability parity with the reference's L5 layer (evaluate.py / demo_image.py):
``predict`` (multi-scale x rotation x horizontal-flip ensemble forward,
reference evaluate.py:83-161), ``find_peaks`` (NMS + sub-pixel centroid,
:169-203), ``find_connections`` (20-point limb line-integral scoring + greedy
1-1 matching, :206-276), ``find_people`` (greedy subset assembly with
overwrite / merge-disjoint / competition semantics, :279-498), ``process``
(:500-542), ``format_results`` / ``validation`` (:563-622, gated on
pycocotools which this offline image lacks).

MI355X-first design differences from the reference (behavior preserved):

  * The whole ensemble stays ON DEVICE as torch tensors — resizing, padding,
    rotation, flip ensembling and score-map averaging are bicubic
    ``F.interpolate`` / ``grid_sample`` on the GPU instead of cv2 on the host;
    only the final few hundred peak rows ever cross PCIe.
  * Peak NMS + centroid refinement and the O(limbs x nA x nB x 20) limb
    line-integral scoring run as HIP kernels (ops/csrc/postproc.hip,
    limb_match.hip); the host keeps the greedy matching and assembly over
    device-scored candidates. This is the fix for the reference's 5.2-FPS
    pure-Python bottleneck (reference README.md:68). ``matching="device"``
    (``assign_batch``) also moves candidate enumeration, the acceptance
    criteria and the greedy 1-1 matching into one kernel, leaving the host
    ``find_people`` and one synchronisation per batch. ``assembly="device"``
    (``people_batch``) adds the greedy person assembly and the COCO keypoint
    gather as a fourth kernel (people_assemble.hip), bit-identical to
    ``find_people``: the one copy back then carries finished people only.
  * Everything falls back to the same torch ops on CPU so the pipeline is
    unit-testable without a GPU.
  * Every stage is written once, for a list of images and a planar
    (N, heat + paf, H, W) buffer; ``predict``, ``find_peaks``,
    ``find_connections`` and ``process`` are the N = 1 wrappers.
"""
from __future__ import annotations

import collections
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from ..config import CanonicalConfig, InferenceParams
from ..ops._backend import use_hip_for, hip_extension
from ..ops.assignment import (MAX_PEAKS, OVERFLOW, assemble_people,
                              canonical_peaks, decode_assignment, decode_people,
                              limb_match)
from ..ops.ensemble import ensemble_merge
from ..utils import keypoint_heatmap_nms, refine_centroid


# --------------------------------------------------------------------------
# device-side image ops (replace the reference's cv2 calls)
# --------------------------------------------------------------------------

def _to_device_image(image, device, dtype=torch.float32):
    """(H, W, 3) numpy uint8/float or torch tensor -> (H, W, 3) fp32 in [0,1]."""
    if isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image))
    else:
        t = image
    t = t.to(device=device)
    if t.dtype == torch.uint8:
        t = t.to(dtype) / 255.0
    else:
        t = t.to(dtype)
    return t


def _rotate_nchw(x, angle_deg, inverse=False):
    """Rotate an (N, C, H, W) batch about its center (reference cv2.warpAffine
    with getRotationMatrix2D; the reference passes (h/2, w/2) as the cv2
    center which is an x/y mix-up for non-square inputs — inputs there are
    always padded square; we rotate about the true center)."""
    if angle_deg == 0:
        return x
    a = math.radians(angle_deg if not inverse else -angle_deg)
    cos, sin = math.cos(a), math.sin(a)
    # grid_sample samples the INPUT at the transformed output coordinates, so
    # the theta matrix is the inverse rotation; normalized coords are square
    # only if H == W, so fold the aspect ratio in explicitly:
    # x' = cos*x - sin*(y*H/W); y' = sin*(x*W/H) + cos*y
    H, W = x.shape[2], x.shape[3]
    theta = torch.tensor([[cos, -sin * H / W, 0.0],
                          [sin * W / H, cos, 0.0]],
                         dtype=torch.float32, device=x.device)
    xf = x.float()
    grid = F.affine_grid(theta[None].expand(x.shape[0], -1, -1), xf.shape,
                         align_corners=False)
    out = F.grid_sample(xf, grid, mode="bilinear", padding_mode="zeros",
                        align_corners=False)
    return out.to(x.dtype)


def _resolve_params(params, model_params):
    """Fill missing ``params`` / ``model_params`` from ``InferenceParams``."""
    if params is None or model_params is None:
        p, mp = InferenceParams().as_params_dict()
        params = params or p
        model_params = model_params or mp
    return params, model_params


def _scaled_geometry(H, W, scale, pad_to):
    """``(sh, sw, pad_h, pad_w)``: the size an (H, W) image is resized to at
    ``scale`` and the right/bottom padding up to a multiple of ``pad_to``."""
    # cap absurdly large upscales (reference evaluate.py:94-96)
    if scale * H > 2600 or scale * W > 3800:
        scale = min(2600 / H, 3800 / W)
    sh, sw = max(int(round(H * scale)), 1), max(int(round(W * scale)), 1)
    return sh, sw, (pad_to - sh % pad_to) % pad_to, (pad_to - sw % pad_to) % pad_to


# --------------------------------------------------------------------------
# predict: multi-scale / rotation / flip ensemble forward, many images per
# forward, fused ensemble merge
# --------------------------------------------------------------------------

def _output_channels(config: CanonicalConfig):
    """``(chan_order, flip_perm)``: where the ``[heat | paf]`` output channels
    sit in the network's ``[paf | heat]`` output, and the L/R permutation of the
    mirrored view in that output order."""
    n_heat = config.num_layers - config.paf_layers
    n_paf = config.paf_layers
    chan_order = list(range(n_paf, n_paf + n_heat)) + list(range(n_paf))
    flip_perm = [int(c) for c in config.flip_heat_ord] + \
        [n_heat + int(c) for c in config.flip_paf_ord]
    return chan_order, flip_perm


@torch.no_grad()
def _predict_groups(images, model, config, params, model_params, max_views,
                    device=None, dtype=None):
    """Ensemble forward of a list of images (reference evaluate.py:83-161).
    Returns ``[(indices, maps)]``, one entry per distinct image size: ``maps``
    is the planar fp32 (n, heat + paf, H, W) average of the images ``indices``
    in that order."""
    params, model_params = _resolve_params(params, model_params)
    if device is None:
        device = next(model.parameters()).device
    if dtype is None:
        dtype = next(model.parameters()).dtype
    if max_views < 2:
        raise ValueError("max_views must allow an image and its mirror (>= 2)")
    chunk = max_views // 2

    chan_order, flip_perm = _output_channels(config)
    rotations = params.get("rotation_search", [0.0])
    pad_to = model_params["max_downsample"]
    pad_value = model_params["padValue"] / 255.0

    by_size = {}
    for i, image in enumerate(images):
        img = _to_device_image(image, device)
        by_size.setdefault((img.shape[0], img.shape[1]), []).append((i, img))

    groups = []
    for (H, W), members in by_size.items():
        idxs = [i for i, _ in members]
        imgs = torch.stack([t for _, t in members]).permute(0, 3, 1, 2)  # NCHW
        n = len(idxs)
        maps = torch.empty(n, len(chan_order), H, W, device=device,
                           dtype=torch.float32)
        multiplier = [s * model_params["boxsize"] / H
                      for s in params["scale_search"]]
        n_runs = len(multiplier) * len(rotations)
        first = True
        for scale in multiplier:
            sh, sw, pad_h, pad_w = _scaled_geometry(H, W, scale, pad_to)
            scaled = F.interpolate(imgs, size=(sh, sw), mode="bicubic",
                                   align_corners=False)
            padded0 = F.pad(scaled, (0, pad_w, 0, pad_h), value=pad_value)
            ph, pw = padded0.shape[2], padded0.shape[3]
            for angle in rotations:
                padded = _rotate_nchw(padded0, angle)
                flipped = torch.flip(padded, dims=[3])
                for lo in range(0, n, chunk):
                    hi = min(lo + chunk, n)
                    batch = torch.cat([padded[lo:hi], flipped[lo:hi]]) \
                        .permute(0, 2, 3, 1).contiguous().to(dtype)   # NHWC
                    out = model(batch)[-1][0]            # last stack, scale 0
                    stride = ph // out.shape[2]
                    assert out.shape[2] * stride == ph and \
                        out.shape[3] * stride == pw, "non-integer output stride"
                    if angle == 0:
                        ensemble_merge(out, flip_perm, stride, (sh, sw), (H, W),
                                       scale=1.0 / n_runs, out=maps[lo:hi],
                                       accumulate=not first,
                                       chan_order=chan_order)
                        continue
                    # rotated runs keep the torch chain, batched along N
                    v = out.float()[:, chan_order]
                    merged = (v[:hi - lo] +
                              torch.flip(v[hi - lo:], dims=[-1])[:, flip_perm]) * 0.5
                    up = F.interpolate(merged, size=(ph, pw), mode="bicubic",
                                       align_corners=False)
                    up = _rotate_nchw(up, angle, inverse=True)[:, :, :sh, :sw]
                    up = F.interpolate(up, size=(H, W), mode="bicubic",
                                       align_corners=False) / n_runs
                    if first:
                        maps[lo:hi] = up
                    else:
                        maps[lo:hi] += up
                first = False
        groups.append((idxs, maps))
    return groups


def predict_batch(images, model, config: CanonicalConfig, params=None,
                  model_params=None, max_views=16, device=None, dtype=None):
    """Run the ensemble forward over a list of (H, W, 3) images.

    Images are grouped by size; per scale and rotation each group goes through
    the model as ``[views | mirrored views]`` in chunks of at most ``max_views``
    views, and rotation-free runs are merged by the fused ``ensemble_merge``
    kernel. Returns one ``(heatmap_avg, paf_avg)`` per image in input order:
    (H, W, C) fp32 views, at the ORIGINAL image resolution, of the group's
    planar buffer on ``device`` (stays on GPU when one is used).
    """
    n_heat = config.num_layers - config.paf_layers
    results = [None] * len(images)
    for idxs, maps in _predict_groups(images, model, config, params,
                                      model_params, max_views, device, dtype):
        for j, i in enumerate(idxs):
            results[i] = (maps[j, :n_heat].permute(1, 2, 0),
                          maps[j, n_heat:].permute(1, 2, 0))
    return results


def predict(image, model, config: CanonicalConfig, params=None, model_params=None,
            device=None, dtype=None):
    """``predict_batch`` for one image: ``(heatmap_avg, paf_avg)`` as (H, W, C)
    fp32 tensors on ``device``. The two are views of one planar
    (heat + paf, H, W) buffer, not separately allocated tensors."""
    return predict_batch([image], model, config, params, model_params,
                         device=device, dtype=dtype)[0]


# --------------------------------------------------------------------------
# find_peaks
# --------------------------------------------------------------------------

def _rows_to_peaks(rows, n_parts):
    """(c, x, y, score, peak) rows in (c, y, x) order -> ``all_peaks``."""
    all_peaks = [[] for _ in range(n_parts)]
    for gid, row in enumerate(rows):
        c = int(row[0])
        all_peaks[c].append((float(row[1]), float(row[2]), float(row[3]), gid))
    return all_peaks


def find_peaks_batch(maps, params, config: CanonicalConfig, max_peaks=512):
    """NMS + sub-pixel refinement over the 18 keypoint channels (reference
    evaluate.py:169-203) of every image of a planar (N, planes, H, W) buffer
    whose first ``heat_layers`` planes are the keypoint maps: one kernel launch
    and one device->host copy for the batch.

    Returns one ``all_peaks`` per image, the reference's structure: a list of
    ``heat_layers`` lists of ``(x, y, score, id)`` tuples, ids per image.
    """
    n_parts = config.heat_layers  # 18 keypoint channels (bkg excluded)
    radius = int(params["offset_radius"])
    thre1 = float(params["thre1"])
    maps = maps.contiguous().float()
    out = []
    if use_hip_for(maps):
        buf = hip_extension().peaks_batched(maps, n_parts, thre1, radius,
                                            max_peaks).cpu().numpy()
        counts = np.ascontiguousarray(buf[:, 0, 0]).view(np.int32)
        for n in range(buf.shape[0]):
            rows = buf[n, 1:1 + min(int(counts[n]), max_peaks)]
            # atomics make device order nondeterministic: impose (c, y, x) order
            rows = rows[np.lexsort((rows[:, 1], rows[:, 2], rows[:, 0]))]
            out.append(_rows_to_peaks(rows, n_parts))
        return out
    heat = maps[:, :n_parts]
    nmsed = keypoint_heatmap_nms(heat, kernel=3, thre=thre1).cpu().numpy()
    heat_np = heat.cpu().numpy()
    for n in range(heat_np.shape[0]):
        rows = []
        for c in range(n_parts):
            ys, xs = np.nonzero(nmsed[n, c])
            for y, x in zip(ys, xs):
                xr, yr, sc = refine_centroid(heat_np[n, c], (int(x), int(y)), radius)
                rows.append((c, xr, yr, sc, heat_np[n, c, y, x]))
        rows = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
        out.append(_rows_to_peaks(rows, n_parts))
    return out


def find_peaks(heatmap_avg, params, config: CanonicalConfig, max_peaks=512):
    """``find_peaks_batch`` for one (H, W, C) torch map."""
    heat = heatmap_avg[..., :config.heat_layers].permute(2, 0, 1)[None]
    return find_peaks_batch(heat, params, config, max_peaks)[0]


# --------------------------------------------------------------------------
# find_connections
# --------------------------------------------------------------------------

def _limb_scores_host(paf_np, pa, pb, mid_num, thre2):
    """CPU scoring of one candidate segment (same math as limb_score_kernel).
    Short limbs sample fewer points (reference evaluate.py:228)."""
    H, W = paf_np.shape
    ax, ay, bx, by = pa[0], pa[1], pb[0], pb[1]
    norm = math.hypot(bx - ax, by - ay) + 1e-9
    mn = min(int(round(norm)) + 1, mid_num)
    xs = np.round(np.linspace(ax, bx, mn)).astype(int).clip(0, W - 1)
    ys = np.round(np.linspace(ay, by, mn)).astype(int).clip(0, H - 1)
    v = paf_np[ys, xs]
    mean = float(v.mean()) + min(0.5 * H / norm - 1.0, 0.0)
    return mean, float((v > thre2).mean()), float(norm)


def _candidate_triples(all_peaks, limbs):
    """Every (limb, peakA id, peakB id) candidate and its (limb, i, j) position."""
    cand_triples = []
    pair_meta = []  # (k, i, j)
    for k, (a_part, b_part) in enumerate(limbs):
        for i, pa in enumerate(all_peaks[a_part]):
            for j, pb in enumerate(all_peaks[b_part]):
                cand_triples.append((k, pa[3], pb[3]))
                pair_meta.append((k, i, j))
    return cand_triples, pair_meta


def _greedy_match(all_peaks, scores, pair_meta, params, config: CanonicalConfig):
    """Greedy 1-1 matching per limb type over scored candidates (the host half
    of ``find_connections``). ``scores[i]`` = (prior score, pass ratio, length)
    of candidate ``pair_meta[i]`` = (limb, i, j), grouped by limb in order."""
    connect_ration = float(params["connect_ration"])
    limbs = config.limbs_conn
    connection_all, special_k = [], []
    ptr = 0
    counts = {}
    for k, i, j in pair_meta:
        counts[k] = counts.get(k, 0) + 1
    for k, (a_part, b_part) in enumerate(limbs):
        nA, nB = len(all_peaks[a_part]), len(all_peaks[b_part])
        if nA == 0 or nB == 0:
            special_k.append(k)
            connection_all.append([])
            continue
        n_k = counts.get(k, 0)
        block = scores[ptr:ptr + n_k]
        meta = pair_meta[ptr:ptr + n_k]
        ptr += n_k

        candidates = []
        for (kk, i, j), (s_prior, pass_ratio, length) in zip(meta, block):
            pa = all_peaks[a_part][i]
            pb = all_peaks[b_part][j]
            # coincident peaks of two part types form a zero-length segment;
            # the reference rejects them outright (evaluate.py:229 norm == 0)
            if length < 1e-6:
                continue
            # criterion1: enough samples above thre2; criterion2: positive score
            if pass_ratio >= connect_ration and s_prior > 0:
                combined = 0.5 * s_prior + 0.25 * pa[2] + 0.25 * pb[2]
                candidates.append((i, j, float(s_prior), float(length), combined))
        candidates.sort(key=lambda c: c[4], reverse=True)

        used_i, used_j = set(), set()
        conn = []
        for i, j, s, length, _ in candidates:
            if i in used_i or j in used_j:
                continue
            conn.append([all_peaks[a_part][i][3], all_peaks[b_part][j][3],
                         s, i, j, length])
            used_i.add(i)
            used_j.add(j)
            if len(conn) >= min(nA, nB):
                break
        connection_all.append(np.asarray(conn, dtype=np.float64).reshape(-1, 6))
    return connection_all, special_k


def find_connections_batch(all_peaks_list, maps, params, config: CanonicalConfig,
                           first_limb_plane=None):
    """Score + greedily match candidate limbs (reference evaluate.py:206-276)
    for every image of a planar (N, planes, H, W) buffer whose limb maps start
    at plane ``first_limb_plane``: the heat count of a pipeline buffer by
    default, 0 for bare PAF maps. Every image's (limb_type, peakA, peakB)
    triples are scored in one kernel launch with one copy back; the greedy 1-1
    matching per limb type runs per image on the host.

    Returns one ``(connection_all, special_k)`` per image in the reference's
    format: per limb type either an (n, 6) array
    ``[idA, idB, score, i, j, length]`` or an empty list.
    """
    if first_limb_plane is None:
        first_limb_plane = config.num_layers - config.paf_layers
    mid_num = int(params["mid_num"])
    thre2 = float(params["thre2"])
    maps = maps.contiguous().float()
    planes = maps.shape[1]
    cands, metas, flat_peaks = [], [], []
    for n, all_peaks in enumerate(all_peaks_list):
        triples, meta = _candidate_triples(all_peaks, config.limbs_conn)
        base = len(flat_peaks)
        flat_peaks.extend(sorted((p for sub in all_peaks for p in sub),
                                 key=lambda p: p[3]))
        # scoring picks its plane by the first field: this image's limb k
        cands.extend((n * planes + first_limb_plane + k, base + ia, base + ib)
                     for k, ia, ib in triples)
        metas.append(meta)
    scores = np.zeros((0, 3), dtype=np.float32)
    if cands and use_hip_for(maps):
        peaks_dev = torch.tensor([[0.0, p[0], p[1], p[2], 0.0] for p in flat_peaks],
                                 dtype=torch.float32, device=maps.device)
        cand_dev = torch.tensor(cands, dtype=torch.int32, device=maps.device)
        scores = hip_extension().limb_scores(maps, peaks_dev, cand_dev, mid_num,
                                             thre2).cpu().numpy()
    elif cands:
        planes_np = maps.cpu().numpy().reshape(-1, maps.shape[2], maps.shape[3])
        scores = np.array([
            _limb_scores_host(planes_np[plane], flat_peaks[ia], flat_peaks[ib],
                              mid_num, thre2)
            for (plane, ia, ib) in cands], dtype=np.float32)
    out, ptr = [], 0
    for all_peaks, meta in zip(all_peaks_list, metas):
        out.append(_greedy_match(all_peaks, scores[ptr:ptr + len(meta)], meta,
                                 params, config))
        ptr += len(meta)
    return out


def find_connections(all_peaks, paf_avg, image_height, params, config: CanonicalConfig):
    """``find_connections_batch`` for one (H, W, paf_layers) torch map."""
    return find_connections_batch([all_peaks], paf_avg.permute(2, 0, 1)[None],
                                  params, config, first_limb_plane=0)[0]


# --------------------------------------------------------------------------
# assign_batch: peaks -> connections on the device, one host synchronisation
# --------------------------------------------------------------------------

def _assign_host(maps, params, config, max_peaks=512):
    """The host-matching path in ``assign_batch``'s return format."""
    peaks = find_peaks_batch(maps, params, config, max_peaks)
    conns = find_connections_batch(peaks, maps, params, config)
    return [(pk, c, sk) for pk, (c, sk) in zip(peaks, conns)]


def assign_batch(maps, params, config: CanonicalConfig, max_peaks=512,
                 max_part=64):
    """``find_peaks_batch`` + ``find_connections_batch`` of a planar
    (N, heat + paf, H, W) pipeline buffer with the matching on the device:
    ``peaks_batched`` -> ``peaks_canonical`` -> ``limb_match`` are queued
    without a host synchronisation in between, one copy brings peaks, offsets,
    connection rows and counts back, and numpy decodes them.

    Returns one ``(all_peaks, connection_all, special_k)`` per image. An image
    in which a part has more than ``max_part`` (<= 64) peaks is redone through
    the host path, so results are never truncated. On CPU maps the host path
    runs for every image.
    """
    n_parts = config.heat_layers
    first_limb_plane = config.num_layers - config.paf_layers
    maps = maps.contiguous().float()
    if not use_hip_for(maps):
        return _assign_host(maps, params, config, max_peaks)
    if max_peaks > MAX_PEAKS:
        raise ValueError(f"device matching ranks at most {MAX_PEAKS} peaks per "
                         f"image (max_peaks={max_peaks})")
    N = maps.shape[0]
    if N == 0:
        return []
    buf = hip_extension().peaks_batched(maps, n_parts, float(params["thre1"]),
                                        int(params["offset_radius"]), max_peaks)
    peaks, offsets = canonical_peaks(buf, n_parts)
    rows, counts = limb_match(maps, peaks, offsets, config.limbs_conn,
                              first_limb_plane, int(params["mid_num"]),
                              float(params["thre2"]),
                              float(params["connect_ration"]), max_part)
    # one copy, one synchronisation: the int32 tensors travel as fp32 bits
    parts = (peaks, offsets.view(torch.float32), rows, counts.view(torch.float32))
    flat = torch.cat([t.reshape(-1) for t in parts]).cpu().numpy()
    host, lo = [], 0
    for t in parts:
        host.append(flat[lo:lo + t.numel()].reshape(t.shape))
        lo += t.numel()
    counts_np = host[3].view(np.int32)
    out = decode_assignment(host[0], host[1].view(np.int32), host[2], counts_np)
    for n in np.nonzero((counts_np == OVERFLOW).any(axis=1))[0]:
        out[n] = _assign_host(maps[n:n + 1], params, config, max_peaks)[0]
    return out


# --------------------------------------------------------------------------
# find_people: greedy subset assembly (host — tiny)
# --------------------------------------------------------------------------

def find_people(connection_all, special_k, all_peaks, params, config: CanonicalConfig,
                stats=None):
    """Greedy person assembly (reference evaluate.py:279-498).

    subset rows are (n_slots, 2): slot ``[part] = (candidate_id, confidence)``,
    ``[-2] = (total_score, _)``, ``[-1] = (n_parts, longest_limb)``.
    Semantics preserved from the reference: assign-if-empty (with length
    prior), overwrite-if-better, merge-disjoint-subsets (confidence-gated),
    two-person competition resolution, new-person creation, and final pruning
    (< 2 parts or mean score < 0.45). A dict passed as ``stats`` receives
    ``max_live``, the most subset rows alive at once (the capacity the device
    assembly needs), and ``branches``, how often each branch decided.
    """
    len_rate = float(params["len_rate"])
    connection_tole = float(params["connection_tole"])
    remove_recon = int(params.get("remove_recon", 0))
    n_slots = config.heat_layers + 2  # 18 parts + count + score rows = 20

    subset = -1 * np.ones((0, n_slots, 2))
    count = stats is not None        # bookkeeping only when it is asked for
    max_live = 0
    branches = collections.Counter()
    candidate = np.array([p for sub in all_peaks for p in sub], dtype=np.float64) \
        .reshape(-1, 4)

    for k, (index_a, index_b) in enumerate(config.limbs_conn):
        if k in special_k:
            continue
        conns = connection_all[k]
        part_as = conns[:, 0]
        part_bs = conns[:, 1]

        for i in range(len(conns)):
            score_i = conns[i][2]
            length_i = conns[i][-1]
            found = 0
            subset_idx = [-1, -1]
            for j in range(len(subset)):
                if int(subset[j][index_a][0]) == int(part_as[i]) or \
                        int(subset[j][index_b][0]) == int(part_bs[i]):
                    if found >= 2:
                        continue
                    subset_idx[found] = j
                    found += 1

            if found == 1:
                j = subset_idx[0]
                if int(subset[j][index_b][0]) == -1 and \
                        len_rate * subset[j][-1][1] > length_i:
                    # B slot empty and limb not absurdly longer than what this
                    # person already has: assign
                    if count:
                        branches["assign"] += 1
                    subset[j][index_b] = [part_bs[i], score_i]
                    subset[j][-1][0] += 1
                    subset[j][-1][1] = max(length_i, subset[j][-1][1])
                    subset[j][-2][0] += candidate[int(part_bs[i]), 2] + score_i
                elif int(subset[j][index_b][0]) != int(part_bs[i]):
                    if subset[j][index_b][1] >= score_i:
                        # existing connection is more confident
                        if count:
                            branches["keep"] += 1
                    else:
                        if len_rate * subset[j][-1][1] <= length_i:
                            if count:
                                branches["too_long"] += 1
                            continue
                        # replace: subtract the old point + limb confidence
                        if count:
                            branches["overwrite"] += 1
                        subset[j][-2][0] -= candidate[int(subset[j][index_b][0]), 2] \
                            + subset[j][index_b][1]
                        subset[j][index_b] = [part_bs[i], score_i]
                        subset[j][-2][0] += candidate[int(part_bs[i]), 2] + score_i
                        subset[j][-1][1] = max(length_i, subset[j][-1][1])
                elif int(subset[j][index_b][0]) == int(part_bs[i]) and \
                        subset[j][index_b][1] <= score_i:
                    # redundant connection reaching the same keypoint with a
                    # better score: refresh the stored confidence
                    if count:
                        branches["refresh"] += 1
                    subset[j][-2][0] -= candidate[int(subset[j][index_b][0]), 2] \
                        + subset[j][index_b][1]
                    subset[j][index_b] = [part_bs[i], score_i]
                    subset[j][-2][0] += candidate[int(part_bs[i]), 2] + score_i
                    subset[j][-1][1] = max(length_i, subset[j][-1][1])

            elif found == 2:
                j1, j2 = subset_idx
                membership1 = (subset[j1][..., 0] >= 0).astype(int)[:-2]
                membership2 = (subset[j2][..., 0] >= 0).astype(int)[:-2]
                if not np.any(membership1 + membership2 == 2):
                    # disjoint -> merge, but only if this limb is trustworthy
                    min_limb1 = np.min(subset[j1, :-2, 1][membership1 == 1])
                    min_limb2 = np.min(subset[j2, :-2, 1][membership2 == 1])
                    min_tolerance = min(min_limb1, min_limb2)
                    if score_i < connection_tole * min_tolerance or \
                            len_rate * subset[j1][-1][1] <= length_i:
                        if count:
                            branches["merge_refused"] += 1
                        continue
                    if count:
                        branches["merge"] += 1
                    subset[j1][:-2] += subset[j2][:-2] + 1
                    subset[j1][-2:][:, 0] += subset[j2][-2:][:, 0]
                    subset[j1][-2][0] += score_i
                    subset[j1][-1][1] = max(length_i, subset[j1][-1][1])
                    subset = np.delete(subset, j2, 0)
                else:
                    # two different people compete for this limb
                    if conns[i][0] in subset[j1, :-2, 0]:
                        c1 = np.where(subset[j1, :-2, 0] == conns[i][0])
                        c2 = np.where(subset[j2, :-2, 0] == conns[i][1])
                    else:
                        c1 = np.where(subset[j1, :-2, 0] == conns[i][1])
                        c2 = np.where(subset[j2, :-2, 0] == conns[i][0])
                    if len(c1[0]) == 0 or len(c2[0]) == 0:
                        continue
                    c1, c2 = int(c1[0][0]), int(c2[0][0])
                    if score_i < subset[j1][c1][1] and score_i < subset[j2][c2][1]:
                        if count:
                            branches["compete_skip"] += 1
                        continue
                    if count:
                        branches["compete"] += 1
                    small_j, remove_c = (j1, c1)
                    if subset[j1][c1][1] > subset[j2][c2][1]:
                        small_j, remove_c = (j2, c2)
                    if remove_recon > 0:
                        subset[small_j][-2][0] -= \
                            candidate[int(subset[small_j][remove_c][0]), 2] + \
                            subset[small_j][remove_c][1]
                        subset[small_j][remove_c] = [-1, -1]
                        subset[small_j][-1][0] -= 1

            elif found == 0:
                row = -1 * np.ones((n_slots, 2))
                row[index_a] = [part_as[i], score_i]
                row[index_b] = [part_bs[i], score_i]
                row[-1] = [2, length_i]
                row[-2][0] = candidate[int(part_as[i]), 2] + \
                    candidate[int(part_bs[i]), 2] + score_i
                subset = np.concatenate((subset, row[None]), axis=0)
                if count:
                    max_live = max(max_live, len(subset))
                    branches["new"] += 1

    # prune: fewer than 2 parts, or mean per-part score below 0.45
    keep = [i for i in range(len(subset))
            if subset[i][-1][0] >= 2 and
            subset[i][-2][0] / subset[i][-1][0] >= 0.45]
    if count:
        stats["max_live"] = max_live
        stats["branches"] = dict(branches)
    return subset[keep], candidate


# --------------------------------------------------------------------------
# process / validation / demo glue
# --------------------------------------------------------------------------

def subsets_to_keypoints(subset, candidate, config: CanonicalConfig):
    """Convert assembled subsets to COCO-17 keypoint rows
    (reference evaluate.py:522-542)."""
    keypoints = []
    for s in subset:
        ids = s[:config.heat_layers, 0]
        internal = []
        for index in ids:
            if index == -1:
                internal.append((0.0, 0.0))
            else:
                internal.append(tuple(candidate[int(index)][:2]))
        coco = [None] * 17
        for dt_index, gt_index in config.dt_gt_mapping.items():
            if gt_index is None:
                continue
            coco[gt_index] = internal[dt_index]
        keypoints.append((coco, 1 - 1.0 / s[-2][0] if s[-2][0] > 0 else 0.0))
    return keypoints


def _check_modes(matching, assembly):
    if matching not in ("host", "device"):
        raise ValueError(f"matching must be 'host' or 'device', got {matching!r}")
    if assembly not in ("host", "device"):
        raise ValueError(f"assembly must be 'host' or 'device', got {assembly!r}")
    if assembly == "device" and matching != "device":
        raise ValueError("assembly='device' consumes the connection rows of "
                         "matching='device'")


def _people_host(assigned, params, config):
    """``find_people`` + ``subsets_to_keypoints`` per assigned image."""
    out = []
    for all_peaks, connection_all, special_k in assigned:
        subset, candidate = find_people(connection_all, special_k, all_peaks,
                                        params, config)
        out.append(subsets_to_keypoints(subset, candidate, config))
    return out


def people_batch(maps, params, config: CanonicalConfig, max_peaks=512,
                 max_part=64, max_people=128, assembly="device"):
    """Peaks, limb matching and person assembly of a planar
    (N, heat + paf, H, W) pipeline buffer: one list of (coco_keypoints, score)
    per image. With ``assembly="device"`` on a GPU, ``peaks_batched`` ->
    ``peaks_canonical`` -> ``limb_match`` -> ``people_assemble`` are queued
    without a host synchronisation in between, and one copy brings back the
    people counts, the COCO coordinates and the summed scores of finished
    people only. An image the kernels flag as overflowed (a part with more than
    ``max_part`` peaks, or more than ``max_people`` subset rows alive at once)
    is redone through the host path, so results are never truncated. On CPU
    maps, or with ``assembly="host"``, this is ``assign_batch`` followed by the
    host ``find_people``."""
    if assembly not in ("host", "device"):
        raise ValueError(f"assembly must be 'host' or 'device', got {assembly!r}")
    maps = maps.contiguous().float()
    if assembly == "host" or not use_hip_for(maps):
        return _people_host(assign_batch(maps, params, config, max_peaks, max_part),
                            params, config)
    if max_peaks > MAX_PEAKS:
        raise ValueError(f"device matching ranks at most {MAX_PEAKS} peaks per "
                         f"image (max_peaks={max_peaks})")
    n_parts = config.heat_layers
    N = maps.shape[0]
    if N == 0:
        return []
    buf = hip_extension().peaks_batched(maps, n_parts, float(params["thre1"]),
                                        int(params["offset_radius"]), max_peaks)
    peaks, offsets = canonical_peaks(buf, n_parts)
    rows, counts = limb_match(maps, peaks, offsets, config.limbs_conn,
                              config.num_layers - config.paf_layers,
                              int(params["mid_num"]), float(params["thre2"]),
                              float(params["connect_ration"]), max_part)
    n_people, subset, keypoints = assemble_people(
        peaks, offsets, rows, counts, config.limbs_conn, config.dt_gt_mapping,
        float(params["len_rate"]), float(params["connection_tole"]),
        int(params.get("remove_recon", 0)), max_people)
    # one copy, one synchronisation: int32 and fp64 travel as fp32 bits
    totals = subset[:, :, n_parts, 0].contiguous()
    parts = (n_people.view(torch.float32), keypoints, totals.view(torch.float32))
    flat = torch.cat([t.reshape(-1) for t in parts]).cpu().numpy()
    host, lo = [], 0
    for t in parts:
        host.append(flat[lo:lo + t.numel()].reshape(t.shape))
        lo += t.numel()
    out = decode_people(host[0].view(np.int32), host[1],
                        host[2].view(np.float64), config.dt_gt_mapping)
    for n in (n for n, people in enumerate(out) if people is None):
        out[n] = _people_host(_assign_host(maps[n:n + 1], params, config,
                                           max_peaks), params, config)[0]
    return out


@torch.no_grad()
def process_batch(images, model, config: CanonicalConfig, params=None,
                  model_params=None, max_views=16, matching="host",
                  assembly="host"):
    """Full pipeline for a list of images (reference evaluate.py:500-542):
    batched forward and ensemble merge, batched peak and limb kernels, then the
    per-image greedy assembly. ``matching="host"`` scores limb candidates on
    the device and matches them on the host; ``"device"`` does both in
    ``assign_batch``. ``assembly="device"`` (with ``matching="device"``) also
    assembles the people on the device (``people_batch``), so only finished
    people come back. Returns one list of (coco_keypoints, score) per image, in
    input order."""
    _check_modes(matching, assembly)
    params, model_params = _resolve_params(params, model_params)
    results = [None] * len(images)
    for idxs, maps in _predict_groups(images, model, config, params,
                                      model_params, max_views):
        if assembly == "device":
            people = people_batch(maps, params, config)
        else:
            assign = assign_batch if matching == "device" else _assign_host
            people = _people_host(assign(maps, params, config), params, config)
        for i, found in zip(idxs, people):
            results[i] = found
    return results


def process(image, model, config: CanonicalConfig, params=None, model_params=None,
            matching="host", assembly="host"):
    """``process_batch`` for one image -> list of (coco_keypoints, score)."""
    return process_batch([image], model, config, params, model_params,
                         matching=matching, assembly=assembly)[0]


def format_results(keypoints, res_file):
    """COCO results JSON (reference evaluate.py:563-582)."""
    out = []
    for image_id, people in keypoints.items():
        for keypoint_list, score in people:
            flat = []
            for pt in keypoint_list:
                x, y = (0.0, 0.0) if pt is None else pt
                flat.extend([float(x), float(y), 1 if (x > 0 or y > 0) else 0])
            out.append({"image_id": image_id, "category_id": 1,
                        "keypoints": flat, "score": float(score)})
    os.makedirs(os.path.dirname(res_file) or ".", exist_ok=True)
    with open(res_file, "w") as f:
        json.dump(out, f)
    return out


def validation(model, config: CanonicalConfig, ann_file, images_directory,
               dump_name, validation_ids=None, params=None, model_params=None):
    """COCO keypoint evaluation over validation images
    (reference evaluate.py:585-622). Requires pycocotools + an image reader —
    both absent in this offline build image, so this raises a clear error
    there and runs where they exist."""
    try:
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except ImportError as e:  # pragma: no cover
        raise RuntimeError("validation() requires pycocotools") from e

    coco_gt = COCO(ann_file)
    if validation_ids is None:
        validation_ids = coco_gt.getImgIds()[:500]
    keypoints = {}
    for image_id in validation_ids:
        name = coco_gt.imgs[image_id]["file_name"]
        img = _read_image(os.path.join(images_directory, name))
        keypoints[image_id] = process(img, model, config, params, model_params)
    res_file = f"results/{dump_name}_results.json"
    format_results(keypoints, res_file)
    coco_dt = coco_gt.loadRes(res_file)
    coco_eval = COCOeval(coco_gt, coco_dt, "keypoints")
    coco_eval.params.imgIds = validation_ids
    coco_eval.evaluate()
    coco_eval.accumulate()
    coco_eval.summarize()
    return coco_eval


def _read_image(path):  # pragma: no cover - needs image files
    """BGR uint8 (H, W, 3), matching the reference's cv2.imread convention."""
    try:
        import cv2
        return cv2.imread(path)
    except ImportError:
        from PIL import Image
        return np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1]
