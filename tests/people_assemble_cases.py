"""Hand-made inputs for the person-assembly tests (CPU and GPU): the
``(peaks, offsets, rows, counts)`` arrays of ``canonical_peaks`` / ``limb_match``
built from small connection graphs, the host oracle (``find_people`` on
``decode_assignment`` of the same arrays) and one directed graph per branch of
``find_people``. Every value is fp32-representable, so the oracle and a kernel
see the same numbers.

Canonical limbs used below (index: partA -> partB): 0: 1->0, 1: 1->14,
5: 0->14, 9: 1->2, 12: 1->5, 13: 5->6, 14: 6->7, 21: 0->2, 22: 0->5.
"""
import numpy as np

from improved_body_parts_amd.engine import find_people, subsets_to_keypoints
from improved_body_parts_amd.ops.assignment import (NO_PEAKS, OVERFLOW,
                                                    decode_assignment)

f32 = lambda v: float(np.float32(v))


def make_peaks(config, points):
    """{part: [(x, y, score), ...]} -> ``all_peaks`` with ids in row order."""
    all_peaks, gid = [], 0
    for c in range(config.heat_layers):
        sub = []
        for x, y, s in points.get(c, []):
            sub.append((f32(x), f32(y), f32(s), gid))
            gid += 1
        all_peaks.append(sub)
    return all_peaks


def graph(config, n_per_part, conns, score=0.75):
    """A graph from peak counts per part and connections
    ``(limb, i, j, score, length)`` between the i-th peak of the limb's part A
    and the j-th of its part B, in the order given. Peak (part, i) sits at
    ``(8 part + 1, 8 i + 2)``; ``score`` is one value for all peaks or
    ``{(part, i): value}`` over a default of 0.75."""
    per_peak = score if isinstance(score, dict) else {}
    base = 0.75 if isinstance(score, dict) else score
    all_peaks = make_peaks(config, {
        c: [(8.0 * c + 1, 8.0 * i + 2, per_peak.get((c, i), base))
            for i in range(n)] for c, n in n_per_part.items()})
    rows = {}
    for k, i, j, s, length in conns:
        a, b = config.limbs_conn[k]
        rows.setdefault(k, []).append(
            [all_peaks[a][i][3], all_peaks[b][j][3], f32(s), i, j, f32(length)])
    return all_peaks, rows


def encode(config, graphs, max_peaks=64, max_part=8, overflow=()):
    """Graphs -> numpy ``(peaks, offsets, rows, counts)`` in the layouts of
    ``canonical_peaks`` / ``limb_match``. A limb with an empty part gets
    ``NO_PEAKS``; ``overflow`` lists (image, limb) counts to set to
    ``OVERFLOW``. Rows past a limb's count hold garbage."""
    N, C, L = len(graphs), config.heat_layers, len(config.limbs_conn)
    peaks = np.zeros((N, max_peaks, 5), dtype=np.float32)
    offsets = np.zeros((N, C + 1), dtype=np.int32)
    rows = np.full((N, L, max_part, 6), 9999.0, dtype=np.float32)
    counts = np.zeros((N, L), dtype=np.int32)
    for n, (all_peaks, conns) in enumerate(graphs):
        r = 0
        for c, sub in enumerate(all_peaks):
            offsets[n, c] = r
            for pk in sub:
                assert pk[3] == r
                peaks[n, r] = [c, pk[0], pk[1], pk[2], 0.0]
                r += 1
        offsets[n, C] = r
        assert r <= max_peaks
        for k, (a, b) in enumerate(config.limbs_conn):
            if not all_peaks[a] or not all_peaks[b]:
                assert k not in conns
                counts[n, k] = NO_PEAKS
                continue
            rk = np.asarray(conns.get(k, []), dtype=np.float32).reshape(-1, 6)
            assert len(rk) <= max_part
            counts[n, k] = len(rk)
            rows[n, k, :len(rk)] = rk
    for n, k in overflow:
        counts[n, k] = OVERFLOW
    return peaks, offsets, rows, counts


def oracle(config, params, arrays):
    """The host result per image of ``arrays``: ``(subset, keypoints, stats)``
    from ``find_people`` / ``subsets_to_keypoints`` on ``decode_assignment``;
    ``None`` for an image with an overflowed limb."""
    out = []
    for all_peaks, conn, special_k in decode_assignment(*arrays):
        if any(c is None for c in conn):
            out.append(None)
            continue
        stats = {}
        subset, cand = find_people(conn, special_k, all_peaks, params, config,
                                   stats=stats)
        out.append((subset, subsets_to_keypoints(subset, cand, config), stats))
    return out


def keypoint_array(people):
    """(coco_keypoints, score) list -> fp32 (n, 17, 2), (0, 0) for ``None``."""
    return np.asarray([[(0.0, 0.0) if pt is None else pt for pt in coco]
                       for coco, _ in people], dtype=np.float32).reshape(-1, 17, 2)


# --------------------------------------------------------------------------
# one graph per branch
# --------------------------------------------------------------------------

TINY = f32(1e-12)     # TINY + 1.0 rounds in fp64: its low bits sit below 2^-52

# two necks, noses and right eyes; limb 5 crosses nose 0 to eye 1
_RIVALS = {1: 2, 0: 2, 14: 2}


def _rivals(conf_nose0, conf_eye1, cross):
    return (_RIVALS, [(0, 0, 0, conf_nose0, 5.0), (0, 1, 1, 0.8, 5.0),
                      (1, 0, 0, 0.8, 5.0), (1, 1, 1, conf_eye1, 5.0),
                      (5, 0, 1, cross, 5.0)])


# two halves {neck, nose} and {Lsho, Lelb, Lwri}, then nose -> Lsho
def _halves(join_score, join_len, elbow_conf=0.8):
    return ({1: 1, 0: 1, 5: 1, 6: 1, 7: 1},
            [(0, 0, 0, 0.8, 5.0), (13, 0, 0, elbow_conf, 5.0),
             (14, 0, 0, 0.8, 5.0), (22, 0, 0, join_score, join_len)])


# name -> (peaks per part, connections, remove_recon, branch counts of the
# oracle, people that survive)
DIRECTED = {
    "new": ({1: 1, 0: 1}, [(0, 0, 0, 0.8, 5.0)], 0, {"new": 1}, 1),
    "assign": ({1: 1, 0: 1, 14: 1},
               [(0, 0, 0, 0.8, 5.0), (1, 0, 0, 0.7, 6.0)], 0,
               {"new": 1, "assign": 1}, 1),
    # 16 * 5 = 80 <= 80: the length prior refuses
    "assign_too_long": ({1: 1, 0: 1, 14: 1},
                        [(0, 0, 0, 0.8, 5.0), (1, 0, 0, 0.7, 80.0)], 0,
                        {"new": 1, "too_long": 1}, 1),
    # neck -> Rsho 0 at 0.3, then nose -> Rsho 1 at 0.9 replaces it
    "overwrite": ({1: 1, 0: 1, 2: 2},
                  [(0, 0, 0, 0.8, 5.0), (9, 0, 0, 0.3, 5.0),
                   (21, 0, 1, 0.9, 7.0)], 0,
                  {"new": 1, "assign": 1, "overwrite": 1}, 1),
    "overwrite_too_long": ({1: 1, 0: 1, 2: 2},
                           [(0, 0, 0, 0.8, 5.0), (9, 0, 0, 0.3, 5.0),
                            (21, 0, 1, 0.9, 81.0)], 0,
                           {"new": 1, "assign": 1, "too_long": 1}, 1),
    "keep": ({1: 1, 0: 1, 2: 2},
             [(0, 0, 0, 0.8, 5.0), (9, 0, 0, 0.9, 5.0), (21, 0, 1, 0.3, 7.0)],
             0, {"new": 1, "assign": 1, "keep": 1}, 1),
    # the same Rsho again through the nose, with a better score
    "refresh": ({1: 1, 0: 1, 2: 1},
                [(0, 0, 0, 0.8, 5.0), (9, 0, 0, 0.3, 5.0), (21, 0, 0, 0.9, 7.0)],
                0, {"new": 1, "assign": 1, "refresh": 1}, 1),
    "merge": _halves(0.7, 6.0) + (0, {"new": 2, "assign": 1, "merge": 1}, 1),
    # 0.5 < 0.7 * 0.8
    "merge_low_score": _halves(0.5, 6.0) +
    (0, {"new": 2, "assign": 1, "merge_refused": 1}, 2),
    # 16 * 5 <= 80, score fine
    "merge_too_long": _halves(0.7, 80.0) +
    (0, {"new": 2, "assign": 1, "merge_refused": 1}, 2),
    "merge_tiny_conf": _halves(0.7, 6.0, elbow_conf=TINY) +
    (0, {"new": 2, "assign": 1, "merge": 1}, 1),
    # conf of nose 0 in person 0 is 0.3, of eye 1 in person 1 is 0.6
    "compete_keep_both": _rivals(0.3, 0.6, 0.5) +
    (0, {"new": 2, "assign": 2, "compete": 1}, 2),
    "compete_remove_first": _rivals(0.3, 0.6, 0.5) +
    (1, {"new": 2, "assign": 2, "compete": 1}, 2),
    "compete_remove_second": _rivals(0.6, 0.3, 0.5) +
    (1, {"new": 2, "assign": 2, "compete": 1}, 2),
    "compete_both_better": _rivals(0.6, 0.7, 0.5) +
    (1, {"new": 2, "assign": 2, "compete_skip": 1}, 2),
    # person 0 = {neck 0, nose 0} loses its nose to the competition: one part
    "prune_count": ({1: 2, 0: 2, 14: 1},
                    [(0, 0, 0, 0.3, 5.0), (0, 1, 1, 0.8, 5.0),
                     (1, 1, 0, 0.9, 5.0), (5, 0, 0, 0.5, 5.0)], 1,
                    {"new": 2, "assign": 1, "compete": 1}, 1),
    # (0.25 + 0.25 + 0.125) / 2 < 0.45 next to a person that stays
    "prune_mean": ({1: 2, 0: 2},
                   [(0, 0, 0, 0.125, 5.0), (0, 1, 1, 0.8, 5.0)], 0,
                   {"new": 2}, 1),
}
PRUNE_MEAN_SCORES = {(1, 0): 0.25, (0, 0): 0.25}


def directed_graph(config, name):
    n_per_part, conns = DIRECTED[name][:2]
    score = PRUNE_MEAN_SCORES if name == "prune_mean" else 0.75
    return graph(config, n_per_part, conns, score)


# --------------------------------------------------------------------------
# random connection graphs (the generator of test_find_people_invariants_fuzz,
# values rounded to fp32)
# --------------------------------------------------------------------------

def random_graph(config, rng, max_per_part, drop):
    n_per_part = rng.integers(0, max_per_part + 1, config.heat_layers)
    all_peaks = make_peaks(config, {
        part: [(rng.uniform(0, 127), rng.uniform(0, 127), rng.uniform(0.2, 1.0))
               for _ in range(n_per_part[part])]
        for part in range(config.heat_layers)})
    conns = {}
    for k, (a, b) in enumerate(config.limbs_conn):
        nA, nB = len(all_peaks[a]), len(all_peaks[b])
        if nA == 0 or nB == 0:
            continue
        rows = []
        used_i, used_j = set(), set()
        order = [(i, j) for i in range(nA) for j in range(nB)]
        rng.shuffle(order)
        for i, j in order:
            if i in used_i or j in used_j:
                continue
            if rng.random() < drop:
                continue
            used_i.add(i)
            used_j.add(j)
            rows.append([all_peaks[a][i][3], all_peaks[b][j][3],
                         f32(rng.uniform(0.1, 1.5)), i, j,
                         f32(rng.uniform(3, 120))])
        if rows:
            conns[k] = rows
    return all_peaks, conns


def check_invariants(config, subset):
    """The structural invariants of test_find_people_invariants_fuzz."""
    seen_ids = set()
    for s in subset:
        ids = [int(v) for v in s[:config.heat_layers, 0] if v >= 0]
        assert len(ids) == len(set(ids)), "duplicate part inside one person"
        for v in ids:
            assert v not in seen_ids, "candidate assigned to two people"
            seen_ids.add(v)
        assert s[-1][0] >= 2
        assert len(ids) == int(s[-1][0]), f"count {s[-1][0]} != assigned {len(ids)}"
