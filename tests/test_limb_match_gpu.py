"""Device-side limb matching (peaks_canonical + limb_match, assign_batch and
process_batch(matching="device")) against the existing GPU path:
find_peaks_batch + find_connections_batch, i.e. the limb_scores kernel plus the
host ``_greedy_match``. Connection rows are compared after ordering each limb
by its first peak id (see ``_by_peak_id`` in test_ensemble_merge_gpu.py)."""
import numpy as np
import pytest
import torch

from improved_body_parts_amd.config import GetConfig, InferenceParams, TrainingOpt
from improved_body_parts_amd.engine import (
    assign_batch, find_connections_batch, find_peaks_batch, find_people,
    process_batch)
from improved_body_parts_amd.models import NetworkEval
from improved_body_parts_amd.ops._backend import hip_extension
from improved_body_parts_amd.ops.assignment import (
    OVERFLOW, canonical_peaks, decode_assignment, limb_match)

from test_inference_batch import (PERSON_A, PERSON_B, PERSON_C, synth_batch,
                                  synth_maps)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def config():
    return GetConfig("Canonical")


@pytest.fixture(scope="module")
def params():
    return InferenceParams().as_params_dict()[0]


@pytest.fixture(scope="module")
def synth(config, params):
    """synth_batch on the device with the oracle's result, computed once."""
    maps = synth_batch(config).cuda()
    peaks = find_peaks_batch(maps, params, config)
    conns = find_connections_batch(peaks, maps, params, config)
    return maps, peaks, conns


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------

def _by_peak_id(conns):
    return [c[np.argsort(c[:, 0])] if len(c) else c for c in conns]


def _assert_same_assignment(got, want_peaks, want, label=""):
    """``got`` = (all_peaks, connection_all, special_k) of the device matching,
    ``want`` = (connection_all, special_k) of the oracle. Both score with the
    same device function, so rows are compared exactly."""
    all_peaks, conn_g, sk_g = got
    conn_w, sk_w = want
    assert all_peaks == want_peaks, label
    assert sk_g == sk_w, label
    assert len(conn_g) == len(conn_w)
    for k, (g, w) in enumerate(zip(_by_peak_id(conn_g), _by_peak_id(conn_w))):
        assert g is not None, f"{label} limb {k}: unresolved overflow"
        assert len(g) == len(w), f"{label} limb {k}: {len(g)} rows, oracle {len(w)}"
        if len(w):
            assert g.dtype == np.float64 and g.shape[1] == 6
            diff = np.abs(g - w).max()
            if diff:
                print(f"{label} limb {k}: max abs diff {diff:.3e}")
            np.testing.assert_array_equal(g, w, err_msg=f"{label} limb {k}")
        else:
            assert type(g) is type(w)


def _make_peaks(config, points):
    """{part: [(x, y, score), ...]} -> ``all_peaks`` with ids in row order and
    fp32-representable values."""
    all_peaks, gid = [], 0
    for c in range(config.heat_layers):
        sub = []
        for x, y, s in points.get(c, []):
            sub.append((float(np.float32(x)), float(np.float32(y)),
                        float(np.float32(s)), gid))
            gid += 1
        all_peaks.append(sub)
    return all_peaks


def _device_peaks(all_peaks_list, n_parts, max_peaks):
    """The canonical (peaks, offsets) tensors of hand-made ``all_peaks``."""
    N = len(all_peaks_list)
    peaks = np.zeros((N, max_peaks, 5), dtype=np.float32)
    offsets = np.zeros((N, n_parts + 1), dtype=np.int32)
    for n, all_peaks in enumerate(all_peaks_list):
        r = 0
        for c, sub in enumerate(all_peaks):
            offsets[n, c] = r
            for pk in sub:
                assert pk[3] == r
                peaks[n, r] = [c, pk[0], pk[1], pk[2], 0.0]
                r += 1
        offsets[n, n_parts] = r
    return torch.from_numpy(peaks).cuda(), torch.from_numpy(offsets).cuda()


def _raw_match(maps, all_peaks_list, params, config, max_part=64, max_peaks=256):
    """limb_match on hand-made peaks -> (decoded results, counts)."""
    peaks, offsets = _device_peaks(all_peaks_list, config.heat_layers, max_peaks)
    rows, counts = limb_match(
        maps, peaks, offsets, config.limbs_conn,
        config.num_layers - config.paf_layers, params["mid_num"],
        params["thre2"], params["connect_ration"], max_part=max_part)
    assert rows.shape == (len(all_peaks_list), len(config.limbs_conn), max_part, 6)
    counts = counts.cpu().numpy()
    return decode_assignment(peaks.cpu().numpy(), offsets.cpu().numpy(),
                             rows.cpu().numpy(), counts), counts


def _paf_maps(config, H, W, paf):
    """(1, heat + paf, H, W) device maps: empty keypoint planes, ``paf`` limbs."""
    n_heat = config.num_layers - config.paf_layers
    maps = torch.zeros(1, config.num_layers, H, W)
    maps[0, n_heat:] = paf
    return maps.cuda()


def _oracle_combined(all_peaks, maps, params, config):
    """Per limb the ``combined`` values of the candidates that survive the
    host's filters, from the oracle's own scores (the limb_scores kernel) and
    in the host's arithmetic."""
    first = config.num_layers - config.paf_layers
    flat = sorted((p for sub in all_peaks for p in sub), key=lambda p: p[3])
    cands, meta = [], []
    for k, (a, b) in enumerate(config.limbs_conn):
        for pa in all_peaks[a]:
            for pb in all_peaks[b]:
                cands.append((first + k, pa[3], pb[3]))
                meta.append((k, pa, pb))
    peaks_dev = torch.tensor([[0.0, p[0], p[1], p[2], 0.0] for p in flat],
                             dtype=torch.float32, device=maps.device)
    cand_dev = torch.tensor(cands, dtype=torch.int32, device=maps.device)
    scores = hip_extension().limb_scores(
        maps, peaks_dev, cand_dev, int(params["mid_num"]),
        float(params["thre2"])).cpu().numpy()
    out = {}
    for (k, pa, pb), (s_prior, pass_ratio, length) in zip(meta, scores):
        if length < 1e-6:
            continue
        if pass_ratio >= float(params["connect_ration"]) and s_prior > 0:
            out.setdefault(k, []).append(
                0.5 * s_prior + 0.25 * pa[2] + 0.25 * pb[2])
    return out


# --------------------------------------------------------------------------
# 1. canonical order
# --------------------------------------------------------------------------

def _host_canonical(buf_np, max_peaks):
    out = []
    for n in range(buf_np.shape[0]):
        cnt = min(int(buf_np[n, 0, :1].view(np.int32)[0]), max_peaks)
        rows = buf_np[n, 1:1 + cnt]
        out.append(rows[np.lexsort((rows[:, 1], rows[:, 2], rows[:, 0]))])
    return out


def test_canonical_order(config, params, synth):
    maps = synth[0]
    C = config.heat_layers
    ext = hip_extension()
    buf = ext.peaks_batched(maps, C, float(params["thre1"]),
                            int(params["offset_radius"]), 512)
    peaks, offsets = canonical_peaks(buf, C)
    assert peaks.shape == (3, 512, 5) and peaks.dtype == torch.float32
    assert offsets.shape == (3, C + 1) and offsets.dtype == torch.int32
    peaks, offsets = peaks.cpu().numpy(), offsets.cpu().numpy()
    full = _host_canonical(buf.cpu().numpy(), 512)
    assert [len(r) for r in full] == [12, 0, 6]
    for n, want in enumerate(full):
        # equals the host lexsort of the same buffer
        np.testing.assert_array_equal(peaks[n, :len(want)], want)
        assert not peaks[n, len(want):].any()
        # offsets equal the per-channel counts
        per_channel = np.bincount(want[:, 0].astype(int), minlength=C)
        np.testing.assert_array_equal(offsets[n],
                                      np.concatenate([[0], np.cumsum(per_channel)]))

    # max_peaks=4: the counter overshoots the cap; the count is clamped and
    # every row is one of the uncapped rows
    buf4 = ext.peaks_batched(maps, C, float(params["thre1"]),
                             int(params["offset_radius"]), 4)
    raw = buf4.cpu().numpy()[:, 0, 0].view(np.int32)
    assert raw.tolist() == [12, 0, 6]
    peaks4, offsets4 = canonical_peaks(buf4, C)
    peaks4, offsets4 = peaks4.cpu().numpy(), offsets4.cpu().numpy()
    assert offsets4[:, -1].tolist() == [4, 0, 4]
    for n in range(3):
        cnt = offsets4[n, -1]
        allowed = {tuple(r) for r in full[n].tolist()}
        got = peaks4[n, :cnt]
        assert len({tuple(r) for r in got.tolist()}) == cnt
        for row in got.tolist():
            assert tuple(row) in allowed, f"image {n}: foreign row {row}"
        np.testing.assert_array_equal(
            got, got[np.lexsort((got[:, 1], got[:, 2], got[:, 0]))])
        assert (np.diff(offsets4[n]) >= 0).all() and offsets4[n, 0] == 0


# --------------------------------------------------------------------------
# 2. pipeline equality
# --------------------------------------------------------------------------

def test_assign_batch_equals_oracle(config, params, synth):
    maps, want_peaks, want_conns = synth
    got = assign_batch(maps, params, config)
    assert len(got) == 3
    people = []
    for n in range(3):
        _assert_same_assignment(got[n], want_peaks[n], want_conns[n], f"image {n}")
        sub_g, cand_g = find_people(got[n][1], got[n][2], got[n][0], params, config)
        # the oracle's rows in the same (peak id) order: the rank of scores
        # that tie to rounding is not part of the result
        sub_w, cand_w = find_people(_by_peak_id(want_conns[n][0]), want_conns[n][1],
                                    want_peaks[n], params, config)
        sub_o, _ = find_people(_by_peak_id(got[n][1]), got[n][2], got[n][0],
                               params, config)
        np.testing.assert_array_equal(sub_o, sub_w)
        np.testing.assert_array_equal(cand_g, cand_w)
        people.append(len(sub_g))
    assert people == [2, 0, 1]
    # deterministic: no atomics anywhere after the peak search
    again = assign_batch(maps, params, config)
    for a, b in zip(got, again):
        assert a[0] == b[0] and a[2] == b[2]
        for x, y in zip(a[1], b[1]):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


# --------------------------------------------------------------------------
# 3. random contest
# --------------------------------------------------------------------------

def test_random_contest(config, params):
    """5 x 7 and 7 x 5 candidate tiles (even parts have 5 peaks, odd parts 7, so
    5 x 5 and 7 x 7 occur too) of long random segments on random PAF planes:
    nearly every candidate survives and competes for rows and columns."""
    rs = np.random.RandomState(30)
    paf = torch.from_numpy(
        rs.uniform(0.2, 1.0, (config.paf_layers, 64, 64)).astype(np.float32))
    maps = _paf_maps(config, 64, 64, paf)
    points = {c: [(rs.uniform(1, 62), rs.uniform(1, 62), rs.uniform(0.3, 1.0))
                  for _ in range(5 if c % 2 == 0 else 7)]
              for c in range(config.heat_layers)}
    all_peaks = _make_peaks(config, points)
    shapes = {(len(all_peaks[a]), len(all_peaks[b])) for a, b in config.limbs_conn}
    assert {(5, 7), (7, 5)} <= shapes

    # precondition on the oracle's own scores: no two combined values of a limb
    # within 1e-6, so the ranking does not hang on rounding
    combined = _oracle_combined(all_peaks, maps, params, config)
    assert len(combined) == len(config.limbs_conn)
    for k, vals in combined.items():
        assert len(vals) >= 20, f"limb {k}: only {len(vals)} candidates survive"
        gaps = np.diff(np.sort(np.asarray(vals, dtype=np.float64)))
        assert gaps.min() > 1e-6, f"limb {k}: combined scores {gaps.min():.2e} apart"

    want_conn, want_sk = find_connections_batch([all_peaks], maps, params, config)[0]
    (got,), counts = _raw_match(maps, [all_peaks], params, config)
    assert got[0] == all_peaks and got[2] == want_sk == []
    for k, (g, w) in enumerate(zip(got[1], want_conn)):
        a_part, b_part = config.limbs_conn[k]
        full = min(len(all_peaks[a_part]), len(all_peaks[b_part]))
        assert counts[0, k] == len(w) == full, f"limb {k}"
        sel_g = {(int(r[3]), int(r[4])) for r in g}
        sel_w = {(int(r[3]), int(r[4])) for r in w}
        assert sel_g == sel_w, f"limb {k}: {sorted(sel_g)} != {sorted(sel_w)}"
        g, w = _by_peak_id([g])[0], _by_peak_id([w])[0]
        np.testing.assert_array_equal(g[:, [0, 1, 3, 4]], w[:, [0, 1, 3, 4]])
        err = np.abs(g[:, [2, 5]] - w[:, [2, 5]]).max()
        if err:
            print(f"limb {k}: score/length max abs diff {err:.3e}")
        assert err <= 1e-6
        # the device emits rows in selection order: best combined first
        comb = [0.5 * np.float32(r[2]) + 0.25 * all_peaks[a_part][int(r[3])][2]
                + 0.25 * all_peaks[b_part][int(r[4])][2] for r in got[1][k]]
        assert all(x > y for x, y in zip(comb, comb[1:])), f"limb {k}: {comb}"


# --------------------------------------------------------------------------
# 4. exact ties
# --------------------------------------------------------------------------

def test_exact_ties(config, params):
    """Constant PAF = 1, equal peak scores, segments shorter than H / 2: every
    score is exactly 1 and every ``combined`` bitwise equal, so only the tie
    rule (smaller i * nB + j first) decides. Limb (2, 3) is 3 x 5, limb (5, 6)
    is 5 x 3; limb (9, 10) is 2 x 2 with A0 and B0 coincident: that zero-length
    pair is rejected, so (0, 1) and (1, 0) are taken instead of (0, 0), (1, 1)."""
    maps = _paf_maps(config, 64, 64, 1.0)
    line = lambda n, x0, y: [(x0 + 4.0 * i, y, 0.75) for i in range(n)]
    points = {2: line(3, 10.0, 8.0), 3: line(5, 12.0, 20.0),
              5: line(5, 10.0, 30.0), 6: line(3, 12.0, 42.0),
              9: [(40.0, 50.0, 0.75), (50.0, 50.0, 0.75)],
              10: [(40.0, 50.0, 0.75), (50.0, 58.0, 0.75)]}
    all_peaks = _make_peaks(config, points)
    k35, k53, k22 = (config.limbs_conn.index(l) for l in ((2, 3), (5, 6), (9, 10)))

    combined = _oracle_combined(all_peaks, maps, params, config)
    assert sorted(combined) == sorted([k35, k53, k22])
    assert [len(combined[k]) for k in (k35, k53, k22)] == [15, 15, 3]
    for vals in combined.values():
        assert len({np.float32(v).tobytes() for v in vals}) == 1

    (got,), counts = _raw_match(maps, [all_peaks], params, config)
    sel = lambda k: [(int(r[3]), int(r[4])) for r in got[1][k]]
    assert sel(k35) == [(0, 0), (1, 1), (2, 2)]
    assert sel(k53) == [(0, 0), (1, 1), (2, 2)]
    assert sel(k22) == [(0, 1), (1, 0)]
    assert counts[0].tolist() == [
        {k35: 3, k53: 3, k22: 2}.get(k, -1) for k in range(len(config.limbs_conn))]
    for k in (k35, k53, k22):
        assert (got[1][k][:, 2] == 1.0).all()
    want = find_connections_batch([all_peaks], maps, params, config)[0]
    _assert_same_assignment(got, all_peaks, want, "ties")


# --------------------------------------------------------------------------
# 5. full tile
# --------------------------------------------------------------------------

def test_full_tile(config, params):
    """nA = nB = 64 on limb (2, 3) of a 128 x 128 map: 4096 candidates, 64
    rounds, bit 63 of both masks."""
    rs = np.random.RandomState(5)
    paf = torch.from_numpy(
        rs.uniform(0.2, 1.0, (config.paf_layers, 128, 128)).astype(np.float32))
    maps = _paf_maps(config, 128, 128, paf)
    points = {c: [(rs.uniform(1, 126), rs.uniform(1, 126), rs.uniform(0.3, 1.0))
                  for _ in range(64)] for c in (2, 3)}
    all_peaks = _make_peaks(config, points)
    k = config.limbs_conn.index((2, 3))
    want = find_connections_batch([all_peaks], maps, params, config)[0]
    assert len(want[0][k]) == 64, "oracle does not use every row and column"
    (got,), counts = _raw_match(maps, [all_peaks], params, config)
    assert counts[0, k] == 64
    assert {int(r[3]) for r in got[1][k]} == set(range(64))
    assert {int(r[4]) for r in got[1][k]} == set(range(64))
    _assert_same_assignment(got, all_peaks, want, "full tile")


# --------------------------------------------------------------------------
# 6. overflow
# --------------------------------------------------------------------------

def _check_overflow(maps, params, config, max_part, part, n_expected):
    """Image 0 of ``maps`` has ``n_expected`` > max_part peaks of ``part``: the
    raw op reports -2 for exactly that image's limbs of the part, and
    assign_batch still equals the oracle everywhere."""
    C = config.heat_layers
    want_peaks = find_peaks_batch(maps, params, config)
    want_conns = find_connections_batch(want_peaks, maps, params, config)
    assert len(want_peaks[0][part]) == n_expected
    assert all(len(sub) <= max_part for n, pk in enumerate(want_peaks)
               for c, sub in enumerate(pk) if (n, c) != (0, part))
    buf = hip_extension().peaks_batched(maps, C, float(params["thre1"]),
                                        int(params["offset_radius"]), 512)
    peaks, offsets = canonical_peaks(buf, C)
    _, counts = limb_match(maps, peaks, offsets, config.limbs_conn,
                           config.num_layers - config.paf_layers,
                           params["mid_num"], params["thre2"],
                           params["connect_ration"], max_part=max_part)
    counts = counts.cpu().numpy()
    for k, (a, b) in enumerate(config.limbs_conn):
        other = b if a == part else a
        hit = part in (a, b) and len(want_peaks[0][other]) > 0
        assert (counts[0, k] == OVERFLOW) == hit, f"limb {k}: {counts[0, k]}"
    assert (counts[0] == OVERFLOW).any()
    assert not (counts[1:] == OVERFLOW).any()
    got = assign_batch(maps, params, config, max_part=max_part)
    for n in range(len(got)):
        _assert_same_assignment(got[n], want_peaks[n], want_conns[n], f"image {n}")


def test_overflow_small(config, params):
    """max_part=2, three peaks of part 0 in image 0 only."""
    maps = torch.stack([
        synth_maps(config, [PERSON_A, PERSON_B, {0: (60.0, 100.0)}]),
        synth_maps(config, []),
        synth_maps(config, [PERSON_C])]).cuda()
    _check_overflow(maps, params, config, 2, 0, 3)


def test_overflow_65_peaks(config, params):
    """65 peaks of part 0 at max_part=64; constant limb planes so that the
    redone image has real connections."""
    grid = [(8.0 + 14 * i, 8.0 + 14 * j) for j in range(9) for i in range(9)][:65]
    crowd = [{0: xy} for xy in grid] + [{1: (15.0, 15.0)}, {1: (71.0, 57.0)}]
    maps = torch.stack([synth_maps(config, crowd),
                        synth_maps(config, [PERSON_C])])
    maps[:, config.num_layers - config.paf_layers:] = 0.5
    _check_overflow(maps.cuda(), params, config, 64, 0, 65)


# --------------------------------------------------------------------------
# 7. process_batch on the device
# --------------------------------------------------------------------------

def test_process_batch_device_matching(config):
    torch.manual_seed(0)
    model = NetworkEval(TrainingOpt(nstack=1, batch_size=1), config,
                        bn=True).cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.float()
    model.eval()
    p, mp = InferenceParams().as_params_dict()
    mp = dict(mp)
    mp["boxsize"] = 64
    rs = np.random.RandomState(1)
    imgs = [rs.rand(64, 64, 3).astype(np.float32) for _ in range(3)]
    host = process_batch(imgs, model, config, p, mp, matching="host")
    dev = process_batch(imgs, model, config, p, mp, matching="device")
    print("people per image:", [len(r) for r in host])
    assert len(dev) == len(host) == 3
    for g, w in zip(dev, host):
        assert len(g) == len(w)
        for (kg, sg), (kw, sw) in zip(g, w):
            assert kg == kw and sg == sw
    with pytest.raises(ValueError):
        process_batch(imgs, model, config, p, mp, matching="bogus")
