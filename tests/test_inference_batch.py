"""Inference pipeline on the CPU: composed resample tables, predict /
predict_batch against the per-image torch-chain oracle, process_batch and the
batched post-processing against their per-image wrappers (grouping, chunking,
per-image offsets), and the batch endpoints of the service."""
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from improved_body_parts_amd.config import GetConfig, InferenceParams, TrainingOpt
from improved_body_parts_amd.engine import (
    find_connections, find_connections_batch, find_peaks, find_peaks_batch,
    find_people, predict, predict_batch, process, process_batch)
from improved_body_parts_amd.models import NetworkEval
from improved_body_parts_amd.ops.ensemble import (
    TABLE_K, axis_table, compose_axis_matrix, ensemble_merge, table_to_matrix)

from inference_oracle import reference_predict


@pytest.fixture(scope="module")
def config():
    return GetConfig("Canonical")


@pytest.fixture(scope="module")
def model(config):
    torch.manual_seed(0)
    return NetworkEval(TrainingOpt(nstack=1, batch_size=1), config, bn=True).eval()


def _params(boxsize, **over):
    p, mp = InferenceParams().as_params_dict()
    p, mp = dict(p), dict(mp)
    mp["boxsize"] = boxsize
    p.update(over)
    return p, mp


# --------------------------------------------------------------------------
# composed tap tables against the torch chain
# --------------------------------------------------------------------------

# (h4, w4, stride, sh, sw, H, W)
CHAIN_SHAPES = [
    (16, 16, 4, 60, 52, 48, 41),
    (16, 32, 4, 50, 120, 75, 180),
    (160, 160, 4, 640, 640, 512, 512),
    (8, 8, 4, 30, 27, 97, 13),
    (16, 16, 4, 64, 64, 64, 64),      # identity second pass: sh == ph == H
    (24, 20, 2, 45, 38, 61, 50),      # stride 2
]


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_composed_tables_match_torch_chain(shape):
    """R = D . U[:sh] per axis, stored as (start, 8 fp32 taps), reproduces
    interpolate -> crop -> interpolate. atol 2e-5 = 10x the 2e-6 error of the
    fp32 torch chain itself against the fp64 composition; |R| row sums stay
    <= 1.39, so the error does not grow with size."""
    h4, w4, stride, sh, sw, H, W = shape
    x = torch.rand(3, h4, w4, generator=torch.Generator().manual_seed(1))
    up = F.interpolate(x[None], size=(h4 * stride, w4 * stride), mode="bicubic",
                       align_corners=False)[:, :, :sh, :sw]
    want = F.interpolate(up, size=(H, W), mode="bicubic", align_corners=False)[0]

    ys, yw, yspan = axis_table(h4, stride, sh, H)
    xs, xw, xspan = axis_table(w4, stride, sw, W)
    assert yw.shape == (H, TABLE_K) and xw.shape == (W, TABLE_K)
    # stride >= 4: the 4 intermediate pixels of a bicubic read cover at most two
    # source floors, so a row spans at most 5 source taps
    bound = 5 if stride >= 4 else TABLE_K
    assert yspan <= bound and xspan <= bound, (yspan, xspan)
    assert ys.min() >= 0 and xs.min() >= 0
    Ry = table_to_matrix(ys, yw, h4)
    Rx = table_to_matrix(xs, xw, w4)
    # one bicubic pass has |row| sum 1 + 2 * 0.75 * t * (1 - t) <= 1.375, so the
    # composition is bounded by 1.375^2 at any size; at stride 4 it stays <= 1.39
    gain = 1.39 if stride >= 4 else 1.375 ** 2
    assert np.abs(Ry).sum(1).max() <= gain and np.abs(Rx).sum(1).max() <= gain
    # the fp32 table is the fp64 operator rounded once
    assert np.abs(Ry - compose_axis_matrix(h4, stride, sh, H)).max() < 1e-7
    got = Ry @ x.double().numpy() @ Rx.T
    err = np.abs(got - want.double().numpy()).max()
    print(f"composed vs chain {shape}: max abs err {err:.3e}")
    assert err <= 2e-5


def test_ensemble_merge_cpu_writes_and_accumulates():
    g = torch.Generator().manual_seed(2)
    v = torch.rand(4, 6, 8, 8, generator=g)
    perm = [1, 0, 2, 4, 3, 5]
    one = ensemble_merge(v, perm, 4, (30, 27), (33, 21), scale=0.5)
    assert one.shape == (2, 6, 33, 21) and one.dtype == torch.float32
    acc = one.clone()
    ensemble_merge(v, perm, 4, (30, 27), (33, 21), scale=0.5, out=acc,
                   accumulate=True)
    assert torch.allclose(acc, 2 * one, atol=1e-6)
    # mirroring the input and swapping the views mirrors the output
    sw = torch.cat([v[2:], v[:2]])
    inv = np.argsort(perm)
    full = ensemble_merge(v, perm, 4, (32, 32), (32, 32))
    mirrored = ensemble_merge(sw, perm, 4, (32, 32), (32, 32))
    assert torch.allclose(torch.flip(mirrored, dims=[-1])[:, inv], full, atol=1e-6)


# --------------------------------------------------------------------------
# predict and predict_batch against the per-image torch chain
# --------------------------------------------------------------------------

def _three_images():
    rs = np.random.RandomState(3)
    return [rs.rand(96, 80, 3).astype(np.float32),
            rs.rand(64, 64, 3).astype(np.float32),
            rs.rand(96, 80, 3).astype(np.float32)]


def _check_predict_batch(model, config, p, mp, atol):
    imgs = _three_images()
    got = predict_batch(imgs, model, config, p, mp)
    assert len(got) == 3
    worst = 0.0
    for img, (heat, paf) in zip(imgs, got):
        h_ref, p_ref = reference_predict(img, model, config, p, mp)
        assert heat.shape == h_ref.shape and paf.shape == p_ref.shape
        # (H, W, C) views of the planar buffer: the planar permute is free
        assert heat.permute(2, 0, 1).is_contiguous()
        assert paf.permute(2, 0, 1).is_contiguous()
        worst = max(worst, float((heat - h_ref).abs().max()),
                    float((paf - p_ref).abs().max()))
    print(f"predict_batch vs torch chain: max abs diff {worst:.3e}")
    assert worst <= atol


@pytest.mark.parametrize("hw,boxsize,over", [
    ((64, 64), 64, {}),
    ((96, 80), 96, {}),
    ((96, 80), 120, {"scale_search": [0.8, 1.0]}),
], ids=["64x64-box64", "96x80-box96", "96x80-box120-two-scales"])
def test_predict_equals_torch_chain(model, config, hw, boxsize, over):
    """One image through the batched pipeline: on the CPU the merge is the
    same eager chain over the same values, so the maps are bit-identical."""
    p, mp = _params(boxsize, **over)
    img = np.random.RandomState(4).rand(*hw, 3).astype(np.float32)
    heat, paf = predict(img, model, config, p, mp)
    h_ref, p_ref = reference_predict(img, model, config, p, mp)
    assert heat.dtype == torch.float32 and heat.shape == h_ref.shape
    assert paf.dtype == torch.float32 and paf.shape == p_ref.shape
    print(f"predict vs torch chain {hw} box {boxsize}: max abs diff "
          f"{max(float((heat - h_ref).abs().max()), float((paf - p_ref).abs().max())):.3e}")
    assert torch.equal(heat, h_ref) and torch.equal(paf, p_ref)


def test_predict_rotation_matches_torch_chain(model, config):
    """A rotated run of one image against the per-image (H, W, C) chain."""
    p, mp = _params(120, rotation_search=[0.0, 30.0])
    img = _three_images()[0]
    heat, paf = predict(img, model, config, p, mp)
    h_ref, p_ref = reference_predict(img, model, config, p, mp)
    worst = max(float((heat - h_ref).abs().max()),
                float((paf - p_ref).abs().max()))
    print(f"predict (rotated) vs torch chain: max abs diff {worst:.3e}")
    assert worst <= 1e-4


def test_predict_batch_matches_predict(model, config):
    """Two 96x80 images and one 64x64: the same-size group and the mixed-size
    split. boxsize 120 makes the search scale 1.25 for the 96-high images.
    atol 1e-4 on fp32 CPU (2e-5 for the resample plus slack for the CPU conv
    choosing another algorithm at another batch size)."""
    p, mp = _params(120)
    _check_predict_batch(model, config, p, mp, 1e-4)


def test_predict_batch_multiscale(model, config):
    """Two scales: exercises accumulate and scale = 1 / n_runs."""
    p, mp = _params(120, scale_search=[0.8, 1.0])
    _check_predict_batch(model, config, p, mp, 1e-4)


def test_predict_batch_rotation_fallback(model, config):
    """A rotated run keeps the torch chain, batched along N."""
    p, mp = _params(120, rotation_search=[0.0, 30.0])
    _check_predict_batch(model, config, p, mp, 1e-4)


def test_predict_batch_max_views_chunks(model, config):
    """max_views=2 pushes one image per forward; results do not change."""
    p, mp = _params(96)
    imgs = _three_images()
    a = predict_batch(imgs, model, config, p, mp, max_views=2)
    b = predict_batch(imgs, model, config, p, mp, max_views=16)
    for (ha, pa), (hb, pb) in zip(a, b):
        assert torch.allclose(ha, hb, atol=1e-4) and torch.allclose(pa, pb, atol=1e-4)
    with pytest.raises(ValueError):
        predict_batch(imgs, model, config, p, mp, max_views=1)


# --------------------------------------------------------------------------
# batched post-processing against the per-image functions
# --------------------------------------------------------------------------

def synth_maps(config, people, H=128, W=128, sigma=3.0):
    """Gaussian-blob heatmaps and limb ridges for a list of people
    (part index -> (x, y)), as planar (heat + paf, H, W)."""
    n_heat = config.num_layers - config.paf_layers
    heat = np.zeros((n_heat, H, W), dtype=np.float32)
    paf = np.zeros((config.paf_layers, H, W), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for person in people:
        for part, (x, y) in person.items():
            g = np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * sigma ** 2))
            heat[part] = np.maximum(heat[part], g)
        for k, (a, b) in enumerate(config.limbs_conn):
            if a in person and b in person:
                ax, ay = person[a]
                bx, by = person[b]
                vx, vy = bx - ax, by - ay
                t = ((xx - ax) * vx + (yy - ay) * vy) / (vx * vx + vy * vy + 1e-9)
                t = np.clip(t, 0, 1)
                d2 = (xx - (ax + t * vx)) ** 2 + (yy - (ay + t * vy)) ** 2
                paf[k] = np.maximum(paf[k], np.exp(-d2 / (2 * sigma ** 2)))
    return torch.from_numpy(np.concatenate([heat, paf]))


PERSON_A = {0: (30.0, 20.0), 1: (30.0, 35.0), 2: (20.0, 35.0), 3: (18.0, 55.0),
            5: (40.0, 35.0), 6: (42.0, 55.0)}
PERSON_B = {0: (90.0, 25.0), 1: (90.0, 40.0), 2: (80.0, 40.0), 3: (78.0, 60.0),
            5: (100.0, 40.0), 6: (102.0, 60.0)}
PERSON_C = {0: (60.0, 70.0), 1: (60.0, 85.0), 2: (50.0, 85.0), 3: (48.0, 105.0),
            5: (70.0, 85.0), 6: (72.0, 105.0)}


def synth_batch(config):
    """Three images with 2, 0 and 1 people: the empty one in the middle
    catches offset errors."""
    return torch.stack([synth_maps(config, [PERSON_A, PERSON_B]),
                        synth_maps(config, []),
                        synth_maps(config, [PERSON_C])])


def assert_same_connections(got, want):
    (conn_g, sk_g), (conn_w, sk_w) = got, want
    assert sk_g == sk_w
    assert len(conn_g) == len(conn_w)
    for a, b in zip(conn_g, conn_w):
        assert len(a) == len(b)
        if len(a):
            np.testing.assert_allclose(np.asarray(a), np.asarray(b), atol=1e-4)


def test_batched_postprocessing_matches_per_image(config):
    p, _ = _params(128)
    maps = synth_batch(config)
    n_heat = config.num_layers - config.paf_layers
    peaks = find_peaks_batch(maps, p, config)
    conns = find_connections_batch(peaks, maps, p, config)
    n_people = []
    for n in range(3):
        heat = maps[n, :n_heat].permute(1, 2, 0)
        paf = maps[n, n_heat:].permute(1, 2, 0)
        ref_peaks = find_peaks(heat, p, config)
        assert peaks[n] == ref_peaks
        ref_conn = find_connections(ref_peaks, paf, 128, p, config)
        assert_same_connections(conns[n], ref_conn)
        sub_g, cand_g = find_people(*conns[n], peaks[n], p, config)
        sub_w, cand_w = find_people(*ref_conn, ref_peaks, p, config)
        np.testing.assert_array_equal(sub_g, sub_w)
        np.testing.assert_array_equal(cand_g, cand_w)
        n_people.append(len(sub_g))
    assert n_people == [2, 0, 1]


def test_process_batch_matches_process(model, config):
    p, mp = _params(64)
    rs = np.random.RandomState(5)
    imgs = [rs.rand(64, 64, 3).astype(np.float32),
            rs.rand(48, 64, 3).astype(np.float32),
            rs.rand(64, 64, 3).astype(np.float32)]
    got = process_batch(imgs, model, config, p, mp)
    want = [process(i, model, config, p, mp) for i in imgs]
    assert isinstance(got, list) and len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, list) and len(g) == len(w)
        for (kg, sg), (kw, sw) in zip(g, w):
            assert len(kg) == len(kw) == 17
            assert abs(sg - sw) < 1e-3
    assert process_batch([], model, config, p, mp) == []


# --------------------------------------------------------------------------
# service
# --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def service():
    from improved_body_parts_amd.serve import PoseService
    svc = PoseService(config_name="Canonical", nstack=1, device="cpu", bf16=False)
    svc.model_params = dict(svc.model_params)
    svc.model_params["boxsize"] = 64
    return svc


def test_infer_many_matches_infer(service):
    rs = np.random.RandomState(6)
    imgs = [rs.rand(64, 64, 3).astype(np.float32) for _ in range(2)]
    many = service.infer_many(imgs)
    assert len(many) == 2
    for img, people in zip(imgs, many):
        one = service.infer(img)
        assert len(people) == len(one)
        for a, b in zip(people, one):
            assert set(a) == set(b) == {"score", "keypoints"}


def test_pose_batch_endpoint(service):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    from improved_body_parts_amd.serve import create_app
    client = TestClient(create_app(service=service))
    imgs = np.random.RandomState(7).rand(2, 64, 64, 3).astype(np.float32)
    buf = io.BytesIO()
    np.save(buf, imgs)
    r = client.post("/pose_batch", content=buf.getvalue())
    assert r.status_code == 200, r.text
    j = r.json()
    assert isinstance(j, list) and len(j) == 2
    for item in j:
        assert item["image_size"] == [64, 64]
        assert isinstance(item["people"], list)
    # JSON list of images, sizes may differ
    import json
    body = json.dumps([imgs[0].tolist(), imgs[1, :48].tolist()]).encode()
    r = client.post("/pose_batch", content=body,
                    headers={"content-type": "application/json"})
    assert r.status_code == 200, r.text
    assert [it["image_size"] for it in r.json()] == [[64, 64], [48, 64]]
    # one image is not a batch; garbage is rejected
    buf = io.BytesIO()
    np.save(buf, imgs[0])
    assert client.post("/pose_batch", content=buf.getvalue()).status_code == 400
    assert client.post("/pose_batch", content=b"nonsense").status_code == 400
    # /pose is unchanged
    r = client.post("/pose", content=buf.getvalue())
    assert r.status_code == 200 and set(r.json()) == {"people", "image_size"}
