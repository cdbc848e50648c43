"""Deterministic inputs shared by tests/test_reference_parity.py and the
recipe that records the upstream reference's answers (oracle/make_parity_golden.py).

Everything here is seeded through numpy's legacy ``RandomState`` (whose stream
is frozen across numpy releases) so the recorded answers under
tests/golden/reference_parity/ stay valid wherever the suite runs.
"""
import gzip
import json
import os
import zlib

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "golden", "reference_parity")

# (golden name, reference module, our class name, constructor kwargs)
MODEL_CASES = [
    ("posenet", "models.posenet", "PoseNet", {"increase": 32}),
    ("posenet_final", "models.posenet_final", "PoseNetFinal", {"increase": 32}),
    ("posenet2", "models.posenet2", "PoseNetAttention", {"increase": 32}),
    ("posenet3", "models.posenet3", "PoseNetLight", {"increase": 32}),
    ("posenet_independent", "models.posenet_independent", "PoseNetIndependent",
     {"increase": 32}),
    ("ae_pose", "models.ae_pose", "AEPoseNet", {}),
]

GROUPING_PEOPLE = [
    {0: (60.0, 40.0), 1: (60.0, 70.0), 2: (35.0, 72.0), 3: (30.0, 112.0),
     5: (85.0, 72.0), 6: (90.0, 112.0), 8: (45.0, 135.0), 11: (75.0, 135.0)},
    {0: (180.0, 50.0), 1: (180.0, 80.0), 2: (155.0, 82.0), 3: (150.0, 122.0),
     5: (205.0, 82.0), 6: (210.0, 122.0), 8: (165.0, 145.0), 11: (195.0, 145.0)},
]
CROWDED_CASES = [(rr, seed) for rr in (0, 1) for seed in (123, 77, 2024)]


def golden_path(name):
    return os.path.join(GOLDEN_DIR, name)


def load_json(name):
    """Read a recorded JSON answer; the bulky ones are stored gzipped."""
    opener = gzip.open if name.endswith(".gz") else open
    with opener(golden_path(name), "rt") as f:
        return json.load(f)


def loss_inputs(seed, num_layers, nstack, n=2):
    """Random multi-scale predictions + (mask, gt) for the loss parity tests."""
    rs = np.random.RandomState(seed)
    pred = [[torch.from_numpy(
        (rs.standard_normal((n, num_layers, 128 // (2 ** s), 128 // (2 ** s)))
         * 0.1).astype(np.float32)) for s in range(5)] for _ in range(nstack)]
    mask = torch.from_numpy((rs.rand(n, 1, 128, 128) > 0.2).astype(np.float32))
    gt = torch.from_numpy(rs.rand(n, num_layers, 128, 128).astype(np.float32))
    return pred, mask, gt


def heatmapper_people(cfg):
    from improved_body_parts_amd.data import sample_people
    return sample_people(np.random.default_rng(5), cfg.width, cfg.height,
                         max_people=3)


def pad_image():
    return np.random.RandomState(0).randint(0, 255, (37, 53, 3)).astype(np.uint8)


CENTROID_ANCHORS = [(5, 7), (0, 0), (39, 39), (20, 20)]


def centroid_map():
    return np.random.RandomState(1).rand(40, 40).astype(np.float32)


def coco_joints():
    rs = np.random.RandomState(4)
    joints = rs.rand(5, 17, 3).astype(np.float64) * 100
    joints[:, :, 2] = rs.randint(0, 4, (5, 17))
    return joints


def synth_scene(config, people, H=256, W=256, sigma=3.0):
    n_heat = config.num_layers - config.paf_layers
    heat = np.zeros((H, W, n_heat), dtype=np.float32)
    paf = np.zeros((H, W, config.paf_layers), dtype=np.float32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    for person in people:
        for part, (x, y) in person.items():
            g = np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / (2 * sigma ** 2))
            heat[..., part] = np.maximum(heat[..., part], g)
        for k, (a, b) in enumerate(config.limbs_conn):
            if a in person and b in person:
                ax, ay = person[a]
                bx, by = person[b]
                vx, vy = bx - ax, by - ay
                L2 = vx * vx + vy * vy + 1e-9
                t = np.clip(((xx - ax) * vx + (yy - ay) * vy) / L2, 0, 1)
                d2 = (xx - (ax + t * vx)) ** 2 + (yy - (ay + t * vy)) ** 2
                paf[..., k] = np.maximum(paf[..., k],
                                         np.exp(-d2 / (2 * sigma ** 2)))
    return heat, paf


def crowded_people(seed, remove_recon, H=320, W=320):
    from improved_body_parts_amd.data import sample_people
    rng = np.random.default_rng(seed + remove_recon)
    people = []
    for p in sample_people(rng, W, H, max_people=5):
        d = {j: (float(p[j, 0]), float(p[j, 1])) for j in range(18)
             if p[j, 2] < 2 and 0 <= p[j, 0] < W and 0 <= p[j, 1] < H}
        if d:
            people.append(d)
    return people


def peaks_to_json(all_peaks):
    return [[[float(p[0]), float(p[1]), float(p[2]), int(p[3])] for p in sub]
            for sub in all_peaks]


def peaks_from_json(obj):
    return [[(p[0], p[1], p[2], int(p[3])) for p in sub] for sub in obj]


def conns_to_json(conn_all):
    return [np.asarray(c, dtype=np.float64).reshape(-1, 6).tolist()
            for c in conn_all]


def fill_state_dict(model):
    """Overwrite every floating tensor of ``model.state_dict()`` with values
    that depend only on the tensor's NAME and shape, so two implementations
    with the same parameter layout get bit-identical weights without a
    checkpoint file. Scales keep a deep conv+BN+ReLU stack well conditioned."""
    sd = model.state_dict()
    out = {}
    for k in sorted(sd):
        t = sd[k]
        if not t.is_floating_point():
            out[k] = t.clone()
            continue
        rs = np.random.RandomState(zlib.crc32(k.encode()))
        v = rs.standard_normal(t.numel()).reshape(tuple(t.shape))
        if k.endswith("running_var"):
            v = 0.5 + np.abs(v)
        elif k.endswith("running_mean") or k.endswith("bias"):
            v = 0.1 * v
        elif t.dim() >= 2:
            v = v * np.sqrt(2.0 / max(t[0].numel(), 1))
        else:
            v = 1.0 + 0.1 * v
        out[k] = torch.from_numpy(np.ascontiguousarray(v)).to(t.dtype)
    model.load_state_dict(out)
    return model


def model_input():
    return torch.from_numpy(np.random.RandomState(7).rand(1, 64, 64, 3))


def state_layout(model):
    """{name: [shape, dtype]} of a module's state_dict."""
    return {k: [list(v.shape), str(v.dtype)]
            for k, v in model.state_dict().items()}
