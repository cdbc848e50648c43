#!/usr/bin/env python3
"""Record the upstream reference implementation's answers for
tests/test_reference_parity.py.

    python oracle/make_parity_golden.py --reference /path/to/Improved-Body-Parts

imports the upstream repository (never vendored here), feeds it the seeded
inputs of tests/parity_inputs.py and writes what it returns to
tests/golden/reference_parity/. The suite then compares this project against
those recorded answers, so it needs no copy of the upstream code. Re-run only
when tests/parity_inputs.py changes.
"""
import argparse
import gzip
import importlib
import json
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import parity_inputs as P  # noqa: E402


def stub_ref_modules():
    """Stub the reference's unused heavy imports (cv2/torchvision optional)."""
    if "cv2" not in sys.modules:
        from improved_body_parts_amd.data.heatmapper import _erode3x3
        fake = types.ModuleType("cv2")
        fake.erode = lambda m, kernel: _erode3x3(np.asarray(m, np.float32))
        sys.modules["cv2"] = fake
    if "torchvision" not in sys.modules:
        sys.modules["torchvision"] = types.ModuleType("torchvision")


def import_reference_evaluate():
    """Import reference evaluate.py with its unused heavy deps stubbed."""
    stub_ref_modules()
    tv = sys.modules["torchvision"]
    tv.__path__ = []
    tvm = types.ModuleType("torchvision.models")
    tvm.densenet = types.ModuleType("densenet")
    tv.models = tvm
    sys.modules["torchvision.models"] = tvm
    for name in ["tqdm", "matplotlib", "matplotlib.pyplot", "pycocotools",
                 "pycocotools.coco", "pycocotools.cocoeval", "configobj"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pycocotools.coco"].COCO = object
    sys.modules["pycocotools.cocoeval"].COCOeval = object
    sys.modules["tqdm"].tqdm = lambda x: x

    class _ConfigObj(dict):
        def __init__(self, path):
            super().__init__()
            section = None
            for line in open(path):
                line = line.split("#")[0].strip()
                if not line:
                    continue
                if line.startswith("["):
                    section = line.strip("[]")
                    self[section] = {}
                    continue
                if "=" in line and section:
                    k, v = (s.strip() for s in line.split("=", 1))
                    self[section][k] = v
    sys.modules["configobj"].ConfigObj = _ConfigObj
    argv = sys.argv
    sys.argv = ["evaluate.py"]
    try:
        import evaluate as ref_eval
    finally:
        sys.argv = argv
    return ref_eval


def dump_json(name, obj):
    text = json.dumps(obj) + "\n"
    if name.endswith(".gz"):   # mtime=0: same input, same bytes
        with open(P.golden_path(name), "wb") as raw, \
                gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
            f.write(text.encode())
    else:
        with open(P.golden_path(name), "w") as f:
            f.write(text)


def record_tables_and_scalars():
    from config.config import COCOSourceConfig as RefSrc
    from config.config import GetConfig as RefGetConfig
    from models.loss_model import MultiTaskLoss as RefLoss
    from models.loss_model_parallel import MultiTaskLossParallel as RefLossPar
    from py_cocodata_server.py_data_heatmapper import Heatmapper as RefHeatmapper
    from utils import util as ref_util
    from improved_body_parts_amd.config import GetConfig, TrainingOpt

    ref = RefGetConfig("Canonical")
    cfg = GetConfig("Canonical")
    opt = TrainingOpt(nstack=2, batch_size=2, nstack_weight=[1, 1])
    rec = {"config": {
        "num_layers": ref.num_layers, "paf_layers": ref.paf_layers,
        "limb_from": list(ref.limb_from), "limb_to": list(ref.limb_to),
        "heat_start": ref.heat_start, "bkg_start": ref.bkg_start,
        "flip_heat_ord": np.asarray(ref.flip_heat_ord).tolist(),
        "flip_paf_ord": np.asarray(ref.flip_paf_ord).tolist(),
        "dt_gt_mapping": {str(k): v for k, v in ref.dt_gt_mapping.items()},
        "offset_layers": ref.offset_layers,
    }}

    pred, mask, gt = P.loss_inputs(0, cfg.num_layers, opt.nstack)
    rec["focal_l2_loss"] = float(RefLoss(opt, cfg)(pred, (mask, gt)))
    pred, mask, gt = P.loss_inputs(3, cfg.num_layers, opt.nstack)
    rec["parallel_loss"] = float(RefLossPar(opt, cfg)(pred, (mask, gt)))

    theirs, pad = ref_util.padRightDownCorner(P.pad_image(), 64, 128)
    np.save(P.golden_path("pad_image.npy"), np.asarray(theirs))
    rec["pad"] = [int(p) for p in pad]

    fmap = P.centroid_map()
    rec["refine_centroid"] = [
        [float(v) for v in ref_util.refine_centroid(fmap, a, 2)]
        for a in P.CENTROID_ANCHORS]

    joints = P.coco_joints()
    conv = RefSrc("d.h5").convert({"joints": joints.copy(), "image": "x.jpg"},
                                  ref)
    np.save(P.golden_path("coco_convert_joints.npy"),
            np.asarray(conv["joints"], dtype=np.float64))

    ref_hm = RefHeatmapper(ref)
    people = P.heatmapper_people(cfg)
    mask_all = np.ones(cfg.mask_shape, dtype=np.float32)
    maps = np.asarray(ref_hm.create_heatmaps(people.astype(float).copy(),
                                             mask_all), dtype=np.float32)
    np.savez_compressed(P.golden_path("heatmapper.npz"), people=people,
                        heatmaps=maps)
    try:
        ref_hm.put_offset(np.zeros((1, 18, 3), np.float32))
        rec["put_offset_raises"] = None
    except Exception as e:  # recorded, not handled: the test pins the type
        rec["put_offset_raises"] = type(e).__name__
    dump_json("tables.json", rec)


def record_grouping(ref_eval):
    from improved_body_parts_amd.config import GetConfig, InferenceParams
    from improved_body_parts_amd.engine.inference import find_peaks
    config = GetConfig("Canonical")

    def run(people, size, remove_recon):
        params, _ = InferenceParams().as_params_dict()
        params["remove_recon"] = remove_recon
        heat, paf = P.synth_scene(config, people, H=size, W=size)
        all_peaks = P.peaks_from_json(P.peaks_to_json(
            find_peaks(torch.from_numpy(heat), params, config)))
        conn, special = ref_eval.find_connections(all_peaks, paf, size,
                                                  dict(params))
        subset, cand = ref_eval.find_people(conn, special, all_peaks,
                                            dict(params))
        return {"all_peaks": P.peaks_to_json(all_peaks),
                "connections": P.conns_to_json(conn),
                "special_k": [int(k) for k in special],
                "subset": np.asarray(subset, dtype=np.float64).tolist(),
                "candidate": np.asarray(cand, dtype=np.float64).tolist()}

    rec = {"two_people": run(P.GROUPING_PEOPLE, 256, 0)}
    for rr, seed in P.CROWDED_CASES:
        rec[f"crowded_{rr}_{seed}"] = run(P.crowded_people(seed, rr), 320, rr)
    dump_json("grouping.json.gz", rec)


def record_models():
    x = P.model_input()
    layouts = {}
    for name, refmod, _ours, kwargs in P.MODEL_CASES:
        rm = importlib.import_module(refmod)
        ref = rm.PoseNet(2, 256, 50, bn=True, **kwargs)
        layouts[name] = P.state_layout(ref)
        P.fill_state_dict(ref).double().eval()
        with torch.no_grad():
            out = ref(x)
        if name == "ae_pose":   # [nstack][1] nesting
            arrs = {f"stack{i}": out[i][0] for i in range(2)}
        else:                   # last stack, 5 scales
            assert len(out) == 2
            arrs = {f"scale{s}": out[1][s] for s in range(5)}
        # stored in float32: its rounding (6e-8) is far inside the tests' 1e-5
        np.savez_compressed(P.golden_path(f"{name}_forward.npz"),
                            **{k: v.float().numpy() for k, v in arrs.items()})
    # the layout our trainer's checkpoints must load into (increase=128)
    from models.posenet import PoseNet as RefPoseNet
    layouts["posenet_inc128"] = P.state_layout(
        RefPoseNet(2, 256, 50, bn=True, increase=128))
    dump_json("layouts.json.gz", layouts)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reference", required=True,
                    help="checkout of the upstream reference repository")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    warnings.filterwarnings("ignore")
    os.makedirs(P.GOLDEN_DIR, exist_ok=True)
    ref_eval = import_reference_evaluate()
    record_tables_and_scalars()
    record_grouping(ref_eval)
    record_models()
    print(f"wrote {P.GOLDEN_DIR}")


if __name__ == "__main__":
    main()
