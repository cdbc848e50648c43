"""End-to-end pipeline FPS: predict -> peaks -> connections -> greedy assembly
per image (the reference's whole-pipeline context: 7-8 FPS for the community
C++ rebuild, 5.2 FPS for the pure-Python assignment stage alone)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from improved_body_parts_amd.config import GetConfig, TrainingOpt, InferenceParams
from improved_body_parts_amd.data import SyntheticPoseDataset
from improved_body_parts_amd.engine.inference import process, process_batch
from improved_body_parts_amd.models import NetworkEval

import argparse
ap = argparse.ArgumentParser()
ap.add_argument("--train-steps", type=int, default=300,
                help="brief training first so the pipeline sees REAL peaks "
                     "(random-init nets produce none and make assembly free)")
ap.add_argument("--batch", type=int, nargs="+", default=[1],
                help="images per process_batch() call; 1 = per-image process(). "
                     "Several values are measured in turn on the same model")
ap.add_argument("--images", type=int, default=24, help="images per timed pass")
ap.add_argument("--repeats", type=int, default=1, help="timed passes per --batch")
ap.add_argument("--matching", choices=["host", "device"], nargs="+",
                default=["host"],
                help="where limb candidates are matched; several values "
                     "alternate inside each repeat on the same model")
ap.add_argument("--assembly", choices=["host", "device"], nargs="+",
                default=["host"],
                help="where people are assembled ('device' only pairs with "
                     "--matching device); several values alternate as well")
args = ap.parse_args()

config = GetConfig("Canonical")
opt = TrainingOpt(nstack=4, batch_size=1)
model = NetworkEval(opt, config, bn=True).cuda().bfloat16()
for m in model.modules():
    if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
        m.float()
if args.train_steps:
    from improved_body_parts_amd.engine import FusedSGD
    from improved_body_parts_amd.models import Network
    topt = TrainingOpt(nstack=2, batch_size=8, nstack_weight=[1, 1])
    tnet = Network(topt, config, bn=True, dist=True).cuda().bfloat16()
    for m in tnet.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.float()
    tnet.train()
    sgd = FusedSGD(tnet.parameters(), lr=4e-4, momentum=0.9, weight_decay=1e-4)
    tds = SyntheticPoseDataset(config, length=1 << 30, render=True, seed=11)
    for step in range(args.train_steps):
        b = [tds.generate(step * 8 + k)[:3] for k in range(8)]
        imgs_t = torch.stack([torch.from_numpy(x[0]) for x in b]).cuda().bfloat16()
        mms = torch.stack([torch.from_numpy(x[1]) for x in b]).cuda().bfloat16()
        hms = torch.stack([torch.from_numpy(np.ascontiguousarray(x[2])) for x in b]).cuda().bfloat16()
        lr = 4e-4 * min((step + 1) / 50.0, 1.0)
        for g in sgd.param_groups:
            g["lr"] = lr
        sgd.zero_grad(set_to_none=True)
        loss = tnet((imgs_t, mms, hms))
        if float(loss.detach()) < 1e6:
            loss.backward()
            sgd.step()
    # evaluate with the 2-stack trained net (weights are what matter for
    # realistic peak counts; note nstack in the printout)
    opt = topt
    model = NetworkEval(opt, config, bn=True).cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.float()
    model.posenet.load_state_dict(tnet.posenet.state_dict())
model.eval()
p, mp = InferenceParams().as_params_dict()
ds = SyntheticPoseDataset(config, length=64, render=True, seed=3)
imgs = [ds.generate(i % 64)[0] for i in range(args.images)]


def measure(batch_size, matching, assembly):
    """Warm up, then time one pass over ``imgs``; returns (img/s, people)."""
    if batch_size > 1:
        def run(batch):
            return sum(len(r) for r in process_batch(batch, model, config, p, mp,
                                                     matching=matching,
                                                     assembly=assembly))
        chunks = [imgs[i:i + batch_size] for i in range(0, len(imgs), batch_size)]
        # warm every batch size the timed loop uses
        for n in sorted({len(c) for c in chunks}):
            run(imgs[:n])
    else:
        def run(batch):
            return len(process(batch[0], model, config, p, mp, matching=matching,
                               assembly=assembly))
        chunks = [[img] for img in imgs]
        for img in imgs[:4]:
            run([img])                               # warmup
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n_people = 0
    for chunk in chunks:
        n_people += run(chunk)
    torch.cuda.synchronize()
    return len(imgs) / (time.perf_counter() - t0), n_people


# several --batch values alternate inside each repeat, so they see the same
# machine state and their spread can be compared
for rep in range(args.repeats):
    for b, matching, assembly in ((b, m, a) for b in args.batch
                                  for m in args.matching for a in args.assembly
                                  if a == "host" or m == "device"):
        fps, n_people = measure(b, matching, assembly)
        label = f"process_batch(batch={b})" if b > 1 else "process()"
        if matching != "host":
            label = label[:-1] + (", " if b > 1 else "") + f"matching={matching})"
        if assembly != "host":
            label = label[:-1] + f", assembly={assembly})"
        print(f"end-to-end {label} {fps:.1f} img/s over {len(imgs)} images "
              f"({n_people} people found; 512^2, {opt.nstack}-stack, single scale, "
              f"flip ensemble, {'trained ' + str(args.train_steps) + ' steps' if args.train_steps else 'random-init'})",
              flush=True)
