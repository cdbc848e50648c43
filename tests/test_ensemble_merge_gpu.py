"""Device tests of the batched inference path: the fused ensemble_merge kernel
against the torch chain, the peak and limb kernels against the host path,
single-image predict against the per-image torch chain, and process_batch
against per-image process."""
import numpy as np
import pytest
import torch

from improved_body_parts_amd.config import GetConfig, InferenceParams, TrainingOpt
from improved_body_parts_amd.engine import (
    find_connections, find_connections_batch, find_peaks, find_peaks_batch,
    find_people, predict, process, process_batch, subsets_to_keypoints)
from improved_body_parts_amd.models import NetworkEval
from improved_body_parts_amd.ops.ensemble import ensemble_merge

from inference_oracle import reference_predict
from test_inference_batch import (PERSON_A, PERSON_B,
                                  assert_same_connections, synth_batch,
                                  synth_maps)

pytestmark = pytest.mark.gpu

C = 50
# (h4, w4, sh, sw, H, W) at stride 4: odd W, up- and downscaling, a crop inside
# the padding, and the identity second pass
SHAPES = [(16, 16, 60, 52, 48, 41), (16, 32, 50, 120, 75, 180),
          (16, 16, 64, 64, 64, 64)]
ATOL = 2e-5   # 10x the fp32 torch chain's own error against the fp64 composition


@pytest.fixture(scope="module")
def config():
    return GetConfig("Canonical")


def _perm(seed=0):
    perm = np.random.RandomState(seed).permutation(C)
    assert not np.array_equal(perm, np.arange(C))
    return perm


def _views(n, h4, w4, dtype, seed):
    """(2n, C, h4, w4) values exactly representable in ``dtype``: the fp32 CPU
    copy for the oracle and the channels_last device tensor as the model emits."""
    g = torch.Generator().manual_seed(seed)
    v = torch.rand(2 * n, C, h4, w4, generator=g).to(dtype)
    dev = v.cuda().contiguous(memory_format=torch.channels_last)
    return v.float(), dev


@pytest.fixture(scope="module")
def oracle():
    """CPU torch-chain results, computed once per case and never modified."""
    cache = {}

    def get(shape, dtype, n, seed, scale):
        key = (shape, dtype, n, seed, scale)
        if key not in cache:
            h4, w4, sh, sw, H, W = shape
            cpu, _ = _views(n, h4, w4, dtype, seed)
            cache[key] = ensemble_merge(cpu, _perm(), 4, (sh, sw), (H, W),
                                        scale=scale)
        return cache[key]
    return get


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_torch_chain(shape, dtype, oracle):
    h4, w4, sh, sw, H, W = shape
    _, dev = _views(2, h4, w4, dtype, seed=1)
    got = ensemble_merge(dev, _perm(), 4, (sh, sw), (H, W), scale=1.0)
    assert got.shape == (2, C, H, W) and got.dtype == torch.float32
    assert got.is_contiguous()
    want = oracle(shape, dtype, 2, 1, 1.0)
    err = float((got.cpu() - want).abs().max())
    print(f"ensemble_merge {shape} {dtype}: max abs err {err:.3e}")
    assert err <= ATOL
    # no atomics, one owner per element: bitwise repeatable
    again = ensemble_merge(dev, _perm(), 4, (sh, sw), (H, W), scale=1.0)
    assert torch.equal(got, again)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_accumulates(shape, oracle):
    h4, w4, sh, sw, H, W = shape
    _, dev1 = _views(2, h4, w4, torch.float32, seed=1)
    _, dev2 = _views(2, h4, w4, torch.float32, seed=2)
    # garbage in the buffer: the first run must overwrite it, not add to it
    acc = torch.full((2, C, H, W), 7.0, device="cuda")
    ensemble_merge(dev1, _perm(), 4, (sh, sw), (H, W), scale=0.5, out=acc)
    ensemble_merge(dev2, _perm(), 4, (sh, sw), (H, W), scale=0.5, out=acc,
                   accumulate=True)
    want = oracle(shape, torch.float32, 2, 1, 0.5) + \
        oracle(shape, torch.float32, 2, 2, 0.5)
    err = float((acc.cpu() - want).abs().max())
    print(f"ensemble_merge accumulate {shape}: max abs err {err:.3e}")
    assert err <= ATOL


def test_kernel_single_image_and_channel_order(oracle):
    shape = SHAPES[0]
    h4, w4, sh, sw, H, W = shape
    _, dev = _views(1, h4, w4, torch.bfloat16, seed=3)
    got = ensemble_merge(dev, _perm(), 4, (sh, sw), (H, W))
    assert float((got.cpu() - oracle(shape, torch.bfloat16, 1, 3, 1.0))
                 .abs().max()) <= ATOL
    # a channel subset in another order, written into a slice of a larger buffer
    order = list(range(30, 50)) + list(range(0, 10))
    perm = np.random.RandomState(4).permutation(len(order))
    cpu, _ = _views(1, h4, w4, torch.bfloat16, seed=3)
    want = ensemble_merge(cpu, perm, 4, (sh, sw), (H, W), chan_order=order)
    buf = torch.zeros(3, len(order), H, W, device="cuda")
    ensemble_merge(dev, perm, 4, (sh, sw), (H, W), out=buf[1:2], chan_order=order)
    assert float((buf[1].cpu() - want[0]).abs().max()) <= ATOL
    assert float(buf[0].abs().max()) == 0 and float(buf[2].abs().max()) == 0


# --------------------------------------------------------------------------
# peaks_batched
# --------------------------------------------------------------------------

def _params():
    return InferenceParams().as_params_dict()[0]


def _rows(all_peaks):
    return [[(pk[0], pk[1], pk[2]) for pk in sub] for sub in all_peaks]


def test_peaks_batched_matches_find_peaks(config):
    p = _params()
    maps = synth_batch(config)
    got = find_peaks_batch(maps.cuda(), p, config)
    assert len(got) == 3
    totals = []
    for n in range(3):
        # host path as oracle
        want = find_peaks(maps[n, :config.heat_layers].permute(1, 2, 0), p, config)
        for c, (g, w) in enumerate(zip(got[n], want)):
            assert len(g) == len(w), f"image {n} channel {c}"
            for pg, pw in zip(g, w):
                assert abs(pg[0] - pw[0]) <= 1e-4 and abs(pg[1] - pw[1]) <= 1e-4
                assert abs(pg[2] - pw[2]) <= 1e-5
                assert pg[3] == pw[3]
        totals.append(sum(len(s) for s in got[n]))
    assert totals == [12, 0, 6]


def test_peaks_batched_cap_is_per_image(config):
    p = _params()
    small = {0: (60.0, 70.0), 1: (60.0, 85.0), 2: (50.0, 85.0)}
    maps = torch.stack([synth_maps(config, [PERSON_A, PERSON_B]),
                        synth_maps(config, []),
                        synth_maps(config, [small])]).cuda()
    full = find_peaks_batch(maps, p, config)
    capped = find_peaks_batch(maps, p, config, max_peaks=4)
    assert sum(len(s) for s in full[0]) == 12
    for n in range(3):
        assert sum(len(s) for s in capped[n]) <= 4
        for c in range(config.heat_layers):
            allowed = _rows(full[n])[c]
            for row in _rows(capped[n])[c]:
                assert row in allowed, f"image {n} channel {c}: foreign row {row}"
    assert sum(len(s) for s in capped[0]) == 4
    assert capped[1] == full[1] and capped[2] == full[2]


# --------------------------------------------------------------------------
# full pipeline
# --------------------------------------------------------------------------

def _by_peak_id(result):
    """Each limb's connection rows ordered by their first peak id. The two
    people of image 0 are copies of each other, so their limb scores tie to
    within rounding; the kernel's serial fp32 sum and the host's numpy mean
    may rank such a pair either way, and the rank of equal scores is not part
    of the result (the 1-1 matching makes the first id unique per limb)."""
    conns, special_k = result
    return [c[np.argsort(c[:, 0])] if len(c) else c for c in conns], special_k


def test_batched_postprocessing_on_device(config):
    p = _params()
    maps = synth_batch(config)
    n_heat = config.num_layers - config.paf_layers
    peaks = find_peaks_batch(maps.cuda(), p, config)
    conns = find_connections_batch(peaks, maps.cuda(), p, config)
    people = []
    for n in range(3):
        # host path on the CPU maps as oracle
        heat = maps[n, :n_heat].permute(1, 2, 0)
        paf = maps[n, n_heat:].permute(1, 2, 0)
        ref_peaks = find_peaks(heat, p, config)
        ref_conn = find_connections(ref_peaks, paf, 128, p, config)
        assert_same_connections(_by_peak_id(conns[n]), _by_peak_id(ref_conn))
        sub_g, cand_g = find_people(*conns[n], peaks[n], p, config)
        sub_w, cand_w = find_people(*ref_conn, ref_peaks, p, config)
        np.testing.assert_allclose(sub_g, sub_w, atol=1e-4)
        np.testing.assert_allclose(cand_g, cand_w, atol=1e-4)
        kg = subsets_to_keypoints(sub_g, cand_g, config)
        kw = subsets_to_keypoints(sub_w, cand_w, config)
        assert len(kg) == len(kw)
        people.append(len(kg))
    assert people == [2, 0, 1]


def _bf16_model(config):
    torch.manual_seed(0)
    model = NetworkEval(TrainingOpt(nstack=1, batch_size=1), config,
                        bn=True).cuda().bfloat16()
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.float()
    return model.eval()


def test_predict_single_matches_torch_chain_on_device(config):
    """One image ends in the fused ensemble_merge kernel; the oracle is the
    per-image eager chain on the device. At scale 1 the same-size bicubic
    resize is an exact identity, so both feed the network a bit-identical
    (2, h, w, 3) batch and only the merge differs. 96x80 pads to 128x128 and
    exercises the crop. Bound: the kernel's ATOL times max(1, max|oracle|)."""
    model = _bf16_model(config)
    p, mp = InferenceParams().as_params_dict()
    p, mp = dict(p), dict(mp)
    p["scale_search"] = [1.0]
    p["rotation_search"] = [0.0]
    rs = np.random.RandomState(2)
    for (H, W), boxsize in (((64, 64), 64), ((96, 80), 96)):
        mp["boxsize"] = boxsize
        img = rs.rand(H, W, 3).astype(np.float32)
        heat, paf = predict(img, model, config, p, mp)
        h_ref, p_ref = reference_predict(img, model, config, p, mp)
        assert heat.is_cuda and heat.dtype == torch.float32
        assert heat.shape == h_ref.shape and paf.shape == p_ref.shape
        err = max(float((heat - h_ref).abs().max()),
                  float((paf - p_ref).abs().max()))
        mag = max(float(h_ref.abs().max()), float(p_ref.abs().max()))
        print(f"predict vs torch chain on device {H}x{W}: max abs diff "
              f"{err:.3e}, max |oracle| {mag:.3e}")
        assert err <= ATOL * max(1.0, mag)


def test_process_batch_matches_process_on_device(config):
    model = _bf16_model(config)
    p, mp = InferenceParams().as_params_dict()
    mp = dict(mp)
    mp["boxsize"] = 64
    rs = np.random.RandomState(1)
    imgs = [rs.rand(64, 64, 3).astype(np.float32) for _ in range(3)]
    got = process_batch(imgs, model, config, p, mp)
    want = [process(i, model, config, p, mp) for i in imgs]
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert isinstance(g, list) and len(g) == len(w)
        for (kg, sg), (kw, sw) in zip(g, w):
            assert len(kg) == len(kw) == 17
