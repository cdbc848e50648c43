"""Device-matching layers without a GPU: the numpy decode of the kernels'
buffers, the CPU fallbacks of the two ops, ``assign_batch`` and the
``matching`` keyword of ``process_batch`` / ``PoseService``."""
import numpy as np
import pytest
import torch

from improved_body_parts_amd.config import GetConfig, InferenceParams, TrainingOpt
from improved_body_parts_amd.engine import (
    assign_batch, find_connections_batch, find_peaks_batch, find_people, process,
    process_batch)
from improved_body_parts_amd.models import NetworkEval
from improved_body_parts_amd.ops.assignment import (
    NO_PEAKS, OVERFLOW, canonical_peaks, decode_assignment, limb_match)

from test_inference_batch import synth_batch


@pytest.fixture(scope="module")
def config():
    return GetConfig("Canonical")


def _params():
    return InferenceParams().as_params_dict()[0]


# --------------------------------------------------------------------------
# decode_assignment on hand-built buffers
# --------------------------------------------------------------------------

def _hand_built():
    """One image, 3 parts (2 / 0 / 1 peaks), max_peaks 4, 3 limbs, max_part 2."""
    peaks = np.zeros((1, 4, 5), dtype=np.float32)
    peaks[0, 0] = [0, 10.5, 3.25, 0.9, 0.95]
    peaks[0, 1] = [0, 4.0, 7.0, 0.8, 0.85]
    peaks[0, 2] = [2, 6.0, 1.0, 0.7, 0.75]
    offsets = np.array([[0, 2, 2, 3]], dtype=np.int32)
    rows = np.full((1, 3, 2, 6), 99.0, dtype=np.float32)   # garbage past counts
    rows[0, 0, 0] = [1, 2, 0.625, 1, 0, 6.5]
    counts = np.array([[1, NO_PEAKS, 0]], dtype=np.int32)
    return peaks, offsets, rows, counts


def test_decode_assignment_structures():
    (all_peaks, connection_all, special_k), = decode_assignment(*_hand_built())
    # ids equal row indices; values are Python floats of the fp32 rows
    assert all_peaks == [[(10.5, 3.25, float(np.float32(0.9)), 0),
                          (4.0, 7.0, float(np.float32(0.8)), 1)],
                         [],
                         [(6.0, 1.0, float(np.float32(0.7)), 2)]]
    assert all(type(v) is float for sub in all_peaks for pk in sub for v in pk[:3])
    # a -1 count lands in special_k with []
    assert special_k == [1]
    assert isinstance(connection_all[1], list) and connection_all[1] == []
    # a count of 0 gives an empty (0, 6) array, rows come back float64
    assert connection_all[2].shape == (0, 6)
    assert connection_all[2].dtype == np.float64
    assert connection_all[0].dtype == np.float64
    np.testing.assert_array_equal(connection_all[0],
                                  [[1, 2, 0.625, 1, 0, 6.5]])


def test_decode_assignment_marks_overflow():
    peaks, offsets, rows, counts = _hand_built()
    counts[0, 0] = OVERFLOW
    (_, connection_all, special_k), = decode_assignment(peaks, offsets, rows, counts)
    assert connection_all[0] is None and special_k == [1]


# --------------------------------------------------------------------------
# CPU fallbacks of the ops
# --------------------------------------------------------------------------

def _encode(all_peaks_list, max_peaks, rng):
    """``all_peaks`` -> a peaks_batched-style buffer in shuffled (arrival) order."""
    buf = np.zeros((len(all_peaks_list), 1 + max_peaks, 5), dtype=np.float32)
    for n, all_peaks in enumerate(all_peaks_list):
        rows = [(c, pk[0], pk[1], pk[2], 0.0)
                for c, sub in enumerate(all_peaks) for pk in sub]
        rows = [rows[i] for i in rng.permutation(len(rows))]
        buf[n, 0, 0] = np.array([len(rows)], dtype=np.int32).view(np.float32)[0]
        buf[n, 1:1 + len(rows)] = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
    return torch.from_numpy(buf)


def test_ops_fall_back_to_host_on_cpu(config):
    """canonical_peaks -> limb_match -> decode_assignment on CPU tensors is the
    host path: same peaks, same connections, same special_k."""
    p = _params()
    maps = synth_batch(config)
    want_peaks = find_peaks_batch(maps, p, config)
    want_conns = find_connections_batch(want_peaks, maps, p, config)
    buf = _encode(want_peaks, 32, np.random.RandomState(0))
    peaks, offsets = canonical_peaks(buf, config.heat_layers)
    assert peaks.shape == (3, 32, 5) and peaks.dtype == torch.float32
    assert offsets.shape == (3, config.heat_layers + 1)
    assert offsets.dtype == torch.int32
    assert offsets[:, -1].tolist() == [12, 0, 6]
    rows, counts = limb_match(
        maps, peaks, offsets, config.limbs_conn,
        config.num_layers - config.paf_layers, p["mid_num"], p["thre2"],
        p["connect_ration"], max_part=8)
    assert rows.shape == (3, len(config.limbs_conn), 8, 6)
    assert counts.dtype == torch.int32
    got = decode_assignment(peaks.numpy(), offsets.numpy(), rows.numpy(),
                            counts.numpy())
    for n in range(3):
        all_peaks, connection_all, special_k = got[n]
        assert all_peaks == want_peaks[n]
        assert special_k == want_conns[n][1]
        for g, w in zip(connection_all, want_conns[n][0]):
            assert len(g) == len(w)
            if len(w):
                assert g.dtype == np.float64
                np.testing.assert_array_equal(g, w)
    # a part with more peaks than max_part is reported, not truncated
    _, counts1 = limb_match(
        maps, peaks, offsets, config.limbs_conn,
        config.num_layers - config.paf_layers, p["mid_num"], p["thre2"],
        p["connect_ration"], max_part=1)
    assert (counts1[0] == OVERFLOW).any() and not (counts1[1:] == OVERFLOW).any()
    with pytest.raises(ValueError):
        limb_match(maps, peaks, offsets, config.limbs_conn, 0, 20, 0.1, 0.8,
                   max_part=65)


def test_assign_batch_cpu_equals_host_path(config):
    p = _params()
    maps = synth_batch(config)
    peaks = find_peaks_batch(maps, p, config)
    conns = find_connections_batch(peaks, maps, p, config)
    got = assign_batch(maps, p, config)
    assert len(got) == 3
    people = []
    for n, (all_peaks, connection_all, special_k) in enumerate(got):
        assert all_peaks == peaks[n]
        assert special_k == conns[n][1]
        for g, w in zip(connection_all, conns[n][0]):
            np.testing.assert_array_equal(np.asarray(g), np.asarray(w))
        people.append(len(find_people(connection_all, special_k, all_peaks, p,
                                      config)[0]))
    assert people == [2, 0, 1]


# --------------------------------------------------------------------------
# the matching keyword
# --------------------------------------------------------------------------

def test_process_batch_matching_keyword(config):
    torch.manual_seed(0)
    model = NetworkEval(TrainingOpt(nstack=1, batch_size=1), config, bn=True).eval()
    p, mp = InferenceParams().as_params_dict()
    mp = dict(mp)
    mp["boxsize"] = 64
    rs = np.random.RandomState(5)
    imgs = [rs.rand(64, 64, 3).astype(np.float32),
            rs.rand(48, 64, 3).astype(np.float32)]
    host = process_batch(imgs, model, config, p, mp, matching="host")
    assert process_batch(imgs, model, config, p, mp) == host
    assert process_batch(imgs, model, config, p, mp, matching="device") == host
    assert process(imgs[0], model, config, p, mp, matching="device") == host[0]
    with pytest.raises(ValueError):
        process_batch(imgs, model, config, p, mp, matching="bogus")
    with pytest.raises(ValueError):
        process(imgs[0], model, config, p, mp, matching="bogus")


def test_pose_service_forwards_matching():
    from improved_body_parts_amd.serve import PoseService
    svc = PoseService(config_name="Canonical", nstack=1, device="cpu", bf16=False,
                      matching="device")
    svc.model_params = dict(svc.model_params)
    svc.model_params["boxsize"] = 64
    img = np.random.RandomState(6).rand(64, 64, 3).astype(np.float32)
    assert svc.matching == "device"
    assert svc.infer_many([img]) == [svc.infer(img)]
    with pytest.raises(ValueError):
        PoseService(config_name="Canonical", nstack=1, device="cpu", bf16=False,
                    matching="bogus")
