"""Person assembly without a GPU: the ``assembly`` keyword of ``process_batch``
/ ``process`` / ``PoseService``, the CPU path of ``assemble_people`` (which is
the oracle of the GPU tests) against ``find_people`` + ``subsets_to_keypoints``
on hand-made inputs, the branch each directed graph is meant to take, and
``decode_people``."""
import numpy as np
import pytest
import torch

from improved_body_parts_amd.config import GetConfig, InferenceParams, TrainingOpt
from improved_body_parts_amd.engine import (people_batch, process, process_batch)
from improved_body_parts_amd.models import NetworkEval
from improved_body_parts_amd.ops.assignment import (
    MAX_PEOPLE, OVERFLOW, assemble_people, decode_people)

from people_assemble_cases import (DIRECTED, TINY, check_invariants,
                                   directed_graph, encode, graph, keypoint_array,
                                   oracle, random_graph)
from test_inference_batch import synth_batch


@pytest.fixture(scope="module")
def config():
    return GetConfig("Canonical")


def _params(remove_recon=0):
    p = dict(InferenceParams().as_params_dict()[0])
    p["remove_recon"] = remove_recon
    return p


def _assemble(config, params, arrays, max_people=MAX_PEOPLE):
    return tuple(t.numpy() for t in assemble_people(
        *(torch.from_numpy(a) for a in arrays), config.limbs_conn,
        config.dt_gt_mapping, params["len_rate"], params["connection_tole"],
        params["remove_recon"], max_people))


# --------------------------------------------------------------------------
# the assembly keyword
# --------------------------------------------------------------------------

def test_process_batch_assembly_keyword(config):
    torch.manual_seed(0)
    model = NetworkEval(TrainingOpt(nstack=1, batch_size=1), config, bn=True).eval()
    p, mp = InferenceParams().as_params_dict()
    mp = dict(mp)
    mp["boxsize"] = 64
    rs = np.random.RandomState(5)
    imgs = [rs.rand(64, 64, 3).astype(np.float32),
            rs.rand(48, 64, 3).astype(np.float32)]
    host = process_batch(imgs, model, config, p, mp, matching="device",
                         assembly="host")
    assert process_batch(imgs, model, config, p, mp, matching="device") == host
    assert process_batch(imgs, model, config, p, mp, matching="device",
                         assembly="device") == host
    assert process(imgs[0], model, config, p, mp, matching="device",
                   assembly="device") == host[0]
    for call, arg in ((process_batch, imgs), (process, imgs[0])):
        with pytest.raises(ValueError):
            call(arg, model, config, p, mp, matching="device", assembly="bogus")
        with pytest.raises(ValueError):
            call(arg, model, config, p, mp, matching="host", assembly="device")
        with pytest.raises(ValueError):
            call(arg, model, config, p, mp, assembly="device")


def test_pose_service_forwards_assembly():
    from improved_body_parts_amd.serve import PoseService
    kw = dict(config_name="Canonical", nstack=1, device="cpu", bf16=False)
    svc = PoseService(matching="device", assembly="device", **kw)
    svc.model_params = dict(svc.model_params)
    svc.model_params["boxsize"] = 64
    img = np.random.RandomState(6).rand(64, 64, 3).astype(np.float32)
    assert svc.assembly == "device"
    assert svc.infer_many([img]) == [svc.infer(img)]
    assert PoseService(**kw).assembly == "host"
    with pytest.raises(ValueError):
        PoseService(matching="device", assembly="bogus", **kw)
    with pytest.raises(ValueError):
        PoseService(matching="host", assembly="device", **kw)


def test_people_batch_cpu_equals_host_chain(config):
    p = _params()
    maps = synth_batch(config)
    host = people_batch(maps, p, config, assembly="host")
    assert [len(r) for r in host] == [2, 0, 1]
    assert people_batch(maps, p, config, assembly="device") == host
    assert people_batch(maps, p, config) == host
    with pytest.raises(ValueError):
        people_batch(maps, p, config, assembly="bogus")


# --------------------------------------------------------------------------
# assemble_people on CPU tensors
# --------------------------------------------------------------------------

def _assert_equals_oracle(got, want, label=""):
    n_people, subset, keypoints = got
    for n, w in enumerate(want):
        if w is None:
            assert n_people[n] == OVERFLOW, f"{label} image {n}"
            continue
        sub, people, _ = w
        assert n_people[n] == len(sub), f"{label} image {n}"
        np.testing.assert_array_equal(subset[n, :len(sub)], sub)
        np.testing.assert_array_equal(keypoints[n, :len(sub)],
                                      keypoint_array(people))


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_case_takes_its_branch(config, name):
    """The oracle itself: each directed graph is decided by the branch it is
    named after, and the CPU op returns the oracle's rows."""
    _, _, remove_recon, branches, survivors = DIRECTED[name]
    p = _params(remove_recon)
    arrays = encode(config, [directed_graph(config, name)])
    (sub, people, stats), = oracle(config, p, arrays)
    assert stats["branches"] == branches
    assert len(sub) == survivors
    _assert_equals_oracle(_assemble(config, p, arrays), [(sub, people, stats)], name)


def test_directed_slot_values(config):
    """What the deciding branch leaves in the subset rows of the oracle."""
    def run(name):
        p = _params(DIRECTED[name][2])
        return oracle(config, p, encode(config, [directed_graph(config, name)]))[0][0]

    assert run("assign_too_long")[0, 14, 0] == -1
    assert run("overwrite")[0, 2].tolist() == [3, np.float32(0.9)]
    assert run("overwrite_too_long")[0, 2].tolist() == [2, np.float32(0.3)]
    assert run("keep")[0, 2].tolist() == [2, np.float32(0.9)]
    assert run("refresh")[0, 2].tolist() == [2, np.float32(0.9)]
    merged = run("merge")
    assert merged[0, -1].tolist() == [5, 6.0]
    assert [int(v) for v in merged[0, :-2, 0] if v >= 0] == [0, 1, 2, 3, 4]
    # the tiny confidence went through c + 1.0 and lost its low bits
    tiny = run("merge_tiny_conf")
    assert tiny[0, 6, 1] != TINY and tiny[0, 6, 1] == -1.0 + (TINY + 1.0)
    assert tiny[0, 5, 1] == tiny[0, 6, 1]
    # competition: nothing changes with remove_recon 0; with 1 the weaker of
    # (nose 0 in person 0, eye 1 in person 1) is cut out, either way round
    both = run("compete_keep_both")
    assert both[0, 0, 0] == 0 and both[1, 14, 0] == 5
    first = run("compete_remove_first")
    assert first[0, 0].tolist() == [-1, -1] and first[1, 14, 0] == 5
    assert first[0, -1, 0] == 2
    second = run("compete_remove_second")
    assert second[0, 0, 0] == 0 and second[1, 14].tolist() == [-1, -1]
    skipped = run("compete_both_better")
    assert skipped[0, 0, 0] == 0 and skipped[1, 14, 0] == 5
    assert run("prune_count")[0, 1, 0] == 3      # neck 1's person is the one left
    assert run("prune_mean")[0, 1, 0] == 3


def test_assemble_people_cpu_batch_and_overflow(config):
    """A batch: random graphs, an image with an overflowed limb, one with too
    many live rows for max_people, and an empty one."""
    rng = np.random.default_rng(7)
    p = _params(1)
    graphs = [random_graph(config, rng, 3, 0.4) for _ in range(4)]
    graphs.append(graph(config, {}, []))
    arrays = encode(config, graphs, overflow=[(1, 0)])
    want = oracle(config, p, arrays)
    assert want[1] is None and want[4][0].shape == (0, 20, 2)
    live = [w[2]["max_live"] for w in want if w is not None]
    assert max(live) > 2
    got = _assemble(config, p, arrays)
    assert got[0].dtype == np.int32 and got[0].shape == (5,)
    assert got[1].dtype == np.float64 and got[1].shape == (5, MAX_PEOPLE, 20, 2)
    assert got[2].dtype == np.float32 and got[2].shape == (5, MAX_PEOPLE, 17, 2)
    _assert_equals_oracle(got, want)
    for w in want:
        if w is not None:
            check_invariants(config, w[0])
    # max_people=2: images whose table held more than two rows overflow
    got2 = _assemble(config, p, arrays, max_people=2)
    assert got2[1].shape == (5, 2, 20, 2)
    want2 = [None if w is None or w[2]["max_live"] > 2 else w for w in want]
    assert sum(w is None for w in want2) > 1 and want2[4] is not None
    _assert_equals_oracle(got2, want2)
    # a peak id outside the image's peaks is an overflow, not an index
    bad = [a.copy() for a in arrays]
    k = int(np.nonzero(bad[3][0] > 0)[0][0])
    bad[2][0, k, 0, 1] = 60.0
    assert _assemble(config, p, bad)[0][0] == OVERFLOW


def test_assemble_people_validates(config):
    p = _params()
    arrays = [torch.from_numpy(a) for a in
              encode(config, [directed_graph(config, "new")])]
    args = (config.limbs_conn, config.dt_gt_mapping, 16.0, 0.7, 0)
    for bad in (0, MAX_PEOPLE + 1):
        with pytest.raises(ValueError):
            assemble_people(*arrays, *args, max_people=bad)
    with pytest.raises(ValueError):
        assemble_people(arrays[0].double(), *arrays[1:], *args)
    with pytest.raises(ValueError):
        assemble_people(arrays[0], arrays[1][:, :-1], *arrays[2:], *args)
    with pytest.raises(ValueError):
        assemble_people(*arrays[:3], arrays[3].long(), *args)
    with pytest.raises(ValueError):
        assemble_people(*arrays, config.limbs_conn[:-1], *args[1:])
    with pytest.raises(ValueError):
        assemble_people(*arrays, config.limbs_conn, {0: 17}, 16.0, 0.7, 0)


# --------------------------------------------------------------------------
# decode_people
# --------------------------------------------------------------------------

def test_decode_people_round_trip(config):
    n_people = np.array([2, OVERFLOW, 0], dtype=np.int32)
    keypoints = np.full((3, 4, 17, 2), 777.0, dtype=np.float32)   # garbage
    keypoints[0, 0] = np.arange(34, dtype=np.float32).reshape(17, 2) + 0.5
    keypoints[0, 1] = 0.0
    keypoints[0, 1, 3] = [12.25, 7.0]
    totals = np.full((3, 4), np.nan)
    totals[0, :2] = [4.0, -1.0]
    out = decode_people(n_people, keypoints, totals, config.dt_gt_mapping)
    assert out[1] is None and out[2] == []
    (kp0, s0), (kp1, s1) = out[0]
    assert s0 == 1 - 1.0 / 4.0 and s1 == 0.0
    assert kp0 == [(2.0 * g + 0.5, 2.0 * g + 1.5) for g in range(17)]
    assert kp1[3] == (12.25, 7.0) and kp1[0] == (0.0, 0.0)
    assert all(type(pt) is tuple for pt in kp0)
    # a COCO slot no part maps to is None, as subsets_to_keypoints leaves it
    mapping = dict(config.dt_gt_mapping)
    mapping[17] = None
    assert decode_people(n_people, keypoints, totals, mapping)[0][0][0][3] is None
