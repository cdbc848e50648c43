"""Grouped SE launch: five maps in one launch per stage, each output
bit-identical to the single inference path (same per-problem arithmetic and
reduction order)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from improved_body_parts_amd.ops import _backend, spatial

CL = torch.channels_last


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    assert _backend.hip_available(), \
        "HIP extension must be built and loaded on a GPU box"


def _items(sizes, c, n, seed):
    torch.manual_seed(seed)
    items = []
    for s in sizes:
        x = torch.randn(n, c, s, s).cuda().bfloat16().contiguous(
            memory_format=CL)
        fc1 = torch.nn.Linear(c, c // 16).cuda().bfloat16()
        fc2 = torch.nn.Linear(c // 16, c).cuda().bfloat16()
        items.append((x, fc1, fc2))
    return items


@pytest.mark.parametrize("sizes,c", [
    pytest.param([32, 16, 8, 4, 2], 64, id="five-scales-c64"),
    pytest.param([12, 6, 3], 320, id="two-channel-blocks-odd-sizes"),
    pytest.param([4] * 9, 64, id="list-of-9"),
])
def test_grouped_se_equals_single(sizes, c):
    items = _items(sizes, c, 2, seed=len(sizes) + c)
    with torch.no_grad():
        want = [spatial.se_layer_hip(*it) for it in items]
        junk = torch.full((16 << 20,), float("nan"), device="cuda")
        del junk
        got = spatial.se_layer_group_hip(items)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.stride() == w.stride()
        assert not torch.isnan(g.float()).any()
        assert torch.equal(g, w), f"problem {i} ({sizes[i]}^2) differs"
    # against the definition, loosely: the gate is a sigmoid in (0, 1)
    x0 = items[0][0].float()
    assert (got[0].float().abs() <= x0.abs() + 1e-6).all()


def test_grouped_se_switch_restores_single_calls(monkeypatch):
    items = _items([8, 4], 64, 2, seed=3)
    monkeypatch.setenv("IBP_SE_GROUP", "0")
    ext = _backend.hip_extension()
    called = []
    real = ext.se_layer_grouped
    monkeypatch.setattr(ext, "se_layer_grouped",
                        lambda *a: called.append(1) or real(*a))
    with torch.no_grad():
        off = spatial.se_layer_group_hip(items)
        assert not called
        monkeypatch.setenv("IBP_SE_GROUP", "1")
        on = spatial.se_layer_group_hip(items)
    assert called == [1]
    for a, b in zip(off, on):
        assert torch.equal(a, b)
