"""The grouped entry points off the HIP path: plain per-member calls with the
same results as the single entry points, every residual kind included."""
import torch
from torch import nn

from improved_body_parts_amd import ops


def _items():
    torch.manual_seed(0)
    items = []
    for cin, cout, k, size in [(8, 16, 3, 6), (16, 8, 1, 5), (8, 8, 3, 4)]:
        conv = nn.Conv2d(cin, cout, k, padding=(k - 1) // 2, bias=False)
        bn = nn.BatchNorm2d(cout).eval()
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
        items.append(dict(x=torch.randn(2, cin, size, size), conv=conv, bn=bn,
                          act=True))
    out = lambda it: torch.randn(2, it["conv"].out_channels,
                                 *it["x"].shape[2:])
    items[0].update(residual_post=out(items[0]), residual_post2=out(items[0]))
    items[1].update(residual=out(items[1]), residual_post=out(items[1]),
                    residual_post2=out(items[1]))
    items[2].update(bn=None, act=False)
    return items


def test_conv_bn_act_group_matches_single_calls():
    items = _items()
    with torch.no_grad():
        got = ops.conv_bn_act_group(items)
        a, b, c = items
        want = [
            ops.conv_bn_act(a["x"], a["conv"], a["bn"], act=True,
                            training=False, residual_post=a["residual_post"],
                            residual_post2=a["residual_post2"]),
            ops.conv_bn_add_act(b["x"], b["conv"], b["bn"], b["residual"],
                                act=True, training=False,
                                residual_post=b["residual_post"])
            + b["residual_post2"],
            ops.conv_bn_act(c["x"], c["conv"], None, act=False,
                            training=False),
        ]
    assert len(got) == 3
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    # and against the definition for the member with every residual
    with torch.no_grad():
        v = b["bn"](b["conv"](b["x"])) + b["residual"]
        v = torch.nn.functional.leaky_relu(v, 0.01)
        v = v + b["residual_post"] + b["residual_post2"]
    assert torch.allclose(got[1], v, atol=1e-6)


def test_conv_bn_act_group_empty_and_single():
    assert ops.conv_bn_act_group([]) == []
    it = _items()[:1]
    with torch.no_grad():
        (y,) = ops.conv_bn_act_group(it)
    assert y.shape == (2, 16, 6, 6)


def test_se_layer_group_matches_single_calls():
    torch.manual_seed(1)
    items = [(torch.randn(2, 32, s, s), nn.Linear(32, 2), nn.Linear(2, 32))
             for s in (5, 3, 1)]
    with torch.no_grad():
        got = ops.se_layer_group(items)
        want = [ops.se_layer(*it) for it in items]
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert ops.se_layer_group([]) == []
