"""Per-shape timing of the convs whose epilogue dominates (batch-4 inference).

Every shape runs with the full fused epilogue the network uses: folded-BN
scale/shift + LeakyReLU, plus the pre-activation skip where the layer closes
a bottleneck. MIOpen runs the bare conv (no epilogue) as the yardstick.
Bytes = input + weights + output (+ residual), so the GB/s column can be set
against the measured HBM copy rate.
"""
import os, sys; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, time
import torch.nn.functional as F
from improved_body_parts_amd.ops import conv_kernels
CL = torch.channels_last


def bench(fn, iters=50, warm=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


shapes = [  # (n, cin, cout, hw, k, residual)
    (4, 256, 128, 128, 1, False),
    (4, 128, 256, 128, 1, True),
    (4, 384, 192, 64, 1, False),
    (4, 192, 384, 64, 1, True),
    (4, 256, 50, 128, 1, False),
    (4, 50, 256, 128, 1, False),
    (4, 512, 512, 16, 3, False),   # split-K
    (4, 640, 640, 8, 3, False),    # split-K
    (4, 256, 256, 128, 3, False),  # control: MFMA-bound
    (16, 256, 128, 128, 1, False),  # the shape quoted against the copy rate
]
for (n, cin, cout, hw, k, with_res) in shapes:
    x = torch.randn(n, cin, hw, hw, device="cuda").bfloat16().contiguous(memory_format=CL)
    w = (torch.randn(cout, cin, k, k, device="cuda") * 0.05).bfloat16()
    scale = torch.rand(cout, device="cuda") + 0.5
    shift = torch.randn(cout, device="cuda")
    res = (torch.randn(n, cout, hw, hw, device="cuda").bfloat16()
           .contiguous(memory_format=CL)) if with_res else None
    pad = (k - 1) // 2
    run = lambda: conv_kernels.conv_fwd(x, w, (1, 1), (pad, pad), (1, 1),
                                        scale, shift, res, True)
    assert run() is not None
    t_mfma = bench(run)
    wcl = w.contiguous(memory_format=CL)
    t_lib = bench(lambda: F.conv2d(x, wcl, None, 1, pad, 1))
    flops = 2 * n * hw * hw * cout * cin * k * k
    nbytes = 2 * (x.numel() + w.numel() + n * hw * hw * cout * (2 if with_res else 1))
    print(f"{(n,cin,cout,hw,k)}{'+res' if with_res else ''}: mfma {t_mfma*1e3:.1f} us "
          f"({flops/t_mfma/1e9:.0f} TF, {nbytes/t_mfma/1e6:.0f} GB/s) "
          f"| miopen {t_lib*1e3:.1f} us | ratio {t_lib/t_mfma:.2f}x")
