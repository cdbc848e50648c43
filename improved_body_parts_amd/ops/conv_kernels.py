"""MFMA implicit-GEMM convolution dispatch.

The CDNA4 kernels (csrc/conv_mfma.hip) implement NHWC bf16 convolution as an
implicit GEMM on the bf16 matrix cores:
    C[M=N*Ho*Wo][N=Cout] = A[M][K=KH*KW*Cin] @ B[K][Cout]
with fwd, dgrad (stride-1: conv with 180-rotated transposed weights) and
split-K wgrad. Weight packs are cached against the weight's version counter.

Each entry point returns ``None`` when the shape is outside the kernel's
envelope, and the caller falls back to the library conv.
"""
from __future__ import annotations

import os

import torch

from ._backend import hip_extension
from ._cache import versioned

_CL = torch.channels_last

DISABLE = os.environ.get("IBP_AMD_DISABLE_MFMA_CONV") == "1"


def _supported(x, stride):
    """Envelope of the MFMA kernels: bf16, square stride. Any Cin (subpieces
    crossing filter-tap boundaries — the 7x7 Cin=3 stem — take the kernel's
    per-element gather path), any padding (Ho/Wo are passed explicitly)."""
    return not DISABLE and x.dtype == torch.bfloat16 \
        and stride[0] == stride[1]


def _cl(t):
    return None if t is None else t.contiguous(memory_format=_CL)


# epilogue: (scale, shift, residual, act, residual_post, residual_post2)
_NO_EPI = (None, None, None, False, None, None)


def _conv_args(x, pack, w_shape, stride, padding, dilation, epi=_NO_EPI,
               zs=1, out_hw=None):
    """One conv as the extension's forward entries take it: ``(x, pack, geom,
    *epi)`` with x and the residuals channels_last and ``geom`` the row ``[N,
    H, W, Cin, Cout, KH, KW, stride, pad_h, pad_w, dil_h, dil_w, Ho, Wo, zs]``.
    ``w_shape`` is ``(Cout, Cin, KH, KW)`` of the conv that runs, ``epi`` its
    epilogue in the order of ``_NO_EPI``; ``out_hw`` overrides the output size
    that follows from the padding (asymmetric pads, dgrad)."""
    x = x.contiguous(memory_format=_CL)
    n, cin, h, w_ = x.shape
    cout, _, kh, kw = w_shape
    if out_hw is None:
        out_hw = (
            (h + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1,
            (w_ + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1)
    geom = [n, h, w_, cin, cout, kh, kw, stride[0], padding[0], padding[1],
            dilation[0], dilation[1], out_hw[0], out_hw[1], zs]
    scale, shift, residual, act, residual_post, residual_post2 = epi
    return (x, pack, geom, scale, shift, _cl(residual), bool(act),
            _cl(residual_post), _cl(residual_post2))


def _pack_pair(weight: torch.Tensor):
    """Both packs of a weight, regenerated when its version changes.

    On GPU bf16 weights this is ONE pack_weight_kernel launch into two
    persistent buffers; weights change every optimizer step, so the previous
    per-pack eager flip/permute/reshape chains re-ran ~500 small kernels per
    training step (~1.5% in launch overhead alone)."""
    return versioned(weight, "pair", (weight._version,), _build_pair, weight)


def _build_pair(prev, weight):
    cout, cin, kh, kw = weight.shape
    w = weight.detach()
    use_kernel = w.is_cuda and w.dtype == torch.bfloat16 and w.is_contiguous()
    if use_kernel:
        if prev is not None and prev[2]:
            fwd_buf, dgr_buf = prev[0], prev[1]
        else:
            fwd_buf = torch.empty(cout, kh * kw * cin, dtype=torch.bfloat16,
                                  device=w.device)
            dgr_buf = torch.empty(cin, kh * kw * cout, dtype=torch.bfloat16,
                                  device=w.device)
        hip_extension().pack_conv_weight(w, fwd_buf, dgr_buf)
    else:
        wd = w.to(torch.bfloat16)
        fwd_buf = wd.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()
        dgr_buf = torch.flip(wd, dims=(2, 3)).permute(1, 2, 3, 0) \
            .reshape(cin, -1).contiguous()
    return fwd_buf, dgr_buf, use_kernel


def packed_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, kh, kw] -> bf16 [Cout][kh*kw*Cin] contiguous (N-major for
    the kernel's B-tile row loads)."""
    return _pack_pair(weight)[0]


def packed_weight_dgrad(weight: torch.Tensor) -> torch.Tensor:
    """Weights for dgrad-as-conv: rotate 180° spatially, swap Cin/Cout ->
    [Cin][kh*kw*Cout]."""
    return _pack_pair(weight)[1]


# ---------------------------------------------------------------------------
# 7x7 s2 stem as a space-to-depth 4x4 s1 conv
# ---------------------------------------------------------------------------
# The Cin=3 stem forces the kernel's per-element tap gather (Cin % 8 != 0).
# Rewriting x (N,3,H,W) as S (N,12->16,H/2,W/2) with channel
# c' = (py*2+px)*3 + c turns it into a 4x4 stride-1 conv over 16 channels
# (kh = 2*kh' + py - 1, effective pad (2 left, 1 right)) — every subpiece is
# tap-uniform and 16-B vectorizable. Same trick for wgrad; dgrad is never
# needed (the stem is the input layer).

def _is_stem(x, w_shape, stride, padding, dilation):
    return (w_shape[2] == 7 and w_shape[3] == 7
            and stride[0] == 2 and stride[1] == 2 and x.shape[1] == 3
            and padding[0] == 3 and padding[1] == 3
            and dilation[0] == 1 and dilation[1] == 1
            and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0)


def _stem_s2d_input(x):
    """(N,3,H,W) channels_last -> (N,16,H/2,W/2) channels_last (padded c')."""
    import torch.nn.functional as F
    n, _, h, w = x.shape
    v = x.contiguous(memory_format=_CL).permute(0, 2, 3, 1)  # N,H,W,3
    v = v.reshape(n, h // 2, 2, w // 2, 2, 3).permute(0, 1, 3, 2, 4, 5)
    v = v.reshape(n, h // 2, w // 2, 12)
    v = F.pad(v, (0, 4))                                     # c' 12..15 = 0
    return v.permute(0, 3, 1, 2)  # NCHW view over NHWC storage


_STEM_LUT = {}


def _stem_weight_lut(device):
    """Flat source indices: W'[c'][kh'][kw'] position backing W[c][kh][kw]."""
    lut = _STEM_LUT.get(device)
    if lut is not None:
        return lut
    import numpy as np
    src = np.zeros(3 * 7 * 7, np.int64)
    for c in range(3):
        for kh in range(7):
            for kw in range(7):
                py, kh2 = (kh + 1) & 1, (kh + 1) >> 1
                px, kw2 = (kw + 1) & 1, (kw + 1) >> 1
                cp = (py * 2 + px) * 3 + c
                src[(c * 7 + kh) * 7 + kw] = (cp * 4 + kh2) * 4 + kw2
    lut = torch.from_numpy(src).to(device)
    _STEM_LUT[device] = lut
    return lut


def _stem_pack_weight(_, weight):
    """[64,3,7,7] -> packed bf16 [64][K=4*4*16] for the s2d conv."""
    w = weight.detach().to(torch.bfloat16)
    cout = w.shape[0]
    wp = torch.zeros(cout, 16, 4, 4, dtype=w.dtype, device=w.device)
    wp.view(cout, -1)[:, _stem_weight_lut(w.device)] = w.reshape(cout, -1)
    # -> [cout][kh'*kw'*c'] (tap-major, channel fastest) like packed_weight
    return wp.permute(0, 2, 3, 1).reshape(cout, -1).contiguous()


def _stem_fwd(x, weight, epi):
    s = _stem_s2d_input(x)
    pack = versioned(weight, "s2d", (weight._version,), _stem_pack_weight,
                     weight)
    y = hip_extension().conv_mfma_fwd(*_conv_args(
        s, pack, (weight.shape[0], 16, 4, 4), (1, 1), (2, 2), (1, 1), epi,
        out_hw=s.shape[2:]))
    return y.permute(0, 3, 1, 2)


def _wgrad(x, dy, w_shape, stride, padding, dilation):
    x, dy = _cl(x), _cl(dy)
    n, cin, h, w_ = x.shape
    cout, _, kh, kw = w_shape
    return hip_extension().conv_mfma_wgrad(
        x, dy, n, h, w_, cin, cout, kh, kw, stride[0], padding[0], padding[1],
        dilation[0], dilation[1], dy.shape[2], dy.shape[3])


def _stem_wgrad(x, dy, w_shape):
    cout = w_shape[0]
    dwp = _wgrad(_stem_s2d_input(x), dy, (cout, 16, 4, 4), (1, 1), (2, 2),
                 (1, 1))
    lut = _stem_weight_lut(x.device)
    return dwp.reshape(cout, -1)[:, lut].reshape(cout, 3, 7, 7)


def conv_fwd(x, weight, stride, padding, dilation,
             scale=None, shift=None, residual=None, act=False,
             residual_post=None, residual_post2=None):
    """MFMA conv forward; with scale/shift/residual/act set, the folded-BN
    (+residual +leaky) epilogue runs inside the conv kernel — the whole
    Conv+BN+LeakyReLU module is ONE kernel on the inference path.
    ``residual_post``/``residual_post2`` are added AFTER the activation (the
    hourglass up1+deconv1 join and the cross-stack feature-cache add)."""
    if not _supported(x, stride):
        return None
    epi = (scale, shift, residual, act, residual_post, residual_post2)
    if _is_stem(x, weight.shape, stride, padding, dilation):
        return _stem_fwd(x, weight, epi)
    y = hip_extension().conv_mfma_fwd(*_conv_args(
        x, packed_weight(weight), weight.shape, stride, padding, dilation,
        epi))
    return y.permute(0, 3, 1, 2)  # NHWC buffer -> NCHW view (channels_last)


def conv_fwd_group(members):
    """Several INDEPENDENT conv forwards in one grouped launch per 8 members
    (plus one grouped split-K combine). ``members`` is a list of dicts with
    the :func:`conv_fwd` arguments (``x weight stride padding dilation`` and
    the optional ``scale shift residual act residual_post residual_post2``).
    Every member runs the plan it would get alone, so each output equals the
    single call bit for bit. Returns the outputs in order, or ``None`` when a
    member is outside the grouped envelope (the caller then issues the
    members one by one)."""
    # one list per argument of conv_mfma_fwd; plain appends (docs/KERNELS.md)
    cols = [[] for _ in range(9)]
    for m in members:
        x, weight = m["x"], m["weight"]
        stride, padding, dilation = m["stride"], m["padding"], m["dilation"]
        if not _supported(x, stride) \
                or _is_stem(x, weight.shape, stride, padding, dilation):
            return None
        row = _conv_args(
            x, packed_weight(weight), weight.shape, stride, padding, dilation,
            (m.get("scale"), m.get("shift"), m.get("residual"), m.get("act"),
             m.get("residual_post"), m.get("residual_post2")))
        for col, v in zip(cols, row):
            col.append(v)
    ys = hip_extension().conv_mfma_fwd_grouped(*cols)
    return [y.permute(0, 3, 1, 2) for y in ys]


# ---------------------------------------------------------------------------
# nearest-x2 upsample folded into the 3x3 conv that follows it
# ---------------------------------------------------------------------------
# A 3x3 conv over a nearest-x2 image multiplies each low-resolution pixel by
# two or three weights and adds the products. Per output parity (py, px) the
# layer is a 2x2 conv over the low-resolution map:
#   y[n, 2i+py, 2j+px] = sum_{a,b} E[py][px][a][b] . x_low[n, i+a-(1-py), j+b-(1-px)]
#   E[py][px][a][b]    = sum_{kh in R(py,a)} sum_{kw in R(px,b)} W[kh][kw]
#   R(0,0)={0}  R(0,1)={1,2}  R(1,0)={0,1}  R(1,1)={2}
# with zeros outside the low-resolution map (the full-resolution zero padding
# lands on low-resolution index -1 / H). 4/9 of the MACs, no upsampled tensor.

_UPFOLD_ROWS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}


def upfold_weight_reference(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> [4, Cout, 2, 2, Cin] folded weights in the
    weight's dtype, parity ``py*2+px`` outermost. Pure torch, any device;
    each sum runs from zero in the accumulation dtype (fp32 for bf16/fp16
    weights, else the weight's own) with kh ascending, then kw — the order of
    ``pack_upfold_weight_kernel`` — and is rounded once."""
    cout, cin, kh, kw = weight.shape
    assert kh == 3 and kw == 3
    acc_t = torch.float32 if weight.dtype in (torch.bfloat16, torch.float16) \
        else weight.dtype
    w = weight.detach().to(acc_t)
    out = torch.zeros(4, cout, 2, 2, cin, dtype=acc_t, device=weight.device)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    acc = out[py * 2 + px, :, a, b]
                    for r in _UPFOLD_ROWS[(py, a)]:
                        for c in _UPFOLD_ROWS[(px, b)]:
                            acc += w[:, :, r, c]
    return out.to(weight.dtype)


def upfold_packed_weight(weight: torch.Tensor) -> torch.Tensor:
    """bf16 [4][Cout][4*Cin] folded packs of a 3x3 weight, one
    ``pack_upfold_weight_kernel`` launch per weight version."""
    return versioned(weight, "upfold", (weight._version,), _upfold_pack,
                     weight)


def _upfold_pack(_, weight):
    w = weight.detach().to(torch.bfloat16)
    cout, cin = w.shape[:2]
    if w.is_cuda:
        out = torch.empty(4, cout, 4 * cin, dtype=torch.bfloat16,
                          device=w.device)
        hip_extension().pack_upfold_weight(w.contiguous(), out)
        return out
    return upfold_weight_reference(w).reshape(4, cout, 4 * cin)


def upfold_supported(x, weight, stride, padding, dilation) -> bool:
    """Envelope of :func:`upfold_fwd`: bf16 CUDA input, 3x3 stride-1 pad-1
    undilated conv, Cin % 64 == 0 (every K-chunk inside one tap) and
    Cout % 8 == 0 (16-byte stores)."""
    cout, cin, kh, kw = weight.shape
    return (not DISABLE and x.is_cuda and x.dtype == torch.bfloat16
            and (kh, kw) == (3, 3) and tuple(stride) == (1, 1)
            and tuple(padding) == (1, 1) and tuple(dilation) == (1, 1)
            and x.shape[1] == cin and cin % 64 == 0 and cout % 8 == 0)


def upfold_fwd(x_low, weight, scale=None, shift=None, act=False,
               residual_post=None, residual_post2=None):
    """``conv_fwd(upsample2x_nearest(x_low), weight, pad 1, ...)`` without the
    upsampled tensor: four parity 2x2 convs in one grouped launch, each
    storing its own pixels of the full-resolution output. The folded weights
    carry one more bf16 rounding than the 3x3 pack (docs/KERNELS.md)."""
    x = _cl(x_low)
    n, cin, h, w_ = x.shape
    cout = weight.shape[0]
    post = []
    for r in (residual_post, residual_post2):
        if r is not None:
            assert tuple(r.shape) == (n, cout, 2 * h, 2 * w_), \
                f"residual {tuple(r.shape)} is not the upsampled output shape"
            r = _cl(r).permute(0, 2, 3, 1)
        post.append(r)
    # the layer's geometry row: H x W is the low resolution, Ho x Wo twice it
    geom = [n, h, w_, cin, cout, 3, 3, 1, 1, 1, 1, 1, 2 * h, 2 * w_, 1]
    y = hip_extension().conv_mfma_upfold_fwd(
        x.permute(0, 2, 3, 1), upfold_packed_weight(weight), geom, scale,
        shift, act, *post)
    return y.permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------
# two 1x1 convs whose outputs are only added: one conv over both inputs
# ---------------------------------------------------------------------------
# act(sa.(Wa.a) + ta + sb.(Wb.b) + tb) = act([sa.Wa | sb.Wb] . [a | b] + (ta + tb))
# One GEMM over K = Ca + Cb whose A rows come from two tensors (the kernel's
# CAT gather); the per-channel scales move into the weight rows, which costs
# one more bf16 rounding of the weights, and the second conv's output is never
# written (docs/KERNELS.md, "Two-source 1x1 conv").

def cat_weight_reference(wa, wb, scale_a=None, scale_b=None, shift_a=None,
                         shift_b=None):
    """``(pack, shift)`` of the two-source conv, pure torch on the weights'
    device: pack bf16 ``[Cout][Ca + Cb]`` with source a first, every element
    ``float(w) * scale[co]`` (one fp32 multiply, scale 1 when absent) rounded
    to bf16 once; shift fp32 ``shift_a + shift_b`` (absent = 0). Bit-equal to
    ``pack_cat_weight_kernel``."""
    cout = wa.shape[0]
    assert wb.shape[0] == cout and tuple(wa.shape[2:]) == (1, 1) \
        and tuple(wb.shape[2:]) == (1, 1)
    halves = []
    for w, s in ((wa, scale_a), (wb, scale_b)):
        h = w.detach().to(torch.bfloat16).float().reshape(cout, -1)
        if s is not None:
            h = h * s.detach().float().reshape(cout, 1)
        halves.append(h.to(torch.bfloat16))
    zero = torch.zeros(cout, dtype=torch.float32, device=wa.device)
    shift = (zero if shift_a is None else shift_a.detach().float()) \
        + (zero if shift_b is None else shift_b.detach().float())
    return torch.cat(halves, dim=1).contiguous(), shift


def cat_pack(prev, wa, wb, scale_a, scale_b, shift_a, shift_b):
    """``(pack, ones, shift)`` for :func:`conv_cat_fwd`: one
    ``pack_cat_weight_kernel`` launch on GPU bf16 weights (into ``prev``'s
    buffers when given), the host reference elsewhere. ``ones`` is the unit
    scale the split-K combine needs beside a shift."""
    cout = wa.shape[0]
    k = wa.shape[1] + wb.shape[1]
    wa, wb = wa.detach(), wb.detach()
    if wa.is_cuda and wa.dtype == torch.bfloat16 and wb.dtype == wa.dtype:
        if prev is not None:
            pack, ones, shift = prev
        else:
            pack = torch.empty(cout, k, dtype=torch.bfloat16, device=wa.device)
            ones = torch.ones(cout, dtype=torch.float32, device=wa.device)
            shift = torch.empty(cout, dtype=torch.float32, device=wa.device)
        hip_extension().pack_cat_weight(wa.contiguous(), wb.contiguous(),
                                        scale_a, scale_b, shift_a, shift_b,
                                        pack, shift)
        return pack, ones, shift
    pack, shift = cat_weight_reference(wa, wb, scale_a, scale_b, shift_a,
                                       shift_b)
    return pack, torch.ones_like(shift), shift


def cat_supported(a, weight_a, b, weight_b) -> bool:
    """Envelope of :func:`conv_cat_fwd`: bf16 CUDA inputs over the same
    pixels, 1x1 weights with equal Cout, Ca % 64 == 0 (every K-chunk inside
    one source). The second source may have any width."""
    return (not DISABLE and a.is_cuda and b.is_cuda
            and a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16
            and tuple(weight_a.shape[2:]) == (1, 1)
            and tuple(weight_b.shape[2:]) == (1, 1)
            and weight_a.shape[0] == weight_b.shape[0]
            and a.shape[1] == weight_a.shape[1]
            and b.shape[1] == weight_b.shape[1]
            and weight_a.shape[1] % 64 == 0
            and a.shape[0] == b.shape[0] and a.shape[2:] == b.shape[2:])


def conv_cat_fwd(a, weight_a, b, weight_b, pack, scale=None, shift=None,
                 act=False, residual_post=None, residual_post2=None):
    """``act(scale * (pack . [a | b]) + shift) (+ residual_post [+2])`` — the
    1x1 convs ``weight_a`` over ``a`` and ``weight_b`` over ``b`` as ONE conv
    over K = Ca + Cb with ``pack`` from :func:`cat_pack` (the weights are
    passed for their shapes only)."""
    a = a.contiguous(memory_format=_CL)
    n, ca, h, w_ = a.shape
    cout = weight_a.shape[0]
    geom = [n, h, w_, ca, cout, 1, 1, 1, 0, 0, 1, 1, h, w_, 1]
    y = hip_extension().conv_mfma_fwd(
        a, pack, geom, scale, shift, None, bool(act), _cl(residual_post),
        _cl(residual_post2), b.contiguous(memory_format=_CL))
    return y.permute(0, 3, 1, 2)


def conv_dgrad(dy, weight, x_shape, stride, padding, dilation):
    """dx = stride-1 conv of the (virtually) zero-dilated dy with 180-rotated
    transposed weights; pad' = dil*(K-1) - pad, gather stride zs = stride."""
    if not _supported(dy, stride):
        return None
    cout, _, kh, kw = weight.shape
    pad = (dilation[0] * (kh - 1) - padding[0],
           dilation[1] * (kw - 1) - padding[1])
    if pad[0] < 0 or pad[1] < 0:
        return None
    # the conv that runs maps dy's Cout channels to x's Cin
    dx = hip_extension().conv_mfma_fwd(*_conv_args(
        dy, packed_weight_dgrad(weight), (x_shape[1], cout, kh, kw), (1, 1),
        pad, dilation, zs=stride[0], out_hw=x_shape[2:]))
    return dx.permute(0, 3, 1, 2)


def conv_wgrad(x, dy, w_shape, stride, padding, dilation):
    """Hand-written MFMA weight gradient (csrc/conv_wgrad.hip).

    The contraction runs over M = N*Ho*Wo — the strided dimension of both
    NHWC operands — so fragments are staged through LDS [64 m][16 ch]
    subtiles with a permuted row order and consumed with gfx950's hardware
    transpose read ``ds_read_b64_tr_b16`` (round 1 left this on MIOpen
    igemm_wrw; the builtin ``__builtin_amdgcn_ds_read_tr16_b64_v4i16``
    makes the layout tractable). Any KHxKW/stride/dilation; bf16 only."""
    if not _supported(x, stride) or dy.dtype != torch.bfloat16:
        return None
    if _is_stem(x, w_shape, stride, padding, dilation):
        return _stem_wgrad(x, dy, w_shape)
    return _wgrad(x, dy, w_shape, stride, padding, dilation)
