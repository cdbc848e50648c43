"""Per-image torch-chain ensemble forward, kept as the tests' oracle for
``predict`` / ``predict_batch``. It shares no code with the package's
pipeline (one image at a time, (H, W, C) layout, eager flip-merge, upsample,
crop and resize); nothing in the package may import it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from improved_body_parts_amd.config import InferenceParams


def _to_device_image(image, device, dtype=torch.float32):
    """(H, W, 3) numpy uint8/float or torch tensor -> (H, W, 3) fp32 in [0,1]."""
    if isinstance(image, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(image))
    else:
        t = image
    t = t.to(device=device)
    if t.dtype == torch.uint8:
        t = t.to(dtype) / 255.0
    else:
        t = t.to(dtype)
    return t


def _resize_hwc(t, out_h, out_w):
    """Bicubic resize of an (H, W, C) tensor (reference cv2.INTER_CUBIC)."""
    x = t.permute(2, 0, 1)[None]
    x = F.interpolate(x, size=(out_h, out_w), mode="bicubic", align_corners=False)
    return x[0].permute(1, 2, 0)


def _rotate_hwc(t, angle_deg, inverse=False):
    """Rotate an (H, W, C) tensor about its center (reference cv2.warpAffine
    with getRotationMatrix2D; the reference passes (h/2, w/2) as the cv2
    center which is an x/y mix-up for non-square inputs — inputs there are
    always padded square; we rotate about the true center)."""
    if angle_deg == 0:
        return t
    a = math.radians(angle_deg if not inverse else -angle_deg)
    cos, sin = math.cos(a), math.sin(a)
    # grid_sample samples the INPUT at the transformed output coordinates, so
    # the theta matrix is the inverse rotation; normalized coords are square
    # here only if H == W, so fold the aspect ratio in explicitly.
    H, W = t.shape[0], t.shape[1]
    # aspect handling in normalized coords: x' = cos*x - sin*(y*H/W);
    # y' = sin*(x*W/H) + cos*y
    theta = torch.tensor([[cos, -sin * H / W, 0.0],
                          [sin * W / H, cos, 0.0]],
                         dtype=torch.float32, device=t.device)
    x = t.permute(2, 0, 1)[None].float()
    grid = F.affine_grid(theta[None], x.shape, align_corners=False)
    out = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros",
                        align_corners=False)
    return out[0].permute(1, 2, 0).to(t.dtype)


@torch.no_grad()
def reference_predict(image, model, config, params=None, model_params=None,
                      device=None, dtype=None):
    """Run the ensemble forward (reference evaluate.py:83-161).

    Returns ``(heatmap_avg, paf_avg)`` as (H, W, C) fp32 torch tensors at the
    ORIGINAL image resolution, on ``device`` (stays on GPU when one is used).
    """
    if params is None or model_params is None:
        p, mp = InferenceParams().as_params_dict()
        params = params or p
        model_params = model_params or mp
    if device is None:
        device = next(model.parameters()).device
    if dtype is None:
        dtype = next(model.parameters()).dtype

    img = _to_device_image(image, device)
    H, W = img.shape[0], img.shape[1]
    flip_heat = torch.as_tensor(np.asarray(config.flip_heat_ord), device=device,
                                dtype=torch.long)
    flip_paf = torch.as_tensor(np.asarray(config.flip_paf_ord), device=device,
                               dtype=torch.long)
    n_heat = config.num_layers - config.paf_layers  # 18 + 2
    n_paf = config.paf_layers
    heatmap_avg = torch.zeros(H, W, n_heat, device=device)
    paf_avg = torch.zeros(H, W, n_paf, device=device)

    multiplier = [s * model_params["boxsize"] / H for s in params["scale_search"]]
    rotations = params.get("rotation_search", [0.0])
    pad_to = model_params["max_downsample"]
    pad_value = model_params["padValue"] / 255.0

    for scale in multiplier:
        # cap absurdly large upscales (reference evaluate.py:94-96)
        if scale * H > 2600 or scale * W > 3800:
            scale = min(2600 / H, 3800 / W)
        for angle in rotations:
            sh, sw = max(int(round(H * scale)), 1), max(int(round(W * scale)), 1)
            scaled = _resize_hwc(img, sh, sw)
            pad_h = (pad_to - sh % pad_to) % pad_to
            pad_w = (pad_to - sw % pad_to) % pad_to
            padded = F.pad(scaled.permute(2, 0, 1), (0, pad_w, 0, pad_h),
                           value=pad_value).permute(1, 2, 0)
            if angle != 0:
                padded = _rotate_hwc(padded, angle)
            flipped = torch.flip(padded, dims=[1])
            batch = torch.stack([padded, flipped]).to(dtype)     # (2, h, w, 3) NHWC

            out = model(batch)
            out = out[-1][0].float()                             # last stack, scale 0
            paf = out[:, :n_paf]
            heat = out[:, n_paf:n_paf + n_heat]

            # flip ensemble: mirror the flipped copy back and permute L/R channels
            paf_f = torch.flip(paf[1], dims=[-1])[flip_paf]
            heat_f = torch.flip(heat[1], dims=[-1])[flip_heat]
            paf = (paf[0] + paf_f) * 0.5
            heat = (heat[0] + heat_f) * 0.5

            # x stride upsample, unrotate, unpad, resize to original
            ph, pw = padded.shape[0], padded.shape[1]
            up = F.interpolate(torch.cat([heat, paf])[None], size=(ph, pw),
                               mode="bicubic", align_corners=False)[0]
            if angle != 0:
                up = _rotate_hwc(up.permute(1, 2, 0), angle, inverse=True) \
                    .permute(2, 0, 1)
            up = up[:, :sh, :sw]
            up = F.interpolate(up[None], size=(H, W), mode="bicubic",
                               align_corners=False)[0].permute(1, 2, 0)

            n_runs = len(multiplier) * len(rotations)
            heatmap_avg += up[..., :n_heat] / n_runs
            paf_avg += up[..., n_heat:] / n_runs

    return heatmap_avg, paf_avg
