"""Shared by tests/test_input_host.py and tests/test_gpu_input.py: the float64 restatement of the input contract
(fgvc_amd.datasets.preprocess_tapvid_frames: the same formulas with every tensor in float64, the interpolation included), the kernel's
cases and the frames they run on.  Data generation and a restatement of the project's own function; nothing of the reference."""
import numpy as np
import torch

from fgvc_amd.datasets import _M_RGB2XYZ, _WHITE_D65
from tests.golden.clips import moving_texture


def rgb_to_lab_f64(rgb: torch.Tensor) -> torch.Tensor:
    """datasets.rgb_to_lab with every tensor in float64: (..., 3, h, w) in [0, 1] -> L*a*b*."""
    x = rgb.to(torch.float64)
    lin = torch.where(x > 0.04045, ((x + 0.055) / 1.055).clamp_min(0) ** 2.4, x / 12.92)
    r, g, b = lin.unbind(-3)
    xyz = [(m[0] * r + m[1] * g + m[2] * b) / w for m, w in zip(_M_RGB2XYZ, _WHITE_D65)]
    f = [torch.where(t > 0.008856, t.clamp_min(1e-12) ** (1.0 / 3.0), 7.787 * t + 16.0 / 116.0) for t in xyz]
    L = torch.where(xyz[1] > 0.008856, 116.0 * f[1] - 16.0, 903.3 * xyz[1])
    return torch.stack([L, 500.0 * (f[0] - f[1]), 200.0 * (f[1] - f[2])], -3)


def preprocess_f64(frames_uint8: torch.Tensor, size=None) -> torch.Tensor:
    """datasets.preprocess_tapvid_frames in float64 on the CPU: (T, h0, w0, 3) uint8 -> (T, 3, h, w) float64."""
    x = frames_uint8.cpu().permute(0, 3, 1, 2).to(torch.float64)
    if size is not None and tuple(x.shape[-2:]) != tuple(size):
        x = torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    lab = rgb_to_lab_f64((x / 255.0).clamp(0, 1))
    mean = torch.tensor([50.0, 0.0, 0.0], dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor([50.0, 127.0, 127.0], dtype=torch.float64).view(1, 3, 1, 1)
    return (lab - mean) / std


def texture_u8(T, h, w, seed, drift=(3, -2)) -> torch.Tensor:
    """(T, h, w, 3) uint8: tests/golden/clips.py's moving texture shifted to 0..255 (pure integer arithmetic: the same bytes everywhere)."""
    x = moving_texture(T, h, w, seed, drift=drift).astype(np.int16) + 128
    return torch.from_numpy(np.ascontiguousarray(x.astype(np.uint8).transpose(0, 2, 3, 1)))


def dark_cube() -> torch.Tensor:
    """(1, 108, 128, 3): all 24^3 triples with channels in 0..23 -- the linear branch of the sRGB transfer (x <= 0.04045 <=> v <= 10) next
    to its power branch, and the linear branch of the Lab function (t <= 0.008856) next to its cube root."""
    v = torch.arange(24 ** 3)
    rgb = torch.stack([v // 576, (v // 24) % 24, v % 24], -1).to(torch.uint8)
    return rgb.reshape(1, 108, 128, 3).contiguous()


def lattice_cube() -> torch.Tensor:
    """(1, 64, 64, 3): the 16-level lattice 0, 17, .., 255 of the full colour cube."""
    v = torch.arange(16 ** 3)
    rgb = (torch.stack([v // 256, (v // 16) % 16, v % 16], -1) * 17).to(torch.uint8)
    return rgb.reshape(1, 64, 64, 3).contiguous()


def greys() -> torch.Tensor:
    """(1, 16, 16, 3): the 256 greys."""
    return torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).repeat(1, 1, 1, 3).contiguous()


# name -> (frames (T, h0, w0, 3) uint8, size (h, w) | None, pad (left, right, top, bottom)): the smallest shapes at which the kernel can go
# wrong -- a width that is no multiple of the lane's 4 columns nor 4-byte aligned per row, a down- and an up-scale (the edge clamp on all
# four sides), one source pixel, pads that shift the lane's columns off the frame's, and colours on both branches of both piecewise functions
def kernel_cases():
    return {
        "same_2x19x23": (texture_u8(2, 19, 23, 1), None, (0, 0, 0, 0)),
        "down_3x37x53_to_24x40": (texture_u8(3, 37, 53, 2), (24, 40), (0, 0, 0, 0)),
        "up_2x19x23_to_41x47": (texture_u8(2, 19, 23, 3), (41, 47), (0, 0, 0, 0)),
        "one_pixel_to_3x5": (torch.tensor([201, 96, 13], dtype=torch.uint8).view(1, 1, 1, 3), (3, 5), (0, 0, 0, 0)),
        "same_2x16x20_pad": (texture_u8(2, 16, 20, 4), None, (1, 2, 0, 1)),
        "down_2x16x20_to_9x13_pad": (texture_u8(2, 16, 20, 5), (9, 13), (0, 3, 1, 0)),
        "dark_cube": (dark_cube(), None, (0, 0, 0, 0)),
        "lattice_cube": (lattice_cube(), None, (0, 0, 0, 0)),
        "greys": (greys(), None, (0, 0, 0, 0)),
    }


ERROR_FLOOR = 2.0 ** -22       # guards a case on which the torch chain happens to be exact
