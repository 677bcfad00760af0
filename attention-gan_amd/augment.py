"""Differentiable augmentation of discriminator inputs (DiffAugment, Zhao et al. 2020): the policy names and the transform of
include/agan.h (agan_diffaug_*) restated in plain torch ops.

`diffaug_reference` is the ORACLE of the HIP kernels (backend/functional.py: diffaug), not a second product path: any dtype, any
device, differentiable by autograd.  The training step never calls it."""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch
from torch import Tensor

COLOR, TRANSLATION, CUTOUT = 1, 2, 4             # include/agan.h: AGAN_DIFFAUG_*
_BITS = {"color": COLOR, "translation": TRANSLATION, "cutout": CUTOUT}


def parse_policy(policy: Union[str, int, None]) -> int:
    """"color,translation,cutout" (any subset, any order; "" or None = nothing) -> the bit mask; an int in 0..7 passes through."""
    if policy is None:
        return 0
    if isinstance(policy, int) and not isinstance(policy, bool):
        if not 0 <= policy <= 7:
            raise ValueError(f"augmentation policy {policy} outside 0..7")
        return policy
    if not isinstance(policy, str):
        raise ValueError(f"augmentation policy must be a string of names, an int or None, got {type(policy).__name__}")
    mask = 0
    for name in (p.strip() for p in policy.split(",")):
        if not name:
            continue
        if name not in _BITS:
            raise ValueError(f"unknown augmentation {name!r}: expected a comma-separated subset of {', '.join(_BITS)}")
        mask |= _BITS[name]
    return mask


def policy_names(policy: int) -> str:
    """the inverse of parse_policy, names in stage order"""
    policy = parse_policy(policy)
    return ",".join(n for n, b in _BITS.items() if policy & b)


def translation_offsets(u: Tensor, H: int, W: int) -> Tuple[Tensor, Tensor]:
    """(ty, tx) int64 [N]: out[y][x] = z[y - ty][x - tx]"""
    u32 = u.detach().to(torch.float32)
    Sy, Sx = int(0.125 * H + 0.5), int(0.125 * W + 0.5)
    ty = torch.clamp((u32[:, 3] * float(2 * Sy + 1)).to(torch.int64), max=2 * Sy) - Sy
    tx = torch.clamp((u32[:, 4] * float(2 * Sx + 1)).to(torch.int64), max=2 * Sx) - Sx
    return ty, tx


def cutout_offsets(u: Tensor, H: int, W: int) -> Tuple[Tensor, Tensor]:
    """(oy, ox) int64 [N]: the cut covers rows oy - ch // 2 <= y < oy - ch // 2 + ch, ch = int(0.5 H + 0.5); columns alike"""
    u32 = u.detach().to(torch.float32)
    ch, cw = int(0.5 * H + 0.5), int(0.5 * W + 0.5)
    oy = torch.clamp((u32[:, 5] * float(H + 1 - ch % 2)).to(torch.int64), max=H - ch % 2)
    ox = torch.clamp((u32[:, 6] * float(W + 1 - cw % 2)).to(torch.int64), max=W - cw % 2)
    return oy, ox


def color_terms(x: Tensor, u: Tensor):
    """(v, w, M, z) of the colour stage, broadcastable against x [N, C, H, W]"""
    N = x.shape[0]
    uf = u.to(x.dtype)
    b = (uf[:, 0] - 0.5).view(N, 1, 1, 1)
    s = (2.0 * uf[:, 1]).view(N, 1, 1, 1)
    c = (uf[:, 2] + 0.5).view(N, 1, 1, 1)
    v = x + b
    m = v.mean(dim=1, keepdim=True)
    w = s * (v - m) + m
    M = w.mean(dim=(1, 2, 3), keepdim=True)
    return v, w, M, c * (w - M) + M


def diffaug_reference(x: Tensor, u: Tensor, policy: Union[str, int, None]) -> Tensor:
    """The transform of include/agan.h on x [N, C, H, W] with uniforms u [N, 8]: colour, translation, cutout, each if its bit is set.
    The integer offsets come from the fp32 values of u (products formed in fp32) whatever x's dtype is."""
    policy = parse_policy(policy)
    if x.dim() != 4 or u.dim() != 2 or u.shape[0] != x.shape[0] or u.shape[1] != 8:
        raise ValueError(f"diffaug_reference: expected x [N, C, H, W] and u [N, 8], got {tuple(x.shape)} and {tuple(u.shape)}")
    N, C, H, W = x.shape
    z = x
    if policy & COLOR:
        z = color_terms(z, u)[3]
    ys = torch.arange(H, device=x.device).view(1, H, 1)
    xs = torch.arange(W, device=x.device).view(1, 1, W)
    if policy & TRANSLATION:
        ty, tx = translation_offsets(u, H, W)
        sy, sx = ys - ty.view(N, 1, 1), xs - tx.view(N, 1, 1)                       # [N, H, 1], [N, 1, W]
        inside = ((sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)).view(N, 1, H, W)
        rows = sy.clamp(0, H - 1).view(N, 1, H, 1).expand(N, C, H, W)
        cols = sx.clamp(0, W - 1).view(N, 1, 1, W).expand(N, C, H, W)
        z = torch.where(inside, z.gather(2, rows).gather(3, cols), torch.zeros((), dtype=z.dtype, device=z.device))
    if policy & CUTOUT:
        oy, ox = cutout_offsets(u, H, W)
        ch, cw = int(0.5 * H + 0.5), int(0.5 * W + 0.5)
        y0, x0 = (oy - ch // 2).view(N, 1, 1), (ox - cw // 2).view(N, 1, 1)
        cut = ((ys >= y0) & (ys < y0 + ch) & (xs >= x0) & (xs < x0 + cw)).view(N, 1, H, W)
        z = torch.where(cut, torch.zeros((), dtype=z.dtype, device=z.device), z)
    return z
