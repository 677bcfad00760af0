"""Differentiable augmentation of discriminator inputs (DiffAugment, Zhao et al. 2020): the policy names and the transform of
include/agan.h (agan_diffaug_*) restated in plain torch ops.

`diffaug_reference` is the ORACLE of the HIP kernels (backend/functional.py: diffaug), not a second product path: any dtype, any
device, differentiable by autograd.  The training step never calls it.

Adaptive discriminator augmentation (Karras et al. 2020): with q and p every stage is applied per sample with probability p (the
gated entries agan_diffaug_gated_*), `AdaController` keeps p in device memory and steers it by two small HIP launches
(agan_ada_observe / agan_ada_update), and `ada_reference` restates the controller in Python integers and doubles, as its oracle.

The geometric stages of that paper (x-flip, quarter turns, isotropic scale, rotation, anisotropic scale) are ONE bilinear affine warp
in front of DiffAugment's stages (agan_geoaug_matrix / agan_affine_warp_*): `parse_geometry` names them, and
`geometry_matrices_reference`, `affine_warp_reference` and `geoaug_reference` are the oracle of those kernels."""
from __future__ import annotations

import math
import struct
from typing import Dict, Optional, Tuple, Union

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


def gate_masks(q: Tensor, p) -> Tensor:
    """bool [N, 3]: stage k of sample n passes its gate iff q[n, k] < p, compared in fp32 (include/agan.h); p: a number or a
    one-element tensor.  A NaN p passes nothing."""
    q32 = q.detach().to(torch.float32)
    p32 = p.detach().to(device=q32.device, dtype=torch.float32).reshape(()) if isinstance(p, Tensor) else torch.tensor(float(p), dtype=torch.float32, device=q32.device)
    return q32[:, :3] < p32


def diffaug_reference(x: Tensor, u: Tensor, policy: Union[str, int, None], q: Optional[Tensor] = None, p=None) -> Tensor:
    """The transform of include/agan.h on x [N, C, H, W] with uniforms u [N, 8]: colour, translation, cutout, each if its bit is set.
    The integer offsets come from the fp32 values of u (products formed in fp32) whatever x's dtype is.

    With q [N, 4] and p (the gated entries, agan_diffaug_gated_*): stage k runs for sample n iff its bit is set and q[n, k] < p in
    fp32; a sample whose gate is off keeps the stage's input, selected by torch.where, so its values pass unchanged."""
    policy = parse_policy(policy)
    if x.dim() != 4 or u.dim() != 2 or u.shape[0] != x.shape[0] or u.shape[1] != 8:
        raise ValueError(f"diffaug_reference: expected x [N, C, H, W] and u [N, 8], got {tuple(x.shape)} and {tuple(u.shape)}")
    if (q is None) != (p is None):
        raise ValueError("diffaug_reference: q and p come together or not at all")
    N, C, H, W = x.shape
    if q is not None and (q.dim() != 2 or tuple(q.shape) != (N, 4)):
        raise ValueError(f"diffaug_reference: q must be [{N}, 4], got {tuple(q.shape)}")
    gates = None if q is None else gate_masks(q, p).to(x.device)

    def gated(k: int, staged: Tensor, before: Tensor) -> Tensor:
        return staged if gates is None else torch.where(gates[:, k].view(N, 1, 1, 1), staged, before)

    z = x
    if policy & COLOR:
        z = gated(0, color_terms(z, u)[3], z)
    ys = torch.arange(H, device=x.device).view(1, H, 1)
    xs = torch.arange(W, device=x.device).view(1, 1, W)
    if policy & TRANSLATION:
        ty, tx = translation_offsets(u, H, W)
        sy, sx = ys - ty.view(N, 1, 1), xs - tx.view(N, 1, 1)                       # [N, H, 1], [N, 1, W]
        inside = ((sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)).view(N, 1, H, W)
        rows = sy.clamp(0, H - 1).view(N, 1, H, 1).expand(N, C, H, W)
        cols = sx.clamp(0, W - 1).view(N, 1, 1, W).expand(N, C, H, W)
        z = gated(1, torch.where(inside, z.gather(2, rows).gather(3, cols), torch.zeros((), dtype=z.dtype, device=z.device)), z)
    if policy & CUTOUT:
        oy, ox = cutout_offsets(u, H, W)
        ch, cw = int(0.5 * H + 0.5), int(0.5 * W + 0.5)
        y0, x0 = (oy - ch // 2).view(N, 1, 1), (ox - cw // 2).view(N, 1, 1)
        cut = ((ys >= y0) & (ys < y0 + ch) & (xs >= x0) & (xs < x0 + cw)).view(N, 1, H, W)
        z = gated(2, torch.where(cut, torch.zeros((), dtype=z.dtype, device=z.device), z), z)
    return z


# --------------------------------------------------------------------------------------------------------------
# geometric stages (include/agan.h: agan_geoaug_matrix / agan_affine_warp_*): ONE bilinear affine warp per tensor
# --------------------------------------------------------------------------------------------------------------
XFLIP, ROT90, SCALE, ROTATE, ANISO = 1, 2, 4, 8, 16              # include/agan.h: AGAN_GEOAUG_*
GEO_UNIFORMS = 16                                                # per sample: slots 0..4 stage values, 8..12 stage gates
_GEO_BITS = {"xflip": XFLIP, "rot90": ROT90, "scale": SCALE, "rotate": ROTATE, "aniso": ANISO}


def parse_geometry(geometry: Union[str, int, None]) -> int:
    """"xflip,rot90,scale,rotate,aniso" (any subset, any order; "" or None = nothing) -> the bit mask; an int in 0..31 passes
    through.  Separate from parse_policy: the geometric stages are one warp in front of DiffAugment's, with a mask of their own."""
    if geometry is None:
        return 0
    if isinstance(geometry, int) and not isinstance(geometry, bool):
        if not 0 <= geometry <= 31:
            raise ValueError(f"geometry {geometry} outside 0..31")
        return geometry
    if not isinstance(geometry, str):
        raise ValueError(f"geometry must be a string of names, an int or None, got {type(geometry).__name__}")
    mask = 0
    for name in (p.strip() for p in geometry.split(",")):
        if not name:
            continue
        if name not in _GEO_BITS:
            raise ValueError(f"unknown geometric augmentation {name!r}: expected a comma-separated subset of {', '.join(_GEO_BITS)}")
        mask |= _GEO_BITS[name]
    return mask


def geometry_names(geometry: int) -> str:
    """the inverse of parse_geometry, names in stage order"""
    geometry = parse_geometry(geometry)
    return ",".join(n for n, b in _GEO_BITS.items() if geometry & b)


def geometry_gates(g: Tensor, p) -> Tensor:
    """bool [N, 5]: stage k of sample n passes its gate iff g[n, 8 + k] < p, compared in fp32; a NaN p passes nothing"""
    g32 = g.detach().to(torch.float32)
    p32 = p.detach().to(device=g32.device, dtype=torch.float32).reshape(()) if isinstance(p, Tensor) else torch.tensor(float(p), dtype=torch.float32, device=g32.device)
    return g32[:, 8:13] < p32


def geometry_matrices_reference(g: Tensor, geometry: Union[str, int, None], p=None) -> Tensor:
    """M [N, 6] = (a, b, tx, c, d, ty) of include/agan.h (agan_geoaug_matrix) from the uniforms g [N, 16], in g's dtype: the product,
    left to right, of the applied stages' output -> source maps.  A stage applies iff its bit is set and -- with p -- g[n, 8 + k] < p
    in fp32; one that does not apply is skipped (torch.where keeps the running product, it is not multiplied by an identity).  The
    decisions (flip, quarter turn, gates) come from the fp32 values of g whatever its dtype is."""
    geometry = parse_geometry(geometry)
    if g.dim() != 2 or g.shape[1] != GEO_UNIFORMS:
        raise ValueError(f"geometry_matrices_reference: expected g [N, {GEO_UNIFORMS}], got {tuple(g.shape)}")
    N, dt, dev = g.shape[0], g.dtype, g.device
    g32 = g.detach().to(torch.float32)
    gates = None if p is None else geometry_gates(g, p)

    def on(k: int) -> Tensor:
        m = torch.full((N,), bool(geometry >> k & 1), device=dev)
        return m if gates is None else m & gates[:, k]

    def stage(rows) -> Tensor:
        return torch.stack([torch.stack(list(r), dim=1) for r in rows], dim=1)      # [N, 2, 2]

    def mul(L: Tensor, S: Tensor, m: Tensor) -> Tensor:
        a, b, c, d = L[:, 0, 0], L[:, 0, 1], L[:, 1, 0], L[:, 1, 1]
        P = stage(((a * S[:, 0, 0] + b * S[:, 1, 0], a * S[:, 0, 1] + b * S[:, 1, 1]),
                   (c * S[:, 0, 0] + d * S[:, 1, 0], c * S[:, 0, 1] + d * S[:, 1, 1])))
        return torch.where(m.view(N, 1, 1), P, L)

    one, zero = torch.ones(N, dtype=dt, device=dev), torch.zeros(N, dtype=dt, device=dev)
    L = stage(((one, zero), (zero, one)))
    L = mul(L, stage(((-one, zero), (zero, one))), on(0) & (g32[:, 0] >= 0.5))
    k = torch.clamp((4.0 * g32[:, 1]).to(torch.int64), max=3)
    c = torch.tensor([1, 0, -1, 0], dtype=dt, device=dev)[k]
    s = torch.tensor([0, 1, 0, -1], dtype=dt, device=dev)[k]
    L = mul(L, stage(((c, -s), (s, c))), on(1))
    sc = torch.exp2(0.7 * g[:, 2] - 0.35)
    L = mul(L, stage(((sc, zero), (zero, sc))), on(2))
    th = (2.0 * g[:, 3] - 1.0) * math.pi
    c, s = torch.cos(th), torch.sin(th)
    L = mul(L, stage(((c, -s), (s, c))), on(3))
    r = torch.exp2(0.7 * g[:, 4] - 0.35)
    L = mul(L, stage(((r, zero), (zero, 1.0 / r))), on(4))
    return torch.stack([L[:, 0, 0], L[:, 0, 1], zero, L[:, 1, 0], L[:, 1, 1], zero], dim=1)


def affine_warp_reference(x: Tensor, M: Tensor) -> Tensor:
    """The warp of include/agan.h (agan_affine_warp_fwd) on x [N, C, H, W] with M [N, 6], every operation in x's dtype and in the
    header's order: bilinear taps about the image centre, zero outside the image.  Differentiable in x by autograd (the transpose
    agan_affine_warp_bwd computes); M gets no gradient."""
    if x.dim() != 4 or M.dim() != 2 or tuple(M.shape) != (x.shape[0], 6):
        raise ValueError(f"affine_warp_reference: expected x [N, C, H, W] and M [N, 6], got {tuple(x.shape)} and {tuple(M.shape)}")
    N, C, H, W = x.shape
    dt, dev = x.dtype, x.device
    M = M.detach().to(device=dev, dtype=dt)
    cy, cx = (H - 1) / 2, (W - 1) / 2
    oy = (torch.arange(H, dtype=dt, device=dev) - cy).view(1, H, 1)
    ox = (torch.arange(W, dtype=dt, device=dev) - cx).view(1, 1, W)
    v = lambda i: M[:, i].view(N, 1, 1)
    sx = (v(0) * ox + v(1) * oy) + (v(2) * W + cx)
    sy = (v(3) * ox + v(4) * oy) + (v(5) * H + cy)
    x0f, y0f = torch.floor(sx), torch.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    x0 = x0f.clamp(-2, W).to(torch.int64)                                   # (anything outside [-1, W - 1] has no tap inside)
    y0 = y0f.clamp(-2, H).to(torch.int64)
    flat = x.reshape(N, C, H * W)
    out = torch.zeros_like(x)
    for j, wy in ((0, 1 - fy), (1, fy)):
        for i, wx in ((0, 1 - fx), (1, fx)):
            yy, xx = y0 + j, x0 + i
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).view(N, 1, H * W).expand(N, C, H * W)
            val = flat.gather(2, idx).view(N, C, H, W)
            out = out + torch.where(inside.view(N, 1, H, W), val * (wy * wx).view(N, 1, H, W), torch.zeros((), dtype=dt, device=dev))
    return out


def geoaug_reference(x: Tensor, g: Tensor, geometry: Union[str, int, None], p=None) -> Tensor:
    """matrices from the uniforms (in x's dtype), then the warp: what GanTrainStep(geometry=...) applies in front of DiffAugment"""
    return affine_warp_reference(x, geometry_matrices_reference(g.to(x.dtype), geometry, p))


# --------------------------------------------------------------------------------------------------------------
# the controller of p (include/agan.h: agan_ada_observe / agan_ada_update)
# --------------------------------------------------------------------------------------------------------------
ADA_WORDS = ("sum", "count", "calls", "adjustments", "p", "r_t")           # words 0..5 of the device state, in order


def _f32(v: float) -> float:
    """v rounded to fp32, as a Python float"""
    return struct.unpack("<f", struct.pack("<f", float(v)))[0]


def ada_new_state(p: float = 0.0) -> Dict:
    return {"sum": 0, "count": 0, "calls": 0, "adjustments": 0, "p": _f32(p), "r_t": 0.0}


def ada_tally(score, threshold: float = 0.5) -> Tuple[int, int]:
    """(#(score > threshold) - #(score < threshold), n) of agan_ada_observe, in Python integers; a NaN counts in n only.  The
    comparison is the fp32 one: scores and threshold are taken at their fp32 values."""
    vals = torch.as_tensor(score).detach().to(torch.float32).reshape(-1).cpu()
    t = torch.tensor(float(threshold), dtype=torch.float32)
    return int((vals > t).sum()) - int((vals < t).sum()), int(vals.numel())


def ada_reference(state: Dict, slots, interval: int, target: float, rate: float, p_max: float) -> Dict:
    """One agan_ada_update call in plain Python integers and doubles -- the ORACLE of the kernel, not a product path.  `state`: the
    dict of ada_new_state (words 0..5), changed in place and returned; `slots`: one (tally, n) pair per discriminator as ada_tally
    gives them, None or n == 0 for a discriminator that has not observed since the last call."""
    for slot in slots:
        if slot is not None and int(slot[1]) > 0:
            state["sum"] += int(slot[0])
            state["count"] += int(slot[1])
    state["calls"] += 1
    if state["calls"] < int(interval):
        return state
    total, count = state["sum"], state["count"]
    state["sum"] = state["count"] = state["calls"] = 0
    if count <= 0:
        return state
    r = float(total) / float(count)
    d = float(count) * float(rate)
    p = float(state["p"])
    if r > target:
        p = p + d
    elif r < target:
        p = p - d
    p = min(max(p, 0.0), float(p_max))
    state["p"], state["r_t"] = _f32(p), _f32(r)
    state["adjustments"] += 1
    return state


class AdaController:
    """The augmentation probability p in device memory and the two launches that steer it (adaptive discriminator augmentation,
    Karras et al. 2020): observe(i, score) tallies sign(D_i(real) - threshold) into discriminator i's slot, update() folds the slots
    into the window and, every `interval` calls, moves p by  (real scores in the window) * rate  towards r_t > target.  `self.p` is
    a float32 VIEW of the state's word 4: what backend.functional.diffaug is handed; nothing is read on the host until sync().

    rate = 1 / (kimg * 1000 * n_discriminators): every real image is scored by each discriminator, so count * rate is
    "real images seen in the window / (kimg * 1000)", the paper's step.  With target=None p is a constant: observe() and update()
    launch nothing.  The configuration is the constructor's; the state dicts carry words 0..5 only."""

    def __init__(self, device, n_discriminators: int, p: float = 0.0, target: Optional[float] = None, interval: int = 4,
                 kimg: float = 500.0, p_max: float = 1.0, threshold: float = 0.5):
        if not 1 <= int(n_discriminators) <= 4:
            raise ValueError(f"AdaController: {n_discriminators} discriminators outside 1..4")
        if not 0.0 < float(p_max) <= 1.0:
            raise ValueError(f"AdaController: p_max {p_max} outside (0, 1]")
        if not 0.0 <= float(p) <= float(p_max):
            raise ValueError(f"AdaController: p {p} outside [0, p_max = {p_max}]")
        if int(interval) < 1:
            raise ValueError(f"AdaController: interval {interval} below 1")
        if not float(kimg) > 0.0:
            raise ValueError(f"AdaController: kimg {kimg} is not positive")
        if target is not None and not -1.0 <= float(target) <= 1.0:
            raise ValueError(f"AdaController: target {target} outside [-1, 1], the range of r_t")
        self.n, self.interval, self.p_max, self.threshold = int(n_discriminators), int(interval), float(p_max), float(threshold)
        self.target = None if target is None else float(target)
        self.kimg = float(kimg)
        self.rate = 1.0 / (self.kimg * 1000.0 * self.n)
        self.p0 = _f32(p)
        self.state = torch.zeros(16, dtype=torch.int32, device=device)
        self.p = self.state[4:5].view(torch.float32)
        self.p.fill_(self.p0)

    @property
    def adaptive(self) -> bool:
        return self.target is not None

    def slot(self, i: int) -> Tensor:
        if not 0 <= i < self.n:
            raise IndexError(f"AdaController: discriminator {i} of {self.n}")
        return self.state[8 + 2 * i:10 + 2 * i]

    def observe(self, i: int, score: Tensor) -> None:
        if self.adaptive:
            from .backend import functional as HF
            HF.ada_observe_(score, self.slot(i), self.threshold)

    def update(self) -> None:
        if self.adaptive:
            from .backend import functional as HF
            HF.ada_update_(self.state, self.n, self.interval, self.target, self.rate, self.p_max)

    def _words(self) -> Dict:
        w = self.state[:6].cpu()                            # the one host read
        f = w[4:6].view(torch.float32)
        return {"sum": int(w[0]), "count": int(w[1]), "calls": int(w[2]), "adjustments": int(w[3]), "p": float(f[0]), "r_t": float(f[1])}

    def sync(self) -> Dict:
        w = self._words()
        return {"p": w["p"], "r_t": w["r_t"], "adjustments": w["adjustments"]}

    def state_dict(self) -> Dict:
        return self._words()

    def load_state_dict(self, sd: Dict) -> None:
        """Words 0..5; the observation slots restart empty.  The configuration stays the constructor's."""
        w = torch.zeros(16, dtype=torch.int32)
        for k, name in enumerate(ADA_WORDS[:4]):
            w[k] = int(sd[name])
        w[4:6].view(torch.float32).copy_(torch.tensor([float(sd["p"]), float(sd["r_t"])], dtype=torch.float32))
        self.state.copy_(w)

    def reset(self) -> None:
        self.state.zero_()
        self.p.fill_(self.p0)
