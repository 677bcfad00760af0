"""Layer plan of the Inception-v3 image-encoder trunk (networks/cnn_encoder.py::CNNEncoder) for the library's kernels.

Pure Python (no torch, no device): the list of every resize, conv, pool of the trunk in execution order, each with its geometry,
the tensors it reads and writes, and the channel range it writes of its destination (the branches of a Mixed block write straight
into their slice of the block output: no concatenation).  backend/functional.py::inception_trunk runs it forward and, reversed,
backward; tests/test_host_inception_plan.py checks it against torch's shape rules on the CPU.

Tensors are named; `relu` marks a tensor whose every element is a ReLU output (every conv output, every Mixed block output).  In the
backward a kernel that writes the gradient of such a tensor multiplies it by ReLU'(tensor) -- each addend is masked, so the sum
of the gradient is masked exactly once (by linearity).  The max-pool slices of Mixed_6a / Mixed_7a hold maxima of ReLU outputs: their
positivity equals that of the pooled element the backward routes to, whose own mask the pool's backward applies, so the factor
there is the same 0 or 1.  A tensor several ops read gets its gradient as a launch-ordered sum: in the reversed plan the first
op to reach it writes (`accumulate` False), the others add.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

TRUNK_SIZE = 299          # cnn_encoder.py:75 -- every image is resized to 299x299
FEATURES = "Mixed_6e"     # [B, 768, 17, 17] -> emb_features
POOLED = "pooled"         # [B, 2048] -> emb_cnn_code


@dataclass
class Tensor:
    name: str
    C: int
    H: int
    W: int
    relu: bool


@dataclass
class Op:
    kind: str                       # "resize" | "conv" | "maxpool" | "avgpool" | "gap"
    src: str
    dst: str
    C: int                          # input channels read (conv: Cin; pools: channels)
    H: int
    W: int
    OH: int
    OW: int
    out_c0: int = 0                 # first channel of dst this op writes
    out_ctot: int = 0               # channels of dst
    name: str = ""                  # conv: module path of the _ConvBNReLU (e.g. "Mixed_5b.branch5x5_2")
    Cout: int = 0
    k: Tuple[int, int] = (1, 1)     # conv taps (KH, KW)
    s: Tuple[int, int] = (1, 1)     # conv stride (SH, SW)
    p: Tuple[int, int] = (0, 0)     # conv padding (PH, PW)
    accumulate: bool = False        # backward: add into the gradient of src (another op already wrote it)

    def flops(self, B: int) -> int:
        """algorithmic multiply-adds x 2 of the forward (convs only; the data gradient costs the same)"""
        if self.kind != "conv":
            return 0
        return 2 * B * self.Cout * self.OH * self.OW * self.C * self.k[0] * self.k[1]


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


@dataclass
class Plan:
    H: int
    W: int
    ops: List[Op] = field(default_factory=list)
    tensors: Dict[str, Tensor] = field(default_factory=dict)

    def convs(self) -> List[Op]:
        return [o for o in self.ops if o.kind == "conv"]

    def flops_per_image(self, backward: bool = True) -> int:
        f = sum(o.flops(1) for o in self.ops)
        return 2 * f if backward else f

    # ---- builder -----------------------------------------------------------------------------------------------------
    def _tensor(self, name, C, H, W, relu):
        if name in self.tensors:
            t = self.tensors[name]
            assert (t.C, t.H, t.W) == (C, H, W), f"{name}: {t} vs {(C, H, W)}"
            return t
        t = self.tensors[name] = Tensor(name, C, H, W, relu)
        return t

    def conv(self, name, src, dst, cout, k, s=1, p=0, out_c0=0, out_ctot=None):
        (kh, kw), (sh, sw), (ph, pw) = _pair(k), _pair(s), _pair(p)
        t = self.tensors[src]
        oh, ow = (t.H + 2 * ph - kh) // sh + 1, (t.W + 2 * pw - kw) // sw + 1
        ctot = cout if out_ctot is None else out_ctot
        self._tensor(dst, ctot, oh, ow, True)
        self.ops.append(Op("conv", src, dst, t.C, t.H, t.W, oh, ow, out_c0, ctot, name, cout, (kh, kw), (sh, sw), (ph, pw)))
        return dst

    def maxpool(self, src, dst, out_c0=0, out_ctot=None, relu=False):
        t = self.tensors[src]
        oh, ow = (t.H - 3) // 2 + 1, (t.W - 3) // 2 + 1
        ctot = t.C if out_ctot is None else out_ctot
        self._tensor(dst, ctot, oh, ow, relu)
        self.ops.append(Op("maxpool", src, dst, t.C, t.H, t.W, oh, ow, out_c0, ctot))
        return dst

    def avgpool(self, src, dst):
        t = self.tensors[src]
        self._tensor(dst, t.C, t.H, t.W, False)
        self.ops.append(Op("avgpool", src, dst, t.C, t.H, t.W, t.H, t.W, 0, t.C))
        return dst


def _mixed_a(P: Plan, blk: str, src: str, pool: int) -> str:
    out = blk
    ctot = 64 + 64 + 96 + pool
    P.conv(f"{blk}.branch1x1", src, out, 64, 1, out_c0=0, out_ctot=ctot)
    a = P.conv(f"{blk}.branch5x5_1", src, f"{blk}.b5_1", 48, 1)
    P.conv(f"{blk}.branch5x5_2", a, out, 64, 5, p=2, out_c0=64, out_ctot=ctot)
    b = P.conv(f"{blk}.branch3x3dbl_1", src, f"{blk}.d_1", 64, 1)
    b = P.conv(f"{blk}.branch3x3dbl_2", b, f"{blk}.d_2", 96, 3, p=1)
    P.conv(f"{blk}.branch3x3dbl_3", b, out, 96, 3, p=1, out_c0=128, out_ctot=ctot)
    q = P.avgpool(src, f"{blk}.pool")
    P.conv(f"{blk}.branch_pool", q, out, pool, 1, out_c0=224, out_ctot=ctot)
    return out


def _mixed_b(P: Plan, blk: str, src: str) -> str:
    cin = P.tensors[src].C
    ctot = 384 + 96 + cin
    P.conv(f"{blk}.branch3x3", src, blk, 384, 3, s=2, out_c0=0, out_ctot=ctot)
    b = P.conv(f"{blk}.branch3x3dbl_1", src, f"{blk}.d_1", 64, 1)
    b = P.conv(f"{blk}.branch3x3dbl_2", b, f"{blk}.d_2", 96, 3, p=1)
    P.conv(f"{blk}.branch3x3dbl_3", b, blk, 96, 3, s=2, out_c0=384, out_ctot=ctot)
    P.maxpool(src, blk, out_c0=480, out_ctot=ctot, relu=True)
    return blk


def _mixed_c(P: Plan, blk: str, src: str, c7: int) -> str:
    ctot = 768
    P.conv(f"{blk}.branch1x1", src, blk, 192, 1, out_c0=0, out_ctot=ctot)
    a = P.conv(f"{blk}.branch7x7_1", src, f"{blk}.s_1", c7, 1)
    a = P.conv(f"{blk}.branch7x7_2", a, f"{blk}.s_2", c7, (1, 7), p=(0, 3))
    P.conv(f"{blk}.branch7x7_3", a, blk, 192, (7, 1), p=(3, 0), out_c0=192, out_ctot=ctot)
    b = P.conv(f"{blk}.branch7x7dbl_1", src, f"{blk}.d_1", c7, 1)
    b = P.conv(f"{blk}.branch7x7dbl_2", b, f"{blk}.d_2", c7, (7, 1), p=(3, 0))
    b = P.conv(f"{blk}.branch7x7dbl_3", b, f"{blk}.d_3", c7, (1, 7), p=(0, 3))
    b = P.conv(f"{blk}.branch7x7dbl_4", b, f"{blk}.d_4", c7, (7, 1), p=(3, 0))
    P.conv(f"{blk}.branch7x7dbl_5", b, blk, 192, (1, 7), p=(0, 3), out_c0=384, out_ctot=ctot)
    q = P.avgpool(src, f"{blk}.pool")
    P.conv(f"{blk}.branch_pool", q, blk, 192, 1, out_c0=576, out_ctot=ctot)
    return blk


def _mixed_d(P: Plan, blk: str, src: str) -> str:
    cin = P.tensors[src].C
    ctot = 320 + 192 + cin
    a = P.conv(f"{blk}.branch3x3_1", src, f"{blk}.t_1", 192, 1)
    P.conv(f"{blk}.branch3x3_2", a, blk, 320, 3, s=2, out_c0=0, out_ctot=ctot)
    b = P.conv(f"{blk}.branch7x7x3_1", src, f"{blk}.s_1", 192, 1)
    b = P.conv(f"{blk}.branch7x7x3_2", b, f"{blk}.s_2", 192, (1, 7), p=(0, 3))
    b = P.conv(f"{blk}.branch7x7x3_3", b, f"{blk}.s_3", 192, (7, 1), p=(3, 0))
    P.conv(f"{blk}.branch7x7x3_4", b, blk, 192, 3, s=2, out_c0=320, out_ctot=ctot)
    P.maxpool(src, blk, out_c0=512, out_ctot=ctot, relu=True)
    return blk


def _mixed_e(P: Plan, blk: str, src: str) -> str:
    ctot = 2048
    P.conv(f"{blk}.branch1x1", src, blk, 320, 1, out_c0=0, out_ctot=ctot)
    a = P.conv(f"{blk}.branch3x3_1", src, f"{blk}.t_1", 384, 1)
    P.conv(f"{blk}.branch3x3_2a", a, blk, 384, (1, 3), p=(0, 1), out_c0=320, out_ctot=ctot)
    P.conv(f"{blk}.branch3x3_2b", a, blk, 384, (3, 1), p=(1, 0), out_c0=704, out_ctot=ctot)
    b = P.conv(f"{blk}.branch3x3dbl_1", src, f"{blk}.d_1", 448, 1)
    b = P.conv(f"{blk}.branch3x3dbl_2", b, f"{blk}.d_2", 384, 3, p=1)
    P.conv(f"{blk}.branch3x3dbl_3a", b, blk, 384, (1, 3), p=(0, 1), out_c0=1088, out_ctot=ctot)
    P.conv(f"{blk}.branch3x3dbl_3b", b, blk, 384, (3, 1), p=(1, 0), out_c0=1472, out_ctot=ctot)
    q = P.avgpool(src, f"{blk}.pool")
    P.conv(f"{blk}.branch_pool", q, blk, 192, 1, out_c0=1856, out_ctot=ctot)
    return blk


_PLANS: Dict[Tuple[int, int], Plan] = {}


def build_plan(H: int, W: int) -> Plan:
    """The trunk's plan for [B, 3, H, W] images (cached per input size)."""
    key = (int(H), int(W))
    if key in _PLANS:
        return _PLANS[key]
    P = Plan(*key)
    P._tensor("image", 3, H, W, False)
    P._tensor("x299", 3, TRUNK_SIZE, TRUNK_SIZE, False)
    P.ops.append(Op("resize", "image", "x299", 3, H, W, TRUNK_SIZE, TRUNK_SIZE, 0, 3))
    x = P.conv("Conv2d_1a_3x3", "x299", "Conv2d_1a_3x3", 32, 3, s=2)
    x = P.conv("Conv2d_2a_3x3", x, "Conv2d_2a_3x3", 32, 3)
    x = P.conv("Conv2d_2b_3x3", x, "Conv2d_2b_3x3", 64, 3, p=1)
    x = P.maxpool(x, "pool1")
    x = P.conv("Conv2d_3b_1x1", x, "Conv2d_3b_1x1", 80, 1)
    x = P.conv("Conv2d_4a_3x3", x, "Conv2d_4a_3x3", 192, 3)
    x = P.maxpool(x, "pool2")
    x = _mixed_a(P, "Mixed_5b", x, 32)
    x = _mixed_a(P, "Mixed_5c", x, 64)
    x = _mixed_a(P, "Mixed_5d", x, 64)
    x = _mixed_b(P, "Mixed_6a", x)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        x = _mixed_c(P, blk, x, c7)
    assert x == FEATURES
    x = _mixed_d(P, "Mixed_7a", x)
    x = _mixed_e(P, "Mixed_7b", x)
    x = _mixed_e(P, "Mixed_7c", x)
    t = P.tensors[x]
    P._tensor(POOLED, t.C, 1, 1, False)
    P.ops.append(Op("gap", x, POOLED, t.C, t.H, t.W, 1, 1, 0, t.C))
    # backward write/accumulate order: FEATURES is seeded by the external gradient first; then the reversed plan
    written = {FEATURES}
    for o in reversed(P.ops):
        o.accumulate = o.src in written
        written.add(o.src)
    _PLANS[key] = P
    return P


def slices(plan: Plan) -> Dict[str, List[Tuple[int, int]]]:
    """dst tensor -> [(c0, c1)] channel ranges written by the ops that produce it (in plan order)"""
    out: Dict[str, List[Tuple[int, int]]] = {}
    for o in plan.ops:
        n = o.Cout if o.kind == "conv" else o.C
        out.setdefault(o.dst, []).append((o.out_c0, o.out_c0 + n))
    return out


def saved_tensors(plan: Plan) -> List[str]:
    """tensors the backward reads: the ReLU outputs (their masks) -- everything else is freed after the forward"""
    return [n for n, t in plan.tensors.items() if t.relu]


def conv_count(plan: Optional[Plan] = None) -> int:
    return len((plan or build_plan(TRUNK_SIZE, TRUNK_SIZE)).convs())
