"""Bit-exact sweep of the general 2-D conv (include/agan.h: agan_conv2d_fwd / agan_conv2d_dgrad) over every conv geometry of the
Inception-v3 image-encoder trunk, forward and data gradient.

Operands are drawn from small dyadic grids (integers |k| <= 4 times a power of two per tensor), so every product and partial sum is
exact in fp32 in any order: the kernel output must equal torch's CPU float64 result bit for bit.  The first table runs each geometry at
its real spatial size with reduced channel counts; the second runs one production-size case per geometry family with bias, the ReLU
epilogue, the ReLU mask, channel-slice input and output and `accumulate`.  The library's launch observer (agan_timer_arm /
agan_timer_last_kernel) names the kernel every call ran: the k-table MFMA gather's general instantiation.
"""
import ctypes
import importlib
from ctypes import byref

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")

EX, EW, EDY, EB = -2, -3, -1, -5

# B, Cin, H, W, Cout, (KH, KW), (SH, SW), (PH, PW)   -- the trunk's geometries at their real spatial sizes, few channels
GEOMS = [
    (2, 3, 299, 299, 8, (3, 3), (2, 2), (0, 0)),      # Conv2d_1a (dgrad: 3 output channels on a padded tile)
    (2, 8, 35, 35, 16, (3, 3), (2, 2), (0, 0)),       # Mixed_6a branch3x3 / dbl_3
    (2, 8, 17, 17, 16, (3, 3), (2, 2), (0, 0)),       # Mixed_7a
    (2, 8, 149, 149, 8, (3, 3), (1, 1), (0, 0)),      # Conv2d_2a
    (2, 8, 73, 73, 16, (3, 3), (1, 1), (0, 0)),       # Conv2d_4a
    (2, 8, 147, 147, 16, (3, 3), (1, 1), (1, 1)),     # Conv2d_2b
    (2, 8, 35, 35, 16, (3, 3), (1, 1), (1, 1)),       # Mixed_5b-d dbl_2/3, Mixed_6a dbl_2
    (2, 16, 8, 8, 16, (3, 3), (1, 1), (1, 1)),        # Mixed_7b/c dbl_2
    (2, 8, 35, 35, 16, (5, 5), (1, 1), (2, 2)),       # Mixed_5b-d branch5x5_2
    (2, 8, 17, 17, 16, (1, 7), (1, 1), (0, 3)),       # Mixed_6b-e, 7a
    (2, 8, 17, 17, 16, (7, 1), (1, 1), (3, 0)),
    (2, 16, 8, 8, 16, (1, 3), (1, 1), (0, 1)),        # Mixed_7b/c
    (2, 16, 8, 8, 16, (3, 1), (1, 1), (1, 0)),
    (2, 16, 73, 73, 8, (1, 1), (1, 1), (0, 0)),       # 1x1 everywhere
    (2, 16, 17, 17, 48, (1, 1), (1, 1), (0, 0)),
]

# production size, one per family, with every epilogue option: (geometry, in_c0, in_ctot, out_c0, out_ctot)
PROD = [
    ((4, 288, 35, 35, 384, (3, 3), (2, 2), (0, 0)), 0, 288, 0, 768),         # Mixed_6a branch3x3 into its slice
    ((4, 80, 73, 73, 192, (3, 3), (1, 1), (0, 0)), 0, 80, 0, 192),          # Conv2d_4a
    ((4, 448, 8, 8, 384, (3, 3), (1, 1), (1, 1)), 0, 448, 0, 384),          # Mixed_7b dbl_2
    ((4, 48, 35, 35, 64, (5, 5), (1, 1), (2, 2)), 0, 48, 64, 288),          # Mixed_5c branch5x5_2 into [64, 128)
    ((4, 160, 17, 17, 192, (7, 1), (1, 1), (3, 0)), 0, 160, 192, 768),      # Mixed_6c branch7x7_3
    ((4, 384, 8, 8, 384, (1, 3), (1, 1), (0, 1)), 16, 416, 320, 2048),     # Mixed_7b branch3x3_2a, sliced input too
    ((4, 768, 17, 17, 192, (1, 1), (1, 1), (0, 0)), 0, 768, 576, 768),      # Mixed_6b branch_pool
]


def grid(shape, e, gen, lim=4):
    return torch.randint(-lim, lim + 1, shape, generator=gen).double() * 2.0 ** e


def desc(g, in_c0=0, in_ctot=None, out_c0=0, out_ctot=None):
    B, cin, H, W, cout, k, s, p = g
    oh, ow = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
    d = L.Conv2dDesc(B, cin, H, W, cout, oh, ow, k[0], k[1], s[0], s[1], p[0], p[1], in_c0, in_ctot or cin, out_c0, out_ctot or cout)
    return d, oh, ow


class KernelLog:
    def __init__(self):
        self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
        L.call("agan_timer_create", ctypes.byref(self.e0))
        L.call("agan_timer_create", ctypes.byref(self.e1))
        self.name = ctypes.create_string_buffer(1024)

    def arm(self):
        L.call("agan_timer_arm", self.e0, self.e1)

    def last(self):
        torch.cuda.synchronize()
        L.call("agan_timer_last_kernel", self.name, 1024)
        return self.name.value.decode()


@pytest.fixture(scope="module")
def log():
    return KernelLog()


def run(g, log, *, bias=False, relu=False, mask=False, acc=False, in_c0=0, in_ctot=None, out_c0=0, out_ctot=None, seed=0):
    gen = torch.Generator().manual_seed(seed)
    B, cin, H, W, cout, k, s, p = g
    in_ctot, out_ctot = in_ctot or cin, out_ctot or cout
    d, oh, ow = desc(g, in_c0, in_ctot, out_c0, out_ctot)
    x = grid((B, in_ctot, H, W), EX, gen)
    w = grid((cout, cin) + k, EW, gen)
    b = grid((cout,), EB, gen, 16) if bias else None
    y0 = grid((B, out_ctot, oh, ow), EB, gen)                   # what the sliced output tensor holds outside this conv's channels
    dy = grid((B, out_ctot, oh, ow), EDY, gen)
    dx0 = grid((B, in_ctot, H, W), EDY - 3, gen)                # an earlier branch's gradient (accumulate)
    m = grid((B, in_ctot, H, W), 0, gen, 1) if mask else None  # the ReLU mask: {-1, 0, 1}
    # fp64 reference
    xs = x[:, in_c0:in_c0 + cin]
    ref = F.conv2d(xs, w, b, stride=s, padding=p)
    if relu:
        ref = ref.clamp_min(0)
    y_want = y0.clone()
    y_want[:, out_c0:out_c0 + cout] = ref
    gx = torch.nn.grad.conv2d_input(xs.shape, w, dy[:, out_c0:out_c0 + cout].contiguous(), stride=s, padding=p)
    if mask:
        gx = gx * (m[:, in_c0:in_c0 + cin] > 0)
    dx_want = dx0.clone() if acc else torch.zeros_like(dx0)
    if acc:
        dx_want[:, in_c0:in_c0 + cin] += gx
    else:
        dx_want[:, in_c0:in_c0 + cin] = gx
    # library
    wd = w.float().to(DEV)
    wkf, wkd = HF.conv2d_pack(wd, d, 0), HF.conv2d_pack(wd, d, 1)
    # (every device operand is bound to a name until the call returns: a temporary freed while the argument list is still being
    # evaluated could be handed to the next allocation -- the k-table -- and overwritten before the kernel reads it)
    y, xd, bd = y0.float().to(DEV), x.float().to(DEV), (b.float().to(DEV) if bias else None)
    ktf, ktd = HF.conv2d_ktable(d, 0, DEV), HF.conv2d_ktable(d, 1, DEV)
    dyd, md = dy.float().to(DEV), (m.float().to(DEV) if mask else None)
    log.arm()
    L.call("agan_conv2d_fwd", HF._p(xd), HF._p(wkf), HF._p(bd), HF._p(y), byref(d), HF._p(ktf), L.ACT_RELU if relu else L.ACT_NONE,
           None, 0, HF._stream())
    kf = log.last()
    dx = dx0.float().to(DEV) if acc else torch.full(dx0.shape, float("nan"), device=DEV)
    if not acc:
        dx[:, in_c0:in_c0 + cin] = 0          # (channels outside the slice keep whatever the tensor held)
        dx_want = torch.where(torch.arange(in_ctot).view(1, -1, 1, 1).expand_as(dx_want) < in_c0, torch.nan, dx_want)
        dx_want = torch.where(torch.arange(in_ctot).view(1, -1, 1, 1).expand_as(dx_want) >= in_c0 + cin, torch.nan, dx_want)
    log.arm()
    L.call("agan_conv2d_dgrad", HF._p(dyd), HF._p(wkd), HF._p(dx), byref(d), HF._p(ktd), HF._p(md), int(acc), None, 0, HF._stream())
    kd = log.last()
    return (y.cpu().double(), y_want), (dx.cpu().double(), dx_want), (kf, kd)


def exact(got, want):
    return torch.equal(torch.nan_to_num(got, nan=12345.0), torch.nan_to_num(want, nan=12345.0))


@pytest.mark.parametrize("g", GEOMS, ids=lambda g: f"{g[1]}x{g[2]}x{g[3]}-k{g[5][0]}x{g[5][1]}s{g[6][0]}p{g[7][0]}x{g[7][1]}-{g[4]}")
def test_conv2d_general_exact(g, log):
    (y, yw), (dx, dxw), (kf, kd) = run(g, log, seed=sum(g[1:5]))
    assert exact(y, yw), f"forward differs at {int((y != yw).sum())} elements; kernel {kf}"
    assert exact(dx, dxw), f"data gradient differs at {int((dx != dxw).sum())} elements; kernel {kd}"
    for k in (kf, kd):
        assert "conv_gather_f32_kernel" in k and "true>" in k.replace(" ", ""), k
    print(f"\n{g}: fwd {kf} | dgrad {kd}")


@pytest.mark.parametrize("case", PROD, ids=lambda c: f"{c[0][1]}to{c[0][4]}-k{c[0][5][0]}x{c[0][5][1]}s{c[0][6][0]}")
def test_conv2d_general_production_epilogues(case, log):
    g, in_c0, in_ctot, out_c0, out_ctot = case
    (y, yw), (dx, dxw), (kf, kd) = run(g, log, bias=True, relu=True, mask=True, acc=True, in_c0=in_c0, in_ctot=in_ctot, out_c0=out_c0,
                                       out_ctot=out_ctot, seed=g[1])
    assert exact(y, yw), f"forward differs at {int((y != yw).sum())} elements; kernel {kf}"
    assert exact(dx, dxw), f"data gradient differs at {int((dx != dxw).sum())} elements; kernel {kd}"
    print(f"\n{g}: fwd {kf} | dgrad {kd}")


def test_conv2d_rejects_what_no_route_takes():
    lib = L.load()
    bad = [
        L.Conv2dDesc(1, 8, 16, 16, 8, 8, 8, 4, 4, 2, 2, 1, 1, 0, 8, 0, 8),      # 4x4 stride 2: forward fine, no data-gradient route
        L.Conv2dDesc(1, 8, 16, 16, 8, 7, 7, 3, 3, 2, 2, 1, 1, 0, 8, 0, 8),      # wrong output size
        L.Conv2dDesc(1, 8, 16, 16, 8, 16, 16, 7, 7, 1, 1, 3, 3, 0, 8, 0, 8),    # 49 taps
        L.Conv2dDesc(1, 8, 16, 16, 8, 16, 16, 3, 3, 1, 1, 1, 1, 4, 8, 0, 8),    # input slice past the tensor
    ]
    assert lib.agan_conv2d_pack_mode(byref(bad[0]), 0) == L.PACK_FWD
    assert lib.agan_conv2d_pack_mode(byref(bad[0]), 1) == -1
    for d in bad[1:]:
        assert lib.agan_conv2d_pack_mode(byref(d), 0) == -1
        assert lib.agan_conv2d_fwd(None, None, None, None, byref(d), None, 0, None, 0, None) == -1
    d = bad[0]
    for prec in range(6):
        assert lib.agan_conv2d_effective_prec(byref(d), prec) == L.PREC_F32
