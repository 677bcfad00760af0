"""Pools and bilinear resize of the Inception-v3 trunk (csrc/pool_resize.hip) against torch's CPU float64 ops.

* max pool 3x3 stride 2: forward and backward bit-exact, on inputs full of exact ties (all-zero windows as after a ReLU, repeated
  values) where torch's tie-break (first maximum in row-major window order) decides where the gradient goes, plus a NaN case;
* avg pool 3x3 s1 p1 (/9), global 8x8 mean and the bilinear resize to 299 (align_corners=False) from 64 / 128 / 256: forward and
  backward within 1e-6 relative of float64;
* every backward is a fixed-order gather: two runs are identical bit for bit.
"""
import importlib

import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")
_p, _s = HF._p, HF._stream


def _maxpool(x, dy, c0=0, ctot=None, mask=None, acc_into=None):
    B, C, H, W = x.shape
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    ctot = ctot or C
    y = torch.full((B, ctot, OH, OW), 7.0, device=DEV)
    am = torch.empty(B * C * OH * OW, dtype=torch.uint8, device=DEV)
    L.call("agan_maxpool3s2_fwd", _p(x), _p(y), _p(am), B, C, H, W, c0, ctot, _s())
    dx = acc_into.clone() if acc_into is not None else torch.empty_like(x)
    L.call("agan_maxpool3s2_bwd", _p(dy), _p(am), _p(mask), _p(dx), B, C, H, W, c0, ctot, int(acc_into is not None), _s())
    torch.cuda.synchronize()
    return y, am, dx


def _ref_maxpool(x, dy):
    xd = x.double().cpu().requires_grad_(True)
    y = F.max_pool2d(xd, 3, 2)
    y.backward(dy.double().cpu())
    return y.detach(), xd.grad


@pytest.mark.parametrize("H", [147, 71, 35, 17])
def test_maxpool_ties_bit_exact(H):
    g = torch.Generator().manual_seed(H)
    B, C = 2, 5
    # post-ReLU-like values: mostly zeros, few distinct positives -> exact ties in most windows
    x = torch.randint(-3, 3, (B, C, H, H), generator=g).clamp_min(0).float()
    x[:, 0] = 0.0                                        # whole channel of all-zero windows
    OH = (H - 3) // 2 + 1
    dy = (torch.randint(-8, 9, (B, C, OH, OH), generator=g).float() * 0.25)
    yw, dxw = _ref_maxpool(x, dy)
    y, _, dx = _maxpool(x.to(DEV), dy.to(DEV))
    assert torch.equal(y.cpu().double(), yw)
    assert torch.equal(dx.cpu().double(), dxw)
    _, _, dx2 = _maxpool(x.to(DEV), dy.to(DEV))
    assert torch.equal(dx, dx2)


def test_maxpool_nan_slice_mask_accumulate():
    g = torch.Generator().manual_seed(1)
    B, C, H = 2, 4, 17
    x = torch.randint(-2, 3, (B, C, H, H), generator=g).float()
    x[0, 1, 4, 4] = float("nan")
    x[1, 2, 0, 0] = float("nan")
    x[1, 2, 1, 2] = float("nan")
    OH = (H - 3) // 2 + 1
    dy = torch.randint(-8, 9, (B, C + 3, OH, OH), generator=g).float() * 0.5
    c0, ctot = 2, C + 3
    base = torch.randint(-4, 5, (B, C, H, H), generator=g).float() * 0.125
    mask = torch.randint(-1, 2, (B, C, H, H), generator=g).float()
    yw, dxw = _ref_maxpool(x, dy[:, c0:c0 + C])
    dxw = base.double() + dxw * (mask.double() > 0)
    y, _, dx = _maxpool(x.to(DEV), dy.to(DEV), c0, ctot, mask.to(DEV), base.to(DEV))
    y = y.cpu().double()
    assert torch.equal(torch.nan_to_num(y[:, c0:c0 + C], nan=99.0), torch.nan_to_num(yw, nan=99.0))
    assert (y[:, :c0] == 7.0).all() and (y[:, c0 + C:] == 7.0).all(), "the pool wrote outside its channel slice"
    assert torch.equal(dx.cpu().double(), dxw)


def test_avgpool_and_global_mean():
    g = torch.Generator().manual_seed(2)
    B, C, H = 2, 6, 35
    x = torch.randn(B, C, H, H, generator=g)
    dy = torch.randn(B, C, H, H, generator=g)
    xd = x.double().requires_grad_(True)
    yw = F.avg_pool2d(xd, 3, 1, 1, count_include_pad=True)
    yw.backward(dy.double())
    xg, dyg = x.to(DEV), dy.to(DEV)
    y = torch.empty(B, C, H, H, device=DEV)
    L.call("agan_avgpool3s1_fwd", _p(xg), _p(y), B, C, H, H, _s())
    dx = torch.empty(B, C, H, H, device=DEV)
    L.call("agan_avgpool3s1_bwd", _p(dyg), None, _p(dx), B, C, H, H, 0, _s())
    dx2 = torch.empty_like(dx)
    L.call("agan_avgpool3s1_bwd", _p(dyg), None, _p(dx2), B, C, H, H, 0, _s())
    assert rel_err(y, yw.detach()) < 1e-6
    assert rel_err(dx, xd.grad) < 1e-6
    assert torch.equal(dx, dx2)
    # global 8x8 mean
    x8 = torch.randn(B, 64, 8, 8, generator=g)
    d8 = torch.randn(B, 64, generator=g)
    xd = x8.double().requires_grad_(True)
    m = F.avg_pool2d(xd, 8).flatten(1)
    m.backward(d8.double())
    x8g, d8g = x8.to(DEV), d8.to(DEV)
    y8 = torch.empty(B, 64, device=DEV)
    L.call("agan_global_avgpool_fwd", _p(x8g), _p(y8), B, 64, 64, _s())
    g8 = torch.empty(B, 64, 8, 8, device=DEV)
    L.call("agan_global_avgpool_bwd", _p(d8g), None, _p(g8), B, 64, 64, 0, _s())
    assert rel_err(y8, m.detach()) < 1e-6
    assert rel_err(g8, xd.grad) < 1e-6


@pytest.mark.parametrize("H", [64, 128, 256, 300])
def test_resize_bilinear(H):
    g = torch.Generator().manual_seed(H)
    B, C, O = 2, 3, 299
    x = torch.randn(B, C, H, H, generator=g)
    dy = torch.randn(B, C, O, O, generator=g)
    xd = x.double().requires_grad_(True)
    yw = F.interpolate(xd, size=(O, O), mode="bilinear", align_corners=False)
    yw.backward(dy.double())
    xg, dyg = x.to(DEV), dy.to(DEV)
    y = torch.empty(B, C, O, O, device=DEV)
    L.call("agan_resize_bilinear_fwd", _p(xg), _p(y), B, C, H, H, O, O, _s())
    dx = torch.empty(B, C, H, H, device=DEV)
    L.call("agan_resize_bilinear_bwd", _p(dyg), _p(dx), B, C, H, H, O, O, _s())
    dx2 = torch.empty_like(dx)
    L.call("agan_resize_bilinear_bwd", _p(dyg), _p(dx2), B, C, H, H, O, O, _s())
    assert rel_err(y, yw.detach()) < 1e-6
    assert rel_err(dx, xd.grad) < 1e-6
    assert torch.equal(dx, dx2)
