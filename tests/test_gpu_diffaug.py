"""The augmentation kernels (csrc/diffaug.hip, backend.functional.diffaug) against augment.diffaug_reference.

Shapes: rows shorter than a 16-byte chunk and W % 4 != 0 ([.., 5, 7]: the one-pixel path), C = 1 and C = 4, W % 4 == 0 with the
16-byte path ([2, 4, 24, 40], [5, 3, 64, 64]), and more than one workgroup per sample in both launches ([2, 3, 128, 128]:
49152 elements = 12 chunks of the sum, 16 workgroups of the apply).

Without COLOR the kernels only move bits, so they must EQUAL the reference.  With COLOR the bound is
    |y - ref64|  <= 64 * 2^-24 * (max|x| + 0.5)   per sample,        |dx - ref64| <= 64 * 2^-24 * max|dy|   per sample
(about a dozen roundings, every intermediate below 10 (max|x| + 0.5)).  Measured on MI355X over all shapes and COLOR policies
(test_colour_bound prints every figure): forward at most 0.0582 of the bound, i.e. 3.8 * 2^-24 (max|x| + 0.5); backward at most
0.0613 of it, i.e. 4.0 * 2^-24 max|dy|.
"""
import ctypes
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

A = importlib.import_module("attention-gan_amd.augment")
HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")

DEV = torch.device("cuda", 0)
SHAPES = [(1, 1, 5, 7), (3, 3, 5, 7), (2, 2, 6, 8), (2, 4, 24, 40), (5, 3, 64, 64), (2, 3, 128, 128)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
ALMOST_ONE = 1.0 - 2.0 ** -24
EDGES = (0.0, 0.5, ALMOST_ONE)         # translation: -S, 0, +S; cutout: clipped at the low border, fully inside, clipped at the high border
BOUND = 64 * 2.0 ** -24


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _edge_rounds(N, seed):
    """lists of u [N, 8]: every pair (row edge, column edge) of EDGES for translation and for cutout, then two random draws"""
    g = _gen(seed)
    combos = [(a, b, c, d) for (a, b) in ((p, q) for p in EDGES for q in EDGES) for (c, d) in ((a, b), (b, a))]
    rounds = []
    for i in range(0, len(combos), N):
        u = torch.rand(N, 8, generator=g)
        for n in range(N):
            u[n, 3:7] = torch.tensor(combos[(i + n) % len(combos)])
        rounds.append(u)
    return rounds + [torch.rand(N, 8, generator=g), torch.rand(N, 8, generator=g)]


def _both(x, u, policy, r):
    """(y, dx) of the kernels for upstream gradient r"""
    x = x.clone().requires_grad_(True)
    y = HF.diffaug(x, u, policy)
    y.backward(r)
    return y.detach(), x.grad


def _ref(x, u, policy, r):
    x = x.clone().requires_grad_(True)
    y = A.diffaug_reference(x, u, policy)
    y.backward(r)
    return y.detach(), x.grad


@pytest.mark.parametrize("policy", [A.TRANSLATION, A.CUTOUT, A.TRANSLATION | A.CUTOUT], ids=["translation", "cutout", "both"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_is_exact(shape, policy):
    g = _gen(sum(shape) + policy)
    x = torch.randn(shape, generator=g).to(DEV)
    r = torch.randn(shape, generator=g).to(DEV)
    for u in _edge_rounds(shape[0], 7 * policy + shape[2]):
        u = u.to(DEV)
        y, dx = _both(x, u, policy, r)
        y_ref, dx_ref = _ref(x, u, policy, r)
        assert torch.equal(y, y_ref), f"forward, u = {u.tolist()}"
        assert torch.equal(dx, dx_ref), f"backward, u = {u.tolist()}"
    # the edges really were hit: a shift of +-S and of 0, a cut at each border
    H, W = shape[2:]
    ty = torch.cat([A.translation_offsets(u, H, W)[0] for u in _edge_rounds(shape[0], 0)])
    S = int(0.125 * H + 0.5)
    assert {-S, 0, S} <= set(ty.tolist())


@pytest.mark.parametrize("policy", [1, 3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_integer_operands_pass_through_an_identity_colour_stage(shape, policy):
    """u0 = u1 = u2 = 0.5: b = 0, s = 1, c = 1, and the kernels' fma forms make the colour stage the identity bit for bit"""
    g = _gen(sum(shape) + 100 + policy)
    x = torch.randint(-8, 9, shape, generator=g).float().to(DEV)
    r = torch.randint(-8, 9, shape, generator=g).float().to(DEV)
    for u in _edge_rounds(shape[0], policy)[-4:]:
        u[:, :3] = 0.5
        u = u.to(DEV)
        y, dx = _both(x, u, policy, r)
        y_ref, dx_ref = _ref(x, u, policy & ~A.COLOR, r)                 # x after the gather alone
        assert torch.equal(y, y_ref) and torch.equal(dx, dx_ref)


_WORST = {"fwd": 0.0, "bwd": 0.0}


@pytest.mark.parametrize("policy", [1, 3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_colour_bound(shape, policy):
    g = _gen(sum(shape) + 200 + policy)
    N = shape[0]
    x = torch.randn(shape, generator=g)
    r = torch.randn(shape, generator=g)
    for u in _edge_rounds(N, 50 + policy)[-3:]:
        y, dx = _both(x.to(DEV), u.to(DEV), policy, r.to(DEV))
        y_ref, dx_ref = _ref(x.double(), u.double(), policy, r.double())
        lim_y = BOUND * (x.abs().amax(dim=(1, 2, 3)) + 0.5).double()
        lim_dx = BOUND * r.abs().amax(dim=(1, 2, 3)).double()
        err_y = (y.cpu().double() - y_ref).abs().amax(dim=(1, 2, 3))
        err_dx = (dx.cpu().double() - dx_ref).abs().amax(dim=(1, 2, 3))
        _WORST["fwd"] = max(_WORST["fwd"], float((err_y / lim_y).max()))
        _WORST["bwd"] = max(_WORST["bwd"], float((err_dx / lim_dx).max()))
        print(f"diffaug {shape} policy {policy}: forward error {float((err_y / lim_y).max()):.4f} of the bound, "
              f"backward {float((err_dx / lim_dx).max()):.4f} (worst so far {_WORST['fwd']:.4f} / {_WORST['bwd']:.4f})")
        assert bool((err_y <= lim_y).all()), f"forward: {err_y.tolist()} > {lim_y.tolist()}"
        assert bool((err_dx <= lim_dx).all()), f"backward: {err_dx.tolist()} > {lim_dx.tolist()}"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pair_form(shape):
    g = _gen(sum(shape) + 300)
    N = shape[0]
    a0, b0 = torch.randn(shape, generator=g).to(DEV), torch.randn(shape, generator=g).to(DEV)
    u = torch.rand(2 * N, 8, generator=g).to(DEV)
    r = torch.randn((2 * N,) + shape[1:], generator=g).to(DEV)
    for policy in (7, 6):
        whole = torch.cat([a0, b0]).requires_grad_(True)
        y_cat = HF.diffaug(whole, u, policy)
        y_cat.backward(r)
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = HF.diffaug((a, b), u, policy)
        assert torch.equal(y, y_cat)
        y.backward(r)
        assert torch.equal(a.grad, whole.grad[:N]) and torch.equal(b.grad, whole.grad[N:])
        # a source that does not ask gets no gradient; the other one gets the same bits
        for first in (True, False):
            a, b = a0.clone().requires_grad_(first), b0.clone().requires_grad_(not first)
            HF.diffaug((a, b), u, policy).backward(r)
            want, idle = (a, b) if first else (b, a)
            assert idle.grad is None
            assert torch.equal(want.grad, whole.grad[:N] if first else whole.grad[N:])
        assert not HF.diffaug((a0, b0), u, policy).requires_grad


def _raw(name, *args):
    return getattr(L.load(), name)(*args)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_calls_give_the_same_bytes_with_a_poisoned_workspace(shape):
    N, C, H, W = shape
    g = _gen(sum(shape) + 400)
    x, r = torch.randn(shape, generator=g).to(DEV), torch.randn(shape, generator=g).to(DEV)
    u = torch.rand(N, 8, generator=g).to(DEV)
    nbytes = L.load().agan_diffaug_ws_bytes(N, C, H, W)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    st = HF._stream()
    outs = []
    for fill in (float("nan"), 1e30):
        y, dx = torch.empty_like(x), torch.empty_like(x)
        ws.fill_(fill)
        assert _raw("agan_diffaug_fwd", _ptr(x), None, N, 0, _ptr(u), 7, _ptr(y), C, H, W, _ptr(ws), nbytes, st) == 0
        ws.fill_(fill)
        assert _raw("agan_diffaug_bwd", _ptr(r), _ptr(u), 7, _ptr(dx), N, C, H, W, _ptr(ws), nbytes, st) == 0
        outs.append((y, dx))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())
    y_f, dx_f = _both(x, u, 7, r)                                        # and they are what the autograd bridge returns
    assert torch.equal(outs[0][0], y_f) and torch.equal(outs[0][1], dx_f)


def test_argument_checks():
    N, C, H, W = 2, 3, 8, 8
    x, y = torch.zeros(N, C, H, W, device=DEV), torch.zeros(N, C, H, W, device=DEV)
    u = torch.rand(N, 8, device=DEV)
    nbytes = L.load().agan_diffaug_ws_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    st = HF._stream()
    ok = dict(x=_ptr(x), u=_ptr(u), y=_ptr(y), N=N, C=C, H=H, W=W, policy=7, ws=_ptr(ws), nbytes=nbytes)

    def fwd(**kw):
        a = dict(ok, **kw)
        return _raw("agan_diffaug_fwd", a["x"], None, a["N"], 0, a["u"], a["policy"], a["y"], a["C"], a["H"], a["W"], a["ws"], a["nbytes"], st)

    def bwd(**kw):
        a = dict(ok, **kw)
        return _raw("agan_diffaug_bwd", a["x"], a["u"], a["policy"], a["y"], a["N"], a["C"], a["H"], a["W"], a["ws"], a["nbytes"], st)

    for call in (fwd, bwd):
        assert call() == 0
        for kw in (dict(C=0), dict(C=5), dict(H=0), dict(W=0), dict(N=0), dict(N=-1), dict(policy=8), dict(policy=-1), dict(x=None),
                   dict(u=None), dict(y=None), dict(ws=None), dict(N=1 << 22, C=4, H=16, W=8)):
            assert call(**kw) == L.EINVAL, kw
        assert call(nbytes=nbytes - 1) == L.EWORKSPACE
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        HF.diffaug(torch.zeros(1, 5, 8, 8, device=DEV), torch.rand(1, 8, device=DEV), 7)
    with pytest.raises(ValueError):
        HF.diffaug(x, torch.rand(N + 1, 8, device=DEV), 7)
    with pytest.raises(ValueError):
        HF.diffaug((x, x[:1]), torch.rand(N + 1, 8, device=DEV), 7)
    with pytest.raises(L.AganError):
        HF.diffaug(x.cpu(), u.cpu(), 7)
