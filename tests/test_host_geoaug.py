"""CPU-side tests of the geometric augmentation's statement in torch ops (augment.py: parse_geometry, geometry_matrices_reference,
affine_warp_reference -- the oracle of tests/test_gpu_geoaug.py): the stage names, the matrices' exact cases, determinant range and
gates, the warp against torch.flip / torch.rot90 and a zero-filled shift, the adjoint identity the backward kernel implements, and the
C ABI's argument checks (which return before any device work)."""
import importlib

import pytest
import torch

A = importlib.import_module("attention-gan_amd.augment")
L = importlib.import_module("attention-gan_amd.backend.lib")

ALL = "xflip,rot90,scale,rotate,aniso"
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def _g(n, seed=0, dtype=torch.float64):
    return torch.rand(n, 16, generator=torch.Generator().manual_seed(seed), dtype=torch.float32).to(dtype)


def test_parse_geometry():
    assert A.parse_geometry(ALL) == 31 and A.parse_geometry("aniso, xflip") == 17
    assert A.parse_geometry("") == 0 and A.parse_geometry(None) == 0 and A.parse_geometry(21) == 21
    for mask in range(32):
        assert A.parse_geometry(A.geometry_names(mask)) == mask
    assert A.geometry_names(31) == ALL
    assert (A.XFLIP, A.ROT90, A.SCALE, A.ROTATE, A.ANISO) == (1, 2, 4, 8, 16)
    assert (L.GEOAUG_XFLIP, L.GEOAUG_ROT90, L.GEOAUG_SCALE, L.GEOAUG_ROTATE, L.GEOAUG_ANISO) == (1, 2, 4, 8, 16)
    assert L.GEOAUG_ALL == 31 and L.GEOAUG_UNIFORMS == A.GEO_UNIFORMS == 16
    for bad in ("flip", "xflip;rot90", "color", "rot"):
        with pytest.raises(ValueError):
            A.parse_geometry(bad)
    for bad in (32, -1, 1.5, True):
        with pytest.raises(ValueError):
            A.parse_geometry(bad)
    # the two parsers stay apart: DiffAugment's refuses the geometric names and the other way round
    with pytest.raises(ValueError):
        A.parse_policy("xflip")
    with pytest.raises(ValueError):
        A.parse_geometry("cutout")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_matrices_identity_bits_when_nothing_applies(dtype):
    g = _g(64, 1, dtype)
    for M in (A.geometry_matrices_reference(g, 0), A.geometry_matrices_reference(g, None), A.geometry_matrices_reference(g, ALL, 0.0),
              A.geometry_matrices_reference(g, ALL, float("nan"))):
        assert M.dtype == dtype and M.tolist() == [IDENTITY] * 64
    g[:, 0] = 0.25                                                        # xflip enabled, not drawn: skipped
    assert A.geometry_matrices_reference(g, "xflip").tolist() == [IDENTITY] * 64
    g[:, 3] = 0.5                                                         # theta = 0: cos = 1 and sin = 0 exactly
    assert A.geometry_matrices_reference(g, "rotate").tolist() == [IDENTITY] * 64


def test_matrices_of_flip_and_quarter_turns_are_exact():
    g = _g(256, 2, torch.float32)
    M = A.geometry_matrices_reference(g, "xflip,rot90")
    assert bool(((M == 0) | (M == 1) | (M == -1)).all())
    assert bool((M[:, 2] == 0).all()) and bool((M[:, 5] == 0).all())
    det = M[:, 0] * M[:, 4] - M[:, 1] * M[:, 3]
    flipped = g[:, 0] >= 0.5
    assert torch.equal(det, torch.where(flipped, -1.0, 1.0))
    assert bool(flipped.any()) and not bool(flipped.all())
    # the table: k = min(int(4 g1), 3), also at the ends of the range
    g = torch.zeros(5, 16)
    g[:, 1] = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24])
    M = A.geometry_matrices_reference(g, "rot90")
    assert M[:, [0, 1, 3, 4]].tolist() == [[1, 0, 0, 1], [0, -1, 1, 0], [-1, 0, 0, -1], [0, 1, -1, 0], [0, 1, -1, 0]]


def test_determinant_range_over_many_draws():
    g = _g(10000, 3)
    M = A.geometry_matrices_reference(g, ALL)
    det = (M[:, 0] * M[:, 4] - M[:, 1] * M[:, 3]).abs()
    lo, hi = 2.0 ** -0.7, 2.0 ** 0.7
    print("|det| range:", float(det.min()), float(det.max()), "allowed", lo, hi)
    assert float(det.min()) >= lo * (1 - 1e-12) and float(det.max()) <= hi * (1 + 1e-12)
    # aniso and rotate keep areas: alone their determinant is 1; scale alone is s^2
    M = A.geometry_matrices_reference(g, "rotate,aniso")
    assert float(((M[:, 0] * M[:, 4] - M[:, 1] * M[:, 3]) - 1).abs().max()) <= 1e-12
    M = A.geometry_matrices_reference(g, "scale")
    s = torch.exp2(0.7 * g[:, 2] - 0.35)
    assert torch.equal(M[:, 0], s) and torch.equal(M[:, 4], s) and bool((M[:, 1] == 0).all())


def test_gate_semantics():
    g = _g(512, 4)
    p = 0.4
    gates = A.geometry_gates(g, p)
    assert gates.shape == (512, 5) and torch.equal(gates, g[:, 8:13].float() < torch.tensor(p, dtype=torch.float32))
    for k, name in enumerate(ALL.split(",")):
        gated = A.geometry_matrices_reference(g, name, p)
        plain = A.geometry_matrices_reference(g, name)
        ident = torch.tensor(IDENTITY, dtype=torch.float64).expand(512, 6)
        assert torch.equal(gated, torch.where(gates[:, k:k + 1], plain, ident)), name
    # all stages: a sample equals the ungated matrix of exactly the stages that passed
    gated = A.geometry_matrices_reference(g, ALL, p)
    for n in range(32):
        mask = sum(1 << k for k in range(5) if bool(gates[n, k]))
        assert torch.equal(gated[n], A.geometry_matrices_reference(g[n:n + 1], mask)[0])
    # q == p is off (strict compare), p >= 1 passes everything, a tensor p is read as fp32
    g[:, 8:13] = 0.4
    assert A.geometry_matrices_reference(g.float(), ALL, torch.tensor([0.4])).tolist() == [IDENTITY] * 512
    assert torch.equal(A.geometry_matrices_reference(g, ALL, 1.0), A.geometry_matrices_reference(g, ALL))


@pytest.mark.parametrize("H", [5, 6])
def test_warp_equals_flip_and_quarter_turns(H):
    x = torch.randn(8, 3, H, H, generator=torch.Generator().manual_seed(H))
    g = torch.zeros(8, 16)
    g[:, 0] = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.9, 0.9, 0.9, 0.9])
    g[:, 1] = torch.tensor([0.1, 0.3, 0.6, 0.99] * 2)
    y = A.geoaug_reference(x, g, "xflip,rot90")
    for n in range(8):
        t = x[n].flip(-1) if n >= 4 else x[n]
        assert torch.equal(y[n], torch.rot90(t, n % 4, (-2, -1))), n
    assert torch.equal(A.geoaug_reference(x, g, "xflip")[4:], x[4:].flip(-1))
    assert torch.equal(A.geoaug_reference(x, g, 0), x)
    # flip alone needs no square image
    xr = torch.randn(2, 2, H, H + 3, generator=torch.Generator().manual_seed(9))
    M = torch.tensor([[-1.0, 0, 0, 0, 1, 0], [1.0, 0, 0, 0, -1, 0]])
    y = A.affine_warp_reference(xr, M)
    assert torch.equal(y[0], xr[0].flip(-1)) and torch.equal(y[1], xr[1].flip(-2))


def test_warp_whole_pixel_shift_is_zero_filled():
    H, W = 5, 8
    x = torch.randn(3, 2, H, W, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    M = torch.tensor([IDENTITY] * 3, dtype=torch.float64)
    M[0, 2] = 1.0 / W                                                     # source = output + 1 in x
    M[1, 5] = -2.0 / H                                                    # source = output - 2 in y
    M[2, 2] = 1.0                                                         # a whole image away: nothing left
    y = A.affine_warp_reference(x, M)
    assert torch.equal(y[0, :, :, :W - 1], x[0, :, :, 1:]) and bool((y[0, :, :, W - 1] == 0).all())
    assert torch.equal(y[1, :, 2:], x[1, :, :H - 2]) and bool((y[1, :, :2] == 0).all())
    assert bool((y[2] == 0).all())


@pytest.mark.parametrize("geometry", [0, 3, 4, 8, 16, 31])
def test_adjoint(geometry):
    gen = torch.Generator().manual_seed(20 + geometry)
    x = torch.randn(4, 3, 9, 12, generator=gen, dtype=torch.float64, requires_grad=True)
    r = torch.randn(4, 3, 9, 12, generator=gen, dtype=torch.float64)
    M = A.geometry_matrices_reference(_g(4, 30 + geometry), geometry)
    M[:, 2], M[:, 5] = 0.11, -0.07                                        # with a translation too
    y = A.affine_warp_reference(x, M)
    grad, = torch.autograd.grad((y * r).sum(), x)
    lhs, rhs = float((y.detach() * r).sum()), float((x.detach() * grad).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    # the map is linear, not affine: zero goes to zero
    assert float(A.affine_warp_reference(torch.zeros_like(x.detach()), M).abs().max()) == 0.0


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every refusal comes before device work, so it can be checked without a GPU (pointers are never followed)."""
    import ctypes
    lib = L.load()
    p = ctypes.c_void_p(4096)                                           # a non-null token
    ok = dict(x0=p, x1=None, n0=2, n1=0, M=p, y=p, C=3, H=8, W=8)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.agan_affine_warp_fwd(a["x0"], a["x1"], a["n0"], a["n1"], a["M"], a["y"], a["C"], a["H"], a["W"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.agan_affine_warp_bwd(a["x0"], a["M"], a["y"], a["n0"], a["C"], a["H"], a["W"], None)

    for call in (fwd, bwd):
        for kw in (dict(C=0), dict(C=5), dict(C=-1), dict(H=0), dict(W=-1), dict(H=-8), dict(n0=0), dict(n0=-2), dict(x0=None), dict(M=None),
                   dict(y=None), dict(n0=1 << 20, C=4, H=32, W=16), dict(H=(1 << 24) + 1, W=1, n0=1, C=1)):
            assert call(**kw) == L.EINVAL, kw
            assert lib.agan_last_error()
    assert fwd(n1=-1, x1=p) == L.EINVAL

    def matrix(g=p, pp=None, geometry=31, M=p, n=4):
        return lib.agan_geoaug_matrix(g, pp, geometry, M, n, None)

    for kw in (dict(g=None), dict(M=None), dict(n=0), dict(n=-3), dict(geometry=32), dict(geometry=-1)):
        assert matrix(**kw) == L.EINVAL, kw
        assert lib.agan_last_error()
