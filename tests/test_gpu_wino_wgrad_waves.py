"""The fp32 Winograd weight gradient (csrc/conv_wino.hip, conv_wino_wgrad_f32_kernel) as a workgroup of 8 waves, two per SIMD.

Waves 0-3 accumulate Winograd positions 0-7 of their 32 x 32 (cout, cin) fragment pair, waves 4-7 positions 8-15; every thread stages one
(tile, channel) pair per operand; after the octet loop the two groups swap halves of their accumulators through LDS and each finishes
half of the fragment's registers.  What can go wrong is an assignment: a position, fragment, tile, channel or register that lands in the
wrong place -- so every case has

(a) an exact part: operands on a dyadic grid (as tests/test_gpu_conv_exact.py builds them), every product and every partial sum exact in
    fp32 INCLUDING Winograd's 1/2 factors, in any summation order and under any pixel split, and the result must EQUAL torch's CPU fp64
    `conv2d_weight`.  Budget (asserted below): with |x| <= rx grid units of 2^EX and |dy| <= rdy units of 2^EDY, a transformed x value
    (B^T d B: 4 terms) is at most 4 rx units, a transformed dy value (G e G^T) a multiple of 2^(EDY - 2) of at most 4 rdy such units; an
    accumulator sums at most T = B (OH/2) (OW/2) tile products and an output of A^T M A at most 9 accumulators: 9 T (4 rx) (4 rdy) units
    of 2^(EX + EDY - 2) must stay below 2^24;
(b) a bounded part: random normal operands under the bound and rule tests/test_gpu_wino.py applies to this kernel's weight gradient
    (max |error| / max |reference| per tensor <= its TOL, against the fp64 reference).

Shapes are the smallest the plan takes (B (OH/2) (OW/16) >= 1024 tile octets, OW % 16 == 0, channels >= 32, Cin % 4 == 0, Cout % 8 == 0).
Every call asserts through agan_timer_last_kernel that the Winograd weight-gradient kernel ran: a re-route cannot pass on another kernel.
"""
import ctypes
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-5          # max |error| / max |reference| per tensor: tests/test_gpu_wino.py's TOL, restated

HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")

KERNEL = "conv_wino_wgrad_f32_kernel"
EX, EDY = -2, -1            # grid steps of x and dy (tests/test_gpu_conv_exact.py)
RX, RDY = 3, 4              # integer ranges of the grid operands

CASES = {
    # B, Cin, H, W, Cout
    "handover": (8, 32, 64, 64, 32),         # one partial 64 x 64 channel tile (fragments fi = fj = 0 only), 1024 octets
    "partial-tiles": (9, 96, 64, 64, 40),    # cin tiles 64 + 32, cout 40 of 64 (8 of the second fragment), 1152 octets (72 splits of 16)
    "non-square": (8, 64, 32, 128, 64),      # 8 octets per tile row, 16 tile rows; a full channel tile: all four fragment pairs
    "ragged-split": (10, 32, 206, 16, 32),   # 1030 octets in 61 splits of 17: the last one has 10; one octet per tile row (both edge columns in it)
}


def _ref_dw(x, dy, cout):
    """fp64 conv2d_weight on the CPU"""
    B, cin = x.shape[:2]
    return torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), stride=1, padding=1)


def _grid(shape, gen, lim, exp):
    return (torch.randint(-lim, lim + 1, shape, generator=gen, dtype=torch.int64).double() * 2.0 ** exp).float()


_OPERANDS = {}


def operands(name):
    """-> dict of CPU tensors for a case, built once: grid operands with their exact gradient, normal operands with their fp64 gradient"""
    hit = _OPERANDS.get(name)
    if hit is not None:
        return hit
    B, Cin, H, W, Cout = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    tiles = B * (H // 2) * (W // 2)
    assert 9 * tiles * (4 * RX) * (4 * RDY) < 2 ** 24, f"{name}: the grid operands are not exact in fp32 through the Winograd transforms"
    xg, dyg = _grid((B, Cin, H, W), gen, RX, EX), _grid((B, Cout, H, W), gen, RDY, EDY)
    dwg = _ref_dw(xg, dyg, Cout)
    assert torch.equal(dwg.float().double(), dwg)
    xn, dyn = torch.randn(B, Cin, H, W, generator=gen), torch.randn(B, Cout, H, W, generator=gen)
    dwn = _ref_dw(xn, dyn, Cout)
    # a dw to accumulate into: on the grid of dw (exact part), of the gradient's own scale (bounded part)
    pre_g = _grid((Cout, Cin, 3, 3), gen, 1000, EX + EDY)
    pre_n = torch.randn(Cout, Cin, 3, 3, generator=gen) * float(dwn.std())
    out = dict(xg=xg, dyg=dyg, dwg=dwg.float(), xn=xn, dyn=dyn, dwn=dwn, pre_g=pre_g, pre_n=pre_n)
    _OPERANDS[name] = out
    return out


class Wgrad:
    """agan_conv_wgrad of one geometry in the fp32 mode, timed so that the library names the main kernel of every call"""

    def __init__(self, name):
        B, Cin, H, W, Cout = CASES[name]
        HF.set_precision(L.PREC_F32)
        self.lib = L.load()
        self.shape = (Cout, Cin, 3, 3)
        self.gf, self.pf = HF.conv_geoms("same", B, Cin, H, W, Cout, 3)[:2]
        self.nbytes = int(self.lib.agan_conv_wgrad_ws_bytes(ctypes.byref(self.gf)))
        self.ws = torch.empty(max(self.nbytes, 16), dtype=torch.uint8, device=DEV)
        self.kt = HF.ktable(self.gf, torch.device(DEV))
        self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
        L.call("agan_timer_create", ctypes.byref(self.e0))
        L.call("agan_timer_create", ctypes.byref(self.e1))
        self.name = ctypes.create_string_buffer(1024)

    def __call__(self, x, dy, dw=None):
        """-> dw on the CPU; dw given: accumulate into (a copy of) it"""
        xd, dyd = x.to(DEV), dy.to(DEV)
        out = torch.full(self.shape, 7.0, device=DEV) if dw is None else dw.to(DEV).clone()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.call("agan_timer_arm", self.e0, self.e1)
        L.call("agan_conv_wgrad", ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(dyd.data_ptr()), ctypes.c_void_p(out.data_ptr()),
               ctypes.byref(self.gf), ctypes.c_void_p(self.kt.data_ptr()), self.pf, 3, 3, L.PREC_F32, 0 if dw is None else 1,
               ctypes.c_void_p(self.ws.data_ptr()), self.nbytes, stream, None, None)
        torch.cuda.synchronize()
        L.call("agan_timer_last_kernel", self.name, 1024)
        ran = self.name.value.decode()
        assert KERNEL in ran, f"the call ran {ran or 'no timed kernel'!r}, not {KERNEL}"
        return out.cpu()

    def close(self):
        L.call("agan_timer_destroy", self.e0)
        L.call("agan_timer_destroy", self.e1)


@pytest.fixture
def wgrad(request):
    w = Wgrad(request.param)
    yield w
    w.close()


def _first_difference(got, want):
    ne = got != want
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return f"{int(ne.sum())} of {got.numel()} elements differ; first at (cout, cin, r, s) = {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}"


@pytest.mark.parametrize("name,wgrad", [(n, n) for n in CASES], indirect=["wgrad"])
def test_weight_gradient_is_exact_on_grid_operands(name, wgrad):
    op = operands(name)
    got = wgrad(op["xg"], op["dyg"])
    assert torch.equal(got, op["dwg"]), f"{name}: " + _first_difference(got, op["dwg"])


@pytest.mark.parametrize("name,wgrad", [(n, n) for n in CASES], indirect=["wgrad"])
def test_weight_gradient_is_within_the_winograd_bound_on_normal_operands(name, wgrad):
    op = operands(name)
    got = wgrad(op["xn"], op["dyn"])
    err = float((got.double() - op["dwn"]).abs().max() / op["dwn"].abs().max())
    print(f"{name}: max |error| / max |reference| = {err:.3e} (bound {TOL:.0e})")
    assert err <= TOL, f"{name}: weight gradient max error / max |ref| = {err:.3e} > {TOL:.0e}"


@pytest.mark.parametrize("wgrad", ["handover"], indirect=True)
def test_accumulate_into_a_prefilled_gradient(wgrad):
    """accumulate = 1: the slab sum adds the gradient to what dw holds -- exactly on grid operands, within the bound on normal ones"""
    op = operands("handover")
    got = wgrad(op["xg"], op["dyg"], dw=op["pre_g"])
    want = op["pre_g"] + op["dwg"]
    assert torch.equal(want.double(), op["pre_g"].double() + op["dwg"].double())
    assert torch.equal(got, want), "grid operands: " + _first_difference(got, want)
    got = wgrad(op["xn"], op["dyn"], dw=op["pre_n"])
    want = op["pre_n"].double() + op["dwn"]
    err = float((got.double() - want).abs().max() / want.abs().max())
    print(f"accumulate: max |error| / max |reference| = {err:.3e} (bound {TOL:.0e})")
    assert err <= TOL, f"accumulated weight gradient max error / max |ref| = {err:.3e} > {TOL:.0e}"
