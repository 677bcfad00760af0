"""The fp32 Winograd gathers of the conv4x4 stride-2 layers (csrc/conv_wino.hip: conv_wino_s2_f32_kernel<4>, the polyphase forward, and
conv_wino_cls_f32_kernel<4>, the class-wise data gradient) as workgroups of 8 waves, two per SIMD.

Waves w and w + 4 share a cout fragment: waves 0-3 accumulate Winograd positions 0-4 (of every phase / both channel octets of a 16-channel
chunk), waves 4-7 positions 5-8; every thread stages half the raw patch and transforms half the pieces, and after the chunk loop the two
waves swap halves of their accumulators through LDS and each finishes eight of the fragment's sixteen registers.
What can go wrong is an assignment: a phase, octet, position, tile, channel or register half that lands in the wrong place -- so every
case has

(a) an exact part: operands on the dyadic grid of tests/test_gpu_conv_exact.py (integers times 2^EX / 2^EW / 2^EDY).  The transforms of
    F(2x2, 2x2) are all +-1, so every product and partial sum is exact in fp32 in any order and under any split, and the result must EQUAL
    torch's CPU fp64 convolution (conv2d / conv2d_input).  Budget (asserted below): a transformed input value has 4 terms (<= 4 r_in
    units), a transformed weight 4 terms (<= 4 r_w units); an output sums four accumulators, each over C gathered channels x 16 taps'
    worth of such products at most: 4 C 16 (4 r_in) (4 r_w) grid units must stay below 2^24;
(b) a bounded part: random normal operands, max |error| / max |reference| per tensor <= the TOL tests/test_gpu_wino.py applies to these
    paths, against the fp64 reference; the measured value is printed.

Every call asserts through agan_timer_last_kernel (the launch observer) that the intended kernel ran: a re-route cannot pass on the
direct kernel.
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

FWD_KERNEL, DGRAD_KERNEL = "conv_wino_s2_f32_kernel<4>", "conv_wino_cls_f32_kernel<4>"
EX, EW, EDY = -2, -3, -1    # grid steps of x, w and dy (tests/test_gpu_conv_exact.py)
RIN, RW = 3, 4              # integer ranges of the gathered operand (x forward, dy backward) and of the weights

# forward geometry B, Cin, H, W, Cout
FWD_CASES = {
    "one-chunk": (16, 8, 128, 128, 96),          # ONE input-channel chunk (prologue only); three of four cout fragments; 512 workgroups, unsplit
    "split": (8, 128, 128, 128, 128),            # 256 blocks: the input-channel split, 2 x 8 chunks, slabs and the slab sum
    "ragged": (8, 24, 96, 176, 160),             # three chunks (both LDS buffers in both roles); 44 tile columns = 5 x 8 + 4; cout tail 32 of the second 128
    "small-maps": (127, 128, 16, 16, 512),       # 4 x 4 tiles per image: two images per block, odd batch (last block half empty); split launch
}
# the data gradient gathers Cout channels of dy into Cin channels of dx
DGRAD_CASES = {
    "one-chunk": (16, 128, 64, 64, 16),          # ONE 16-channel chunk; 512 workgroups over the four classes
    "two-chunks": (16, 128, 64, 64, 32),         # one chunk per LDS buffer
    "ragged": (11, 104, 48, 112, 48),            # three chunks; 28 tile columns = 3 x 8 + 4; output-channel tail (8 of the fourth fragment)
}


def _grid(shape, gen, lim, exp):
    return (torch.randint(-lim, lim + 1, shape, generator=gen, dtype=torch.int64).double() * 2.0 ** exp).float()


def _ref(direction, a, w, shape):
    """fp64 on the CPU: the forward of x = a, or the data gradient of dy = a for an input of `shape`"""
    if direction == "fwd":
        return torch.nn.functional.conv2d(a.double(), w.double(), None, 2, 1)
    return torch.nn.grad.conv2d_input(shape, w.double(), a.double(), stride=2, padding=1)


_OPERANDS = {}


def operands(direction, name):
    """-> dict of CPU tensors for a case, built once: grid operands with their exact result, normal operands with their fp64 result"""
    hit = _OPERANDS.get((direction, name))
    if hit is not None:
        return hit
    B, Cin, H, W, Cout = (FWD_CASES if direction == "fwd" else DGRAD_CASES)[name]
    gen = torch.Generator().manual_seed(sum(map(ord, direction + name)))
    xshape, wshape, yshape = (B, Cin, H, W), (Cout, Cin, 4, 4), (B, Cout, H // 2, W // 2)
    ashape, chans, ea = (xshape, Cin, EX) if direction == "fwd" else (yshape, Cout, EDY)
    assert 4 * chans * 16 * (4 * RIN) * (4 * RW) < 2 ** 24, f"{direction} {name}: the grid operands are not exact in fp32 through the Winograd transforms"
    ag, wg = _grid(ashape, gen, RIN, ea), _grid(wshape, gen, RW, EW)
    rg = _ref(direction, ag, wg, xshape)
    assert torch.equal(rg.float().double(), rg)
    an, wn = torch.randn(ashape, generator=gen), torch.randn(wshape, generator=gen) / (chans * 16) ** 0.5
    rn = _ref(direction, an, wn, xshape)
    out = dict(ag=ag, wg=wg, rg=rg.float(), an=an, wn=wn, rn=rn)
    _OPERANDS[(direction, name)] = out
    return out


class KernelLog:
    """launch observer: arms the library's timer hook before every conv-engine call and asks it afterwards which main kernel ran"""

    def __init__(self):
        self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
        L.call("agan_timer_create", ctypes.byref(self.e0))
        L.call("agan_timer_create", ctypes.byref(self.e1))
        self.name = ctypes.create_string_buffer(1024)
        self.phase, self.seen = None, {}

    def begin(self, kind, phase, g, in_esz=4, out_esz=4):
        L.call("agan_timer_arm", self.e0, self.e1)
        self.phase = phase

    def end(self):
        torch.cuda.synchronize()
        L.call("agan_timer_last_kernel", self.name, 1024)
        self.seen[self.phase] = self.name.value.decode()

    def close(self):
        L.call("agan_timer_destroy", self.e0)
        L.call("agan_timer_destroy", self.e1)


@pytest.fixture
def log():
    HF.set_precision(L.PREC_F32)
    lg = KernelLog()
    HF.set_launch_observer(lg)
    yield lg
    HF.set_launch_observer(None)
    lg.close()


def run(direction, log, a, w, xshape):
    """the layer's forward (a = x) or data gradient (a = dy) on the library -> CPU tensor; asserts which kernel ran"""
    log.seen = {}
    wd = w.to(DEV)
    if direction == "fwd":
        out = HF.conv2d(a.to(DEV), wd, None, "down")
        phase, kernel = "fwd", FWD_KERNEL
    else:
        xd = torch.zeros(xshape, device=DEV).requires_grad_(True)
        HF.conv2d(xd, wd, None, "down").backward(a.to(DEV))
        out, phase, kernel = xd.grad, "dgrad", DGRAD_KERNEL
    torch.cuda.synchronize()
    ran = log.seen.get(phase, "")
    assert kernel in ran, f"the {phase} call ran {ran or 'no timed kernel'!r}, not {kernel}"
    return out.detach().cpu()


def _first_difference(got, want):
    ne = got != want
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return f"{int(ne.sum())} of {got.numel()} elements differ; first at (b, c, y, x) = {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}"


ALL = [("fwd", n) for n in FWD_CASES] + [("dgrad", n) for n in DGRAD_CASES]


def _xshape(direction, name):
    return (FWD_CASES if direction == "fwd" else DGRAD_CASES)[name][:4]


@pytest.mark.parametrize("direction,name", ALL)
def test_gather_is_exact_on_grid_operands(direction, name, log):
    op = operands(direction, name)
    got = run(direction, log, op["ag"], op["wg"], _xshape(direction, name))
    assert got.shape == op["rg"].shape
    assert torch.equal(got, op["rg"]), f"{direction} {name}: " + _first_difference(got, op["rg"])


@pytest.mark.parametrize("direction,name", ALL)
def test_gather_is_within_the_winograd_bound_on_normal_operands(direction, name, log):
    op = operands(direction, name)
    got = run(direction, log, op["an"], op["wn"], _xshape(direction, name))
    err = float((got.double() - op["rn"]).abs().max() / op["rn"].abs().max())
    print(f"{direction} {name}: max |error| / max |reference| = {err:.3e} (bound {TOL:.0e})")
    assert err <= TOL, f"{direction} {name}: max error / max |ref| = {err:.3e} > {TOL:.0e}"


@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
def test_halo_rows_and_columns_read_zeros(direction, log):
    """a one-hot operand at the image corners: the halo rows / columns of the Winograd patches must read zeros, not the neighbouring row,
    image or channel (the buffer offsets of out-of-image pixels alias valid memory: they are masked, not range-checked)"""
    B, Cin, H, W, Cout = (FWD_CASES if direction == "fwd" else DGRAD_CASES)["one-chunk"]
    a = torch.zeros((B, Cin, H, W) if direction == "fwd" else (B, Cout, H // 2, W // 2))
    a[:, :, 0, 0] = 1.0
    a[:, :, -1, -1] = 2.0
    a[:, :, 0, -1] = 3.0
    a[:, :, -1, 0] = 5.0
    w = torch.randn(Cout, Cin, 4, 4, generator=torch.Generator().manual_seed(5))
    got = run(direction, log, a, w, (B, Cin, H, W))
    ref = _ref(direction, a, w, (B, Cin, H, W)).float()
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
