"""Bit-exact sweep of the convolution engine: every arithmetic mode, both 16-bit storage modes, every main conv kernel.

Every operand is drawn from a small dyadic grid (integers |k| <= 4, or ternary {-1, 0, 1} on the production-size layers, times a
power of two per tensor).  Every product and every partial sum the engine can form is then exactly representable in fp32, in any order
and in any mode: the bf16 / f16 / bf16x3 / bf16x6 / f16x3 splits leave their lower planes zero, the f16x3 power-of-two scaling is exact,
the Winograd transforms use only 0.5 and +-1, and slab sums add exact fp32 partials.  So the correct result is known exactly (torch's CPU
convolution in float64) and every kernel's output must equal it bit for bit -- or, with 16-bit activation storage, equal it rounded once
to nearest-even.  A wrong tap, channel, halo, tile, split or lane fails with zero tolerance.

The sweep runs once per module (fixture `sweep`): one fp64 reference per geometry, shared by all modes.  A launch observer records
which kernel the library ran for every (mode, case, phase); `test_the_sweep_reaches_every_conv_kernel` checks that the table below
still reaches every main kernel, so a change to the planning rules that moves a case off its intended kernel cannot pass silently.
Routing notes in the table name what the default plan takes in the fp32 mode (f32) and in the one-plane 16-bit modes (16).
"""
import ctypes
import importlib
import multiprocessing as mp
import os
import re
import time
import traceback

import pytest
import torch

from helpers import collect_from_children

pytestmark = pytest.mark.gpu
DEV = "cuda"

HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")
from oracle import attngan_oracle as O   # noqa: E402  (checker only: upsample2)

# mode -> (precision, activation storage)
MODES = {
    "f32": (L.PREC_F32, None),
    "bf16x6": (L.PREC_BF16X6, None),
    "f16x3": (L.PREC_F16X3, None),
    "bf16x3": (L.PREC_BF16X3, None),
    "bf16": (L.PREC_BF16, None),
    "f16": (L.PREC_F16, None),
    "bf16+s16": (L.PREC_BF16, "bf16"),
    "f16+s16": (L.PREC_F16, "f16"),
}
STORAGE_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16}

# power-of-two grid steps: x, w, dy (and a bias on the grid of y).  Units of y / dx / dw: 2^-5, 2^-4, 2^-3 -- every operand, output and
# stored value is a normal number of fp32, bf16 and f16 (f16 keeps nonzero magnitudes in [2^-14, 2^15): see _check_budget)
EX, EW, EDY = -2, -3, -1
BUDGET = 2 ** 20          # largest exact partial sum in grid units: 16x headroom below fp32's 24 bits

CASES = [
    # kind, B, Cin, H, W, Cout, flags ("b": bias, "t": ternary operands, "k1": 1x1 kernel).  Comment: the main kernel of forward / data
    # gradient / weight gradient in the f32 mode, then in the one-plane 16-bit modes ("16"; "/in16": 16-bit input under 16-bit storage),
    # as the first MI355X run recorded them.  The two-plane modes (bf16x3, f16x3, bf16x6) take the patch kernels wherever "16" names p16.
    # gather<N> = conv_gather_f32_kernel with N-channel tiles; rows = conv_wgrad_rows_kernel; p16 gk<G> = conv_p16_kernel, geometry kind G
    # ---- k-table gather: the three cout tiles, with and without K split; the fp32 weight gradients -------------------------------------
    ("same", 2, 64, 8, 8, 128, "b"),        # f32: gather128 (K split 2) / gather64 (K split 4) / conv_wgrad_f32; 16: p16 gk0 / p16 gk0 / rows
    ("down", 2, 16, 32, 32, 128, "b"),      # f32: gather128 unsplit / gather32 K split / conv_wgrad_f32; 16: p16 gk2 / p16 gk1 / rows gk2
    ("same", 2, 24, 12, 20, 72, ""),        # f32: gather64 / gather32 / rows; 16: rows of 20 are not whole 16-byte blocks of 16-bit values ->
                                            #   p16 on fp32 input even under 16-bit storage / p16 / conv_patch_wgrad
    ("same", 3, 16, 24, 40, 36, ""),        # f32: gather32, cout tile 36 of 64 / gather32 / rows; 16: p16 / patch (dgrad Cin 36 % 8 != 0) / rows
    ("same", 1, 264, 8, 8, 64, ""),         # last 32-channel chunk holds 8: f32 gather64 (K split) / gather128 / conv_wgrad_f32; 16: p16 (9 stages)
    ("same", 1, 257, 8, 8, 40, ""),         # one channel in the last chunk: f32 gather32; 16: Cin % 8 != 0 -> patch / p16 / rows
    ("same", 2, 32, 8, 8, 48, "k1b"),       # 1x1 conv: gather64 / gather32 / conv_wgrad_f32 in every mode (16-bit output under storage)
    ("same", 3, 48, 1, 1, 64, "b"),         # 3x3 on 1x1 maps: gather64 / gather64 / conv_wgrad_f32 in every mode
    # ---- fp32 Winograd ---------------------------------------------------------------------------------------------------------------
    ("same", 8, 16, 64, 64, 128, ""),       # f32: conv_wino_h / gather32 / rows (fp32 operands); 16: p16 / p16 / rows
    ("same", 8, 16, 64, 64, 100, ""),       # f32: conv_wino_f32 (Cout % 8 != 0) / gather32 / rows; 16: p16, partial cout tile / patch / rows
    ("same", 2, 40, 128, 128, 72, ""),      # f32: conv_wino_h / conv_wino_h / conv_wino_wgrad; 16: p16, last stage 8 of 32 channels / p16 / rows
    ("same", 4, 8, 128, 128, 36, ""),       # f32: conv_wino_f32 <2> (Cout < 96, Cout % 8 != 0: 64 tiles x 64 channels, 256 blocks -- the smallest that
                                            #   the plan takes) / gather32 / rows
    ("down", 16, 16, 128, 128, 128, ""),    # f32: conv_wino_s2 / gather32 / conv_wgrad_f32; 16: p16 gk2 / p16 gk1 / rows gk2
    ("down", 16, 128, 64, 64, 32, ""),      # f32: gather32 / conv_wino_cls / conv_wgrad_f32; 16: p16 gk2 / p16 gk1, both column classes / rows
    # ---- <= 4 output channels: vector-ALU kernels, fp32 arithmetic in every mode ---------------------------------------------------------------
    ("same", 2, 32, 64, 64, 3, "b"),        # conv_small_strip (channels split over the waves) / gather32 / wgrad_small_strip
    ("same", 1, 5, 128, 128, 3, ""),        # conv_small_strip (one channel group) / gather32 / wgrad_small_strip
    ("same", 2, 8, 50, 50, 3, "b"),         # rows of 50 are not whole 4-pixel strips: conv_small_n <9, 3> / gather32 / wgrad_small_n
    ("down", 2, 3, 64, 64, 16, "b"),        # RGB input: gather32 (Cin <= 4) / conv_small_dgrad4_strip / conv_wgrad_f32
    ("down", 2, 16, 16, 16, 1, ""),         # conv_small_n <16, 4> / gather32 / conv_wgrad_f32
    ("same", 1, 8, 64, 64, 2, ""),          # 2 channels: conv_small_strip <NC 2, channels split> / gather32 / wgrad_small_strip <NC 2>
    ("same", 1, 5, 64, 64, 4, ""),          # 4 channels: conv_small_strip <NC 4, one channel group> / gather32 / wgrad_small_strip <NC 4>
    ("down", 1, 2, 8, 8, 8, ""),            # data gradient to 2 channels: conv_small_dgrad4_strip <NC 2, channels split>
    ("down", 1, 4, 8, 8, 6, ""),            # data gradient to 4 channels: conv_small_dgrad4_strip <NC 4, one channel group>
    ("linear", 6, 40, 1, 1, 1, "b"),        # nn.Linear to 1 output: linear_small_n / gather32 / conv_wgrad_f32
    ("linear", 5, 256, 1, 1, 100, "b"),     # nn.Linear 256 -> 100 as 1x1 maps, tiles spanning images: gather128 / gather128 / conv_wgrad_f32
    # ---- row-block gather, patch kernels, row-resident weight gradient -----------------------------------------------------------------------
    ("same", 2, 12, 16, 16, 64, ""),        # 16: Cin % 8 != 0 -> patch / p16 / rows, two 32-channel chunks (f32: gather64 / gather32 / rows)
    ("same", 5, 64, 8, 8, 160, ""),         # 8x8 maps: tiles span two images, ragged last tile (B = 5), two cout tiles; 16: p16 / p16 / rows
    ("same", 2, 64, 8, 128, 128, ""),       # rows wgrad: two 64-column tiles per row, halo blocks loaded; 16: p16 / p16 / rows
    ("same", 2, 32, 16, 64, 96, ""),        # rows wgrad: one tile per row, cout tile not full
    ("same", 2, 72, 16, 32, 64, ""),        # rows wgrad: <= 64 output channels, odd chunk count (72 = 2 x 32 + 8)
    ("same", 2, 16, 4, 4, 32, "b"),         # 4x4 maps: 16: patch / patch / conv_patch_wgrad (rows need 8 columns); f32: gather32 / conv_wgrad_f32
    ("same", 1, 8, 4, 512, 32, ""),         # rows of 512: 16: p16 / p16 / rows
    ("same", 1, 16, 2, 1024, 48, ""),       # rows of 1024, two rows: 16: p16 / p16 / rows
    ("same", 1, 32, 24, 40, 96, "b"),       # non-square, batch 1: 16: p16 / p16 / rows
    ("down", 3, 48, 32, 32, 80, ""),        # 16: p16 gk2, 3 stages of 16 / p16 gk1, both column classes / rows gk2, cout tile not full
    ("down", 6, 128, 16, 16, 64, "b"),      # 8x8 outputs, tiles of two images: 16: p16 gk2 / p16 gk1 / rows gk2
    ("down", 2, 32, 8, 8, 64, ""),          # 4x4 outputs: 16: patch (p16 gk2 on 16-bit input) / patch / conv_patch_wgrad
    ("down", 1, 16, 8, 1024, 32, ""),       # 4 x 512 outputs: 16: p16 gk2 / p16 gk1 / rows gk2
    ("down", 2, 12, 16, 24, 40, ""),        # Cin % 8 != 0: 16: patch / p16 gk1 / conv_patch_wgrad (rows of 12 outputs)
    ("up", 2, 64, 8, 32, 64, ""),           # upsample conv: f32 gather64 / gather64 / conv_wgrad_f32; 16: p16 gk1, both column classes / p16 gk2 /
                                            #   rows on the upsampled image built in LDS
    ("up", 2, 32, 16, 64, 128, ""),         # -> 32 x 128: 16: p16 gk1 / p16 gk2 / rows (upsample form) with halo, 128-channel tile
    ("up", 1, 32, 4, 4, 64, ""),            # 4x4 -> 8x8, batch 1: 16: patch / patch / rows (upsample form)
    ("up", 2, 12, 8, 8, 48, ""),            # Cin % 8 != 0: 16: patch on the folded classes / p16 gk2 / rows (upsample form)
    ("same", 2, 32, 16, 16, 256, ""),       # 256 output channels (two p16 128-channel tiles; one 256-channel tile under AGAN_P16_TILE=2)
    ("up", 1, 32, 8, 8, 224, ""),           # 224 output channels, batch 1: the smallest cout of AGAN_P16_TILE=2
    # ---- production layers of the metric configuration (ternary operands: the weight gradient sums B*OH*OW terms) -----------------------------
    ("same", 24, 32, 64, 64, 64, "t"),      # generator conv3x3 at 64 px: f32 conv_wino_h / conv_wino_h / conv_wino_wgrad; 16: p16 / p16 / rows
    ("up", 24, 32, 64, 64, 64, "t"),        # generator upsample conv 64 -> 128 px: f32 gather64 / gather32 / conv_wgrad_f32; 16: p16 gk1 / gk2 / rows
    ("up", 8, 32, 128, 128, 64, "t"),       # 128 -> 256 px, batch 8 of 24 (B*OH*OW <= 2^20): the kernels of the row above; 2^19 output pixels
                                            #   fill far more than one round of workgroups, so no split rule changes with the batch
    ("down", 48, 64, 128, 128, 128, "t"),   # discriminator 4x4 s2, real + fake batch: f32 conv_wino_s2 / gather64 / conv_wgrad_f32; 16: p16 gk2 / gk1
    ("down", 48, 256, 32, 32, 512, "t"),    # f32: conv_wino_s2 / conv_wino_cls / conv_wgrad_f32; 16: p16 gk2 / p16 gk1 / rows gk2
]


def case_id(c):
    kind, B, Cin, H, W, Cout, flags = c
    return f"{kind}-B{B}-{Cin}x{H}x{W}-{Cout}" + (f"-{flags}" if flags else "")


CASE_BY_ID = {case_id(c): c for c in CASES}
# layers whose forward has no 16-bit-output kernel: under 16-bit storage they return fp32 (besides the <= 4-channel ones, the patch-kernel
# routes, which take fp32 tensors only)
FP32_OUTPUT_UNDER_STORAGE = {"same-B1-257x8x8-40", "same-B2-12x16x16-64", "same-B2-16x4x4-32-b", "down-B2-12x16x24-40", "up-B1-32x4x4-64",
                             "up-B2-12x8x8-48"}
assert len(CASE_BY_ID) == len(CASES)


def _ksize(kind, flags):
    if kind == "linear" or "k1" in flags:
        return 1
    return 4 if kind == "down" else 3


def _grid(shape, gen, exp, ternary):
    """integers in [-4, 4] (or {-1, 0, 1}), uniform -- sign-balanced, zeros included -- times 2^exp"""
    lim = 1 if ternary else 4
    return torch.randint(-lim, lim + 1, shape, generator=gen, dtype=torch.int64).double() * 2.0 ** exp


def _conv_ref(kind, x, w, b, k):
    F = torch.nn.functional
    if kind == "down":
        return F.conv2d(x, w, b, 2, 1)
    if kind == "up":
        return F.conv2d(O.upsample2(x), w, b, 1, 1)
    return F.conv2d(x, w, b, 1, k // 2)


def _check_budget(c, x, w, dy, b):
    """every partial sum stays within BUDGET grid units (exact in fp32 with 16x headroom)"""
    kind, B, Cin, H, W, Cout, flags = c
    k = _ksize(kind, flags)
    r = lambda t, e: int((t.abs().max() / 2.0 ** e).item())       # noqa: E731
    rx, rw, rdy = r(x, EX), r(w, EW), r(dy, EDY)
    OH, OW = dy.shape[2], dy.shape[3]
    terms = {
        "forward": Cin * k * k * rx * rw + (r(b, EX + EW) if b is not None else 0),
        "data gradient": Cout * k * k * (4 if kind == "up" else 1) * rdy * rw,
        "weight gradient": B * OH * OW * rx * rdy,
    }
    for what, t in terms.items():
        assert t <= BUDGET, f"{case_id(c)}: {what} sums {t} grid units > 2^20: not exact in fp32 -- use ternary operands or a smaller batch"


_REF_CACHE = {}


def reference(c):
    """-> dict of CPU tensors: operands (fp32, on the grid) and the exact fp32 results, computed once per geometry in float64"""
    cid = case_id(c)
    hit = _REF_CACHE.get(cid)
    if hit is not None:
        return hit
    kind, B, Cin, H, W, Cout, flags = c
    k = _ksize(kind, flags)
    tern = "t" in flags
    gen = torch.Generator().manual_seed(sum(map(ord, cid)))
    x = _grid((B, Cin, H, W), gen, EX, tern).requires_grad_(True)
    w = _grid((Cout, Cin, k, k), gen, EW, tern).requires_grad_(True)
    b = _grid((Cout,), gen, EX + EW, tern).requires_grad_(True) if "b" in flags else None
    y = _conv_ref(kind, x, w, b, k)
    dy = _grid(tuple(y.shape), gen, EDY, tern)
    _check_budget(c, x.detach(), w.detach(), dy, b)
    y.backward(dy)
    f = lambda t: None if t is None else t.detach().float()        # noqa: E731  (exact: every value fits fp32's 24 bits)
    ref = dict(x=f(x), w=f(w), b=f(b), dy=f(dy), y=f(y), dx=f(x.grad), dw=f(w.grad), db=f(b.grad) if b is not None else None)
    for key in ("y", "dx", "dw", "db"):
        if ref[key] is not None:
            assert torch.equal(ref[key].double(), dict(y=y, dx=x.grad, dw=w.grad, db=b.grad if b is not None else None)[key].detach()), \
                f"{cid}: {key} not exact in fp32"
    _REF_CACHE[cid] = ref
    return ref


class set_mode:
    def __init__(self, name):
        self.prec, self.storage = MODES[name]

    def __enter__(self):
        HF.set_precision(self.prec)
        HF.set_activation_storage(self.storage)
        return self

    def __exit__(self, *exc):
        HF.set_activation_storage(None)
        HF.set_precision(L.PREC_F32)
        return False


class KernelLog:
    """launch observer (as bench.py's ConvTimer): arms the library's timer hook before every conv-engine call and asks it afterwards which
    main kernel ran (agan_timer_last_kernel: the demangled symbol) and with which split (agan_timer_last_split: K split of a gather,
    pixel split of a weight gradient; 1 = unsplit).  seen: {phase: (kernel, split)}"""

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
        self.seen[self.phase] = (self.name.value.decode() or "unknown", int(L.load().agan_timer_last_split()))

    def take(self):
        seen, self.seen = self.seen, {}
        return seen


def mismatch(what, got, want):
    """'' if got equals want bit for bit (+0 == -0), else a report: differing count, first index, got / want"""
    got = got.detach()
    want = want.to(got.device)
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{what}: {got.dtype} {tuple(got.shape)} vs expected {want.dtype} {tuple(want.shape)}"
    ne = got != want
    n = int(ne.sum())
    if n == 0:
        return ""
    idx = tuple(int(i) for i in ne.nonzero()[0])
    return f"{what}: {n} of {got.numel()} elements differ; first at {idx}: got {float(got[idx])!r}, want {float(want[idx])!r}"


def _lrelu(z):
    """the kernels' LeakyReLU on fp32 values: z > 0 ? z : 0.2f * z (one fp32 rounding)"""
    return torch.where(z > 0, z, z * torch.tensor(0.2, dtype=torch.float32))


def _inputs(c, mode, ref):
    storage = MODES[mode][1]
    tdt = STORAGE_DTYPE[storage] if storage else torch.float32
    xd = ref["x"].to(DEV).to(tdt).requires_grad_(True)
    wd = ref["w"].to(DEV).requires_grad_(True)
    bd = ref["b"].to(DEV).requires_grad_(True) if ref["b"] is not None else None
    return xd, wd, bd


def _forward(c, xd, wd, bd, **kw):
    kind, B, Cin, H, W, Cout, flags = c
    if kind == "linear":
        return HF.linear(xd.view(B, Cin), wd.view(Cout, Cin), bd, **kw).view(B, Cout, 1, 1)
    return HF.conv2d(xd, wd, bd, kind, **kw)


def y_dtype(c, mode):
    """the dtype conv2d must return: the storage type under 16-bit storage, except where no kernel of the layer writes 16 bits"""
    storage = MODES[mode][1]
    if storage is None or c[5] <= 4 or case_id(c) in FP32_OUTPUT_UNDER_STORAGE:
        return torch.float32
    return STORAGE_DTYPE[storage]


def run_case(c, mode, ref):
    """forward + backward of one case in one mode -> list of mismatch reports (empty: bit-exact).  (The data gradient comes back in
    x's dtype whatever the kernel wrote: autograd casts it.)"""
    xd, wd, bd = _inputs(c, mode, ref)
    y = _forward(c, xd, wd, bd)
    y.backward(ref["dy"].to(DEV).to(y.dtype))
    out = [mismatch("forward", y, ref["y"].to(y_dtype(c, mode))),
           mismatch("data gradient", xd.grad, ref["dx"].to(xd.dtype)),
           mismatch("weight gradient", wd.grad, ref["dw"])]
    if bd is not None:
        out.append(mismatch("bias gradient", bd.grad, ref["db"]))
    return [m for m in out if m]


def run_sweep(cases, modes):
    """-> ({(mode, case id): [mismatch reports or an exception]}, {(mode, case id, phase): (kernel, split)}, cpu seconds, gpu seconds)"""
    log = KernelLog()
    results, kernels = {}, {}
    cpu = gpu = 0.0
    HF.set_launch_observer(log)
    try:
        for c in cases:
            t0 = time.perf_counter()
            ref = reference(c)
            cpu += time.perf_counter() - t0
            t0 = time.perf_counter()
            for mode in modes:
                with set_mode(mode):
                    try:
                        results[(mode, case_id(c))] = run_case(c, mode, ref)
                    except L.AganError as e:
                        results[(mode, case_id(c))] = [f"library error: {e}"]
                for phase, ran in log.take().items():
                    kernels[(mode, case_id(c), phase)] = ran
            torch.cuda.synchronize()
            gpu += time.perf_counter() - t0
            _REF_CACHE.pop(case_id(c), None)       # (each geometry is swept once: keep host memory flat)
    finally:
        HF.set_launch_observer(None)
    return results, kernels, cpu, gpu


def short(name):
    """'void agan::conv::(anonymous namespace)::conv_p16_kernel<0, 1, ...>(...)' -> 'conv_p16_kernel<0, 1, ...>'"""
    m = re.search(r"(\w+_kernel\d*)(<[^()]*>)?", name)
    return (m.group(1) + (m.group(2) or "")) if m else name


def show(ran):
    """(kernel, split) -> 'conv_gather_f32_kernel<...> /2' (the split factor after the slash when the launch was split)"""
    name, split = ran
    return short(name) + (f" /{split}" if split > 1 else "")


def template_args(name, kernel):
    m = re.search(rf"\b{kernel}<([^()]*)>", name)
    return [a.strip() for a in m.group(1).split(",")] if m else None


@pytest.fixture(scope="module")
def sweep():
    results, kernels, cpu, gpu = run_sweep(CASES, list(MODES))
    print(f"\nconv exact sweep: {len(CASES)} geometries x {len(MODES)} modes; fp64 CPU references {cpu:.1f} s, GPU runs (incl. checks) {gpu:.1f} s")
    for mode in MODES:
        print(f"-- kernels reached in mode {mode}")
        for c in CASES:
            cid = case_id(c)
            row = "  ".join(f"{ph}={show(kernels[(mode, cid, ph)]) if (mode, cid, ph) in kernels else '-'}" for ph in ("fwd", "dgrad", "wgrad"))
            print(f"   {cid:34s} {row}")
    return results, kernels


@pytest.mark.parametrize("case", list(CASE_BY_ID))
@pytest.mark.parametrize("mode", list(MODES))
def test_conv_is_bit_exact_on_grid_operands(sweep, mode, case):
    results, kernels = sweep
    bad = results[(mode, case)]
    ran = ", ".join(f"{ph}: {show(kernels[(mode, case, ph)])}" for ph in ("fwd", "dgrad", "wgrad") if (mode, case, ph) in kernels)
    assert not bad, f"{mode} {case} ({ran}):\n  " + "\n  ".join(bad)


# Main kernels the table must reach, per mode that routes there: (name, template arguments where the form matters, split) -- split None: any,
# 1: an unsplit launch, "split": a K- or pixel-split launch, n: exactly that split factor.  The p16 kernel's arguments are
# <ET, GK, BN, IN16, OUT16, NI, PX2, WC, LPX>; the k-table gather's <BM, BN, WM, WN, ODT>; the row-resident weight gradient's
# <ET, NPL, GK, CI2, X16, Y16, NIX, NIY, PC, UPS>.
GATHER_TILES = [("conv_gather_f32_kernel", {1: bn}, split) for bn in ("128", "64", "32") for split in (1, "split")]
F32_KERNELS = GATHER_TILES + [
    ("conv_wino_h_f32_kernel", {}, None), ("conv_wino_f32_kernel", {0: "4"}, None), ("conv_wino_f32_kernel", {0: "2"}, None),
    ("conv_wino_s2_f32_kernel", {}, None),
    ("conv_wino_cls_f32_kernel", {}, None), ("conv_wino_wgrad_f32_kernel", {}, None), ("conv_wgrad_f32_kernel", {}, None),
    ("conv_wgrad_rows_kernel", {}, None),
]
SMALL_KERNELS = [(k, {}, None) for k in ("conv_small_n_kernel", "conv_small_strip_kernel", "conv_small_dgrad4_strip_kernel",
                                         "wgrad_small_n_kernel", "wgrad_small_strip_kernel", "linear_small_n_kernel")]
PATCH_KERNELS = [("conv_patch_kernel2", {}, None), ("conv_patch_wgrad_kernel", {}, None)]
ROWS = [("conv_wgrad_rows_kernel", {}, None)]
ROWS_UP = [("conv_wgrad_rows_kernel", {9: "true"}, None)]
P16_F32_IN = [("conv_p16_kernel", {1: gk, 3: "false"}, None) for gk in ("0", "1", "2")]
P16_16_IN = [("conv_p16_kernel", {1: gk, 3: "true"}, None) for gk in ("0", "1", "2")]
P16_SPLIT = [("conv_p16_kernel", {}, "split"), ("conv_p16_kernel", {}, 1)]
EXPECTED_KERNELS = {
    "f32": F32_KERNELS + SMALL_KERNELS,
    "bf16x6": PATCH_KERNELS + ROWS + SMALL_KERNELS,
    "f16x3": PATCH_KERNELS + ROWS + SMALL_KERNELS,
    "bf16x3": PATCH_KERNELS + ROWS + ROWS_UP + SMALL_KERNELS,
    "bf16": P16_F32_IN + P16_SPLIT + PATCH_KERNELS + ROWS + ROWS_UP + SMALL_KERNELS,
    "f16": P16_F32_IN + P16_SPLIT + PATCH_KERNELS + ROWS + ROWS_UP + SMALL_KERNELS,
    "bf16+s16": P16_16_IN + [P16_F32_IN[0]] + P16_SPLIT + PATCH_KERNELS + [("conv_wgrad_rows_kernel", {4: "true"}, None)] + ROWS_UP + SMALL_KERNELS,
    "f16+s16": P16_16_IN + [P16_F32_IN[0]] + P16_SPLIT + PATCH_KERNELS + [("conv_wgrad_rows_kernel", {4: "true"}, None)] + ROWS_UP + SMALL_KERNELS,
}
# the launches the table's comments label as split or unsplit (split factors from the plans: plan_gather, plan_p16)
LABELLED_SPLITS = [
    ("f32", "same-B2-64x8x8-128-b", "fwd", ("conv_gather_f32_kernel", {1: "128"}, 2)),
    ("f32", "same-B2-64x8x8-128-b", "dgrad", ("conv_gather_f32_kernel", {1: "64"}, 4)),
    ("f32", "down-B2-16x32x32-128-b", "fwd", ("conv_gather_f32_kernel", {1: "128"}, 1)),
    ("f32", "down-B2-16x32x32-128-b", "dgrad", ("conv_gather_f32_kernel", {1: "32"}, 2)),
    ("f32", "same-B2-24x12x20-72", "fwd", ("conv_gather_f32_kernel", {1: "64"}, 1)),
    ("f32", "same-B3-16x24x40-36", "fwd", ("conv_gather_f32_kernel", {1: "32"}, 1)),
    ("f32", "same-B1-264x8x8-64", "fwd", ("conv_gather_f32_kernel", {1: "64"}, 9)),
    ("bf16", "same-B1-264x8x8-64", "fwd", ("conv_p16_kernel", {1: "0", 3: "false"}, 2)),
    ("f16+s16", "same-B1-264x8x8-64", "fwd", ("conv_p16_kernel", {1: "0", 3: "true"}, 2)),
]


def _matches(name, kernel, args):
    if not re.search(rf"\b{kernel}\b", name):
        return False
    if not args:
        return True
    have = template_args(name, kernel)
    return have is not None and all(i < len(have) and have[i] == v for i, v in args.items())


def reached(ran, spec):
    """does a recorded launch (kernel, split) fit spec (kernel, template arguments, split)?"""
    (name, split), (kernel, args, want) = ran, spec
    if not _matches(name, kernel, args):
        return False
    return want is None or (split > 1 if want == "split" else split == want)


def test_the_sweep_reaches_every_conv_kernel(sweep):
    _, kernels = sweep
    missing = []
    for mode, want in EXPECTED_KERNELS.items():
        ran = [r for (m, _, _), r in kernels.items() if m == mode]
        for spec in want:
            if not any(reached(r, spec) for r in ran):
                missing.append(f"{mode}: {spec}")
    for mode, cid, phase, spec in LABELLED_SPLITS:
        r = kernels.get((mode, cid, phase))
        if r is None or not reached(r, spec):
            missing.append(f"{mode} {cid} {phase}: wanted {spec}, ran {show(r) if r else 'nothing'}")
    assert not missing, "kernels / splits no case of the table reaches any more:\n  " + "\n  ".join(missing)


# ---- epilogues and in-place accumulation ---------------------------------------------------------------------------------------------------
EPILOGUE_CASES = [
    # case, mode, the forward kernel (LeakyReLU epilogue), the data-gradient kernel (mask epilogue): (name, template arguments, split)
    ("same-B2-64x8x8-128-b", "bf16", ("conv_p16_kernel", {3: "false"}, None), ("conv_p16_kernel", {3: "false"}, None)),
    ("same-B2-64x8x8-128-b", "f16+s16", ("conv_p16_kernel", {3: "true", 4: "true"}, None), ("conv_p16_kernel", {3: "true", 4: "true"}, None)),
    ("same-B2-12x16x16-64", "bf16", ("conv_patch_kernel2", {}, None), ("conv_p16_kernel", {}, None)),
    ("same-B2-12x16x16-64", "bf16x3", ("conv_patch_kernel2", {}, None), ("conv_patch_kernel2", {}, None)),
    # f32 gather: unsplit forward, K-split data gradient; K-split forward (the epilogues then run in the slab sum)
    ("down-B2-16x32x32-128-b", "f32", ("conv_gather_f32_kernel", {1: "128"}, 1), ("conv_gather_f32_kernel", {1: "32"}, 2)),
    ("same-B2-64x8x8-128-b", "f32", ("conv_gather_f32_kernel", {1: "128"}, 2), ("conv_gather_f32_kernel", {1: "64"}, 4)),
]


def _case_and_ref(cid):
    c = CASE_BY_ID[cid]
    return c, reference(c)


class observed:
    """`with observed() as log:` -- a KernelLog installed as the launch observer for the block"""

    def __enter__(self):
        self.log = KernelLog()
        HF.set_launch_observer(self.log)
        return self.log

    def __exit__(self, *exc):
        HF.set_launch_observer(None)
        return False


def _ran(log, phase, spec, what):
    """'' if the launch of `phase` fits spec, else a report"""
    r = log.seen.get(phase)
    return "" if (r is not None and reached(r, spec)) else f"{what}: wanted {spec}, ran {show(r) if r else 'nothing'}"


@pytest.mark.parametrize("cid,mode,fwd,dgrad", EPILOGUE_CASES)
def test_fused_leaky_relu_epilogue_is_exact(cid, mode, fwd, dgrad):
    c, ref = _case_and_ref(cid)
    with set_mode(mode), observed() as log:
        xd, wd, bd = _inputs(c, mode, ref)
        with torch.no_grad():
            y = _forward(c, xd, wd, bd, act=L.ACT_LRELU)
    bad = [m for m in (_ran(log, "fwd", fwd, "forward kernel"),
                       mismatch("LeakyReLU forward", y, _lrelu(ref["y"]).to(y_dtype(c, mode)))) if m]
    assert not bad, f"{mode} {cid}: " + "; ".join(bad)


@pytest.mark.parametrize("cid,mode,fwd,dgrad", EPILOGUE_CASES)
def test_leaky_relu_mask_in_the_dgrad_epilogue_is_exact(cid, mode, fwd, dgrad):
    """the consumer's data-gradient epilogue multiplies by LeakyReLU'(its input) (HF.ActHandoff): x > 0 ? dx : 0.2f * dx"""
    c, ref = _case_and_ref(cid)
    with set_mode(mode), observed() as log:
        xd, wd, bd = _inputs(c, mode, ref)
        y = _forward(c, xd, wd, bd, handoff_in=HF.ActHandoff())
        y.backward(ref["dy"].to(DEV).to(y.dtype))
    want = torch.where(ref["x"] > 0, ref["dx"], ref["dx"] * torch.tensor(0.2, dtype=torch.float32))
    bad = [m for m in (_ran(log, "dgrad", dgrad, "data-gradient kernel"), mismatch("masked data gradient", xd.grad, want.to(xd.dtype)),
                       mismatch("weight gradient", wd.grad, ref["dw"])) if m]
    assert not bad, f"{mode} {cid}: " + "; ".join(bad)


ACCUMULATE_CASES = [
    # case, mode, the weight-gradient kernel that must take the accumulating call
    ("down-B2-16x32x32-128-b", "f32", ("conv_wgrad_f32_kernel", {}, "split")),    # pixel split: adds in its slab sum; bias gradient
    ("same-B2-32x8x8-48-k1b", "f32", ("conv_wgrad_f32_kernel", {}, 1)),           # unsplit: adds in the kernel's own epilogue
    ("same-B2-40x128x128-72", "f32", ("conv_wino_wgrad_f32_kernel", {}, None)),   # the transposing slab sum adds
    ("same-B8-16x64x64-128", "f32", ("conv_wgrad_rows_kernel", {}, None)),        # fp32 operands
    ("same-B2-12x16x16-64", "bf16", ("conv_wgrad_rows_kernel", {}, None)),        # one plane
    ("up-B2-64x8x32-64", "f16+s16", ("conv_wgrad_rows_kernel", {4: "true", 9: "true"}, None)),  # upsample form, 16-bit storage
    ("same-B2-16x4x4-32-b", "bf16x3", ("conv_patch_wgrad_kernel", {}, None)),
    ("same-B2-32x64x64-3-b", "f32", ("wgrad_small_strip_kernel", {}, None)),
    ("same-B2-8x50x50-3-b", "f32", ("wgrad_small_n_kernel", {}, None)),
]


@pytest.mark.parametrize("cid,mode,wgrad", ACCUMULATE_CASES)
def test_second_backward_accumulates_in_place_exactly(cid, mode, wgrad):
    """gradients into registered flat-buffer slices (HF.GradDst, as optim.py wires them): the first backward overwrites, the second
    reaches the kernels' accumulate flag and must leave exactly twice the gradient"""
    c, ref = _case_and_ref(cid)
    nw = ref["w"].numel()
    nb = ref["b"].numel() if ref["b"] is not None else 0
    flat = torch.full((nw + nb,), 7.0, device=DEV)           # (stale values: the first backward must overwrite them)
    HF.register_flat(flat)
    wdst = HF.GradDst(flat, 0, nw)
    bdst = HF.GradDst(flat, nw, nb) if nb else None
    got, bad = [], []
    try:
        with set_mode(mode), observed() as log:
            xd, wd, bd = _inputs(c, mode, ref)
            for rep in range(2):
                y = _forward(c, xd, wd, bd, wdst=wdst, bdst=bdst)
                y.backward(ref["dy"].to(DEV).to(y.dtype))
                got.append(flat.clone())
                bad.append(_ran(log, "wgrad", wgrad, f"weight-gradient kernel of backward {rep + 1}"))
                log.take()
    finally:
        HF.unregister_flat(flat)
    assert wdst.edges == 2, f"expected two weight-gradient contributions into the flat slice, got {wdst.edges}"
    for rep, g in enumerate(got, 1):
        bad.append(mismatch(f"weight gradient after backward {rep}", g[:nw].view_as(ref["w"]), rep * ref["dw"]))
        if nb:
            bad.append(mismatch(f"bias gradient after backward {rep}", g[nw:], rep * ref["db"]))
    bad = [m for m in bad if m]
    assert not bad, f"{mode} {cid}: " + "; ".join(bad)


# ---- the register-tile forms of the row-block gather (AGAN_P16_TILE = 1 / 2), each in a fresh process -----------------------------------------
# The sweep's cases with >= 96 output channels (the register-tile forms need 96 for tile 1, 224 for tile 2; smaller layers keep the
# round-3 tile) in the one-plane modes.  Between them they must reach the WC = 2 form of every geometry kind.
P16_TILE_CASES = [c for c in CASES if c[5] >= 96 and c[0] != "linear"]
P16_TILE_MODES = ("bf16", "f16", "f16+s16")
P16_TILE_FORM = {1: {2: "128", 7: "2", 8: "8"}, 2: {2: "256", 7: "2", 8: "7"}}     # conv_p16_kernel <.., BN, .., WC, LPX> of each form


def _p16_tile_worker(tile, q):
    os.environ["AGAN_P16_TILE"] = str(tile)          # plan_p16 reads it once (a static): set before the first conv call
    try:
        results, kernels, _, _ = run_sweep(P16_TILE_CASES, P16_TILE_MODES)
        q.put(("ok", results, kernels))
    except BaseException:
        q.put(("error", traceback.format_exc(), None))


@pytest.mark.parametrize("tile", [1, 2])
def test_p16_register_tile_forms_are_bit_exact(tile):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_p16_tile_worker, args=(tile, q))
    p.start()
    try:
        (status, results, kernels), = collect_from_children(q, [p], timeout=300.0)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
    assert status == "ok", f"AGAN_P16_TILE={tile} child failed:\n{results}"
    print(f"\nAGAN_P16_TILE={tile}: conv_p16_kernel launches")
    for (mode, cid, phase), ran in sorted(kernels.items()):
        if "conv_p16_kernel" in ran[0]:
            print(f"   {mode:8s} {cid:30s} {phase:5s} {show(ran)}")
    bad = [f"{m} {cid}: " + "; ".join(r) for (m, cid), r in results.items() if r]
    assert not bad, f"AGAN_P16_TILE={tile}:\n  " + "\n  ".join(bad)
    for gk in ("0", "1", "2"):
        spec = ("conv_p16_kernel", {**P16_TILE_FORM[tile], 1: gk}, None)
        assert any(reached(r, spec) for r in kernels.values()), f"AGAN_P16_TILE={tile}: no case ran the form {spec}"
