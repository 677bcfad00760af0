"""The dynamic-memory kernels (csrc/memory.hip) through functional.memory_write / memory_read: outputs and every gradient within
helpers.RTOL (1e-3 of the tensor's largest magnitude) of the float64 CPU references, and bit-identical between two runs.

Read, B = 3: (C, T, H x W) = (4, 5, 6 x 6) | (64, 17, 18 x 18) | (8, 33, 16 x 16) -- the three word tiers (16 / 32 / 64) and the three
channel tiers, one workgroup with a ragged tail (36 pixels) and two workgroups whose partial slabs are summed (324 pixels; 256 fills
one exactly), the smallest and the largest channel count, ragged caption lengths with one sample of a single live word.  Each case
with and without a gradient at the attention map, and with the response layer's gradients written to / added into a flat slice.
Write: (B, T, Md) = (3, 5, 8) | (2, 17, 512)."""
import importlib

import pytest
import torch

from helpers import RTOL, assert_close
from memory_cases import assert_clear_of_zero, away_from_zero, mask_of

pytestmark = pytest.mark.gpu

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")

DEV = torch.device("cuda", 0)
B = 3
READ_CASES = [(4, 5, 6, 6), (64, 17, 18, 18), (8, 33, 16, 16)]
WRITE_CASES = [(3, 5, 8), (2, 17, 512)]


# ---------------------------------------------------------------------------------------------------------------------- read
_READ = {}


def read_case(C, T, H, W):
    """seeded inputs and the float64 reference (outputs, gradients with and without dattn), made once per shape and left unchanged"""
    key = (C, T, H, W)
    if key not in _READ:
        g = torch.Generator().manual_seed(100 + C + T)
        h = torch.randn(B, C, H, W, generator=g)
        kv = torch.relu(torch.randn(B, T, 2 * C, generator=g)) * (2.0 / C ** 0.5)     # keys and values are ReLU outputs; scores O(1)
        lens = [T, 1, T // 2 + 1]
        mask = mask_of(lens, T)
        rw, rb = torch.randn(1, 2 * C, 1, 1, generator=g) * 0.3, torch.randn(1, generator=g)
        dx, dattn = torch.randn(B, 2 * C, H, W, generator=g), torch.randn(B, T, H, W, generator=g)
        assert int(mask.sum(dim=1).min()) >= 1                  # every sample has a live word
        ref = {}
        for with_dattn in (False, True):
            leaves = [t.double().requires_grad_(True) for t in (h, kv, rw, rb)]
            x, attn = HF.memory_read_reference(leaves[0], leaves[1], mask, leaves[2], leaves[3])
            outs, gouts = ((x, attn), (dx.double(), dattn.double())) if with_dattn else ((x,), (dx.double(),))
            grads = torch.autograd.grad(outs, leaves, gouts)
            ref[with_dattn] = dict(x=x.detach(), attn=attn.detach(), dh=grads[0], dkv=grads[1], drw=grads[2], drb=grads[3])
        assert bool(torch.isfinite(ref[True]["x"]).all())
        assert float(ref[True]["attn"][1, 1:].abs().max()) == 0.0        # the single-live-word sample ignores every other word
        _READ[key] = dict(h=h, kv=kv, mask=mask, rw=rw, rb=rb, dx=dx, dattn=dattn, ref=ref)
    return _READ[key]


def run_read(case, with_dattn, accumulate, prefill):
    """one forward + backward on the device -> dict of outputs and gradients.  The response parameters own slices of a flat gradient
    buffer: `accumulate` marks them as already written in this backward, so the kernel must ADD to `prefill`; otherwise it overwrites."""
    h, kv = (case[k].to(DEV).requires_grad_(True) for k in ("h", "kv"))
    rw, rb = (torch.nn.Parameter(case[k].to(DEV)) for k in ("rw", "rb"))
    flat = prefill.to(DEV).clone()
    n = rw.numel()
    rw._agan_grad_dst, rb._agan_grad_dst = HF.GradDst(flat, 3, n), HF.GradDst(flat, 3 + n + 2, 1)
    rw._agan_grad_dst.written = rb._agan_grad_dst.written = bool(accumulate)
    x, attn = HF.memory_read(h, kv, case["mask"].to(DEV), rw, rb)
    outs, gouts = ((x, attn), (case["dx"].to(DEV), case["dattn"].to(DEV))) if with_dattn else ((x,), (case["dx"].to(DEV),))
    torch.autograd.backward(outs, gouts)
    torch.cuda.synchronize()
    return dict(x=x.detach(), attn=attn.detach(), dh=h.grad, dkv=kv.grad, flat=flat)


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("with_dattn", [False, True], ids=["dx", "dx+dattn"])
@pytest.mark.parametrize("C,T,H,W", READ_CASES)
def test_memory_read_vs_float64_and_twice(C, T, H, W, with_dattn, accumulate):
    case = read_case(C, T, H, W)
    ref = case["ref"][with_dattn]
    n = 2 * C
    g = torch.Generator().manual_seed(7)
    prefill = torch.randn(3 + n + 2 + 1 + 3, generator=g)
    if not accumulate:
        prefill[3:3 + n] = float("nan")                        # an overwrite must not read what was there
        prefill[3 + n + 2] = float("nan")
    got = run_read(case, with_dattn, accumulate, prefill)
    assert tuple(got["x"].shape) == (B, 2 * C, H, W) and tuple(got["attn"].shape) == (B, T, H, W)
    assert_close(got["x"], ref["x"], RTOL, "x")
    assert torch.equal(got["x"][:, :C], got["x"][:, C:])       # both halves are the response
    assert_close(got["attn"], ref["attn"], RTOL, "attn")
    assert float(got["attn"][1, 1:].abs().max()) == 0.0        # masked words get exactly zero
    assert_close(got["dh"], ref["dh"], RTOL, "dh")
    assert_close(got["dkv"], ref["dkv"], RTOL, "dkv")
    flat = got["flat"].cpu().double()
    base = prefill.double() if accumulate else torch.zeros_like(prefill, dtype=torch.float64)
    # what the slices hold: the gradient, or what was there plus the gradient
    assert_close(flat[3:3 + n], base[3:3 + n] + ref["drw"].reshape(-1), RTOL, "drw")
    assert_close(flat[3 + n + 2], base[3 + n + 2] + ref["drb"].reshape(()), RTOL, "drb")
    keep = torch.ones(prefill.numel(), dtype=torch.bool)
    keep[3:3 + n] = False
    keep[3 + n + 2] = False
    assert torch.equal(got["flat"].cpu()[keep], prefill[keep]), "the kernel wrote outside the parameters' slices"
    # the same inputs again: every output and gradient bit for bit
    again = run_read(case, with_dattn, accumulate, prefill)
    for k in ("x", "attn", "dh", "dkv"):
        assert torch.equal(got[k], again[k]), f"{k} differs between two runs"
    assert torch.equal(got["flat"][3:3 + n], again["flat"][3:3 + n]) and torch.equal(got["flat"][3 + n + 2], again["flat"][3 + n + 2])


def test_memory_read_without_flat_slices_and_with_an_unused_attention_map():
    """parameters without a flat destination get ordinary .grad tensors; an attention map nobody differentiates costs no gradient"""
    C, T, H, W = READ_CASES[0]
    case = read_case(C, T, H, W)
    ref = case["ref"][False]
    h, kv = (case[k].to(DEV).requires_grad_(True) for k in ("h", "kv"))
    rw, rb = (torch.nn.Parameter(case[k].to(DEV)) for k in ("rw", "rb"))
    x, attn = HF.memory_read(h, kv, case["mask"].to(DEV), rw, rb)
    x.backward(case["dx"].to(DEV))
    torch.cuda.synchronize()
    assert rw.grad.shape == rw.shape and rb.grad.shape == rb.shape
    assert_close(rw.grad, ref["drw"], RTOL, "drw")
    assert_close(rb.grad, ref["drb"], RTOL, "drb")
    assert_close(h.grad, ref["dh"], RTOL, "dh")


def test_memory_read_refuses_what_it_does_not_build():
    C, T, H, W = READ_CASES[0]
    case = read_case(C, T, H, W)
    h, kv, mask, rw, rb = (case[k].to(DEV) for k in ("h", "kv", "mask", "rw", "rb"))
    with pytest.raises(L.AganError, match="fp32 only"):
        HF.memory_read(h.bfloat16(), kv, mask, rw, rb)
    with pytest.raises(ValueError):
        HF.memory_read(h, kv[:, :, :-1], mask, rw, rb)
    with pytest.raises(L.AganError):
        HF.memory_read(torch.randn(1, 65, 4, 4, device=DEV), torch.randn(1, 3, 130, device=DEV), torch.ones(1, 3, dtype=torch.int64),
                       torch.randn(130, device=DEV), torch.randn(1, device=DEV))


# --------------------------------------------------------------------------------------------------------------------- write
@pytest.mark.parametrize("Bw,T,Md", WRITE_CASES)
def test_memory_write_vs_float64_and_twice(Bw, T, Md):
    g = torch.Generator().manual_seed(200 + Md)
    U = away_from_zero(torch.randn(Bw, T, Md + 1, generator=g))
    Q = away_from_zero(torch.randn(Bw, Md + 1, generator=g))
    dm = torch.randn(Bw, T, Md, generator=g)
    U64, Q64 = U.double().requires_grad_(True), Q.double().requires_grad_(True)
    assert_clear_of_zero(U=U64[..., :Md], Q=Q64[..., :Md])
    want = HF.memory_write_reference(U64, Q64)
    dU64, dQ64 = torch.autograd.grad(want, (U64, Q64), dm.double())

    def run():
        Ud, Qd = U.to(DEV).requires_grad_(True), Q.to(DEV).requires_grad_(True)
        m = HF.memory_write(Ud, Qd)
        m.backward(dm.to(DEV))
        torch.cuda.synchronize()
        return m.detach(), Ud.grad, Qd.grad
    m, dU, dQ = run()
    assert tuple(m.shape) == (Bw, T, Md)
    assert_close(m, want, RTOL, "m")
    assert_close(dU, dU64, RTOL, "dU")
    assert_close(dQ, dQ64, RTOL, "dQ")
    # the gate column has its own scale: bound it on its own
    assert_close(dU[..., Md], dU64[..., Md], RTOL, "dU gate")
    assert_close(dQ[..., Md], dQ64[..., Md], RTOL, "dQ gate")
    for a, b, what in zip((m, dU, dQ), run(), ("m", "dU", "dQ")):
        assert torch.equal(a, b), f"{what} differs between two runs"
