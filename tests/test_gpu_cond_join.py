"""The join kernels of the text-conditional discriminator head (csrc/cond_join.hip: agan_cond_join_fwd / agan_cond_join_bwd;
backend/functional.py: cond_join) and the one-launch loss (csrc/heads.hip: agan_cond_disc_loss) against their float64 references.

Bound, per element: |got - want| <= (n + 1) * 2^-24 * sum|terms|, n the number of fp32 additions the element takes -- the standard
bound of a recursive sum of n + 1 terms with unit roundoff 2^-24 -- with n and sum|terms| taken from the REFERENCE (the join is linear
with coefficients 0 / 1, so the reference applied to ones counts the terms and applied to absolute values sums them): at most 9 taps
forward, at most 16 (k + 1) terms for dp, at most 1 addition for dyi.  Derived, not tuned.

Measured on MI355X (every test prints its figures): the figures stand in the tests' docstrings."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

HF = importlib.import_module("attention-gan_amd.backend.functional")

DEV = torch.device("cuda", 0)
U = 2.0 ** -24
SHAPES = [(C, B, k, wrong) for C in (8, 24, 64) for B in (2, 3, 5) for k in (1, 2) for wrong in (False, True)]
SHAPES.append((512, 24, 2, True))


def _operands(C, B, k, wrong, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * C + 10 * B + k)
    yi = torch.randn(k * B, C, 4, 4, generator=g)
    p = torch.randn(B, C, 9, generator=g)
    dy = torch.randn((k + wrong) * B, C, 4, 4, generator=g)
    return yi, p, dy


def _ref_grads(yi, p, dy, wrong):
    """the reference's (y, dyi, dp) in float64 on the CPU"""
    a, b = yi.double().requires_grad_(True), p.double().requires_grad_(True)
    y = HF.cond_join_reference(a, b, wrong)
    dyi, dp = torch.autograd.grad(y, (a, b), dy.double())
    return y.detach(), dyi, dp


def _check(what, got, want, count, mag):
    """(count - 1) additions for an element summed from `count` terms of total magnitude mag"""
    bound = count * U * mag                                    # (n + 1) with n = count - 1
    err = (got.detach().double().cpu() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {what}: max |err| {float(err.max()):.2e}, worst err / bound {worst:.3f}, terms per element <= {int(count.max())}")
    assert bool((err <= bound).all()), what
    return worst


@pytest.mark.parametrize("C,B,k,wrong", SHAPES)
def test_kernels_against_float64(C, B, k, wrong):
    """Measured on MI355X over all 37 shapes, worst err / bound: forward 0.56 (max |err| 2.0e-6, at C = 512), dyi 0.50 with wrong rows
    (one correctly rounded addition: half an ulp of a bound of one ulp) and exactly 0 without, dp 0.29 (0.10 at C = 512, B = 24, k = 2,
    where 48 terms give max |err| 8.0e-6)."""
    yi, p, dy = _operands(C, B, k, wrong)
    want_y, want_dyi, want_dp = _ref_grads(yi, p, dy, wrong)
    ones_y, ones_dyi, ones_dp = _ref_grads(torch.zeros_like(yi), torch.ones_like(p), torch.ones_like(dy), wrong)
    abs_y, abs_dyi, abs_dp = _ref_grads(yi.abs(), p.abs(), dy.abs(), wrong)
    a, b = yi.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
    y = HF.cond_join(a, b, wrong)
    assert y.shape == want_y.shape and y.dtype == torch.float32
    dyi, dp = torch.autograd.grad(y, (a, b), dy.to(DEV))
    torch.cuda.synchronize()
    print(f"C {C} B {B} k {k} wrong {wrong}")
    assert int(ones_y.max()) <= 9 and int(ones_dp.max()) <= 16 * (k + 1) and int(ones_dyi.max()) <= 2
    _check("y", y, want_y, ones_y + 1, abs_y)                  # yi + the valid taps
    _check("dyi", dyi, want_dyi, ones_dyi, abs_dyi)
    _check("dp", dp, want_dp, ones_dp, abs_dp)
    # the fp32 reference on the device is the same statement in the same order: equal bits forward
    assert torch.equal(y, HF.cond_join_reference(a.detach(), b.detach(), wrong))


def test_two_runs_give_equal_bits():
    for C, B, k, wrong in ((24, 5, 2, True), (512, 24, 2, True)):
        yi, p, dy = (t.to(DEV) for t in _operands(C, B, k, wrong, seed=3))
        runs = []
        for _ in range(2):
            a, b = yi.clone().requires_grad_(True), p.clone().requires_grad_(True)
            y = HF.cond_join(a, b, wrong)
            runs.append((y.detach(),) + torch.autograd.grad(y, (a, b), dy))
        for first, second in zip(*runs):
            assert torch.equal(first, second)


@pytest.mark.parametrize("wrong", [False, True])
def test_only_the_gradients_asked_for(wrong, monkeypatch):
    """the generator update: only the image term asks.  Without wrong rows its gradient IS dy (no launch); with them it is dy's first
    k * B rows plus the wrong rows on the first group -- one fp32 addition, which torch's add reproduces bit for bit -- and the
    launch is handed no dp."""
    C, B, k = 24, 3, 2
    yi, p, dy = (t.to(DEV) for t in _operands(C, B, k, wrong, seed=5))
    a = yi.clone().requires_grad_(True)
    y = HF.cond_join(a, p, wrong)
    launches, call = [], HF.L.call

    def spy(name, *args):
        launches.append((name, args))
        return call(name, *args)
    monkeypatch.setattr(HF.L, "call", spy)
    (dyi,) = torch.autograd.grad(y, (a,), dy)
    monkeypatch.undo()
    if wrong:
        assert [n for n, _ in launches] == ["agan_cond_join_bwd"] and launches[0][1][1] is not None and launches[0][1][2] is None
    else:
        assert launches == []
    want = dy[:k * B].clone()
    if wrong:
        want[:B] += dy[k * B:]
    assert torch.equal(dyi, want)
    # and only the sentence term asking gives dp alone, equal to the two-sided call's
    b = p.clone().requires_grad_(True)
    (dp,) = torch.autograd.grad(HF.cond_join(yi, b, wrong), (b,), dy)
    a2, b2 = yi.clone().requires_grad_(True), p.clone().requires_grad_(True)
    _, dp2 = torch.autograd.grad(HF.cond_join(a2, b2, wrong), (a2, b2), dy)
    assert torch.equal(dp, dp2)


def test_sixteen_bit_operands_are_widened():
    C, B, k = 8, 2, 2
    yi, p, dy = _operands(C, B, k, True, seed=7)
    a = yi.to(DEV).bfloat16().requires_grad_(True)
    y = HF.cond_join(a, p.to(DEV), True)
    assert y.dtype == torch.float32
    assert torch.equal(y, HF.cond_join(a.detach().float(), p.to(DEV), True))
    (dyi,) = torch.autograd.grad(y, (a,), dy.to(DEV))
    assert dyi.dtype == torch.bfloat16 and dyi.shape == a.shape
    for bad in (yi.to(DEV).double(), yi.to(DEV).long()):
        with pytest.raises(ValueError):
            HF.cond_join(bad, p.to(DEV), True)
    with pytest.raises(ValueError):
        HF.cond_join(yi.to(DEV), p, True)                       # devices differ


@pytest.mark.parametrize("B", [1, 4, 300])
def test_loss_kernel_against_float64(B):
    """Bounds: the loss within 1e-5 of sum|terms| / (2B or 3B) -- logf is good to a few ulp, the guard's addition rounds the argument
    once (relative 2^-24, i.e. absolute 2^-24 in the log) and the block sum adds at most ceil(B / 256) + 8 roundings, together well under
    100 * 2^-24 = 6e-6 of the terms' magnitude; each gradient element within 4 * 2^-23 relative (the guard's addition, the weight's
    rounding and one division).  Measured on MI355X: loss error <= 1.6e-7 relative, gradients <= 1.4e-7 relative."""
    g = torch.Generator().manual_seed(B)
    pu = (torch.rand(2 * B, generator=g) * 0.9 + 0.05)
    pc = (torch.rand(3 * B, generator=g) * 0.9 + 0.05)
    a, b = pu.double().requires_grad_(True), pc.double().requires_grad_(True)
    want = HF.cond_disc_loss_reference(a, b)
    wu, wc = torch.autograd.grad(want, (a, b))
    x, z = pu.to(DEV).requires_grad_(True), pc.to(DEV).requires_grad_(True)
    got = HF.cond_disc_loss(x, z)
    gu, gc = torch.autograd.grad(got, (x, z))
    torch.cuda.synchronize()
    got, want = got.detach(), want.detach()
    err = abs(float(got) - float(want)) / float(want)           # every term is positive: the loss IS sum|terms| weighted
    gerr = max(float(((gu.double().cpu() - wu) / wu).abs().max()), float(((gc.double().cpu() - wc) / wc).abs().max()))
    print(f"B {B}: loss {float(got):.6f} vs {float(want):.6f} (rel {err:.2e}), gradients rel {gerr:.2e}")
    assert err <= 1e-5 and gerr <= 4 * 2.0 ** -23
    # the fp32 reference on the device agrees too, and two launches give equal bits
    assert abs(float(HF.cond_disc_loss_reference(x.detach(), z.detach())) - float(got)) <= 1e-5 * float(got)
    assert torch.equal(got.detach(), HF.cond_disc_loss(x.detach(), z.detach()))
