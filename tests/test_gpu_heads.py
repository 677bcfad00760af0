"""Bare activations, standalone GLU, the GAN / KL loss heads, the CA-net reparametrisation and fused Adam, through the C ABI, against
float64 with stated ulp bounds.

ulp bounds (u = 2^-24, the unit roundoff of fp32): an fp32 expression of k roundings whose terms do not cancel is within k u of its
value relative to the result; a library function (expf, logf, tanhf) adds about 2 u; GLU's sigmoid uses the fast exp (v_exp_f32 of
v log2 e), off by up to |v| u relative for an argument v.  Where a result underflows to 0 in fp32 (sigmoid(-100)), FLT_MIN is the floor.
The sizes cross the kernels' seams: the n & 3 tail lane of the 4-wide element-wise kernels, the single 256-thread block of the heads.
"""
import ctypes
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
GUARD = 64
SENT = 0x7FC0DEAD


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(t):
    """fp32 device copy followed by GUARD NaN-pattern sentinels; returns (view, whole)"""
    t = t.reshape(-1)
    whole = torch.empty(t.numel() + GUARD, dtype=torch.float32, device=DEV)
    whole.view(torch.int32).fill_(SENT)
    whole[:t.numel()].copy_(t.float())
    return whole[:t.numel()], whole


def _empty(n):
    whole = torch.empty(n + GUARD, dtype=torch.float32, device=DEV)
    whole.view(torch.int32).fill_(SENT)
    return whole[:n], whole


def tail_ok(whole, n):
    return bool((whole[n:].view(torch.int32) == SENT).all())


def check(what, got, ref, bound):
    got = got.double().cpu().reshape(-1)
    err = (got - ref.reshape(-1)).abs()
    bad = ~(err <= bound.reshape(-1))
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} outside the bound; first at {i}: got {float(got[i])!r}, "
                             f"want {float(ref.reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i]):.3e}")


def inputs(n, seed, scale=3.0):
    """random values with the edges planted: +-0, exact zeros, saturating magnitudes"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g, dtype=torch.float64) * scale
    edges = torch.tensor([0.0, -0.0, 20.0, -20.0, 100.0, -100.0, 1e-30, -1e-30, 0.0])
    k = min(n, len(edges))
    pos = torch.randperm(n, generator=g)[:k]
    x[pos] = edges[:k].double()
    return x.float().double()


# ------------------------------------------------------------------------------------------------------------ bare activations
SIZES = [1, 2, 3, 4, 5, 257, 2 ** 20 + 3]
ACTS = {L.ACT_LRELU: "lrelu", L.ACT_TANH: "tanh", L.ACT_SIGMOID: "sigmoid"}


def act64(x, act):
    if act == L.ACT_LRELU:
        return torch.where(x > 0, x, x * 0.2)
    if act == L.ACT_TANH:
        return torch.tanh(x)
    return torch.sigmoid(x)


def dact64(y, d, act):
    if act == L.ACT_LRELU:
        return torch.where(y > 0, d, d * 0.2)
    if act == L.ACT_TANH:
        return d * (1 - y * y)
    return d * y * (1 - y)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("act", list(ACTS), ids=list(ACTS.values()))
def test_act_fwd_bwd_vs_float64(act, n):
    """agan_act_fwd: <= 2 u (LeakyReLU: 0.2f is 0.25 u from 0.2, then one rounding, <= 1 u of |y|) / 4 u (tanhf; 1/(1+expf)) of |y|;
    agan_act_bwd from the kernel's own y: LeakyReLU's 0.2f d within 2 u, tanh's d (1 - y^2) within 4 u |dx| + 2 u |d| (1 - y^2 cancels near |y| = 1: y^2 rounds by u),
    sigmoid's d y (1 - y) within 4 u |dx| + 2 u |d y|"""
    x = inputs(n, n + act)
    d = inputs(n, 7 * n + act, 1.0)
    xd, _ = dev(x)
    yd, yw = _empty(n)
    L.call("agan_act_fwd", _p(xd), _p(yd), n, act, HF._stream())
    dd, _ = dev(d)
    dxd, dxw = _empty(n)
    L.call("agan_act_bwd", _p(yd), _p(dd), _p(dxd), n, act, HF._stream())
    torch.cuda.synchronize()
    assert tail_ok(yw, n) and tail_ok(dxw, n), "guard tail overwritten"
    ref = act64(x, act)
    k = 2 if act == L.ACT_LRELU else 4
    check(f"{ACTS[act]} fwd", yd, ref, k * U * ref.abs() + FLT_MIN)
    y = yd.double().cpu()
    dref = dact64(y, d, act)
    if act == L.ACT_LRELU:
        bound = 2 * U * dref.abs()
    elif act == L.ACT_TANH:
        bound = 4 * U * dref.abs() + 2 * U * d.abs()
    else:
        bound = 4 * U * dref.abs() + 2 * U * (d * y).abs()
    check(f"{ACTS[act]} bwd", dxd, dref, bound + FLT_MIN)
    # the sign rule at exactly 0: slope 0.2 there (torch), slope 1 only for y > 0
    if act == L.ACT_LRELU:
        z = (y == 0)
        assert torch.equal(dxd.double().cpu()[z], (d.float() * torch.tensor(0.2, dtype=torch.float32)).double()[z])


@pytest.mark.parametrize("B,C,HW", [(1, 2, 1), (3, 2, 1), (24, 200, 1), (2, 6, 5), (3, 8, 257), (2, 64, 4099)])
def test_glu_fwd_bwd_vs_float64(B, C, HW):
    """standalone GLU over the channel halves (HW = 1: the CA-net's [B, 2c] GLU).  fwd: a sg within 2 (|g| + 4) u |y| (the fast exp,
    the add, the division, the product); bwd: d sg within 2 (|g| + 5) u, and d a sg (1 - sg) within 2 ((|g| + 6) u |dx| + 1.5 u |d a|)
    -- 1 - sg keeps the absolute error of sg, where sg is near 1: 1 + e rounds by up to u (ulp 2^-23 on [1, 2)), the reciprocal by u/2"""
    n = B * C * HW
    x = inputs(n, n).view(B, C, HW)
    d = inputs(n // 2, n + 1, 1.0).view(B, C // 2, HW)
    xd, _ = dev(x)
    yd, yw = _empty(n // 2)
    L.call("agan_glu_fwd", _p(xd), _p(yd), B, C, HW, HF._stream())
    dd, _ = dev(d)
    dxd, dxw = _empty(n)
    L.call("agan_glu_bwd", _p(xd), _p(dd), _p(dxd), B, C, HW, HF._stream())
    torch.cuda.synchronize()
    assert tail_ok(yw, n // 2) and tail_ok(dxw, n), "guard tail overwritten"
    a, gt = x[:, :C // 2], x[:, C // 2:]
    sg = torch.sigmoid(gt)
    check("glu fwd", yd, a * sg, 2 * (gt.abs() + 4) * U * (a * sg).abs() + FLT_MIN)
    da, dg = d * sg, d * a * sg * (1 - sg)
    got = dxd.double().cpu().view(B, C, HW)
    check("glu bwd value half", got[:, :C // 2], da, 2 * (gt.abs() + 5) * U * da.abs() + FLT_MIN)
    check("glu bwd gate half", got[:, C // 2:], dg, 2 * ((gt.abs() + 6) * U * dg.abs() + 1.5 * U * (d * a).abs()) + FLT_MIN)


# ----------------------------------------------------------------------------------------------------------------- loss heads
def probs(n, seed):
    """probabilities in [0, 1] with exact 0 and 1 planted (the +1e-8 terms keep their logs finite)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, generator=g, dtype=torch.float64)
    p[torch.randperm(n, generator=g)[:min(n, 4)]] = torch.tensor([0.0, 1.0, 0.0, 1.0])[:min(n, 4)].double()
    return p.float().double()


def loss_bound(terms, n):
    """a mean of n fp32 terms over one 256-thread block (<= ceil(n/256) serial adds per thread, then an 8-level tree): each term's own
    k roundings plus (ceil(n/256) + 8) u of the running |sum|"""
    return (math.ceil(n / 256) + 8 + 4) * U * float(terms.abs().sum()) / n


@pytest.mark.parametrize("B", [1, 5, 256, 257, 1000])
def test_disc_and_gen_loss_vs_float64(B):
    """-mean(log(pr + 1e-8) + log(1 - pf + 1e-8)) and -mean(log(pf + 1e-8)) with their gradients, at probabilities 0 and 1 included.
    The float64 reference adds 1e-8 in float64; the kernel's fp32 1 + 1e-8f rounds to 1, a difference of 1e-8 absolute in that log."""
    pr, pf = probs(B, B), probs(B, B + 1)
    prd, _ = dev(pr)
    pfd, _ = dev(pf)
    loss = torch.full((1,), float("nan"), device=DEV)
    dpr, dprw = _empty(B)
    dpf, dpfw = _empty(B)
    L.call("agan_disc_loss", _p(prd), _p(pfd), _p(loss), _p(dpr), _p(dpf), B, HF._stream())
    gl = torch.full((1,), float("nan"), device=DEV)
    gpf, gpfw = _empty(B)
    L.call("agan_gen_loss", _p(pfd), _p(gl), _p(gpf), B, HF._stream())
    torch.cuda.synchronize()
    assert tail_ok(dprw, B) and tail_ok(dpfw, B) and tail_ok(gpfw, B)
    a, b = pr + 1e-8, 1 - pf + 1e-8
    terms = torch.log(a) + torch.log(b)
    check("disc loss", loss, -terms.mean().view(1), torch.tensor([loss_bound(terms, B) + 1e-8]))
    check("d p_real", dpr, -1 / (B * a), 4 * U / (B * a))
    check("d p_fake", dpf, 1 / (B * b), 4 * U / (B * b))
    t = torch.log(pf + 1e-8)
    check("gen loss", gl, -t.mean().view(1), torch.tensor([loss_bound(t, B) + 1e-8]))
    check("gen d p_fake", gpf, -1 / (B * (pf + 1e-8)), 4 * U / (B * (pf + 1e-8)))


@pytest.mark.parametrize("n", [1, 100, 257, 1000])
def test_kl_loss_and_reparam_vs_float64(n):
    """-0.5 mean(1 + lv - mu^2 - exp(lv)) with dmu = mu / n, dlv = -0.5 (1 - exp(lv)) / n; c = eps exp(lv / 2) + mu and its backward"""
    g = torch.Generator().manual_seed(n)
    mu = (torch.randn(n, generator=g, dtype=torch.float64) * 2).float().double()
    lv = (torch.randn(n, generator=g, dtype=torch.float64) * 3).float().double()
    lv[0] = 0.0                                           # exp(lv) = 1: dlv = 0 exactly
    eps = torch.randn(n, generator=g, dtype=torch.float64).float().double()
    dc = torch.randn(n, generator=g, dtype=torch.float64).float().double()
    mud, _ = dev(mu)
    lvd, _ = dev(lv)
    epd, _ = dev(eps)
    dcd, _ = dev(dc)
    loss = torch.full((1,), float("nan"), device=DEV)
    dmu, dmuw = _empty(n)
    dlv, dlvw = _empty(n)
    L.call("agan_kl_loss", _p(mud), _p(lvd), _p(loss), _p(dmu), _p(dlv), n, HF._stream())
    c, cw = _empty(n)
    L.call("agan_reparam_fwd", _p(mud), _p(lvd), _p(epd), _p(c), n, HF._stream())
    rmu, rmuw = _empty(n)
    rlv, rlvw = _empty(n)
    L.call("agan_reparam_bwd", _p(lvd), _p(epd), _p(dcd), _p(rmu), _p(rlv), n, HF._stream())
    torch.cuda.synchronize()
    assert all(tail_ok(w, n) for w in (dmuw, dlvw, cw, rmuw, rlvw))
    e = torch.exp(lv)
    terms = 1 + lv - mu * mu - e
    check("kl loss", loss, (-0.5 * terms.mean()).view(1), torch.tensor([loss_bound(torch.stack([1 + 0 * lv, lv, mu * mu, e]), n)]))
    check("kl d mu", dmu, mu / n, 2 * U * (mu / n).abs())
    check("kl d logvar", dlv, -0.5 * (1 - e) / n, (4 * U * (1 - e).abs() + 2 * U * e) * 0.5 / n + FLT_MIN)
    h = torch.exp(0.5 * lv)
    check("reparam c", c, eps * h + mu, 4 * U * ((eps * h).abs() + mu.abs()))
    assert torch.equal(rmu.double().cpu(), dc), "reparam d mu must be dc itself"
    check("reparam d logvar", rlv, dc * eps * 0.5 * h, 5 * U * (dc * eps * h * 0.5).abs() + FLT_MIN)


# ----------------------------------------------------------------------------------------------------------------------- Adam
def adam64(p, m, v, g, t, lr, b1, b2, eps):
    m.mul_(b1).add_((1 - b1) * g)
    v.mul_(b2).add_((1 - b2) * g * g)
    p.sub_(lr / (1 - b1 ** t) * m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 10007])
@pytest.mark.parametrize("gscale", [1.0, 0.5, 1.0 / 3.0])
def test_adam_many_steps_vs_float64(n, gscale):
    """300 steps of agan_adam_step (grad_scale: the data-parallel 1/world) against torch.optim.Adam's update in float64, per tensor:
    max|HIP - f64| <= 2 max|torch.optim.Adam fp32 - f64| + 4 u max|f64| (the fp32 optimiser's own rounding drift is the yardstick;
    the floor covers the one rounding of the stored state)"""
    steps, lr, b1, b2, eps = 300, 2e-4, 0.5, 0.999, 1e-8
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.1 if s % 7 else 0.0) * (1 + s % 5) for s in range(steps)]     # every 7th step zero
    pd, md, vd = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    for s, gr in enumerate(grads):
        gd = gr.to(DEV)
        L.call("agan_adam_step", _p(pd), _p(gd), _p(md), _p(vd), n, _p(state), lr, b1, b2, eps, gscale, HF._stream())
        adam64(p64, m64, v64, gr.double() * gscale, s + 1, lr, b1, b2, eps)
        pt.grad = gr * torch.tensor(gscale, dtype=torch.float32)
        opt.step()
    torch.cuda.synchronize()
    assert int(state[0].cpu()) == steps
    st = opt.state[pt]
    for what, got, want, t32 in (("param", pd, p64, pt.detach()), ("exp_avg", md, m64, st["exp_avg"]), ("exp_avg_sq", vd, v64, st["exp_avg_sq"])):
        e_h = float((got.double().cpu() - want).abs().max())
        e_t = float((t32.double() - want).abs().max())
        bound = 2 * e_t + 4 * U * float(want.abs().max())
        assert e_h <= bound, f"{what}: max err {e_h:.3e} > {bound:.3e} (torch fp32 {e_t:.3e})"


@pytest.mark.parametrize("poke", [0, 1, 2, 999, 1000, 2 ** 20, 2 ** 31 - 2])
def test_adam_bias_correction_coefficients(poke):
    """step_state[0] = poke, one step: the step becomes t = poke + 1 and coef = (lr / (1 - b1^t), 1 / sqrt(1 - b2^t)) rounded once to
    fp32 (within 1 ulp: beta^t by repeated squaring in fp64 is good to ~log2(t) fp64 ulps), and the update uses them"""
    lr, b1, b2, eps = 2e-4, 0.5, 0.999, 1e-8
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    state[0] = poke
    p, gr = torch.ones(5, device=DEV), torch.full((5,), 0.25, device=DEV)
    m, v = torch.zeros(5, device=DEV), torch.zeros(5, device=DEV)
    L.call("agan_adam_step", _p(p), _p(gr), _p(m), _p(v), 5, _p(state), lr, b1, b2, eps, 1.0, HF._stream())
    torch.cuda.synchronize()
    t = poke + 1
    assert int(state[0].cpu()) == t
    coef = state[2:4].cpu().view(torch.float32).double()
    want = torch.tensor([lr / (1 - b1 ** t), 1 / math.sqrt(1 - b2 ** t)], dtype=torch.float64)
    assert bool(((coef - want).abs() <= 2 * U * want).all()), (coef.tolist(), want.tolist())
    m1, v1 = (1 - b1) * 0.25, (1 - b2) * 0.0625
    p1 = 1 - float(coef[0]) * m1 / (math.sqrt(v1) * float(coef[1]) + eps)
    assert bool(((p.cpu().double() - p1).abs() <= 4 * U).all()), (p.tolist(), p1)
