"""Train-mode BatchNorm + activation (csrc/bn_act.hip) on every kernel path, through the C ABI, against float64.

Two kinds of case:

  * bit-exact (EXACT): eps = 0, momentum 0.5 or 0.25, and per (group, channel) a batch built so that every BatchNorm quantity is
    exact in fp32 -- values (mean + {-2, 0, 2} * 2^e with 1/8 of them at each sign, or mean +- 2^e), so the mean is on the grid, the
    variance is 4^e and invstd is 2^-e; n = B/groups * HW a power of two, so the backward's sums / n are exact; gamma, beta and dout on
    the 5 * 2^k grid, so LeakyReLU's 0.2f * z and 0.2f * d are exact too.  Output, dx, dgamma, dbeta, mean and invstd must then equal
    the float64 result (rounded once to the storage type of a 16-bit tensor) bit for bit, up to the sign of a zero; the running
    statistics must equal the float64 update rounded once to fp32 after each group, in group order.  Channel 0 has beta = 0 and 3/4 of
    its values at the mean: z is exactly 0 there, LeakyReLU's kink, where torch's derivative is the slope (0.2), not 1.
  * float64-referenced (RANDOM): random data, eps = 1e-5, every activation including GLU, and the shapes where a kernel changes form
    (odd HW, HW = 4 mod 8, HW = 1, B/groups * HW on both sides of 512, 2048 and 8192).  The channels differ on purpose: one ordinary,
    one whose mean is 10^3 x its spread, one near-constant, one at 1e-3 scale (with a 1e-3-scale dout on the last output channel).
    Each quantity is compared PER CHANNEL, relative to that channel's own scale: err(HIP) <= 2 err(torch fp32 CPU) + FLOOR (+ one
    rounding of a 16-bit stored result).  torch's fp32 CPU BatchNorm is a careful fp32 implementation of the same formulas; the
    kernels do the same fp32 work per element (a handful of roundings, plus the fast exp of GLU's sigmoid: a few ulp of the channel's
    scale, FLOOR = 16 ulp) with their sums in fp64.

A launch log (agan_bn_last_launch) records every kernel instantiation a call ran; `test_the_cases_reach_every_bn_kernel_form`
requires the case tables to reach every form the dispatch rules can pick.  Guard tails after out, dx, dgamma, dbeta, the statistics
and both workspaces must come back untouched.
"""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")

F32, BF16, F16 = L.DT_F32, L.DT_BF16, L.DT_F16
TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
ULP16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
PAIRS = [(F32, F32), (BF16, BF16), (F32, BF16), (F16, F16), (F32, F16)]      # (x / dx, out / dout / residual): bn_dt_ok
ACTS = [L.ACT_NONE, L.ACT_GLU, L.ACT_LRELU]
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
FLOOR = 16 * 2.0 ** -24
# GLU: the sigmoid's fast exp (v_exp_f32 of v * log2 e) is off by up to |v| 2^-24 relative for a gate pre-activation v (|v| < 8 here), and
# the gate half's derivative sg (1 - sg) turns that into up to 4x as much of its own scale where sg is near 0 or 1: 64 ulp
FLOOR_GLU = 64 * 2.0 ** -24
AGAN_EWORKSPACE = -2

# launch-log kinds (include/agan.h: agan_bn_last_launch)
K_STATS, K_STATS_FINAL, K_ROWS, K_FWD_APPLY, K_SMALL_FWD, K_SMALL_BWD, K_BWD_PART, K_BWD_FINAL, K_BWD_APPLY = range(1, 10)
K_ACT_FWD, K_ACT_BWD, K_GLU_FWD, K_GLU_BWD = range(10, 14)

GUARD = 64                                     # elements of sentinel after every device output
WS_GUARD = 256                                 # bytes of sentinel after every workspace
SENTINEL = {4: 0x7FC0DEAD, 2: 0x7E5A, 8: 0x5A5A5A5A5A5A5A5A}
INT_OF = {4: torch.int32, 2: torch.int16, 8: torch.int64}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.view(INT_OF[t.element_size()])


def alloc(n, dtype, init=None):
    """device buffer: n elements (initialised from `init`, else sentinel) followed by GUARD sentinel elements"""
    whole = torch.empty(n + GUARD, dtype=dtype, device=DEV)
    _bits(whole).fill_(SENTINEL[whole.element_size()])
    if init is not None:
        whole[:n].copy_(init.reshape(-1).to(dtype))
    return whole


def guard_ok(whole, n):
    tail = _bits(whole[n:])
    return bool((tail == SENTINEL[whole.element_size()]).all())


def alloc_ws(nbytes):
    ws = torch.full((nbytes + WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return ws


def ws_ok(ws, nbytes):
    return bool((ws[nbytes:] == 0xA5).all())


def last_launch():
    buf = (ctypes.c_int * 64)()
    n = L.load().agan_bn_last_launch(ctypes.cast(buf, ctypes.c_void_p), 64)
    assert 0 <= n <= 64, n
    return [(c // 100000, c // 10000 % 10, c // 1000 % 10, c // 100 % 10, c % 100) for c in buf[:n]]


def q(t, dt):
    """the values a tensor of storage type dt holds (float64)"""
    return t.to(TDT[dt]).double()


# ------------------------------------------------------------------------------------------------------------------ device side
def bn_device(x, gamma, beta, res, dout, act, groups, xdt, odt, eps, mom, rm0, rv0, dg0, db0, accumulate, amax=False):
    """agan_bn_train_fwd_dt + agan_bn_act_bwd_dt on the device.  x [B, C, HW], dout / res [B, Co, HW] (float64, values representable in
    their storage types).  Returns float64 CPU results, the two launch logs and the guard checks."""
    lib = L.load()
    B, C, HW = x.shape
    Co = C // 2 if act == L.ACT_GLU else C
    Bg = B // groups
    nx, no = B * C * HW, B * Co * HW
    xw = alloc(nx, TDT[xdt], x)
    rw = alloc(no, TDT[odt], res) if res is not None else None
    ow = alloc(no, TDT[odt])
    g, b = gamma.float().to(DEV), beta.float().to(DEV)
    mw, iw = alloc(groups * C, torch.float32), alloc(groups * C, torch.float32)
    rmw, rvw = alloc(C, torch.float32, rm0), alloc(C, torch.float32, rv0)
    nbt = alloc(1, torch.int64, torch.tensor([7]))
    fws_n = lib.agan_bn_train_fwd_ws_bytes(Bg, C, HW)
    fws = alloc_ws(fws_n)
    oam = torch.zeros(L.AMAX_SLOT, device=DEV) if amax else None
    st = HF._stream()
    rc = lib.agan_bn_train_fwd_dt(_p(xw), _p(g), _p(b), _p(rw), _p(ow), _p(mw), _p(iw), _p(rmw), _p(rvw), _p(nbt), B, C, HW, eps, mom, act,
                                  groups, _p(fws), fws_n, st, _p(oam), xdt, odt)
    assert rc == 0, (rc, lib.agan_last_error())
    log_f = last_launch()
    dw = alloc(no, TDT[odt], dout)
    dxw = alloc(nx, TDT[xdt])
    dgw, dbw = alloc(C, torch.float32, dg0), alloc(C, torch.float32, db0)
    bws_n = lib.agan_bn_act_bwd_ws_bytes(Bg, C, HW)
    bws = alloc_ws(bws_n)
    dam = torch.zeros(L.AMAX_SLOT, device=DEV) if amax else None
    rc = lib.agan_bn_act_bwd_dt(_p(xw), _p(dw), _p(mw), _p(iw), _p(g), _p(b), _p(dxw), _p(dgw), _p(dbw), B, C, HW, act, accumulate,
                                groups, _p(bws), bws_n, st, _p(dam), xdt, odt)
    assert rc == 0, (rc, lib.agan_last_error())
    log_b = last_launch()
    torch.cuda.synchronize()
    guards = {"out": guard_ok(ow, no), "dx": guard_ok(dxw, nx), "mean": guard_ok(mw, groups * C), "invstd": guard_ok(iw, groups * C),
              "running_mean": guard_ok(rmw, C), "running_var": guard_ok(rvw, C), "nbt": guard_ok(nbt, 1),
              "dgamma": guard_ok(dgw, C), "dbeta": guard_ok(dbw, C), "fwd ws": ws_ok(fws, fws_n), "bwd ws": ws_ok(bws, bws_n),
              "x": guard_ok(xw, nx), "dout": guard_ok(dw, no)}
    cpu = lambda w, n, shape: w[:n].double().cpu().view(*shape)
    r = {"out": cpu(ow, no, (B, Co, HW)), "dx": cpu(dxw, nx, (B, C, HW)), "mean": cpu(mw, groups * C, (groups, C)),
         "invstd": cpu(iw, groups * C, (groups, C)), "running_mean": cpu(rmw, C, (C,)), "running_var": cpu(rvw, C, (C,)),
         "nbt": int(nbt[0]), "dgamma": cpu(dgw, C, (C,)), "dbeta": cpu(dbw, C, (C,)), "log_fwd": log_f, "log_bwd": log_b,
         "guards": guards, "x_unchanged": torch.equal(xw[:nx].double().cpu(), x.reshape(-1))}
    if amax:
        r["out_amax"], r["dx_amax"] = float(oam.max()), float(dam.max())
    return r


# ------------------------------------------------------------------------------------------------------------------- references
def bn_torch(x, gamma, beta, res, dout, act, groups, eps, dtype):
    """train-mode BatchNorm (per group) + activation (+ residual) and its backward (autograd), on the CPU in `dtype`, written out as
    the definition reads: z = (x - mean) / sqrt(var + eps) * gamma + beta.  (F.batch_norm's CPU kernel folds the affine into
    x * alpha + (beta - mean * alpha), which loses a channel's own scale when its mean is far above its spread -- not a yardstick.)"""
    B, C, HW = x.shape
    Bg = B // groups
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    xs, g, b = leaf(x), leaf(gamma), leaf(beta)
    outs = []
    for gi in range(groups):
        xg = xs[gi * Bg:(gi + 1) * Bg]
        m = xg.mean(dim=(0, 2), keepdim=True)
        v = ((xg - m) ** 2).mean(dim=(0, 2), keepdim=True)
        z = (xg - m) * torch.rsqrt(v + eps) * g.view(1, -1, 1) + b.view(1, -1, 1)
        if act == L.ACT_GLU:
            z = F.glu(z, dim=1)
        elif act == L.ACT_LRELU:
            z = F.leaky_relu(z, 0.2)
        outs.append(z)
    y = torch.cat(outs)
    if res is not None:
        y = y + res.to(dtype)
    y.backward(dout.to(dtype))
    return {"out": y.detach().double(), "dx": xs.grad.double(), "dgamma": g.grad.double(), "dbeta": b.grad.double()}


def bn_stats64(x, groups, eps, mom, rm0, rv0):
    """float64 batch statistics per group; running statistics updated per group in batch order, rounded to fp32 after each update
    (what the library stores), with the formulas of the kernels (unbiased variance = var * n / (n - 1))"""
    B, C, HW = x.shape
    Bg = B // groups
    n = Bg * HW
    mom = float(torch.tensor(mom, dtype=torch.float32))
    means, invs, rm, rv = [], [], rm0.double().clone(), rv0.double().clone()
    for gi in range(groups):
        xg = x[gi * Bg:(gi + 1) * Bg].double()
        m = xg.mean(dim=(0, 2))
        var = ((xg - m.view(1, -1, 1)) ** 2).mean(dim=(0, 2))
        means.append(m)
        invs.append(1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32))))
        ub = var * (n / (n - 1)) if n > 1 else var
        rm = ((1.0 - mom) * rm + mom * m).float().double()
        rv = ((1.0 - mom) * rv + mom * ub).float().double()
    return torch.stack(means), torch.stack(invs), rm, rv


def eq(got, want):
    """equal as numbers (+0 == -0), every element"""
    return bool((got == want).all())


def first_diff(got, want):
    d = (got != want).reshape(-1).nonzero()
    if not len(d):
        return "none"
    i = int(d[0])
    return f"{int(len(d))} differ, first at flat {i}: got {float(got.reshape(-1)[i])!r} want {float(want.reshape(-1)[i])!r}"


# ------------------------------------------------------------------------------------------------------------ (a) bit-exact cases
def exact_inputs(B, C, HW, groups, res, seed):
    """x, gamma, beta, residual, dout on the grids described in the module docstring"""
    gen = torch.Generator().manual_seed(seed)
    Bg = B // groups
    n = Bg * HW
    assert n >= 8 and n & (n - 1) == 0, "n = B/groups * HW must be a power of two >= 8"
    x = torch.empty(B, C, HW, dtype=torch.float64)
    for gi in range(groups):
        for c in range(C):
            e = int(torch.randint(-1, 2, (1,), generator=gen))
            if c == 0 or (gi + c) % 2:            # 1/8 at +2, 1/8 at -2, 3/4 at the mean: var 4^e
                v = torch.zeros(n, dtype=torch.float64)
                v[:n // 8], v[n // 8:n // 4] = 2.0, -2.0
            else:                                  # half at +1, half at -1: var 4^e
                v = torch.ones(n, dtype=torch.float64)
                v[n // 2:] = -1.0
            v = v[torch.randperm(n, generator=gen)]
            mean = 0.0 if c == 0 else float(torch.randint(-3, 4, (1,), generator=gen))
            x[gi * Bg:(gi + 1) * Bg, c, :] = ((mean + v) * 2.0 ** e).view(Bg, HW)
    # gamma = +-5/4 or +-5/8, beta on the 5/4 grid, channel 0's beta = 0 (z exactly 0 at its mean)
    gamma = torch.tensor([(-1.0) ** int(torch.randint(0, 2, (1,), generator=gen)) * 5.0 * 2.0 ** -int(torch.randint(2, 4, (1,), generator=gen))
                          for _ in range(C)], dtype=torch.float64)
    beta = torch.randint(-2, 3, (C,), generator=gen).double() * 1.25
    beta[0] = 0.0
    dout = torch.randint(-1, 2, (B, C, HW), generator=gen).double() * 1.25
    r = torch.randint(-4, 5, (B, C, HW), generator=gen).double() * 0.5 if res else None
    return x, gamma, beta, r, dout


def exact_reference(x, gamma, beta, res, dout, act, groups, mom, rm0, rv0, dg0, db0, accumulate):
    ref = bn_torch(x, gamma, beta, res, dout, act, groups, 0.0, torch.float64)
    mean, invstd, rm, rv = bn_stats64(x, groups, 0.0, mom, rm0, rv0)
    ref.update(mean=mean, invstd=invstd, running_mean=rm, running_var=rv)
    if accumulate:
        ref["dgamma"] = ref["dgamma"] + dg0
        ref["dbeta"] = ref["dbeta"] + db0
    # the construction's promise: every quantity the kernels form is exact in fp32 (else the case table is wrong, not the kernel)
    B, C, HW = x.shape
    Bg = B // groups
    for k in ("out", "dx", "dgamma", "dbeta", "mean", "invstd"):
        assert eq(ref[k].float().double(), ref[k]), f"case construction: {k} is not exact in fp32"
    xh = torch.cat([(x[gi * Bg:(gi + 1) * Bg] - mean[gi].view(1, -1, 1)) * invstd[gi].view(1, -1, 1) for gi in range(groups)])
    for gi in range(groups):
        sl = slice(gi * Bg, (gi + 1) * Bg)
        z = xh[sl] * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
        dz = torch.where(z > 0, dout[sl], dout[sl] * 0.2) if act == L.ACT_LRELU else dout[sl]
        c0, c1 = dz.mean(dim=(0, 2), keepdim=True), (dz * xh[sl]).mean(dim=(0, 2), keepdim=True)
        inner = dz - c0 - xh[sl] * c1
        for name, t in (("z", z), ("dz", dz), ("c0", c0), ("c1", c1), ("dz - c0 - xhat c1", inner)):
            assert eq(t.float().double(), t), f"case construction: {name} is not exact in fp32"
    return ref


# (Bg, HW): the path each takes
EXACT_SHAPES = [
    (4, 64),        # n 256: one-launch small kernels, PER 2
    (16, 64),       # n 1024: PER 8
    (16, 256),      # n 4096: PER 32
    (2, 8192),      # n 16384: three-pass kernels, apply width 8 with a 16-bit tensor (4 in fp32)
    (4096, 4),      # n 16384, HW = 4 mod 8: width 4 with 16-bit tensors too
    (32, 1),        # BatchNorm1d rows kernel, scalar sweeps (fp32 x only)
]
EXACT_ACTS = [("none", L.ACT_NONE, False), ("res", L.ACT_NONE, True), ("lrelu", L.ACT_LRELU, False)]


def exact_cases():
    out, i = [], 0
    for Bg, HW in EXACT_SHAPES:
        for an, act, res in EXACT_ACTS:
            for xdt, odt in PAIRS:
                if HW == 1 and xdt != F32:
                    continue
                groups = 1 + i % 3
                accumulate = (i // 3) % 2
                mom = 0.5 if i % 2 else 0.25
                out.append(pytest.param(Bg, HW, act, res, xdt, odt, groups, accumulate, mom, i,
                                        id=f"{Bg}x{HW}-{an}-{DT_NAME[xdt]}.{DT_NAME[odt]}-g{groups}-acc{accumulate}"))
                i += 1
    return out


EXACT_CASES = exact_cases()


def run_exact(Bg, HW, act, res, xdt, odt, groups, accumulate, mom, seed, C=3):
    B = Bg * groups
    x, gamma, beta, r, dout = exact_inputs(B, C, HW, groups, res, seed)
    x, dout = q(x, xdt), q(dout, odt)
    r = q(r, odt) if r is not None else None
    rm0 = torch.tensor([0.75, -1.5, 3.0])[:C].double()
    rv0 = torch.tensor([1.5, 0.25, 2.0])[:C].double()
    dg0 = torch.tensor([0.375, -2.5, 1.0])[:C].double()         # sentinels already in the gradient buffers (accumulate = 1 adds)
    db0 = torch.tensor([-0.75, 1.25, 4.0])[:C].double()
    got = bn_device(x, gamma, beta, r, dout, act, groups, xdt, odt, 0.0, mom, rm0, rv0, dg0, db0, accumulate, amax=True)
    return got, (x, gamma, beta, r, dout, act, groups, mom, rm0, rv0, dg0, db0, accumulate)


@pytest.mark.parametrize("Bg,HW,act,res,xdt,odt,groups,accumulate,mom,seed", EXACT_CASES)
def test_bn_bit_exact(Bg, HW, act, res, xdt, odt, groups, accumulate, mom, seed):
    got, args = run_exact(Bg, HW, act, res, xdt, odt, groups, accumulate, mom, seed)
    ref = exact_reference(*args)
    bad = [k for k, v in got["guards"].items() if not v]
    assert not bad, f"guard tail overwritten: {bad}"
    assert got["x_unchanged"], "x was modified"
    checks = {"out": ref["out"].to(TDT[odt]).double(), "dx": ref["dx"].to(TDT[xdt]).double(), "dgamma": ref["dgamma"],
              "dbeta": ref["dbeta"], "mean": ref["mean"], "invstd": ref["invstd"], "running_mean": ref["running_mean"],
              "running_var": ref["running_var"]}
    wrong = [f"{k}: {first_diff(got[k], v)}" for k, v in checks.items() if not eq(got[k], v)]
    assert not wrong, "not bit-exact:\n  " + "\n  ".join(wrong)
    assert got["nbt"] == 7 + groups, f"num_batches_tracked {got['nbt']} != 7 + {groups}"
    # amax slots: max |value| the kernels computed, folded over the groups (a 16-bit store rounds once after the max is taken)
    for k, am, dt in (("out", got["out_amax"], odt), ("dx", got["dx_amax"], xdt)):
        stored = float(got[k].abs().max())
        tol = ULP16[dt] * stored if dt != F32 else 0.0
        assert abs(am - stored) <= tol, f"{k} amax {am!r} vs max|{k}| {stored!r}"


def test_lrelu_kink_takes_the_slope():
    """BN + LeakyReLU where z is exactly 0 (beta = 0, x == mean): the gradient there is 0.2 * dout, as torch's leaky_relu_backward
    gives.  8 equal values: torch's dbeta is 1.6 for dout = 1, a slope of 1 at the kink would give 8."""
    x = torch.full((8, 2, 1), 3.0, dtype=torch.float64)
    x[:, 1, 0] = torch.tensor([1.0, -1.0] * 4)
    gamma, beta = torch.tensor([1.0, 1.0], dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    dout = torch.ones(8, 2, 1, dtype=torch.float64)
    z2 = torch.zeros(2, dtype=torch.float64)
    got = bn_device(x, gamma, beta, None, dout, L.ACT_LRELU, 1, F32, F32, 1e-5, 0.5, z2, z2 + 1, z2, z2, 0)
    ref = bn_torch(x, gamma, beta, None, dout, L.ACT_LRELU, 1, 1e-5, torch.float64)
    assert float(ref["dbeta"][0]) == pytest.approx(1.6)
    assert eq(got["dbeta"], ref["dbeta"].float().double()), (got["dbeta"], ref["dbeta"])
    # the bare activation takes the same rule at exactly 0 (y = 0 there)
    y = torch.tensor([0.0, -0.0, 1.0, -1.0], device=DEV)
    d = torch.tensor([1.0, 1.0, 1.0, 1.0], device=DEV)
    dx = torch.empty(4, device=DEV)
    L.call("agan_act_bwd", _p(y), _p(d), _p(dx), 4, L.ACT_LRELU, HF._stream())
    assert dx.cpu().tolist() == pytest.approx([0.2, 0.2, 1.0, 0.2])


# ------------------------------------------------------------------------------------------------- (b) float64-referenced cases
# (B, C, HW, groups, note)
RANDOM_SHAPES = [
    (4, 4, 49, 1, "odd HW, n 196: small PER 2, scalar"),
    (40, 4, 12, 1, "HW = 4 mod 8, n 480: small PER 2"),
    (32, 4, 16, 2, "two groups of n 256"),
    (73, 4, 7, 1, "n 511: PER 2"),
    (32, 4, 16, 1, "n 512: PER 2, the last"),
    (19, 4, 27, 1, "n 513: PER 8, the first"),
    (89, 4, 23, 1, "n 2047: PER 8"),
    (32, 4, 64, 1, "n 2048: PER 8, the last"),
    (3, 4, 683, 1, "n 2049: PER 32, the first"),
    (1, 4, 8191, 1, "n 8191: PER 32, batch 1"),
    (2, 4, 4096, 1, "n 8192: PER 32, the last small"),
    (3, 4, 2731, 1, "n 8193: three-pass, the first; odd HW: width 1"),
    (700, 4, 12, 1, "n 8400, HW = 4 mod 8: width 4"),
    (160, 4, 64, 1, "n 10240: width 8 with a 16-bit tensor, 4 in fp32"),
    (8, 4, 3072, 2, "two groups of n 12288"),
    (5, 4, 4099, 1, "n 20495: statistics over several chunks, odd HW"),
    (1500, 4, 12, 1, "n 18000: several chunks, HW = 4 mod 8"),
    (24, 6, 1, 1, "BatchNorm1d at batch 24"),
    (64, 6, 1, 2, "BatchNorm1d, two groups of 32"),
]


def random_inputs(B, C, HW, act, res, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, HW, generator=gen, dtype=torch.float64)
    kinds = []
    for c in range(C):
        k = c % 4
        if k == 0:
            x[:, c] = x[:, c] * 1.5 + 0.3                    # ordinary
        elif k == 1:
            x[:, c] = x[:, c] * 0.5 + 500.0                  # mean 10^3 x std
        elif k == 2:
            x[:, c] = x[:, c] * 3e-4 + 0.7                   # near-constant (var << eps)
        else:
            x[:, c] = x[:, c] * 1e-3                         # 1e-3 scale
        kinds.append(("ordinary", "offset", "near-constant", "small")[k])
    gamma = torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=gen, dtype=torch.float64) * 0.1
    Co = C // 2 if act == L.ACT_GLU else C
    dout = torch.randn(B, Co, HW, generator=gen, dtype=torch.float64)
    dout[:, Co - 1] *= 1e-3
    r = torch.randn(B, Co, HW, generator=gen, dtype=torch.float64) if res else None
    return x, gamma, beta, r, dout, kinds


def random_cases():
    out = []
    for si, (B, C, HW, groups, note) in enumerate(RANDOM_SHAPES):
        for an, act, res in [("none", L.ACT_NONE, False), ("res", L.ACT_NONE, True), ("glu", L.ACT_GLU, False), ("lrelu", L.ACT_LRELU, False)]:
            if res and si % 3:
                continue                                   # the residual on every third shape
            for xdt, odt in PAIRS:
                if HW == 1 and xdt != F32:
                    continue
                out.append(pytest.param(B, C, HW, groups, act, res, xdt, odt, si,
                                        id=f"B{B}-C{C}-HW{HW}-g{groups}-{an}-{DT_NAME[xdt]}.{DT_NAME[odt]}"))
    return out


RANDOM_CASES = random_cases()


def run_random(B, C, HW, groups, act, res, xdt, odt, seed):
    x, gamma, beta, r, dout, kinds = random_inputs(B, C, HW, act, res, seed)
    x, dout = q(x, xdt), q(dout, odt)
    r = q(r, odt) if r is not None else None
    rm0, rv0 = torch.linspace(-1, 1, C, dtype=torch.float64), torch.linspace(0.5, 2, C, dtype=torch.float64)
    z = torch.zeros(C, dtype=torch.float64)
    got = bn_device(x, gamma, beta, r, dout, act, groups, xdt, odt, 1e-5, 0.1, rm0, rv0, z, z, 0, amax=False)
    return got, (x, gamma, beta, r, dout, kinds, rm0, rv0)


def channel_check(what, got, ref, t32, extra, kinds, floor=FLOOR):
    """per channel (axis 1): max|got - ref| / max|ref| <= 2 (same for torch fp32) + floor + extra"""
    scale = ref.abs().amax(dim=(0, 2)).clamp(min=1e-300)
    eh = (got - ref).abs().amax(dim=(0, 2)) / scale
    et = (t32 - ref).abs().amax(dim=(0, 2)) / scale
    bound = 2 * et + floor + extra
    bad = [f"{what}[{c}] ({kinds[c % len(kinds)]}): err {float(eh[c]):.3e} > bound {float(bound[c]):.3e} (torch fp32 {float(et[c]):.3e})"
           for c in range(len(eh)) if not float(eh[c]) <= float(bound[c])]
    return bad


def sum_check(what, got, ref, t32, terms, floor=FLOOR):
    """a per-channel sum: |got - ref| <= 2 |torch fp32 - ref| + floor * (sum of |terms|)"""
    bound = 2 * (t32 - ref).abs() + floor * terms
    return [f"{what}[{c}]: |err| {float((got - ref)[c].abs()):.3e} > bound {float(bound[c]):.3e}"
            for c in range(len(ref)) if not float((got - ref)[c].abs()) <= float(bound[c])]


@pytest.mark.parametrize("B,C,HW,groups,act,res,xdt,odt,seed", RANDOM_CASES)
def test_bn_vs_float64(B, C, HW, groups, act, res, xdt, odt, seed):
    got, (x, gamma, beta, r, dout, kinds, rm0, rv0) = run_random(B, C, HW, groups, act, res, xdt, odt, seed)
    bad = [k for k, v in got["guards"].items() if not v]
    assert not bad, f"guard tail overwritten: {bad}"
    r64 = bn_torch(x, gamma, beta, r, dout, act, groups, 1e-5, torch.float64)
    r32 = bn_torch(x, gamma, beta, r, dout, act, groups, 1e-5, torch.float32)
    Co = C // 2 if act == L.ACT_GLU else C
    okinds = kinds[:Co]
    fl = FLOOR_GLU if act == L.ACT_GLU else FLOOR
    errs = channel_check("out", got["out"], r64["out"], r32["out"], ULP16.get(odt, 0.0), okinds, fl)
    mean, invstd, rm, rv = bn_stats64(x, groups, 1e-5, 0.1, rm0, rv0)
    Bg = B // groups
    xh = torch.cat([(x[gi * Bg:(gi + 1) * Bg] - mean[gi].view(1, -1, 1)) * invstd[gi].view(1, -1, 1) for gi in range(groups)])
    dz = dz_of64(xh, gamma, beta, dout, act)
    # the backward reads mean as the library stores it, in fp32 (one rounding, <= u |mean|): that shifts xhat by dm * invstd and dx by
    # |s| dm invstd (|c1| + |xhat| |c0|), with c0 = mean dz, c1 = mean dz * xhat per group -- large next to the channel's own scale
    # where |mean| >> std (the offset channel).  Twice that, relative to the channel's dx scale, joins the bound.
    stored = torch.zeros(C, dtype=torch.float64)
    for gi in range(groups):
        sl = slice(gi * Bg, (gi + 1) * Bg)
        c0, c1 = dz[sl].mean(dim=(0, 2)).abs(), (dz[sl] * xh[sl]).mean(dim=(0, 2)).abs()
        shift = 2.0 ** -24 * mean[gi].abs() * invstd[gi]
        stored = torch.maximum(stored, (gamma * invstd[gi]).abs() * shift * (c1 + xh[sl].abs().amax(dim=(0, 2)) * c0))
    stored = 2 * stored / r64["dx"].abs().amax(dim=(0, 2)).clamp(min=1e-300)
    errs += channel_check("dx", got["dx"], r64["dx"], r32["dx"], ULP16.get(xdt, 0.0) + stored, kinds, fl)
    # |terms| of the gradient sums, from the float64 pass: dbeta = sum dz, dgamma = sum dz * xhat
    errs += sum_check("dbeta", got["dbeta"], r64["dbeta"], r32["dbeta"], dz.abs().sum(dim=(0, 2)), fl)
    errs += sum_check("dgamma", got["dgamma"], r64["dgamma"], r32["dgamma"], (dz * xh).abs().sum(dim=(0, 2)), fl)
    # statistics: each stored value is the fp64 result rounded once to fp32 (1/2 ulp); the fp64 sums are exact to ~2^-50 except the
    # 16-bit path's 8-value fp32 partial sums of x (<= 7 roundings, each <= 2^-24 of the partial's |x| sum): |d mean| <= 2^-21 mean|x|,
    # which moves var = E[x^2] - mean^2 by <= 2 |mean| |d mean|
    ax = torch.stack([x[gi * Bg:(gi + 1) * Bg].abs().mean(dim=(0, 2)) for gi in range(groups)])
    dm = (2.0 ** -21 if xdt != F32 else 2.0 ** -40) * ax
    var = 1.0 / invstd ** 2 - 1e-5
    dvar = 2 * mean.abs() * dm + 2.0 ** -50 * (var + mean ** 2)
    tol_mean = 2.0 ** -24 * mean.abs() + dm
    tol_inv = 2.0 ** -23 * invstd + 0.5 * invstd * dvar / (var + 1e-5)
    for k, want, tol in (("mean", mean, tol_mean), ("invstd", invstd, tol_inv)):
        d = (got[k] - want).abs()
        if not bool((d <= tol).all()):
            errs.append(f"{k}: |err| {d.max():.3e}, bound {tol.min():.3e}..{tol.max():.3e}")
    n = Bg * HW
    ub = n / (n - 1) if n > 1 else 1.0
    tol_rm = 2.0 ** -23 * (rm.abs() + rm0.abs()) + 0.1 * dm.sum(dim=0)
    tol_rv = 2.0 ** -23 * (rv.abs() + rv0.abs()) + 0.1 * ub * dvar.sum(dim=0)
    for k, want, tol in (("running_mean", rm, tol_rm), ("running_var", rv, tol_rv)):
        d = (got[k] - want).abs()
        if not bool((d <= tol).all()):
            errs.append(f"{k}: |err| {d.tolist()}, bound {tol.tolist()}")
    assert got["nbt"] == 7 + groups
    assert not errs, "\n  ".join([""] + errs)


def dz_of64(xh, gamma, beta, dout, act):
    """float64 dL/dz of the value half (and the gate half under GLU) -- the terms of the dgamma / dbeta sums"""
    z = xh * gamma.view(1, -1, 1) + beta.view(1, -1, 1)
    if act == L.ACT_GLU:
        co = z.shape[1] // 2
        sg = torch.sigmoid(z[:, co:])
        return torch.cat([dout * sg, dout * z[:, :co] * sg * (1 - sg)], dim=1)
    if act == L.ACT_LRELU:
        return torch.where(z > 0, dout, dout * 0.2)
    return dout


# -------------------------------------------------------------------------------------------------------------------- (d) edges
@pytest.mark.parametrize("B,C,HW,groups", [(2, 4, 8192, 1), (8, 4, 3072, 2), (4, 4, 64, 2)])
def test_workspace_one_byte_short_is_refused(B, C, HW, groups):
    """a workspace one byte short of *_ws_bytes returns AGAN_EWORKSPACE and launches nothing"""
    lib = L.load()
    Bg = B // groups
    x = torch.randn(B, C, HW, device=DEV)
    g, b = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    out, dx, dout = torch.zeros_like(x), torch.zeros_like(x), torch.randn_like(x)
    mean, inv = torch.zeros(groups, C, device=DEV), torch.ones(groups, C, device=DEV)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    st = HF._stream()
    fn = lib.agan_bn_train_fwd_ws_bytes(Bg, C, HW)
    if fn > 0:                                              # (the one-launch small path needs none)
        ws = alloc_ws(fn)
        rc = lib.agan_bn_train_fwd_dt(_p(x), _p(g), _p(b), None, _p(out), _p(mean), _p(inv), None, None, None, B, C, HW, 1e-5, 0.1,
                                      L.ACT_NONE, groups, _p(ws), fn - 1, st, None, F32, F32)
        assert rc == AGAN_EWORKSPACE, rc
        assert last_launch() == []
    bn = lib.agan_bn_act_bwd_ws_bytes(Bg, C, HW)
    ws = alloc_ws(bn)
    rc = lib.agan_bn_act_bwd_dt(_p(x), _p(dout), _p(mean), _p(inv), _p(g), _p(b), _p(dx), _p(dg), _p(db), B, C, HW, L.ACT_NONE, 0,
                                groups, _p(ws), bn - 1, st, None, F32, F32)
    assert rc == AGAN_EWORKSPACE, rc
    assert last_launch() == []
    torch.cuda.synchronize()
    assert bool((dx == 0).all()) and bool((dg == 0).all()) and bool((out == 0).all())


@pytest.mark.parametrize("xdt,odt", PAIRS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("HW", [12, 64, 49])
def test_eval_mode_fwd_vs_float64(HW, act, xdt, odt):
    """eval-mode agan_bn_act_fwd_dt with running statistics (mean = running_mean, invstd = 1/sqrt(running_var + eps)) against float64,
    per channel, bounded by twice the error of the same formula in torch fp32 + FLOOR (+ one 16-bit rounding)"""
    B, C = 5, 4
    gen = torch.Generator().manual_seed(HW * 10 + act)
    x, gamma, beta, r, _, kinds = random_inputs(B, C, HW, act, act == L.ACT_NONE, HW + act)
    x = q(x, xdt)
    r = q(r, odt) if r is not None else None
    rm = torch.tensor([0.2, 499.5, 0.7, 0.0], dtype=torch.float64)
    rv = torch.tensor([2.0, 0.3, 1e-7, 1e-6], dtype=torch.float64) * (1 + torch.rand(C, generator=gen, dtype=torch.float64))
    rm, rv = rm.float().double(), rv.float().double()
    invstd = (1.0 / torch.sqrt(rv + 1e-5)).float()
    Co = C // 2 if act == L.ACT_GLU else C
    xw, ow = alloc(B * C * HW, TDT[xdt], x), alloc(B * Co * HW, TDT[odt])
    rw = alloc(B * Co * HW, TDT[odt], r) if r is not None else None
    md, ivd, gd, bd = rm.float().to(DEV), invstd.to(DEV), gamma.float().to(DEV), beta.float().to(DEV)
    L.call("agan_bn_act_fwd_dt", _p(xw), _p(md), _p(ivd), _p(gd), _p(bd), _p(rw), _p(ow), B, C, HW, act, HF._stream(), None, xdt, odt)
    log = last_launch()
    assert [k[0] for k in log] == [K_FWD_APPLY] and log[0][1:4] == (act, xdt, odt), log
    torch.cuda.synchronize()
    assert guard_ok(ow, B * Co * HW)
    got = ow[:B * Co * HW].double().cpu().view(B, Co, HW)

    def ref(dtype):
        z = (x.to(dtype) - rm.to(dtype).view(1, -1, 1)) * torch.rsqrt(rv.to(dtype).view(1, -1, 1) + 1e-5) * gamma.to(dtype).view(1, -1, 1) \
            + beta.to(dtype).view(1, -1, 1)
        z = F.glu(z, dim=1) if act == L.ACT_GLU else (F.leaky_relu(z, 0.2) if act == L.ACT_LRELU else z)
        return (z + r.to(dtype) if r is not None else z).double()
    errs = channel_check("eval out", got, ref(torch.float64), ref(torch.float32), ULP16.get(odt, 0.0), kinds[:Co],
                         FLOOR_GLU if act == L.ACT_GLU else FLOOR)
    assert not errs, "\n  ".join([""] + errs)


# ---------------------------------------------------------------------------------------------------------------- (c) coverage
def required_forms():
    """every kernel form the dispatch rules of agan_bn_train_fwd_dt / agan_bn_act_bwd_dt can pick"""
    req = set()
    for act in ACTS:
        for xdt, odt in PAIRS:
            any16 = xdt != F32 or odt != F32
            for per in (2, 8, 32):
                req.add((K_SMALL_FWD, act, xdt, odt, per))
                req.add((K_SMALL_BWD, act, xdt, odt, per))
            for v in ((1, 4, 8) if any16 else (1, 4)):
                req.add((K_FWD_APPLY, act, xdt, odt, v))
                req.add((K_BWD_APPLY, act, xdt, odt, v))
                req.add((K_BWD_PART, act, xdt, odt, v))
    for xdt in (F32, BF16, F16):
        for w in ((1, 4, 8) if xdt != F32 else (1, 4)):
            req.add((K_STATS, 0, xdt, xdt, w))
    req.add((K_ROWS, 0, F32, F32, 1))
    return req


def test_the_cases_reach_every_bn_kernel_form():
    """run the device side of every case in both tables and require the union of their launch logs to cover required_forms()"""
    seen = set()
    for p in EXACT_CASES:
        got, _ = run_exact(*p.values)
        seen.update(got["log_fwd"] + got["log_bwd"])
    for p in RANDOM_CASES:
        got, _ = run_random(*p.values)
        seen.update(got["log_fwd"] + got["log_bwd"])
    req = required_forms()
    missing = sorted(req - seen)
    assert not missing, f"{len(missing)} of {len(req)} kernel forms not reached: {missing[:20]}"
    stray = sorted(k for k in seen if k[0] in (K_SMALL_FWD, K_SMALL_BWD, K_FWD_APPLY, K_BWD_APPLY, K_BWD_PART, K_STATS) and k not in req)
    assert not stray, f"forms outside the dispatch rules: {stray}"
