"""Sentence-conditioned BatchNorm + activation (csrc/cond_bn.hip) on every kernel form, through the C ABI, against float64.

Every case runs agan_cbn_train_fwd and agan_cbn_act_bwd once on the device (cached: the tests share the results) with guard tails
after every output and both workspaces.  The channels have the personalities of test_gpu_bn_act.py's RANDOM cases (ordinary, mean
10^3 x spread, near-constant, 1e-3 scale); delta makes the samples differ strongly: sample 0 has g[0, c] = gamma[c] + delta[0, c]
exactly 0, sample 1 has g negative and ten times the others' size, the last sample's dout is all zero (with B = 2 that is sample 1).

Criterion, per channel, for out, dx, both halves of ddelta, dgamma and dbeta (the rule of test_gpu_bn_act.py for these kernels):

    err(HIP) <= 2 err(torch fp32 CPU) + FLOOR * (the channel's max |float64 value|),   FLOOR = 16 * 2^-24, 64 * 2^-24 under GLU

both errors against backend.functional.cond_bn_act_reference in float64 (autograd for the gradients); the comparator is the same
function in float32 on the CPU.

Exact: the zero-dout sample's ddelta rows are 0.0; mean, invstd and the running statistics equal agan_bn_train_fwd's on the same x bit
for bit; a second run gives the same bits; accumulate = 1 adds into preset dgamma / dbeta.  A closing test requires the launch logs
(agan_cbn_last_launch) of the case table to cover every kernel form the dispatch can choose.

Measured on MI355X (test_cbn_vs_float64 prints every figure): worst err / bound over the 26 cases 0.50 for dx, 0.41 for ddelta, 0.47 for
dgamma, 0.42 for dbeta, below 0.01 for out.  With xhat of the Q sums in fp32 the case B3-C2-HW1-none missed: dgamma[0] 1.499e-06 against a
bound of 1.050e-06 (torch fp32 4.8e-08) -- two terms that cancel; the kernels form that xhat in fp64 since (4.8e-08).
"""
import ctypes
import functools
import importlib

import pytest
import torch

import test_gpu_bn_act as BN

pytestmark = pytest.mark.gpu
DEV = "cuda"

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")

NONE, GLU = L.ACT_NONE, L.ACT_GLU
ACT_NAME = {NONE: "none", GLU: "glu"}
FLOOR = {NONE: 16 * 2.0 ** -24, GLU: 64 * 2.0 ** -24}
EPS, MOM = 1e-5, 0.1
# launch-log kinds (include/agan.h: agan_cbn_last_launch)
K_ROWS, K_SMALL, K_TWO_PASS, K_FWD, K_BWD_WAVE, K_BWD_BLOCK, K_BWD_FINAL, K_BWD_APPLY = range(1, 9)

# (B, C, HW): the smallest shapes that exercise each piece of indexing, on both sides of every form threshold
SHAPES = [
    (3, 2, 1),          # [B, C] rows statistics, width 1
    (2, 4, 9),          # odd HW
    (3, 6, 25),         # odd HW, three plane pairs per sample
    (2, 4, 12),         # HW = 4 mod 8: width 4
    (3, 4, 64),
    (5, 6, 256),        # n 1280: one-launch statistics, 8 values per thread
    (3, 2, 1024),       # the largest plane a wave sums; n 3072: 32 values per thread
    (3, 2, 1028),       # the smallest plane a workgroup sums
    (2, 4, 2048),       # n 4096: one-launch statistics, one chunk per plane
    (2, 2, 4099),       # n 8198: two-pass statistics, width 1; two chunks per plane, the second ragged
    (2, 4, 16384),      # eight chunks per plane
    (3, 2, 66000),      # 32 chunks per plane, ragged tail
    (7, 16, 64),        # many small planes: more than one workgroup of four waves, the last one partly idle under GLU
]
CASES = [pytest.param(B, C, HW, act, id=f"B{B}-C{C}-HW{HW}-{ACT_NAME[act]}") for B, C, HW in SHAPES for act in (NONE, GLU)]

_p, alloc, guard_ok, alloc_ws, ws_ok = BN._p, BN.alloc, BN.guard_ok, BN.alloc_ws, BN.ws_ok


def last_launch():
    buf = (ctypes.c_int * 16)()
    n = L.load().agan_cbn_last_launch(ctypes.cast(buf, ctypes.c_void_p), 16)
    assert 0 <= n <= 16, n
    return [(c // 100000, c // 10000 % 10, c % 10000) for c in buf[:n]]


def f32(t):
    """float64 values that fp32 holds exactly"""
    return t.float().double()


def inputs(B, C, HW, act, seed):
    x, gamma, beta, _, dout, kinds = BN.random_inputs(B, C, HW, act, False, seed)
    x, gamma, beta, dout = f32(x), f32(gamma), f32(beta), f32(dout)
    gen = torch.Generator().manual_seed(1000 + seed)
    delta = torch.randn(B, 2 * C, generator=gen, dtype=torch.float64)
    delta[:, :C] *= 0.3
    delta[:, C:] *= 0.5
    delta[0, :C] = -gamma                               # g exactly 0 (gamma is an fp32 value: gamma + (-gamma) = 0 in fp32 too)
    if B >= 2:
        delta[1, :C] = -11.0 * gamma                    # g = -10 gamma: negative, ten times the others
        dout[B - 1] = 0.0
    return x, gamma, beta, f32(delta), dout, kinds


def cbn_device(x, gamma, beta, delta, dout, act, rm0, rv0, dg0, db0, accumulate, amax=False):
    """agan_cbn_train_fwd + agan_cbn_act_bwd on the device.  x [B, C, HW], dout [B, Co, HW] (float64 holding fp32 values).  Returns float64
    CPU results, the raw fp32 statistics, the launch logs and the guard checks."""
    lib = L.load()
    B, C, HW = x.shape
    Co = C // 2 if act == GLU else C
    nx, no = B * C * HW, B * Co * HW
    xw, ow = alloc(nx, torch.float32, x), alloc(no, torch.float32)
    g, b = gamma.float().to(DEV), beta.float().to(DEV)
    dlw = alloc(B * 2 * C, torch.float32, delta)
    mw, iw = alloc(C, torch.float32), alloc(C, torch.float32)
    rmw, rvw = alloc(C, torch.float32, rm0), alloc(C, torch.float32, rv0)
    nbt = alloc(1, torch.int64, torch.tensor([7]))
    fws_n = lib.agan_cbn_train_fwd_ws_bytes(B, C, HW)
    fws = alloc_ws(fws_n)
    oam = torch.zeros(L.AMAX_SLOT, device=DEV) if amax else None
    st = HF._stream()
    rc = lib.agan_cbn_train_fwd(_p(xw), _p(g), _p(b), _p(dlw), _p(ow), _p(mw), _p(iw), _p(rmw), _p(rvw), _p(nbt), B, C, HW, EPS, MOM, act,
                                _p(fws), fws_n, st, _p(oam))
    assert rc == 0, (rc, lib.agan_last_error())
    log_f = last_launch()
    dw, dxw = alloc(no, torch.float32, dout), alloc(nx, torch.float32)
    ddw = alloc(B * 2 * C, torch.float32)
    dgw, dbw = alloc(C, torch.float32, dg0), alloc(C, torch.float32, db0)
    bws_n = lib.agan_cbn_act_bwd_ws_bytes(B, C, HW)
    bws = alloc_ws(bws_n)
    dam = torch.zeros(L.AMAX_SLOT, device=DEV) if amax else None
    rc = lib.agan_cbn_act_bwd(_p(xw), _p(dw), _p(mw), _p(iw), _p(g), _p(b), _p(dlw), _p(dxw), _p(ddw), _p(dgw), _p(dbw), B, C, HW, act,
                              accumulate, _p(bws), bws_n, st, _p(dam))
    assert rc == 0, (rc, lib.agan_last_error())
    log_b = last_launch()
    torch.cuda.synchronize()
    guards = {"out": guard_ok(ow, no), "dx": guard_ok(dxw, nx), "mean": guard_ok(mw, C), "invstd": guard_ok(iw, C),
              "running_mean": guard_ok(rmw, C), "running_var": guard_ok(rvw, C), "nbt": guard_ok(nbt, 1), "ddelta": guard_ok(ddw, B * 2 * C),
              "dgamma": guard_ok(dgw, C), "dbeta": guard_ok(dbw, C), "fwd ws": ws_ok(fws, fws_n), "bwd ws": ws_ok(bws, bws_n),
              "x": guard_ok(xw, nx), "dout": guard_ok(dw, no), "delta": guard_ok(dlw, B * 2 * C)}
    raw = lambda w, n: w[:n].detach().cpu().clone()
    r = {"out": raw(ow, no).double().view(B, Co, HW), "dx": raw(dxw, nx).double().view(B, C, HW),
         "ddelta": raw(ddw, B * 2 * C).double().view(B, 2 * C), "dgamma": raw(dgw, C).double(), "dbeta": raw(dbw, C).double(),
         "stats": {k: raw(w, C) for k, w in (("mean", mw), ("invstd", iw), ("running_mean", rmw), ("running_var", rvw))},
         "nbt": int(nbt[0]), "log_fwd": log_f, "log_bwd": log_b, "guards": guards,
         "inputs_unchanged": torch.equal(raw(xw, nx).double(), x.reshape(-1)) and torch.equal(raw(dlw, B * 2 * C).double(), delta.reshape(-1))}
    if amax:
        r["out_amax"], r["dx_amax"] = float(oam.max()), float(dam.max())
    return r


def reference(x, gamma, beta, delta, dout, act, dtype):
    """cond_bn_act_reference and its autograd gradients on the CPU in `dtype` -> float64 tensors"""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    xs, g, b, d = leaf(x), leaf(gamma), leaf(beta), leaf(delta)
    out, _, _ = HF.cond_bn_act_reference(xs, g, b, d, None, None, True, act, EPS, MOM)
    out.backward(dout.to(dtype))
    return {"out": out.detach().double(), "dx": xs.grad.double(), "ddelta": d.grad.double(), "dgamma": g.grad.double(),
            "dbeta": b.grad.double()}


def running0(C):
    return torch.linspace(-1, 1, C, dtype=torch.float64), torch.linspace(0.5, 2, C, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def run_case(B, C, HW, act):
    seed = SHAPES.index((B, C, HW))
    x, gamma, beta, delta, dout, kinds = inputs(B, C, HW, act, seed)
    rm0, rv0 = running0(C)
    z = torch.zeros(C, dtype=torch.float64)
    got = cbn_device(x, gamma, beta, delta, dout, act, rm0, rv0, z, z, 0)
    r64 = reference(x, gamma, beta, delta, dout, act, torch.float64)
    r32 = reference(x, gamma, beta, delta, dout, act, torch.float32)
    return got, r64, r32, (x, gamma, beta, delta, dout, kinds, rm0, rv0)


def criterion(got, r64, r32, act, kinds, names=("out", "dx", "ddelta", "dgamma", "dbeta"), label=""):
    """the failures of the per-channel rule; prints every quantity's worst channel first"""
    as3 = {"out": lambda t: t, "dx": lambda t: t, "ddelta": lambda t: t.unsqueeze(2), "dgamma": lambda t: t.view(1, -1, 1),
           "dbeta": lambda t: t.view(1, -1, 1)}
    errs = []
    for k in names:
        g, a, b = as3[k](got[k]), as3[k](r64[k]), as3[k](r32[k])
        scale = a.abs().amax(dim=(0, 2)).clamp(min=1e-300)
        eh, et = (g - a).abs().amax(dim=(0, 2)) / scale, (b - a).abs().amax(dim=(0, 2)) / scale
        w = int((eh - 2 * et).argmax())
        print(f"{label}{k}: worst channel {w}: err {float(eh[w]):.3e}, torch fp32 {float(et[w]):.3e}, floor {FLOOR[act]:.3e}")
        errs += BN.channel_check(k, g, a, b, 0.0, kinds, FLOOR[act])
    return errs


@pytest.mark.parametrize("B,C,HW,act", CASES)
def test_cbn_vs_float64(B, C, HW, act):
    got, r64, r32, (x, gamma, beta, delta, dout, kinds, rm0, rv0) = run_case(B, C, HW, act)
    bad = [k for k, v in got["guards"].items() if not v]
    assert not bad, f"guard tail overwritten: {bad}"
    assert got["inputs_unchanged"], "x or delta was modified"
    assert got["nbt"] == 8
    errs = criterion(got, r64, r32, act, kinds)
    assert not errs, "\n  ".join([""] + errs)
    if B >= 2:          # the zero-dout sample: its S and Q are sums of zeros
        assert bool((got["ddelta"][B - 1] == 0.0).all()), got["ddelta"][B - 1]
    assert bool((delta[0, :C] + gamma == 0).all())          # (the case construction: g[0] is exactly 0)


@pytest.mark.parametrize("B,C,HW,act", CASES)
def test_statistics_are_bn_train_fwds_bit_for_bit(B, C, HW, act):
    got, _, _, (x, gamma, beta, delta, dout, kinds, rm0, rv0) = run_case(B, C, HW, act)
    z = torch.zeros(C, dtype=torch.float64)
    bn = BN.bn_device(x, gamma, beta, None, dout, act, 1, L.DT_F32, L.DT_F32, EPS, MOM, rm0, rv0, z, z, 0)
    for k, v in got["stats"].items():
        want = bn[k].reshape(-1).float()
        assert torch.equal(v.view(torch.int32), want.view(torch.int32)), f"{k}: {BN.first_diff(v.double(), want.double())}"
    assert got["nbt"] == bn["nbt"]


@pytest.mark.parametrize("B,C,HW,act", CASES)
def test_two_runs_give_the_same_bits(B, C, HW, act):
    got, _, _, (x, gamma, beta, delta, dout, kinds, rm0, rv0) = run_case(B, C, HW, act)
    z = torch.zeros(C, dtype=torch.float64)
    again = cbn_device(x, gamma, beta, delta, dout, act, rm0, rv0, z, z, 0)
    for k in ("out", "dx", "ddelta", "dgamma", "dbeta"):
        assert torch.equal(got[k].float().view(torch.int32), again[k].float().view(torch.int32)), k
    for k in got["stats"]:
        assert torch.equal(got["stats"][k].view(torch.int32), again["stats"][k].view(torch.int32)), k


@pytest.mark.parametrize("B,C,HW,act", CASES)
def test_zero_delta_agrees_with_bn_act(B, C, HW, act):
    """delta = 0 against agan_bn_train_fwd / agan_bn_act_bwd on the same operands.  out: the same bits -- the forward apply is bn_act's
    arithmetic (make_affine / norm_of of bn_common.h on gamma + 0, beta + 0 and the same statistics).  dx, per channel: |cbn - bn| <=
    2 err(torch fp32) + FLOOR * max|float64|, the criterion with bn_act's result in the place of the value compared with.  dgamma, dbeta:
    agan_bn_act_bwd's sums are held by their own test to |err| <= 2 |err(torch fp32)| + FLOOR * (sum of |terms|), not to their own size
    (a sum of signed terms may cancel; its xhat is fp32, here fp64), so the difference is held to that rule.  ddelta is then the
    per-sample split of the conditional kernels' dgamma / dbeta."""
    _, _, _, (x, gamma, beta, _, dout, kinds, rm0, rv0) = run_case(B, C, HW, act)
    zero = torch.zeros(B, 2 * C, dtype=torch.float64)
    z = torch.zeros(C, dtype=torch.float64)
    got = cbn_device(x, gamma, beta, zero, dout, act, rm0, rv0, z, z, 0)
    bn = BN.bn_device(x, gamma, beta, None, dout, act, 1, L.DT_F32, L.DT_F32, EPS, MOM, rm0, rv0, z, z, 0)
    r64 = reference(x, gamma, beta, zero, dout, act, torch.float64)
    r32 = reference(x, gamma, beta, zero, dout, act, torch.float32)
    assert torch.equal(got["out"], bn["out"]), f"out: {BN.first_diff(got['out'], bn['out'])}"
    scale = r64["dx"].abs().amax(dim=(0, 2)).clamp(min=1e-300)
    diff, et = (got["dx"] - bn["dx"]).abs().amax(dim=(0, 2)) / scale, (r32["dx"] - r64["dx"]).abs().amax(dim=(0, 2)) / scale
    print(f"cbn - bn dx: worst {float(diff.max()):.3e}")
    errs = [f"cbn - bn dx[{c}]: {float(diff[c]):.3e} > {float(2 * et[c] + FLOOR[act]):.3e}" for c in range(C)
            if not float(diff[c]) <= float(2 * et[c] + FLOOR[act])]
    mean, invstd, _, _ = BN.bn_stats64(x, 1, EPS, MOM, rm0, rv0)
    xh = (x - mean[0].view(1, -1, 1)) * invstd[0].view(1, -1, 1)
    dz = BN.dz_of64(xh, gamma, beta, dout, act)
    for k, terms in (("dbeta", dz.abs().sum(dim=(0, 2))), ("dgamma", (dz * xh).abs().sum(dim=(0, 2)))):
        print(f"cbn - bn {k}: worst {float(((got[k] - bn[k]).abs() / terms.clamp(min=1e-300)).max()):.3e} of the sum of |terms|")
        errs += BN.sum_check(f"cbn - bn {k}", got[k], bn[k], bn[k] + (r32[k] - r64[k]), terms, FLOOR[act])
    for k, half in (("dgamma", got["ddelta"][:, :C]), ("dbeta", got["ddelta"][:, C:])):
        split = half.sum(dim=0)
        assert bool(((split - got[k]).abs() <= 2.0 ** -22 * half.abs().sum(dim=0)).all()), f"ddelta does not add up to {k}"
    assert not errs, "\n  ".join([""] + errs)


@pytest.mark.parametrize("B,C,HW,act", [(3, 6, 25, GLU), (5, 6, 256, NONE), (2, 2, 4099, GLU), (2, 4, 16384, NONE)])
def test_accumulate_adds_into_preset_gradients_and_amax_slots_fill(B, C, HW, act):
    got, _, _, (x, gamma, beta, delta, dout, kinds, rm0, rv0) = run_case(B, C, HW, act)
    dg0 = f32(torch.linspace(-3, 5, C, dtype=torch.float64))
    db0 = f32(torch.linspace(7, -2, C, dtype=torch.float64))
    acc = cbn_device(x, gamma, beta, delta, dout, act, rm0, rv0, dg0, db0, 1, amax=True)
    assert not [k for k, v in acc["guards"].items() if not v]
    for k, pre in (("dgamma", dg0), ("dbeta", db0)):
        want = (pre.float() + got[k].float()).double()          # one fp32 addition of the preset and the sum rounded to fp32
        assert torch.equal(acc[k], want), f"{k}: {BN.first_diff(acc[k], want)}"
    for k in ("out", "dx", "ddelta"):
        assert torch.equal(acc[k], got[k]), k
    for k, am in (("out", acc["out_amax"]), ("dx", acc["dx_amax"])):
        assert am == float(got[k].abs().max()), f"{k} amax {am!r} vs max|{k}| {float(got[k].abs().max())!r}"


@pytest.mark.parametrize("act", [NONE, GLU])
@pytest.mark.parametrize("B,C,HW", [(3, 6, 25), (2, 4, 12)])
def test_eval_mode_fwd_vs_float64(B, C, HW, act):
    """agan_cbn_act_fwd with running statistics (mean = running_mean, invstd = 1 / sqrt(running_var + eps)) against float64"""
    x, gamma, beta, delta, _, kinds = inputs(B, C, HW, act, 50 + HW + act)
    gen = torch.Generator().manual_seed(HW * 10 + act)
    rm = torch.tensor([0.2, 499.5, 0.7, 0.0, 0.25, 500.25], dtype=torch.float64)[:C]
    rv = torch.tensor([2.0, 0.3, 1e-7, 1e-6, 2.5, 0.2], dtype=torch.float64)[:C] * (1 + torch.rand(C, generator=gen, dtype=torch.float64))
    rm, rv = f32(rm), f32(rv)
    invstd = (1.0 / torch.sqrt(rv + EPS)).float()
    Co = C // 2 if act == GLU else C
    xw, ow, dlw = alloc(B * C * HW, torch.float32, x), alloc(B * Co * HW, torch.float32), alloc(B * 2 * C, torch.float32, delta)
    md, ivd, gd, bd = rm.float().to(DEV), invstd.to(DEV), gamma.float().to(DEV), beta.float().to(DEV)
    L.call("agan_cbn_act_fwd", _p(xw), _p(md), _p(ivd), _p(gd), _p(bd), _p(dlw), _p(ow), B, C, HW, act, HF._stream(), None)
    assert last_launch() == [(K_FWD, act, 4 if HW % 4 == 0 else 1)]
    torch.cuda.synchronize()
    assert guard_ok(ow, B * Co * HW)
    got = {"out": ow[:B * Co * HW].double().cpu().view(B, Co, HW)}
    ref = lambda dt: {"out": HF.cond_bn_act_reference(x.to(dt), gamma.to(dt), beta.to(dt), delta.to(dt), rm.to(dt), rv.to(dt), False, act,
                                                      EPS, MOM)[0].double()}
    errs = criterion(got, ref(torch.float64), ref(torch.float32), act, kinds[:Co], ("out",), "eval ")
    assert not errs, "\n  ".join([""] + errs)


def required_forms():
    """every kernel form the dispatch rules of agan_cbn_train_fwd / agan_cbn_act_bwd can pick"""
    req = {(K_ROWS, 0, 1), (K_TWO_PASS, 0, 1), (K_TWO_PASS, 0, 4)}
    req |= {(K_SMALL, 0, per) for per in (2, 8, 32)}
    for act in (NONE, GLU):
        req.add((K_BWD_FINAL, act, 1))
        for v in (1, 4):
            req |= {(k, act, v) for k in (K_FWD, K_BWD_WAVE, K_BWD_BLOCK, K_BWD_APPLY)}
    return req


def test_the_cases_reach_every_cbn_kernel_form():
    seen = set()
    for p in CASES:
        got = run_case(*p.values)[0]
        assert [k[0] for k in got["log_fwd"]][1:] == [K_FWD] and got["log_fwd"][0][0] in (K_ROWS, K_SMALL, K_TWO_PASS), got["log_fwd"]
        assert [k[0] for k in got["log_bwd"]][1:] == [K_BWD_FINAL, K_BWD_APPLY] and got["log_bwd"][0][0] in (K_BWD_WAVE, K_BWD_BLOCK)
        B, C, HW, act = p.values
        assert got["log_bwd"][0][0] == (K_BWD_WAVE if HW <= 1024 else K_BWD_BLOCK), (HW, got["log_bwd"])
        seen.update(got["log_fwd"] + got["log_bwd"])
    req = required_forms()
    missing = sorted(req - seen)
    assert not missing, f"{len(missing)} of {len(req)} kernel forms not reached: {missing}"
    stray = sorted(seen - req)
    assert not stray, f"forms outside the dispatch rules: {stray}"
