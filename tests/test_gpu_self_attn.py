"""The self-attention kernels (csrc/self_attn.hip) through the C ABI against float64, and the gate kernels.

Inputs are float64 tensors holding fp32 values: q, k, v and do unit normals (q times `qmul` where stated); with B >= 2 the last
sample's do is zero.  Outputs and the workspace start as NaN sentinels, are sized exactly and are followed by guard words
(test_gpu_bn_act's alloc / guard_ok / alloc_ws / ws_ok).

Slices: o per (b, n) against that position's max|o| over channels; lse per element against max(1, |lse|); dq, dk, dv per
(b, channel row) against that row's max.

Rule (test_gpu_damsm.py's): with e_ref = the worst slice of functional.self_attention_reference in fp32 on the CPU against the same in
float64, every slice of the kernel's result is within max(8 e_ref, 64 * 2^-24) of float64 and never more than 1e-4.  The fp32
reference is the yardstick, the kernel under test never is.  Every check prints
`SELF-ATTN-ERR | case | tensor | err | e_ref | err/e_ref | bound` (pytest -s) before it asserts.

Tile sizes of the kernels: a tile is 32 positions (queries and keys alike) and a chunk of the swept axis is 32 positions; a workgroup
owns a block of 32, 64 or 128 positions (1, 2 or 4 waves): the largest whose LDS fits 64 KB and that gives at least 256 workgroups,
else 32; accumulators are 32-row tiles along Dk (1 tile up to 32, else 2) and Dv (1 up to 32, 2 up to 64, else 4).  EDGE_CASES has
one case on each side of every one of these edges, FORM_CASES reaches every kernel form, and the closing test checks the launch logs
for that.

Exact conditions: the zero-do sample's dq, dk, dv are exactly 0.0; with M = 1, o[b, :, n] equals v[b, :, 0] bit for bit, dv is inside
the rule and dq, dk (exactly 0 in float64) are held to 64 * 2^-24 * Dv * max|do| * max|v| * max|k| and that with N * max|q| for
max|k| in absolute terms; a second run of every case gives the same bits.

Measured on an MI355X, worst err / e_ref over the slices of each tensor (the factor 8 holds everywhere; DESIGN.md section 23 has the
table per case): issue cases o 2.29, lse 2.23, dq 3.61, dk 2.92, dv 3.35; edge and form cases o 3.79, lse 2.66, dq 8.22, dk 9.04,
dv 8.36 -- the three above 8 are errors of 3.1e-6, 8.9e-7 and 9.0e-7 under the 64 * 2^-24 floor (sweeps of 8000 to 16384 positions
against 5, where the fp32 reference is lucky); the closest any slice comes to its bound is 81 % (that dq).  With one fp32 chain per
sweep instead of block sums, dq at M = 16384 was 12.2 x e_ref and outside the rule.
"""
import ctypes
import functools
import importlib

import pytest
import torch

from test_gpu_bn_act import alloc, alloc_ws, guard_ok, ws_ok

pytestmark = pytest.mark.gpu
DEV = "cuda"

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")

U = 2.0 ** -24
FLOOR = 64 * U
CEILING = 1e-4
K_FWD, K_DELTA, K_KV, K_Q, K_GATE_FWD, K_GATE_BWD, K_GATE_FINAL = range(1, 8)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _at(t, elems):
    return ctypes.c_void_p(t.data_ptr() + 4 * elems)


def last_launch():
    buf = (ctypes.c_int * 8)()
    n = L.load().agan_self_attn_last_launch(ctypes.cast(buf, ctypes.c_void_p), 8)
    assert 0 <= n <= 8, n
    return [(c // 100000, c // 100 % 1000, c // 10 % 10, c % 10) for c in buf[:n]]          # (kind, block, dk tiles, dv tiles)


# ---------------------------------------------------------------------------------------------------------------------- the cases
# (name, B, N, M, Dk, Dv, fused, qmul, scale)
def _c(name, B, N, M, Dk, Dv, fused=False, qmul=1.0, scale=1.0):
    return (name, B, N, M, Dk, Dv, fused, qmul, scale)


ISSUE_CASES = [
    _c("one-query", 2, 1, 64, 2, 3),
    _c("one-key", 2, 64, 1, 2, 3),
    _c("odd-33x31", 2, 33, 31, 3, 5),
    _c("dk1", 3, 64, 64, 1, 4),
    _c("129x257", 2, 129, 257, 8, 32),
    _c("257x129", 2, 257, 129, 4, 16),
    _c("fused-130", 2, 130, 130, 8, 33, fused=True),
    _c("scores-110", 2, 130, 130, 8, 16, qmul=6.0),
    _c("corner", 2, 200, 200, 64, 128, scale=0.4),
    _c("map32", 1, 1024, 1024, 8, 32),
    _c("map64", 1, 4096, 4096, 4, 16),
]
# One case on each side of every edge.  Blocks: B * ceil(len / 128) >= 256 -> 128, else B * ceil(len / 64) >= 256 -> 64, else 32
# (len = N for the forward and dq kernels, M for the dk / dv kernel), and only if the form's LDS fits 64 KB: with X the image rows of
# the form, 33 X floats (+ 64 in the dk / dv kernel) -- dk / dv: X = W (Dk' + Dv') + 32 dk_tiles + 32 dv_tiles <= 494;
# dq: X = W (Dk' + Dv') + 32 dk_tiles + Dv' <= 496 (Dk', Dv' rounded up to even; W = block / 32).
EDGE_CASES = [
    _c("tile-32x32", 1, 32, 32, 2, 2), _c("tile-31x33", 1, 31, 33, 2, 2), _c("tile-33x32", 1, 33, 32, 2, 2), _c("tile-64x65", 1, 64, 65, 2, 2),
    _c("dk32", 2, 40, 40, 32, 3), _c("dk33", 2, 40, 40, 33, 3), _c("dv32", 2, 40, 40, 2, 32), _c("dv33", 2, 40, 40, 2, 33),
    _c("dv64", 2, 40, 40, 2, 64), _c("dv65", 2, 40, 40, 2, 65),
    _c("n-block128", 2, 16384, 5, 2, 3), _c("n-block64-below128", 2, 16256, 5, 2, 3),
    _c("n-block64", 2, 8192, 5, 2, 3), _c("n-block32-below64", 2, 8128, 5, 2, 3),
    _c("m-block128", 2, 5, 16384, 2, 3), _c("m-block64-below128", 2, 5, 16256, 2, 3),
    _c("m-block64", 2, 5, 8192, 2, 3), _c("m-block32-below64", 2, 5, 8128, 2, 3),
    _c("kv-lds128-fits", 2, 5, 16384, 2, 80), _c("kv-lds128-over", 2, 5, 16384, 2, 81),
    _c("kv-lds64-fits", 2, 5, 16384, 64, 86), _c("kv-lds64-over", 2, 5, 16384, 64, 87),
    _c("q-lds128-fits", 2, 16384, 5, 2, 90), _c("q-lds128-over", 2, 16384, 5, 2, 91),
    _c("q-lds64-fits", 2, 16384, 5, 64, 100), _c("q-lds64-over", 2, 16384, 5, 64, 101),
]
# the blocks (forward, dk / dv, dq) the threshold cases must run with
BLOCKS = {"n-block128": (128, 32, 128), "n-block64-below128": (64, 32, 64), "n-block64": (64, 32, 64), "n-block32-below64": (32, 32, 32),
          "m-block128": (32, 128, 32), "m-block64-below128": (32, 64, 32), "m-block64": (32, 64, 32), "m-block32-below64": (32, 32, 32),
          "kv-lds128-fits": (32, 128, 32), "kv-lds128-over": (32, 64, 32), "kv-lds64-fits": (32, 64, 32), "kv-lds64-over": (32, 32, 32),
          "q-lds128-fits": (128, 32, 128), "q-lds128-over": (128, 32, 64), "q-lds64-fits": (128, 32, 64), "q-lds64-over": (128, 32, 32)}
BLOCK_LEN = {32: 40, 64: 8192, 128: 16384}          # with B = 2
FORM_CASES = [_c(f"form-n{blk}-dk{Dk}-dv{Dv}", 2, n, 5, Dk, Dv) for blk, n in BLOCK_LEN.items() for Dk in (2, 34) for Dv in (3, 34, 66)] + \
             [_c(f"form-m{blk}-dk{Dk}-dv{Dv}", 2, 5, m, Dk, Dv) for blk, m in BLOCK_LEN.items() for Dk in (2, 34) for Dv in (3, 34, 66)]
CASES = ISSUE_CASES + EDGE_CASES + FORM_CASES
IDS = [c[0] for c in CASES]
# every form the dispatch can choose: (kind, block, dk tiles, dv tiles)
FORMS = {(K_FWD, b, 0, t) for b in (32, 64, 128) for t in (1, 2, 4)} | \
        {(K_KV, b, kt, t) for b in (32, 64, 128) for kt in (1, 2) for t in (1, 2, 4)} - {(K_KV, 128, 2, 4)} | \
        {(K_Q, b, kt, 0) for b in (32, 64, 128) for kt in (1, 2)}


@functools.lru_cache(maxsize=None)
def inputs(case):
    name, B, N, M, Dk, Dv, fused, qmul, scale = case
    g = torch.Generator().manual_seed(1000 + IDS.index(name))
    q, k, v, do = (torch.randn(s, generator=g).double() for s in ((B, Dk, N), (B, Dk, M), (B, Dv, M), (B, Dv, N)))
    q = (q.float() * qmul).double()
    if B >= 2:
        do[-1] = 0.0
    return q, k, v, do


def reference(case, dtype):
    """(o, lse, dq, dk, dv) of functional.self_attention_reference and torch autograd in `dtype` on the CPU, as float64"""
    name, B, N, M, Dk, Dv, fused, qmul, scale = case
    q, k, v, do = (t.to(dtype).requires_grad_(i < 3) for i, t in enumerate(inputs(case)))
    o = HF.self_attention_reference(q, k, v, scale)
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    with torch.no_grad():
        lse = torch.logsumexp(scale * torch.bmm(q.transpose(1, 2), k), dim=2)
    return tuple(t.detach().double() for t in (o, lse, dq, dk, dv))


@functools.lru_cache(maxsize=None)
def references(case):
    return reference(case, torch.float32), reference(case, torch.float64)


def device_once(case):
    """-> (o, lse, dq, dk, dv) as float64 CPU tensors and the launch log; guards and the workspace tail checked"""
    name, B, N, M, Dk, Dv, fused, qmul, scale = case
    q, k, v, do = inputs(case)
    lib = L.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if fused:
        assert N == M
        C = 2 * Dk + Dv
        qkv = alloc(B * C * N, torch.float32, torch.cat((q, k, v), dim=1))
        dqkv = alloc(B * C * N, torch.float32)
        qp, kp, vp = _at(qkv, 0), _at(qkv, Dk * N), _at(qkv, 2 * Dk * N)
        dqp, dkp, dvp = _at(dqkv, 0), _at(dqkv, Dk * N), _at(dqkv, 2 * Dk * N)
        in_bs, g_bs = (C * N,) * 3, (C * N,) * 3
    else:
        qd, kd, vd = alloc(q.numel(), torch.float32, q), alloc(k.numel(), torch.float32, k), alloc(v.numel(), torch.float32, v)
        dqd, dkd, dvd = alloc(q.numel(), torch.float32), alloc(k.numel(), torch.float32), alloc(v.numel(), torch.float32)
        qp, kp, vp, dqp, dkp, dvp = _p(qd), _p(kd), _p(vd), _p(dqd), _p(dkd), _p(dvd)
        in_bs = g_bs = (Dk * N, Dk * M, Dv * M)
    dod = alloc(do.numel(), torch.float32, do)
    od, lsed = alloc(B * Dv * N, torch.float32), alloc(B * N, torch.float32)
    rc = lib.agan_self_attn_fwd(qp, kp, vp, _p(od), _p(lsed), B, N, M, Dk, Dv, *in_bs, Dv * N, scale, st)
    assert rc == 0, lib.agan_last_error()
    log = last_launch()
    nbytes = lib.agan_self_attn_bwd_ws_bytes(B, N, M, Dk, Dv)
    assert nbytes > 0
    ws = alloc_ws(nbytes)
    rc = lib.agan_self_attn_bwd(qp, kp, vp, _p(od), _p(lsed), _p(dod), dqp, dkp, dvp, B, N, M, Dk, Dv, *in_bs, Dv * N, Dv * N, *g_bs,
                                scale, _p(ws), nbytes, st)
    assert rc == 0, lib.agan_last_error()
    log += last_launch()
    torch.cuda.synchronize()
    assert ws_ok(ws, nbytes), "workspace tail overwritten"
    assert guard_ok(od, B * Dv * N) and guard_ok(lsed, B * N) and guard_ok(dod, do.numel()), "guard after o / lse / do overwritten"
    if fused:
        assert guard_ok(qkv, B * C * N) and guard_ok(dqkv, B * C * N), "guard after the fused tensors overwritten"
        g = dqkv[:B * C * N].view(B, C, N)
        dqo, dko, dvo = g[:, :Dk], g[:, Dk:2 * Dk], g[:, 2 * Dk:]
    else:
        for whole, ref in ((qd, q), (kd, k), (vd, v), (dqd, q), (dkd, k), (dvd, v)):
            assert guard_ok(whole, ref.numel()), "guard after an operand or a gradient overwritten"
        dqo, dko, dvo = dqd[:q.numel()].view(B, Dk, N), dkd[:k.numel()].view(B, Dk, M), dvd[:v.numel()].view(B, Dv, M)
    out = (od[:B * Dv * N].view(B, Dv, N), lsed[:B * N].view(B, N), dqo, dko, dvo)
    return tuple(t.contiguous().cpu() for t in out), log


@functools.lru_cache(maxsize=None)
def device(case):
    """two runs: the results of the first as fp32 CPU tensors, whether the second gave the same bits, the launch log"""
    first, log = device_once(case)
    second, log2 = device_once(case)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, second))
    return first, same and log == log2, log


# ------------------------------------------------------------------------------------------------------------ the error measure
def slice_errs(x, ref):
    """x, ref [S, K] float64: max|x - ref| / max|ref| per slice; a slice whose reference is exactly 0 has err 0 if x is exactly 0
    there and inf otherwise"""
    num, den = (x - ref).abs().amax(1), ref.abs().amax(1)
    zero = den == 0
    exact = x.abs().amax(1) == 0
    inf, nil = torch.full_like(num, float("inf")), torch.zeros_like(num)
    return torch.where(zero, torch.where(exact, nil, inf), num / den.clamp(min=1e-300)), zero


def check(case, what, got, r32, r64, lse=False):
    got = got.double()
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert bool(torch.isfinite(got).all()), f"{case[0]} {what}: not finite"
    if lse:
        den = r64.abs().clamp(min=1.0)
        e, er = ((got - r64).abs() / den).reshape(-1), ((r32 - r64).abs() / den).reshape(-1)
    else:
        e, _ = slice_errs(got, r64)
        er, zero = slice_errs(r32, r64)
        er = torch.where(zero, torch.zeros_like(er), er)
    e_ref = float(er.max())
    bound = min(max(8 * e_ref, FLOOR), CEILING)
    worst = float(e.max())
    print(f"SELF-ATTN-ERR | {case[0]} | {what} | err {worst:.2e} | e_ref {e_ref:.2e} | err/e_ref {worst / e_ref if e_ref else float('inf'):.2f} "
          f"| bound {bound:.2e}")
    bad = ~(e <= bound)
    assert not bool(bad.any()), f"{case[0]} {what}: {int(bad.sum())} of {e.numel()} slices outside {bound:.2e} (fp32 reference {e_ref:.2e}); " \
                                f"worst {worst:.3e}"


def per_position(o):                    # [B, Dv, N] -> [B * N, Dv]
    return o.permute(0, 2, 1).reshape(-1, o.shape[1])


def per_row(g):                         # [B, D, L] -> [B * D, L]
    return g.reshape(-1, g.shape[2])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_vs_float64(case):
    name, B, N, M, Dk, Dv, fused, qmul, scale = case
    (o, lse, dq, dk, dv), same, log = device(case)
    r32, r64 = references(case)
    q, k, v, do = inputs(case)
    assert [c[0] for c in log] == [K_FWD, K_DELTA, K_KV, K_Q], log
    assert same, "a second run gave other bits"
    if name in BLOCKS:
        assert (log[0][1], log[2][1], log[3][1]) == BLOCKS[name], log
    check(case, "o", per_position(o), per_position(r32[0]), per_position(r64[0]))
    check(case, "lse", lse, r32[1], r64[1], lse=True)
    check(case, "dv", per_row(dv), per_row(r32[4]), per_row(r64[4]))
    if M == 1:
        assert torch.equal(o.view(torch.int32), v[:, :, :1].float().expand(B, Dv, N).contiguous().view(torch.int32)), "o is not v bit for bit"
        assert float(r64[2].abs().max()) == 0.0 and float(r64[3].abs().max()) == 0.0
        base = 64 * U * Dv * float(do.abs().max()) * float(v.abs().max())
        eq, ek = float(dq.abs().max()), float(dk.abs().max())
        print(f"SELF-ATTN-ERR | {name} | dq, dk absolute | {eq:.2e} (bound {base * float(k.abs().max()):.2e}) | {ek:.2e} "
              f"(bound {base * N * float(q.abs().max()):.2e})")
        assert eq <= base * float(k.abs().max()) and ek <= base * N * float(q.abs().max())
    else:
        check(case, "dq", per_row(dq), per_row(r32[2]), per_row(r64[2]))
        check(case, "dk", per_row(dk), per_row(r32[3]), per_row(r64[3]))
    if B >= 2:
        for what, g in (("dq", dq), ("dk", dk), ("dv", dv)):
            assert float(g[-1].abs().max()) == 0.0, f"{what} of the zero-do sample is not exactly 0"
    if qmul != 1.0:
        with torch.no_grad():
            smax = float((scale * torch.bmm(q.transpose(1, 2), k)).abs().max())
        assert smax > 88.0, smax              # a naive exp would overflow


def test_the_cases_reach_every_kernel_form():
    seen = set()
    for case in CASES:
        seen |= set(device(case)[2])
    seen = {f for f in seen if f[0] in (K_FWD, K_KV, K_Q)}
    assert seen == FORMS, (sorted(FORMS - seen), sorted(seen - FORMS))


def test_nothing_of_size_n_by_m_is_allocated():
    B, N, Dk, Dv = 2, 4096, 4, 16
    g = torch.Generator().manual_seed(11)
    q, k, v, do = (torch.randn(s, generator=g).to(DEV) for s in ((B, Dk, N), (B, Dk, N), (B, Dv, N), (B, Dv, N)))
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    o = HF.self_attention(q, k, v)
    o.backward(do)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    scores = B * N * N * 4
    print(f"SELF-ATTN-MEM | forward + backward at (2, 4096, 4096, 4, 16) | rise {rise} B | one score matrix {scores} B")
    assert q.grad is not None and k.grad is not None and v.grad is not None
    assert rise < scores // 8, (rise, scores)


# ------------------------------------------------------------------------------------------------------------------- the gate
@pytest.mark.parametrize("n", [1, 63, 4097, 300000])
def test_gate_kernels(n):
    lib = L.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(n)
    x, y, dout = (torch.randn(n, generator=gen) for _ in range(3))
    g = torch.tensor([0.7])
    runs = []
    for _ in range(2):
        xd, yd, dd, gd = alloc(n, torch.float32, x), alloc(n, torch.float32, y), alloc(n, torch.float32, dout), alloc(1, torch.float32, g)
        out, dy = alloc(n, torch.float32), alloc(n, torch.float32)
        dg_fresh, dg_acc = alloc(1, torch.float32), alloc(1, torch.float32, torch.tensor([2.5]))
        assert lib.agan_scaled_residual_fwd(_p(xd), _p(yd), _p(gd), _p(out), n, st) == 0, lib.agan_last_error()
        assert [c[0] for c in last_launch()] == [K_GATE_FWD]
        nbytes = lib.agan_scaled_residual_bwd_ws_bytes(n)
        ws = alloc_ws(nbytes)
        for dg, acc in ((dg_fresh, 0), (dg_acc, 1)):
            assert lib.agan_scaled_residual_bwd(_p(dd), _p(yd), _p(gd), _p(dy), _p(dg), n, acc, _p(ws), nbytes, st) == 0, lib.agan_last_error()
            assert [c[0] for c in last_launch()] == [K_GATE_BWD, K_GATE_FINAL]
        torch.cuda.synchronize()
        assert ws_ok(ws, nbytes)
        for whole, m in ((xd, n), (yd, n), (dd, n), (gd, 1), (out, n), (dy, n), (dg_fresh, 1), (dg_acc, 1)):
            assert guard_ok(whole, m)
        runs.append(tuple(t.cpu() for t in (out[:n], dy[:n], dg_fresh[:1], dg_acc[:1])))
    out, dy, dg_fresh, dg_acc = runs[0]
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second run gave other bits"
    assert torch.equal(out.view(torch.int32), (x + g * y).view(torch.int32)), "out is not the fp32 torch statement's bits"
    assert torch.equal(dy.view(torch.int32), (g * dout).view(torch.int32))
    terms = dout.double() * y.double()
    exact, tol = float(terms.sum()), 64 * U * float(terms.abs().sum())
    print(f"SELF-ATTN-ERR | gate n={n} | dg | err {abs(float(dg_fresh) - exact):.2e} | bound {tol:.2e}")
    assert abs(float(dg_fresh) - exact) <= tol
    assert abs(float(dg_acc) - (2.5 + exact)) <= tol + 2 * U * abs(2.5 + exact)
