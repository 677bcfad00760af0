"""The spectral-normalisation kernels (csrc/spectral.hip) through the C ABI, per slice against the float64 statement
(backend.functional.spectral_weight_reference), on both sides of the kernels' one dispatch seam (Cout * K <= 8192 | above), with one and two
column segments, and with rows that are and are not 16-byte aligned.

Measure and rule are those of tests/test_gpu_word_corr.py, restated in tests/spectral_cases.py: every slice -- u', v and sigma one slice
each, every row of W_sn and of dW -- is compared with the slice's own float64 maximum and must be within max(8 e_ref, 64 * 2^-24) of
float64, never more than RTOL / 10 = 1e-4, e_ref being the worst slice of the fp32 reference on the same inputs.  W ~ N(0, K^-1/2), u0 a
normalised normal vector, dW_sn ~ N(0, 1).  iterate = 1 starts from (u0, v0); iterate = 0 from the float64 reference's (u', v) of that
iteration rounded to fp32, the state an eval-mode forward meets.  The backward runs with the accumulate flags off, and on onto a random
prior.  Outputs start as NaN sentinels, are sized exactly and are followed by guard words that must survive; the workspace is sized exactly
and NaN-poisoned; every run is repeated and must be bit-identical.  `one` (a 1 x 1 weight) has an identically zero gradient in exact
arithmetic: its dW is checked by |dW| <= 8 * 2^-24 * |dW_sn| / sigma (plus, onto a prior, the rounding of that one sum: 2^-24 |result|).

Every check prints `SPECTRAL-ERR | case | tensor | err | e_ref | err/e_ref | bound` (pytest -s) before it asserts.

Measured on an MI355X: worst slice error / e_ref of the same tensor, over iterate 1 and 0, accumulate off and on, and the shifted bases
(DESIGN.md section 27 carries the same table):

                u'               v                sigma            W_sn/row         dW/row
one             0 / 0            0 / 0            0 / 0            0 / 0            |dW| = 0 (limit 7.4e-7)
head            0 / 0            5.6e-8 / 5.6e-8  8.1e-8 / 3.6e-8  1.0e-7 / 5.6e-8  1.2e-7 / 8.1e-8
first           1.3e-7 / 9.8e-8  5.6e-8 / 6.4e-8  1.6e-7 / 1.6e-7  1.9e-7 / 1.9e-7  2.5e-7 / 2.6e-7
odd             4.9e-8 / 6.3e-8  3.7e-8 / 9.9e-8  9.1e-8 / 9.5e-9  1.2e-7 / 5.8e-8  1.6e-7 / 7.7e-8
tall            2.4e-7 / 1.8e-7  2.7e-7 / 1.5e-7  6.2e-8 / 5.1e-8  1.2e-7 / 1.1e-7  1.6e-7 / 1.7e-7
wide            7.5e-8 / 1.4e-7  1.1e-7 / 9.8e-8  6.8e-8 / 5.1e-8  9.6e-8 / 8.3e-8  1.1e-7 / 1.1e-7
joint           5.5e-8 / 5.6e-8  1.3e-7 / 1.7e-7  8.7e-8 / 3.2e-8  1.3e-7 / 8.3e-8  1.7e-7 / 9.9e-8
joint_odd       7.6e-8 / 6.0e-8  1.2e-7 / 7.9e-8  2.9e-8 / 2.9e-8  8.0e-8 / 8.0e-8  1.1e-7 / 1.0e-7
mid             1.5e-7 / 2.4e-7  9.3e-8 / 3.8e-7  8.4e-8 / 1.3e-7  1.3e-7 / 1.8e-7  1.6e-7 / 2.1e-7
big             1.0e-7 / 4.0e-7  1.5e-7 / 7.1e-7  1.8e-8 / 1.2e-7  7.5e-8 / 1.8e-7  1.0e-7 / 1.9e-7
seam_lo         1.1e-7 / 1.7e-7  2.3e-7 / 1.6e-7  3.7e-8 / 3.7e-8  7.5e-8 / 7.5e-8  1.3e-7 / 1.3e-7
seam_hi         8.7e-8 / 9.9e-8  9.2e-8 / 2.1e-7  6.2e-8 / 6.2e-8  1.1e-7 / 1.1e-7  1.6e-7 / 1.4e-7
joint_big       8.8e-8 / 9.7e-8  1.0e-7 / 1.6e-7  7.4e-8 / 3.7e-8  1.2e-7 / 8.6e-8  1.8e-7 / 1.0e-7
joint_big_odd   1.0e-7 / 1.2e-7  8.8e-8 / 2.2e-7  2.1e-8 / 2.1e-8  6.7e-8 / 6.7e-8  1.1e-7 / 9.0e-8
joint_mixed     1.2e-7 / 1.7e-7  1.2e-7 / 2.9e-7  1.0e-7 / 1.2e-7  1.5e-7 / 1.8e-7  1.8e-7 / 1.5e-7
strips          1.1e-7 / 3.3e-7  1.2e-7 / 3.0e-7  2.7e-8 / 2.7e-8  7.8e-8 / 7.8e-8  9.7e-8 / 1.0e-7

The largest error of any slice is 2.7e-7; 8 e_ref never exceeds the floor 64 * 2^-24 = 3.8e-6, so the floor was the bound everywhere.
"""
import ctypes
import importlib

import pytest
import torch

from spectral_cases import CASE_IDS, CASES, FORM_BIG, FORM_SMALL, U, case_inputs, check_slices, form_of

pytestmark = pytest.mark.gpu
DEV = "cuda"

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")

GUARD = 64
SENT = 0x7FC0DEAD


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(t, shift=0):
    """fp32 device copy followed by GUARD NaN-pattern sentinels, `shift` floats off a 16-byte boundary; returns (view, whole)"""
    t = t.reshape(-1)
    whole = torch.empty(shift + t.numel() + GUARD, dtype=torch.float32, device=DEV)
    whole.view(torch.int32).fill_(SENT)
    whole[shift:shift + t.numel()].copy_(t.float())
    return whole[shift:shift + t.numel()], whole


def poisoned(n, shift=0):
    whole = torch.empty(shift + n + GUARD, dtype=torch.float32, device=DEV)
    whole.view(torch.int32).fill_(SENT)
    return whole[shift:shift + n], whole


def tail_ok(whole, n, shift=0):
    return bool((whole[shift + n:].view(torch.int32) == SENT).all()) and bool((whole[:shift].view(torch.int32) == SENT).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_REF = {}


def _reference(case, iterate, dtype):
    """(u, v, sigma, W_sn, dW) of the torch statement in `dtype` on the CPU; with iterate = 0, from the eval state"""
    _, cout, k0, k1 = case
    W, u0, v0, dW, _ = case_inputs(case)
    if not iterate:
        u0, v0 = eval_state(case)
    w0 = W[:, :k0].to(dtype).clone().requires_grad_(True)
    w1 = W[:, k0:].to(dtype).clone().requires_grad_(True) if k1 else None
    u, v = u0.to(dtype).clone(), v0.to(dtype).clone()
    out = HF.spectral_weight_reference(w0, u, v, bool(iterate), second=w1)
    sn = torch.cat(out, dim=1) if k1 else out
    (sn * dW.to(dtype)).sum().backward()
    grad = torch.cat([w0.grad, w1.grad], dim=1) if k1 else w0.grad
    sigma = torch.dot(u, torch.mv(W.to(dtype), v))
    return u, v, sigma.reshape(1), sn.detach(), grad


def references(case, iterate):
    key = (case[0], iterate)
    if key not in _REF:
        _REF[key] = (_reference(case, iterate, torch.float32), _reference(case, iterate, torch.float64))
    return _REF[key]


def eval_state(case):
    """the (u', v) of the float64 iteration, rounded to fp32: what an eval-mode forward starts from"""
    r64 = references(case, 1)[1]
    return r64[0].float(), r64[1].float()


def hip(case, iterate, accumulate, shift=0):
    """one forward + backward through the C ABI on freshly poisoned, exactly sized buffers; everything comes back on the CPU"""
    lib = L.load()
    name, cout, k0, k1 = case
    K = k0 + k1
    W, u0, v0, dW, prior = case_inputs(case)
    if not iterate:
        u0, v0 = eval_state(case)
    seg = lambda t, s: t[:, :k0].contiguous() if s == 0 else t[:, k0:].contiguous()
    w = [dev(seg(W, s), shift) for s in range(2 if k1 else 1)]
    d = [dev(seg(dW, s), shift) for s in range(2 if k1 else 1)]
    ud, vd = dev(u0), dev(v0)
    nf, nb = lib.agan_spectral_fwd_ws_bytes(cout, k0, k1), lib.agan_spectral_bwd_ws_bytes(cout, k0, k1)
    assert nf % 4 == 0 and nb % 4 == 0 and (nf == 0) == (nb == 0) == (form_of(case) == FORM_SMALL)
    sizes = dict(u=cout, v=K, sigma=1, wsn0=cout * k0, wsn1=cout * k1, dw0=cout * k0, dw1=cout * k1, wsf=nf // 4, wsb=nb // 4)
    buf = {k: poisoned(n, shift if k[:-1] in ("wsn", "dw") else 0) for k, n in sizes.items()}
    if accumulate:
        for s in range(2 if k1 else 1):
            buf[f"dw{s}"][0].copy_(seg(prior, s).reshape(-1))
    second = lambda t: _p(t[0]) if k1 else None
    L.call("agan_spectral_fwd", _p(w[0][0]), second(w[-1]), _p(ud[0]), _p(vd[0]), _p(buf["u"][0]) if iterate else None,
           _p(buf["v"][0]) if iterate else None, _p(buf["sigma"][0]), _p(buf["wsn0"][0]), second(buf["wsn1"]), cout, k0, k1, iterate,
           _p(buf["wsf"][0]) if nf else None, nf, HF._stream())
    codes = (ctypes.c_int * 4)()
    assert lib.agan_spectral_last_launch(codes, 4) == 4 and codes[0] == form_of(case), list(codes)
    ub, vb = (buf["u"][0], buf["v"][0]) if iterate else (ud[0], vd[0])
    L.call("agan_spectral_bwd", _p(d[0][0]), second(d[-1]), _p(buf["wsn0"][0]), second(buf["wsn1"]), _p(ub), _p(vb), _p(buf["sigma"][0]),
           _p(buf["dw0"][0]), second(buf["dw1"]), cout, k0, k1, accumulate, accumulate, _p(buf["wsb"][0]) if nb else None, nb, HF._stream())
    assert lib.agan_spectral_last_launch(codes, 4) == 4 and codes[3] == form_of(case), list(codes)
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert tail_ok(buf[k][1], n, shift if k[:-1] in ("wsn", "dw") else 0), f"{name}: guard around `{k}` overwritten"
    for s, t in enumerate(w):
        assert same_bits(t[0].cpu(), seg(W, s).reshape(-1)) and tail_ok(t[1], t[0].numel(), shift), "W modified"
    assert same_bits(ud[0].cpu(), u0) and same_bits(vd[0].cpu(), v0), "the state was written by the kernels"
    got = {k: buf[k][0].cpu() for k in ("sigma", "wsn0", "wsn1", "dw0", "dw1")}
    got["u"], got["v"] = ub.cpu(), vb.cpu()
    if not iterate:                                                    # u_out / v_out are not written in eval mode
        assert bool((buf["u"][0].view(torch.int32) == SENT).all()) and bool((buf["v"][0].view(torch.int32) == SENT).all())
    return got


def check(case, iterate, accumulate, shift=0):
    name, cout, k0, k1 = case
    got = hip(case, iterate, accumulate, shift)
    again = hip(case, iterate, accumulate, shift)
    for k in got:
        assert same_bits(got[k], again[k]), f"{name}: `{k}` differs between two runs"
        assert not bool(torch.isnan(got[k]).any()), f"{name}: NaN in `{k}` (a sentinel left, or the poisoned workspace read)"
    r32, r64 = references(case, iterate)
    tag = f"{name}/it{iterate}/acc{accumulate}" + (f"/shift{shift}" if shift else "")
    if iterate:
        check_slices(tag, "u'", got["u"].view(1, -1), r32[0].view(1, -1), r64[0].view(1, -1))
        check_slices(tag, "v", got["v"].view(1, -1), r32[1].view(1, -1), r64[1].view(1, -1))
    check_slices(tag, "sigma", got["sigma"].view(1, 1), r32[2].view(1, 1), r64[2].view(1, 1))
    wsn = torch.cat([got["wsn0"].view(cout, k0), got["wsn1"].view(cout, k1)], dim=1)
    check_slices(tag, "W_sn/row", wsn, r32[3], r64[3])
    dw = torch.cat([got["dw0"].view(cout, k0), got["dw1"].view(cout, k1)], dim=1)
    _, _, _, dWsn, prior = case_inputs(case)
    if name == "one":
        lim = 8 * U * float(dWsn.abs().max()) / float(r64[2]) + (U * float(dw.abs().max()) if accumulate else 0.0)
        err = float((dw - (prior if accumulate else 0)).abs().max())
        print(f"SPECTRAL-ERR | {tag} | dW (zero in exact arithmetic) | |dW| {err:.2e} | limit {lim:.2e}")
        assert err <= lim
        return
    if accumulate:
        check_slices(tag, "prior + dW/row", dw, prior + r32[4], prior.double() + r64[4])
    else:
        check_slices(tag, "dW/row", dw, r32[4], r64[4])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("iterate", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_spectral_per_slice_against_float64(case, iterate, accumulate):
    check(case, iterate, accumulate)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("first", "joint", "mid", "joint_big")], ids=lambda c: c[0])
def test_bases_off_a_16_byte_boundary(case):
    """the flat optimiser aligns parameters, but nothing in the C ABI asks for it: weights, outputs and gradients 4 bytes off"""
    check(case, 1, 1, shift=1)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("first", "joint", "mid", "joint_big")], ids=lambda c: c[0])
def test_outputs_may_be_the_state_itself(case):
    """include/agan.h: with iterate = 1, u_out and v_out may be u and v -- the state stored back in place; same bits as into fresh buffers"""
    lib = L.load()
    name, cout, k0, k1 = case
    W, u0, v0, _, _ = case_inputs(case)
    want = hip(case, 1, 0)
    w0, _ = dev(W[:, :k0].contiguous())
    w1 = dev(W[:, k0:].contiguous())[0] if k1 else None
    (u, uw), (v, vw) = dev(u0), dev(v0)
    nf = lib.agan_spectral_fwd_ws_bytes(cout, k0, k1)
    (sigma, _), (o0, _), (o1, _), (ws, _) = poisoned(1), poisoned(cout * k0), poisoned(cout * k1), poisoned(nf // 4)
    L.call("agan_spectral_fwd", _p(w0), _p(w1), _p(u), _p(v), _p(u), _p(v), _p(sigma), _p(o0), _p(o1) if k1 else None, cout, k0, k1, 1,
           _p(ws) if nf else None, nf, HF._stream())
    torch.cuda.synchronize()
    assert tail_ok(uw, cout) and tail_ok(vw, k0 + k1)
    for k, t in (("u", u), ("v", v), ("sigma", sigma), ("wsn0", o0), ("wsn1", o1)):
        assert same_bits(t.cpu(), want[k]), f"{name}: `{k}` in place differs from `{k}` into a fresh buffer"


def test_both_forms_are_reached():
    assert {form_of(c) for c in CASES} == {FORM_SMALL, FORM_BIG}
    assert form_of(CASES[CASE_IDS.index("seam_lo")]) == FORM_SMALL and form_of(CASES[CASE_IDS.index("seam_hi")]) == FORM_BIG


def test_refusals_come_before_any_launch():
    """every refusal of the domain on the return code, with the entry's name in the message; nothing was enqueued (the sentinels stay)"""
    lib = L.load()
    out, whole = poisoned(64)
    p = _p(out)
    n = 1 << 20
    fwd = lambda cout, k0, k1, it=1, w1=p, ws=p, nbytes=n, v=p, uo=p, w0=p: lib.agan_spectral_fwd(w0, w1, p, v, uo, p, p, p, w1, cout, k0, k1, it, ws,
                                                                                                   nbytes, HF._stream())
    bwd = lambda cout, k0, k1, d1=p, ws=p, nbytes=n, d0=p: lib.agan_spectral_bwd(d0, d1, p, d1, p, p, p, p, d1, cout, k0, k1, 0, 1, ws, nbytes,
                                                                                   HF._stream())
    for shape in ((0, 4, 0), (4, 0, 0), (4, 4, -1), (-3, 4, 0), (1 << 16, 1 << 15, 0), (1 << 15, 1 << 15, 1 << 15)):
        assert fwd(*shape) == L.EINVAL and b"spectral_fwd" in lib.agan_last_error()
        assert bwd(*shape) == L.EINVAL and b"spectral_bwd" in lib.agan_last_error()
        assert lib.agan_spectral_fwd_ws_bytes(*shape) == 0 and lib.agan_spectral_bwd_ws_bytes(*shape) == 0
    assert fwd(2, 4, 0, it=2) == L.EINVAL and fwd(2, 4, 0, it=-1) == L.EINVAL
    assert fwd(2, 4, 0, w0=None) == L.EINVAL and fwd(2, 4, 4, w1=None) == L.EINVAL and fwd(2, 4, 0, uo=None) == L.EINVAL
    assert fwd(2, 4, 0, it=0, v=None) == L.EINVAL
    assert bwd(2, 4, 0, d0=None) == L.EINVAL and bwd(2, 4, 4, d1=None) == L.EINVAL
    nf, nb = lib.agan_spectral_fwd_ws_bytes(64, 129, 0), lib.agan_spectral_bwd_ws_bytes(64, 129, 0)
    assert fwd(64, 129, 0, nbytes=nf - 1) == L.EWORKSPACE and fwd(64, 129, 0, ws=None, nbytes=nf) == L.EWORKSPACE
    assert bwd(64, 129, 0, nbytes=nb - 1) == L.EWORKSPACE and bwd(64, 129, 0, ws=None, nbytes=nb) == L.EWORKSPACE
    torch.cuda.synchronize()
    assert bool((whole.view(torch.int32) == SENT).all())


def test_functional_spectral_weight_matches_its_reference():
    """backend.functional.spectral_weight: autograd wiring, the state written back, two forwards before one backward, eval mode"""
    case = ("fn", 24, 72, 40)
    W, u0, v0, dW, _ = case_inputs(case)
    k0 = 72

    def run(fn, dtype, dev_):
        w0 = W[:, :k0].reshape(24, 8, 3, 3).to(dtype).to(dev_).requires_grad_(True)
        w1 = W[:, k0:].reshape(24 * 8, 5).to(dtype).to(dev_).requires_grad_(True)
        u, v = u0.to(dtype).to(dev_), v0.to(dtype).to(dev_)
        a0, a1 = fn(w0, u, v, True, second=w1)
        b0, b1 = fn(w0, u, v, True, second=w1)                          # moves u and v again before a's backward
        d0, d1 = dW[:, :k0].reshape(a0.shape).to(dtype).to(dev_), dW[:, k0:].reshape(a1.shape).to(dtype).to(dev_)
        ((a0 * d0).sum() + (a1 * d1).sum() + 2 * (b0 * d0).sum() - (b1 * d1).sum()).backward()
        with torch.no_grad():
            e0, e1 = fn(w0, u, v, False, second=w1)
        return [t.detach().double().cpu().reshape(24, -1) for t in (a0, a1, b0, b1, e0, e1, w0.grad, w1.grad)] + [u.double().cpu(), v.double().cpu()]
    got = run(HF.spectral_weight, torch.float32, DEV)
    want = run(HF.spectral_weight_reference, torch.float64, "cpu")
    for a, b, what in zip(got, want, ("a0", "a1", "b0", "b1", "eval0", "eval1", "dw0", "dw1", "u", "v")):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"functional {what}: rel err {err:.2e}")
        assert a.shape == b.shape and err <= 1e-5, what
