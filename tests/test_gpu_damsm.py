"""The DAMSM loss kernels (csrc/damsm.hip) through the C ABI, per slice against the float64 oracle, at their dispatch seams and limits.

What test_gpu_parity.py leaves open and this file closes: errors are measured PER SLICE (image, caption, (caption, word), row, batch
element, position) against the slice's own float64 maximum instead of the whole tensor's; the reference is the oracle in float64, with
the oracle in fp32 only as the yardstick of the bound; the upstream gradient, the gammas, lambda, labels and class ids vary; loss, sim,
attn_maps, save, dfeat, dwemb and the workspace start as NaN sentinels, are sized exactly and are followed by guard words; every case
sits on a dispatch seam or a limit of damsm.hip (pair_mfma_ok: S 15|16 and 289|290, D % 64, T 12|13; with_pair_form: D 256|257, T 16|17;
S = D = 320, T = L = 32; B = 127|128, where the cross-entropy kernel needs more than 64 KB of LDS); every run is repeated and must be
bit-identical (no atomics).

Bound: for each tensor of each case, e_ref = the worst slice of the fp32 oracle against the float64 oracle on the same inputs, and every
slice of the kernel's result must be within max(8 e_ref, 64 * 2^-24) of float64, never more than RTOL / 10 = 1e-4.  The factor 8 covers
what differs from the oracle by construction -- another summation order (5 waves, MFMA k-blocks of 4) and __expf in both softmaxes
(about |v| 2^-24 off for an argument v); the floor covers the small cases where the fp32 oracle happens to be nearly exact.  The loss is
held to 1e-5 of its float64 value.  A slice whose float64 values are all exactly 0 must be exactly 0.  No tensor needed a wider factor.

Measured on an MI355X: worst err / e_ref over the slices of each tensor ("0=0": float64 exactly 0 or e_ref = 0, and the kernel exact too).

  words loss             loss   sim    attn_maps  dfeat/image  dwemb/caption  dwemb/word
  mfma-S16               0.41   1.12   1.30       1.84         1.94           1.23
  rows-S15               1.00   0.93   1.11       1.40         1.23           0.64
  mfma-S289              1.00   1.30   1.04       0.79         1.15           1.12
  rows-S290              2.48   1.00   0.86       0.71         0.84           1.43
  mfma-D256              1.00   2.19   0.73       0.67         0.31           0.31
  rows16-D257-T13-S1     4.06   1.00   0=0        0.55         0.77           0.77
  rows32-D96-T17         1.00   0.50   1.00       0.86         0.43           0.59
  limits-D320-T32-S320   7.23   0.99   1.55       1.10         1.48           1.37
  hyper                  1.00   0.56   1.00       1.40         1.39           2.17
  all-masked-B2          0=0    7.58   0.81       0=0          0=0            0=0      (sim: err 1.3e-7, e_ref 1.7e-8)
  B1                     0=0    1.00   1.02       0=0          0=0            0=0
  B127                   1.77   1.08   1.34       2.09         0.69           0.96
  B128                   0.30   1.00   1.10       2.44         1.45           1.70
  (the loss column: err <= 1.3e-7 everywhere, against its own bound of 1e-5)

  sentence loss          loss   dS/row  dots/row  norms  dcnn/row  drnn/row
  B1                     0=0    0=0     80.3      1.45   0=0       0=0        (dots: err 9.0e-8, e_ref 1.1e-9; the floor is the bound)
  D1                     1.00   1.00    1.00      0=0    1.01      2.50       (gradient rows: see the test for their denominator)
  D63                    1.00   0.69    0.95      0.72   0.69      0.95
  D65                    1.00   1.43    0.69      1.00   0.95      1.05
  B24-hyper              9.96   0.85    0.25      0.77   1.15      1.28       (loss: err 9.2e-8, e_ref 9.2e-9)
  B127                   1.00   0.91    0.30      0.89   0.96      0.81
  B128-D1000             1.00   0.88    0.39      0.92   1.26      0.82
  clamp                  6.15   2.57    1.01      0.54   1.31      1.25       (loss: err 9.1e-8)

  func_attention         wctx/element  attn/position  dquery/element  dcontext/element
  limits                 0.92          1.19           1.79            2.13
  limits, dwctx only                                  1.95            2.30
  limits, dattn only                                  1.25            1.18
  ones                   0=0           0=0            0=0             0=0
  L16-S7 (gamma1 2.5)    1.14          1.49           1.04            1.61
  L17-S25                0.68          1.00           0.77            0.81

Every check prints its figures (`DAMSM-ERR | case | tensor | err | e_ref | err/e_ref | bound`, pytest -s) before it asserts.
"""
import ctypes
import importlib
import math

import pytest
import torch

from helpers import RTOL, probe
from oracle import attngan_oracle as O   # (checker only)

pytestmark = pytest.mark.gpu
DEV = "cuda"

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")

U = 2.0 ** -24
FLOOR = 64 * U                 # a 320-term sum in another order says more than the fp32 oracle's luck in a small case
CEILING = RTOL / 10            # no per-slice bound above this, whatever the yardstick says
LOSS_TOL = 1e-5
GUARD = 64
SENT = 0x7FC0DEAD
KMS = 292                      # damsm.hip: row length of the zero-padded feature copy the MFMA pair kernels read


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(t):
    """fp32 device copy followed by GUARD NaN-pattern sentinels; returns (view, whole)"""
    t = t.reshape(-1)
    whole = torch.empty(t.numel() + GUARD, dtype=torch.float32, device=DEV)
    whole.view(torch.int32).fill_(SENT)
    whole[:t.numel()].copy_(t.float())
    return whole[:t.numel()], whole


def poisoned(n):
    """n floats of the NaN sentinel pattern followed by GUARD more; returns (view, whole)"""
    whole = torch.empty(n + GUARD, dtype=torch.float32, device=DEV)
    whole.view(torch.int32).fill_(SENT)
    return whole[:n], whole


def tail_ok(whole, n):
    return bool((whole[n:].view(torch.int32) == SENT).all())


def is_sentinel(t):
    return t.contiguous().view(torch.int32) == SENT


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ the error measure
def slice_errs(x, ref):
    """x, ref [N, K] float64.  err(slice) = max|x - ref| / max|ref| over the slice; a slice whose reference is all exactly 0 has
    err 0 if x is all exactly 0 there and inf otherwise.  Returns (err [N], zero-slice mask [N])."""
    x, ref = x.double(), ref.double()
    num, den = (x - ref).abs().amax(1), ref.abs().amax(1)
    zero = den == 0
    exact = x.abs().amax(1) == 0                       # (NaN compares false)
    inf, nil = torch.full_like(num, float("inf")), torch.zeros_like(num)
    return torch.where(zero, torch.where(exact, nil, inf), num / den.clamp(min=1e-300)), zero


def bound_for(e_ref, factor=8.0):
    return min(max(factor * e_ref, FLOOR), CEILING)


def check_slices(case, what, got, r32, r64, factor=8.0, denom_floor=None, denom=None):
    """every slice of `got` within max(factor * e_ref, FLOOR) (at most CEILING) of the float64 reference, e_ref being the worst slice
    of the fp32 oracle on the same inputs.  denom_floor (sim): each slice is one scalar divided by max(|f64|, denom_floor);
    denom [N] (sentence gradients at D = 1 only, see there): the slices' denominators given instead of max|f64|."""
    got, r32, r64 = (t.detach().double().cpu() for t in (got, r32, r64))
    assert got.shape == r64.shape == r32.shape and got.dim() == 2, (what, got.shape, r64.shape)
    if got.numel() == 0:
        return
    if denom is not None:
        e, er = (got - r64).abs().amax(1) / denom, (r32 - r64).abs().amax(1) / denom
    elif denom_floor is None:
        e, _ = slice_errs(got, r64)
        er, zero = slice_errs(r32, r64)
        er = torch.where(zero, torch.zeros_like(er), er)
    else:
        den = r64.abs().clamp(min=denom_floor)
        e, er = ((got - r64).abs() / den).amax(1), ((r32 - r64).abs() / den).amax(1)
    e_ref = float(er.max())
    b = bound_for(e_ref, factor)
    worst = float(e.max()) if not bool(torch.isnan(e).any()) else float("nan")
    print(f"DAMSM-ERR | {case} | {what} | err {worst:.2e} | e_ref {e_ref:.2e} | err/e_ref {worst / e_ref if e_ref else float('inf'):.2f} | bound {b:.2e}")
    bad = ~(e <= b)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{case} {what}: {int(bad.sum())} of {e.numel()} slices outside {b:.2e} (fp32 oracle {e_ref:.2e}); first slice {i}: err {float(e[i]):.3e}, "
                             f"max|f64| {float(r64[i].abs().max()):.3e}, max|got| {float(got[i].abs().max()):.3e}")


def check_loss(case, got, r32, r64):
    got, r32, r64 = float(got), float(r32), float(r64)
    if r64 == 0.0:
        print(f"DAMSM-ERR | {case} | loss | got {got!r} | f64 exactly 0")
        assert got == 0.0, f"{case} loss: float64 gives exactly 0, got {got!r}"
        return
    e, er = abs(got - r64) / abs(r64), abs(r32 - r64) / abs(r64)
    print(f"DAMSM-ERR | {case} | loss | err {e:.2e} | e_ref {er:.2e} | err/e_ref {e / er if er else float('inf'):.2f} | bound {LOSS_TOL:.2e}")
    assert e <= LOSS_TOL, f"{case} loss: got {got!r}, float64 {r64!r}, rel err {e:.3e} > {LOSS_TOL:.0e}"


class SpyCE:
    """records the similarity matrix the oracle hands to its first cross-entropy (and keeps its gradient)"""

    def __enter__(self):
        self.s, self._orig = None, O._ce

        def spy(logits, labels):
            if self.s is None:
                self.s = logits
                if logits.requires_grad:
                    logits.retain_grad()
            return self._orig(logits, labels)
        O._ce = spy
        return self

    def __exit__(self, *exc):
        O._ce = self._orig
        return False


# --------------------------------------------------------------------------------------------------------------- words loss
def _wcase(name, B, D, T, grid, lens, **kw):
    c = dict(name=name, B=B, D=D, T=T, grid=grid, lens=list(lens), gammas=(4.0, 5.0, 10.0), lam=5.0, labels=None, cids=None, dloss=1.0)
    c.update(kw)
    assert len(c["lens"]) == B and all(1 <= v <= T for v in c["lens"])
    return c


L12 = [12, 3, 1, 7]
WORDS_CASES = [
    _wcase("mfma-S16", 4, 64, 12, (4, 4), L12),                         # MFMA path at its smallest S
    _wcase("rows-S15", 4, 64, 12, (3, 5), L12),                         # one region fewer: thread-per-row <12,256>
    _wcase("mfma-S289", 4, 64, 12, (17, 17), L12),                      # MFMA path at its largest S
    _wcase("rows-S290", 4, 64, 12, (10, 29), L12),                      # one more: thread-per-row
    _wcase("mfma-D256", 4, 256, 12, (17, 17), L12),                     # MFMA at its largest D and T: five waves of channel rows
    _wcase("rows16-D257-T13-S1", 4, 257, 13, (1, 1), [13, 12, 1, 7]),   # <16,320> form, one region
    _wcase("rows32-D96-T17", 4, 96, 17, (5, 5), [17, 16, 1, 9]),        # <32,320> form just past 16 words; D % 64 != 0
    _wcase("limits-D320-T32-S320", 4, 320, 32, (16, 20), [32, 17, 16, 1]),
    _wcase("hyper", 5, 128, 7, (4, 4), [7, 1, 3, 2, 7], gammas=(2.5, 3.0, 7.0), lam=1.5, labels=[1, 0, 3, 2, 4], cids=[3, 7, 3, 9, 7], dloss=-0.37),
    _wcase("all-masked-B2", 2, 64, 12, (17, 17), [12, 12], cids=[5, 5]),
    _wcase("B1", 1, 64, 5, (4, 4), [5]),
    _wcase("B127", 127, 64, 12, (4, 4), [1 + (7 * i) % 12 for i in range(127)], cids=[i % 50 for i in range(127)]),
    _wcase("B128", 128, 64, 3, (4, 4), [1 + (7 * i) % 3 for i in range(128)]),
]


def words_inputs(c, seed):
    g = torch.Generator().manual_seed(seed)
    S = c["grid"][0] * c["grid"][1]
    return torch.randn(c["B"], c["D"], S, generator=g), torch.randn(c["B"], c["D"], c["T"], generator=g)


def words_oracle(c, feat, wemb, dtype):
    B, D = c["B"], c["D"]
    f = feat.to(dtype).view(B, D, *c["grid"]).clone().requires_grad_(True)
    w = wemb.to(dtype).clone().requires_grad_(True)
    labels = torch.arange(B) if c["labels"] is None else torch.tensor(c["labels"])
    with SpyCE() as spy:
        loss, maps = O.words_loss(f, w, labels, c["lens"], c["cids"], *c["gammas"], c["lam"])
    (loss * c["dloss"]).backward()
    return dict(loss=loss.detach(), sim=spy.s.detach(), maps=[m.detach().reshape(m.shape[1], -1) for m in maps],
                dfeat=f.grad.reshape(B, D, -1), dwemb=w.grad)


def words_hip(c, feat, wemb):
    """one forward + backward through the C ABI on freshly poisoned buffers; everything documented comes back on the CPU"""
    lib = L.load()
    B, D, T = c["B"], c["D"], c["T"]
    S = c["grid"][0] * c["grid"][1]
    fd, _ = dev(feat)
    wd, _ = dev(wemb)
    lens = torch.tensor(c["lens"], dtype=torch.int64, device=DEV)
    cids = None if c["cids"] is None else torch.tensor(c["cids"], dtype=torch.int64, device=DEV)
    labels = None if c["labels"] is None else torch.tensor(c["labels"], dtype=torch.int64, device=DEV)
    n_save, ws_bytes = lib.agan_words_loss_save_elems(B, D, T, S), lib.agan_words_loss_bwd_ws_bytes(B, D, T, S)
    assert n_save >= B * B + B * D * S and ws_bytes == B * B * D * (S + T) * 4
    sizes = dict(loss=1, sim=B * B, maps=B * T * S, save=n_save, dfeat=B * D * S, dwemb=B * D * T, ws=ws_bytes // 4)
    buf = {k: poisoned(n) for k, n in sizes.items()}
    dl = torch.tensor([c["dloss"]], dtype=torch.float32, device=DEV)
    g1, g2, g3 = c["gammas"]
    L.call("agan_words_loss_fwd", _p(fd), _p(wd), _p(lens), _p(cids), _p(labels), g1, g2, g3, c["lam"], _p(buf["loss"][0]), _p(buf["sim"][0]),
           _p(buf["maps"][0]), _p(buf["save"][0]), B, D, T, S, HF._stream())
    L.call("agan_words_loss_bwd", _p(fd), _p(wd), _p(lens), _p(buf["save"][0]), _p(dl), g1, g2, g3, c["lam"], _p(buf["dfeat"][0]),
           _p(buf["dwemb"][0]), B, D, T, S, _p(buf["ws"][0]), ws_bytes, HF._stream())
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert tail_ok(buf[k][1], n), f"{c['name']}: guard after `{k}` overwritten"
    assert same_bits(fd.cpu(), feat.reshape(-1)) and same_bits(wd.cpu(), wemb.reshape(-1)), "inputs modified"
    out = {k: buf[k][0].cpu() for k in sizes if k != "ws"}
    out["n_save"] = n_save
    return out


@pytest.mark.parametrize("c", WORDS_CASES, ids=[c["name"] for c in WORDS_CASES])
def test_words_loss_vs_float64(c):
    """agan_words_loss_fwd / _bwd on NaN-poisoned loss, sim, attn_maps, save, dfeat, dwemb and ws (each sized exactly, each followed by a
    guard): loss within 1e-5 of float64; sim per entry, attn_maps per (caption, word), dfeat per image, dwemb per caption and per
    (caption, word) within max(8 e_ref, 64 u) of float64 (e_ref: the fp32 oracle's worst slice on the same inputs); -inf in sim exactly
    on the class mask; the feature copies in `save` exact; padded words: dwemb exactly 0, attn_maps rows not written (include/agan.h);
    a second run on fresh poison bit-identical."""
    name, B, D, T = c["name"], c["B"], c["D"], c["T"]
    S = c["grid"][0] * c["grid"][1]
    lens = c["lens"]
    feat, wemb = words_inputs(c, 1000 + WORDS_CASES.index(c))
    r64, r32 = words_oracle(c, feat, wemb, torch.float64), words_oracle(c, feat, wemb, torch.float32)
    got = words_hip(c, feat, wemb)
    again = words_hip(c, feat, wemb)
    for k in ("loss", "sim", "maps", "save", "dfeat", "dwemb"):
        assert same_bits(got[k], again[k]), f"{name}: `{k}` differs between two runs on the same inputs"

    check_loss(name, got["loss"][0], r32["loss"], r64["loss"])
    # sim [image][caption]: -inf exactly on the class mask, finite elsewhere
    sim = got["sim"].view(B, B)
    mask = torch.zeros(B, B, dtype=torch.bool)
    if c["cids"] is not None:
        ids = torch.tensor(c["cids"])
        mask = (ids.view(-1, 1) == ids.view(1, -1)) & ~torch.eye(B, dtype=torch.bool)
    assert torch.equal(mask, torch.isinf(r64["sim"])), "the oracle's own mask"
    assert bool((sim[mask] == float("-inf")).all()) and bool(torch.isfinite(sim[~mask]).all()), f"{name}: sim mask"
    check_slices(name, "sim", sim[~mask].view(-1, 1), r32["sim"][~mask].view(-1, 1), r64["sim"][~mask].view(-1, 1), denom_floor=1.0)
    # attention maps of caption i against image i: words < lens[i] compared, the other rows left as the caller filled them
    maps = got["maps"].view(B, T, S)
    for i in range(B):
        assert bool(is_sentinel(maps[i, lens[i]:]).all()), f"{name}: attn_maps rows >= lens[{i}] were written"
    pick = lambda ms: torch.cat(list(ms), 0)
    check_slices(name, "attn_maps", pick(maps[i, :lens[i]] for i in range(B)), pick(r32["maps"]), pick(r64["maps"]))
    # save: dS [B*B], then the features transposed to [B][S][D], then (MFMA form) zero-padded to [B][D][KMS]
    save = got["save"]
    assert bool(torch.isfinite(save[:B * B]).all()), f"{name}: dS section of save"
    assert same_bits(save[B * B:B * B + B * D * S].view(B, S, D), feat.transpose(1, 2)), f"{name}: transposed features in save"
    if got["n_save"] != B * B + B * D * S:
        assert got["n_save"] == B * B + B * D * S + B * D * KMS
        padded = torch.zeros(B, D, KMS)
        padded[:, :, :S] = feat
        assert same_bits(save[B * B + B * D * S:].view(B, D, KMS), padded), f"{name}: padded features in save"
    # gradients
    dfeat, dwemb = got["dfeat"].view(B, D, S), got["dwemb"].view(B, D, T)
    for i in range(B):
        assert bool((dwemb[i, :, lens[i]:] == 0).all()), f"{name}: dwemb of caption {i} beyond its {lens[i]} words"
    check_slices(name, "dfeat/image", dfeat.reshape(B, -1), r32["dfeat"].reshape(B, -1), r64["dfeat"].reshape(B, -1))
    check_slices(name, "dwemb/caption", dwemb.reshape(B, -1), r32["dwemb"].reshape(B, -1), r64["dwemb"].reshape(B, -1))
    cols = lambda t: pick(t[i, :, :lens[i]].t() for i in range(B))
    check_slices(name, "dwemb/word", cols(dwemb), cols(r32["dwemb"]), cols(r64["dwemb"]))


# ------------------------------------------------------------------------------------------------------------ sentence loss
def _scase(name, B, D, **kw):
    c = dict(name=name, B=B, D=D, gamma3=10.0, lam=5.0, labels=None, cids=None, dloss=1.0, cnn_scale=None, rnn_scale=None)
    c.update(kw)
    return c


EPS = 1e-8
SENT_CASES = [
    _scase("B1", 1, 64), _scase("D1", 5, 1), _scase("D63", 5, 63), _scase("D65", 5, 65),
    _scase("B24-hyper", 24, 256, gamma3=7.0, lam=1.5, dloss=-0.37, cids=[i % 9 for i in range(24)], labels=[(i + 1) % 24 for i in range(24)]),
    _scase("B127", 127, 256), _scase("B128-D1000", 128, 1000),
    # |c| |r| is about 64 (scales 1, 1), 6.4e-5 (1, 1e-6) -- both far above eps -- or 6.4e-11 (1e-6, 1e-6) / exactly 0 -- far below:
    # the clamp branch of both kernels, with one all-zero row on each side (torch's norm and clamp sub-gradients are the reference)
    _scase("clamp", 6, 64, cnn_scale=[1.0, 1e-6, 1.0, 0.0, 1e-6, 1.0], rnn_scale=[1e-6, 1.0, 0.0, 1.0, 1e-6, 1.0]),
]


def sent_inputs(c, seed):
    g = torch.Generator().manual_seed(seed)
    cnn, rnn = torch.randn(c["B"], c["D"], generator=g), torch.randn(c["B"], c["D"], generator=g)
    if c["cnn_scale"] is not None:
        cnn, rnn = cnn * torch.tensor(c["cnn_scale"]).view(-1, 1), rnn * torch.tensor(c["rnn_scale"]).view(-1, 1)
    return cnn, rnn


def sent_oracle(c, cnn, rnn, dtype):
    B = c["B"]
    a, b = cnn.to(dtype).clone().requires_grad_(True), rnn.to(dtype).clone().requires_grad_(True)
    labels = torch.arange(B) if c["labels"] is None else torch.tensor(c["labels"])
    with SpyCE() as spy:
        loss = O.sentence_loss(a, b, labels, c["cids"], c["gamma3"], c["lam"], EPS)
    (loss * c["dloss"]).backward()
    with torch.no_grad():
        dots, norms = a @ b.t(), torch.cat([a.norm(2, 1), b.norm(2, 1)])
    return dict(loss=loss.detach(), dS=spy.s.grad / c["dloss"], dots=dots, norms=norms, dcnn=a.grad, drnn=b.grad)


@pytest.mark.parametrize("c", SENT_CASES, ids=[c["name"] for c in SENT_CASES])
def test_sentence_loss_vs_float64(c):
    """agan_sent_loss_fwd / _bwd on poisoned buffers: loss within 1e-5; the dS and dots rows and the norms of `save`, dcnn and drnn per
    row within max(8 e_ref, 64 u) of float64 (all-zero reference rows exactly 0); two runs bit-identical"""
    name, B, D = c["name"], c["B"], c["D"]
    cnn, rnn = sent_inputs(c, 2000 + SENT_CASES.index(c))
    r64, r32 = sent_oracle(c, cnn, rnn, torch.float64), sent_oracle(c, cnn, rnn, torch.float32)
    cids = None if c["cids"] is None else torch.tensor(c["cids"], dtype=torch.int64, device=DEV)
    labels = None if c["labels"] is None else torch.tensor(c["labels"], dtype=torch.int64, device=DEV)
    dl = torch.tensor([c["dloss"]], dtype=torch.float32, device=DEV)
    cd, _ = dev(cnn)
    rd, _ = dev(rnn)
    sizes = dict(loss=1, save=2 * B * B + 2 * B, dcnn=B * D, drnn=B * D)
    runs = []
    for _ in range(2):
        buf = {k: poisoned(n) for k, n in sizes.items()}
        L.call("agan_sent_loss_fwd", _p(cd), _p(rd), _p(cids), _p(labels), c["gamma3"], c["lam"], EPS, _p(buf["loss"][0]), _p(buf["save"][0]),
               B, D, HF._stream())
        L.call("agan_sent_loss_bwd", _p(cd), _p(rd), _p(buf["save"][0]), _p(dl), c["gamma3"], c["lam"], EPS, _p(buf["dcnn"][0]),
               _p(buf["drnn"][0]), B, D, HF._stream())
        torch.cuda.synchronize()
        for k, n in sizes.items():
            assert tail_ok(buf[k][1], n), f"{name}: guard after `{k}` overwritten"
        runs.append({k: buf[k][0].cpu() for k in sizes})
    got, again = runs
    for k in sizes:
        assert same_bits(got[k], again[k]), f"{name}: `{k}` differs between two runs on the same inputs"
    check_loss(name, got["loss"][0], r32["loss"], r64["loss"])
    save = got["save"]
    check_slices(name, "dS/row", save[:B * B].view(B, B), r32["dS"], r64["dS"])
    check_slices(name, "dots/row", save[B * B:2 * B * B].view(B, B), r32["dots"], r64["dots"])
    check_slices(name, "norms", save[2 * B * B:].view(-1, 1), r32["norms"].view(-1, 1), r64["norms"].view(-1, 1))
    dc_den = dr_den = None
    if D == 1:
        # the cosine of two scalars is +-1, locally constant: every gradient row is EXACTLY 0 in exact arithmetic, and what float64
        # returns (1e-15) is the rounding residue of sum_i g_ji (r_i / (|c_j| |r_i|) - <c_j, r_i> c_j |r_i| / (|c_j|^3 |r_i|)), two terms
        # that cancel.  max|f64| of such a row is no scale (the fp32 oracle itself is 2.4e9 "off" on it, measured), so here -- and only
        # here -- the row's denominator is the size of the terms that cancel, sum_i |g_ji| |r_i| / (|c_j| |r_i|), from float64.
        a, b = cnn.double(), rnn.double()
        k = (r64["dS"] * c["dloss"]).abs() * c["gamma3"] / (a.norm(2, 1).view(-1, 1) * b.norm(2, 1).view(1, -1)).clamp(min=EPS)
        dc_den, dr_den = (k @ b.abs()).amax(1), (k.t() @ a.abs()).amax(1)
    check_slices(name, "dcnn/row", got["dcnn"].view(B, D), r32["dcnn"], r64["dcnn"], denom=dc_den)
    check_slices(name, "drnn/row", got["drnn"].view(B, D), r32["drnn"], r64["drnn"], denom=dr_den)


# ----------------------------------------------------------------------------------------------------------- func_attention
ATTN_CASES = [("limits", 2, 320, 32, (16, 20), 4.0), ("ones", 2, 1, 1, (1, 1), 4.0), ("L16-S7", 3, 33, 16, (1, 7), 2.5), ("L17-S25", 3, 33, 17, (5, 5), 4.0)]


def attn_oracle(q, ctx, gamma1, dtype, use_w, use_a):
    q, ctx = q.to(dtype).clone().requires_grad_(True), ctx.to(dtype).clone().requires_grad_(True)
    w, a = O.func_attention(q, ctx, gamma1)
    t = 0.0
    if use_w:
        t = t + (w * probe(w.shape, 0.3).to(dtype)).sum()
    if use_a:
        t = t + (a * probe(a.shape, 0.4).to(dtype)).sum()
    t.backward()
    return dict(wctx=w.detach(), attn=a.detach().reshape(a.shape[0], a.shape[1], -1), dquery=q.grad, dcontext=ctx.grad.reshape(*q.shape[:2], -1))


@pytest.mark.parametrize("name,B,D,Lq,grid,gamma1", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_func_attention_vs_float64(name, B, D, Lq, grid, gamma1):
    """agan_func_attention_fwd / _bwd: wctx, dquery and dcontext per batch element, attn per (batch element, position), within
    max(8 e_ref, 64 u) of float64; upstream gradients are the probe weights, both together and (at the limits) each alone with the
    other pointer NULL"""
    S = grid[0] * grid[1]
    g = torch.Generator().manual_seed(3000 + B * 1000 + D + Lq)
    q, ctx = torch.randn(B, D, Lq, generator=g), torch.randn(B, D, *grid, generator=g)
    qd, _ = dev(q)
    xd, _ = dev(ctx)
    scale = 1.0 / math.sqrt(D)
    fwd = dict(wctx=B * D * Lq, attn=B * Lq * S)
    fb = {k: poisoned(n) for k, n in fwd.items()}
    L.call("agan_func_attention_fwd", _p(qd), _p(xd), gamma1, scale, _p(fb["wctx"][0]), _p(fb["attn"][0]), B, D, Lq, S, HF._stream())
    torch.cuda.synchronize()
    for k, n in fwd.items():
        assert tail_ok(fb[k][1], n), f"{name}: guard after `{k}` overwritten"
    dw, _ = dev(probe((B, D, Lq), 0.3))
    da, _ = dev(probe((B, Lq, *grid), 0.4))
    first = True
    for use_w, use_a in [(True, True)] + ([(True, False), (False, True)] if name == "limits" else []):
        tag = name + ("" if use_w and use_a else "-dwctx-only" if use_w else "-dattn-only")
        r64, r32 = attn_oracle(q, ctx, gamma1, torch.float64, use_w, use_a), attn_oracle(q, ctx, gamma1, torch.float32, use_w, use_a)
        if first:
            check_slices(tag, "wctx/element", fb["wctx"][0].view(B, -1), r32["wctx"].reshape(B, -1), r64["wctx"].reshape(B, -1))
            check_slices(tag, "attn/position", fb["attn"][0].view(B * Lq, S), r32["attn"].reshape(B * Lq, S), r64["attn"].reshape(B * Lq, S))
            first = False
        bwd = dict(dquery=B * D * Lq, dcontext=B * D * S)
        bb = {k: poisoned(n) for k, n in bwd.items()}
        L.call("agan_func_attention_bwd", _p(qd), _p(xd), _p(dw if use_w else None), _p(da if use_a else None), gamma1, scale,
               _p(bb["dquery"][0]), _p(bb["dcontext"][0]), B, D, Lq, S, HF._stream())
        torch.cuda.synchronize()
        for k, n in bwd.items():
            assert tail_ok(bb[k][1], n), f"{tag}: guard after `{k}` overwritten"
        check_slices(tag, "dquery/element", bb["dquery"][0].view(B, -1), r32["dquery"].reshape(B, -1), r64["dquery"].reshape(B, -1))
        check_slices(tag, "dcontext/element", bb["dcontext"][0].view(B, -1), r32["dcontext"].reshape(B, -1), r64["dcontext"].reshape(B, -1))
