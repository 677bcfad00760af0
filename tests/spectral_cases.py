"""Shared by the spectral-normalisation tests: the shape cases of the C-ABI test, their inputs, and the per-slice error measure of
tests/word_corr_cases.py, restated (nothing here touches a device)."""
import torch

from helpers import RTOL

U = 2.0 ** -24
FLOOR = 64 * U                 # a sum of a few thousand terms in another order says more than the fp32 reference's luck in a small case
CEILING = RTOL / 10            # no per-slice bound above this, whatever the yardstick says
FACTOR = 8.0
EPS = 1e-12

# name, Cout, K0, K1.  csrc/spectral.hip has ONE dispatch seam, by size alone: Cout * (K0 + K1) <= 8192 runs one workgroup and one launch
# per direction ("small"), anything above the three + two launch form ("big").  `seam_lo` (64 x 128 = 8192) is the last small shape,
# `seam_hi` (64 x 129, an odd K as well) the first big one.  Inside the big form a segment takes 16-byte loads along its rows where its K
# is a multiple of 4 and a lane-per-column form otherwise: `wide`, `mid`, `big`, `joint_big` are aligned, `seam_hi` and `joint_big_odd` are
# not, `joint_mixed` has one segment of each kind; `strips` has more than one 256-column strip and 1024-column chunk per segment, partly
# filled, and more rows than one row block.
CASES = [
    ("one", 1, 1, 0),
    ("head", 1, 128, 0),
    ("first", 8, 48, 0),
    ("odd", 7, 45, 0),
    ("tall", 300, 20, 0),
    ("wide", 5, 4100, 0),
    ("joint", 16, 144, 288),
    ("joint_odd", 6, 54, 27),
    ("mid", 192, 1100, 0),
    ("big", 512, 2048, 0),
    ("seam_lo", 64, 128, 0),
    ("seam_hi", 64, 129, 0),
    ("joint_big", 40, 360, 72),
    ("joint_big_odd", 33, 297, 99),
    ("joint_mixed", 32, 288, 45),
    ("strips", 70, 1300, 1030),
]
CASE_IDS = [c[0] for c in CASES]
SMALL_ELEMS = 8192
FORM_SMALL, FORM_BIG = 1, 2


def form_of(case):
    _, cout, k0, k1 = case
    return FORM_SMALL if cout * (k0 + k1) <= SMALL_ELEMS else FORM_BIG


def case_inputs(case, seed=0):
    """W ~ N(0, K^-1/2) as two segments [Cout, K0], [Cout, K1] (sigma is O(1)), u0 a normalised normal vector, dW_sn ~ N(0, 1) as two
    segments, a random prior gradient as two segments; all fp32 on the CPU"""
    _, cout, k0, k1 = case
    K = k0 + k1
    g = torch.Generator().manual_seed(1000 * seed + 7 * cout + k0 + 3 * k1)
    W = torch.randn(cout, K, generator=g) * K ** -0.5
    u0 = torch.nn.functional.normalize(torch.randn(cout, generator=g), dim=0, eps=EPS)
    v0 = torch.nn.functional.normalize(torch.randn(K, generator=g), dim=0, eps=EPS)
    dW = torch.randn(cout, K, generator=g)
    prior = torch.randn(cout, K, generator=g)
    return W, u0, v0, dW, prior


def slice_errs(x, ref):
    """x, ref [N, K] float64.  err(slice) = max|x - ref| / max|ref| over the slice; a slice whose reference is all exactly 0 has
    err 0 if x is all exactly 0 there and inf otherwise.  Returns (err [N], zero-slice mask [N])."""
    x, ref = x.double(), ref.double()
    num, den = (x - ref).abs().amax(1), ref.abs().amax(1)
    zero = den == 0
    exact = x.abs().amax(1) == 0                       # (NaN compares false)
    inf, nil = torch.full_like(num, float("inf")), torch.zeros_like(num)
    return torch.where(zero, torch.where(exact, nil, inf), num / den.clamp(min=1e-300)), zero


def bound_for(e_ref, factor=FACTOR):
    return min(max(factor * e_ref, FLOOR), CEILING)


def check_slices(case, what, got, r32, r64):
    """every slice (row) of `got` within max(8 e_ref, 64 * 2^-24), at most RTOL / 10, of the float64 reference, e_ref being the worst
    slice of the fp32 reference on the same inputs.  Prints the figures first; returns (err, e_ref)."""
    got, r32, r64 = (t.detach().double().cpu() for t in (got, r32, r64))
    assert got.shape == r64.shape == r32.shape and got.dim() == 2, (what, got.shape, r64.shape)
    e, _ = slice_errs(got, r64)
    er, zero = slice_errs(r32, r64)
    er = torch.where(zero, torch.zeros_like(er), er)
    e_ref = float(er.max())
    b = bound_for(e_ref)
    worst = float(e.max()) if not bool(torch.isnan(e).any()) else float("nan")
    print(f"SPECTRAL-ERR | {case} | {what} | err {worst:.2e} | e_ref {e_ref:.2e} | err/e_ref {worst / e_ref if e_ref else float('inf'):.2f} | bound {b:.2e}")
    bad = ~(e <= b)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{case} {what}: {int(bad.sum())} of {e.numel()} slices outside {b:.2e} (fp32 reference {e_ref:.2e}); first slice {i}: "
                             f"err {float(e[i]):.3e}, max|f64| {float(r64[i].abs().max()):.3e}, max|got| {float(got[i].abs().max()):.3e}")
    return worst, e_ref
