"""Shared by the word-level discriminator's tests: the shape cases of the C-ABI test, their inputs, and the per-slice error measure of
tests/test_gpu_damsm.py, restated (nothing here touches a device)."""
import torch

from helpers import RTOL

U = 2.0 ** -24
FLOOR = 64 * U                 # a 320-term sum in another order says more than the fp32 reference's luck in a small case
CEILING = RTOL / 10            # no per-slice bound above this, whatever the yardstick says
FACTOR = 8.0
GAMMA1, GAMMA2, EPS = 4.0, 5.0, 1e-8

# name, B, D, S, T.  csrc/word_corr.hip has one dispatch seam, T = 16 | 17 (one or two 16-word column tiles): D257 and T16 sit on its
# low side, S290 and T17 on its high side; S15 | S16 and S289 | S290 are the seams of damsm.hip's pair kernels, kept as cases although
# this kernel has one form over S; D257 is not a multiple of the k step of 4 nor of a 16-row tile.
CASES = [
    ("tiny", 2, 7, 1, 1),
    ("S15", 3, 64, 15, 12),
    ("S16", 3, 64, 16, 13),
    ("S289", 4, 256, 289, 18),
    ("S290", 2, 96, 290, 17),
    ("D257", 2, 257, 40, 16),
    ("limits", 3, 320, 320, 32),
    ("B128", 128, 32, 20, 5),
    ("T16", 2, 33, 21, 16),
    ("T17", 2, 33, 21, 17),
]
CASE_IDS = [c[0] for c in CASES]


def case_inputs(case, seed=0):
    """regions [B, D, S], words [B, D, T] with N(0, D^-1/2) entries (standard normals times D ** -0.25: m has unit variance, the
    softmaxes are unsaturated), lens random in [1, T] with lens[0] = T and lens[-1] = 1, dp random; all fp32 / int64 on the CPU"""
    _, B, D, S, T = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + D + S + T)
    regions = torch.randn(B, D, S, generator=g) * D ** -0.25
    words = torch.randn(B, D, T, generator=g) * D ** -0.25
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0], lens[-1] = T, 1
    dp = torch.randn(B, generator=g)
    return regions, words, lens, dp


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
    print(f"WORD-CORR-ERR | {case} | {what} | err {worst:.2e} | e_ref {e_ref:.2e} | err/e_ref {worst / e_ref if e_ref else float('inf'):.2f} | bound {b:.2e}")
    bad = ~(e <= b)
    if bool(bad.any()):
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{case} {what}: {int(bad.sum())} of {e.numel()} slices outside {b:.2e} (fp32 reference {e_ref:.2e}); first slice {i}: "
                             f"err {float(e[i]):.3e}, max|f64| {float(r64[i].abs().max()):.3e}, max|got| {float(got[i].abs().max()):.3e}")
    return worst, e_ref
