"""agan_kmeans_assign / agan_kmeans_update (csrc/kmeans.hip) and data.captions.kmeans on the GPU against a float64 restatement.

Shapes: the cross of N, D and K below with K <= N -- tails in all three dimensions, both load paths of the assignment (D % 4 == 0 moves
16 bytes per lane, any other D 4), both tilings (K <= 32: one chunk of 32 centroids; above: chunks of 128) with the sizes around each
boundary, a K that takes three chunks, and the largest K and D of the domain.

Tolerances (u = 2^-24, S_i = |x_i|^2 + max_c |c|^2):
  * grid operands (integers in [-4, 4]): every product and partial sum is an integer below 2^24, so labels, dist, inertia and the update
    are exact;
  * Gaussian operands: the fp32 score |c|^2 - 2 x.c carries at most D u |c|^2 (the norm) + 2 D u |x||c| <= D u S (the contraction) + 2 u S
    (the fused multiply-add), so two scores compare wrongly only within (4 D + 4) u S, and dist (one more norm, one more add) is within
    (2 D + 4) u S of the float64 distance: both are held to tau S with tau = 4 (D + 2) u;
  * update: an fp64 sum of fp32 values divided once and rounded once to fp32 is within 2^-24 max|X| (1 + tiny) of the float64 mean: held
    to 2^-23 max|X|.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")
CAP = importlib.import_module("attention-gan_amd.data.captions")

NS = (1, 63, 257, 1500)
DS = (1, 3, 64, 130, 132, 513)
KS = (1, 2, 9, 31, 32, 33, 37, 127, 128, 129, 300, 301)      # 32: the tilings' threshold; 128: the centroid chunk
SHAPES = [(n, d, k) for n in NS for d in DS for k in KS if k <= n]
# the edges of the domain: K = 4096 (every thread of the update's prefix pass owns clusters, the last one the totals), D = 4096 under both
# tilings, and K just below the edge with a D that is no multiple of 4
SHAPES += [(4200, 5, 4096), (4200, 8, 4095), (130, 4096, 33), (70, 4096, 9)]
U = 2.0 ** -24


def seed_of(N, D, K, salt=0):
    return (N * 1_000_003 + D * 1009 + K) * 7 + salt


def scores64(x, c):
    """float64 squared distances [N, K] (expanded form: exact on grid operands, 1e-16-relative otherwise)"""
    x, c = x.double(), c.double()
    return ((x * x).sum(1, keepdim=True) + (c * c).sum(1).view(1, -1) - 2.0 * (x @ c.t())).clamp_(min=0.0)


def argmin_first(d):
    return torch.from_numpy(d.numpy().argmin(axis=1)).to(torch.int32)       # numpy: the first minimum


@functools.lru_cache(maxsize=None)
def grid_case(N, D, K):
    """integer operands in [-4, 4]; every centroid from K // 2 on repeats an earlier one, so ties are certain"""
    g = torch.Generator().manual_seed(seed_of(N, D, K))
    x = torch.randint(-4, 5, (N, D), generator=g).float()
    c = torch.randint(-4, 5, (K, D), generator=g).float()
    if K >= 2:
        c[K // 2:] = c[:K - K // 2].clone()
    c[0] = x[N // 2]                                                       # an exact hit: dist 0 for that row
    if K >= 2:
        c[K // 2] = c[0]
    d = scores64(x, c)
    lab = argmin_first(d)
    dist = d.gather(1, lab.long().view(-1, 1)).view(-1)
    return x, c, lab, dist


@functools.lru_cache(maxsize=None)
def gauss_case(N, D, K):
    """clustered rows: Gaussian noise of 0.15 of the distance to the nearest other centroid around Gaussian centroids.  (With
    D = 1 the centroids are a shuffled lattice over [-3, 3]: 300 random points on a line lie closer to each other than fp32 can tell
    apart at the bound's scale, and every row near such a pair would be ambiguous in the reference itself.)"""
    g = torch.Generator().manual_seed(seed_of(N, D, K, 1))
    if D == 1:
        c = ((torch.arange(K, dtype=torch.float32) + 0.5) * (6.0 / K) - 3.0)[torch.randperm(K, generator=g)].view(K, 1)
    else:
        c = torch.randn(K, D, generator=g)
    near = torch.cdist(c.double(), c.double()).fill_diagonal_(float("inf")).min(1).values.float() if K > 1 else torch.full((1,), 2.0)
    own = torch.randint(0, K, (N,), generator=g)
    x = c[own] + 0.15 * near[own].view(N, 1) * torch.randn(N, D, generator=g) / D ** 0.5
    d = scores64(x, c)
    bound = 4 * (D + 2) * U * ((x.double() ** 2).sum(1) + (c.double() ** 2).sum(1).max())
    return x, c, d, bound


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_assign_exact_on_grid(N, D, K):
    x, c, lab, dist = grid_case(N, D, K)
    got, gdist, n_changed, inertia = HF.kmeans_assign(x.to(DEV), c.to(DEV))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), lab)
    assert torch.equal(gdist.cpu().double(), dist)
    assert float(inertia) == float(dist.sum())
    assert int(n_changed) == N
    # against its own labels nothing changes; against labels with one wrong entry, one does
    prev = lab.clone()
    prev[N // 3] = -5
    _, _, n_changed, _ = HF.kmeans_assign(x.to(DEV), c.to(DEV), prev.to(DEV))
    assert int(n_changed) == 1
    assert int(HF.kmeans_assign(x.to(DEV), c.to(DEV), lab.to(DEV))[2]) == 0


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_assign_gaussian_within_bound(N, D, K):
    x, c, d, bound = gauss_case(N, D, K)
    lab64 = argmin_first(d)
    if K > 1:       # the reference alone: rows whose two best centroids are closer than the bound may land either way
        two = d.topk(2, dim=1, largest=False).values
        ambiguous = int(((two[:, 1] - two[:, 0]) <= bound).sum())
        assert ambiguous <= 0.005 * N, f"{ambiguous} of {N} rows have a best / second-best gap under the bound: pick another seed"
    got, gdist, _, inertia = HF.kmeans_assign(x.to(DEV), c.to(DEV))
    got, gdist = got.cpu(), gdist.cpu().double()
    assert int(got.min()) >= 0 and int(got.max()) < K
    mine = d.gather(1, got.long().view(-1, 1)).view(-1)
    excess = mine - d.min(1).values
    print(f"\nN {N} D {D} K {K}: worst excess / bound {float((excess / bound).max()):.3f}, worst |dist - d64| / bound "
          f"{float(((gdist - mine).abs() / bound).max()):.3f}, rows off the float64 argmin {int((got != lab64).sum())}")
    assert bool((excess <= bound).all())
    assert bool(((gdist - mine).abs() <= bound).all())
    assert int((got != lab64).sum()) <= 0.005 * N
    assert abs(float(inertia) - float(gdist.sum())) <= 1e-12 * float(gdist.sum())      # an fp64 sum of the same fp32 values


@pytest.mark.parametrize("N,D,K", [(1500, 40, 37), (1500, 130, 301)])
def test_assign_overlapping_clusters_within_bound(N, D, K):
    """noise of 0.5 per coordinate around centroids of 0.3 per coordinate: the clusters overlap and second-best centroids are close"""
    g = torch.Generator().manual_seed(seed_of(N, D, K, 3))
    c = 0.3 * torch.randn(K, D, generator=g)
    x = c[torch.randint(0, K, (N,), generator=g)] + 0.5 * torch.randn(N, D, generator=g)
    d = scores64(x, c)
    bound = 4 * (D + 2) * U * ((x.double() ** 2).sum(1) + (c.double() ** 2).sum(1).max())
    two = d.topk(2, dim=1, largest=False).values
    assert int(((two[:, 1] - two[:, 0]) <= bound).sum()) <= 0.005 * N
    got, gdist, _, _ = HF.kmeans_assign(x.to(DEV), c.to(DEV))
    got, gdist = got.cpu(), gdist.cpu().double()
    mine = d.gather(1, got.long().view(-1, 1)).view(-1)
    print(f"\nsmallest gap / scale {float(((two[:, 1] - two[:, 0]) / (bound / (4 * (D + 2) * U))).min()):.2e}, "
          f"rows off the float64 argmin {int((got != argmin_first(d)).sum())}")
    assert bool((mine - two[:, 0] <= bound).all()) and bool(((gdist - mine).abs() <= bound).all())
    assert int((got != argmin_first(d)).sum()) <= 0.005 * N


@functools.lru_cache(maxsize=None)
def update_case(N, D, K):
    """grid rows whose cluster means are the integer rows of M exactly (each row M[c] + g has a partner M[c] - g); cluster K - 1 is
    left empty when K >= 2; rows with label -1 and K hold large values that must not reach any sum"""
    g = torch.Generator().manual_seed(seed_of(N, D, K, 2))
    used = K - 1 if K >= 2 else 1
    lab = torch.randint(0, used, (N,), generator=g).to(torch.int32)
    M = torch.randint(-2, 3, (K, D), generator=g).float()
    x = M[lab.long()].clone()
    for cl in range(used):
        rows = (lab == cl).nonzero().view(-1)
        for a, b in zip(rows[0::2].tolist(), rows[1::2].tolist()):
            gg = torch.randint(-2, 3, (D,), generator=g).float()
            x[a] += gg
            x[b] -= gg
    if N >= 8:
        for r, bad in ((1, -1), (N - 2, K), (N // 2, -7), (N // 2 + 1, K + 12345)):
            lab[r] = bad
            x[r] = 1.0e6
        # the rows taken out may have broken a pair: recompute the expected means in float64
    valid = (lab >= 0) & (lab < K)
    counts = torch.bincount(lab[valid].long(), minlength=K).to(torch.int32)
    sums = torch.zeros(K, D, dtype=torch.float64).index_add_(0, lab[valid].long(), x[valid].double())
    prev = torch.randn(K, D, generator=g)
    mean = torch.where((counts > 0).view(K, 1), sums / counts.clamp(min=1).view(K, 1).double(), prev.double())
    return x, lab, prev, counts, mean


@pytest.mark.parametrize("N,D,K", SHAPES)
def test_update_exact_on_grid(N, D, K):
    x, lab, prev, counts, mean = update_case(N, D, K)
    cen, cnt = HF.kmeans_update(x.to(DEV), lab.to(DEV), prev.to(DEV))
    assert cnt.dtype == torch.int32 and torch.equal(cnt.cpu(), counts)
    cen = cen.cpu()
    empty = counts == 0
    assert torch.equal(cen[empty].view(torch.int32), prev[empty].view(torch.int32))      # bit for bit
    # sums of at most 1500 integers below 2^20 are exact in float64; one division, rounded to double then to float: float(mean) exactly
    assert torch.equal(cen[~empty], mean[~empty].to(torch.float32))


@pytest.mark.parametrize("N,D,K", [(1500, 513, 301), (1500, 132, 37), (257, 130, 129), (63, 3, 9), (1, 1, 1)])
def test_update_gaussian_within_bound(N, D, K):
    x, c, d, _ = gauss_case(N, D, K)
    lab = argmin_first(d)
    cen, cnt = HF.kmeans_update(x.to(DEV), lab.to(DEV), c.to(DEV))
    counts = torch.bincount(lab.long(), minlength=K)
    assert torch.equal(cnt.cpu().long(), counts)
    sums = torch.zeros(K, D, dtype=torch.float64).index_add_(0, lab.long(), x.double())
    mean = torch.where((counts > 0).view(K, 1), sums / counts.clamp(min=1).view(K, 1).double(), c.double())
    err = float((cen.cpu().double() - mean).abs().max())
    assert err <= 2.0 ** -23 * float(x.abs().max()), err


def test_update_long_cluster_is_cut_into_pieces():
    """one cluster of 1400 rows (three pieces of 512) beside short ones"""
    N, D, K = 1500, 130, 5
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-4, 5, (N, D), generator=g).float()
    lab = torch.full((N,), 3, dtype=torch.int32)
    lab[::15] = torch.randint(0, 3, (100,), generator=g).to(torch.int32)
    prev = torch.randn(K, D, generator=g)
    cen, cnt = HF.kmeans_update(x.to(DEV), lab.to(DEV), prev.to(DEV))
    counts = torch.bincount(lab.long(), minlength=K)
    assert int(counts[3]) == 1400 and torch.equal(cnt.cpu().long(), counts)
    sums = torch.zeros(K, D, dtype=torch.float64).index_add_(0, lab.long(), x.double())
    want = torch.where((counts > 0).view(K, 1), (sums / counts.clamp(min=1).view(K, 1)).to(torch.float32), prev)
    assert torch.equal(cen.cpu(), want)


@pytest.mark.parametrize("N,D,K", [(1500, 513, 301), (1500, 132, 300), (257, 130, 37), (63, 3, 9)])
def test_two_runs_give_the_same_bytes(N, D, K):
    x, c, d, _ = gauss_case(N, D, K)
    x, c = x.to(DEV), c.to(DEV)
    a, b = HF.kmeans_assign(x, c), HF.kmeans_assign(x, c)
    for s, t in zip(a, b):
        assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()
    u, v = HF.kmeans_update(x, a[0], c), HF.kmeans_update(x, a[0], c)
    for s, t in zip(u, v):
        assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes()


def test_kmeans_twice_with_one_seed():
    x, _, _, _ = gauss_case(1500, 130, 37)
    a = CAP.kmeans(x.to(DEV), 37, n_init=2, max_iter=20, seed=5)
    b = CAP.kmeans(x.to(DEV), 37, n_init=2, max_iter=20, seed=5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and a[3] == b[3]


@functools.lru_cache(maxsize=None)
def blobs(n_blobs=7, per=40, D=24, spread=0.05, seed=3):
    g = torch.Generator().manual_seed(seed)
    centres = 4.0 * torch.randn(n_blobs, D, generator=g)
    planted = torch.arange(n_blobs).repeat_interleave(per)[torch.randperm(n_blobs * per, generator=g)]
    x = centres[planted] + spread * torch.randn(n_blobs * per, D, generator=g)
    return x, planted.to(torch.int32)


def test_kmeans_recovers_planted_blobs():
    x, planted = blobs()
    K = int(planted.max()) + 1
    init = torch.stack([x[(planted == c).nonzero()[0, 0]] for c in range(K)])        # one row of each blob, in blob order
    # the reference alone: from these centroids and from the blob means every row's two best are at least 1 % of the scale apart
    means = torch.stack([x[planted == c].double().mean(0) for c in range(K)])
    for cen in (init.double(), means):
        d = scores64(x, cen)
        two = d.topk(2, dim=1, largest=False).values
        scale = (x.double() ** 2).sum(1) + (cen ** 2).sum(1).max()
        assert bool(((two[:, 1] - two[:, 0]) >= 0.01 * scale).all())
        assert torch.equal(argmin_first(d), planted)
    history = []
    labels, centroids, inertia, n_iter = CAP.kmeans(x.to(DEV), K, init=init, history=history)
    assert n_iter <= 3 and history[-1][3] == 0
    assert np.array_equal(labels, planted.numpy())
    assert float(np.abs(centroids.astype(np.float64) - means.numpy()).max()) <= 2.0 ** -23 * float(x.abs().max())
    assert inertia == history[-1][2]


def test_kmeans_inertia_never_rises_and_best_restart_wins():
    x, c, _, _ = gauss_case(1500, 130, 37)
    # J(labels_t, C_t) >= J(labels_t, C_t+1) (the mean minimises) >= J(labels_t+1, C_t+1) - sum of tau S_i (a label may be that far from
    # the best), and each recorded inertia is within sum of tau S_i of its J: three times the summed bound of the assignment test, with
    # S_i <= |x_i|^2 + max |x|^2 (every centroid is a row or a mean of rows)
    xn = (x.double() ** 2).sum(1)
    bound = 3.0 * float((4 * (130 + 2) * U * (xn + xn.max())).sum())
    history = []
    labels, centroids, inertia, n_iter = CAP.kmeans(x.to(DEV), 37, n_init=3, max_iter=25, seed=1, history=history)
    runs = {}
    for r, it, total, changed in history:
        runs.setdefault(r, []).append(total)
    assert sorted(runs) == [0, 1, 2]
    for r, totals in runs.items():
        for before, after in zip(totals, totals[1:]):
            assert after <= before + bound, (r, before, after)
    finals = [runs[r][-1] for r in sorted(runs)]
    assert inertia == min(finals)
    best = finals.index(min(finals))                                        # the earliest of equal ones
    alone = []
    CAP.kmeans(x.to(DEV), 37, n_init=best + 1, max_iter=25, seed=1, history=alone)
    assert [h for h in alone if h[0] == best] == [h for h in history if h[0] == best]
    # the returned labels are the assignment to the returned centroids
    again = HF.kmeans_assign(x.to(DEV), torch.from_numpy(centroids).to(DEV))[0]
    assert np.array_equal(again.cpu().numpy(), labels)


def test_kmeans_argument_errors():
    x = torch.randn(20, 4, device=DEV)
    with pytest.raises(ValueError):
        CAP.kmeans(x, 21)
    bad = x.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        CAP.kmeans(bad, 3)


def test_domain_violations_are_einval_without_a_launch():
    lib = L.load()
    ok = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = ctypes.c_void_p(ok.data_ptr())
    torch.cuda.synchronize()
    for N, D, K in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4097, 1), (5000, 1, 4097), (1 << 30, 2, 2), (-1, 4, 1)):
        assert lib.agan_kmeans_assign_ws_bytes(N, D, K) == 0 and lib.agan_kmeans_update_ws_bytes(N, D, K) == 0
        assert lib.agan_kmeans_assign(p, p, p, p, p, p, N, D, K, p, 1 << 20, None) == L.EINVAL
        assert lib.agan_last_error()
        assert lib.agan_kmeans_update(p, p, p, p, N, D, K, p, 1 << 20, None) == L.EINVAL
    # a missing pointer and a missing workspace
    assert lib.agan_kmeans_assign(None, p, p, p, p, p, 4, 4, 2, p, 1 << 20, None) == L.EINVAL
    assert lib.agan_kmeans_update(p, None, p, p, 4, 4, 2, p, 1 << 20, None) == L.EINVAL
    assert lib.agan_kmeans_assign(p, p, p, p, p, p, 4, 4, 2, None, 0, None) == L.EINVAL
    assert lib.agan_kmeans_assign(p, p, p, p, p, p, 4, 4, 2, p, 8, None) == L.EWORKSPACE
    torch.cuda.synchronize()
    assert float(ok.abs().sum()) == 0.0                                     # nothing ran
    # through the wrappers: ValueError
    with pytest.raises(ValueError):
        HF.kmeans_assign(torch.zeros(1, 4097, device=DEV), torch.zeros(1, 4097, device=DEV))
    with pytest.raises(ValueError):
        HF.kmeans_assign(torch.zeros(5000, 1, device=DEV), torch.zeros(4097, 1, device=DEV))
    with pytest.raises(ValueError):
        HF.kmeans_update(torch.zeros(5000, 1, device=DEV), torch.zeros(5000, dtype=torch.int32, device=DEV), torch.zeros(4097, 1, device=DEV))
    with pytest.raises(ValueError):
        HF.kmeans_assign(torch.zeros(4, 3, device=DEV), torch.zeros(2, 4, device=DEV))
