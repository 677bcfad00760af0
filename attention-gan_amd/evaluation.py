"""Evaluation of a generator: R-precision, the Frechet distance and the Inception Score, the numbers AttnGAN-style work is judged by,
and three companions that look at the image distribution where the Frechet distance is blind or biased.

  * R-precision: does the DAMSM image code of a generated image retrieve its own caption's sentence embedding among R - 1 mismatched
    ones (cosine similarity, losses/sentence_loss.py without gamma3)?  `r_precision` draws the mismatched captions from OTHER class ids
    (the reference's losses mask same-class pairs as non-mismatches) and ranks them with functional.retrieval_rank: R gathered rows
    per query, no N x N score matrix.
  * Frechet distance between the pooled 2048-vectors of the image encoder's trunk over real and over generated images.  The features
    never leave the device: `FeatureMoments` folds each batch into raw fp64 moments (functional.moments_update) and only mean and
    covariance travel to the host, once, for `frechet_distance`.
  * Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020), `manifold_metrics`: the
    Frechet distance mixes fidelity and diversity into one scalar; these tell a collapsed generator (precision high, recall and
    coverage low) from a diverse but poor one.  They need the feature ROWS of both sets -- `FeatureBank` keeps them on the device --
    and reduce the pairwise distances without ever storing them (functional.knn_radius, functional.manifold_scan).
  * The Kernel Inception Distance (Binkowski et al. 2018), `kernel_distance`: an unbiased estimate at any sample count, for the
    "folder of images" case with fewer samples than feature dimensions, where most of the Frechet distance's spectrum is noise
    (functional.poly_kernel_sum).
  * The Inception Score (Salimans et al. 2016), `inception_score`: exp of the mean KL divergence between an image's class distribution
    under a classifier head on the trunk (CNNEncoder(num_classes=...).logits) and the mean distribution of its split, over 10
    contiguous splits of the images, reported as mean and standard deviation with the label entropy (diversity) and the conditional
    entropy (sharpness) it is made of.  functional.inception_split_scores reads the fp32 logits twice and reduces in float64;
    `inception_score_reference` states the protocol in plain torch.

The trunk's weights are whatever the user loaded (CNNEncoder.load_trunk_state_dict); nothing is downloaded.  A Frechet distance over a
randomly initialised or self-trained trunk orders the checkpoints of one run; it is NOT comparable with published FID values, which
presuppose the ImageNet-trained Inception-v3.  The same holds for precision, recall, density, coverage and the kernel distance, and
for the Inception Score, which in addition presupposes a head trained on the image domain (ImageNet's 1000 classes, or the 200-class
CUB fine-tune of AttnGAN evaluations).  Data-parallel evaluation beyond `FeatureMoments.merge` is out of scope.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .backend import functional as AF
from .trainers.trainer import ModelTrainer, sample_fakes


class FeatureMoments:
    """Streaming raw moments (row count, column sums, upper triangle of x^T x; fp64) of feature rows on `device`.  Raw moments add, so
    the statistics of the real images can be computed once, saved (`state_dict`) and reused for every checkpoint, and parts computed
    separately can be combined (`merge`)."""

    def __init__(self, D: int, device="cpu"):
        if not 1 <= int(D) <= 4096:
            raise ValueError(f"FeatureMoments: D {D} outside 1..4096")
        self.D, self.device, self.count = int(D), torch.device(device), 0
        self.sum = torch.zeros(self.D, dtype=torch.float64, device=self.device)
        self.gram = torch.zeros(self.D, self.D, dtype=torch.float64, device=self.device)      # upper triangle; below it: unspecified

    def update(self, x: Tensor) -> "FeatureMoments":
        """adds the rows of x [n, D] (any n; float32, on this object's device)"""
        if x.dim() != 2 or x.shape[1] != self.D:
            raise ValueError(f"FeatureMoments.update: expected [n, {self.D}], got {tuple(x.shape)}")
        if x.shape[0]:
            AF.moments_update(x.detach().to(self.device, torch.float32), self.sum, self.gram)
            self.count += int(x.shape[0])
        return self

    def merge(self, other: "FeatureMoments") -> "FeatureMoments":
        if other.D != self.D:
            raise ValueError(f"FeatureMoments.merge: D {other.D} into D {self.D}")
        self.sum += other.sum.to(self.device)
        self.gram += other.gram.to(self.device)
        self.count += other.count
        return self

    def _finish(self):
        if self.count < 1:
            raise ValueError("FeatureMoments: no rows yet")
        return AF.moments_finish(self.sum, self.gram, self.count)

    def mean(self) -> Tensor:
        return self._finish()[0]

    def cov(self) -> Tensor:
        """unbiased covariance [D, D], symmetric bit for bit (zeros for a single row)"""
        return self._finish()[1]

    def state_dict(self) -> Dict:
        return {"D": self.D, "count": self.count, "sum": self.sum.cpu().clone(), "gram": torch.triu(self.gram).cpu()}

    def load_state_dict(self, sd: Dict) -> None:
        if int(sd["D"]) != self.D:
            raise ValueError(f"FeatureMoments.load_state_dict: state of D {sd['D']} into D {self.D}")
        self.count = int(sd["count"])
        self.sum.copy_(sd["sum"])
        self.gram.copy_(sd["gram"])


class FeatureBank:
    """Append-only store of float32 feature rows [capacity, D] on `device`: what the manifold metrics and the kernel distance need of a
    set of images.  Like FeatureMoments, the real set is computed once, saved (`state_dict`) and reused for every checkpoint."""

    def __init__(self, D: int, capacity: int, device="cpu"):
        if not 1 <= int(D) <= 4096 or int(capacity) < 1 or int(capacity) * int(D) >= 1 << 31:
            raise ValueError(f"FeatureBank: D {D}, capacity {capacity} outside 1 <= D <= 4096, capacity >= 1, capacity * D < 2^31")
        self.D, self.capacity, self.device, self.count = int(D), int(capacity), torch.device(device), 0
        self.data = torch.empty(self.capacity, self.D, dtype=torch.float32, device=self.device)

    def update(self, x: Tensor) -> "FeatureBank":
        """appends the rows of x [n, D]; ValueError when they do not fit"""
        if x.dim() != 2 or x.shape[1] != self.D:
            raise ValueError(f"FeatureBank.update: expected [n, {self.D}], got {tuple(x.shape)}")
        n = int(x.shape[0])
        if self.count + n > self.capacity:
            raise ValueError(f"FeatureBank.update: {self.count} + {n} rows into a capacity of {self.capacity}")
        self.data[self.count:self.count + n].copy_(x.detach())
        self.count += n
        return self

    def rows(self) -> Tensor:
        """the rows so far, [count, D]: a view of the store"""
        return self.data[:self.count]

    def state_dict(self) -> Dict:
        return {"D": self.D, "capacity": self.capacity, "count": self.count, "rows": self.rows().cpu().clone()}

    def load_state_dict(self, sd: Dict) -> None:
        if int(sd["D"]) != self.D or int(sd["count"]) > self.capacity:
            raise ValueError(f"FeatureBank.load_state_dict: {sd['count']} rows of D {sd['D']} into D {self.D}, capacity {self.capacity}")
        self.count = int(sd["count"])
        self.data[:self.count].copy_(sd["rows"])


def _feature_rows(t, what: str) -> Tensor:
    t = t.rows() if isinstance(t, FeatureBank) else t
    if t.dim() != 2 or t.shape[0] < 1:
        raise ValueError(f"{what}: expected feature rows [n, D], got {tuple(t.shape)}")
    return t.detach().float()


def manifold_metrics(real, fake, k: int = 3) -> Dict:
    """-> {"precision", "recall", "density", "coverage"} of the fake rows [M, D] against the real rows [N, D] (tensors or FeatureBanks
    on one device), from k-nearest-neighbour balls: rad2_real[j] is the squared distance from real row j to its k-th nearest OTHER real
    row, rad2_fake alike.
        precision = share of fake rows inside at least one real ball        (Kynkaanniemi et al. 2019)
        recall    = share of real rows inside at least one fake ball
        density   = number of real balls a fake row lies in, summed over the fake rows, / (k M)        (Naeem et al. 2020)
        coverage  = share of real rows whose nearest fake row lies inside the real row's own ball
    The published defaults are k = 3 for precision and recall and k = 5 for density and coverage; one k serves all four here, call
    twice for both.  Four passes over pairwise distances that are never stored: knn_radius of each set, a scan of fake against real
    and a scan of real against fake.  Both sets are first translated by the real set's column mean: distances do not change, but the
    kernels form them as |q|^2 + |r|^2 - 2 q.r, which cancels badly for features that share a large offset (pooled Inception
    features are non-negative)."""
    real, fake = _feature_rows(real, "manifold_metrics"), _feature_rows(fake, "manifold_metrics")
    if real.shape[1] != fake.shape[1] or real.device != fake.device:
        raise ValueError(f"manifold_metrics: real is {tuple(real.shape)} on {real.device}, fake {tuple(fake.shape)} on {fake.device}")
    k = int(k)
    if not 1 <= k <= 8 or real.shape[0] < k + 1 or fake.shape[0] < k + 1:
        raise ValueError(f"manifold_metrics: k {k} with {real.shape[0]} real and {fake.shape[0]} fake rows (1 <= k <= 8, k + 1 rows each)")
    centre = real.double().mean(0).float()
    real, fake = (real - centre).contiguous(), (fake - centre).contiguous()
    rad_real, rad_fake = AF.knn_radius(real, k), AF.knn_radius(fake, k)
    count_fr, _, _ = AF.manifold_scan(fake, real, rad_real)
    count_rf, near_rf, _ = AF.manifold_scan(real, fake, rad_fake)
    M = fake.shape[0]
    return {"precision": float((count_fr > 0).double().mean()), "recall": float((count_rf > 0).double().mean()),
            "density": float(count_fr.double().sum()) / (k * M), "coverage": float((near_rf <= rad_real).double().mean())}


def kernel_distance(real, fake, subsets: int = 100, subset_size: int = 1000, seed: int = 0) -> Dict:
    """-> {"kid", "kid_std"}: the Kernel Inception Distance, the unbiased estimate of the squared maximum mean discrepancy under the
    kernel (x.y / D + 1)^3, as mean and standard deviation over `subsets` subsets of s = min(subset_size, N, M) rows of each set:
        sum_{i != j} k(x_i, x_j) / (s (s - 1)) + sum_{i != j} k(y_i, y_j) / (s (s - 1)) - 2 sum_{i, j} k(x_i, y_j) / s^2.
    The subsets are drawn without replacement by a host generator seeded with `seed` and gathered on the device; the three sums come
    from functional.poly_kernel_sum.  Deterministic for a seed; the standard deviation of a single subset is 0."""
    real, fake = _feature_rows(real, "kernel_distance"), _feature_rows(fake, "kernel_distance")
    if real.shape[1] != fake.shape[1] or real.device != fake.device:
        raise ValueError(f"kernel_distance: real is {tuple(real.shape)} on {real.device}, fake {tuple(fake.shape)} on {fake.device}")
    N, M = real.shape[0], fake.shape[0]
    s = min(int(subset_size), N, M)
    if int(subsets) < 1 or s < 2:
        raise ValueError(f"kernel_distance: {subsets} subsets of {s} rows (at least 1 subset of at least 2 rows)")
    g = torch.Generator().manual_seed(int(seed))
    sums = []
    for _ in range(int(subsets)):
        x = real[torch.randperm(N, generator=g)[:s].to(real.device)].contiguous()
        y = fake[torch.randperm(M, generator=g)[:s].to(fake.device)].contiguous()
        sums.append(torch.cat([AF.poly_kernel_sum(x, x, True), AF.poly_kernel_sum(y, y, True), AF.poly_kernel_sum(x, y)]))
    t = torch.stack(sums).cpu()                                 # [subsets, 3] float64: the one synchronisation
    est = (t[:, 0] + t[:, 1]) / (s * (s - 1)) - 2.0 * t[:, 2] / (s * s)
    return {"kid": float(est.mean()), "kid_std": float(est.std(unbiased=False))}


def _splits_arg(splits, rows: Optional[int], what: str) -> int:
    """an integer number of splits in 1..min(rows, 1024) (1..1024 while the row count is not known yet), or ValueError"""
    most = 1024 if rows is None else min(rows, 1024)
    if isinstance(splits, bool) or not isinstance(splits, (int, np.integer)) or not 1 <= int(splits) <= most:
        raise ValueError(f"{what}: {splits!r} splits" + ("" if rows is None else f" of {rows} rows") +
                         " (an integer, 1 <= splits <= min(rows, 1024): no split may be empty)")
    return int(splits)


def _logit_rows(logits: Tensor, splits, what: str) -> int:
    if not isinstance(logits, Tensor) or logits.dim() != 2 or logits.shape[1] < 1:
        raise ValueError(f"{what}: expected logits [N, C], got {tuple(logits.shape) if isinstance(logits, Tensor) else type(logits).__name__}")
    return _splits_arg(splits, logits.shape[0], what)


def inception_score_reference(logits: Tensor, splits: int = 10) -> Tensor:
    """-> float64 [splits, 3] on the device of logits [N, C]: (IS_s, Hm_s, Hc_s) of split s = rows [s N // splits, (s + 1) N // splits),
    the contiguous chunks of the published protocol, in plain float64 torch:
        lse_k = m_k + log sum_y exp(l[k][y] - m_k) with m_k the row's maximum;  logp = l[k][y] - lse_k;  p = exp(logp)
        Hc_s = -mean_k sum_y p logp;  q_s = mean_k p[k];  Hm_s = -sum_y q log q        (a term with p == 0 or q == 0 counts as 0)
        IS_s = exp(Hm_s - Hc_s) = exp(mean_k KL(p(.|x_k) || q_s)).
    logp comes from l - lse and never from log(p), so an underflowed or masked (-inf) class gives 0 and not NaN; a row that holds +inf
    or a NaN, or nothing but -inf, makes its own split NaN.  The yardstick of functional.inception_split_scores."""
    splits = _logit_rows(logits, splits, "inception_score_reference")
    l = logits.detach().double()
    N = l.shape[0]
    zero = torch.zeros((), dtype=torch.float64, device=l.device)
    rows = []
    for s in range(splits):
        x = l[s * N // splits:(s + 1) * N // splits]
        m = x.max(1, keepdim=True)[0]
        lse = m + (x - m).exp().sum(1, keepdim=True).log()
        logp = x - lse
        p = logp.exp()
        hc = -torch.where(p == 0, zero, p * logp).sum(1).mean()
        q = p.mean(0)
        hm = -torch.where(q == 0, zero, q * q.log()).sum()
        rows.append(torch.stack([(hm - hc).exp(), hm, hc]))
    return torch.stack(rows)


def inception_score(logits: Tensor, splits: int = 10) -> Dict:
    """-> {"inception_score": mean of the splits' scores, "inception_score_std": their standard deviation (ddof = 0, the published
    np.std), "inception_score_splits": the scores, "label_entropy", "conditional_entropy": the means of Hm and Hc over the splits}
    of classifier logits [N, C] (any float dtype; reduced from float32), by functional.inception_split_scores and one read-back of
    [splits, 3] doubles.  IS = exp(label entropy - conditional entropy) per split: a sharp classifier on diverse images scores high."""
    splits = _logit_rows(logits, splits, "inception_score")
    t = AF.inception_split_scores(logits.detach().float(), splits).cpu()      # the one synchronisation
    return {"inception_score": float(t[:, 0].mean()), "inception_score_std": float(t[:, 0].std(unbiased=False)),
            "inception_score_splits": [float(v) for v in t[:, 0]], "label_entropy": float(t[:, 1].mean()),
            "conditional_entropy": float(t[:, 2].mean())}


def frechet_distance(mu1: Tensor, cov1: Tensor, mu2: Tensor, cov2: Tensor) -> float:
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2), in float64 on the host.  With S1 = V L V^T the last trace is the sum of the
    square roots of the eigenvalues of the symmetric matrix L^(1/2) V^T S2 V L^(1/2) (similar to S1 S2), each clamped at 0: two
    torch.linalg.eigh calls, no matrix square root of a non-symmetric product.  An eigenvalue within D 2^-52 of the largest one's
    size is rounding noise of the factorisation (the usual rank tolerance) and counts as 0: with fewer samples than features most of
    the spectrum is such noise, and the square root would turn 1e-16 into 1e-8, D times over.  The result itself is not clamped, so
    noise around zero shows."""
    mu1, mu2 = (m.detach().to("cpu", torch.float64).view(-1) for m in (mu1, mu2))
    cov1, cov2 = (c.detach().to("cpu", torch.float64) for c in (cov1, cov2))
    D = mu1.numel()
    if mu2.numel() != D or tuple(cov1.shape) != (D, D) or tuple(cov2.shape) != (D, D):
        raise ValueError(f"frechet_distance: shapes {tuple(mu1.shape)}, {tuple(cov1.shape)}, {tuple(mu2.shape)}, {tuple(cov2.shape)}")

    def positive_part(ev: Tensor) -> Tensor:
        return torch.where(ev > D * 2.0 ** -52 * ev.abs().max(), ev, torch.zeros_like(ev))

    lam, V = torch.linalg.eigh(cov1)
    root = positive_part(lam).sqrt()
    inner = root.view(-1, 1) * (V.t() @ cov2 @ V) * root.view(1, -1)
    ev = positive_part(torch.linalg.eigvalsh(0.5 * (inner + inner.t())))
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(cov1) + torch.trace(cov2) - 2.0 * ev.sqrt().sum())


def draw_mismatched(class_ids, R: int, seed: int = 0) -> Tensor:
    """-> int32 [N, R] on the host: column 0 is the row itself, columns 1.. are R - 1 DISTINCT rows of another class id, drawn uniformly
    with a host generator seeded by `seed`.  ValueError if a row has fewer than R - 1 rows of other classes."""
    cls = torch.as_tensor(np.asarray(class_ids)).long().view(-1)
    N, K = cls.numel(), int(R) - 1
    if N < 1 or K < 0:
        raise ValueError(f"draw_mismatched: N {N}, R {R}")
    own = torch.arange(N).view(N, 1)
    if K == 0:
        return own.to(torch.int32)
    order = torch.argsort(cls, stable=True)                     # rows grouped by class: the other classes are what is left of a range
    uniq, counts = torch.unique_consecutive(cls[order], return_counts=True)
    starts = counts.cumsum(0) - counts
    k = torch.searchsorted(uniq, cls)
    n_same, start = counts[k], starts[k]
    m = N - n_same                                              # rows of other classes, per query
    if int(m.min()) < K:
        raise ValueError(f"r_precision: a class leaves only {int(m.min())} rows of other classes, R - 1 = {K} are needed")
    g = torch.Generator().manual_seed(int(seed))
    u = torch.empty(N, K, dtype=torch.int64)                    # positions among the other-class rows
    dense = m < 2 * K
    rows = (~dense).nonzero().view(-1)
    if rows.numel():                                            # many to choose from: draw, then redraw what repeats
        mm = m[rows].view(-1, 1)
        draw = torch.minimum((torch.rand(rows.numel(), K, generator=g, dtype=torch.float64) * mm).long(), mm - 1)
        while True:
            srt, idx = draw.sort(1)
            rep = torch.zeros_like(srt, dtype=torch.bool)
            rep[:, 1:] = srt[:, 1:] == srt[:, :-1]
            if not bool(rep.any()):
                break
            rep = torch.zeros_like(rep).scatter_(1, idx, rep)
            lim = mm.expand_as(draw)[rep]
            draw[rep] = torch.minimum((torch.rand(lim.numel(), generator=g, dtype=torch.float64) * lim).long(), lim - 1)
        u[rows] = draw
    for i in dense.nonzero().view(-1).tolist():                 # few to choose from: a permutation's head
        u[i] = torch.randperm(int(m[i]), generator=g)[:K]
    pos = u + (u >= start.view(N, 1)) * n_same.view(N, 1)       # skip the query's own class in the grouped order
    return torch.cat([own, order[pos]], 1).to(torch.int32)


def r_precision(img_codes: Tensor, sent_embs: Tensor, class_ids, R: int = 100, seed: int = 0, folds: int = 10) -> Dict:
    """Retrieval of each image's own caption among R - 1 captions of other classes (draw_mismatched), by cosine similarity.
    -> {"r_precision": hit rate over all N rows, "r_precision_folds": the hit rates of `folds` equal consecutive parts (AttnGAN's
    "mean over 10 folds"; N % folds trailing rows belong to no fold), "rank": int32 [N] on the codes' device}.  A hit is rank 0: no
    mismatched caption scores as high as the match."""
    if img_codes.dim() != 2 or img_codes.shape != sent_embs.shape:
        raise ValueError(f"r_precision: img_codes {tuple(img_codes.shape)} and sent_embs {tuple(sent_embs.shape)} must both be [N, D]")
    N = img_codes.shape[0]
    if not 1 <= int(folds) <= N:
        raise ValueError(f"r_precision: {folds} folds of {N} rows")
    cand = draw_mismatched(class_ids, R, seed)
    if cand.shape[0] != N:
        raise ValueError(f"r_precision: {cand.shape[0]} class ids for {N} rows")
    rank = AF.retrieval_rank(img_codes.detach().float(), sent_embs.detach().float().to(img_codes.device), cand.to(img_codes.device))
    hit = (rank == 0).to(torch.float64).cpu()
    size = N // int(folds)
    return {"r_precision": float(hit.mean()), "r_precision_folds": [float(hit[f * size:(f + 1) * size].mean()) for f in range(int(folds))],
            "rank": rank}


@contextlib.contextmanager
def _eval_mode(*modules):
    """eval() on every nn.Module among `modules`, their modes restored on exit"""
    mods = [m for m in modules if isinstance(m, torch.nn.Module)]
    was = [m.training for m in mods]
    for m in mods:
        m.eval()
    try:
        yield
    finally:
        for m, w in zip(mods, was):
            m.train(w)


class Evaluator:
    """The loop around the metrics.  `text_encoder(words, lengths) -> (word_embs, sent_embs)` and
    `image_encoder.code_and_pooled(images) -> (cnn_code [B, E], pooled [B, P])` (networks.CNNEncoder, either backend; one trunk pass
    gives both); `generator` as GanTrainStep's.  Batches come in the reference's wire format
    (words, lengths, class_ids, img64, img128, img256)."""

    def __init__(self, generator, text_encoder: Callable, image_encoder, device=None):
        if not hasattr(image_encoder, "code_and_pooled"):
            raise ValueError("Evaluator: the image encoder must provide code_and_pooled(images) -> (cnn_code, pooled) (networks.CNNEncoder does)")
        self.G, self.text_encoder, self.image_encoder = generator, text_encoder, image_encoder
        self.device = torch.device(device) if device is not None else next(generator.parameters()).device

    @torch.no_grad()
    def real_moments(self, batches: Iterable) -> FeatureMoments:
        """feature moments of the batches' 256-pixel real images"""
        fm = None
        with _eval_mode(self.image_encoder):
            for batch in batches:
                _, pooled = self.image_encoder.code_and_pooled(batch[5].to(self.device))
                fm = fm or FeatureMoments(pooled.shape[1], self.device)
                fm.update(pooled)
        if fm is None:
            raise ValueError("Evaluator.real_moments: no batches")
        return fm

    @torch.no_grad()
    def real_statistics(self, batches: Iterable) -> Tuple[FeatureMoments, FeatureBank]:
        """feature moments AND feature rows of the batches' 256-pixel real images, from one trunk pass (the batches are listed first:
        the bank's capacity is their row count)"""
        batches = list(batches)
        if not batches:
            raise ValueError("Evaluator.real_statistics: no batches")
        fm = bank = None
        with _eval_mode(self.image_encoder):
            for batch in batches:
                _, pooled = self.image_encoder.code_and_pooled(batch[5].to(self.device))
                if fm is None:
                    fm = FeatureMoments(pooled.shape[1], self.device)
                    bank = FeatureBank(pooled.shape[1], sum(int(b[5].shape[0]) for b in batches), self.device)
                fm.update(pooled)
                bank.update(pooled)
        return fm, bank

    @torch.no_grad()
    def evaluate(self, batches: Iterable, real: FeatureMoments, n_samples: int, R: int = 100, seed: int = 0,
                 batch_size: Optional[int] = None, folds: int = 10, source: str = "fake", real_features: Optional[FeatureBank] = None,
                 k: int = 3, kid_subsets: int = 100, kid_subset_size: int = 1000, inception_splits: Optional[int] = None) -> Dict:
        """Generates up to n_samples images from the batches' captions (noise from a device generator seeded with `seed`), and returns
        {"r_precision", "r_precision_folds", "rank", "fid", "n"}.  A batch whose shortest caption has fewer than 2 words, or with fewer
        rows than batch_size (default: the first batch's), is skipped -- the reference's batch guard (train.py:112).
        source="real" puts the batches' own 256-pixel images in the generator's place: the ceiling of both numbers for this encoder
        pair.  Deterministic for a seed.
        With real_features (a FeatureBank of real images, e.g. from real_statistics) the generated pooled vectors are kept too and the
        result gains "precision", "recall", "density", "coverage" (manifold_metrics with k) and "kid", "kid_std" (kernel_distance
        with kid_subsets, kid_subset_size and seed).  Without it nothing more is stored or launched.
        With inception_splits (an integer; the published protocol uses 10) the image encoder must offer `logits(pooled)`
        (CNNEncoder(num_classes=...)): the kept rows' class logits are collected too and the result gains "inception_score",
        "inception_score_std", "inception_score_splits", "label_entropy" and "conditional_entropy" (inception_score); source="real"
        gives the real images' score.  More splits than kept rows is a ValueError.  With None nothing more is stored or launched."""
        if source not in ("fake", "real"):
            raise ValueError(f"Evaluator.evaluate: source must be 'fake' or 'real', got {source!r}")
        if real_features is not None and not isinstance(real_features, FeatureBank):
            raise ValueError(f"Evaluator.evaluate: real_features must be a FeatureBank, got {type(real_features).__name__}")
        if inception_splits is not None:
            _splits_arg(inception_splits, None, "Evaluator.evaluate: inception_splits")
            if not hasattr(self.image_encoder, "logits"):
                raise ValueError("Evaluator.evaluate: inception_splits needs an image encoder with logits(pooled) -> class logits "
                                 "(networks.CNNEncoder(num_classes=...))")
        dev = self.device
        rng = torch.Generator(device=dev)
        rng.manual_seed(int(seed))
        masks = ModelTrainer()
        codes: List[Tensor] = []
        sents: List[Tensor] = []
        cids: List[np.ndarray] = []
        feats: List[Tensor] = []
        class_logits: List[Tensor] = []
        fm, n = None, 0
        with _eval_mode(self.G, self.text_encoder, self.image_encoder):
            for batch in batches:
                if n >= n_samples:
                    break
                words, lengths, class_ids, _img64, _img128, img256 = batch
                lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
                if batch_size is None:
                    batch_size = len(words)
                if not lens or min(lens) < 2 or len(words) < batch_size:
                    continue
                word_embs, sent_embs = self.text_encoder(words.to(dev), lengths)
                word_embs, sent_embs = word_embs.contiguous(), sent_embs.contiguous()
                if source == "fake":
                    mask = masks._make_mask(lens, word_embs.shape[2]).to(dev)
                    images = sample_fakes(self.G, word_embs, sent_embs, mask, rng)[-1]
                else:
                    images = img256.to(dev)
                code, pooled = self.image_encoder.code_and_pooled(images)
                keep = min(len(lens), n_samples - n)
                fm = fm or FeatureMoments(pooled.shape[1], dev)
                fm.update(pooled[:keep])
                if real_features is not None:
                    feats.append(pooled[:keep].detach().float())
                if inception_splits is not None:
                    class_logits.append(self.image_encoder.logits(pooled[:keep]).detach().float())
                codes.append(code[:keep])
                sents.append(sent_embs[:keep])
                cids.append(np.asarray(class_ids.detach().cpu() if isinstance(class_ids, Tensor) else class_ids).reshape(-1)[:keep])
                n += keep
        if n == 0:
            raise ValueError("Evaluator.evaluate: no batch passed the guard")
        if inception_splits is not None:
            _splits_arg(inception_splits, n, "Evaluator.evaluate: inception_splits")
        out = r_precision(torch.cat(codes), torch.cat(sents), np.concatenate(cids), R=R, seed=seed, folds=folds)
        out["fid"] = frechet_distance(real.mean(), real.cov(), fm.mean(), fm.cov())
        out["n"] = n
        if real_features is not None:
            fake_rows = torch.cat(feats)
            out.update(manifold_metrics(real_features, fake_rows, k=k))
            out.update(kernel_distance(real_features, fake_rows, subsets=kid_subsets, subset_size=kid_subset_size, seed=seed))
        if inception_splits is not None:
            out.update(inception_score(torch.cat(class_logits), int(inception_splits)))
        return out
