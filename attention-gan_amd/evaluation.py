"""Evaluation of a generator: R-precision and the Frechet distance, the two numbers AttnGAN-style work is judged by.

  * R-precision: does the DAMSM image code of a generated image retrieve its own caption's sentence embedding among R - 1 mismatched
    ones (cosine similarity, losses/sentence_loss.py without gamma3)?  `r_precision` draws the mismatched captions from OTHER class ids
    (the reference's losses mask same-class pairs as non-mismatches) and ranks them with functional.retrieval_rank: R gathered rows
    per query, no N x N score matrix.
  * Frechet distance between the pooled 2048-vectors of the image encoder's trunk over real and over generated images.  The features
    never leave the device: `FeatureMoments` folds each batch into raw fp64 moments (functional.moments_update) and only mean and
    covariance travel to the host, once, for `frechet_distance`.

The trunk's weights are whatever the user loaded (CNNEncoder.load_trunk_state_dict); nothing is downloaded.  A Frechet distance over a
randomly initialised or self-trained trunk orders the checkpoints of one run; it is NOT comparable with published FID values, which
presuppose the ImageNet-trained Inception-v3.  The Inception Score is out of scope (the trunk has no classifier head), and so is
data-parallel evaluation beyond `FeatureMoments.merge`.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, Iterable, List, Optional

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
    """The loop around the two metrics.  `text_encoder(words, lengths) -> (word_embs, sent_embs)` and
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
    def evaluate(self, batches: Iterable, real: FeatureMoments, n_samples: int, R: int = 100, seed: int = 0,
                 batch_size: Optional[int] = None, folds: int = 10, source: str = "fake") -> Dict:
        """Generates up to n_samples images from the batches' captions (noise from a device generator seeded with `seed`), and returns
        {"r_precision", "r_precision_folds", "rank", "fid", "n"}.  A batch whose shortest caption has fewer than 2 words, or with fewer
        rows than batch_size (default: the first batch's), is skipped -- the reference's batch guard (train.py:112).
        source="real" puts the batches' own 256-pixel images in the generator's place: the ceiling of both numbers for this encoder
        pair.  Deterministic for a seed."""
        if source not in ("fake", "real"):
            raise ValueError(f"Evaluator.evaluate: source must be 'fake' or 'real', got {source!r}")
        dev = self.device
        rng = torch.Generator(device=dev)
        rng.manual_seed(int(seed))
        masks = ModelTrainer()
        codes: List[Tensor] = []
        sents: List[Tensor] = []
        cids: List[np.ndarray] = []
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
                codes.append(code[:keep])
                sents.append(sent_embs[:keep])
                cids.append(np.asarray(class_ids.detach().cpu() if isinstance(class_ids, Tensor) else class_ids).reshape(-1)[:keep])
                n += keep
        if n == 0:
            raise ValueError("Evaluator.evaluate: no batch passed the guard")
        out = r_precision(torch.cat(codes), torch.cat(sents), np.concatenate(cids), R=R, seed=seed, folds=folds)
        out["fid"] = frechet_distance(real.mean(), real.cov(), fm.mean(), fm.cov())
        out["n"] = n
        return out
