"""agan_moments_* / agan_retrieval_rank (csrc/eval.hip) and evaluation.Evaluator on the GPU against float64 restatements.

Moments.  Shapes: the cross of n and D below -- tails in both dimensions around the 16-wide fp64 MFMA tile, the 4-row k-step, the
32-row LDS chunk, the 64-wide workgroup tile and the 512-row sum piece -- plus one case more than one tile wide at the real feature
width and the edge of the domain.  fp32 -> fp64 is exact and so is a product of two fp32 values in fp64, so only additions round:
  * grid operands (integers in [-4, 4]): no addition rounds either; sum and the upper triangle of gram are exact, also when the rows
    arrive as three calls into one state;
  * Gaussian operands (mean 3, std 0.5 -- the unfriendly case for raw moments): at most n + O(1) additions per element on either side of
    the comparison, so |gram - ref| <= 2 (n + 8) 2^-53 (|X|^T |X|) and |sum - ref| <= 2 (n + 8) 2^-53 sum_k |x_kj|;
  * finish: mean within 2^-52 relative of sum / count (one division); cov within 8 (n + 8) 2^-53 max|x|^2 n / (n - 1) of torch.cov in
    float64 -- the cancellation bound of the raw-moment form; cov symmetric bit for bit.
Entries below the diagonal of gram are never compared.

Retrieval.  u = 2^-24; a score is within tau = (2 D + 8) u of the float64 cosine: D u for the dot product relative to |q||b| (by
Cauchy-Schwarz the score's own scale), (D / 2 + 1) u per norm, a few u for product and division.  rank[i] must lie in
[#{s64_j > s64_0 + 2 tau}, #{s64_j >= s64_0 - 2 tau}]; the two ends may differ in at most 10 % of the rows (a condition on the test's
inputs, not a measurement of the kernel).  The separated case plants cosines 0.01 apart and demands the planted rank exactly.
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
EV = importlib.import_module("attention-gan_amd.evaluation")

NS = (1, 3, 63, 257, 1500)
DS = (1, 3, 15, 16, 17, 64, 130, 513)
MOMENT_SHAPES = [(n, d) for n in NS for d in DS] + [(70, 2048), (5, 4096)]
EPS53 = 2.0 ** -53
U = 2.0 ** -24


def seed_of(*dims, salt=0):
    s = salt
    for d in dims:
        s = s * 1_000_003 + d
    return s % (1 << 62)


def upper(t):
    return torch.triu(t.cpu())


# ------------------------------------------------------------------------------------------------------------------
# moments
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_case(n, D):
    g = torch.Generator().manual_seed(seed_of(n, D))
    x = torch.randint(-4, 5, (n, D), generator=g).float()
    x64 = x.double()
    return x, x64.sum(0), x64.t() @ x64


@functools.lru_cache(maxsize=None)
def gauss_case(n, D):
    g = torch.Generator().manual_seed(seed_of(n, D, salt=1))
    x = (3.0 + 0.5 * torch.randn(n, D, generator=g)).float()
    x64 = x.double()
    return x, x64.sum(0), x64.t() @ x64, x64.abs().sum(0), x64.abs().t() @ x64.abs()


def run_moments(x, splits=None):
    """-> (sum, gram) on the device after the rows of x went in as one call, or as the consecutive parts `splits`"""
    n, D = x.shape
    s = torch.zeros(D, dtype=torch.float64, device=DEV)
    gm = torch.zeros(D, D, dtype=torch.float64, device=DEV)
    xd = x.to(DEV)
    lo = 0
    for part in (splits or [n]):
        HF.moments_update(xd[lo:lo + part], s, gm)
        lo += part
    assert lo == n
    return s, gm


def three_calls(n):
    """(1, 7, rest), cut short where n has fewer rows"""
    parts = [min(1, n), min(7, max(0, n - 1)), max(0, n - 8)]
    return [p for p in parts if p]


@pytest.mark.parametrize("n,D", MOMENT_SHAPES)
def test_moments_grid_exact(n, D):
    x, ref_sum, ref_gram = grid_case(n, D)
    for splits in (None, three_calls(n)):
        s, gm = run_moments(x, splits)
        assert torch.equal(s.cpu(), ref_sum), f"sum differs (splits {splits})"
        assert torch.equal(upper(gm), torch.triu(ref_gram)), f"upper triangle of gram differs (splits {splits})"


@pytest.mark.parametrize("n,D", MOMENT_SHAPES)
def test_moments_gauss_bounds(n, D):
    x, ref_sum, ref_gram, abs_sum, abs_gram = gauss_case(n, D)
    s, gm = run_moments(x)
    s2, gm2 = run_moments(x)
    assert torch.equal(s, s2) and torch.equal(torch.triu(gm), torch.triu(gm2)), "two runs differ"
    k = 2.0 * (n + 8) * EPS53
    err_s = (s.cpu() - ref_sum).abs()
    err_g = torch.triu((gm.cpu() - ref_gram).abs())
    print(f"n {n} D {D}: max sum err / bound {float((err_s / (k * abs_sum)).max()):.3g}, "
          f"max gram err / bound {float((err_g / (k * abs_gram)).max()):.3g}")
    assert bool((err_s <= k * abs_sum).all())
    assert bool((err_g <= k * abs_gram).all())

    mean, cov = HF.moments_finish(s, gm, n)
    mean2, cov2 = HF.moments_finish(s, gm, n)
    assert torch.equal(mean, mean2) and torch.equal(cov, cov2), "two runs of finish differ"
    want_mean = s.cpu() / n
    assert bool(((mean.cpu() - want_mean).abs() <= 2.0 ** -52 * want_mean.abs()).all())
    cov = cov.cpu()
    assert torch.equal(cov, cov.t()), "cov is not symmetric bit for bit"
    if n == 1:
        assert not bool(cov.any()), "count == 1 must give a zero covariance"
        return
    ref_cov = torch.cov(x.double().t()).view(D, D)
    bound = 8.0 * (n + 8) * EPS53 * float(x.abs().max()) ** 2 * n / (n - 1)
    err_c = float((cov - ref_cov).abs().max())
    print(f"n {n} D {D}: max cov err {err_c:.3g}, bound {bound:.3g}, max|cov| {float(ref_cov.abs().max()):.3g}")
    assert err_c <= bound


def test_moments_bad_arguments():
    x = torch.zeros(4, 8, device=DEV)
    s = torch.zeros(8, dtype=torch.float64, device=DEV)
    gm = torch.zeros(8, 8, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        HF.moments_update(x.double(), s, gm)
    with pytest.raises(ValueError):
        HF.moments_update(x, s.float(), gm)
    with pytest.raises(ValueError):
        HF.moments_update(x, s, gm[:, :4])
    with pytest.raises(ValueError):
        HF.moments_update(torch.zeros(2, 4097, device=DEV), torch.zeros(4097, dtype=torch.float64, device=DEV),
                          torch.zeros(4097, 4097, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        HF.moments_finish(s, gm, 0)
    lib = L.load()
    assert lib.agan_moments_update_ws_bytes(0, 8) == 0 and lib.agan_moments_update_ws_bytes(4, 4097) == 0
    assert lib.agan_moments_update(ctypes.c_void_p(x.data_ptr()), 4, 8, ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(gm.data_ptr()),
                                   None, 0, None) == L.EINVAL


# ------------------------------------------------------------------------------------------------------------------
# retrieval rank
# ------------------------------------------------------------------------------------------------------------------
RETRIEVAL_SHAPES = [(257, 300, 256, 100), (63, 64, 130, 8), (1500, 2000, 256, 100), (257, 300, 3, 100)]


def cosine64(q, bank, cand):
    q, b = q.double(), bank.double()[cand.long()]
    dot = (q.unsqueeze(1) * b).sum(-1)
    return dot / ((q * q).sum(1).sqrt().view(-1, 1) * (b * b).sum(-1).sqrt()).clamp(min=1e-8)


@functools.lru_cache(maxsize=None)
def retrieval_case(N, M, D, R):
    g = torch.Generator().manual_seed(seed_of(N, M, D, R))
    q = torch.randn(N, D, generator=g)
    bank = torch.randn(M, D, generator=g)
    cand = torch.rand(N, M, generator=g).argsort(1)[:, :R].to(torch.int32).contiguous()      # distinct rows per query
    s64 = cosine64(q, bank, cand)
    tau = (2 * D + 8) * U
    lo = (s64[:, 1:] > s64[:, :1] + 2 * tau).sum(1)
    hi = (s64[:, 1:] >= s64[:, :1] - 2 * tau).sum(1)
    return q, bank, cand, s64, tau, lo, hi


@pytest.mark.parametrize("N,M,D,R", RETRIEVAL_SHAPES)
def test_retrieval_gauss(N, M, D, R):
    q, bank, cand, s64, tau, lo, hi = retrieval_case(N, M, D, R)
    ambiguous = float((lo != hi).double().mean())
    print(f"N {N} M {M} D {D} R {R}: {100 * ambiguous:.1f} % of the rows have an ambiguous rank in float64")
    assert ambiguous <= 0.10, "the reference itself cannot tell the rank of too many rows: change the seed, not the cap"
    rank, scores = HF.retrieval_rank(q.to(DEV), bank.to(DEV), cand.to(DEV), want_scores=True)
    rank2, scores2 = HF.retrieval_rank(q.to(DEV), bank.to(DEV), cand.to(DEV), want_scores=True)
    assert torch.equal(rank, rank2) and torch.equal(scores, scores2), "two runs differ"
    only_rank = HF.retrieval_rank(q.to(DEV), bank.to(DEV), cand.to(DEV))
    assert torch.equal(only_rank, rank), "the rank depends on whether the scores are written"
    err = float((scores.cpu().double() - s64).abs().max())
    print(f"max score err {err:.3g}, tau {tau:.3g}")
    assert err <= tau
    r = rank.cpu().long()
    assert bool(((r >= lo) & (r <= hi)).all())


def test_retrieval_separated_ranks_exact():
    """b_j = c_j q^ + sqrt(1 - c_j^2) r^_j with r^_j orthogonal to q: the cosines are the planted c_j, distinct multiples of 0.01, so every
    rank is far from any tie (tau = 1.6e-5 at D = 130) and must come out exactly.  Query i's match sits at position i % R from the top."""
    N, D, R = 96, 130, 24
    g = torch.Generator().manual_seed(11)
    q = torch.randn(N, D, generator=g, dtype=torch.float64)
    qh = q / q.norm(dim=1, keepdim=True)
    levels = torch.arange(-45, 46, dtype=torch.float64) * 0.01
    bank = torch.empty(N * R, D, dtype=torch.float64)
    cand = torch.empty(N, R, dtype=torch.int32)
    want = torch.empty(N, dtype=torch.int64)
    rows = torch.randperm(N * R, generator=g).view(N, R)                                # where each query's candidates live in the bank
    for i in range(N):
        d = levels[torch.randperm(levels.numel(), generator=g)[:R]].sort(descending=True)[0]
        p = i % R                                                                       # the match is the p-th from the top
        others = torch.cat([d[:p], d[p + 1:]])[torch.randperm(R - 1, generator=g)]
        c = torch.cat([d[p].view(1), others])                                           # c[0]: the match's cosine
        want[i] = p
        r = torch.randn(R, D, generator=g, dtype=torch.float64)
        r = r - (r @ qh[i]).view(-1, 1) * qh[i]
        r = r / r.norm(dim=1, keepdim=True)
        b = c.view(-1, 1) * qh[i] + (1 - c * c).sqrt().view(-1, 1) * r
        bank[rows[i]] = b * (0.25 + 4 * torch.rand(R, 1, generator=g, dtype=torch.float64))   # the norm must not matter
        cand[i] = rows[i].to(torch.int32)
    assert sorted(set(want.tolist())) == list(range(R)), "every position is planted"
    rank = HF.retrieval_rank(q.float().to(DEV), bank.float().to(DEV), cand.to(DEV))
    assert torch.equal(rank.cpu().long(), want)


def test_retrieval_d1_pins_the_tie_rule():
    """D = 1: every score is exactly +1 or -1, so ties are certain and `>=` (a tie counts against the match) is what is tested"""
    N, M, R = 70, 90, 33
    g = torch.Generator().manual_seed(5)
    q = (torch.rand(N, 1, generator=g) + 0.1) * (torch.randint(0, 2, (N, 1), generator=g) * 2 - 1)
    bank = (torch.rand(M, 1, generator=g) + 0.1) * (torch.randint(0, 2, (M, 1), generator=g) * 2 - 1)
    cand = torch.rand(N, M, generator=g).argsort(1)[:, :R].to(torch.int32).contiguous()
    sign = torch.sign(q) * torch.sign(bank.view(-1)[cand.long()])                       # [N, R]
    want = (sign[:, 1:] >= sign[:, :1]).sum(1)
    assert 0 < int((sign[:, 0] > 0).sum()) < N
    rank, scores = HF.retrieval_rank(q.to(DEV), bank.to(DEV), cand.to(DEV), want_scores=True)
    assert torch.equal(scores.cpu(), sign)
    assert torch.equal(rank.cpu().long(), want)


def test_retrieval_r1_is_rank_zero():
    g = torch.Generator().manual_seed(6)
    q, bank = torch.randn(37, 20, generator=g), torch.randn(11, 20, generator=g)
    cand = torch.randint(0, 11, (37, 1), generator=g).to(torch.int32)
    rank = HF.retrieval_rank(q.to(DEV), bank.to(DEV), cand.to(DEV))
    assert not bool(rank.any())


@pytest.mark.parametrize("bad", ["M", -1])
def test_retrieval_refuses_a_bad_candidate(bad):
    """a candidate of M or -1: ValueError from the wrapper; at the C level rank -1 for exactly the queries that hold one and NaN for
    that score, the other queries as if nothing had happened.  The index is compared before it is ever part of an address."""
    N, M, D, R = 9, 12, 40, 5
    g = torch.Generator().manual_seed(7)
    q, bank = torch.randn(N, D, generator=g), torch.randn(M, D, generator=g)
    cand = torch.rand(N, M, generator=g).argsort(1)[:, :R].to(torch.int32).contiguous()
    good_rank, good_scores = HF.retrieval_rank(q.to(DEV), bank.to(DEV), cand.to(DEV), want_scores=True)
    broken = cand.clone()
    broken[2, 3] = M if bad == "M" else -1
    broken[7, 0] = M if bad == "M" else -1
    with pytest.raises(ValueError):
        HF.retrieval_rank(q.to(DEV), bank.to(DEV), broken.to(DEV))
    qd, bd, cd = q.to(DEV), bank.to(DEV), broken.to(DEV)
    rank = torch.empty(N, dtype=torch.int32, device=DEV)
    scores = torch.empty(N, R, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    L.call("agan_retrieval_rank", p(qd), p(bd), p(cd), N, M, D, R, p(scores), p(rank), None)
    torch.cuda.synchronize()
    rank, scores = rank.cpu(), scores.cpu()
    assert rank[2] == -1 and rank[7] == -1
    ok = [i for i in range(N) if i not in (2, 7)]
    assert torch.equal(rank[ok], good_rank.cpu()[ok]) and torch.equal(scores[ok], good_scores.cpu()[ok])
    assert bool(torch.isnan(scores[2, 3])) and bool(torch.isnan(scores[7, 0]))
    keep = torch.ones(R, dtype=torch.bool)
    keep[3] = False
    assert torch.equal(scores[2][keep], good_scores.cpu()[2][keep])


def test_retrieval_bad_arguments():
    q, bank = torch.zeros(4, 8, device=DEV), torch.zeros(5, 8, device=DEV)
    cand = torch.zeros(4, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        HF.retrieval_rank(q, bank[:, :4], cand)
    with pytest.raises(ValueError):
        HF.retrieval_rank(q, bank, cand.long())
    with pytest.raises(ValueError):
        HF.retrieval_rank(q, bank, cand[:3])
    with pytest.raises(ValueError):
        HF.retrieval_rank(q, bank, torch.zeros(4, 1025, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        HF.retrieval_rank(q, bank.cpu(), cand)


# ------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

E2E_R, E2E_FOLDS, E2E_SEED, E2E_BATCH = 4, 2, 3, 8


@functools.lru_cache(maxsize=None)
def e2e_setup():
    torch.manual_seed(21)
    G = GEN.Generator(4, 16, 8, 8).to(DEV)
    cnn = ENC.CNNEncoder(16, backend="hip").to(DEV).eval()
    cnn.freeze_all_weights()
    g = torch.Generator().manual_seed(22)
    batches = []
    for b in range(2):
        lengths = torch.randint(2, 7, (E2E_BATCH,), generator=g)
        lengths[0] = 6
        words = torch.randint(1, 20, (E2E_BATCH, 6), generator=g)
        class_ids = (torch.arange(E2E_BATCH) + b) % 4
        imgs = [torch.rand(E2E_BATCH, 3, r, r, generator=g) * 2 - 1 for r in (64, 128, 256)]
        batches.append((words, lengths, class_ids, *imgs))
    return G, cnn, batches


@functools.lru_cache(maxsize=None)
def e2e_text_encoder(backend):
    torch.manual_seed(23)
    return RNN.RNNEncoder(20, embdim=12, nhidden=16, bidirectional=False, backend=backend).to(DEV)


@functools.lru_cache(maxsize=None)
def e2e_real():
    G, cnn, batches = e2e_setup()
    return EV.Evaluator(G, e2e_text_encoder("torch"), cnn, DEV).real_moments(batches)


@pytest.mark.parametrize("text_backend", ["torch", "hip"])
def test_evaluator_matches_a_plain_restatement(text_backend):
    G, cnn, batches = e2e_setup()
    rnn = e2e_text_encoder(text_backend)
    ev = EV.Evaluator(G, rnn, cnn, DEV)
    real = e2e_real()
    out = ev.evaluate(batches, real, 16, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS)
    again = ev.evaluate(batches, real, 16, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS)
    assert out["n"] == 16 and len(out["r_precision_folds"]) == E2E_FOLDS
    assert out["fid"] == again["fid"] and out["r_precision"] == again["r_precision"] and torch.equal(out["rank"], again["rank"])
    assert out["r_precision_folds"] == again["r_precision_folds"]
    assert G.training and rnn.training, "evaluate must restore the modules' modes"

    # the same modules called directly; moments by torch.cov and ranks by the float64 cosine, on the host
    rng = torch.Generator(device=DEV)
    rng.manual_seed(E2E_SEED)
    masks = TR.ModelTrainer()
    G.eval(), rnn.eval()
    try:
        with torch.no_grad():
            codes, sents, pooled, real_pooled, cids = [], [], [], [], []
            for words, lengths, class_ids, _i64, _i128, i256 in batches:
                w, s = rnn(words.to(DEV), lengths)
                noise = torch.randn(E2E_BATCH, 8, device=DEV, generator=rng)
                eps = torch.randn(E2E_BATCH, 8, device=DEV, generator=rng)
                fakes, _, _, _ = G(noise, s.contiguous(), w.contiguous(), masks._make_mask(lengths.tolist(), w.shape[2]).to(DEV), eps)
                codes.append(cnn(fakes[-1])[1].cpu())
                pooled.append(cnn.pooled(fakes[-1]).cpu())
                real_pooled.append(cnn.pooled(i256.to(DEV)).cpu())
                sents.append(s.cpu())
                cids.append(class_ids)
    finally:
        G.train(), rnn.train()
    codes, sents, pooled, real_pooled, cids = (torch.cat(t) for t in (codes, sents, pooled, real_pooled, cids))
    p64, r64 = pooled.double(), real_pooled.double()
    want_fid = EV.frechet_distance(r64.mean(0), torch.cov(r64.t()), p64.mean(0), torch.cov(p64.t()))
    print(f"fid {out['fid']:.12g}, restated {want_fid:.12g}")
    assert abs(out["fid"] - want_fid) <= 1e-6 * abs(want_fid)

    cand = EV.draw_mismatched(cids, E2E_R, E2E_SEED)
    assert not bool((cids[cand[:, 1:].long()] == cids.view(-1, 1)).any())
    s64 = cosine64(codes, sents, cand)
    tau = (2 * 16 + 8) * U
    lo = (s64[:, 1:] > s64[:, :1] + 2 * tau).sum(1)
    hi = (s64[:, 1:] >= s64[:, :1] - 2 * tau).sum(1)
    sure = lo == hi
    assert int(sure.sum()) >= 12, "too few unambiguous rows for the comparison to mean anything"
    rank = out["rank"].cpu().long()
    assert torch.equal(rank[sure], lo[sure])
    assert bool(((rank >= lo) & (rank <= hi)).all())
    hit = (rank == 0).double()
    assert out["r_precision"] == float(hit.mean())
    assert out["r_precision_folds"] == [float(hit[:8].mean()), float(hit[8:].mean())]


def test_evaluator_real_images_against_themselves():
    G, cnn, batches = e2e_setup()
    real = e2e_real()
    assert real.count == 16
    out = EV.Evaluator(G, e2e_text_encoder("torch"), cnn, DEV).evaluate(batches, real, 16, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS,
                                                                       source="real")
    trace = float(torch.trace(real.cov()))
    print(f"self-distance {out['fid']:.3g}, tr S {trace:.3g}")
    assert abs(out["fid"]) <= 1e-6 * (trace + 1.0)


def test_train_step_evaluate_is_the_evaluator():
    G, cnn, batches = e2e_setup()
    rnn = e2e_text_encoder("torch")
    real = e2e_real()
    want = EV.Evaluator(G, rnn, cnn, DEV).evaluate(batches, real, 12, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS)
    step = TR.GanTrainStep(G, [DISC.Disc64(4).to(DEV), DISC.Disc128(4).to(DEV), DISC.Disc256(4).to(DEV)], cnn)
    got = step.evaluate(batches, rnn, real, 12, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS)
    assert got["n"] == want["n"] == 12
    assert got["fid"] == want["fid"] and got["r_precision"] == want["r_precision"] and torch.equal(got["rank"], want["rank"])
