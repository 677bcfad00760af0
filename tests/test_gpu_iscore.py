"""agan_inception_score (csrc/iscore.hip), the classifier head of CNNEncoder(backend="hip") and Evaluator.evaluate(inception_splits=...) on the
GPU against float64 on the CPU.

Shapes.  The kernels' tiling is: a row pass with one wave per row, four rows per workgroup, the row in registers as 1, 2, 4, 8 or 16 float4
groups per lane (C <= 256, 512, 1024, 2048, 4096), 16-byte loads for C % 4 == 0 and 4-byte loads otherwise; a column pass over class chunks
of 256 and PIECES of 64 rows counted from each split's first row; a class pass over chunks of 64 classes; a finish whose 256 threads
stride over the classes and over the split's rows.
  C from (1, 3, 63, 64, 65, 200, 256, 257, 260, 516, 1000, 1002, 2052, 4096): below a wave, either side of 64 (one group per lane, partly
    filled), 256 = one full group and one full class chunk, 257 / 260 = the first column of the second group and class chunk on the 4-byte /
    the 16-byte path, 516 and 2052 = the lower edges of the 4- and 16-group forms, 1000 against 1002 = the 16-byte path on and off in the
    4-group form, 4096 = the cap.
  N from (1, 10, 103, 1000) -- below a workgroup of the row pass, a ragged last workgroup, irregular split boundaries, and splits of
    more than 256 rows (the finish's stride) -- plus the piece edges: a largest split of 63, 64 and 65 rows (N = 63 and 65 with one
    split; N = 191 and 193 with three, whose splits are 63, 64, 64 and 64, 64, 65 rows) and 200 rows in one split (four pieces, the last
    of 8 rows).
  splits from (1, 3, 10, N), those that fit min(N, 1024).

Bound against evaluation.inception_score_reference in float64 on the CPU.  u = 2^-53, eps = (2 C + n_s + 4 max|l| + 32) u with n_s the
largest split: lse is a sum of C terms and its absolute error enters every p as a relative one, together with (|l| + |lse|) u from the
subtraction; q and Hc are sums of at most n_s and n_s C non-negative terms (no cancellation); Hm moves by at most (Hm + 1) eps.  With
Hm, Hc <= log C:  |Hm - ref|, |Hc - ref| <= 2 (log C + 1) eps  and  |IS - ref| / ref <= 4 (log C + 1) eps.
Every bounded comparison prints its worst error / bound per quantity.
"""
import functools
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

HF = importlib.import_module("attention-gan_amd.backend.functional")
EV = importlib.import_module("attention-gan_amd.evaluation")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

U53 = 2.0 ** -53
CS = (1, 3, 63, 64, 65, 200, 256, 257, 260, 516, 1000, 1002, 2052, 4096)
NS = (1, 10, 103, 1000)
PIECE_CASES = [(63, 64, 1), (65, 64, 1), (191, 65, 3), (193, 257, 3), (200, 1000, 1), (200, 3, 1), (65, 1002, 1), (193, 4096, 3)]    # (N, C, splits)
IS_KEYS = ("inception_score", "inception_score_std", "inception_score_splits", "label_entropy", "conditional_entropy")


def splits_for(N):
    return sorted({s for s in (1, 3, 10, N) if s <= min(N, 1024)})


@functools.lru_cache(maxsize=None)
def gauss_logits(N, C, scale=3.0):
    g = torch.Generator().manual_seed((N * 1_000_003 + C) * 1009 + int(scale))
    return scale * torch.randn(N, C, generator=g)


def device_scores(l, S):
    return HF.inception_split_scores(l.to(DEV), S)


def check_bound(l, S, got=None, what=""):
    """compares the device's [S, 3] with the float64 reference under the bound of the docstring; returns the device tensor"""
    N, C = l.shape
    got = device_scores(l, S) if got is None else got
    assert got.dtype == torch.float64 and tuple(got.shape) == (S, 3) and got.device.type == "cuda"
    ref = EV.inception_score_reference(l, S)
    finite = l[torch.isfinite(l)]
    eps = (2 * C + -(-N // S) + 4 * float(finite.abs().max()) + 32) * U53
    b_h, b_is = 2 * (math.log(C) + 1) * eps, 4 * (math.log(C) + 1) * eps
    g = got.cpu()
    assert bool(torch.isfinite(g).all()), f"{what} ({N}, {C}, {S}): non-finite scores"
    e_is = float(((g[:, 0] - ref[:, 0]).abs() / ref[:, 0]).max())
    e_hm, e_hc = float((g[:, 1] - ref[:, 1]).abs().max()), float((g[:, 2] - ref[:, 2]).abs().max())
    print(f"{what}({N}, {C}, {S}): IS err / bound {e_is / b_is:.3g} ({e_is:.3g}), Hm {e_hm / b_h:.3g} ({e_hm:.3g}), Hc {e_hc / b_h:.3g} ({e_hc:.3g})")
    assert e_is <= b_is and e_hm <= b_h and e_hc <= b_h
    return got


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("N", NS)
def test_gauss_grid_within_the_bound(N, C):
    l = gauss_logits(N, C)
    for S in splits_for(N):
        got = check_bound(l, S)
        assert torch.equal(got, device_scores(l, S)), "two runs differ"


@pytest.mark.parametrize("N,C,S", PIECE_CASES)
def test_piece_edges_within_the_bound(N, C, S):
    l = gauss_logits(N, C)
    got = check_bound(l, S)
    assert torch.equal(got, device_scores(l, S)), "two runs differ"


def test_only_the_max_subtraction_keeps_exp_finite():
    l = gauss_logits(40, 50, scale=3000.0)
    assert float(l.abs().max()) > 5000
    check_bound(l, 2, what="3000 N(0, 1) ")


def test_closed_forms_on_the_device():
    C = 1000
    const = device_scores(torch.full((50, C), 1.5), 5).cpu()
    print(f"constant logits: |IS - 1| {float((const[:, 0] - 1).abs().max()):.3g}, bound {64 * U53 * math.log(C):.3g}")
    assert float((const[:, 0] - 1.0).abs().max()) <= 64 * U53 * math.log(C)
    # N = 103, C = 12, S = 10, every row of split s one-hot on class s: a single row that leaks into a neighbouring split breaks this
    l = torch.zeros(103, 12)
    for s in range(10):
        l[s * 103 // 10:(s + 1) * 103 // 10, s] = 60.0
    assert bool((device_scores(l, 10)[:, 0] == 1.0).all())
    l = torch.zeros(120, 12)
    l[torch.arange(120), torch.arange(120) % 12] = 60.0
    for S in (1, 10):
        got = device_scores(l, S).cpu()
        print(f"one-hot on k mod 12, {S} splits: |IS - 12| {float((got[:, 0] - 12).abs().max()):.3g}")
        assert float((got[:, 0] - 12.0).abs().max()) <= 1e-12


@pytest.mark.parametrize("N,C,S", [(103, 7, 10), (1000, 1000, 10)])
def test_a_split_depends_on_its_own_rows_only(N, C, S):
    l = gauss_logits(N, C).to(DEV)
    whole = HF.inception_split_scores(l, S)
    for s in range(S):
        a, b = s * N // S, (s + 1) * N // S
        alone = HF.inception_split_scores(l[a:b], 1)
        assert torch.equal(alone[0], whole[s]), f"split {s} (rows {a}..{b}) alone differs from its row of the {S}-split call"
        assert torch.equal(HF.inception_split_scores(l[a:b].clone(), 1), alone), "the bits depend on where the rows lie"
    # the same logits 4 bytes off a 16-byte boundary: the 4-byte load path, the same bits
    off = torch.empty(N * C + 1, device=DEV)[1:].view(N, C)
    off.copy_(l)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    assert torch.equal(HF.inception_split_scores(off, S), whole), "the bits depend on the load path"


@pytest.mark.parametrize("N,C", [(100, 9), (130, 1000)])
def test_non_finite_values(N, C):
    l = gauss_logits(N, C)
    clean = device_scores(l, 10)
    masked = l.clone()
    masked[:, C // 2] = float("-inf")
    check_bound(masked, 10, what="a column of -inf ")
    k = 3 * N // 10 + 5                                            # a row of split 3
    for bad in (float("nan"), float("inf")):
        broken = l.clone()
        broken[k, C - 1] = bad
        got = device_scores(broken, 10)
        assert bool(torch.isnan(got[3]).all()), f"{bad}: split 3 must be NaN"
        keep = [s for s in range(10) if s != 3]
        assert torch.equal(got[keep], clean[keep]), f"{bad}: the other splits must not move"
    empty = l.clone()
    empty[k] = float("-inf")
    got = device_scores(empty, 10)
    assert bool(torch.isnan(got[3]).all()) and torch.equal(got[[0, 1, 2, 4, 5, 6, 7, 8, 9]], clean[[0, 1, 2, 4, 5, 6, 7, 8, 9]])


def test_argument_errors_on_device_tensors():
    l = torch.zeros(6, 8, device=DEV)
    with pytest.raises(ValueError):
        HF.inception_split_scores(l.double(), 2)
    with pytest.raises(ValueError):
        HF.inception_split_scores(l.view(6, 8, 1), 2)
    with pytest.raises(ValueError):
        HF.inception_split_scores(l, 7)
    with pytest.raises(ValueError):
        HF.inception_split_scores(l, 0)
    assert tuple(HF.inception_split_scores(l, 6).shape) == (6, 3)


# ------------------------------------------------------------------------------------------------------------------
# the head
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [200, 1000])
def test_head_logits_on_the_library(C):
    torch.manual_seed(31 + C)
    enc = ENC.CNNEncoder(16, backend="hip", num_classes=C).to(DEV).eval()
    g = torch.Generator().manual_seed(32)
    pooled = torch.randn(5, 2048, generator=g)
    with torch.no_grad():
        got = enc.logits(pooled.to(DEV))
        again = enc.logits(pooled.to(DEV))
    assert tuple(got.shape) == (5, C) and got.dtype == torch.float32 and torch.equal(got, again)
    w, b = enc.fc.weight.detach().cpu().double(), enc.fc.bias.detach().cpu().double()
    want = F.linear(pooled.double(), w, b)
    bound = (2048 + 2) * 2.0 ** -24 * (pooled.double().abs() @ w.abs().t() + b.abs())
    err = (got.cpu().double() - want).abs()
    print(f"head 2048 -> {C}: worst err / bound {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all())
    enc.train()
    with pytest.raises(RuntimeError):
        enc.logits(pooled.to(DEV))


# ------------------------------------------------------------------------------------------------------------------
# the loop
# ------------------------------------------------------------------------------------------------------------------
class StandInClassifier(torch.nn.Module):
    """a small image encoder on the device that offers code_and_pooled and logits"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(41)
        self.code = torch.nn.Parameter(torch.randn(3 * 64, 16, generator=g) * 0.1)
        self.pool = torch.nn.Parameter(torch.randn(3 * 64, 24, generator=g) * 0.1)
        self.head = torch.nn.Parameter(torch.randn(24, 7, generator=g))

    def code_and_pooled(self, x):
        flat = F.adaptive_avg_pool2d(x, 8).flatten(1)
        return flat @ self.code, torch.relu(flat @ self.pool)

    def logits(self, pooled):
        return pooled @ self.head


E2E_R, E2E_FOLDS, E2E_SEED, E2E_BATCH = 4, 2, 3, 8


@functools.lru_cache(maxsize=None)
def e2e_setup():
    torch.manual_seed(21)
    G = GEN.Generator(4, 16, 8, 8).to(DEV)
    enc = StandInClassifier().to(DEV)
    torch.manual_seed(23)
    rnn = RNN.RNNEncoder(20, embdim=12, nhidden=16, bidirectional=False, backend="torch").to(DEV)
    g = torch.Generator().manual_seed(22)
    batches = []
    for b in range(3):
        lengths = torch.randint(2, 7, (E2E_BATCH,), generator=g)
        lengths[0] = 6
        words = torch.randint(1, 20, (E2E_BATCH, 6), generator=g)
        class_ids = (torch.arange(E2E_BATCH) + b) % 4
        imgs = [torch.rand(E2E_BATCH, 3, r, r, generator=g) * 2 - 1 for r in (64, 128, 256)]
        batches.append((words, lengths, class_ids, *imgs))
    real = EV.Evaluator(G, rnn, enc, DEV).real_moments(batches)
    return G, enc, rnn, batches, real


def same_results(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k], k


def test_evaluate_with_inception_splits_matches_a_plain_restatement():
    G, enc, rnn, batches, real = e2e_setup()
    ev = EV.Evaluator(G, rnn, enc, DEV)
    plain = ev.evaluate(batches, real, 24, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS)
    out = ev.evaluate(batches, real, 24, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS, inception_splits=3)
    assert out["n"] == 24 and set(out) == set(plain) | set(IS_KEYS)
    same_results({k: v for k, v in out.items() if k not in IS_KEYS}, plain)

    # the logits of the same fakes from the same seed, by the modules called directly
    rng = torch.Generator(device=DEV)
    rng.manual_seed(E2E_SEED)
    masks = TR.ModelTrainer()
    G.eval(), rnn.eval()
    try:
        with torch.no_grad():
            rows, real_rows = [], []
            for words, lengths, _cls, _i64, _i128, i256 in batches:
                w, s = rnn(words.to(DEV), lengths)
                noise = torch.randn(E2E_BATCH, 8, device=DEV, generator=rng)
                eps = torch.randn(E2E_BATCH, 8, device=DEV, generator=rng)
                fakes, _, _, _ = G(noise, s.contiguous(), w.contiguous(), masks._make_mask(lengths.tolist(), w.shape[2]).to(DEV), eps)
                rows.append(enc.logits(enc.code_and_pooled(fakes[-1])[1]))
                real_rows.append(enc.logits(enc.code_and_pooled(i256.to(DEV))[1]))
    finally:
        G.train(), rnn.train()
    want = EV.inception_score(torch.cat(rows), 3)
    assert {k: out[k] for k in IS_KEYS} == want
    ref = EV.inception_score_reference(torch.cat(rows).float().cpu(), 3)
    assert out["inception_score"] == pytest.approx(float(ref[:, 0].mean()), rel=1e-12)
    assert len(out["inception_score_splits"]) == 3 and 1.0 <= out["inception_score"] <= 7.0

    own = ev.evaluate(batches, real, 20, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS, source="real", inception_splits=2)
    assert {k: own[k] for k in IS_KEYS} == EV.inception_score(torch.cat(real_rows)[:20], 2)
    with pytest.raises(ValueError):
        ev.evaluate(batches, real, 8, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS, inception_splits=9)


def test_train_step_evaluate_forwards_inception_splits():
    G, enc, rnn, batches, real = e2e_setup()
    want = EV.Evaluator(G, rnn, enc, DEV).evaluate(batches, real, 24, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS, inception_splits=3)
    step = TR.GanTrainStep(G, [DISC.Disc64(4).to(DEV), DISC.Disc128(4).to(DEV), DISC.Disc256(4).to(DEV)], enc)
    got = step.evaluate(batches, rnn, real, 24, R=E2E_R, seed=E2E_SEED, folds=E2E_FOLDS, inception_splits=3)
    same_results(got, want)
    assert set(IS_KEYS) <= set(got)
