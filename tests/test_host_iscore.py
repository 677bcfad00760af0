"""CPU checks of the Inception Score (evaluation.py: inception_score_reference, inception_score, Evaluator.evaluate(inception_splits=...);
the float64 CPU path of functional.inception_split_scores; the classifier head of networks.CNNEncoder; the C ABI's declarations and
argument checks) -- no GPU needed.

The reference against the published code.  `published` below restates the protocol as it is usually written (softmax; kl = p (log p -
log mean p); exp(mean(sum)) per chunk) in float64 numpy.  Both sides evaluate the same quantity in float64 by different routes, so they
differ by rounding only; with u = 2^-53 and eps = (2 C + n_s + 4 max|l| + 32) u (n_s the largest split) each side is within
2 (log C + 1) eps relative of the true IS (the derivation is in tests/test_gpu_iscore.py), and the two within 4 (log C + 1) eps of each other.
"""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")
EV = importlib.import_module("attention-gan_amd.evaluation")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")

NEW_SYMBOLS = {"agan_inception_score_ws_bytes": 3, "agan_inception_score": 8}
U53 = 2.0 ** -53


def test_new_symbols_are_declared_and_bound_with_matching_arity():
    header = open(os.path.join(ROOT, "include", "agan.h")).read()
    assert "#define AGAN_VERSION 101" in header
    for name, arity in NEW_SYMBOLS.items():
        m = re.search(rf"\b{name}\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/agan.h"
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert len(args.split(",")) == arity, f"{name}: {args}"
        assert name in L.EXPORTED_SYMBOLS
        assert len(L._SIGNATURES[name][1]) == arity, f"{name}: bound with {len(L._SIGNATURES[name][1])} arguments"
        assert hasattr(L.load(), name), f"{name} is not exported by the library"
    srcs = re.search(r"^SRCS\s*:=(.*)$", open(os.path.join(ROOT, "attention-gan_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "iscore.hip" in srcs.split()


def test_entry_points_validate_before_touching_the_device():
    lib = L.load()
    P = 16                                  # a non-null dummy pointer value: validation must fail before it is used
    BIG = 1 << 40
    q = lib.agan_inception_score_ws_bytes
    assert q(0, 10, 1) == 0 and q(10, 0, 1) == 0 and q(10, 4097, 1) == 0
    assert q(1 << 20, 2048, 10) == 0                                                    # N * C = 2^31
    assert q(10, 8, 0) == 0 and q(10, 8, 11) == 0 and q(5000, 8, 1025) == 0
    assert q(10, 8, 10) >= 2 * 10 * 8 and q(1030, 8, 1024) > 0 and q(1, 4096, 1) > 0
    # the edge of the domain at C = 1: ceilings of N must not wrap (N + 63 does not fit an int).  The workspace holds two doubles per
    # row (lse, t), one partial per (split, piece of 64 rows) and one term per split
    for N in ((1 << 31) - 1, (1 << 31) - 4, (1 << 31) - 63, (1 << 31) - 64, (1 << 31) - 65):
        for S in (1, 3, 1024):
            pieces = -(-(-(-N // S)) // 64)
            assert q(N, 1, S) >= 16 * N + 8 * S * pieces + 8 * S, (N, S)
            assert q(N, 1, S) <= 16 * N + 8 * S * pieces + 8 * S + 64, (N, S)

    def score(logits=P, N=10, C=8, splits=3, scores=P, ws=P, ws_bytes=BIG):
        return lib.agan_inception_score(logits, N, C, splits, scores, ws, ws_bytes, None)

    for missing in ("logits", "scores", "ws"):
        assert score(**{missing: None}) == L.EINVAL, missing
    assert score(N=0, splits=1) == L.EINVAL
    assert score(C=0) == L.EINVAL and score(C=4097) == L.EINVAL
    assert score(N=1 << 20, C=2048) == L.EINVAL
    assert b"2^31" in lib.agan_last_error()
    assert score(splits=0) == L.EINVAL and score(splits=11) == L.EINVAL                 # splits = N + 1
    assert score(N=5000, splits=1025) == L.EINVAL
    assert b"splits" in lib.agan_last_error()
    assert score(ws_bytes=8) == L.EWORKSPACE
    assert b"workspace" in lib.agan_last_error()


# ------------------------------------------------------------------------------------------------------------------
# the reference against the published code
# ------------------------------------------------------------------------------------------------------------------
def published(logits, splits):
    """the protocol as published, in float64 numpy -> [splits] scores"""
    x = logits.astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    preds = e / e.sum(1, keepdims=True)
    N = preds.shape[0]
    out = []
    for i in range(splits):
        part = preds[i * N // splits:(i + 1) * N // splits]
        kl = part * (np.log(part) - np.log(part.mean(0, keepdims=True)))
        out.append(np.exp(kl.sum(1).mean()))
    return np.array(out)


def bound_eps(N, C, S, max_abs):
    n_s = -(-N // S)
    return (2 * C + n_s + 4 * max_abs + 32) * U53


def gauss_logits(N, C, S, scale=3.0):
    g = torch.Generator().manual_seed(N * 1_000_003 + C * 1009 + S)
    return scale * torch.randn(N, C, generator=g)


@pytest.mark.parametrize("N,C,S", [(103, 7, 10), (1000, 1000, 10), (64, 4096, 3), (10, 1, 10)])
def test_reference_matches_the_published_code(N, C, S):
    l = gauss_logits(N, C, S)
    ref = EV.inception_score_reference(l, S)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (S, 3)
    want = published(l.numpy(), S)
    bound = 4 * (math.log(C) + 1) * bound_eps(N, C, S, float(l.abs().max()))
    err = np.abs(ref[:, 0].numpy() - want) / want
    print(f"({N}, {C}, {S}): worst relative difference {err.max():.3g}, bound {bound:.3g}")
    assert err.max() <= bound
    # IS = exp(Hm - Hc), and both entropies lie in [0, log C]
    assert torch.equal(ref[:, 0], (ref[:, 1] - ref[:, 2]).exp())
    assert bool((ref[:, 1:] >= -1e-15).all()) and bool((ref[:, 1:] <= math.log(C) + 1e-12).all())


# ------------------------------------------------------------------------------------------------------------------
# closed forms
# ------------------------------------------------------------------------------------------------------------------
def one_hot_by_split(N=103, C=12, S=10):
    l = torch.zeros(N, C)
    for s in range(S):
        l[s * N // S:(s + 1) * N // S, s] = 60.0
    return l


def one_hot_cyclic(N=120, C=12):
    l = torch.zeros(N, C)
    l[torch.arange(N), torch.arange(N) % C] = 60.0
    return l


def check_closed_forms(scores_of):
    """scores_of(logits, splits) -> float64 [splits, 3] on the host"""
    C = 1000
    const = scores_of(torch.full((50, C), 1.5), 5)
    assert float((const[:, 0] - 1.0).abs().max()) <= 64 * U53 * math.log(C)
    # every row of split s one-hot on class s: a single row that leaks into a neighbouring split breaks this
    assert bool((scores_of(one_hot_by_split(), 10)[:, 0] == 1.0).all())
    cyc = one_hot_cyclic()
    for S in (1, 10):
        assert float((scores_of(cyc, S)[:, 0] - 12.0).abs().max()) <= 1e-12, f"splits {S}"


def test_closed_forms_reference():
    check_closed_forms(lambda l, S: EV.inception_score_reference(l, S))


def test_closed_forms_cpu_path():
    check_closed_forms(lambda l, S: HF.inception_split_scores(l, S))


@pytest.mark.parametrize("N,C,S", [(103, 7, 10), (300, 130, 4), (10, 1, 10), (1, 5, 1)])
def test_cpu_path_equals_the_reference(N, C, S):
    l = gauss_logits(N, C, S)
    got = HF.inception_split_scores(l, S)
    assert got.dtype == torch.float64 and tuple(got.shape) == (S, 3) and got.device.type == "cpu"
    assert torch.equal(got, EV.inception_score_reference(l, S))


def test_non_finite_rows_on_the_cpu():
    l = gauss_logits(100, 9, 10)
    clean = EV.inception_score_reference(l, 10)
    masked = l.clone()
    masked[:, 4] = float("-inf")
    out = EV.inception_score_reference(masked, 10)
    assert bool(torch.isfinite(out).all())
    assert torch.allclose(out, EV.inception_score_reference(masked[:, [0, 1, 2, 3, 5, 6, 7, 8]], 10), rtol=1e-13, atol=0)
    for bad in (float("nan"), float("inf")):
        broken = l.clone()
        broken[35, 2] = bad
        for fn in (EV.inception_score_reference, HF.inception_split_scores):
            out = fn(broken, 10)
            assert bool(torch.isnan(out[3]).all())
            keep = [s for s in range(10) if s != 3]
            assert torch.equal(out[keep], clean[keep])
    empty = l.clone()
    empty[35] = float("-inf")
    assert bool(torch.isnan(EV.inception_score_reference(empty, 10)[3]).all())


def test_inception_score_dict_and_argument_errors():
    l = gauss_logits(103, 7, 10)
    out = EV.inception_score(l, 10)
    assert set(out) == {"inception_score", "inception_score_std", "inception_score_splits", "label_entropy", "conditional_entropy"}
    ref = EV.inception_score_reference(l, 10).numpy()
    assert out["inception_score_splits"] == ref[:, 0].tolist()
    assert out["inception_score"] == pytest.approx(ref[:, 0].mean(), rel=1e-15)
    assert out["inception_score_std"] == pytest.approx(np.std(ref[:, 0]), rel=1e-12)
    assert out["label_entropy"] == pytest.approx(ref[:, 1].mean(), rel=1e-15)
    assert out["conditional_entropy"] == pytest.approx(ref[:, 2].mean(), rel=1e-15)
    assert EV.inception_score(l.double(), 10) == out, "any float dtype is reduced from float32"
    for fn in (EV.inception_score, EV.inception_score_reference):
        for bad in (0, 104, 1025, 2.5):
            with pytest.raises(ValueError):
                fn(l, bad)
        with pytest.raises(ValueError):
            fn(l.view(-1), 1)
        with pytest.raises(ValueError):
            fn(l.view(103, 7, 1), 1)
    with pytest.raises(ValueError):
        HF.inception_split_scores(l.double(), 10)
    with pytest.raises(ValueError):
        HF.inception_split_scores(l.view(103, 7, 1), 10)
    with pytest.raises(ValueError):
        HF.inception_split_scores(l, 104)
    with pytest.raises(ValueError):
        HF.inception_split_scores(torch.zeros(2, 4097), 1)


# ------------------------------------------------------------------------------------------------------------------
# the loop
# ------------------------------------------------------------------------------------------------------------------
class StubGenerator(nn.Module):
    z_dim, cond_dim = 4, 4

    def __init__(self):
        super().__init__()
        self.proj = nn.Linear(4 + 4 + 6, 3 * 8 * 8)

    def forward(self, noise, sent, words, mask, eps):
        img = torch.tanh(self.proj(torch.cat([noise, eps, sent + (words * mask.unsqueeze(1)).sum(2)], 1))).view(-1, 3, 8, 8)
        return [img[:, :, ::4, ::4], img[:, :, ::2, ::2], img], None, None, None


class StubImageEncoder(nn.Module):
    """code_and_pooled only: no classifier head"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(8)
        self.code = nn.Parameter(torch.randn(192, 6, generator=g))
        self.pool = nn.Parameter(torch.randn(192, 10, generator=g))

    def code_and_pooled(self, x):
        flat = x.flatten(1)
        return flat @ self.code, torch.relu(flat @ self.pool)


class StubClassifier(StubImageEncoder):
    def __init__(self):
        super().__init__()
        self.head = nn.Parameter(torch.randn(10, 5, generator=torch.Generator().manual_seed(9)))

    def logits(self, pooled):
        return pooled @ self.head


class StubTextEncoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = nn.Embedding(30, 6)

    def forward(self, words, lengths):
        w = self.emb(words).transpose(1, 2)                                              # [B, 6, T]
        return w, w.mean(2)


def _stub_batches(seed=9, rows=(6, 6, 6, 4)):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b, n in enumerate(rows):
        lengths = torch.randint(2, 6, (n,), generator=g)
        lengths[0] = 5
        imgs = [torch.rand(n, 3, r, r, generator=g) * 2 - 1 for r in (2, 4, 8)]
        out.append((torch.randint(0, 30, (n, 5), generator=g), lengths, (torch.arange(n) + b) % 3, *imgs))
    return out


def test_evaluate_with_inception_splits():
    torch.manual_seed(10)
    G, txt = StubGenerator(), StubTextEncoder()
    plain_enc, enc = StubImageEncoder(), StubClassifier()
    batches = _stub_batches()
    ev = EV.Evaluator(G, txt, enc, "cpu")
    real = ev.real_moments(batches)
    old = ev.evaluate(batches, real, 100, R=3, seed=7, folds=2)
    assert set(old) == {"r_precision", "r_precision_folds", "rank", "fid", "n"}
    new = ev.evaluate(batches, real, 100, R=3, seed=7, folds=2, inception_splits=3)
    assert set(new) == set(old) | {"inception_score", "inception_score_std", "inception_score_splits", "label_entropy", "conditional_entropy"}
    assert new["fid"] == old["fid"] and torch.equal(new["rank"], old["rank"]) and new["n"] == old["n"] == 18
    assert len(new["inception_score_splits"]) == 3 and 1.0 - 1e-12 <= new["inception_score"] <= 5.0 + 1e-12
    # the real images' score is the score of their own logits
    own = ev.evaluate(batches, real, 100, R=3, seed=7, folds=2, source="real", inception_splits=2)
    with torch.no_grad():
        want = EV.inception_score(torch.cat([enc.logits(enc.code_and_pooled(b[5])[1]) for b in batches[:3]]), 2)
    assert {k: own[k] for k in want} == want
    # argument errors
    with pytest.raises(ValueError, match="logits"):
        EV.Evaluator(G, txt, plain_enc, "cpu").evaluate(batches, real, 100, R=3, inception_splits=3)
    with pytest.raises(ValueError):
        ev.evaluate(batches, real, 100, R=3, inception_splits=19)                       # 18 rows are kept
    with pytest.raises(ValueError):
        ev.evaluate(batches, real, 100, R=3, inception_splits=0)
    with pytest.raises(ValueError):
        ev.evaluate(batches, real, 100, R=3, inception_splits=2.5)


# ------------------------------------------------------------------------------------------------------------------
# the classifier head
# ------------------------------------------------------------------------------------------------------------------
def test_cnn_encoder_default_is_unchanged_and_the_head_comes_last():
    torch.manual_seed(7)
    old = ENC.CNNEncoder()
    torch.manual_seed(7)
    explicit = ENC.CNNEncoder(num_classes=None)
    torch.manual_seed(7)
    headed = ENC.CNNEncoder(num_classes=10)
    old_sd, headed_sd = old.state_dict(), headed.state_dict()
    assert list(explicit.state_dict()) == list(old_sd) and not hasattr(old, "fc")
    assert not any(k.startswith("fc.") for k in old_sd)
    assert list(headed_sd) == list(old_sd) + ["fc.weight", "fc.bias"]
    for k, v in old_sd.items():
        assert torch.equal(v, headed_sd[k]), k
    assert tuple(headed.fc.weight.shape) == (10, 2048) and tuple(headed.fc.bias.shape) == (10,)
    assert not headed.fc.weight.requires_grad and not headed.fc.bias.requires_grad
    assert [n for n, p in headed.named_parameters() if p.requires_grad] == [n for n, p in old.named_parameters() if p.requires_grad]
    with pytest.raises(ValueError):
        ENC.CNNEncoder(num_classes=0)


def test_head_loads_and_logits():
    torch.manual_seed(3)
    enc = ENC.CNNEncoder(num_classes=10)
    g = torch.Generator().manual_seed(4)
    w, b = torch.randn(10, 2048, generator=g), torch.randn(10, generator=g)
    stem = torch.randn_like(enc.Conv2d_1a_3x3.conv.weight)
    code_before = enc.emb_cnn_code.weight.clone()
    enc.load_trunk_state_dict({"fc.weight": w, "fc.bias": b, "Conv2d_1a_3x3.conv.weight": stem, "AuxLogits.fc.bias": torch.zeros(10),
                               "emb_cnn_code.weight": torch.zeros(256, 2048)})
    assert torch.equal(enc.fc.weight, w) and torch.equal(enc.fc.bias, b) and torch.equal(enc.Conv2d_1a_3x3.conv.weight, stem)
    assert torch.equal(enc.emb_cnn_code.weight, code_before)
    with pytest.raises(ValueError) as err:
        enc.load_trunk_state_dict({"fc.weight": torch.zeros(200, 2048), "fc.bias": torch.zeros(200)})
    assert "(200, 2048)" in str(err.value) and "(10, 2048)" in str(err.value)
    assert torch.equal(enc.fc.weight, w), "a refused load must leave the head alone"
    # a head-less encoder ignores fc.* as before
    plain = ENC.CNNEncoder()
    plain.load_trunk_state_dict({"fc.weight": w, "fc.bias": b, "Conv2d_1a_3x3.conv.weight": stem})
    assert torch.equal(plain.Conv2d_1a_3x3.conv.weight, stem) and not hasattr(plain, "fc")

    pooled = torch.randn(5, 2048, generator=g)
    with pytest.raises(RuntimeError):
        enc.logits(pooled)                                                              # train mode
    with pytest.raises(ValueError):
        plain.eval().logits(pooled)
    with pytest.raises(ValueError):
        plain.train().logits(pooled)
    enc.eval()
    with torch.no_grad():
        assert torch.equal(enc.logits(pooled), torch.nn.functional.linear(pooled, w, b))
