"""CPU tests of the word-level discriminator (ControlGAN section 3.2): the plain-torch statement of the score
(backend.functional.word_corr_reference) against autograd's gradcheck and against the properties include/agan.h states, the module
(networks.discriminators.WordLevelDisc) on CPU tensors, the refusals of the Python layers, and the argument checks of the four C entries
(agan_word_corr_*), which answer before any device is touched."""
import importlib

import pytest
import torch

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

B, D, S, T = 2, 5, 6, 4
LENS = torch.tensor([4, 2])


def _inputs(dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    regions = (torch.randn(B, D, S, generator=g, dtype=torch.float64) * D ** -0.25).to(dtype)
    words = (torch.randn(B, D, T, generator=g, dtype=torch.float64) * D ** -0.25).to(dtype)
    return regions, words


def test_reference_passes_gradcheck_in_float64():
    regions, words = _inputs()
    regions.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: HF.word_corr_reference(x, words, LENS, 1)[0], (regions,))


@pytest.mark.parametrize("shift", [0, 1])
def test_reference_weights_sum_to_one_and_scores_are_probabilities(shift):
    regions, words = _inputs()
    p, r, g = HF.word_corr_reference(regions, words, LENS, shift)
    assert p.shape == (B,) and r.shape == (B, T) and g.shape == (B, T)
    assert bool(((p > 0) & (p < 1)).all())
    for b in range(B):
        Lc = int(LENS[(b + shift) % B])
        assert abs(float(g[b, :Lc].sum()) - 1.0) < 1e-12 and bool((g[b, :Lc] > 0).all())
        assert bool((g[b, Lc:] == 0).all()) and bool((r[b, Lc:] == 0).all())
        assert bool((r[b, :Lc].abs() <= 1 + 1e-12).all())


def test_reference_never_reads_words_beyond_the_length():
    regions, words = _inputs()
    poisoned = words.clone()
    poisoned[1, :, 2:] = float("nan")
    for shift in (0, 1):
        for a, b in zip(HF.word_corr_reference(regions, words, LENS, shift), HF.word_corr_reference(regions, poisoned, LENS, shift)):
            assert torch.equal(a, b)


def test_shift_one_is_shift_zero_on_rolled_captions():
    regions, words = _inputs()
    for a, b in zip(HF.word_corr_reference(regions, words, LENS, 1), HF.word_corr_reference(regions, words.roll(-1, 0), LENS.roll(-1), 0)):
        assert torch.equal(a, b)


def test_weighting_the_context_before_the_cosine_changes_nothing():
    """why the departure exists: the paper multiplies ctx_l by the self-attention weight BEFORE the cosine, which is scale-invariant"""
    regions, words = _inputs()
    _, r, g = HF.word_corr_reference(regions, words, LENS, 0)
    for b in range(B):
        Lc = int(LENS[b])
        w, n = words[b, :, :Lc].t(), regions[b]
        alpha = torch.softmax(4.0 * torch.softmax(w @ n, dim=0), dim=1)
        ctx = (alpha @ n.t()) * g[b, :Lc, None]                       # the paper's order
        cos = (ctx * w).sum(1) / (ctx.norm(dim=1) * w.norm(dim=1)).clamp(min=1e-8)
        assert float((cos - r[b, :Lc]).abs().max()) < 1e-12
        assert float(g[b, :Lc].max() - g[b, :Lc].min()) > 1e-3        # (the weights are not uniform: they would matter if they could)


def test_module_key_identity_init_and_cpu_forward():
    torch.manual_seed(0)
    d = DISC.WordLevelDisc(D)
    assert list(d.state_dict()) == ["perception.weight"]
    assert torch.equal(d.perception.weight.detach(), torch.eye(D).view(D, D, 1, 1))
    assert [k for k, _ in d.named_parameters()] == ["perception.weight"]
    regions, words = _inputs(torch.float32)
    maps = regions.view(B, D, 2, 3)
    for shift in (0, 1):
        p, r, g = d.correlations(maps, words, LENS, shift)
        want = HF.word_corr_reference(regions, words, LENS, shift, 4.0, 5.0)
        assert torch.equal(d(maps, words, LENS, shift), p)
        for a, b in zip((p, r, g), want):
            assert torch.allclose(a, b, rtol=0, atol=1e-6)
    # a non-identity perception layer is applied to the image side
    with torch.no_grad():
        d.perception.weight.copy_(torch.randn(D, D, 1, 1))
    n = torch.einsum("oc,bcs->bos", d.perception.weight.detach().view(D, D), regions)
    want = HF.word_corr_reference(n, words, LENS, 0, 4.0, 5.0)[0]
    assert torch.allclose(d(maps, words, LENS), want, rtol=0, atol=1e-6)
    p = d(maps, words, LENS)
    p.sum().backward()
    assert d.perception.weight.grad is not None and float(d.perception.weight.grad.abs().max()) > 0


def test_losses_follow_their_formulas_on_cpu():
    DL = importlib.import_module("attention-gan_amd.losses.disc_loss")
    GL = importlib.import_module("attention-gan_amd.losses.gen_loss")
    d = DISC.WordLevelDisc(D)
    regions, words = _inputs(torch.float32)
    real, fake = regions.view(B, D, 2, 3), regions.flip(0).view(B, D, 2, 3) * 0.7
    p_rc, p_rw, p_f = d(real, words, LENS, 0), d(real, words, LENS, 1), d(fake, words, LENS, 0)
    want_d = (-torch.log(p_rc + 1e-8)).mean() + ((-torch.log(1 - p_rw + 1e-8)).mean() + (-torch.log(1 - p_f + 1e-8)).mean()) / 2
    assert torch.allclose(DL.WordLevelDiscLoss().get_loss(d, fake, real, words, LENS), want_d, rtol=1e-6, atol=0)
    assert torch.allclose(GL.WordLevelGenLoss().get_loss(d, fake, words, LENS), (-torch.log(p_f + 1e-8)).mean(), rtol=1e-6, atol=0)


def test_words_that_require_grad_are_refused():
    regions, words = _inputs(torch.float32)
    words.requires_grad_(True)
    with pytest.raises(ValueError, match="constants"):
        HF.word_corr_reference(regions, words, LENS)
    with pytest.raises(ValueError, match="constants"):
        HF.word_corr(regions, words, LENS)
    with pytest.raises(ValueError, match="constants"):
        DISC.WordLevelDisc(D)(regions.view(B, D, 2, 3), words, LENS)


def test_python_layer_refuses_bad_arguments():
    regions, words = _inputs(torch.float32)
    for shift in (-1, B, 1.0, True):
        with pytest.raises(ValueError, match="shift"):
            HF.word_corr_reference(regions, words, LENS, shift)
    with pytest.raises(ValueError, match="words must be"):
        HF.word_corr_reference(regions, words[:, :3], LENS)
    with pytest.raises(ValueError, match="word_corr_reference runs anywhere"):
        HF.word_corr(regions, words, LENS)                               # CPU tensors: the kernels do not run there


def test_trainer_refuses_a_word_disc_without_image_encoder():
    G = GEN.Generator(8, 32, 16, 16)
    Ds = [DISC.Disc64(8)]
    with pytest.raises(ValueError, match="image_encoder"):
        TR.GanTrainStep(G, Ds, None, word_disc=DISC.WordLevelDisc(32))


# ---------------------------------------------------------------------------------------------- the C entries' argument checks
P = 1                       # a non-null dummy pointer value: validation must fail before it is used
GOOD = (4, 64, 12, 289)     # B, D, T, S inside every range
BAD = [(0, 64, 12, 289), (-3, 64, 12, 289), (129, 64, 12, 289), (4, 0, 12, 289), (4, -1, 12, 289), (4, 321, 12, 289),
       (4, 64, 0, 289), (4, 64, -2, 289), (4, 64, 33, 289), (4, 64, 12, 0), (4, 64, 12, -17), (4, 64, 12, 321)]


def corr_fwd(lib, dims, shift=0, regions=P, words=P, lens=P, p=P, r=P, g=P, save=P):
    return lib.agan_word_corr_fwd(regions, words, lens, shift, 4.0, 5.0, 1e-8, p, r, g, save, *dims, None)


def corr_bwd(lib, dims, shift=0, regions=P, words=P, lens=P, save=P, dp=P, dregions=P):
    return lib.agan_word_corr_bwd(regions, words, lens, shift, save, dp, 4.0, 5.0, 1e-8, dregions, *dims, None, 0, None)


@pytest.mark.parametrize("dims", BAD, ids=lambda d: "B{}-D{}-T{}-S{}".format(*d))
def test_entries_refuse_out_of_range_shapes(dims):
    lib = L.load()
    assert corr_fwd(lib, dims) == L.EINVAL
    assert b"word_corr_fwd" in lib.agan_last_error()
    assert corr_bwd(lib, dims) == L.EINVAL
    assert b"word_corr_bwd" in lib.agan_last_error()
    assert corr_fwd(lib, GOOD, regions=None) == L.EINVAL            # (leaves another message behind)
    assert lib.agan_word_corr_save_elems(*dims) == 0
    assert b"word_corr_save_elems" in lib.agan_last_error()
    assert corr_fwd(lib, GOOD, regions=None) == L.EINVAL
    assert lib.agan_word_corr_bwd_ws_bytes(*dims) == 0
    assert b"word_corr_bwd_ws_bytes" in lib.agan_last_error()


@pytest.mark.parametrize("shift", [-1, 4, 5, 1 << 20])
def test_entries_refuse_a_shift_outside_the_batch(shift):
    lib = L.load()
    assert corr_fwd(lib, GOOD, shift) == L.EINVAL
    assert b"word_corr_fwd: shift" in lib.agan_last_error()
    assert corr_bwd(lib, GOOD, shift) == L.EINVAL
    assert b"word_corr_bwd: shift" in lib.agan_last_error()


def test_entries_refuse_null_pointers():
    lib = L.load()
    for missing in ("regions", "words", "lens", "p", "r", "g", "save"):
        assert corr_fwd(lib, GOOD, **{missing: None}) == L.EINVAL
        assert b"word_corr_fwd: null pointer" in lib.agan_last_error()
    for missing in ("regions", "words", "lens", "save", "dp", "dregions"):       # (the workspace is empty: `ws` may be null)
        assert corr_bwd(lib, GOOD, **{missing: None}) == L.EINVAL
        assert b"word_corr_bwd: null pointer" in lib.agan_last_error()


def test_size_queries_inside_the_range():
    lib = L.load()
    Bq, Dq, Tq, Sq = GOOD
    assert lib.agan_word_corr_save_elems(Bq, Dq, Tq, Sq) == Bq * 5 * Tq      # per-word statistics only: no [T, S] map is stored
    assert lib.agan_word_corr_save_elems(128, 320, 32, 320) == 128 * 5 * 32
    assert lib.agan_word_corr_bwd_ws_bytes(Bq, Dq, Tq, Sq) == 0
    assert lib.agan_word_corr_bwd_ws_bytes(128, 320, 32, 320) == 0
