"""networks.discriminators.WordLevelDisc and the two word-level losses on the device against the float64 statement
(backend.functional.word_corr_reference behind a float64 1x1 perception layer): nef 32, 17 x 17 regions, B 4, T 10, lens (10, 3, 2, 7),
shifts 0 and 1, a non-identity perception weight.  Forward (p, r, g), the gradient at the regions and the gradient of
`perception.weight` are within the project's RTOL = 1e-3 (relative to the tensor's largest float64 value); every measured value is
printed.  Measured on an MI355X: see the docstrings of the tests."""
import importlib

import pytest
import torch

from helpers import RTOL, rel_err

pytestmark = pytest.mark.gpu

HF = importlib.import_module("attention-gan_amd.backend.functional")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
DL = importlib.import_module("attention-gan_amd.losses.disc_loss")
GL = importlib.import_module("attention-gan_amd.losses.gen_loss")

DEV = torch.device("cuda", 0)
NEF, HW, B, T = 32, 17, 4, 10
LENS = [10, 3, 2, 7]


def _inputs(seed=5):
    g = torch.Generator().manual_seed(seed)
    s = NEF ** -0.25
    return dict(real=torch.randn(B, NEF, HW, HW, generator=g) * s, fake=torch.randn(B, NEF, HW, HW, generator=g) * s,
                words=torch.randn(B, NEF, T, generator=g) * s, dp=torch.randn(B, generator=g),
                weight=torch.eye(NEF) + 0.3 * torch.randn(NEF, NEF, generator=g) / NEF ** 0.5)


def _module(weight):
    d = DISC.WordLevelDisc(NEF).to(DEV)
    with torch.no_grad():
        d.perception.weight.copy_(weight.view(NEF, NEF, 1, 1))
    return d


def _f64(weight, regions, words, shift):
    """(p, r, g) of the statement in float64 on the CPU; weight and regions are float64 leaves or plain tensors"""
    n = torch.einsum("oc,bchw->bohw", weight, regions)
    return HF.word_corr_reference(n, words.double(), LENS, shift, 4.0, 5.0)


@pytest.mark.parametrize("shift", [0, 1])
def test_forward_and_backward_against_float64(shift):
    """Measured on an MI355X (shift 0 / shift 1): p 5.5e-8 / 7.5e-8, r 2.1e-7 / 1.5e-7, g 1.6e-7 / 1.6e-7, d regions 1.7e-6 / 1.7e-6,
    d perception.weight 1.7e-6 / 1.4e-6 (the perception conv runs in fp32 on the device, in float64 in the reference)."""
    d_in = _inputs()
    disc = _module(d_in["weight"])
    x = d_in["real"].to(DEV).requires_grad_(True)
    lens = torch.tensor(LENS, dtype=torch.int64, device=DEV)
    p, r, g = disc.correlations(x, d_in["words"].to(DEV), lens, shift)
    assert torch.equal(disc(x, d_in["words"].to(DEV), lens, shift), p)
    (p * d_in["dp"].to(DEV)).sum().backward()
    w64 = d_in["weight"].double().requires_grad_(True)
    x64 = d_in["real"].double().requires_grad_(True)
    p64, r64, g64 = _f64(w64, x64, d_in["words"], shift)
    (p64 * d_in["dp"].double()).sum().backward()
    for what, got, want in (("p", p, p64), ("r", r, r64), ("g", g, g64), ("d regions", x.grad, x64.grad),
                            ("d perception.weight", disc.perception.weight.grad.view(NEF, NEF), w64.grad)):
        e = rel_err(got, want.detach())
        print(f"WordLevelDisc shift {shift}: {what}: rel err {e:.2e}")
        assert e <= RTOL, what


def test_losses_follow_their_formulas():
    """Measured on an MI355X: WordLevelDiscLoss 1.4e-7, WordLevelGenLoss 6.4e-7, d perception.weight of the discriminator loss 1.2e-6."""
    d_in = _inputs()
    disc = _module(d_in["weight"])
    lens = torch.tensor(LENS, dtype=torch.int64, device=DEV)
    real, fake, words = d_in["real"].to(DEV), d_in["fake"].to(DEV), d_in["words"].to(DEV)
    dl = DL.WordLevelDiscLoss().get_loss(disc, fake, real, words, lens)
    dl.backward()
    gl = GL.WordLevelGenLoss().get_loss(disc, fake, words, lens)
    w64 = d_in["weight"].double().requires_grad_(True)
    p_rc, p_rw, p_f = (_f64(w64, t.double(), d_in["words"], s)[0] for t, s in ((d_in["real"], 0), (d_in["real"], 1), (d_in["fake"], 0)))
    want_d = (-torch.log(p_rc + 1e-8)).mean() + ((-torch.log(1 - p_rw + 1e-8)).mean() + (-torch.log(1 - p_f + 1e-8)).mean()) / 2
    want_g = (-torch.log(p_f + 1e-8)).mean()
    want_d.backward()
    for what, got, want in (("WordLevelDiscLoss", dl, want_d), ("WordLevelGenLoss", gl, want_g),
                            ("d perception.weight of the discriminator loss", disc.perception.weight.grad.view(NEF, NEF), w64.grad)):
        e = rel_err(got, want.detach())
        print(f"{what}: rel err {e:.2e}")
        assert e <= RTOL, what
    with pytest.raises(ValueError, match="at least 2"):
        DL.WordLevelDiscLoss().get_loss(disc, fake[:1], real[:1], words[:1], lens[:1])
