"""Generator adversarial losses with the reference's interface (losses/gen_loss.py)."""
from __future__ import annotations

import torch
from torch import Tensor
from torch.nn import Module

from ..backend import functional as HF


class GenLoss:
    def make_labels_for_real_imgs(self, num_labels: int, device="cuda") -> Tensor:
        return torch.ones(num_labels, device=device)

    def get_loss(self, discriminator: Module, fake_images: Tensor, augment=None) -> Tensor:
        """`augment`: an optional callable applied to the images before D (the generator's gradient flows through it)."""
        raise NotImplementedError


class NonSaturatingGenLoss(GenLoss):
    """-mean(log(D(G(z)) + 1e-8))  (gen_loss.py:42-46)."""

    def get_loss(self, discriminator: Module, fake_images: Tensor, augment=None) -> Tensor:
        if augment is not None:
            fake_images = augment(fake_images)
        return HF.ns_gen_loss(discriminator(fake_images))


class ConditionalGenLoss(GenLoss):
    """-mean(log(Du(G(z)) + 1e-8)) - mean(log(Dc(G(z), s) + 1e-8)): the generator's adversarial term against a text-conditional
    discriminator (AttnGAN's generator_loss: errG = cond_errG + uncond_errG, here in the non-saturating log form).  One trunk pass;
    both heads read its 4x4 code."""

    def get_loss(self, discriminator: Module, fake_images: Tensor, sent: Tensor, augment=None) -> Tensor:
        if getattr(discriminator, "COND_DNET", None) is None:
            raise ValueError(f"ConditionalGenLoss: {type(discriminator).__name__} has no COND_DNET; build it with "
                             f"cond_dim=<sentence-embedding width>")
        if augment is not None:
            fake_images = augment(fake_images)
        h = discriminator.features(fake_images)
        return HF.ns_gen_loss(discriminator.uncond(h)) + HF.ns_gen_loss(discriminator.cond(h, sent))


class StandardGenLoss(GenLoss):
    """BCE(D(G(z)), 1)  (gen_loss.py:21-35).  Not used by train.py:74; the discriminator runs on the HIP kernels, the
    cross-entropy over its [B] probabilities is a stock ATen elementwise op."""

    def get_loss(self, discriminator: Module, fake_images: Tensor, augment=None) -> Tensor:
        if augment is not None:
            fake_images = augment(fake_images)
        p = discriminator(fake_images)
        return torch.nn.functional.binary_cross_entropy(p, self.make_labels_for_real_imgs(p.shape[0], device=p.device))


class WordLevelGenLoss:
    """m(-log(p(G, c) + 1e-8)): the generator's term against the word-level discriminator (networks.discriminators.WordLevelDisc),
    on the fakes' region features and the matching captions."""

    def get_loss(self, word_disc: Module, fake_regions: Tensor, words: Tensor, lens) -> Tensor:
        return (-torch.log(word_disc(fake_regions, words, lens, 0) + 1e-8)).mean()
