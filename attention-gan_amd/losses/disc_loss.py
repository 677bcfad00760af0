"""Discriminator losses with the reference's interface (losses/disc_loss.py)."""
from __future__ import annotations

import torch
from torch import Tensor
from torch.nn import Module

from ..backend import functional as HF


class DiscLoss:
    def make_labels_for_real_imgs(self, num_labels: int, label_smooth=0.8, device="cuda") -> Tensor:
        return torch.empty(num_labels, device=device).uniform_(label_smooth, 1.0)

    def make_labels_for_fake_imgs(self, num_labels: int, device="cuda") -> Tensor:
        return torch.zeros(num_labels, device=device)

    def get_loss(self, discriminator: Module, fake_images: Tensor, real_images: Tensor, augment=None, observe=None) -> Tensor:
        """`augment`: an optional callable applied to the images before D.  It is handed the PAIR (real_images, fake_images) and
        returns the augmented [real; fake] batch as one tensor (backend.functional.diffaug does both in one pass).
        `observe`: an optional callable handed the REAL samples' scores (probabilities, detached), the overfitting signal of
        adaptive augmentation (augment.AdaController.observe)."""
        raise NotImplementedError


class NonSaturatingDiscLoss(DiscLoss):
    """-mean(log(D(x)+1e-8) + log(1-D(G(z))+1e-8)); the real batch goes through D first (disc_loss.py:55-61).

    With a discriminator of this package the two passes are ONE pass over the concatenated [real; fake] batch inside
    `functional.bn_groups(2)`: every BatchNorm still normalises each half with its own statistics and updates its running
    statistics twice, real first -- the reference's results -- while every convolution runs once on twice the pixels (half
    the launches; the deep 4x4..16x16 layers, M = 384 pixels per batch, fill their tiles twice as well).  `batch_pairs = False`
    restores the two separate passes."""

    batch_pairs = True

    def get_loss(self, discriminator: Module, fake_images: Tensor, real_images: Tensor, augment=None, observe=None) -> Tensor:
        if (self.batch_pairs and getattr(discriminator, "supports_batch_groups", False) and discriminator.training
                and fake_images.is_cuda and fake_images.shape == real_images.shape):
            # with an augmentation, ITS kernel writes the concatenation: the un-augmented torch.cat pass is never run
            both = torch.cat([real_images, fake_images], dim=0) if augment is None else augment((real_images, fake_images))
            with HF.bn_groups(2):
                score = discriminator(both)
            if observe is not None:
                observe(score.detach()[:real_images.shape[0]])
            return HF.ns_disc_loss_paired(score)
        if augment is not None:
            both = augment((real_images, fake_images))
            real_images, fake_images = both[:real_images.shape[0]], both[real_images.shape[0]:]
        dx_score = discriminator(real_images)
        if observe is not None:
            observe(dx_score.detach())
        dg_score = discriminator(fake_images)
        return HF.ns_disc_loss(dx_score, dg_score)


def _conditional(discriminator: Module, who: str) -> None:
    if getattr(discriminator, "COND_DNET", None) is None:
        raise ValueError(f"{who}: {type(discriminator).__name__} has no COND_DNET; build it with cond_dim=<sentence-embedding width>")


class ConditionalDiscLoss(DiscLoss):
    """The discriminator loss of AttnGAN's text-conditional discriminators (discriminator_loss in its miscc/losses.py): every image is
    scored twice, alone and jointly with a sentence embedding (COND_DNET), and the joint head also sees the mismatched pairs -- a real
    image with another sample's caption, the only adversarial signal for "this image does not show this sentence":

        (m(-log Du(x)) + m(-log Dc(x, s))) / 2 + (m(-log(1 - Du(G))) + m(-log(1 - Dc(G, s))) + m(-log(1 - Dc(x, s')))) / 3

    Departures from AttnGAN: the mismatched pairs are the B cyclic pairs (x_b, s_{(b+1) mod B}) where AttnGAN takes B - 1 and drops
    the last -- equal groups are what functional.bn_groups takes; and the terms are this project's non-saturating log form with its
    1e-8 guards (functional.cond_disc_loss), not BCELoss.

    Paired path (the default, as NonSaturatingDiscLoss): ONE trunk pass over [real; fake] -- or over the augmenter's output -- under
    bn_groups(2), then uncond(h), cond(h, sent, wrong=True) and ONE loss launch.  The wrong pairs reuse the real rows' (augmented)
    code, as AttnGAN reuses real_features.  `batch_pairs = False`, or a discriminator without `supports_batch_groups`, runs the
    trunk and each head separately per batch -- real, fake, then the wrong pairs through the joint head -- with the same results.
    `observe` is handed the UNCONDITIONAL real scores, so the overfitting signal of adaptive augmentation keeps its meaning."""

    batch_pairs = True

    def get_loss(self, discriminator: Module, fake_images: Tensor, real_images: Tensor, sent: Tensor, augment=None, observe=None) -> Tensor:
        _conditional(discriminator, "ConditionalDiscLoss")
        b = real_images.shape[0]
        if (self.batch_pairs and getattr(discriminator, "supports_batch_groups", False) and discriminator.training
                and fake_images.is_cuda and fake_images.shape == real_images.shape):
            both = torch.cat([real_images, fake_images], dim=0) if augment is None else augment((real_images, fake_images))
            with HF.bn_groups(2):
                h = discriminator.features(both)
            pu = discriminator.uncond(h)
            if observe is not None:
                observe(pu.detach()[:b])
            return HF.cond_disc_loss(pu, discriminator.cond(h, sent, wrong=True))
        if augment is not None:
            both = augment((real_images, fake_images))
            real_images, fake_images = both[:b], both[b:]
        # separate passes in the paired path's BatchNorm call order: trunk real, fake; joint head real, fake, wrong
        h_real = discriminator.features(real_images)
        pu_real = discriminator.uncond(h_real)
        if observe is not None:
            observe(pu_real.detach())
        h_fake = discriminator.features(fake_images)
        pu_fake = discriminator.uncond(h_fake)
        pc = [discriminator.cond(h_real, sent), discriminator.cond(h_fake, sent), discriminator.cond(h_real, sent.roll(-1, 0))]
        return HF.cond_disc_loss(torch.cat([pu_real, pu_fake]), torch.cat(pc))


class StandardDiscLoss(DiscLoss):
    """BCE variant (disc_loss.py:26-47); not used by train.py:74-75.  The discriminator passes run on the HIP kernels, the
    cross-entropy over [B] probabilities is a stock ATen elementwise op."""

    def get_loss(self, discriminator: Module, fake_images: Tensor, real_images: Tensor, augment=None, observe=None) -> Tensor:
        """(BCE(D(G(z)), 0) + BCE(D(x), U(0.8, 1))) / 2 -- fake batch first, smoothed real labels (disc_loss.py:31-47)."""
        bce = torch.nn.functional.binary_cross_entropy
        if augment is not None:
            both = augment((real_images, fake_images))
            real_images, fake_images = both[:real_images.shape[0]], both[real_images.shape[0]:]
        p_fake = discriminator(fake_images)
        loss_fake = bce(p_fake, self.make_labels_for_fake_imgs(p_fake.shape[0], device=p_fake.device))
        p_real = discriminator(real_images)
        if observe is not None:
            observe(p_real.detach())
        loss_real = bce(p_real, self.make_labels_for_real_imgs(p_real.shape[0], device=p_real.device))
        return (loss_fake + loss_real) / 2


class WordLevelDiscLoss:
    """The word-level discriminator's loss (ControlGAN's word-level terms in this project's non-saturating log form with its 1e-8
    guards), p = networks.discriminators.WordLevelDisc:

        m(-log(p(x, c) + 1e-8)) + (m(-log(1 - p(x, c') + 1e-8)) + m(-log(1 - p(G, c) + 1e-8))) / 2,     m = mean over B

    x the real images' regions, G the fakes', c the captions and c' the cyclic mismatch (image b with caption (b + 1) mod B, the
    pairs ConditionalDiscLoss uses).  The perception layer runs ONCE over [real; fake]: the real rows feed both real terms.  The
    log terms are stock ATen elementwise ops on [B] probabilities: deterministic, and capturable."""

    def get_loss(self, word_disc: Module, fake_regions: Tensor, real_regions: Tensor, words: Tensor, lens) -> Tensor:
        b = real_regions.shape[0]
        if b < 2:
            raise ValueError("WordLevelDiscLoss: the mismatched pairs need at least 2 captions")
        if fake_regions.shape != real_regions.shape:
            raise ValueError(f"WordLevelDiscLoss: real regions {tuple(real_regions.shape)}, fake regions {tuple(fake_regions.shape)}")
        n = word_disc.perceive(torch.cat([real_regions, fake_regions], dim=0))
        p_real = word_disc.score(n[:b], words, lens, 0)[0]
        p_wrong = word_disc.score(n[:b], words, lens, 1)[0]
        p_fake = word_disc.score(n[b:], words, lens, 0)[0]
        return (-torch.log(p_real + 1e-8)).mean() + ((-torch.log(1 - p_wrong + 1e-8)).mean() + (-torch.log(1 - p_fake + 1e-8)).mean()) / 2
