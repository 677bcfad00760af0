"""`ModelTrainer` helpers with the reference's names (trainers/trainer.py:13-127) and the GAN train step of
train.py:109-151 as a reusable object (`GanTrainStep`) with flat-buffer Adam and overlapped gradient all-reduce."""
from __future__ import annotations

import collections
import contextlib
import copy
import logging
import math
import os
from typing import Callable, Dict, List, Optional, Sequence

import torch
from torch import Tensor
from torch.nn import Module

from ..augment import GEO_UNIFORMS, AdaController, parse_geometry, parse_policy
from ..backend import functional as HF
from ..dataparallel import GradBuckets, any_rank, averaged_buffers, broadcast_module_, rank_of, world_size
from ..losses.disc_loss import ConditionalDiscLoss, NonSaturatingDiscLoss, WordLevelDiscLoss
from ..losses.gen_loss import ConditionalGenLoss, NonSaturatingGenLoss, WordLevelGenLoss
from ..losses.KL_loss import KL_loss
from ..losses.sentence_loss import SentenceLoss
from ..losses.words_loss import WordsLoss
from ..optim import FlatAdam, FlatEMA


def _device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


class ModelTrainer:
    """Label / noise / denormalise / checkpoint helpers (reference trainer.py:20-43,109-127)."""

    def __init__(self):
        pass

    def _make_match_labels(self, batch_size: int) -> Tensor:
        labels = torch.arange(batch_size, dtype=torch.int64, device=_device())
        # lets the DAMSM losses use the kernels' built-in arange targets (no copy, no readback); the tag carries the tensor's version
        # counter, so an in-place edit of the labels (labels[i] = j, labels.copy_(perm)) voids it and the values travel as given
        labels._agan_arange = (batch_size, labels._version)
        return labels

    def _count_parameters(self, model: Module):
        n = sum(p.numel() for p in model.parameters() if p.requires_grad)
        print(f"Model {model.__class__.__name__} has {n} parameters")
        return n

    def _make_noise(self, batch_size: int, z_dim: int) -> Tensor:
        return torch.randn(batch_size, z_dim, dtype=torch.float32, device=_device())

    def _make_mask(self, lengths, maxlen: Optional[int] = None) -> Tensor:
        """[[1]*len + [0]*(max-len)] int64 (train.py:96-100).  A device tensor of lengths is turned into the mask on the device
        (no host sync; `maxlen` = padded caption length, the reference's max(lengths))."""
        if isinstance(lengths, Tensor) and lengths.is_cuda:
            if maxlen is None:
                raise ValueError("_make_mask: maxlen is required for device-resident lengths")
            return (torch.arange(maxlen, device=lengths.device).view(1, -1) < lengths.view(-1, 1)).to(torch.int64)
        lens = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        mx = max(lens) if maxlen is None else int(maxlen)
        return torch.tensor([[1] * l + [0] * (mx - l) for l in lens], dtype=torch.int64, device=_device())

    def _denormalise_single(self, tensor: Tensor) -> Tensor:
        return tensor * 0.5 + 0.5

    def _denormalise_multiple(self, tensors: List[Tensor]) -> List[Tensor]:
        return [self._denormalise_single(t) for t in tensors]

    def _plot_history(self, *args, **kwargs) -> None:
        raise NotImplementedError("loss-curve plotting is outside the hot-path scope (SURVEY.md section 2 #7): the histories are "
                                  "plain lists of device scalars (g_losses, d_losses, damsm_losses)")

    def _image_grid(self, fake_images: List[Tensor]) -> List[Tensor]:
        """The reference's evaluation grid (trainers/trainer.py:68-98) as TENSORS: per resolution the first n*n images (n*n = the
        largest square number <= the batch, :76-78) tiled row-major into one [3, n*res, n*res] uint8 image (values clamped to [0, 1]
        like imshow does for float data).  No matplotlib: the caller decides where pixels go."""
        num = len(fake_images[0])
        square = next((i for i in range(num, 0, -1) if math.isqrt(i) ** 2 == i), 1)
        n = math.isqrt(square)
        grids = []
        for images in fake_images:
            c, h, w = images.shape[1:]
            g = images[:square].detach().float().clamp(0.0, 1.0).reshape(n, n, c, h, w).permute(2, 0, 3, 1, 4).reshape(c, n * h, n * w)
            grids.append((g * 255.0 + 0.5).to(torch.uint8))
        return grids

    def _plot_image_grid(self, fake_images: List[Tensor], epoch: Optional[int] = None, folder: str = 'generated_images') -> List[str]:
        """_image_grid written to {folder}/epoch_{e}-{res}x{res}.ppm (binary PPM: the reference writes PNGs through matplotlib,
        trainers/trainer.py:93-98; same file stems).  Returns the paths."""
        os.makedirs(folder, exist_ok=True)
        paths = []
        for g, images in zip(self._image_grid(fake_images), fake_images):
            res = images.shape[-1]
            stem = f"epoch_{epoch}-{res}x{res}" if epoch else f"_{res}x{res}"
            path = f"{folder}/{stem}.ppm"
            hwc = g.permute(1, 2, 0).contiguous().cpu().numpy()
            with open(path, "wb") as f:
                f.write(f"P6\n{hwc.shape[1]} {hwc.shape[0]}\n255\n".encode())
                f.write(hwc.tobytes())
            paths.append(path)
        return paths

    def _save_weights(self, modules: List, root_folder='saved_weights') -> None:
        """state_dict per module at {root}/{ClassName}.pkl.  Optimisers get an index suffix so that the reference's
        four `Adam` objects no longer overwrite one Adam.pkl (SURVEY.md §5 checkpoint note)."""
        os.makedirs(root_folder, exist_ok=True)
        seen: Dict[str, int] = {}
        for m in modules:
            name = m.__class__.__name__
            k = seen.get(name, 0)
            seen[name] = k + 1
            path = f"{root_folder}/{name}.pkl" if k == 0 else f"{root_folder}/{name}_{k}.pkl"
            torch.save(m.state_dict(), path)
            print(f'Module {name} weights saved to {path}')

    def _load_weights(self, modules: List[Module], root_folder='saved_weights') -> None:
        """Mirror of _save_weights: the k-th module of a class reads {ClassName}_{k}.pkl (k = 0: no suffix); nn.Modules are put
        in eval mode like the reference does (trainer.py:124), optimisers are not."""
        seen: Dict[str, int] = {}
        for m in modules:
            name = m.__class__.__name__
            k = seen.get(name, 0)
            seen[name] = k + 1
            path = f"{root_folder}/{name}.pkl" if k == 0 else f"{root_folder}/{name}_{k}.pkl"
            try:
                m.load_state_dict(torch.load(path, weights_only=True))
                if isinstance(m, Module):
                    m.eval()
                print(f'Module {name} weights loaded from {path}')
            except FileNotFoundError:
                print(f'FAILED: Module {name}... weights at path {path} were not found')


# what the generator's forward leaves for the rest of the step
# (aug_u: the augmentation's uniforms [3 * len(Ds), B, 8], None without a policy; aug_q: the per-stage gate uniforms
# [3 * len(Ds), B, 4], None unless the augmentation has a probability; aug_m: the geometric stages' matrices [3 * len(Ds), B, 6],
# None without `geometry`; sent: the sentence embeddings, detached, for the conditional discriminator heads, None unless `conditional`)
_Forward = collections.namedtuple("_Forward", "labels mask fakes attn mu logvar aug_u aug_q aug_m sent", defaults=(None, None))


def _forked(streams, i: int, main):
    """Context for work on discriminator i's stream, which first waits for `main`; without streams, the current one as it is."""
    if streams is None:
        return contextlib.nullcontext()
    streams[i].wait_stream(main)
    return torch.cuda.stream(streams[i])


class GanTrainStep(ModelTrainer):
    """One batch of GanTrainer.train_gan (train.py:109-151): three discriminator updates, then one generator update.

    Results-identical departures from the script: fakes are detached in the D updates (the reference back-props
    through G there and discards the result at :132); D weight gradients are not produced in the G update.
    BatchNorm call order per D is kept: real batch, fake batch (D update), fake batch again (G update).

    `augment`: a DiffAugment policy ("color,translation,cutout", any subset; augment.parse_policy) applied to every image a
    discriminator sees -- real and fake in its own update, fake again in the generator update, where the gradient flows through
    the transform (backend.functional.diffaug: two launches per tensor).  The uniforms are ONE torch.rand draw per step from
    `self.rng`, taken in _gen_forward right after noise and eps: aug_u [3 * len(Ds), B, 8], slot 3i for discriminator i's real
    batch, 3i + 1 for its fake batch, 3i + 2 for the fake batch in the generator update.  The image encoder (DAMSM branch)
    sees the un-augmented image; generate_images and evaluate never augment.  The policy is configuration, not checkpoint
    content.  With None (default) nothing is drawn and no kernel runs.

    `ema`: the decay of an exponential moving average of the generator (optim.FlatEMA; `ema_warmup`: beta_t = min(ema, (1 + t) /
    (10 + t))).  `self.G_ema` is a copy of the generator taken before training whose weights and BatchNorm running statistics follow
    the live ones by ONE launch right after the generator's Adam step -- in step(), inside capture()'s graph and inside the Adam
    graph of capture_segments() alike; warm-up steps count.  generate_images(use_ema=True) and evaluate(use_ema=True) sample it;
    state_dict() carries it as "generator_ema" and "ema".  With None (default) there is no copy, no launch and no checkpoint key.

    `augment_p`, `ada_target`: apply every stage of `augment` to every sample with probability p instead of always (adaptive
    discriminator augmentation, Karras et al. 2020; both need a non-empty `augment` or `geometry`).  `augment_p` alone is a fixed probability;
    `ada_target` lets p adapt, starting from `augment_p or 0.0`: every discriminator's real scores are tallied on its own stream
    (r_t = E[sign(D(real) - 0.5)]), and ONE one-thread launch next to the averaging update -- after the generator's Adam step, in
    step(), capture() and capture_segments() alike -- moves p every `ada_interval` steps by (real scores seen) / (ada_kimg * 1000 *
    len(Ds)) up while r_t > ada_target and down while below, inside [0, ada_p_max].  p lives in device memory (self.ada.p, the
    step's result "ada_p"); the kernels read it when they run, every augmentation call of a step reads the same value, and nothing
    is read on the host (self.ada.sync() does, on request).  The gates are one more torch.rand draw from `self.rng` right after
    aug_u: aug_q [3 * len(Ds), B, 4], slots as for aug_u.  state_dict() carries the controller's words as "ada" with `ada_target`
    only; a checkpoint without the key loads with p at its initial value.  Under torch.distributed `augment_p` works and
    `ada_target` is refused: whether r_t is per rank or all-reduced is not decided yet.

    `geometry`: the paper's geometric stages ("xflip,rot90,scale,rotate,aniso", any subset; augment.parse_geometry) as ONE bilinear
    affine warp with zero fill (backend.functional.affine_warp) applied to the same tensors IN FRONT of `augment`'s stages --
    geometry before colour, the paper's order -- and differentiated in the generator update by a gather with a fixed summation
    order.  The uniforms are one more torch.rand draw from `self.rng`, the LAST of _gen_forward's draws: aug_g [3 * len(Ds), B, 16],
    slots as for aug_u; one small launch right after it (backend.functional.geometry_matrices) turns all of them into matrices,
    which do not depend on the resolution.  With `augment_p` / `ada_target` (which need a non-empty `augment` OR `geometry`) every
    geometric stage is gated per sample by slots 8..12 of its uniforms against the same device-resident p.  The image encoder,
    generate_images and evaluate never see the warp; the stages are configuration, not checkpoint content.  With None (default)
    nothing is drawn and no kernel runs.

    `conditional`: text-conditional discriminators, AttnGAN's own: every discriminator must carry COND_DNET (built with cond_dim =
    the sentence embedding's width; ValueError otherwise).  The discriminator updates use losses.disc_loss.ConditionalDiscLoss --
    unconditional and joint sentence-image scores of the real and the fake batch plus the joint scores of the B mismatched pairs
    (real image b, caption (b + 1) mod B; AttnGAN takes B - 1), which reuse the real batch's augmented code -- and the generator update
    losses.gen_loss.ConditionalGenLoss, both on the step's `sent_embs`, detached (the text encoder is frozen).  Eager step, capture()
    and capture_segments() alike; `augment`, `geometry`, `augment_p` / `ada_target` (fed the UNCONDITIONAL real scores), `ema` and
    torch.distributed work unchanged, and checkpoints need nothing new: the head's parameters live in the discriminators' state_dict
    (AttnGAN's keys) and flat optimisers.  With False (default) no module, launch, random draw or result key is added.

    `word_disc`: ControlGAN's word-level discriminator (networks.discriminators.WordLevelDisc; needs `image_encoder`, ValueError
    otherwise), with `word_lambda` the weight of its term in the generator's loss.  It is broadcast like the other modules and has its
    own FlatAdam (the discriminators' lr and betas) and GradBuckets.  One more phase, after the image discriminators' updates and before
    the generator's: the regions of real_imgs[-1] and of fakes[-1].detach() come from the frozen encoder under no_grad, then
    losses.disc_loss.WordLevelDiscLoss, backward, exchange and the optimiser step (observer tag "DW"; result "dw_loss").  In the
    generator update the regions the DAMSM branch computes anyway also go through the (frozen) module and word_lambda *
    losses.gen_loss.WordLevelGenLoss joins the total (result "gw_loss").  Eager step, capture() and capture_segments() -- two more
    graphs, DW backward and DW Adam -- alike; `conditional`, `augment`, `geometry`, `ada_target`, `ema` and torch.distributed work
    unchanged, and the encoder, hence this discriminator, sees un-augmented images as the DAMSM branch does.  state_dict() carries
    "word_disc" and "word_optim"; a checkpoint without them loads: the module stays as it is and its optimiser starts fresh.  With None
    (default) no module, launch, random draw, result key or checkpoint key is added.
    """

    def __init__(self, generator: Module, discriminators: Sequence[Module], image_encoder: Optional[Callable] = None,
                 gen_lr: float = 2e-4, disc_lr: float = 2e-4, gamma1: float = 4.0, gamma2: float = 5.0, gamma3: float = 10.0,
                 wlambda: float = 5.0, slambda: float = 5.0, bucket_bytes: int = 64 << 20, group=None, seed: int = 0,
                 g_bucket_bytes: Optional[int] = None, augment: Optional[str] = None, ema: Optional[float] = None,
                 ema_warmup: bool = True, augment_p: Optional[float] = None, ada_target: Optional[float] = None, ada_interval: int = 4,
                 ada_kimg: float = 500.0, ada_p_max: float = 1.0, geometry: Optional[str] = None, conditional: bool = False,
                 word_disc: Optional[Module] = None, word_lambda: float = 1.0):
        super().__init__()
        if word_disc is not None and image_encoder is None:
            raise ValueError("GanTrainStep: word_disc scores the image encoder's region features: it needs image_encoder")
        if conditional and any(getattr(d, "COND_DNET", None) is None for d in discriminators):
            raise ValueError("GanTrainStep: conditional=True needs every discriminator built with cond_dim=<sentence-embedding width> "
                             "(networks.discriminators: COND_DNET)")
        self.conditional = bool(conditional)
        if (augment_p is not None or ada_target is not None) and not (parse_policy(augment) or parse_geometry(geometry)):
            raise ValueError("GanTrainStep: augment_p and ada_target need a non-empty augment policy")
        if ada_target is not None and world_size(group) > 1:
            raise ValueError("GanTrainStep: ada_target is single-process for now (how r_t is formed over ranks is not decided); "
                             "augment_p works under torch.distributed")
        # the augmentation's probability in device memory, with its controller when it adapts (augment.AdaController checks the values)
        self.ada = (AdaController(next(generator.parameters()).device, len(discriminators), p=0.0 if augment_p is None else float(augment_p),
                                  target=ada_target, interval=ada_interval, kimg=ada_kimg, p_max=ada_p_max)
                    if augment_p is not None or ada_target is not None else None)
        if ema is not None and not 0.0 < float(ema) < 1.0:
            raise ValueError(f"GanTrainStep: ema must be a decay inside (0, 1) or None, got {ema}")
        self.augment = parse_policy(augment)                # bit mask; 0 = no augmentation
        self.geometry = parse_geometry(geometry)            # bit mask of the geometric stages; 0 = no warp
        self.G, self.Ds, self.image_encoder = generator, list(discriminators), image_encoder
        self.group = group
        self.word_disc, self.word_lambda = word_disc, float(word_lambda)
        for m in [self.G] + self.Ds + ([word_disc] if word_disc is not None else []):
            broadcast_module_(m, 0, group)
        # noise and the CA-net's eps come from a generator of this object, seeded per RANK: replicas share the initial weights
        # (broadcast above) but must draw different z / eps for their different captions
        dev0 = next(self.G.parameters()).device
        self.rank = rank_of(group)
        self.rng = torch.Generator(device=dev0)
        self.rng.manual_seed(int(seed) * 1000003 + self.rank)
        # sampling (generate_images) draws from a generator of its own: looking at samples mid-training must not shift the
        # training noise stream
        self.sample_rng = torch.Generator(device=dev0)
        self.sample_rng.manual_seed(int(seed) * 1000003 + 500009 + self.rank)
        # the averaged generator is copied while the live parameters are still plain tensors (FlatAdam re-homes them next)
        self.G_ema = copy.deepcopy(self.G) if ema is not None else None
        self.g_opt = FlatAdam(self.G.parameters(), lr=gen_lr, betas=(0.5, 0.999))
        self.g_ema = FlatEMA(self.G, self.G_ema, self.g_opt, float(ema), ema_warmup) if ema is not None else None
        self.d_opts = [FlatAdam(d.parameters(), lr=disc_lr, betas=(0.5, 0.999)) for d in self.Ds]
        # the generator's 28 MB would be ONE 64 MB bucket, launched when its whole backward is done and fully exposed: it goes out in
        # 8 MB buckets instead, so all but the last travel under the ~10 ms of backward that remain
        self.g_buckets = GradBuckets(self.g_opt, min(bucket_bytes, 8 << 20) if g_bucket_bytes is None else g_bucket_bytes, group)
        self.d_buckets = [GradBuckets(o, bucket_bytes, group) for o in self.d_opts]
        # the word-level discriminator: an optimiser and buckets of its own, like every other discriminator
        self.w_opt = FlatAdam(word_disc.parameters(), lr=disc_lr, betas=(0.5, 0.999)) if word_disc is not None else None
        self.w_buckets = GradBuckets(self.w_opt, bucket_bytes, group) if word_disc is not None else None
        self.word_disc_loss, self.word_gen_loss = WordLevelDiscLoss(), WordLevelGenLoss()
        # issue order of the three independent discriminator updates: LARGEST first (Disc256: 273 MB of gradients, the long pole of
        # the exchange), so that its buckets travel while the smaller discriminators still compute.  Results do not depend on it.
        self.d_order = sorted(range(len(self.Ds)), key=lambda i: -self.d_opts[i].numel)
        dev = next(self.G.parameters()).device
        self.words_loss = WordsLoss(dev, gamma1, gamma2, gamma3, wlambda)
        self.sent_loss = SentenceLoss(dev, gamma3, slambda)
        self.disc_loss, self.gen_loss = ((ConditionalDiscLoss(), ConditionalGenLoss()) if self.conditional else
                                         (NonSaturatingDiscLoss(), NonSaturatingGenLoss()))
        self.g_losses: List = []
        self.d_losses: List = []
        self.damsm_losses: List = []
        self.overlap_discriminators = True
        # optional: weight gradients on a side stream per compute stream (functional.set_wgrad_side_stream), joined by every
        # optimiser step.  Measured on MI355X at the metric config: 763 vs 778 images/s with it on -- the step is a sum of
        # kernels that each fill the chip, so the extra concurrency only adds cache pressure.  Off by default.
        self.overlap_weight_gradients = False
        self._streams: List = []
        # optional observer `f(tag, optimiser)` called right before each optimiser consumes its gradients (after the gradient
        # exchange), tag in {"D0", "D1", "D2", "G"}: tests read the flat gradient buffers through it
        self.on_gradients: Optional[Callable] = None
        # optional observer `f(i, score)` of discriminator i's real scores as the controller of `ada_target` is handed them
        self.on_real_scores: Optional[Callable] = None

    def _d_streams(self, n: int, device) -> List:
        if len(self._streams) != n:
            self._streams = [torch.cuda.Stream(device=device) for _ in range(n)]
        return self._streams

    def step(self, word_embs: Tensor, sent_embs: Tensor, lengths, class_ids, real_imgs: Sequence[Tensor],
             noise: Optional[Tensor] = None, eps: Optional[Tensor] = None, aug_u: Optional[Tensor] = None,
             aug_q: Optional[Tensor] = None, aug_g: Optional[Tensor] = None) -> Dict[str, Tensor]:
        if word_embs.is_cuda and not (isinstance(lengths, Tensor) and lengths.is_cuda):
            # host-side caption lengths (the reference's DataLoader hands over a list / CPU tensor): ONE pinned, non-blocking
            # copy up front -- a blocking H2D copy in the middle of the step drains the launch pipeline (~4 ms per step)
            host = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1)
            lengths = host.pin_memory().to(word_embs.device, non_blocking=True)
        if word_embs.is_cuda:
            HF.amax_begin_step(word_embs.device)        # zeroed amax slots of this step (fp16 split mode only; one fill launch)
        prev_side = HF.set_wgrad_side_stream(self.overlap_weight_gradients and word_embs.is_cuda)
        try:
            return self._step(word_embs, sent_embs, lengths, class_ids, real_imgs, noise, eps, aug_u, aug_q, aug_g)
        finally:
            HF.set_wgrad_side_stream(prev_side)

    def _step(self, word_embs, sent_embs, lengths, class_ids, real_imgs, noise, eps, aug_u=None, aug_q=None,
              aug_g=None) -> Dict[str, Tensor]:
        fw = self._gen_forward(word_embs, sent_embs, lengths, noise, eps, aug_u, aug_q, aug_g)
        out: Dict[str, Tensor] = {}
        # ---- discriminator updates (train.py:123-130) ----
        # The three updates are independent of each other (each D has its own weights, optimiser and images), so each runs on
        # its own HIP stream: the deep 4x4/8x8 layers of one discriminator (tiny grids) overlap the wide early layers of another.
        # Autograd replays each backward on the stream its forward ran on.
        main = torch.cuda.current_stream() if fw.fakes[0].is_cuda else None
        streams = self._d_streams(len(self.Ds), fw.fakes[0].device) if (main is not None and self.overlap_discriminators) else None
        if streams is not None:
            for st in streams:                      # discriminator weight gradients run on the (otherwise idle) main stream
                HF.set_side_stream_for(st, main)
        for i in self.d_order:
            with _forked(streams, i, main):
                self._d_backward(i, fw, real_imgs, out, arm=True)
                self._apply(f"D{i}", self.d_opts[i], self.d_buckets[i].finish())
        if streams is not None:
            for st in streams:
                main.wait_stream(st)
        # ---- word-level discriminator update: after the image discriminators', before the generator's ----
        if self.word_disc is not None:
            self._dw_backward(fw, word_embs, lengths, real_imgs, out, arm=True)
            self._apply("DW", self.w_opt, self.w_buckets.finish())
        # ---- generator update (train.py:132-151) ----
        self._g_backward(fw, word_embs, sent_embs, lengths, class_ids, out, streams, arm=True)
        self._apply("G", self.g_opt, self.g_buckets.finish())
        if self.g_ema is not None:
            self.g_ema.update()
        if self.ada is not None:
            self.ada.update()                       # (every discriminator stream has been joined twice since the tallies)
        # loss histories stay device tensors: no .item() host sync inside the step (reference syncs at train.py:130,144-145)
        self.d_losses.append(out[f"d_loss{len(self.Ds) - 1}"])
        self.g_losses.append(out[f"g_loss{len(self.Ds) - 1}"])
        if "w_loss" in out:
            self.damsm_losses.append(out["w_loss"] + out["s_loss"])
        return self._results(fw, out)

    # -- the phases of the step: _step() runs them eagerly, capture_segments() records each into a graph of its own --------
    def _gen_forward(self, word_embs, sent_embs, lengths, noise, eps, aug_u=None, aug_q=None, aug_g=None) -> "_Forward":
        b = word_embs.shape[0]
        labels = self._make_match_labels(b)
        mask = self._make_mask(lengths, word_embs.shape[2])
        if noise is None:
            noise = torch.randn(b, self.G.z_dim, dtype=torch.float32, device=word_embs.device, generator=self.rng)
        if eps is None:
            eps = torch.randn(b, self.G.cond_dim, dtype=torch.float32, device=word_embs.device, generator=self.rng)
        if not self.augment:
            aug_u = None
        elif aug_u is None:                                 # drawn HERE, after noise and eps: the one place whose graph registers self.rng
            aug_u = torch.rand(3 * len(self.Ds), b, 8, dtype=torch.float32, device=word_embs.device, generator=self.rng)
        elif tuple(aug_u.shape) != (3 * len(self.Ds), b, 8):
            raise ValueError(f"aug_u must be [{3 * len(self.Ds)}, {b}, 8], got {tuple(aug_u.shape)}")
        if self.ada is None:
            aug_q = None
        elif aug_q is None:                                 # the gates' uniforms: same place, same generator, right after aug_u
            aug_q = torch.rand(3 * len(self.Ds), b, 4, dtype=torch.float32, device=word_embs.device, generator=self.rng)
        elif tuple(aug_q.shape) != (3 * len(self.Ds), b, 4):
            raise ValueError(f"aug_q must be [{3 * len(self.Ds)}, {b}, 4], got {tuple(aug_q.shape)}")
        sent = sent_embs.detach() if self.conditional else None      # (the text encoder is frozen: no gradient leaves the heads)
        if not self.geometry:
            return _Forward(labels, mask, *self.G(noise, sent_embs, word_embs, mask, eps), aug_u, aug_q, None, sent)
        slots = 3 * len(self.Ds)
        if aug_g is None:                                   # the geometric stages' uniforms: the last draw of the step
            aug_g = torch.rand(slots, b, GEO_UNIFORMS, dtype=torch.float32, device=word_embs.device, generator=self.rng)
        elif tuple(aug_g.shape) != (slots, b, GEO_UNIFORMS):
            raise ValueError(f"aug_g must be [{slots}, {b}, {GEO_UNIFORMS}], got {tuple(aug_g.shape)}")
        # every slot's matrices by ONE launch: they do not depend on the resolution, so the discriminators' sizes share them
        aug_m = HF.geometry_matrices(aug_g.reshape(-1, GEO_UNIFORMS), self.geometry, None if self.ada is None else self.ada.p)
        return _Forward(labels, mask, *self.G(noise, sent_embs, word_embs, mask, eps), aug_u, aug_q, aug_m.view(slots, b, 6), sent)

    def _augmenter(self, fw: "_Forward", first: int, count: int) -> Optional[Callable]:
        """What the losses apply to the images before D: slots first .. first + count - 1 of the step's uniforms, one per tensor;
        the geometric warp first, then DiffAugment's stages."""
        color = self._diffaugmenter(fw, first, count)
        if fw.aug_m is None:
            return color
        m = fw.aug_m[first:first + count].reshape(-1, 6)    # (adjacent slots: a view, no launch)
        if color is None:
            return lambda xs: HF.affine_warp(xs, m)
        return lambda xs: color(HF.affine_warp(xs, m))

    def _diffaugmenter(self, fw: "_Forward", first: int, count: int) -> Optional[Callable]:
        if fw.aug_u is None:
            return None
        u = fw.aug_u[first:first + count].reshape(-1, 8)    # (adjacent slots: a view, no launch)
        if fw.aug_q is None:
            return lambda xs: HF.diffaug(xs, u, self.augment)
        q, p = fw.aug_q[first:first + count].reshape(-1, 4), self.ada.p
        return lambda xs: HF.diffaug(xs, u, self.augment, q, p)

    def _d_backward(self, i: int, fw: "_Forward", real_imgs, out: Dict[str, Tensor], arm: bool = False) -> None:
        """Discriminator i's gradients on the current stream; `arm`: its buckets exchange them from the backward's hooks."""
        self.d_opts[i].zero_grad()
        if arm:
            self.d_buckets[i].arm()
        aug = self._augmenter(fw, 3 * i, 2)                 # (None without a policy: the call is then the one it always was)
        if self.conditional:                                # (the unconditional real scores are what the controller is handed)
            observe = (lambda score: self._observe(i, score)) if self.ada is not None and self.ada.adaptive else None
            loss = self.disc_loss.get_loss(self.Ds[i], fw.fakes[i].detach(), real_imgs[i], fw.sent, augment=aug, observe=observe)
        elif self.ada is not None and self.ada.adaptive:    # the real scores' signs go to discriminator i's slot, on this stream
            loss = self.disc_loss.get_loss(self.Ds[i], fw.fakes[i].detach(), real_imgs[i], augment=aug,
                                           observe=lambda score: self._observe(i, score))
        else:
            loss = (self.disc_loss.get_loss(self.Ds[i], fw.fakes[i].detach(), real_imgs[i]) if aug is None else
                    self.disc_loss.get_loss(self.Ds[i], fw.fakes[i].detach(), real_imgs[i], augment=aug))
        loss.backward()
        out[f"d_loss{i}"] = loss.detach()

    def _dw_backward(self, fw: "_Forward", word_embs, lengths, real_imgs, out: Dict[str, Tensor], arm: bool = False) -> None:
        """The word-level discriminator's gradients on the current stream: regions of the largest real and fake images from the frozen
        encoder (un-augmented, no graph), then WordLevelDiscLoss."""
        self.w_opt.zero_grad()
        if arm:
            self.w_buckets.arm()
        with torch.no_grad():
            real_regions, _ = self.image_encoder(real_imgs[-1])
            fake_regions, _ = self.image_encoder(fw.fakes[-1].detach())
        loss = self.word_disc_loss.get_loss(self.word_disc, fake_regions, real_regions, word_embs.detach(), lengths)
        loss.backward()
        out["dw_loss"] = loss.detach()

    def _observe(self, i: int, score: Tensor) -> None:
        if self.on_real_scores is not None:
            self.on_real_scores(i, score)
        self.ada.observe(i, score)

    def _g_backward(self, fw: "_Forward", word_embs, sent_embs, lengths, class_ids, out: Dict[str, Tensor],
                    streams: Optional[List] = None, arm: bool = False) -> None:
        """The generator's gradients through the frozen discriminators.  With `streams` (one per discriminator) the adversarial
        terms fan out over them and are joined on the current stream; without, everything runs on the current stream."""
        self.g_opt.zero_grad()
        if arm:
            self.g_buckets.arm()
        main = torch.cuda.current_stream() if streams is not None else None
        frozen = self.Ds + ([self.word_disc] if self.word_disc is not None else [])
        for d in frozen:
            d.requires_grad_(False)
        try:
            # adversarial terms: one stream per discriminator again (forward here, autograd replays the dgrad chains on the same
            # streams); the DAMSM branch (image encoder + words/sentence loss) rides on the last discriminator's stream
            terms = []
            for i, d in enumerate(self.Ds):
                with _forked(streams, i, main):
                    aug = self._augmenter(fw, 3 * i + 2, 1)
                    if self.conditional:
                        gl = self.gen_loss.get_loss(d, fw.fakes[i], fw.sent, augment=aug)
                    else:
                        gl = self.gen_loss.get_loss(d, fw.fakes[i]) if aug is None else self.gen_loss.get_loss(d, fw.fakes[i], augment=aug)
                    terms.append(gl)
                    out[f"g_loss{i}"] = gl.detach()
                    if i == len(self.Ds) - 1 and self.image_encoder is not None:
                        regions, code = self.image_encoder(fw.fakes[i])
                        wl, _ = self.words_loss.get_loss(regions, word_embs, fw.labels, lengths, class_ids)
                        sl = self.sent_loss.get_loss(code, sent_embs, fw.labels, class_ids)
                        terms += [wl, sl]
                        out["w_loss"], out["s_loss"] = wl.detach(), sl.detach()
                        if self.word_disc is not None:      # the same regions through the frozen word-level discriminator
                            gw = self.word_gen_loss.get_loss(self.word_disc, regions, word_embs.detach(), lengths)
                            terms.append(gw * self.word_lambda)
                            out["gw_loss"] = gw.detach()
            if streams is not None:
                for st in streams:
                    main.wait_stream(st)
            total = terms[0]
            for t in terms[1:]:
                total = total + t
            kl = KL_loss(fw.mu, fw.logvar)
            total = total + kl
            out["kl"], out["g_total"] = kl.detach(), total.detach()
            total.backward()
        finally:
            for d in frozen:
                d.requires_grad_(True)

    def _apply(self, tag: str, opt: FlatAdam, scale: float) -> None:
        if self.on_gradients is not None:
            opt.join_and_rebind()
            self.on_gradients(tag, opt)
        opt.step(scale)

    def _results(self, fw: "_Forward", out: Dict[str, Tensor]) -> Dict[str, Tensor]:
        if self.ada is not None and self.ada.adaptive:
            out["ada_p"] = self.ada.p                       # the LIVE device view: read it after the step, clone it to keep a value
        out["fake_imgs"] = [f.detach() for f in fw.fakes]
        out["attn_maps"] = [a.detach() for a in fw.attn]
        out["mu"], out["logvar"] = fw.mu.detach(), fw.logvar.detach()
        return out

    def _warm_up(self, who: str, word_embs, sent_embs, lengths, real_imgs, warmup: int, noise, eps, aug_u=None, aug_q=None,
                 aug_g=None) -> None:
        """What both captures do first: `warmup` real train steps off the default stream, then the host-side tables."""
        if not (isinstance(lengths, Tensor) and lengths.is_cuda and lengths.dtype == torch.int64):
            raise ValueError(f"{who}(): lengths must be an int64 device tensor")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up off the default stream: tables, caches, allocator pools
            for _ in range(max(1, warmup)):
                self.step(word_embs, sent_embs, lengths, None, real_imgs, noise, eps, aug_u, aug_q, aug_g)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        HF.build_pack_tables()                             # the batched re-pack's job tables: host work, not capturable

    # -- whole-step HIP graph ----------------------------------------------------------------------------------------
    def capture(self, word_embs: Tensor, sent_embs: Tensor, lengths: Tensor, real_imgs: Sequence[Tensor], warmup: int = 2,
                noise: Optional[Tensor] = None, eps: Optional[Tensor] = None, aug_u: Optional[Tensor] = None,
                aug_q: Optional[Tensor] = None, aug_g: Optional[Tensor] = None) -> "GraphedStep":
        """Capture one full train step (all four optimiser updates, every stream) into a HIP graph.

        The arguments become the graph's STATIC input buffers: copy each new batch into them (`.copy_()`) and call `replay()`.
        `lengths` must be a device int64 tensor (no host reads inside the step); noise and the CA-net eps are drawn inside the
        graph (graph-safe Philox state) unless static `noise` / `eps` buffers are given, and so are the augmentation's uniforms
        (`aug_u`, with an `augment` policy; `aug_q`, the gates' uniforms, with `augment_p` / `ada_target`; `aug_g`, with `geometry`,
        whose matrix launch is part of the graph and reads the live p); BatchNorm counters, the
        Adam step counters and the augmentation probability with its controller's window live in device memory, so replays keep
        advancing -- and adapting -- exactly like eager steps.  The warm-up steps are real
        training steps.  Single-process only: with world_size > 1 run the eager `step()`."""
        if self.g_buckets.active:
            raise RuntimeError("capture(): the all-reduce path is not captured; use step() under torch.distributed")
        self._warm_up("capture", word_embs, sent_embs, lengths, real_imgs, warmup, noise, eps, aug_u, aug_q, aug_g)
        graph = torch.cuda.CUDAGraph()
        if self.rng.device.type == "cuda":
            graph.register_generator_state(self.rng)       # noise / eps draws inside the graph advance this generator on replay
        with torch.cuda.graph(graph):
            out = self.step(word_embs, sent_embs, lengths, None, real_imgs, noise, eps, aug_u, aug_q, aug_g)
        return GraphedStep(graph, out, self)

    def _mark_replayed(self) -> None:
        """A replayed graph ran every Adam step and the averaging update without their host code: say what adam_step_ and ema_update_
        say, or the next EAGER use of a network (generate_images, step) runs on packs of the weights from before the replay."""
        for holder in [self.g_opt, self.g_ema, self.w_opt] + self.d_opts:
            if holder is not None:
                HF.mark_flat_written(holder.flat)

    # -- segment-wise HIP graphs for world > 1 --------------------------------------------------------------------------
    def capture_segments(self, word_embs: Tensor, sent_embs: Tensor, lengths: Tensor, real_imgs: Sequence[Tensor], warmup: int = 2,
                         noise: Optional[Tensor] = None, eps: Optional[Tensor] = None, aug_u: Optional[Tensor] = None,
                         aug_q: Optional[Tensor] = None, aug_g: Optional[Tensor] = None) -> "SegmentedStep":
        """The train step as NINE HIP graphs (eleven with `word_disc`: its backward and its Adam step, replayed on the main stream between
        the discriminators' and the generator's) with the gradient exchange launched between them -- the form for world_size > 1, where
        the whole-step graph of capture() cannot be used (the RCCL collectives are not captured) and an eager step costs every rank
        ~11 ms of Python per 27 ms step on host cores the 8 ranks share:

            [G forward]  ->  per discriminator, largest first, each on its own stream:
                                 [D_i forward + backward]  -> all-reduce of D_i's flat gradient  ->  [Adam D_i]
                         ->  [G update: forward through the three D, DAMSM, KL, backward]  -> all-reduce of G's gradient  ->  [Adam G]

        A discriminator's exchange is issued when ITS backward graph has finished (not bucket by bucket inside it, as the eager
        step's hooks do), so it overlaps the backward graphs of the OTHER discriminators -- the largest (Disc256, 273 MB) goes
        first -- and nothing overlaps the generator's 28 MB.  The arguments become static input buffers exactly as for capture();
        the graphs share one memory pool and must be replayed in capture order (SegmentedStep.replay does).  Results are
        bit-identical to the eager step (tests/test_gpu_dataparallel.py, one-rank `nccl` rehearsal)."""
        self._warm_up("capture_segments", word_embs, sent_embs, lengths, real_imgs, warmup, noise, eps, aug_u, aug_q, aug_g)
        # memory pools: graphs that share a pool must never run concurrently (a later capture re-uses the temporaries an earlier one
        # freed).  The three discriminator updates replay CONCURRENTLY on their own streams, so each gets a private pool for its two
        # graphs; the generator's graphs, which run alone, share one.
        pool = torch.cuda.graph_pool_handle()
        d_pools = [torch.cuda.graph_pool_handle() for _ in self.Ds]
        # thread-local capture: the process group's watchdog thread polls its events (hipEventQuery) at any time, which a GLOBAL-mode
        # capture turns into "operation not permitted when stream is capturing" in THAT thread and kills the process (seen once in
        # the one-rank nccl rehearsal, round 3)
        mode = "thread_local"
        seg = SegmentedStep(self)
        buckets = [self.g_buckets] + self.d_buckets + ([self.w_buckets] if self.w_buckets is not None else [])
        armed = [bk._armed for bk in buckets]
        for bk in buckets:
            bk._armed = False                              # no hook-driven collectives inside a capture
        prev_side = HF.set_wgrad_side_stream(False)
        try:
            # ---- generator forward ----
            g0 = torch.cuda.CUDAGraph()
            if self.rng.device.type == "cuda":
                g0.register_generator_state(self.rng)
            with torch.cuda.graph(g0, pool=pool, capture_error_mode=mode):
                HF.amax_begin_step(word_embs.device)
                fw = self._gen_forward(word_embs, sent_embs, lengths, noise, eps, aug_u, aug_q, aug_g)
            seg.gen_forward = g0
            out: Dict[str, Tensor] = {}
            # ---- discriminator updates: backward graph, (exchange), Adam graph ----
            for i in self.d_order:
                opt = self.d_opts[i]
                gb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gb, pool=d_pools[i], capture_error_mode=mode):
                    self._d_backward(i, fw, real_imgs, out)
                    opt.join_and_rebind()
                ga = torch.cuda.CUDAGraph()
                with torch.cuda.graph(ga, pool=d_pools[i], capture_error_mode=mode):
                    opt.step(self.d_buckets[i].scale)
                seg.d_backward[i], seg.d_adam[i] = gb, ga
            # ---- word-level discriminator update: runs alone between the discriminators and the generator, in the shared pool ----
            if self.word_disc is not None:
                gwb = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gwb, pool=pool, capture_error_mode=mode):
                    self._dw_backward(fw, word_embs, lengths, real_imgs, out)
                    self.w_opt.join_and_rebind()
                gwa = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gwa, pool=pool, capture_error_mode=mode):
                    self.w_opt.step(self.w_buckets.scale)
                seg.dw_backward, seg.dw_adam = gwb, gwa
            # ---- generator update: one stream, no class ids (as in the warm-up steps) ----
            gg = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gg, pool=pool, capture_error_mode=mode):
                self._g_backward(fw, word_embs, sent_embs, lengths, None, out)
                self.g_opt.join_and_rebind()
            gadam = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gadam, pool=pool, capture_error_mode=mode):
                self.g_opt.step(self.g_buckets.scale)
                if self.g_ema is not None:
                    self.g_ema.update()
                if self.ada is not None:
                    self.ada.update()
            seg.g_backward, seg.g_adam = gg, gadam
            seg.out = self._results(fw, out)
        finally:
            HF.set_wgrad_side_stream(prev_side)
            for bk, a in zip(buckets, armed):
                bk._armed = a
        return seg

    # -- checkpoint / resume (the reference only saves, and its four `Adam` objects share one Adam.pkl) --
    def state_dict(self, all_ranks: bool = True) -> Dict:
        """Checkpoint of the whole step: weights, BatchNorm buffers, the four optimisers and the noise generators' states (so a
        resumed run continues the z / eps sequence instead of replaying it from the seed).

        Under torch.distributed two things are PER REPLICA: the BatchNorm running statistics (local batches, as in the reference's
        single-process BN) and the noise generators (seeded seed * 1000003 + rank, so that replicas draw different z / eps).  With
        `all_ranks=True` (default) the checkpoint holds the MEAN of the running statistics over the ranks and the generator state of
        EVERY rank (`rng` / `sample_rng` = {rank: state}), so every rank writes the same file -- this is a COLLECTIVE: every rank of
        the group must call state_dict(), a lone `if rank == 0: save(step.state_dict())` would hang.  For that pattern pass
        `all_ranks=False`: no communication, the calling rank's own statistics and its own generator states ({rank: state} with one
        entry) are saved.  The live buffers and generators are never modified either way."""
        mine = {"rng": self.rng.get_state(), "sample_rng": self.sample_rng.get_state()}
        w = world_size(self.group)
        sd = {"generator": self.G.state_dict(), "discriminators": [d.state_dict() for d in self.Ds],
              "g_optim": self.g_opt.state_dict(), "d_optims": [o.state_dict() for o in self.d_opts],
              "rng": {self.rank: mine["rng"]}, "sample_rng": {self.rank: mine["sample_rng"]}, "rng_world": w}
        averaged = list(zip([self.G] + self.Ds, [sd["generator"]] + sd["discriminators"]))
        if self.g_ema is not None:
            # the averaged generator (its parameters are identical on every rank by construction, its running statistics per replica
            # like the live ones) and the average's configuration and update count
            e = self.g_ema.state_dict()
            sd["generator_ema"] = e.pop("shadow")
            sd["ema"] = e
            averaged.append((self.G_ema, sd["generator_ema"]))
        if self.ada is not None and self.ada.adaptive:
            sd["ada"] = self.ada.state_dict()              # (one host read; single-process by construction)
        if self.word_disc is not None:                     # (no buffers: nothing to average over the ranks)
            sd["word_disc"], sd["word_optim"] = self.word_disc.state_dict(), self.w_opt.state_dict()
        if all_ranks and w > 1:
            import torch.distributed as dist
            for m, msd in averaged:
                for k, v in averaged_buffers(m, self.group).items():
                    msd[k] = v
            gathered = [None] * w
            dist.all_gather_object(gathered, mine, group=self.group)
            for key in ("rng", "sample_rng"):
                sd[key] = {r: gathered[r][key].cpu() for r in range(w)}
        return sd

    @staticmethod
    def _restore_generator(gen: torch.Generator, saved, rank: int) -> None:
        """Put `gen` where rank `rank` of the checkpointed run left it.  `saved` is {rank: state} (or, from checkpoints written before
        the states were keyed by rank, one bare state = the saving rank's, by convention rank 0).  A rank the checkpoint has no state
        for (rank-0-only save, or a resume on more ranks) gets a state DERIVED from the saved one and its rank -- deterministic, and
        different on every rank, which is what the per-rank seeds are for (identical z / eps on all replicas would collapse the
        effective noise batch to one shard's)."""
        import hashlib
        if isinstance(saved, dict):
            if rank in saved:
                gen.set_state(saved[rank].cpu())
                return
            base = saved[min(saved)]
        else:
            if rank == 0:
                gen.set_state(saved.cpu())
                return
            base = saved
        digest = hashlib.sha256(base.cpu().numpy().tobytes() + int(rank).to_bytes(8, "little")).digest()
        gen.manual_seed(int.from_bytes(digest[:8], "little") & ((1 << 63) - 1))

    def load_state_dict(self, sd: Dict) -> None:
        """A checkpoint without "generator_ema" / "ema" (written before the average existed, or by a run without `ema`) is accepted by
        a trainer with `ema`: the average restarts as a copy of the loaded generator with an update count of 0.  decay and warm-up are
        configuration: the constructor's values hold, a differing saved decay is logged."""
        self.G.load_state_dict(sd["generator"])
        self.g_opt.load_state_dict(sd["g_optim"])
        if self.g_ema is not None:
            if "generator_ema" in sd and "ema" in sd:
                self.g_ema.load_state_dict({"shadow": sd["generator_ema"], "updates": sd["ema"]["updates"]})
                if float(sd["ema"]["decay"]) != self.g_ema.decay:
                    logging.getLogger(__name__).warning("GanTrainStep: the checkpoint's average was kept with decay %g, this run uses %g",
                                                        float(sd["ema"]["decay"]), self.g_ema.decay)
            else:
                self.g_ema.copy_from_live()
        if self.ada is not None and self.ada.adaptive:
            if "ada" in sd:
                self.ada.load_state_dict(sd["ada"])
            else:
                self.ada.reset()                           # a checkpoint of a run without adaptation: p at its initial value
        if self.word_disc is not None:
            if "word_disc" in sd and "word_optim" in sd:
                self.word_disc.load_state_dict(sd["word_disc"])
                self.w_opt.load_state_dict(sd["word_optim"])
            else:                                          # a checkpoint of a run without the module: it stays as it is, its optimiser starts fresh
                with torch.no_grad():
                    self.w_opt.exp_avg.zero_()
                    self.w_opt.exp_avg_sq.zero_()
                    self.w_opt.step_state.zero_()
                self.w_opt.step_count = 0
        for d, o, ds, os_ in zip(self.Ds, self.d_opts, sd["discriminators"], sd["d_optims"]):
            d.load_state_dict(ds)
            if getattr(d, "norm", "batch") == "spectral" and any(k.endswith(".running_mean") for k in ds):
                # a norm="batch" checkpoint warm-starts a spectrally normalised discriminator: its weights are loaded (the module ignores
                # the BatchNorm entries); the saved moments belong to another parameter list, so the optimiser starts fresh
                with torch.no_grad():
                    o.exp_avg.zero_()
                    o.exp_avg_sq.zero_()
                    o.step_state.zero_()
                o.step_count = 0
            else:
                o.load_state_dict(os_)
        # noise streams, per rank (checkpoints written before these were saved simply restart them from the seed)
        for key, gen in (("rng", self.rng), ("sample_rng", self.sample_rng)):
            if sd.get(key) is not None:
                self._restore_generator(gen, sd[key], self.rank)

    @torch.no_grad()
    def generate_images(self, word_embs: Tensor, sent_embs: Tensor, lengths, noise: Optional[Tensor] = None,
                        train_mode_bn: bool = False, eps: Optional[Tensor] = None, use_ema: bool = False) -> List[Tensor]:
        """Sampling path; images mapped from [-1,1] to [0,1].  Same kernels as training, forward only.

        train_mode_bn=False (default): test.py:77-87 -- eval-mode generator (running BatchNorm statistics).
        train_mode_bn=True: the EPOCH-END sample exactly as train.py:154-158 takes it -- under no_grad but WITHOUT .eval(): every
        BatchNorm normalises with the statistics of this batch and pushes them into its running statistics (one more update per
        epoch, which the next checkpoint carries), `noise` is the fixed input of train.py:105.
        use_ema=True samples the averaged generator (`ema` at construction); it never runs batch statistics."""
        G = self._sampled_generator(use_ema, train_mode_bn)
        mask = self._make_mask(lengths, word_embs.shape[2])
        return self._denormalise_multiple(sample_fakes(G, word_embs, sent_embs, mask, self.sample_rng, noise, eps, train_mode_bn))

    def _sampled_generator(self, use_ema: bool, train_mode_bn: bool = False) -> Module:
        if not use_ema:
            return self.G
        if self.g_ema is None:
            raise ValueError("use_ema=True needs a GanTrainStep built with ema=<decay>")
        if train_mode_bn:
            raise ValueError("use_ema=True cannot be combined with train_mode_bn=True: the averaged generator never runs batch statistics")
        return self.G_ema

    def evaluate(self, batches, text_encoder: Callable, real, n_samples: int, use_ema: bool = False, **kwargs) -> Dict:
        """R-precision and Frechet distance of this step's generator under its own image encoder (evaluation.Evaluator.evaluate:
        `real` is a FeatureMoments of real images, e.g. from Evaluator.real_moments; kwargs: R, seed, batch_size, folds, and
        real_features, k, kid_subsets, kid_subset_size for precision / recall, density / coverage and the kernel distance;
        inception_splits for the Inception Score, which needs an image encoder with a classifier head: CNNEncoder(num_classes=...));
        of the averaged generator with use_ema=True."""
        from ..evaluation import Evaluator
        dev = next(self.G.parameters()).device
        return Evaluator(self._sampled_generator(use_ema), text_encoder, self.image_encoder, dev).evaluate(batches, real, n_samples, **kwargs)

    # -- the loop around the step (train.py:107-158) -------------------------------------------------------------------
    def skip_batch(self, lengths, batch_rows: int, batch_size: int) -> bool:
        """The reference's batch guard (train.py:112: `if min(lengths) < 2 or len(words) < BATCH_SIZE: continue`), decided for the
        whole data-parallel group: a rank that skipped on its own would leave the others waiting in the gradient all-reduce, so
        every rank contributes its local verdict to ONE small MAX all-reduce and all skip together if any shard fails the guard
        (dataparallel.any_rank).  A collective under torch.distributed: every rank calls it once per batch, in step."""
        lens = lengths.tolist() if hasattr(lengths, "tolist") else list(lengths)
        local = (min(int(v) for v in lens) < 2) if len(lens) else True
        local = local or int(batch_rows) < int(batch_size)
        return any_rank(local, self.group, next(self.G.parameters()).device)

    def train_epoch(self, batches, text_encoder: Callable, batch_size: int, max_batches: Optional[int] = None) -> int:
        """One pass over `batches` (tuples in the reference's wire format, data/bedrooms.py:229-236: words, lengths, class_ids,
        img64, img128, img256) as train.py:109-151 runs it: guard (skip_batch), frozen text encoder, step().  Under data parallelism
        every rank iterates ITS shard of the data with the same number of batches.  Returns the number of steps taken."""
        dev = next(self.G.parameters()).device
        steps = 0
        for n, batch in enumerate(batches):
            if max_batches is not None and n >= max_batches:
                break
            words, lengths, class_ids, img64, img128, img256 = batch
            if self.skip_batch(lengths, len(words), batch_size):
                continue
            with torch.no_grad():
                word_embs, sent_embs = text_encoder(words.to(dev), lengths)
            cids = class_ids.detach().cpu().numpy() if isinstance(class_ids, Tensor) else class_ids      # train.py:114
            self.step(word_embs.contiguous(), sent_embs.contiguous(), lengths, cids, [img64.to(dev), img128.to(dev), img256.to(dev)])
            steps += 1
        return steps


@torch.no_grad()
def sample_fakes(G: Module, word_embs: Tensor, sent_embs: Tensor, mask: Tensor, rng: torch.Generator, noise: Optional[Tensor] = None,
                 eps: Optional[Tensor] = None, train_mode_bn: bool = False) -> List[Tensor]:
    """The one sampling path (GanTrainStep.generate_images, evaluation.Evaluator): the generator's images in [-1, 1], one per stage,
    under no_grad, in eval mode unless train_mode_bn; noise and eps that are not given are drawn from `rng`, noise first.  The
    generator's mode is restored."""
    was_training = G.training
    G.train(bool(train_mode_bn))
    try:
        b = word_embs.shape[0]
        if noise is None:
            noise = torch.randn(b, G.z_dim, dtype=torch.float32, device=word_embs.device, generator=rng)
        if eps is None:
            eps = torch.randn(b, G.cond_dim, dtype=torch.float32, device=word_embs.device, generator=rng)
        fakes, _, _, _ = G(noise, sent_embs, word_embs, mask, eps)
        return fakes
    finally:
        G.train(was_training)


class GraphedStep:
    """A captured train step: `replay()` runs it; `out` holds the static result tensors (losses, fake images)."""

    def __init__(self, graph, out: Dict[str, Tensor], trainer: "GanTrainStep"):
        self.graph, self.out, self.t = graph, out, trainer

    def replay(self) -> Dict[str, Tensor]:
        self.graph.replay()
        self.t._mark_replayed()
        return self.out


class SegmentedStep:
    """The graphs of GanTrainStep.capture_segments and the eager gradient exchange between them; `replay()` runs one train step."""

    def __init__(self, trainer: "GanTrainStep"):
        self.t = trainer
        self.gen_forward = None
        self.d_backward: Dict[int, object] = {}
        self.d_adam: Dict[int, object] = {}
        self.g_backward = self.g_adam = None
        self.dw_backward = self.dw_adam = None              # with a word-level discriminator only
        self.out: Dict[str, Tensor] = {}

    def replay(self) -> Dict[str, Tensor]:
        t = self.t
        main = torch.cuda.current_stream()
        self.gen_forward.replay()
        streams = t._d_streams(len(t.Ds), next(t.G.parameters()).device)
        for i in t.d_order:                                # largest discriminator first: its exchange travels under the others' graphs
            with _forked(streams, i, main):
                self.d_backward[i].replay()
                t.d_buckets[i].exchange_all()              # on the comm stream, behind this stream; this stream waits for it
                self.d_adam[i].replay()
        for st in streams:
            main.wait_stream(st)
        if self.dw_backward is not None:
            self.dw_backward.replay()
            t.w_buckets.exchange_all()
            self.dw_adam.replay()
        self.g_backward.replay()
        t.g_buckets.exchange_all()
        self.g_adam.replay()
        t._mark_replayed()
        return self.out


class DAMSMTrainStep(ModelTrainer):
    """One batch of DAMSMTrainer.pretrain_damsm (pretrain_damsm.py:114-134): image encoder on the 256x256 image, text encoder
    on the captions, words + sentence loss (HIP kernels), clip_grad_norm_(RNN, 0.25), one Adam(lr 2e-3, betas (0.5, 0.999))
    over the RNN parameters and the image encoder's trainable heads.  The encoders are the caller's modules: by default stock PyTorch-ROCm
    ones; `RNNEncoder(..., backend="hip")` runs the text encoder's forward and backward-through-time on the library's kernels, and
    `CNNEncoder(..., backend="hip", hip_train=True)` the image encoder's train-mode trunk (batch-statistics BatchNorm, running
    statistics updated; with backend="hip" alone CNNEncoder's train mode is stock)."""

    def __init__(self, rnn: Module, cnn: Module, lr: float = 2e-3, rnn_grad_clip: float = 0.25, gamma1: float = 4.0,
                 gamma2: float = 5.0, gamma3: float = 10.0, wlambda: float = 5.0, slambda: float = 5.0):
        super().__init__()
        self.rnn, self.cnn, self.clip = rnn, cnn, rnn_grad_clip
        # ONE Adam over the RNN and the image encoder's trainable heads (pretrain_damsm.py:69-73), as one fused launch on a flat
        # buffer; the RNN's parameters come first so that clip_grad_norm_ (:133) sees them as one contiguous slice
        params = list(rnn.parameters()) + [p for p in cnn.parameters() if p.requires_grad]
        self.optim = FlatAdam(params, lr=lr, betas=(0.5, 0.999))
        self._rnn_count = sum(1 for p in rnn.parameters() if p.requires_grad)
        dev = next(rnn.parameters()).device
        self.words_loss = WordsLoss(dev, gamma1, gamma2, gamma3, wlambda)
        self.sent_loss = SentenceLoss(dev, gamma3, slambda)
        self.loss_history: List = []

    def step(self, captions: Tensor, lengths, class_ids, img256: Tensor) -> Dict[str, Tensor]:
        b = captions.shape[0]
        labels = self._make_match_labels(b)
        words_features, sent_code = self.cnn(img256)
        word_embs, sent_embs = self.rnn(captions, lengths)
        self.optim.zero_grad()
        wloss, _ = self.words_loss.get_loss(words_features, word_embs, labels, lengths, class_ids)
        sloss = self.sent_loss.get_loss(sent_code, sent_embs, labels, class_ids)
        loss = wloss + sloss
        loss.backward()
        self.optim.join_and_rebind()                       # every p.grad is now its slice of the flat gradient buffer
        torch.nn.utils.clip_grad_norm_(self.rnn.parameters(), self.clip)       # scales those slices in place (pretrain_damsm.py:133)
        self.optim.step()
        self.loss_history.append(loss.detach())
        return {"loss": loss.detach(), "w_loss": wloss.detach(), "s_loss": sloss.detach()}
