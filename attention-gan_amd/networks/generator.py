"""Three-stage AttnGAN generator with the reference's interface (networks/generator.py:12-66)."""
from __future__ import annotations

from typing import List, Optional, Tuple

from torch import Tensor, nn

from .generator_submodules import GenInitialStage, GenMakeImage, GenNextStage, VarAutoEncoder


class Generator(nn.Module):
    """`cond_bn` (not in the reference): the BatchNorm of every upBlock is conditional on the CA-net code `condition`
    (utilities/layers.py: HipCondBatchNorm2d), which then reaches every scale and trains the CA-net through it.  Its extra weights
    ('...2.cond.weight', one per upBlock) start at zero without a random draw: under one seed every other parameter equals the
    unconditional generator's, and so does the function until they are trained.  Warm start: load an unconditional checkpoint with
    strict=False -- only those keys are reported missing and they stay zero.

    `self_attn` (not in the reference): 32 or 64 puts a self-attention block (utilities/layers.py: SelfAttention2d, keys
    `gen1.self_attn.{qkv.weight, proj.weight, gamma}`) on the 32x32 map (between gen1.upsample3 and upsample4, 2 gf_dim channels) or
    the 64x64 map (after upsample4, gf_dim channels) of the initial stage.  The block is built LAST, because its two convs draw from
    the torch RNG: under one seed every other parameter equals the plain generator's, and with gamma = 0 so does the function.
    Warm start: load a plain checkpoint with strict=False -- exactly the three new keys are reported missing.

    `memory` (not in the reference): every refinement stage (gen2, gen3) replaces its attention module and the concat by a dynamic
    memory (networks/memory.py: DynamicMemory, DM-GAN's stage; keys `gen{2,3}.memory.{word,image,kv,response}.{weight,bias}`, no
    `gen{2,3}.attention.*`), `memory_dim` wide (None: 2 emb_dim).  gf_dim <= 64 and at most 64 words.  Its layers draw from the torch RNG
    where the attention's conv drew, so a memory generator shares neither initial values nor checkpoints with the plain one.

    `channel_attn` (not in the reference): every refinement stage also runs ControlGAN's channel-wise word attention
    (networks/attention.py: ChannelAttention) next to its attention module, on the 64 x 64 (gen2), 128 x 128 (gen3) and, in Generator4,
    256 x 256 (gen4) map, and concatenates its output as a third part: the residual blocks are 3 gf_dim wide and the up block is
    upBlock(3 gf_dim, gf_dim).  New keys `gen{2,3}.channel_attn.perception.weight` [hw * hw, emb_dim]; `gen{2,3}.attention.conv1.weight`
    stays.  gf_dim <= 64 and at most 64 words.  A plain checkpoint does NOT load into it (the residual and up-block shapes differ), and
    the initial values differ from the plain generator's from gen2 on.  Combines with `cond_bn` and `self_attn`; together with `memory`
    it is a ValueError (the memory stage has its own channel plan).  The defaults build exactly the plain generator."""

    # side of the map each refinement stage reads
    _STAGE_HW = {"gen2": 64, "gen3": 128, "gen4": 256}

    def __init__(self, gf_dim: int, emb_dim: int, z_dim: int, cond_dim: int, cond_bn: bool = False, self_attn: Optional[int] = None,
                 _defer_self_attn: bool = False, memory: bool = False, memory_dim: Optional[int] = None, channel_attn: bool = False):
        super().__init__()
        self.gf_dim, self.emb_dim, self.z_dim, self.cond_dim, self.cond_bn = gf_dim, emb_dim, z_dim, cond_dim, bool(cond_bn)
        self.memory, self.memory_dim, self.channel_attn = bool(memory), memory_dim, bool(channel_attn)
        if self.memory and self.channel_attn:
            raise ValueError("memory=True and channel_attn=True do not combine: the memory stage has its own channel plan")
        # creation order = the reference's, so the same torch seed yields the same initial weights
        self.vae = VarAutoEncoder(emb_dim=emb_dim, cond_dim=cond_dim)
        self.gen1 = GenInitialStage(gf_dim=gf_dim * 16, z_dim=z_dim, cond_dim=cond_dim, cond_bn=cond_bn)
        self.img_out1 = GenMakeImage(gf_dim=gf_dim)
        self.gen2 = self._next_stage("gen2")
        self.img_out2 = GenMakeImage(gf_dim=gf_dim)
        self.gen3 = self._next_stage("gen3")
        self.img_out3 = GenMakeImage(gf_dim=gf_dim)
        if not _defer_self_attn:         # (a subclass with further stages adds the block after them)
            self.gen1.add_self_attn(self_attn)

    def _next_stage(self, name: str) -> GenNextStage:
        return GenNextStage(gf_dim=self.gf_dim, emb_dim=self.emb_dim, num_residual_blocks=2,
                            cond_bn_dim=self.cond_dim if self.cond_bn else None, memory=self.memory, memory_dim=self.memory_dim,
                            channel_attn_hw=self._STAGE_HW[name] if self.channel_attn else None)

    def _run_stage(self, stage: GenNextStage, images: Tensor, word_embs: Tensor, mask: Tensor, condition: Tensor):
        if self.cond_bn:
            return stage(images, word_embs, mask, condition)
        return stage(images, word_embs, mask)

    def forward(self, noise: Tensor, sent_emb: Tensor, word_embs: Tensor, mask: Tensor, eps: Optional[Tensor] = None):
        """(noise [B,z], sent_emb [B,emb], word_embs [B,emb,T], mask [B,T]) ->
        (fake_imgs [64,128,256], attn_maps [64x64, 128x128], mu, logvar) -- the reference returns 2 attention maps
        (generator.py:59,64) despite its docstring."""
        fake_imgs: List[Tensor] = []
        attn_maps: List[Tensor] = []
        condition, mu, logvar = self.vae(sent_emb, eps)
        images = self.gen1(noise, condition)
        fake_imgs.append(self.img_out1(images))
        for stage, head in ((self.gen2, self.img_out2), (self.gen3, self.img_out3)):
            images, attn = self._run_stage(stage, images, word_embs, mask, condition)
            fake_imgs.append(head(images))
            attn_maps.append(attn)
        return (fake_imgs, attn_maps, mu, logvar)


class Generator1(nn.Module):
    """Stage-1 only (BASELINE.json configs[1]: 64x64 G + D): the CA-net, the initial stage and its image head of the generator
    above (generator.py:26-30 of the reference), nothing of stages 2 / 3 -- same submodule names, so a full Generator's
    `vae.*`, `gen1.*`, `img_out1.*` entries load into it.  forward() keeps the Generator's signature and return shape
    (one image, no attention maps), so trainers.GanTrainStep drives it with a single discriminator."""

    def __init__(self, gf_dim: int, emb_dim: int, z_dim: int, cond_dim: int, cond_bn: bool = False, self_attn: Optional[int] = None):
        super().__init__()
        self.gf_dim, self.emb_dim, self.z_dim, self.cond_dim, self.cond_bn = gf_dim, emb_dim, z_dim, cond_dim, bool(cond_bn)
        self.vae = VarAutoEncoder(emb_dim=emb_dim, cond_dim=cond_dim)
        self.gen1 = GenInitialStage(gf_dim=gf_dim * 16, z_dim=z_dim, cond_dim=cond_dim, cond_bn=cond_bn)
        self.img_out1 = GenMakeImage(gf_dim=gf_dim)
        self.gen1.add_self_attn(self_attn)         # last: see Generator

    def forward(self, noise: Tensor, sent_emb: Tensor, word_embs: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                eps: Optional[Tensor] = None):
        condition, mu, logvar = self.vae(sent_emb, eps)
        return ([self.img_out1(self.gen1(noise, condition))], [], mu, logvar)
