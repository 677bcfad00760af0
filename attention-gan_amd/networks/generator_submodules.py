"""Generator stages with the reference's constructors, forward signatures and parameter names
(networks/generator_submodules.py), executed on the HIP kernels."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from ..backend import functional as HF
from ..backend import lib as L
from ..utilities.layers import GLU, HipBatchNorm1d, HipConv2d, HipLinear, Layers, SelfAttention2d
from .attention import AttentionModule, ChannelAttention
from .memory import DynamicMemory


class _FcBnGlu(nn.Module):
    """Linear(no bias) -> BatchNorm1d -> GLU with the reference Sequential's keys '0.weight', '1.*' (:36-40)."""

    def __init__(self, fin: int, fout: int):
        super().__init__()
        self.add_module("0", HipLinear(fin, fout, bias=False))
        self.add_module("1", HipBatchNorm1d(fout))

    def forward(self, x: Tensor) -> Tensor:
        return getattr(self, "1").fused(getattr(self, "0")(x), L.ACT_GLU)


class GenInitialStage(nn.Module):
    """(noise, condition) -> [B, gf_dim/16, 64, 64]: fc+BN1d+GLU, view [B,gf_dim,4,4], four upBlocks (:13-66).  `cond_bn`: the
    upBlocks' BatchNorms are conditional on `condition` as well (not in the reference).  `self_attn` (not in the reference): the
    feature-map size at which a SelfAttention2d block sits -- 32: between upsample3 and upsample4 (gf_dim/8 channels), 64: after
    upsample4 (gf_dim/16 channels); None: no block, no module, no key."""

    def __init__(self, gf_dim: int, z_dim: int, cond_dim: int, cond_bn: bool = False, self_attn: Optional[int] = None):
        super().__init__()
        self.gf_dim, self.z_dim, self.cond_dim, self.cond_bn = gf_dim, z_dim, cond_dim, bool(cond_bn)
        self.self_attn, self._self_attn_after = None, 0
        self.define_module()
        self.add_self_attn(self_attn)

    def add_self_attn(self, at: Optional[int]) -> None:
        """Constructs the block (keys `self_attn.*`).  Its two convs draw from the torch RNG, so a network that wants every other
        parameter to equal the plain network's under one seed calls this AFTER it has built everything else (Generator does)."""
        if at is None:
            return
        if at not in (32, 64):
            raise ValueError(f"self_attn={at!r}: the block sits on the 32x32 or the 64x64 map of the initial stage (32, 64 or None)")
        if self.self_attn is not None:
            raise ValueError("this stage already has a self-attention block")
        self._self_attn_after = 3 if at == 32 else 4
        self.self_attn = SelfAttention2d(self.gf_dim // (8 if at == 32 else 16))

    def define_module(self):
        ng = self.gf_dim
        self.fc = _FcBnGlu(self.z_dim + self.cond_dim, ng * 4 * 4 * 2)
        cd = self.cond_dim if self.cond_bn else None
        self.upsample1 = Layers.upBlock(ng, ng // 2, cd)
        self.upsample2 = Layers.upBlock(ng // 2, ng // 4, cd)
        self.upsample3 = Layers.upBlock(ng // 4, ng // 8, cd)
        self.upsample4 = Layers.upBlock(ng // 8, ng // 16, cd)

    def forward(self, noise: Tensor, condition: Tensor) -> Tensor:
        x = self.fc(torch.cat((noise, condition), 1)).view(-1, self.gf_dim, 4, 4)
        for i, up in enumerate((self.upsample1, self.upsample2, self.upsample3, self.upsample4)):
            x = up(x, condition) if self.cond_bn else up(x)
            if self._self_attn_after == i + 1:
                x = self.self_attn(x)
        return x


class GenNextStage(nn.Module):
    """attention -> concat -> residual blocks -> upBlock (:69-120).  Returns (images [B,gf,2h,2w], attn [B,T,h,w]).
    `cond_bn_dim`: the upBlock's BatchNorm is conditional on a [B, cond_bn_dim] code that forward() then takes (not in the
    reference); the residual blocks' BatchNorms stay as they are.  `memory` (not in the reference): a DynamicMemory (networks/memory.py,
    keys `memory.*`, `memory_dim` wide) stands where the attention module and the concat stand -- the stage then has no `attention`
    child, and the residual blocks run on the module's [B, 2 gf_dim, h, w] output.  `channel_attn_hw` (not in the reference): the side
    of the stage's input map; a ChannelAttention (networks/attention.py, key `channel_attn.perception.weight` [hw * hw, emb_dim]) then
    runs next to the attention module and the stage is cat(images, context, f) -> residual blocks of width 3 gf_dim ->
    upBlock(3 gf_dim, gf_dim); the returned map is still the spatial one.  Not together with `memory`, which has its own channel plan."""

    def __init__(self, gf_dim: int, emb_dim: int, num_residual_blocks: int, cond_bn_dim: Optional[int] = None, memory: bool = False,
                 memory_dim: Optional[int] = None, channel_attn_hw: Optional[int] = None):
        super().__init__()
        self.gf_dim, self.emb_dim, self.num_residual_blocks, self.cond_bn_dim = gf_dim, emb_dim, num_residual_blocks, cond_bn_dim
        self.use_memory, self.memory_dim, self.channel_attn_hw = bool(memory), memory_dim, channel_attn_hw
        if memory_dim is not None and not self.use_memory:
            raise ValueError("memory_dim is the width of the dynamic memory: it needs memory=True")
        if channel_attn_hw is not None and self.use_memory:
            raise ValueError("channel_attn_hw and memory=True do not combine: the memory stage has its own channel plan")
        self.define_module()

    def define_module(self):
        if self.use_memory:
            self.memory = DynamicMemory(nc_in=self.gf_dim, emb_dim=self.emb_dim, memory_dim=self.memory_dim)
        else:
            self.attention = AttentionModule(nc_in=self.gf_dim, emb_dim=self.emb_dim)
        width = 2
        if self.channel_attn_hw is not None:
            self.channel_attn = ChannelAttention(nc_in=self.gf_dim, emb_dim=self.emb_dim, hw=self.channel_attn_hw)
            width = 3
        self.residual = self._make_layer(Layers.ResBlock, self.gf_dim * width)
        self.upsample = Layers.upBlock(self.gf_dim * width, self.gf_dim, self.cond_bn_dim)

    def _make_layer(self, block, channel_num: int):
        return nn.Sequential(*[block(channel_num) for _ in range(self.num_residual_blocks)])

    def forward(self, images: Tensor, word_embs: Tensor, mask: Tensor, condition: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        if self.cond_bn_dim is not None and condition is None:
            raise ValueError("GenNextStage was built with cond_bn_dim: forward() needs the [B, cond_bn_dim] condition")
        if self.use_memory:
            self.memory.apply_mask(mask=mask)
            x, attn = self.memory(images, word_embs)
            x = self.residual(x)
        else:
            self.attention.apply_mask(mask=mask)
            context, attn = self.attention(images, word_embs)
            if self.channel_attn_hw is None:
                x = self.residual(torch.cat((images, context), 1))
            else:
                self.channel_attn.apply_mask(mask=mask)
                f, _ = self.channel_attn(images, word_embs)
                x = self.residual(torch.cat((images, context, f), 1))
        if self.cond_bn_dim is None:
            return self.upsample(x), attn
        return self.upsample(x, condition), attn


class _ConvTanh(nn.Module):
    """conv3x3(gf,3) + tanh with the reference Sequential's key '0.weight' (:134-138)."""

    def __init__(self, gf_dim: int):
        super().__init__()
        self.add_module("0", HipConv2d(gf_dim, 3, 3, 1, 1, False))

    def forward(self, x: Tensor) -> Tensor:
        return HF.activation(getattr(self, "0")(x), L.ACT_TANH)


class GenMakeImage(nn.Module):
    def __init__(self, gf_dim: int):
        super().__init__()
        self.gf_dim = gf_dim
        self.img = _ConvTanh(gf_dim)

    def forward(self, images: Tensor) -> Tensor:
        return self.img(images)


class VarAutoEncoder(nn.Module):
    """Conditioning augmentation (:145-170): Linear(emb, 4*cond) -> GLU -> (mu, logvar); c = eps*exp(logvar/2)+mu.

    The reference draws eps with torch.cuda.FloatTensor(...).normal_() (:163); here it is torch.randn on the
    input's device.  `forward(text_embedding, eps=None)` accepts an explicit eps so tests can replay a recorded draw.
    """

    def __init__(self, emb_dim: int, cond_dim=100):
        super().__init__()
        self.emb_dim, self.cond_dim = emb_dim, cond_dim
        self.fc = HipLinear(emb_dim, cond_dim * 4, bias=True)
        self.relu = GLU()

    def encode(self, text_embedding: Tensor):
        x = self.relu(self.fc(text_embedding))
        return x[:, :self.cond_dim], x[:, self.cond_dim:]

    def reparametrize(self, mu: Tensor, logvar: Tensor, eps: Optional[Tensor] = None) -> Tensor:
        if eps is None:
            eps = torch.randn(mu.shape, dtype=mu.dtype, device=mu.device)
        return HF.reparametrize(mu, logvar, eps)

    def forward(self, text_embedding: Tensor, eps: Optional[Tensor] = None):
        mu, logvar = self.encode(text_embedding)
        return self.reparametrize(mu, logvar, eps), mu, logvar
