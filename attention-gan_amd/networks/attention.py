"""Word-context attention with the reference's interface (networks/attention.py), one HIP pass per direction."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from ..backend import functional as HF
from ..backend import lib as L
from ..utilities.layers import HipLinear, Layers


class AttentionModule(nn.Module):
    """Drop-in for reference AttentionModule (attention.py:15-79): same ctor, `apply_mask`, `forward` and the
    single parameter `conv1.weight` [nc_in, emb_dim, 1, 1]."""

    def __init__(self, nc_in: int, emb_dim: int):
        super().__init__()
        self.nc_in = nc_in
        self.conv1 = Layers.conv1x1(in_planes=emb_dim, out_planes=nc_in)
        self.mask = None

    def apply_mask(self, mask: Tensor) -> None:
        self.mask = mask

    def forward(self, images: Tensor, words: Tensor, scaled=True) -> Tuple[Tensor, Tensor]:
        """images [B,nc_in,h,w], words [B,emb_dim,T], self.mask [B,T] (0 = ignore) -> (context [B,nc_in,h,w], attn [B,T,h,w])."""
        (batch, nc_in, h, w) = images.shape
        (batch_w, emb_dim, seq_len) = words.shape
        (batch_m, seq_len_m) = self.mask.shape       # raises like the reference if no mask was applied
        return HF.attention(images, words, self.conv1.weight, self.mask, scaled)


class ChannelAttention(nn.Module):
    """Channel-wise word attention (ControlGAN, Li et al., NeurIPS 2019; not in the reference), the companion of AttentionModule:
    there every pixel attends over the words, here every CHANNEL of the stage's feature map does, seeing each word through a learned
    per-position projection.  With N = hw * hw, p a pixel and F = perception.weight [N, emb_dim]:

      perceive  wt[b, t, p] = sum_e F[p, e] words[b, e, t]                 (HF.linear on the B * T rows of words^T: its output IS wt)
      score     m[b, c, t]  = scale * sum_p images[b, c, p] wt[b, t, p]    masked words: -inf
      attend    alpha[b, c, :] = softmax_t m[b, c, :]
      read      f[b, c, p]  = sum_t alpha[b, c, t] wt[b, t, p]             (score, attend, read: HF.channel_attention)

    `apply_mask`, then forward(images [B, nc_in, hw, hw], words [B, emb_dim, T]) -> (f [B, nc_in, hw, hw], alpha [B, nc_in, T]).
    One parameter, `perception.weight`: the map size is part of the module, and another size is a ValueError.  nc_in <= 64, T <= 64.

    `scale`: the paper has none.  That is `scale=1.0`; the default None means 1 / sqrt(N), A DEPARTURE FROM THE PAPER: the score sums
    N products, and at N = 4096 with the default nn.Linear init the unscaled softmax is one-hot at initialisation (float64, Generator(4,
    16, 10, 10), B 3, T 5, seeds 1..3: the median over the (b, c) rows of max_t alpha is 0.9993 .. 1.0000; with 1 / sqrt(N) it is
    0.38 .. 0.45 and no row is above 0.67).  fp32 in every precision mode (the modes change how the perception layer multiplies);
    16-bit activation storage raises.  A sample whose words are all masked gives NaN, as AttentionModule does."""

    def __init__(self, nc_in: int, emb_dim: int, hw: int, scale: Optional[float] = None):
        super().__init__()
        if isinstance(hw, bool) or not isinstance(hw, int) or hw < 1:
            raise ValueError(f"hw={hw!r}: the side of the square feature map, a positive integer")
        self.nc_in, self.emb_dim, self.hw = nc_in, emb_dim, hw
        self.scale = None if scale is None else float(scale)
        self.perception = HipLinear(emb_dim, hw * hw, bias=False)
        self.mask = None

    def apply_mask(self, mask: Tensor) -> None:
        self.mask = mask

    def forward(self, images: Tensor, words: Tensor) -> Tuple[Tensor, Tensor]:
        if HF.get_activation_storage() != L.DT_F32 or images.dtype != torch.float32:
            raise L.AganError("ChannelAttention: the channel-attention kernels are fp32 only; 16-bit activation storage "
                              "(set_activation_storage) is not built for them")
        (batch, nc_in, h, w) = images.shape
        (batch_w, emb_dim, seq_len) = words.shape
        (batch_m, seq_len_m) = self.mask.shape       # raises like AttentionModule if no mask was applied
        if h != self.hw or w != self.hw:
            raise ValueError(f"ChannelAttention was built for {self.hw} x {self.hw} maps (perception.weight has {self.hw * self.hw} rows), "
                             f"got {h} x {w}")
        wt = self.perception(words.transpose(1, 2).reshape(batch_w * seq_len, emb_dim)).view(batch_w, seq_len, h * w)
        return HF.channel_attention(images, wt, self.mask, self.scale)


def func_attention(query: Tensor, context: Tensor, gamma1=4.0, scaled=True):
    """Parameter-free DAMSM attention (reference attention.py:82-120): query [B,D,L], context [B,D,ih,iw] ->
    (weightedContext [B,D,L], attn [B,L,ih,iw])."""
    return HF.func_attention(query, context, gamma1, scaled)
