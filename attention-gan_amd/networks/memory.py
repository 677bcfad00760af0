"""Dynamic memory for a refinement stage (DM-GAN, Zhu et al., CVPR 2019; not in the reference), on the HIP kernels of csrc/memory.hip."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from ..backend import functional as HF
from ..backend import lib as L
from ..utilities.layers import HipConv2d, HipLinear


class DynamicMemory(nn.Module):
    """Takes AttentionModule's place in a refinement stage: `apply_mask`, then forward(images [B, nc_in, h, w], words [B, emb_dim, T])
    -> (x [B, 2 nc_in, h, w], attn [B, T, h, w]), where x is what the stage's residual blocks consume (the response r twice along the
    channels, DM-GAN's channel plan) -- there is no torch.cat after it.

      write    hbar = mean over the pixels of images, DETACHED;  U = word(words[b, :, t]);  Q = image(hbar[b])
               g = sigmoid(U[Md] + Q[Md]);  m[b, t, :] = relu(U[:Md]) g + relu(Q[:Md]) (1 - g)                    (HF.memory_write)
      address  kv = relu(kv(m)): keys kv[:, :, :nc_in], values kv[:, :, nc_in:];  attn = softmax over the live words of k . images
      respond  o = v . attn;  g_r = sigmoid(response(cat(images, o)));  r = images (1 - g_r) + g_r o              (HF.memory_read)

    Parameters (the state_dict keys): word = Linear(emb_dim, Md + 1), image = Linear(nc_in, Md + 1), kv = Linear(Md, 2 nc_in),
    response.weight [1, 2 nc_in, 1, 1] and response.bias [1] (a 1x1 conv's parameters; the gate itself runs inside the read kernel).
    memory_dim Md defaults to 2 emb_dim.  nc_in <= 64 and T <= 64.  Everything of size B x T runs on HF.linear, HF.activation and the
    write kernel; fp32 in every precision mode (the modes change how the three linear layers multiply); 16-bit activation storage
    raises."""

    def __init__(self, nc_in: int, emb_dim: int, memory_dim: Optional[int] = None):
        super().__init__()
        if memory_dim is None:
            memory_dim = 2 * emb_dim
        if isinstance(memory_dim, bool) or not isinstance(memory_dim, int) or memory_dim < 1:
            raise ValueError(f"memory_dim={memory_dim!r}: a positive integer, or None for 2 * emb_dim")
        self.nc_in, self.emb_dim, self.memory_dim = nc_in, emb_dim, memory_dim
        self.word = HipLinear(emb_dim, memory_dim + 1)
        self.image = HipLinear(nc_in, memory_dim + 1)
        self.kv = HipLinear(memory_dim, 2 * nc_in)
        self.response = HipConv2d(2 * nc_in, 1, 1, 1, 0, bias=True)         # parameter holder
        self.mask = None

    def apply_mask(self, mask: Tensor) -> None:
        self.mask = mask

    def forward(self, images: Tensor, words: Tensor) -> Tuple[Tensor, Tensor]:
        if HF.get_activation_storage() != L.DT_F32 or images.dtype != torch.float32:
            raise L.AganError("DynamicMemory: the memory kernels store fp32 only; 16-bit activation storage "
                              "(set_activation_storage) is not built for them")
        (batch, nc_in, h, w) = images.shape
        (batch_w, emb_dim, seq_len) = words.shape
        (batch_m, seq_len_m) = self.mask.shape       # raises like AttentionModule if no mask was applied
        Md = self.memory_dim
        U = self.word(words.transpose(1, 2).reshape(batch_w * seq_len, emb_dim)).view(batch_w, seq_len, Md + 1)
        Q = self.image(HF.spatial_mean(images))
        m = HF.memory_write(U, Q)
        kv = HF.activation(self.kv(m.view(batch_w * seq_len, Md)), L.ACT_RELU).view(batch_w, seq_len, 2 * nc_in)
        return HF.memory_read(images, kv, self.mask, self.response.weight, self.response.bias)
