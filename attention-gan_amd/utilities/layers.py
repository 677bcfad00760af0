"""`Layers` factory with the reference's names and state_dict keys, running on the gfx950 kernels.

Mirrors utilities/layers.py of the reference (factory names, argument meaning, parameter names / Sequential
indices, default initialisation and RNG consumption order) but every block executes as fused HIP stages:

    conv (implicit GEMM, MFMA)  ->  batch statistics  ->  normalise + GLU / LeakyReLU / residual add

`nn.Upsample` never runs: an upBlock's nearest-x2 + conv3x3 is folded into four parity-class 2x2 convolutions on
the low-resolution input (include/agan.h), so the 4x larger tensor is never written or read.
"""
from __future__ import annotations

from math import floor
from typing import List, Optional, Sequence

import torch
from torch import Tensor, nn

from ..backend import functional as HF
from ..backend import lib as L


class SpectralState:
    """mixin of a weight holder under spectral normalisation (Miyato et al. 2018; HF.spectral_weight): the parameter is `weight_orig`,
    the power iteration's state the buffers `weight_u` [Cout] and `weight_v` [K] -- the state_dict keys of
    torch.nn.utils.spectral_norm, whose modules load these entries with strict=True and the other way round.  u and v are drawn as
    normalised N(0, 1) vectors (`draw=False` leaves them zero for an owner that draws later: draw_spectral_state_).  A checkpoint
    that has `weight` and no `weight_orig` loads as a warm start: `weight` becomes `weight_orig`, u and v stay as they are."""

    spectral = False

    def _init_spectral(self, draw: bool = True) -> None:
        self.spectral = True
        w = self.weight
        del self._parameters["weight"]
        self.register_parameter("weight_orig", w)
        self.register_buffer("weight_u", w.detach().new_zeros(w.shape[0]))
        self.register_buffer("weight_v", w.detach().new_zeros(w.numel() // w.shape[0]))
        if draw:
            self.draw_spectral_state_()

    @torch.no_grad()
    def draw_spectral_state_(self) -> None:
        for b in (self.weight_u, self.weight_v):
            b.copy_(nn.functional.normalize(b.normal_(0, 1), dim=0, eps=1e-12))

    def weight_sn(self) -> Tensor:
        """this forward's normalised weight: one power iteration in train mode, none in eval mode (torch's rule)"""
        return HF.spectral_weight(self.weight_orig, self.weight_u, self.weight_v, self.training)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        if self.spectral and prefix + "weight" in state_dict and prefix + "weight_orig" not in state_dict:
            state_dict[prefix + "weight_orig"] = state_dict.pop(prefix + "weight")      # (load_state_dict works on its own copy)
            for name in ("weight_u", "weight_v"):
                state_dict.setdefault(prefix + name, getattr(self, name))
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


def draw_spectral_state_(module: nn.Module) -> None:
    """draw u and v of every spectrally normalised holder inside `module`, in module order (for owners that built them with draw=False)"""
    for m in module.modules():
        if getattr(m, "spectral", False):
            m.draw_spectral_state_()


class HipConv2d(SpectralState, nn.Conv2d):
    """Parameter holder with nn.Conv2d's init; forward is the HIP implicit-GEMM conv.  `spectral=True`: the weight is divided by its
    largest singular value at every forward (SpectralState); the normalised weight is a fresh tensor per call, so the conv runs
    without a pack cache and without a flat gradient destination -- HF.spectral_weight's backward writes the parameter's gradient."""

    def __init__(self, cin: int, cout: int, k: int, stride: int, pad: int, bias: bool, kind: Optional[str] = None, spectral: bool = False,
                 draw: bool = True):
        super().__init__(cin, cout, kernel_size=k, stride=stride, padding=pad, bias=bias)
        if kind is None:
            if stride == 1 and pad == (k - 1) // 2 and k % 2 == 1:
                kind = "same"
            elif stride == 2 and k == 4 and pad == 1:
                kind = "down"
            elif 1 <= k <= 5 and 1 <= stride <= 3 and 0 <= pad <= 3:
                kind = "any"         # the general trainable conv (include/agan.h: agan_conv2d_train_*)
            else:
                raise NotImplementedError(f"conv k={k} s={stride} p={pad} is not on the AttnGAN hot path")
        self.kind = kind
        self._packed = {}        # packed-weight cache (layout copies for the kernels; not part of state_dict)
        if spectral:
            self._init_spectral(draw)

    def forward(self, x: Tensor, act: int = L.ACT_NONE, handoff_out=None, handoff_in=None) -> Tensor:
        """`act` (only where HF.conv_fuses_activation allows it) applies the following activation in the conv epilogue;
        the handoffs link such a conv to its single consumer (HF.ActHandoff)."""
        if self.spectral:
            return self._forward_spectral(x, act, handoff_out, handoff_in)
        if self.kind == "any":       # no fused activation, no handoff (FusedChain.run never asks for one)
            return HF.conv2d(x, self.weight, self.bias, "any", None, HF.grad_dst(self.weight),
                             HF.grad_dst(self.bias) if self.bias is not None else None, act, handoff_out, None,
                             self.stride, self.padding)
        return HF.conv2d(x, self.weight, self.bias, self.kind, self._packed, HF.grad_dst(self.weight),
                         HF.grad_dst(self.bias) if self.bias is not None else None, act, handoff_out, handoff_in)

    def _forward_spectral(self, x: Tensor, act: int, handoff_out, handoff_in) -> Tensor:
        """the conv on this forward's normalised weight: no pack cache and no flat destination for a tensor that is new at every call"""
        bdst = HF.grad_dst(self.bias) if self.bias is not None else None
        if self.kind == "any":
            return HF.conv2d(x, self.weight_sn(), self.bias, "any", None, None, bdst, act, handoff_out, None, self.stride, self.padding)
        return HF.conv2d(x, self.weight_sn(), self.bias, self.kind, None, None, bdst, act, handoff_out, handoff_in)


class HipLinear(SpectralState, nn.Linear):
    def __init__(self, *args, spectral: bool = False, draw: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        self._packed = {}
        if spectral:
            self._init_spectral(draw)

    def forward(self, x: Tensor) -> Tensor:
        if self.spectral:
            return HF.linear(x, self.weight_sn(), self.bias, None, None, HF.grad_dst(self.bias) if self.bias is not None else None)
        return HF.linear(x, self.weight, self.bias, self._packed, HF.grad_dst(self.weight),
                         HF.grad_dst(self.bias) if self.bias is not None else None)


class _BNState:
    """mixin: fused normalise+activation using this module's affine parameters and running statistics."""

    def fused(self, x: Tensor, act: int, residual: Optional[Tensor] = None) -> Tensor:
        if self.momentum is None or not self.track_running_stats or not self.affine:
            raise NotImplementedError("only the default BatchNorm configuration is on the hot path")
        return HF.bn_act(x, self.weight, self.bias, self.running_mean, self.running_var, self.num_batches_tracked,
                         self.training, act, residual, self.eps, self.momentum)


class HipBatchNorm2d(nn.BatchNorm2d, _BNState):
    def forward(self, x: Tensor) -> Tensor:
        return self.fused(x, L.ACT_NONE)


class HipCondBatchNorm2d(HipBatchNorm2d):
    """BatchNorm2d whose affine terms depend on a per-sample code: gamma[c] + dgamma[b, c], beta[c] + dbeta[b, c] with
    (dgamma, dbeta) = cond(code), one bias-free linear layer (HF.cond_bn_act).  `cond.weight` starts at ZERO and is allocated
    without a draw from the torch RNG, so the module starts as the plain BatchNorm2d it extends, and a network built with it under a
    seed has every other parameter equal to the unconditional network's under that seed."""

    def __init__(self, num_features: int, cond_dim: int):
        super().__init__(num_features)
        self.cond = HipLinear(cond_dim, 2 * num_features, bias=False, device="meta")      # (no storage, no draw)
        self.cond.weight = nn.Parameter(torch.zeros(2 * num_features, cond_dim))

    def forward(self, x: Tensor, condition: Tensor) -> Tensor:
        return self.fused_cond(x, condition, L.ACT_NONE)

    def fused_cond(self, x: Tensor, condition: Tensor, act: int) -> Tensor:
        if self.momentum is None or not self.track_running_stats or not self.affine:
            raise NotImplementedError("only the default BatchNorm configuration is on the hot path")
        return HF.cond_bn_act(x, self.weight, self.bias, self.cond(condition), self.running_mean, self.running_var,
                              self.num_batches_tracked, self.training, act, self.eps, self.momentum)


class SelfAttention2d(nn.Module):
    """Self-attention block over the positions of a feature map (SAGAN's non-local block): x + gamma * proj(attention(qkv(x))),
    where qkv is one bias-free 1x1 conv whose output channels are Dk = max(1, C // qk_ratio) queries, Dk keys and
    Dv = max(1, C // v_ratio) values, the attention is HF.self_attention_qkv with scale 1 and proj a bias-free 1x1 conv back to C.
    `gamma` starts at ZERO: the block starts as the identity, and a network built with it computes what the network without it
    computes until gamma is trained.  The attention and the gate are fp32 in every precision mode (the 16-bit modes change how the
    two convs multiply); 16-bit activation storage raises."""

    def __init__(self, channels: int, qk_ratio: int = 8, v_ratio: int = 2):
        super().__init__()
        self.channels = channels
        self.dk, self.dv = max(1, channels // qk_ratio), max(1, channels // v_ratio)
        self.qkv = HipConv2d(channels, 2 * self.dk + self.dv, 1, 1, 0, bias=False)
        self.proj = HipConv2d(self.dv, channels, 1, 1, 0, bias=False)
        self.gamma = nn.Parameter(torch.zeros(1))

    def forward(self, x: Tensor) -> Tensor:
        if HF.get_activation_storage() != L.DT_F32 or x.dtype != torch.float32:
            raise L.AganError("SelfAttention2d: the self-attention kernels store fp32 only; 16-bit activation storage "
                              "(set_activation_storage) is not built for them")
        return HF.scaled_residual(x, self.proj(HF.self_attention_qkv(self.qkv(x), self.dk, self.dv)), self.gamma)


class HipBatchNorm1d(nn.BatchNorm1d, _BNState):
    def forward(self, x: Tensor) -> Tensor:
        return self.fused(x, L.ACT_NONE)


class GLU(nn.Module):
    """Gated linear unit over channel halves (reference layers.py:13-26)."""

    def forward(self, x: Tensor) -> Tensor:
        assert x.size(1) % 2 == 0, 'channels dont divide 2!'
        return HF.glu(x)


class _Stage:
    __slots__ = ("conv", "bn", "act")

    def __init__(self, conv: str, bn: Optional[str], act: int):
        self.conv, self.bn, self.act = conv, bn, act


class FusedChain(nn.Module):
    """A reference `nn.Sequential` of conv/BN/activation layers, executed stage by stage on the HIP kernels.

    Children are registered under the reference Sequential's integer names so `state_dict()` keys match
    (e.g. upBlock -> '1.weight', '2.weight', '2.running_mean', ...).
    """

    def __init__(self):
        super().__init__()
        self._stages: List[_Stage] = []

    def add_stage(self, conv_idx: int, conv: HipConv2d, bn_idx: Optional[int], act: int, cond_dim: Optional[int] = None) -> "FusedChain":
        """`cond_dim`: the stage's BatchNorm is a HipCondBatchNorm2d on a code of that width, which run() then needs"""
        self.add_module(str(conv_idx), conv)
        if bn_idx is not None:
            self.add_module(str(bn_idx), HipBatchNorm2d(conv.out_channels) if cond_dim is None
                            else HipCondBatchNorm2d(conv.out_channels, cond_dim))
        self._stages.append(_Stage(str(conv_idx), None if bn_idx is None else str(bn_idx), act))
        return self

    def run(self, x: Tensor, residual: Optional[Tensor] = None, condition: Optional[Tensor] = None) -> Tensor:
        last = len(self._stages) - 1
        handoff = None
        for i, st in enumerate(self._stages):
            conv = getattr(self, st.conv)
            if st.bn is None and HF.conv_fuses_activation(st.act, conv.out_channels, conv.kind):
                # conv + LeakyReLU in one kernel (no BatchNorm in between); if a conv of this chain is its only consumer, that
                # conv's dgrad epilogue does the activation backward as well
                handoff = HF.ActHandoff() if i < last else None
                x = conv(x, st.act, handoff, None)
                continue
            y = conv(x, L.ACT_NONE, None, handoff)
            handoff = None
            if st.bn is not None:
                bn = getattr(self, st.bn)
                if isinstance(bn, HipCondBatchNorm2d):
                    if condition is None:
                        raise ValueError("this block's BatchNorm is conditional: forward(x, condition) needs the code")
                    if residual is not None:
                        raise NotImplementedError("the conditional BatchNorm takes no residual")
                    x = bn.fused_cond(y, condition, st.act)
                else:
                    x = bn.fused(y, st.act, residual if i == last else None)
            elif st.act != L.ACT_NONE:
                x = HF.activation(y, st.act)
            else:
                x = y
        return x

    def forward(self, x: Tensor, condition: Optional[Tensor] = None) -> Tensor:
        return self.run(x, condition=condition)


class _ReluChain(FusedChain):
    def forward(self, x: Tensor) -> Tensor:
        return torch.relu(self.run(x))


class ResBlock(nn.Module):
    """conv3x3 C->2C, BN, GLU, conv3x3 C->C, BN, += x   (reference layers.py:156-176; keys block.{0,1,3,4}.*)."""

    def __init__(self, channel_num: int):
        super().__init__()
        c = channel_num
        self.block = (FusedChain()
                      .add_stage(0, HipConv2d(c, c * 2, 3, 1, 1, False), 1, L.ACT_GLU)
                      .add_stage(3, HipConv2d(c, c, 3, 1, 1, False), 4, L.ACT_NONE))

    def forward(self, x: Tensor) -> Tensor:
        return self.block.run(x, residual=x)      # the residual add rides in the last normalise kernel


class Layers:
    """Static factories, same names/arguments as the reference's `Layers`."""

    @staticmethod
    def GLU() -> GLU:
        return GLU()

    @staticmethod
    def calculate_out_hw(hw: int, k: int, s: int, p=0) -> int:
        return floor(((hw + 2 * p - k) / s) + 1)

    @staticmethod
    def conv(in_channels: int, out_channels: int, in_hw: int, out_hw: int, max_kern=4, max_stride=3, max_pad=3) -> nn.Conv2d:
        cands = [(k, s, p) for k in range(1, max_kern + 1) for s in range(1, max_stride + 1) for p in range(max_pad + 1)
                 if Layers.calculate_out_hw(in_hw, k, s, p) == out_hw]
        if not cands:
            raise Exception('Could not find valid parameters to produce output hw')
        k, s, p = max(cands, key=lambda t: (t[0], t[2], t[1]))
        return HipConv2d(in_channels, out_channels, k, s, p, False)

    @staticmethod
    def conv1x1(in_planes: int, out_planes: int, bias=False) -> nn.Conv2d:
        return HipConv2d(in_planes, out_planes, 1, 1, 0, bias)

    @staticmethod
    def conv3x3(in_planes: int, out_planes: int) -> nn.Conv2d:
        return HipConv2d(in_planes, out_planes, 3, 1, 1, False)

    @staticmethod
    def conv4x4DownSpatial(in_planes: int, out_planes: int, bias=True) -> nn.Conv2d:
        return HipConv2d(in_planes, out_planes, 4, 2, 1, bias)

    @staticmethod
    def upBlock(in_planes: int, out_planes: int, cond_dim: Optional[int] = None) -> FusedChain:
        """Upsample(x2) -> conv3x3(in, 2*out) -> BN -> GLU; keys '1.weight', '2.*' (index 0/3 hold no state).  With `cond_dim` the
        BatchNorm is conditional on a [B, cond_dim] code (HipCondBatchNorm2d: one more key, '2.cond.weight') and the block is called
        as forward(x, condition)."""
        return FusedChain().add_stage(1, HipConv2d(in_planes, out_planes * 2, 3, 1, 1, False, kind="up"), 2, L.ACT_GLU, cond_dim)

    @staticmethod
    def upBlockReLU(in_planes: int, out_planes: int) -> FusedChain:
        """Upsample(x2) -> conv3x3(in, out) -> BN -> ReLU (reference layers.py:71-80; unused by the training path): the folded
        upsample conv and the fused BatchNorm of upBlock, followed by a stock ReLU."""
        return _ReluChain().add_stage(1, HipConv2d(in_planes, out_planes, 3, 1, 1, False, kind="up"), 2, L.ACT_NONE)

    @staticmethod
    def downBlockLeakyReLU(in_planes: int, out_planes: int) -> FusedChain:
        return FusedChain().add_stage(0, HipConv2d(in_planes, out_planes, 4, 2, 1, True), 1, L.ACT_LRELU)

    @staticmethod
    def Block3x3_relu(in_planes: int, out_planes: int) -> FusedChain:
        return FusedChain().add_stage(0, HipConv2d(in_planes, out_planes * 2, 3, 1, 1, False), 1, L.ACT_GLU)

    @staticmethod
    def _norm(norm: str) -> bool:
        """is a discriminator block's `norm` the spectral mode?  ("batch", the default: the reference's conv + BatchNorm)"""
        if norm not in ("batch", "spectral"):
            raise ValueError(f"norm={norm!r}: 'batch' or 'spectral'")
        return norm == "spectral"

    # The discriminators' blocks take norm="spectral": the conv is spectrally normalised (HipConv2d(spectral=True)) and the stage has NO
    # BatchNorm (BatchNorm cancels any rescaling of the weight before it) -- conv + LeakyReLU then run as one kernel (FusedChain.run).
    # draw=False leaves u and v for the owner to draw after all its children exist (draw_spectral_state_).
    @staticmethod
    def Block3x3_leakRelu(in_planes: int, out_planes: int, norm: str = "batch", draw: bool = True) -> FusedChain:
        sn = Layers._norm(norm)
        return FusedChain().add_stage(0, HipConv2d(in_planes, out_planes, 3, 1, 1, False, spectral=sn, draw=draw), None if sn else 1,
                                      L.ACT_LRELU)

    @staticmethod
    def downBlock(in_planes: int, out_planes: int, norm: str = "batch", draw: bool = True) -> FusedChain:
        sn = Layers._norm(norm)
        return FusedChain().add_stage(0, HipConv2d(in_planes, out_planes, 4, 2, 1, False, spectral=sn, draw=draw), None if sn else 1,
                                      L.ACT_LRELU)

    @staticmethod
    def encode_image_by_16times(df_dims: int, norm: str = "batch", draw: bool = True) -> FusedChain:
        """Four stride-2 conv4x4 stages 3->df->2df->4df->8df; the first has no BN (keys 0,2,3,5,6,8,9).  norm="spectral": none has,
        and every conv is spectrally normalised (keys 0,2,5,8 .weight_orig / .weight_u / .weight_v)."""
        d = df_dims
        sn = Layers._norm(norm)
        chain = FusedChain().add_stage(0, HipConv2d(3, d, 4, 2, 1, False, spectral=sn, draw=draw), None, L.ACT_LRELU)
        for idx, (ci, co) in zip((2, 5, 8), ((d, 2 * d), (2 * d, 4 * d), (4 * d, 8 * d))):
            chain.add_stage(idx, HipConv2d(ci, co, 4, 2, 1, False, spectral=sn, draw=draw), None if sn else idx + 1, L.ACT_LRELU)
        return chain

    @staticmethod
    def ResBlock(channel_num: int) -> ResBlock:
        return ResBlock(channel_num)
