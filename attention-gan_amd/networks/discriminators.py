"""Sigmoid discriminators with the reference's interface (networks/discriminators.py:10-70): unconditional as the reference's, and
with `cond_dim` AttnGAN's joint sentence-image head (COND_DNET) next to the unconditional one.  norm="spectral" (not in the reference;
SNGAN's, SAGAN's and XMC-GAN's discriminator mode): every weight is spectrally normalised and there is no BatchNorm anywhere."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from ..backend import functional as HF
from ..backend import lib as L
from ..utilities.layers import HipBatchNorm2d, HipConv2d, HipLinear, Layers, SpectralState, draw_spectral_state_


class _SpectralHolder(SpectralState, nn.Conv2d):
    """parameter holder of a spectrally normalised logit head: nn.Conv2d's init, then weight -> weight_orig, weight_u, weight_v"""

    def __init__(self, cin: int):
        super().__init__(cin, 1, kernel_size=4, stride=4)
        self._init_spectral(draw=False)


class _LogitHead(nn.Module):
    """Conv2d(8df, 1, k=4, s=4) + Sigmoid on the 4x4 code: a dot product per image (keys '0.weight', '0.bias').  `spectral`: the
    1 x (8df * 16) weight is divided by its spectral norm, which for one row is its Euclidean norm; the bias is untouched (keys
    '0.weight_orig', '0.weight_u', '0.weight_v', '0.bias'; u and v are drawn by the owning discriminator)."""

    def __init__(self, cin: int, spectral: bool = False):
        super().__init__()
        self.add_module("0", _SpectralHolder(cin) if spectral else nn.Conv2d(cin, 1, kernel_size=4, stride=4))   # parameter holder only
        self._sn = spectral
        self._packed = {}

    def forward(self, x: Tensor) -> Tensor:
        conv = getattr(self, "0")
        b, c, h, w = x.shape
        if (h, w) != (4, 4):
            raise ValueError(f"discriminator head expects a 4x4 code, got {h}x{w}")
        if self._sn:
            logit = HF.linear(x.reshape(b, c * 16), conv.weight_sn().view(1, c * 16), conv.bias, None, None, HF.grad_dst(conv.bias))
        else:
            logit = HF.linear(x.reshape(b, c * 16), conv.weight.view(1, c * 16), conv.bias, self._packed,
                              HF.grad_dst(conv.weight), HF.grad_dst(conv.bias))
        return HF.activation(logit, L.ACT_SIGMOID)


class _Held:
    """mixin of a parameter holder whose owner writes and reads its state_dict entry (_JointConv): no entry of its own"""

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        pass

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        pass


class _HeldConv2d(_Held, HipConv2d):
    pass


class _HeldLinear(_Held, HipLinear):
    pass


class _JointConv(nn.Module):
    """AttnGAN's jointConv = Block3x3_leakRelu(8df + nef, 8df) on cat(h, rep(s)), stored split: the sentence channels are constant over
    the 4x4 map, so conv3x3(cat(h, rep(s)), W) = conv3x3(h, W[:, :8df]) + the border-aware tap sums of P = s . W[:, 8df:]
    (backend/functional.py: cond_join).  `image` holds W[:, :8df]; `sentence` holds W[:, 8df:] arranged [c][t][e], so that
    sentence(s).view(B, 8df, 9) is P.  Both are ordinary parameters (flat optimiser, packed weight forms).  state_dict shows
    AttnGAN's keys: '0.weight' [8df, 8df + nef, 3, 3] -- the concatenation, assembled on save and split on load -- and '1.*', the
    BatchNorm.  `spectral`: no BatchNorm; the two parts are divided by the ONE spectral norm of the joint weight (buffers weight_u,
    weight_v) and the keys are '0.weight_orig', '0.weight_u', '0.weight_v' in AttnGAN's column order."""

    def __init__(self, c: int, nef: int, spectral: bool = False):
        super().__init__()
        self.c, self.nef, self.spectral = c, nef, spectral
        self.image = _HeldConv2d(c, c, 3, 1, 1, False)
        self.sentence = _HeldLinear(nef, 9 * c, bias=False)
        if spectral:
            # ONE sigma and ONE u over [image | sentence]: `sentence` viewed [c, 9 nef] is a column permutation of AttnGAN's sentence
            # block, and singular values and u do not depend on column order -- this is the spectral norm of AttnGAN's joint layer.
            # weight_v is kept in the stored column order and permuted on save and load, as the weight is.  No BatchNorm.
            self.register_buffer("weight_u", torch.zeros(c))
            self.register_buffer("weight_v", torch.zeros(9 * c + 9 * nef))
        else:
            self.add_module("1", HipBatchNorm2d(c))
        # ONE default init of the joint conv (the fan-in of AttnGAN's layer: (8df + nef) * 9), then split; the two holders' own draws above
        # are overwritten.  (COND_DNET is built after every other child, so the draws shift nothing that existed before.)
        joint = nn.Conv2d(c + nef, c, kernel_size=3, stride=1, padding=1, bias=False)
        self._split_(joint.weight.detach())

    @torch.no_grad()
    def _split_(self, w: Tensor) -> None:
        c, nef = self.c, self.nef
        self.image.weight.copy_(w[:, :c])
        self.sentence.weight.copy_(w[:, c:].reshape(c, nef, 9).permute(0, 2, 1).reshape(9 * c, nef))

    @torch.no_grad()
    def draw_spectral_state_(self) -> None:
        for b in (self.weight_u, self.weight_v):
            b.copy_(nn.functional.normalize(b.normal_(0, 1), dim=0, eps=1e-12))

    def _v_to_attngan(self, v: Tensor) -> Tensor:
        """v from the stored column order [image | (t, e)] to AttnGAN's [image | (e, t)]"""
        n = 9 * self.c
        return torch.cat([v[:n], v[n:].view(9, self.nef).t().reshape(-1)])

    def _v_from_attngan(self, v: Tensor) -> Tensor:
        n = 9 * self.c
        return torch.cat([v[:n], v[n:].view(self.nef, 9).t().reshape(-1)])

    def weights_sn(self):
        """(image weight, sentence weight) of this forward, both divided by the joint weight's one sigma"""
        return HF.spectral_weight(self.image.weight, self.weight_u, self.weight_v, self.training, second=self.sentence.weight)

    def joint_weight(self) -> Tensor:
        """W [8df, 8df + nef, 3, 3] of AttnGAN's layout from the two stored parts (differentiable: the test oracles use it)"""
        c, nef = self.c, self.nef
        ws = self.sentence.weight.view(c, 9, nef).permute(0, 2, 1).reshape(c, nef, 3, 3)
        return torch.cat([self.image.weight, ws], dim=1)

    # the two stored parts appear as the single concatenated key (they write and read no entries of their own: _Held); the BatchNorm
    # child keeps its entries
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        w = self.joint_weight()
        destination[prefix + ("0.weight_orig" if self.spectral else "0.weight")] = w if keep_vars else w.detach()
        if self.spectral:
            destination[prefix + "0.weight_u"] = self.weight_u.clone()
            destination[prefix + "0.weight_v"] = self._v_to_attngan(self.weight_v)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        key = prefix + "0.weight"
        if self.spectral:
            # a checkpoint with `0.weight` and no `0.weight_orig` is a warm start: the weight loads, u and v stay as they are
            if prefix + "0.weight_orig" in state_dict or key not in state_dict:
                key = prefix + "0.weight_orig"
                for name, n, put in (("weight_u", self.c, lambda t: t), ("weight_v", 9 * (self.c + self.nef), self._v_from_attngan)):
                    k = prefix + "0." + name
                    if k not in state_dict:
                        if strict:
                            missing_keys.append(k)
                    elif tuple(state_dict[k].shape) != (n,):
                        error_msgs.append(f"size mismatch for {k}: copying a param with shape {tuple(state_dict[k].shape)} from checkpoint, "
                                          f"the shape in current model is {(n,)}.")
                    else:
                        with torch.no_grad():
                            getattr(self, name).copy_(put(state_dict[k].to(getattr(self, name).dtype)))
        if key not in state_dict:
            if strict:
                missing_keys.append(key)
            return
        w = state_dict[key]
        want = (self.c, self.c + self.nef, 3, 3)
        if tuple(w.shape) != want:
            error_msgs.append(f"size mismatch for {key}: copying a param with shape {tuple(w.shape)} from checkpoint, the shape in "
                              f"current model is {want}.")
            return
        self._split_(w.to(self.image.weight.dtype))


class _CondDNet(nn.Module):
    """AttnGAN's D_GET_LOGITS(bcondition=True): jointConv on the code and the sentence, then the logit head (keys jointConv.{0,1}.*,
    outlogits.0.*)."""

    def __init__(self, c: int, nef: int, spectral: bool = False):
        super().__init__()
        self.jointConv = _JointConv(c, nef, spectral)
        self.outlogits = _LogitHead(c, spectral)


class _Disc(nn.Module):
    # every BatchNorm inside is a HipBatchNorm2d and nothing else couples samples of a batch, so a [real; fake] batch may go
    # through in one pass under functional.bn_groups(2) (losses/disc_loss.py)
    # (norm="spectral" has no BatchNorm at all: still nothing couples the samples)
    supports_batch_groups = True
    norm = "batch"

    def _set_norm(self, norm: str) -> dict:
        """called FIRST by the constructors: checks `norm` and returns the keywords the Layers factories take for it"""
        self.norm = norm
        return dict(norm=norm, draw=False) if Layers._norm(norm) else {}

    def _add_cond(self, df_dim: int, cond_dim: Optional[int]) -> None:
        """called LAST by the constructors: the existing children keep their initial values under a given seed.  Under
        norm="spectral" the draws of every u and v follow, after COND_DNET's: a seed gives the weights it gives norm="batch"."""
        self.cond_dim = cond_dim
        if cond_dim is None:
            self.COND_DNET = None          # (a plain attribute: no module, no state_dict key, no random draw)
        elif int(cond_dim) < 1:
            raise ValueError(f"cond_dim must be a positive sentence-embedding width or None, got {cond_dim}")
        else:
            self.COND_DNET = _CondDNet(df_dim * 8, int(cond_dim), self.norm == "spectral")
        if self.norm == "spectral":
            draw_spectral_state_(self)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """norm="spectral" warm-starts from a norm="batch" checkpoint: the entries of its BatchNorms (every module that has a
        `running_mean`) are ignored, a `weight` loads as `weight_orig`, u and v stay as they are"""
        if self.norm == "spectral":
            bn = {k.rsplit(".", 1)[0] for k in state_dict if k.endswith(".running_mean")}
            state_dict = {k: v for k, v in state_dict.items() if k.rsplit(".", 1)[0] not in bn}
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _tail(self, x: Tensor) -> Tensor:
        return self.outlogits(x).view(-1)

    def forward(self, X: Tensor) -> Tensor:
        return self._tail(self.features(X))

    def uncond(self, h: Tensor) -> Tensor:
        """the unconditional scores from a 4x4 code (forward(X) = uncond(features(X)))"""
        return self._tail(h)

    def cond(self, h: Tensor, sent: Tensor, wrong: bool = False) -> Tensor:
        """The conditional scores [(k + wrong) * B] from a code h [k * B, 8df, 4, 4] -- k consecutive groups of B rows, row n showing
        caption n mod B -- and the sentence embeddings sent [B, nef]: AttnGAN's COND_DNET(h, c_code).  With `wrong`, B more scores pair
        the FIRST group's codes (the real images' in a discriminator update) with the next sample's caption, cyclically: AttnGAN's
        mismatched pairs, here B of them (AttnGAN has B - 1 and drops the last) so that the groups are equal, which bn_groups takes.

        Image conv once over all k * B rows, linear once over the B captions, cond_join, then jointConv.1 as fused BatchNorm +
        LeakyReLU under bn_groups(k + wrong): in train mode the BatchNorm behaves as k + wrong consecutive calls in the order of the
        groups (real, fake, wrong), each with its own statistics and its own running-statistic update."""
        net = self.COND_DNET
        if net is None:
            raise ValueError(f"{type(self).__name__} was built without cond_dim: it has no COND_DNET")
        jc = net.jointConv
        if sent.dim() != 2 or sent.shape[1] != jc.nef:
            raise ValueError(f"cond: sentence embeddings must be [B, {jc.nef}], got {tuple(sent.shape)}")
        B = sent.shape[0]
        if h.dim() != 4 or tuple(h.shape[1:]) != (jc.c, 4, 4) or h.shape[0] < B or h.shape[0] % B:
            raise ValueError(f"cond: the code must be [k * {B}, {jc.c}, 4, 4], got {tuple(h.shape)}")
        if wrong and B < 2:
            raise ValueError("cond: the mismatched pairs (wrong=True) need at least 2 captions")
        k = h.shape[0] // B
        if jc.spectral:
            wi, ws = jc.weights_sn()
            y = HF.cond_join(HF.conv2d(h, wi, None, "same"), HF.linear(sent, ws).view(B, jc.c, 9), wrong)
            return net.outlogits(HF.activation(y, L.ACT_LRELU)).view(-1)
        y = HF.cond_join(jc.image(h), jc.sentence(sent).view(B, jc.c, 9), wrong)
        with HF.bn_groups(k + int(bool(wrong))):
            y = getattr(jc, "1").fused(y, L.ACT_LRELU)
        return net.outlogits(y).view(-1)


class Disc64(_Disc):
    def __init__(self, df_dim: int, cond_dim: Optional[int] = None, norm: str = "batch"):
        super().__init__()
        kw = self._set_norm(norm)
        self.img_code_s16 = Layers.encode_image_by_16times(df_dim, **kw)
        self.outlogits = _LogitHead(df_dim * 8, bool(kw))
        self._add_cond(df_dim, cond_dim)

    def features(self, X: Tensor) -> Tensor:
        return self.img_code_s16(X)


class Disc128(_Disc):
    def __init__(self, df_dim: int, cond_dim: Optional[int] = None, norm: str = "batch"):
        super().__init__()
        kw = self._set_norm(norm)
        self.img_code_s16 = Layers.encode_image_by_16times(df_dim, **kw)
        self.img_code_s32 = Layers.downBlock(df_dim * 8, df_dim * 16, **kw)
        self.img_code_s32_1 = Layers.Block3x3_leakRelu(df_dim * 16, df_dim * 8, **kw)
        self.outlogits = _LogitHead(df_dim * 8, bool(kw))
        self._add_cond(df_dim, cond_dim)

    def features(self, X: Tensor) -> Tensor:
        return self.img_code_s32_1(self.img_code_s32(self.img_code_s16(X)))


class Disc256(_Disc):
    def __init__(self, df_dim: int, cond_dim: Optional[int] = None, norm: str = "batch"):
        super().__init__()
        kw = self._set_norm(norm)
        self.img_code_s16 = Layers.encode_image_by_16times(df_dim, **kw)
        self.img_code_s32 = Layers.downBlock(df_dim * 8, df_dim * 16, **kw)
        self.img_code_s64 = Layers.downBlock(df_dim * 16, df_dim * 32, **kw)
        self.img_code_s64_1 = Layers.Block3x3_leakRelu(df_dim * 32, df_dim * 16, **kw)
        self.img_code_s64_2 = Layers.Block3x3_leakRelu(df_dim * 16, df_dim * 8, **kw)
        self.outlogits = _LogitHead(df_dim * 8, bool(kw))
        self._add_cond(df_dim, cond_dim)

    def features(self, X: Tensor) -> Tensor:
        x = self.img_code_s64(self.img_code_s32(self.img_code_s16(X)))
        return self.img_code_s64_2(self.img_code_s64_1(x))


class WordLevelDisc(nn.Module):
    """ControlGAN's word-level discriminator (Li et al., NeurIPS 2019, section 3.2; not in the reference): how well every WORD of a
    caption is shown by the regions of an image, pooled into one probability per (image, caption) pair.

    regions [B, nef, h, w] are the frozen image encoder's region features, words [B, nef, T] the frozen text encoder's word
    embeddings, lens [B] the caption lengths.  `perception` (the paper's F', a bias-free 1x1 conv on the image side, the module's only
    parameter: key `perception.weight`) starts as the IDENTITY, so that at step 0 the score is the pretrained encoders' own
    word-region correlation and not noise.  Then backend.functional.word_corr (include/agan.h states the formulas): func_attention of
    the words over the perceived regions, the cosine r_l of every word with its context, the word self-attention weight g_l, and
    p = sum_l g_l sigmoid(gamma2 r_l) in (0, 1).  Image b is scored against caption (b + shift) mod B: shift 0 the matching pairs,
    shift 1 the cyclic mismatched ones.  One departure from the paper, whose self-attention weight multiplies the context before the
    (scale-invariant) cosine and so cancels: here it weights the word's term of the pooled score.

    The gradient reaches the regions and `perception.weight`; the words are constants (ValueError if they require grad).  CUDA
    tensors run the HIP kernels (h * w <= 320, nef <= 320, T <= 32, B <= 128); CPU tensors run word_corr_reference on stock ops."""

    def __init__(self, nef: int, gamma1: float = 4.0, gamma2: float = 5.0):
        super().__init__()
        if isinstance(nef, bool) or not isinstance(nef, int) or nef < 1:
            raise ValueError(f"nef={nef!r}: the embedding width, a positive integer")
        self.nef, self.gamma1, self.gamma2 = nef, float(gamma1), float(gamma2)
        self.perception = Layers.conv1x1(nef, nef)
        with torch.no_grad():
            self.perception.weight.copy_(torch.eye(nef).view(nef, nef, 1, 1))

    def perceive(self, regions: Tensor) -> Tensor:
        """F'(regions): [k, nef, h, w] -> [k, nef, h, w]"""
        if regions.dim() != 4 or regions.shape[1] != self.nef:
            raise ValueError(f"WordLevelDisc: regions must be [B, {self.nef}, h, w], got {tuple(regions.shape)}")
        if regions.is_cuda:
            return self.perception(regions)
        return torch.nn.functional.conv2d(regions, self.perception.weight)

    def score(self, perceived: Tensor, words: Tensor, lens, shift: int = 0):
        """(p, r, g) from regions that went through `perceive` already (the discriminator loss scores the real batch twice)"""
        fn = HF.word_corr if perceived.is_cuda else HF.word_corr_reference
        return fn(perceived, words, lens, shift, self.gamma1, self.gamma2)

    def correlations(self, regions: Tensor, words: Tensor, lens, shift: int = 0):
        """-> (p [B], r [B, T], g [B, T]): the score, the per-word cosines and the word weights (0 beyond a caption's length)"""
        return self.score(self.perceive(regions), words, lens, shift)

    def forward(self, regions: Tensor, words: Tensor, lens, shift: int = 0) -> Tensor:
        return self.correlations(regions, words, lens, shift)[0]
