"""Caption encoder with the reference's interface (networks/rnn_encoder.py:12-96).

Embedding -> dropout -> bidirectional LSTM.  Constructor arguments, `forward(captions, caption_lengths) -> (word_embs
[B,nhidden,T_max], sent_embs [B,nhidden])`, parameter names (`embedding.weight`, `rnn.weight_ih_l0`, ...) and the uniform(-0.1, 0.1)
embedding init follow the reference.  Two backends compute the same contract on the same parameters (the state_dict keys are the same):

* `backend="torch"` (default): stock PyTorch-ROCm -- nn.Embedding, the dropout module, pack_padded_sequence(enforce_sorted=False),
  MIOpen's nn.LSTM, pad_packed_sequence.
* `backend="hip"`: the library's kernels in train and eval mode, fp32 in every precision mode (backend/functional.py: embedding,
  linear, lstm; include/agan.h: agan_embedding_*, agan_lstm_*).  The embedding gather reads the first T_max = max(lengths) columns of
  the captions; `self.dropout` (torch's module and RNG) acts on the gathered embeddings; the input projection of each direction runs
  on the linear-layer engine; one launch runs the recurrence of both directions with per-row lengths read from device memory.  The
  backward is run-to-run identical (fixed summation order, no atomics).  It takes nlayers == 1 and a per-direction hidden size that
  is a multiple of 16 up to 128; the setter refuses anything else.  word_embs is a transposed view of a [B, T_max, nhidden] tensor as
  on the stock path, 0 at t >= length.  Under no_grad, or with every parameter frozen, nothing is kept for a backward.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor, nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence


class RNNEncoder(nn.Module):
    BACKENDS = ("torch", "hip")

    def __init__(self, vocabsize: int, embdim=300, dropprob=0.5, nhidden=128, nlayers=1, bidirectional=True, backend: str = "torch"):
        super().__init__()
        self.vocabsize, self.embdim, self.dropprob, self.nlayers = vocabsize, embdim, dropprob, nlayers
        self.bidirectional = bidirectional
        self.ndirections = 2 if bidirectional else 1
        self.nhidden = nhidden // self.ndirections
        self.embedding = nn.Embedding(vocabsize, embdim)
        self.dropout = nn.Dropout(dropprob)
        self.rnn = nn.LSTM(input_size=embdim, hidden_size=self.nhidden, num_layers=nlayers, batch_first=True,
                           dropout=dropprob if nlayers > 1 else 0.0, bidirectional=bidirectional)
        self.embedding.weight.data.uniform_(-0.1, 0.1)
        self.backend = backend

    @property
    def backend(self) -> str:
        return self._backend

    @backend.setter
    def backend(self, value: str) -> None:
        if value not in self.BACKENDS:
            raise ValueError(f"RNNEncoder backend must be one of {self.BACKENDS}, got {value!r}")
        if value == "hip":
            if self.nlayers != 1:
                raise ValueError(f"RNNEncoder backend 'hip' runs one LSTM layer, got nlayers={self.nlayers}")
            if self.nhidden % 16 or not 16 <= self.nhidden <= 128:
                raise ValueError(f"RNNEncoder backend 'hip' needs a per-direction hidden size that is a multiple of 16 in 16..128, "
                                 f"got {self.nhidden}")
        self._backend = value

    def init_hidden_cell_states(self, batch_size: int) -> Tuple[Tensor, Tensor]:
        w = next(self.parameters())
        shape = (self.nlayers * self.ndirections, batch_size, self.nhidden)
        return w.new_zeros(shape), w.new_zeros(shape)

    def freeze_all_weights(self):
        for p in self.parameters():
            p.requires_grad = False

    def forward(self, captions: Tensor, caption_lengths) -> Tuple[Tensor, Tensor]:
        lens = [int(v) for v in (caption_lengths.tolist() if hasattr(caption_lengths, "tolist") else caption_lengths)]
        if self._backend == "hip":
            return self._forward_hip(captions, lens)
        x = self.dropout(self.embedding(captions))
        packed = pack_padded_sequence(x, lengths=lens, batch_first=True, enforce_sorted=False)
        out, (hidden, _cell) = self.rnn(packed, self.init_hidden_cell_states(len(lens)))
        out = pad_packed_sequence(out, batch_first=True)[0]                    # [B, T_max, nhidden]
        word_embs = out.transpose(1, 2)                                        # [B, nhidden, T_max]
        sent_embs = hidden.transpose(0, 1).contiguous().view(-1, self.ndirections * self.nhidden)
        return word_embs, sent_embs

    def _forward_hip(self, captions: Tensor, lens) -> Tuple[Tensor, Tensor]:
        from ..backend import functional as AF
        B, Tc = captions.shape
        if len(lens) != B or any(not 1 <= n <= Tc for n in lens):
            raise ValueError(f"caption lengths must be {B} values in 1..{Tc}, got {lens}")
        T = max(lens)
        dev = captions.device
        lens_dev = torch.tensor(lens, dtype=torch.int32).to(dev)
        x = self.dropout(AF.embedding(captions, self.embedding.weight, T))                 # [B, T, E]
        x = x.reshape(B * T, self.embdim)
        sfx = ["", "_reverse"][:self.ndirections]
        caches = self.__dict__.setdefault("_agan_ih_cache", tuple({} for _ in sfx))
        r = self.rnn
        xg = [AF.linear(x, getattr(r, "weight_ih_l0" + s), getattr(r, "bias_ih_l0" + s), caches[d]).view(B, T, 4 * self.nhidden)
              for d, s in enumerate(sfx)]
        whh = [getattr(r, "weight_hh_l0" + s) for s in sfx]
        bhh = [getattr(r, "bias_hh_l0" + s) for s in sfx]
        save = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        out, sent_embs = AF.lstm(xg, whh, bhh, lens_dev, save)                            # [B, T, nhidden], [B, nhidden]
        return out.transpose(1, 2), sent_embs
