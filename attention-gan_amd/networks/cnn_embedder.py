"""Image embedder of the caption preprocessing (reference networks/cnn_embedder.py:14-38).

The reference embeds every image with a torchvision ResNet-18 whose weights it downloads at construction, and clusters the pooled
512-vectors into pseudo-captions (data/bedrooms.py:255-256).  Nothing is downloaded here and there is no ResNet: `ImageEmbedder` keeps
the reference's contract

    embed(images [M, 3, H, W] float, batch_size) -> [M, E] on the CPU

over the project's own Inception-v3 trunk (networks.cnn_encoder.CNNEncoder): frozen, in eval mode, on the library's kernels
(backend="hip") when it lives on an MI355X.  The embedding is the trunk's pooled 2048-vector (CNNEncoder.pooled), not the output of the
randomly initialised `emb_cnn_code` head.  Weights come through CNNEncoder.load_trunk_state_dict from a file the user supplies; with
the random initialisation the embedding is a fixed random feature map, which still clusters, only less meaningfully.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor, nn

from .cnn_encoder import CNNEncoder


class ImageEmbedder(nn.Module):
    EMBED_DIM = 2048

    def __init__(self, device="cpu", backend: Optional[str] = None, trunk_state: Optional[Dict[str, Tensor]] = None):
        """backend: "hip" or "torch"; None = "hip" on a GPU device, "torch" on the CPU (the library has no CPU path, and asking for
        "hip" on the CPU raises when embed() runs).  trunk_state: a torchvision inception_v3 state_dict (load_trunk_state_dict)."""
        super().__init__()
        device = torch.device(device)
        self.model = CNNEncoder(backend=backend or ("hip" if device.type == "cuda" else "torch"))
        if trunk_state is not None:
            self.model.load_trunk_state_dict(trunk_state)
        self.freeze_model()
        self.to(device)

    @property
    def device(self) -> torch.device:
        return self.model.emb_cnn_code.weight.device

    def freeze_model(self) -> None:
        self.model.freeze_all_weights()
        self.model.eval()

    def train(self, mode: bool = True):
        return super().train(False)              # an embedder is never in train mode (batch statistics would depend on the batch)

    def embed(self, images: Tensor, batch_size: int = 32) -> Tensor:
        """images [M, 3, H, W] float in [-1, 1], on any device -> [M, 2048] on the CPU, batch_size images at a time, in order"""
        out = []
        with torch.no_grad():
            for s in range(0, images.shape[0], batch_size):
                batch = images[s:s + batch_size].to(self.device, dtype=torch.float32)
                out.append(self.model.pooled(batch).detach().cpu())
        return torch.cat(out, dim=0)
