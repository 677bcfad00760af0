"""Pseudo-captions and class ids from image clusters (reference data/bedrooms.py:28-361): the step between a folder of images and the
shards data/batches.py reads.

The reference's training data has no human captions.  It embeds every image with a CNN, clusters the embeddings once per k of a ladder
of k values, appends the token `k{k}c{c}` of each clustering to the image's caption (coarse to fine) and takes the finest clustering as
the class id that the DAMSM losses mask same-class pairs with.  This module keeps that surface:

    SingleImage, Vocab, Dataset, HierarchicalClusterer, CaptionHandler          (the reference's names and methods)
    kmeans, determine_k_values, load_image_folder                               (what they stand on here)

What differs, and why:
  * clustering is Lloyd's k-means on the library's kernels (backend.functional.kmeans_assign / kmeans_update; float64 torch on a CPU
    tensor) instead of scikit-learn's KMeans.  `method="kmeans"` is the only method: the reference's UMAP reduction and its
    agglomerative linkages need packages this project does not depend on (and its default `method='agglomerative'` matches none of
    its own branches), so any other name raises ValueError.  Seeding is k distinct random rows, not k-means++.
  * class ids are the finest clustering's cluster index.  The reference numbers the finest labels through a `set`, whose order depends
    on string hashing; only EQUALITY of class ids is ever used (losses/words_loss.py, sentence_loss.py), so the partition is the same.
  * CaptionHandler.get_captions ranks candidate keys with difflib.SequenceMatcher(...).ratio() instead of rapidfuzz's ratio: the same
    rule (the best-matching key among those that contain the name), a different similarity measure on near-ties.
  * images are kept as uint8 [3, 256, 256] (what a shard stores); the 64 and 128 pixel images are the loaders' derived planes
    (data/batches.py: downsample_reference) rather than two more PIL resizes.
"""
from __future__ import annotations

import difflib
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import batches

METHODS = ("kmeans",)


# ----------------------------------------------------------------------------------------------------------------------------------
# k-means
# ----------------------------------------------------------------------------------------------------------------------------------
def kmeans(X, k: int, *, n_init: int = 3, max_iter: int = 100, seed: int = 0, init: Union[str, np.ndarray, Tensor] = "random",
           history: Optional[list] = None) -> Tuple[np.ndarray, np.ndarray, float, int]:
    """Lloyd's k-means -> (labels int32 [N], centroids float32 [k, D], inertia, n_iter) of the best restart, as numpy arrays.

    X: [N, D] array or tensor.  A device tensor is clustered on the library's kernels where it lives, anything else on the CPU path of
    backend.functional (float64 arithmetic, the same rules).  An iteration assigns every row to its nearest centroid (lowest index on a
    tie) and moves every centroid to the mean of its rows (a centroid without rows stays).  A restart ends when no label changed --
    the host reads that 4-byte count once per iteration -- or after max_iter assignments; its labels, centroids and inertia (sum of
    squared distances) are those of its last assignment.  The restart with the lowest inertia wins, the earliest on a tie.

    init="random": each restart starts from k distinct rows drawn by numpy.random.default_rng(seed) (one generator for all restarts).
    An explicit [k, D] array is used as given, once (n_init restarts from one start would be the same run).
    history: a list that receives (restart, iteration, inertia, n_changed) per iteration (costs one more 8-byte read each).

    Raises ValueError for non-finite X (one check per call), k > N or k < 1.  Out of scope: k-means++ seeding, UMAP reduction and the
    agglomerative methods of the reference (see the module header)."""
    from ..backend import functional as F
    x = X if isinstance(X, Tensor) else torch.from_numpy(np.ascontiguousarray(X))
    if x.dim() != 2:
        raise ValueError(f"kmeans: X must be [N, D], got {tuple(x.shape)}")
    x = x.to(torch.float32).contiguous()
    N, D = x.shape
    k = int(k)
    if k < 1 or k > N:
        raise ValueError(f"kmeans: k = {k} for {N} rows (need 1 <= k <= N)")
    if not bool(torch.isfinite(x).all()):
        raise ValueError("kmeans: X holds non-finite values")
    if isinstance(init, str):
        if init != "random":
            raise ValueError(f"kmeans: init {init!r} is not supported (\"random\" or an explicit [k, D] array; no k-means++)")
        rng = np.random.default_rng(seed)
        starts = [x[torch.from_numpy(np.sort(rng.choice(N, size=k, replace=False))).to(x.device)] for _ in range(max(1, int(n_init)))]
    else:
        c0 = init if isinstance(init, Tensor) else torch.from_numpy(np.ascontiguousarray(init))
        if tuple(c0.shape) != (k, D):
            raise ValueError(f"kmeans: init must be [{k}, {D}], got {tuple(c0.shape)}")
        starts = [c0.to(device=x.device, dtype=torch.float32)]
    best = None
    for r, cen in enumerate(starts):
        cen = cen.contiguous()
        labels, n_iter = None, 0
        while True:
            labels, _, n_changed, inertia = F.kmeans_assign(x, cen, labels)
            n_iter += 1
            changed = int(n_changed)
            if history is not None:
                history.append((r, n_iter, float(inertia), changed))
            if changed == 0 or n_iter >= max_iter:
                break
            cen, _ = F.kmeans_update(x, labels, cen)
        total = float(inertia)
        if best is None or total < best[2]:
            best = (labels.cpu().numpy(), cen.cpu().numpy(), total, n_iter)
    return best


def determine_k_values(max_vocab_size: int = 600, min_k: int = 5) -> List[int]:
    """The reference's ladder (bedrooms.py:291-304): max_vocab_size // 2, // 4, // 8 ... while above min_k, ascending.  The values sum to
    less than max_vocab_size, so the cluster tokens never outgrow the vocabulary.  (600, 5) -> [9, 18, 37, 75, 150, 300]."""
    out, factor = [], 2
    k = max_vocab_size // factor
    while k > min_k:
        out.append(k)
        factor *= 2
        k = max_vocab_size // factor
    return out[::-1]


# ----------------------------------------------------------------------------------------------------------------------------------
# images, vocabulary, dataset
# ----------------------------------------------------------------------------------------------------------------------------------
class SingleImage:
    """One image and what the clustering gives it (reference bedrooms.py:28-56).  img256 is uint8 [3, 256, 256] (or None for an entry
    that only carries a caption)."""

    def __init__(self, fpath: str, img256: Optional[np.ndarray] = None):
        self.fpath = fpath
        self.img256 = img256
        self.caption: List[str] = []
        self.class_id: Optional[int] = None      # must be assigned

    def assign_class_id(self, class_id: int) -> None:
        self.class_id = int(class_id)

    @property
    def caption_length(self) -> int:
        return len(self.caption)


class Vocab:
    """Word <-> index map (reference bedrooms.py:59-101).  Index 0 is the padding of a shard's `words`, so the words start at 1 with
    '[UNK]', which `process` substitutes for a word it has not seen (the reference looks '[UNK]' up without ever adding it)."""

    UNK = "[UNK]"

    def __init__(self):
        self.word2count: Dict[str, int] = {}
        self.index2word: Dict[int, str] = {}
        self.word2index: Dict[str, int] = {}
        self.n_words = 1                         # index 0: padding
        self.vocab_built = False
        self._addWord(self.UNK)
        self.word2count[self.UNK] = 0

    def process(self, tokens: Sequence[str]) -> List[int]:
        """words -> indices; an unknown word becomes '[UNK]'"""
        unk = self.word2index[self.UNK]
        return [self.word2index.get(w, unk) for w in tokens]

    def words(self, indices: Sequence[int]) -> List[str]:
        return [self.index2word[int(i)] for i in indices]

    def buildVocab(self, dataset: "Dataset") -> None:
        for image in dataset.images:
            self._addCaption(image.caption)
        self.vocab_built = True

    def buildVocabFromMapping(self, mapping: dict) -> None:
        for caption, _ in mapping.values():
            self._addCaption(caption)
        self.vocab_built = True

    def _addCaption(self, caption: Sequence[str]) -> None:
        for word in caption:
            self._addWord(word)

    def _addWord(self, word: str) -> None:
        if word not in self.word2index:
            self.word2index[word] = self.n_words
            self.word2count[word] = 1
            self.index2word[self.n_words] = word
            self.n_words += 1
        else:
            self.word2count[word] += 1


def load_image_folder(rootdir: str, max_images: int = 100) -> List[SingleImage]:
    """Every .jpg under rootdir (sorted walk) as two SingleImages, the picture resized to 256 x 256 RGB uint8 and its mirrored twin under
    the path + '_r', as the reference's Dataset.make_data / makeImage do (bedrooms.py:118-164; PIL's default bilinear resize, which
    is what torchvision's Resize calls).  Stops once more than min(max_images, 2 * files) entries exist, like the reference."""
    from PIL import Image
    paths = []
    for d, dirs, files in os.walk(rootdir):
        dirs.sort()
        paths += [os.path.join(d, f) for f in sorted(files) if f.lower().endswith(".jpg")]
    limit = min(max_images, 2 * len(paths))
    out: List[SingleImage] = []
    for p in paths:
        with Image.open(p) as im:
            a = np.asarray(im.convert("RGB").resize((256, 256), Image.BILINEAR), dtype=np.uint8).transpose(2, 0, 1)
        out += [SingleImage(p, np.ascontiguousarray(a)), SingleImage(p + "_r", np.ascontiguousarray(a[:, :, ::-1]))]
        if len(out) > limit:
            break
    return out


class Dataset:
    """The images of a run with their captions, class ids and vocabulary (reference bedrooms.py:104-238).  Built from a folder
    (rootdir) or from SingleImages made elsewhere (images)."""

    def __init__(self, rootdir: Optional[str] = None, max_images: int = 100, images: Optional[Sequence[SingleImage]] = None):
        if (rootdir is None) == (images is None):
            raise ValueError("Dataset: give rootdir or images")
        self.rootdir = rootdir
        self.images: List[SingleImage] = list(images) if images is not None else load_image_folder(rootdir, max_images)
        self.paths_to_images = {img.fpath: img for img in self.images}
        self.vocab = Vocab()

    @property
    def max_seqlen(self) -> int:
        return max(len(img.caption) for img in self.images)

    def save_captions_and_class_ids(self, path: str) -> None:
        """the reference's JSON shape: {path: [caption, class_id]}"""
        with open(path, "w") as f:
            json.dump({img.fpath: [img.caption, img.class_id] for img in self.images}, f)

    def load_captions_and_class_ids(self, path: str) -> None:
        with open(path) as f:
            mapping = json.load(f)
        for fpath, (caption, class_id) in mapping.items():
            img = self.paths_to_images[fpath]
            img.caption, img.class_id = list(caption), class_id

    def write_shards(self, directory: str, shard_size: int = 4096) -> List[str]:
        """Writes the dataset as 256-only shards (batches.write_shard) of at most shard_size images, in image order; builds the vocabulary
        first if that has not happened.  -> the shard paths, ready for batches.ShardBatches / DeviceShardBatches."""
        if shard_size < 1:
            raise ValueError(f"write_shards: shard_size {shard_size}")
        for img in self.images:
            if img.img256 is None or img.class_id is None or not img.caption:
                raise ValueError(f"write_shards: {img.fpath} has no image, caption or class id (run HierarchicalClusterer.cluster first)")
        if not self.vocab.vocab_built:
            self.vocab.buildVocab(self)
        os.makedirs(directory, exist_ok=True)
        T = self.max_seqlen
        paths = []
        for s in range(0, len(self.images), shard_size):
            part = self.images[s:s + shard_size]
            words = np.zeros((len(part), T), dtype=np.int64)
            for i, img in enumerate(part):
                words[i, :len(img.caption)] = self.vocab.process(img.caption)
            path = os.path.join(directory, f"shard_{len(paths):05d}.npz")
            batches.write_shard(path, words, np.array([len(img.caption) for img in part]), np.array([img.class_id for img in part]),
                                img256=np.stack([img.img256 for img in part]))
            paths.append(path)
        return paths


# ----------------------------------------------------------------------------------------------------------------------------------
# clustering into captions
# ----------------------------------------------------------------------------------------------------------------------------------
class HierarchicalClusterer:
    """Clusters a dataset's images once per k of the ladder and writes captions and class ids into it (reference bedrooms.py:241-304).

    embedder: any object with `embed(images [M, 3, 256, 256] float in [-1, 1], batch_size) -> [M, E]` (networks.cnn_embedder.ImageEmbedder
    is the project's).  The clustering runs on the embedder's `device` attribute if it has one, else where the embeddings are -- with
    ImageEmbedder on an MI355X that is the library's kernels."""

    def __init__(self, embedder):
        self.embedder = embedder

    def cluster(self, dataset: Dataset, max_vocab_size: int = 600, min_clusters: int = 5, batch_size: int = 32, method: str = "kmeans",
                seed: int = 0) -> None:
        """In place: appends one token `k{k}c{c}` per k of determine_k_values(max_vocab_size, min_clusters) to every image's caption,
        coarse to fine -- one independent k-means per k, the clusterings are not nested (as in the reference) -- and assigns the finest
        clustering's cluster index c as the class id.  (The reference numbers the class ids through a set of the finest labels, in
        string-hash order; only their equality is used, and that partition is the same.)"""
        if method not in METHODS:
            raise ValueError(f"cluster: method {method!r} is not supported; the supported method is \"kmeans\"")
        k_values = determine_k_values(max_vocab_size, min_clusters)
        if not k_values:
            raise ValueError(f"cluster: no k between min_clusters = {min_clusters} and max_vocab_size / 2 = {max_vocab_size // 2}")
        parts = []                               # one embed call per batch: only batch_size images exist as float32 at a time
        for s in range(0, len(dataset.images), batch_size):
            u8 = np.stack([img.img256 for img in dataset.images[s:s + batch_size]])
            e = self.embedder.embed(batches.scale_255_to_1(torch.from_numpy(u8)), batch_size=batch_size)
            parts.append(e if isinstance(e, Tensor) else torch.from_numpy(np.asarray(e)))
        X = torch.cat(parts, dim=0)
        X = X.detach().to(device=getattr(self.embedder, "device", None) or X.device, dtype=torch.float32)
        labels = None
        for k in k_values:
            labels, _, _, _ = kmeans(X, k, seed=seed)
            for img, c in zip(dataset.images, labels.tolist()):
                img.caption.append(f"k{k}c{c}")
        for img, c in zip(dataset.images, labels.tolist()):
            img.assign_class_id(c)


class CaptionHandler:
    """Captions by image name from a saved captions file, for generation (reference bedrooms.py:307-361)."""

    def __init__(self, vocab_path: str):
        self.vocab_path = vocab_path
        self.vocab = Vocab()
        self.img2caption: Dict[str, List[str]] = {}
        with open(vocab_path) as f:
            mapping = json.load(f)
        self.vocab.buildVocabFromMapping(mapping)
        for path, (caption, _) in mapping.items():
            self.img2caption[path] = caption

    @property
    def vocab_size(self) -> int:
        return self.vocab.n_words

    def get_captions(self, imgnames: Sequence[str]) -> List[List[str]]:
        return [self._get_caption(name) for name in imgnames]

    def swap_captions(self, captions: Sequence[List[str]], num: int = 1, reverse: bool = False) -> List[List[str]]:
        """Swaps `num` tokens between two captions: the most global (first) ones, or with reverse the most local (last) ones."""
        assert len(captions) == 2
        c1, c2 = captions
        new1, new2 = c1[:], c2[:]
        for i in range(1, num + 1):
            i = -i if reverse else i - 1
            new1[i], new2[i] = c2[i], c1[i]
        return [new1, new2]

    def preprocess(self, captions: Sequence[Sequence[str]]) -> Tuple[Tensor, Tensor]:
        """captions -> (indices int64 [B, T], lengths int64 [B]); the captions of one call have one length, as the clusterer makes them"""
        indices = [self.vocab.process(c) for c in captions]
        return torch.tensor(indices, dtype=torch.int64), torch.tensor([len(i) for i in indices], dtype=torch.int64)

    def _get_caption(self, imgname: str) -> List[str]:
        """the caption of the key that contains imgname and resembles it most (difflib's ratio; the reference uses rapidfuzz's)"""
        best, best_ratio = None, 0.0
        for path in self.img2caption:
            if imgname in path:
                r = difflib.SequenceMatcher(None, imgname, path).ratio()
                if r > best_ratio:
                    best, best_ratio = path, r
        if best is None:
            raise KeyError(f"no caption key contains {imgname!r}")
        return self.img2caption[best]
