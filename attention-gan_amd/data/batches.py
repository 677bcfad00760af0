"""Batch wire format of the training loop (reference data/bedrooms.py:209-238).

The reference's DataLoader yields the tuple  (words [B,T] int64, lengths [B] int64, class_ids [B] int64,
img64, img128, img256 float32 in [-1,1])  -- train.py:111.  This module is the tuple itself, produced either synthetically (benchmarks,
tests) or from pre-resized uint8 shards on disk.  What lies upstream of it -- image folders, k-means pseudo-captions and class ids,
vocabulary building -- is data/captions.py, whose Dataset.write_shards writes the shards read here.

Shard format (.npz, data only): `words` int64 [N,T] (0-padded), `lengths` int64 [N], `class_ids` int64 [N],
`img64` / `img128` / `img256` uint8 [N,3,R,R].  Pixels are mapped with (x - 127.5) / 127.5 like the reference's
Training.scale_255_to_1 (utilities/training.py:23-25).  A shard may hold `img256` alone: the two smaller images are then resampled
from it (antialiased bilinear, downsample_reference below).

Two loaders yield the same tuples in the same order: ShardBatches converts each batch on the host and copies fp32 to the device;
DeviceShardBatches keeps a shard's uint8 images in device memory and makes a batch with one kernel (backend.functional.image_prep).
"""
from __future__ import annotations

from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

Batch = Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]


def scale_255_to_1(images: Tensor) -> Tensor:
    return (images.float() - 127.5) / 127.5


def scale_1_to_255(images: Tensor) -> Tensor:
    return images * 127.5 + 127.5


def synthetic_batches(batch_size: int, seq_len: int = 10, vocab: int = 1000, n_batches: int = 1, seed: int = 0,
                      device="cpu") -> Iterator[Batch]:
    """Random-token captions + uniform images at 64/128/256 (BASELINE.json north_star's synthetic workload)."""
    g = torch.Generator().manual_seed(seed)
    for _ in range(n_batches):
        words = torch.randint(1, vocab, (batch_size, seq_len), generator=g)
        lengths = torch.randint(2, seq_len + 1, (batch_size,), generator=g)
        words = words * (torch.arange(seq_len).view(1, -1) < lengths.view(-1, 1))          # zero-pad past each length
        class_ids = torch.randint(0, 50, (batch_size,), generator=g)
        imgs = [torch.rand(batch_size, 3, r, r, generator=g) * 2 - 1 for r in (64, 128, 256)]
        yield tuple(t.to(device) for t in (words, lengths, class_ids, *imgs))


_IMAGE_KEYS = ("img64", "img128", "img256")


def downsample_reference(u8: Tensor, factor: int, dtype=torch.float32) -> Tensor:
    """[..., H, W] uint8 -> [..., H / factor, W / factor] in [-1, 1]: scale_255_to_1 of the image resampled with the antialiased bilinear
    (triangle) filter of torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False), restated in integers.

    Per axis, output o takes taps factor*o - factor/2 .. factor*o + 3*factor/2 - 1 with weights [1 3 3 1] (factor 2) or
    [1 3 5 7 7 5 3 1] (factor 4); taps outside the image are dropped and the rest renormalised.  The weighted byte sum is an exact
    integer `num` over an integer `den`, and the result is the one division (2 num - 255 den) / (255 den) done in float64 and rounded
    to `dtype`: for float32 that is the correctly rounded value (a quotient of integers below 2^24 is never within 2^-49 of a float32
    rounding boundary unless it sits on it exactly, so the float64 step cannot tip the rounding).  It is what ShardBatches yields for a
    256-only shard, and the expected value of agan_image_prep's derived planes."""
    if factor not in (2, 4):
        raise ValueError(f"downsample_reference: factor {factor} is not 2 or 4")
    if u8.dtype != torch.uint8 or u8.dim() < 2 or u8.shape[-1] % factor or u8.shape[-2] % factor:
        raise ValueError(f"downsample_reference: expected uint8 [..., H, W] with H and W multiples of {factor}, got {u8.dtype} {tuple(u8.shape)}")
    w = torch.tensor([1, 3, 3, 1] if factor == 2 else [1, 3, 5, 7, 7, 5, 3, 1], dtype=torch.int64)
    h = factor // 2

    def along_last(x: Tensor) -> Tensor:                                  # zero padding = a dropped tap
        return (torch.nn.functional.pad(x, (h, h)).unfold(-1, 2 * factor, factor) * w).sum(-1)

    x = u8.to(torch.int64)
    num = along_last(along_last(x).transpose(-1, -2)).transpose(-1, -2)
    den_x = along_last(torch.ones(u8.shape[-1], dtype=torch.int64))
    den_y = along_last(torch.ones(u8.shape[-2], dtype=torch.int64))
    den = den_y.view(-1, 1) * den_x.view(1, -1)
    return ((2 * num - 255 * den).double() / (255 * den).double()).to(dtype)


def _load_shard(path: str) -> dict:
    with np.load(path, allow_pickle=False, mmap_mode=None) as npz:
        keys = ("words", "lengths", "class_ids") + tuple(k for k in _IMAGE_KEYS if k in npz.files)
        z = {k: npz[k] for k in keys}                                     # NpzFile re-reads per access
    if "img256" not in z or (("img64" in z) != ("img128" in z)):
        raise ValueError(f"{path}: a shard holds img64, img128 and img256, or img256 alone (found {sorted(k for k in z if k.startswith('img'))})")
    return z


class ShardBatches:
    """Iterates the batch tuple over one or more .npz shards; short / too-short-caption batches are skipped exactly as the
    training loop does (train.py:112: `min(lengths) < 2 or len(words) < BATCH_SIZE`)."""

    def __init__(self, paths: Sequence[str], batch_size: int, device="cpu", shuffle: bool = True, seed: int = 0):
        self.paths, self.batch_size, self.device, self.shuffle = list(paths), batch_size, device, shuffle
        self.rng = np.random.default_rng(seed)

    def __iter__(self) -> Iterator[Batch]:
        for path in self.paths:
            z = _load_shard(path)
            n = len(z["lengths"])
            order = self.rng.permutation(n) if self.shuffle else np.arange(n)
            for s in range(0, n - self.batch_size + 1, self.batch_size):
                idx = np.sort(order[s:s + self.batch_size])
                lengths = torch.from_numpy(z["lengths"][idx])
                if int(lengths.min()) < 2:
                    continue
                words = torch.from_numpy(z["words"][idx])[:, :int(lengths.max())]
                class_ids = torch.from_numpy(z["class_ids"][idx])
                if "img64" in z:
                    imgs = [scale_255_to_1(torch.from_numpy(z[k][idx])) for k in _IMAGE_KEYS]
                else:                                                     # 256-only shard
                    u8 = torch.from_numpy(z["img256"][idx])
                    imgs = [downsample_reference(u8, 4), downsample_reference(u8, 2), scale_255_to_1(u8)]
                yield tuple(t.to(self.device, non_blocking=True) for t in (words, lengths, class_ids, *imgs))


class _Slot:
    """One output set of DeviceShardBatches: pinned staging + device copy of a batch's small tensors, and its three images."""

    def __init__(self):
        self.host = self.dev = None          # uint8 [capacity]: words | lengths | class_ids | rows | flip, each section 16-byte aligned
        self.images: Optional[List[Tensor]] = None
        self.copied = self.ready = self.released = None      # events: staging read / batch complete / last use by the consumer enqueued


class DeviceShardBatches:
    """ShardBatches' tuples, in ShardBatches' order, from uint8 images that stay in device memory.

    Per shard, the uint8 image arrays go to pinned host memory and are uploaded once, asynchronously, on a copy stream.  Per batch the
    host sends only the row indices, the mirror flags and the captions (one pinned staging block, one copy) and ONE kernel
    (backend.functional.image_prep) gathers, mirrors and scales the images at the three resolutions.  With flip_prob = 0 the batches
    equal ShardBatches(paths, batch_size, device=device, shuffle=shuffle, seed=seed)'s bit for bit: shard order, permutation, np.sort
    of each batch's indices, the min(lengths) < 2 skip and the trim of `words` to max(lengths) are the same code path.

    flip_prob: each sample of a shard gets a coin from the same numpy generator, drawn after the shard's permutation (the reference
    stores a mirrored copy of every image instead, data/bedrooms.py:139-141).  No coin is drawn at flip_prob = 0.

    Prefetch and validity.  Batch n+1 is made on a side stream while the caller's stream runs step n; the caller's stream waits on a
    "ready" event before it sees a batch.  The host waits for the device only to reuse a staging block, that is when it has run three
    batches ahead of it.  A YIELDED BATCH STAYS VALID UNTIL THE ITERATOR HAS BEEN ADVANCED TWICE: work that uses batch n may be
    enqueued up to the call that returns batch n+2.  Each advance records an event on the caller's stream, and the set of batch n is
    rewritten only behind the event of that second advance.  One batch of look-ahead under this contract takes three output sets (the
    one being made, the one just handed out, the one handed out before it); at batch 24 a set is 25 MB.  Enqueue the work on the
    stream that is current when the iterator is advanced.

    into=(img64, img128, img256): the kernel writes straight into these tensors (the static inputs of GanTrainStep.capture) on the
    current stream, with no look-ahead and no second copy: the images are valid until the next advance, then hold the next batch --
    which is what graphed.replay() wants.  words / lengths / class_ids follow the rule above.

    A shard whose uint8 images exceed max_resident_bytes raises ValueError: split the shard (there is no host-side fallback)."""

    SETS = 3

    def __init__(self, paths: Sequence[str], batch_size: int, device, shuffle: bool = True, seed: int = 0, flip_prob: float = 0.0,
                 into: Optional[Sequence[Tensor]] = None, max_resident_bytes: int = 16 << 30):
        from ..backend import lib as L
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.AganError(f"DeviceShardBatches: device {self.device}; resident shards live on an MI355X (no CPU fallback -- ShardBatches is the host loader)")
        if not 0.0 <= float(flip_prob) <= 1.0:
            raise ValueError(f"flip_prob {flip_prob} outside [0, 1]")
        self.paths, self.batch_size, self.shuffle, self.flip_prob = list(paths), int(batch_size), shuffle, float(flip_prob)
        self.max_resident_bytes = int(max_resident_bytes)
        self.rng = np.random.default_rng(seed)
        self.into = None if into is None else list(into)
        if self.into is not None and len(self.into) != 3:
            raise ValueError("into: expected (img64, img128, img256)")

    # -- host side: shards and the batches they hold ------------------------------------------------------------------------------
    def _check_resident(self, path: str, z: dict) -> None:
        nbytes = sum(int(z[k].nbytes) for k in _IMAGE_KEYS if k in z)
        if nbytes > self.max_resident_bytes:
            raise ValueError(f"{path}: {nbytes} bytes of uint8 images exceed max_resident_bytes = {self.max_resident_bytes}: split the shard")

    def _upload(self, z: dict, copy_stream, user_streams) -> Tuple[list, object, list]:
        """-> ([img256, img128 | (H, W), img64 | (H, W)] as image_prep planes, event of the upload, the pinned copies it reads)"""
        planes, pinned = [], []
        with torch.cuda.stream(copy_stream):
            for k in reversed(_IMAGE_KEYS):
                if k in z:
                    host = torch.empty(z[k].shape, dtype=torch.uint8, pin_memory=True)
                    host.numpy()[...] = z[k]
                    dev = torch.empty(z[k].shape, dtype=torch.uint8, device=self.device)
                    dev.copy_(host, non_blocking=True)
                    for st in user_streams:
                        dev.record_stream(st)
                    pinned.append(host)
                    planes.append(dev)
                else:
                    f = 256 // int(k[3:])
                    H, W = z["img256"].shape[2:]
                    if H % f or W % f:
                        raise ValueError(f"img256 of {H} x {W} cannot be divided by {f} for {k}")
                    planes.append((H // f, W // f))
            done = torch.cuda.Event()
            done.record(copy_stream)
        return planes, done, pinned

    def _jobs(self):
        """-> (shard dict, sorted sample indices, mirror flags or None) per batch that passes the guard, in ShardBatches' order"""
        for path in self.paths:
            z = _load_shard(path)
            self._check_resident(path, z)
            n = len(z["lengths"])
            order = self.rng.permutation(n) if self.shuffle else np.arange(n)
            coins = (self.rng.random(n) < self.flip_prob) if self.flip_prob > 0.0 else None
            for s in range(0, n - self.batch_size + 1, self.batch_size):
                idx = np.sort(order[s:s + self.batch_size])
                if int(z["lengths"][idx].min()) < 2:
                    continue
                yield z, idx, (coins[idx] if coins is not None else None)

    # -- device side --------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _sections(B: int, T: int) -> Tuple[int, int, int, int, int, int]:
        up = lambda v: (v + 15) & ~15
        o_len = up(8 * B * T)
        o_cid = o_len + up(8 * B)
        o_row = o_cid + up(8 * B)
        o_flip = o_row + up(4 * B)
        return 0, o_len, o_cid, o_row, o_flip, o_flip + up(B)

    def _launch(self, slot: _Slot, job, resident, stream, consumer) -> Batch:
        """Enqueue one batch on `stream` into `slot` behind the consumer's release event; -> the tuple (valid after slot.ready)."""
        from ..backend import functional as HF
        z, idx, coins = job
        planes, uploaded = resident
        B = len(idx)
        lengths = z["lengths"][idx]
        T = int(lengths.max())
        o_words, o_len, o_cid, o_row, o_flip, total = self._sections(B, T)
        if slot.host is None or slot.host.numel() < total:
            slot.host = torch.empty(max(total, self._sections(B, z["words"].shape[1])[-1]), dtype=torch.uint8, pin_memory=True)
            slot.dev = torch.empty(slot.host.numel(), dtype=torch.uint8, device=self.device)
            slot.copied = None
        shapes = [(B, p.shape[1], p.shape[2], p.shape[3]) if isinstance(p, Tensor) else (B, planes[0].shape[1], p[0], p[1]) for p in planes]
        if self.into is not None:
            images = [self.into[2], self.into[1], self.into[0]]
        else:
            if slot.images is None or [tuple(t.shape) for t in slot.images] != shapes:
                slot.images = [torch.empty(sh, device=self.device) for sh in shapes]
            images = slot.images
        if slot.copied is not None:
            slot.copied.synchronize()            # the copy that last read this staging block: three batches ago, long done
        h = slot.host.numpy()
        h[o_words:o_words + 8 * B * T].view(np.int64).reshape(B, T)[...] = z["words"][idx][:, :T]
        h[o_len:o_len + 8 * B].view(np.int64)[...] = lengths
        h[o_cid:o_cid + 8 * B].view(np.int64)[...] = z["class_ids"][idx]
        h[o_row:o_row + 4 * B].view(np.int32)[...] = idx
        if coins is not None:
            h[o_flip:o_flip + B] = coins
        if slot.released is None:
            slot.copied, slot.ready, slot.released = torch.cuda.Event(), torch.cuda.Event(), torch.cuda.Event()
        slot.released.record(consumer)           # everything the consumer has enqueued on the set's earlier batch lies before this
        stream.wait_event(slot.released)
        stream.wait_event(uploaded)
        with torch.cuda.stream(stream):
            for t in (slot.dev, *images):
                t.record_stream(stream)
            slot.dev[:total].copy_(slot.host[:total], non_blocking=True)
            slot.copied.record(stream)
            d = slot.dev
            rows = d[o_row:o_row + 4 * B].view(torch.int32)
            flip = d[o_flip:o_flip + B] if coins is not None else None
            HF.image_prep(planes, rows, flip, out=images)
            slot.ready.record(stream)
        words = d[o_words:o_words + 8 * B * T].view(torch.int64).view(B, T)
        return (words, d[o_len:o_len + 8 * B].view(torch.int64), d[o_cid:o_cid + 8 * B].view(torch.int64), images[2], images[1], images[0])

    def __iter__(self) -> Iterator[Batch]:
        dev = self.device
        direct = self.into is not None
        jobs = self._jobs()
        job = next(jobs, None)                     # (an over-sized first shard is refused before any device work)
        copy_stream = torch.cuda.Stream(dev)
        side = None if direct else torch.cuda.Stream(dev)
        slots = [_Slot() for _ in range(self.SETS)]
        resident = {}                              # id(shard dict) -> (planes, upload event, pinned copies); the current shard only

        def launch(n, job):
            consumer = torch.cuda.current_stream(dev)
            stream = consumer if direct else side
            key = id(job[0])
            if key not in resident:
                resident.clear()
                resident[key] = self._upload(job[0], copy_stream, (stream,))
            planes, uploaded, _ = resident[key]
            slot = slots[n % self.SETS]
            return slot, self._launch(slot, job, (planes, uploaded), stream, consumer)

        n = 0
        if direct:
            while job is not None:                 # nothing is made ahead: `into` holds exactly the batch handed out
                _, batch = launch(n, job)
                yield batch
                n, job = n + 1, next(jobs, None)
            return
        ahead = launch(n, job) if job is not None else None
        while ahead is not None:
            slot, batch = ahead
            n, job = n + 1, next(jobs, None)
            ahead = launch(n, job) if job is not None else None
            torch.cuda.current_stream(dev).wait_event(slot.ready)
            yield batch


def write_shard(path: str, words: np.ndarray, lengths: np.ndarray, class_ids: np.ndarray, img64: Optional[np.ndarray] = None,
                img128: Optional[np.ndarray] = None, img256: Optional[np.ndarray] = None) -> None:
    """img64 and img128 may both be left out: a 256-only shard, whose smaller images the loaders resample from img256."""
    if img256 is None or (img64 is None) != (img128 is None):
        raise ValueError("write_shard: give img64, img128 and img256, or img256 alone")
    images = {k: a for k, a in zip(_IMAGE_KEYS, (img64, img128, img256)) if a is not None}
    for k, a in images.items():
        r = int(k[3:])
        if a.dtype != np.uint8 or a.shape[1:] != (3, r, r):
            raise ValueError(f"img{r} must be uint8 [N,3,{r},{r}]")
    np.savez(path, words=words.astype(np.int64), lengths=lengths.astype(np.int64), class_ids=class_ids.astype(np.int64), **images)
