"""torch.autograd bridges onto the C ABI of libagan_hip.so.

PyTorch is plumbing here: it owns device memory (caching allocator), the current HIP stream and the autograd
tape.  Every numerical op on the hot path is a hand-written gfx950 kernel reached through `lib.call`.
All tensors are NCHW fp32 like the reference's.
"""
from __future__ import annotations

import ctypes
import math
from ctypes import byref, c_void_p
from typing import Dict, Optional, Tuple

import contextlib
import os
import weakref

import torch
from torch import Tensor
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import lib as L

# arithmetic mode used by the MFMA contractions; PREC_F32 = exact fp32 products (parity mode, the default)
_PRECISION = [L.PREC_F32]


def set_precision(p: int) -> None:
    if int(p) != _PRECISION[0]:
        # the batched re-pack (packed_weight / _repack_group) refreshes EVERY registered pack of a layout family: forget the ones the
        # old mode registered (they re-register on their next use), or a later mode keeps re-packing layouts nothing reads
        for rng in _FLAT_RANGES:
            rng.forget()
    _PRECISION[0] = int(p)


def get_precision() -> int:
    return _PRECISION[0]


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> c_void_p:
    """raw handle of torch's current HIP stream (what every library call enqueues on)"""
    if _RAW_STREAM is not None:              # ~10x cheaper than building a torch.cuda.Stream object per launch
        return c_void_p(_RAW_STREAM(torch.cuda.current_device()))
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[Tensor]) -> Optional[c_void_p]:
    return None if t is None else c_void_p(t.data_ptr())


def _dev(t: Tensor, what: str) -> Tensor:
    if not t.is_cuda:
        raise L.AganError(f"{what}: tensor is on {t.device}; the AttnGAN HIP path runs on an MI355X only (no CPU fallback)")
    if t.dtype != torch.float32:
        if t.dtype in _DT_OF:            # a 16-bit activation arriving at a kernel without typed storage: widen at the boundary
            return t.float().contiguous()
        raise L.AganError(f"{what}: expected float32, got {t.dtype}")
    return t.contiguous()


# ---- 16-bit activation storage (include/agan.h: AGAN_DT_*) ------------------------------------------------------------------
# Off by default: every tensor in HBM is fp32 like the reference's.  set_activation_storage("bf16" | "f16") -- valid with
# set_precision(PREC_BF16 / PREC_F16) -- lets conv outputs, BatchNorm inputs / outputs and their gradients live in the operand
# type of the matrix cores: rounded ONCE when stored, loaded without conversion, half the bytes.  Kernels without typed storage
# (attention, the <= 4-channel convs, losses) widen their inputs at the boundary (_dev).
_DT_OF = {torch.bfloat16: L.DT_BF16, torch.float16: L.DT_F16}
_TORCH_OF = {L.DT_F32: torch.float32, L.DT_BF16: torch.bfloat16, L.DT_F16: torch.float16}
_STORAGE = [L.DT_F32]


def set_activation_storage(kind) -> None:
    dt = {None: L.DT_F32, "f32": L.DT_F32, "bf16": L.DT_BF16, "f16": L.DT_F16}[kind]
    _STORAGE[0] = dt


def get_activation_storage() -> int:
    """the storage type 16-bit-capable kernels produce right now: AGAN_DT_F32 unless the precision mode matches the request"""
    dt = _STORAGE[0]
    if dt == L.DT_BF16 and _PRECISION[0] == L.PREC_BF16:
        return dt
    if dt == L.DT_F16 and _PRECISION[0] == L.PREC_F16:
        return dt
    return L.DT_F32


def _fp32_only(what: str, family: str, *tensors: Tensor) -> None:
    """the guard of an entry point whose kernels have no 16-bit storage forms"""
    if get_activation_storage() != L.DT_F32 or any(t.dtype in _DT_OF for t in tensors):
        raise L.AganError(f"{what}: the {family} kernels store fp32 only; 16-bit activation storage (set_activation_storage) and "
                          f"16-bit tensors are not built for them")


def _dt(t: Tensor) -> int:
    return L.DT_F32 if t.dtype == torch.float32 else _DT_OF[t.dtype]


def _act(t: Tensor, what: str) -> Tensor:
    """an activation tensor for a kernel WITH typed storage: fp32 or a 16-bit type, contiguous, on the device"""
    if not t.is_cuda:
        raise L.AganError(f"{what}: tensor is on {t.device}; the AttnGAN HIP path runs on an MI355X only (no CPU fallback)")
    if t.dtype != torch.float32 and t.dtype not in _DT_OF:
        raise L.AganError(f"{what}: expected float32 / bfloat16 / float16, got {t.dtype}")
    return t.contiguous()


_DT_SUPPORT: dict = {}


def _gather_types(g: "L.ConvGeom", pe: int, x: Tensor, want_out: int):
    """-> (x, storage type of the output) for a gather of geometry g in arithmetic mode pe: the 16-bit storage the caller would like
    where the kernel for this geometry offers it (agan_conv_gather_dt_supported), else fp32 -- widening a 16-bit x when the layer
    cannot read it as it stands (the deep 4x4 layers, whose rows are shorter than one 16-byte block)."""
    def ok(xin, out):
        if xin == L.DT_F32 and out == L.DT_F32:
            return True
        key = (g.B, g.Cin, g.IH, g.IW, g.Cout, g.OH, g.OW, g.R, g.S, g.OS, g.SY, g.DY, g.OY[0], g.OY[1], pe, xin, out)
        hit = _DT_SUPPORT.get(key)
        if hit is None:
            hit = _DT_SUPPORT[key] = bool(L.load().agan_conv_gather_dt_supported(byref(g), pe, xin, out))
        return hit
    outs = [want_out, L.DT_F32] if want_out != L.DT_F32 else [L.DT_F32]
    for out in outs:
        if ok(_dt(x), out):
            return x, out
    x = x.float()
    for out in outs:
        if ok(L.DT_F32, out):
            return x, out
    return x, L.DT_F32


def _ws(nbytes: int, like: Tensor) -> Tuple[Optional[Tensor], Optional[c_void_p]]:
    if nbytes <= 0:
        return None, None
    t = torch.empty(nbytes, dtype=torch.uint8, device=like.device)
    return t, c_void_p(t.data_ptr())


# --------------------------------------------------------------------------------------------------------------
# gradient destinations: optim.FlatAdam tags every parameter with `_agan_grad_dst = (flat_grad, offset, numel)`.  Backward
# kernels then write weight gradients straight into the flat buffer and hand autograd a fresh view of it, so AccumulateGrad
# adopts the view (p.grad is None at that point) instead of launching one `grad += new` kernel per parameter.
# --------------------------------------------------------------------------------------------------------------
def grad_dst(param):
    return getattr(param, "_agan_grad_dst", None)


def _grad_out(dst, shape, like: Tensor):
    """-> (buffer the backward kernel writes, accumulate flag for the kernel, value handed back to autograd).

    Without a flat destination: a scratch tensor that autograd accumulates as usual.  With one, the FIRST contribution of a
    backward pass overwrites the parameter's slice of the flat buffer and autograd adopts a view of it as p.grad; a parameter
    used again in the same backward (a discriminator sees the real and the fake batch) has the kernel ADD into the slice and
    autograd gets None for that edge -- no `grad += new` launches, no copies."""
    if dst is None:
        t = torch.empty(shape, dtype=torch.float32, device=like.device)
        return t, 0, t
    if dst.locked:
        raise L.AganError("a backward kernel is about to write into a flat gradient slice whose bucket is already being all-reduced: "
                          "call zero_grad() (and GradBuckets.arm()) before running another backward under data parallelism")
    view = dst.flat[dst.offset:dst.offset + dst.numel].view(shape)
    dst.edges += 1
    if dst.written:
        return view, 1, None
    dst.written = True
    return view, 0, view


class GradDst:
    """Slice of a FlatAdam gradient buffer that belongs to one parameter.  `written`: a kernel has produced the slice in this
    backward; `edges`: how many kernel contributions went into it (FlatAdam._rebind tells a harmless autograd clone from a summed
    stock edge with it); `locked`: the slice's bucket has been handed to the gradient exchange (GradBuckets._launch)."""
    __slots__ = ("flat", "offset", "numel", "written", "edges", "locked")

    def __init__(self, flat: Tensor, offset: int, numel: int):
        self.flat, self.offset, self.numel, self.written, self.edges, self.locked = flat, offset, numel, False, 0, False

    def reset(self) -> None:
        self.written, self.edges, self.locked = False, 0, False


# --------------------------------------------------------------------------------------------------------------
# convolution geometry (see include/agan.h: agan_conv_geom)
# --------------------------------------------------------------------------------------------------------------
def _geom(B, Cin, IH, IW, Cout, OH, OW, R, S, OS, SY, DY, OY) -> L.ConvGeom:
    g = L.ConvGeom()
    g.B, g.Cin, g.IH, g.IW, g.Cout, g.OH, g.OW = B, Cin, IH, IW, Cout, OH, OW
    g.R, g.S, g.OS, g.SY, g.DY = R, S, OS, SY, DY
    g.OY[0], g.OY[1] = OY
    return g


_GEOM_CACHE = {}


def conv_geoms(kind: str, B: int, Cin: int, H: int, W: int, Cout: int, k: int):
    """-> (fwd geom, fwd pack mode, dgrad geom, dgrad pack mode, (OH, OW)) for the conv kinds on the path.

    same : k x k, stride 1, pad (k-1)/2          utilities/layers.py:45-53 (and nn.Linear as 1x1 on a 1x1 image)
    down : 4 x 4, stride 2, pad 1                utilities/layers.py:122,139-150
    up   : nearest x2 upsample then 3x3 pad 1    utilities/layers.py:64-65, folded into 4 parity classes of 2x2 taps
    """
    key = (kind, B, Cin, H, W, Cout, k)
    hit = _GEOM_CACHE.get(key)
    if hit is not None:
        return hit
    if kind == "same":
        p = (k - 1) // 2
        out = (_geom(B, Cin, H, W, Cout, H, W, k, k, 1, 1, 1, (-p, -p)), L.PACK_FWD,
               _geom(B, Cout, H, W, Cin, H, W, k, k, 1, 1, 1, (-p, -p)), L.PACK_DGRAD_S1, (H, W))
    elif kind == "down":
        if k != 4 or H % 2 or W % 2:
            raise L.AganError(f"down conv needs k=4 and even H,W (got k={k}, {H}x{W})")
        out = (_geom(B, Cin, H, W, Cout, H // 2, W // 2, 4, 4, 1, 2, 1, (-1, -1)), L.PACK_FWD,
               _geom(B, Cout, H // 2, W // 2, Cin, H, W, 2, 2, 2, 1, -1, (0, 1)), L.PACK_DGRAD_4x4S2, (H // 2, W // 2))
    elif kind == "up":
        if k != 3:
            raise L.AganError("upsample conv needs k=3")
        out = (_geom(B, Cin, H, W, Cout, 2 * H, 2 * W, 2, 2, 2, 1, 1, (-1, 0)), L.PACK_UP_FWD,
               _geom(B, Cout, 2 * H, 2 * W, Cin, H, W, 4, 4, 1, 2, 1, (-1, -1)), L.PACK_UP_DGRAD, (2 * H, 2 * W))
    else:
        raise L.AganError(f"unknown conv kind {kind!r}")
    _GEOM_CACHE[key] = out
    return out


# Packed weights are cached per owning module (a plain dict the module passes in): a parameter is re-packed only when
# it changed -- in-place version bump (load_state_dict), new storage (.to(), FlatAdam re-homing) or an optimiser step
# that wrote through the raw pointer.  Optimiser steps are tracked per flat buffer (register_flat): the generator's Adam
# step must not invalidate the discriminators' packed weights.  Writes through a raw pointer into memory that is not a
# registered flat buffer bump the global epoch instead.  Without a cache dict every call re-packs.
_WEIGHT_EPOCH = [0]
_FLAT_RANGES: list = []          # the registered _FlatRange records


def _stamp(t: Tensor) -> Tuple[int, int]:
    """what shows that a tensor changed without a raw-pointer write: new storage moves the address, an in-place edit the version"""
    return t.data_ptr(), t._version


class _FlatRange:
    """A registered flat parameter buffer: its address range, the epoch that raw-pointer writes advance, the pack entries of its
    views and their device job tables {layout family: (table, jobs, blocks)}.  `registered` turns False when the range is dropped:
    an entry that still points here then finds its range by address again."""
    __slots__ = ("start", "end", "epoch", "entries", "tables", "registered")

    def __init__(self, start: int, end: int, epoch: int):
        self.start, self.end, self.epoch, self.entries, self.tables, self.registered = start, end, epoch, [], {}, True

    def written(self) -> None:
        """a kernel wrote the buffer through its raw pointer: every pack of its views is stale"""
        self.epoch += 1

    def forget(self) -> None:
        """drop every entry and job table; an entry registers again at its next use"""
        for e in self.entries:
            e.rng = None
        self.entries, self.tables = [], {}


class _PackEntry:
    """One packed form of one weight: the value of the owning module's cache[(mode, prec)] and, while `rng` is a range, a member
    of that range's `entries` -- the same object.  `ptr`, `tver`, `dims` say which tensor `wk` was packed from; `epoch` and
    `flat_epoch` are the global epoch and the range's (-1 outside any range) at the time of the pack."""
    __slots__ = ("rng", "mode", "prec", "dims", "ptr", "tver", "wk", "epoch", "flat_epoch")

    def __init__(self, mode: int, prec: int):
        self.rng, self.mode, self.prec, self.dims, self.ptr, self.tver, self.wk = None, mode, prec, None, 0, -1, None
        self.epoch = self.flat_epoch = -1

    def packed(self) -> None:
        """`wk` was just written from the tensor the entry names"""
        self.epoch, self.flat_epoch = _WEIGHT_EPOCH[0], self.rng.epoch if self.rng is not None else -1


def bump_weight_epoch() -> None:
    _WEIGHT_EPOCH[0] += 1


def _drop_ranges(gone) -> None:
    for r in _FLAT_RANGES:
        r.registered = not gone(r)
    _FLAT_RANGES[:] = [r for r in _FLAT_RANGES if r.registered]


def register_flat(flat: Tensor) -> None:
    """Declare a flat parameter buffer whose views are conv/linear weights and which agan_adam_step updates in place."""
    start = flat.data_ptr()
    end = start + flat.numel() * flat.element_size()
    # a buffer registered earlier that overlaps this one has been freed (the allocator handed its memory out again): drop it,
    # and start above every epoch seen so far so that no cached pack of recycled memory can look fresh
    top = max([r.epoch for r in _FLAT_RANGES] + [0])
    _drop_ranges(lambda r: r.start < end and r.end > start)
    _FLAT_RANGES.append(_FlatRange(start, end, top + 1))


def unregister_flat(flat: Tensor) -> None:
    start = flat.data_ptr()
    _drop_ranges(lambda r: r.start == start)


def _flat_range(ptr: int) -> Optional[_FlatRange]:
    for r in _FLAT_RANGES:
        if r.start <= ptr < r.end:
            return r
    return None


_PACK_JOB_DTYPE = [("w", "<u8"), ("wk", "<u8"), ("mode", "<i4"), ("cout", "<i4"), ("cin", "<i4"), ("kh", "<i4"), ("kw", "<i4"),
                   ("first_block", "<i4")]          # include/agan.h: agan_pack_job


def _pack_table(rng: _FlatRange, prec: int):
    """device job table of a flat buffer's pack entries of ONE layout family (`prec`: the fp32 k-table layouts, or one of the 16-bit
    patch layouts); built on the host, one H2D copy; rebuilt when an entry was added or changed (packed_weight empties `tables`)"""
    hit = rng.tables.get(prec)
    if hit is None:
        import numpy as np
        if torch.cuda.is_current_stream_capturing():
            raise L.AganError("packed-weight job table missing during HIP-graph capture: run a warm-up step and "
                              "build_pack_tables() first (GanTrainStep.capture does)")
        lib = L.load()
        entries = [e for e in rng.entries if e.prec == prec]
        jobs = np.zeros(len(entries), dtype=_PACK_JOB_DTYPE)
        first = 0
        for i, e in enumerate(entries):
            jobs[i] = (e.ptr, e.wk.data_ptr(), e.mode, *e.dims, first)
            first += lib.agan_pack_job_blocks_prec(e.mode, *e.dims, prec)
        table = torch.from_numpy(jobs.view(np.uint8).copy()).to(entries[0].wk.device)
        hit = rng.tables[prec] = (table, len(entries), first)
    return hit


def build_pack_tables() -> None:
    """Build every missing job table now (host work + H2D copies), e.g. before capturing a HIP graph."""
    for rng in _FLAT_RANGES:
        for prec in sorted({e.prec for e in rng.entries}):
            _pack_table(rng, prec)


def _repack_group(rng: _FlatRange, prec: int) -> None:
    """Re-pack every registered packed weight of one flat buffer and one layout family in a single launch (agan_pack_weights).
    After an optimiser step all of them are stale at once, and most are a few KB: one launch instead of one ~10-17 us launch per
    tensor and mode (1.7 ms per step in the 16-bit modes before they took this path too)."""
    table, n, total = _pack_table(rng, prec)
    L.call("agan_pack_weights", _p(table), n, total, prec, _stream())
    for e in rng.entries:
        if e.prec == prec:
            e.packed()


_EFF_PREC = {}


def effective_precision(g: L.ConvGeom) -> int:
    """The arithmetic mode a gather geometry really runs in under the current precision setting (include/agan.h:
    agan_conv_effective_prec): the 16-bit patch kernels take the 3x3 / 2x2-per-class / 4x4-s2 geometries, everything else is fp32."""
    prec = _PRECISION[0]
    if prec == L.PREC_F32:
        return prec
    key = (prec, g.B, g.Cin, g.IH, g.IW, g.Cout, g.OH, g.OW, g.R, g.S, g.OS, g.SY, g.DY, g.OY[0], g.OY[1])
    hit = _EFF_PREC.get(key)
    if hit is None:
        hit = _EFF_PREC[key] = int(L.load().agan_conv_effective_prec(byref(g), prec))
    return hit


_EFF_WPREC = {}


def wgrad_effective_precision(g: L.ConvGeom, pack_mode: int) -> int:
    """the arithmetic mode the weight gradient of forward geometry g runs in (include/agan.h: agan_conv_wgrad_effective_prec)"""
    prec = _PRECISION[0]
    if prec == L.PREC_F32:
        return prec
    key = (prec, pack_mode, g.B, g.Cin, g.IH, g.IW, g.Cout, g.OH, g.OW, g.R, g.S, g.OS, g.SY, g.DY, g.OY[0], g.OY[1])
    hit = _EFF_WPREC.get(key)
    if hit is None:
        hit = _EFF_WPREC[key] = int(L.load().agan_conv_wgrad_effective_prec(byref(g), pack_mode, prec))
    return hit


def packed_weight(w: Tensor, mode: int, cache: Optional[dict] = None, prec: Optional[int] = None) -> Tensor:
    if prec is None:
        prec = _PRECISION[0]
    ent = cache.get((mode, prec)) if cache is not None else None
    ptr, tver = _stamp(w)
    # the range the entry knows, while that range is registered and the tensor has not moved; else the one at the tensor's address
    rng = ent.rng if (ent is not None and ent.ptr == ptr and ent.rng is not None and ent.rng.registered) else _flat_range(ptr)
    # packed from exactly this tensor, and listed under the range the tensor lies in now (written out: the hit path is ~2 calls per conv)
    if ent is not None and ent.rng is rng and ent.ptr == ptr and ent.tver == tver and ent.dims == w.shape:
        if ent.epoch == _WEIGHT_EPOCH[0] and ent.flat_epoch == (rng.epoch if rng is not None else -1):
            return ent.wk                       # and no raw-pointer write since: fresh
        if rng is not None:
            # same tensor, only the optimiser epoch moved: its whole group (same layout family) is stale -> one batched launch
            _repack_group(rng, prec)
            return ent.wk
    dims = tuple(w.shape)
    n = L.load().agan_packed_weight_bytes(mode, *dims, prec)
    if n == 0:
        raise L.AganError(f"pack mode {mode} / precision {prec} does not take a {dims[2]}x{dims[3]} kernel")
    if ent is None:
        ent = _PackEntry(mode, prec)
    if ent.wk is None or ent.wk.numel() != n or ent.wk.device != w.device:
        ent.wk = torch.empty(n, dtype=torch.uint8, device=w.device)
    L.call("agan_pack_weight", _p(w), _p(ent.wk), mode, *dims, prec, _stream())
    if cache is not None:
        cache[(mode, prec)] = ent
        if ent.rng is not rng:                  # first pack, or the tensor now lies in another range: move the entry there
            if ent.rng is not None:
                ent.rng.entries.remove(ent)
                ent.rng.tables = {}
            ent.rng = rng
            if rng is not None:
                rng.entries.append(ent)
        ent.ptr, ent.tver, ent.dims = ptr, tver, dims
        ent.packed()
        if rng is not None:
            rng.tables = {}                     # job tables are rebuilt at the next batched re-pack
    return ent.wk


_KTABLE_CACHE = {}


def ktable(g: L.ConvGeom, device) -> Tensor:
    """Reduction-index table of a geometry (include/agan.h: agan_conv_ktable), built once per (geometry, device)."""
    key = (g.Cin, g.IH, g.IW, g.R, g.S, g.DY, str(device))
    t = _KTABLE_CACHE.get(key)
    if t is None:
        n = L.load().agan_conv_ktable_elems(byref(g))
        t = torch.empty(n, dtype=torch.int32, device=device)
        L.call("agan_conv_ktable", byref(g), _p(t), _stream())
        _KTABLE_CACHE[key] = t
    return t


# optional launch observer (bench.py times the conv engine with HIP events through it): begin(kind, phase, geom) / end()
_OBSERVER = [None]


def set_launch_observer(obs) -> None:
    _OBSERVER[0] = obs


# --------------------------------------------------------------------------------------------------------------
# amax slots (AGAN_PREC_F16X3, include/agan.h).  The fp16 split mode needs max|x| of every tensor a conv gathers.  The kernel that
# PRODUCES the tensor (BatchNorm forward / backward apply, a conv epilogue) folds that maximum into a small device slot while
# it writes the tensor; the slot travels with the tensor OBJECT (autograd hands the same Python object from a producer Function
# to its consumer, forward and backward) through an identity-keyed registry.  A tensor that arrives without a slot (torch.cat,
# the image batch, a gradient autograd summed from two edges) gets one from agan_absmax: one extra read of that tensor.
# Slots come from a zeroed arena window that amax_begin_step() opens (ONE fill launch per train step, graph-capturable);
# outside a step every slot is its own torch.zeros.  Only LARGE tensors take the fused route (_AMAX_FUSE_MIN).
# --------------------------------------------------------------------------------------------------------------
_AMAX_REG: dict = {}
_AMAX_ARENA: dict = {}            # device -> [arena tensor, window index, next slot, limit]
_AMAX_WINDOW, _AMAX_WINDOWS = 1024, 4


def _needs_amax() -> bool:
    """modes whose kernels want max|x| of the tensors they gather: the fp16 split (every gather and weight gradient) and bf16x6 (its
    weight gradients run on the fp16-split kernel: include/agan.h, agan_conv_wgrad_effective_prec)"""
    return _PRECISION[0] in (L.PREC_F16X3, L.PREC_BF16X6)


def amax_begin_step(device) -> None:
    """Open a fresh zeroed window of amax slots for one train step (no-op unless a mode that needs them is on)."""
    if not _needs_amax():
        return
    ent = _AMAX_ARENA.get(device)
    if ent is None:
        ent = _AMAX_ARENA[device] = [torch.zeros(_AMAX_WINDOWS * _AMAX_WINDOW * L.AMAX_SLOT, dtype=torch.float32, device=device), -1, 0, 0]
    ent[1] = (ent[1] + 1) % _AMAX_WINDOWS
    lo = ent[1] * _AMAX_WINDOW * L.AMAX_SLOT
    ent[0][lo:lo + _AMAX_WINDOW * L.AMAX_SLOT].zero_()
    ent[2], ent[3] = ent[1] * _AMAX_WINDOW, (ent[1] + 1) * _AMAX_WINDOW


def _amax_new(device) -> Tensor:
    ent = _AMAX_ARENA.get(device)
    if ent is not None and ent[2] < ent[3]:
        i = ent[2]
        ent[2] += 1
        return ent[0][i * L.AMAX_SLOT:(i + 1) * L.AMAX_SLOT]
    return torch.zeros(L.AMAX_SLOT, dtype=torch.float32, device=device)


def _amax_put(t: Tensor, slot: Tensor) -> None:
    k = id(t)
    _AMAX_REG[k] = (weakref.ref(t, lambda _r, k=k: _AMAX_REG.pop(k, None)), slot)


def amax_of(t: Tensor) -> Tensor:
    """the amax slot of a tensor: the one its producer filled, else a fresh one filled by agan_absmax"""
    e = _AMAX_REG.get(id(t))
    if e is not None and e[0]() is t:
        return e[1]
    slot = _amax_new(t.device)
    L.call("agan_absmax", _p(t), t.numel(), _p(slot), _stream())
    _amax_put(t, slot)
    return slot


_AMAX_FUSE_MIN = int(os.environ.get("AGAN_AMAX_FUSE_MIN", 1 << 22))      # elements: below this a separate agan_absmax launch (~5 us) is as cheap as the fused commit


def _amax_out(t: Tensor) -> Optional[Tensor]:
    """slot for a kernel that is about to produce the LARGE tensor `t` (None unless the fp16 split mode is on): the producer folds
    max|t| into it while it streams the tensor, which saves the consumer conv a second pass over tens of megabytes"""
    if not _needs_amax() or t.numel() < _AMAX_FUSE_MIN:
        return None
    slot = _amax_new(t.device)
    _amax_put(t, slot)
    return slot


def _gather(x: Tensor, wk: Tensor, bias: Optional[Tensor], g: L.ConvGeom, out: Tensor, kind: str = "", phase: str = "",
            act: int = 0, lrelu_mask: Optional[Tensor] = None, prec: int = L.PREC_F32, in_amax: Optional[Tensor] = None) -> None:
    lib = L.load()
    nbytes = lib.agan_conv_gather_ws_bytes(byref(g), prec)
    ws, wsp = _ws(nbytes, x)
    kt = ktable(g, x.device)
    obs = _OBSERVER[0]
    if obs is not None:
        obs.begin(kind, phase, g, x.element_size(), out.element_size())
    out_amax = _amax_out(out) if prec != L.PREC_F32 else None       # the 16-bit kernels fold max|out| into a slot as they store
    L.call("agan_conv_gather_dt", _p(x), _p(wk), _p(bias), _p(out), byref(g), _p(kt), prec, act, _p(lrelu_mask), wsp, nbytes,
           _stream(), _p(in_amax), _p(out_amax), _dt(x), _dt(out))
    if obs is not None:
        obs.end()


# Weight gradients feed nothing but the optimiser, so a training step may fork them onto a side stream: they then overlap the
# HBM-bound kernels (BatchNorm / activation backward, slab sums) of the data-gradient chain instead of queueing between them.
_SIDE_STREAMS: Dict[int, "torch.cuda.Stream"] = {}
_SIDE_DIRTY: Dict[int, bool] = {}
_WGRAD_SIDE = [False]


def set_wgrad_side_stream(flag: bool) -> bool:
    """Fork weight/bias gradients that go straight into a flat gradient buffer (grad_dst) onto a per-stream side stream.
    Whoever reads those gradients must call join_side_stream() on the forking stream first (FlatAdam.step and GradBuckets do)."""
    old = _WGRAD_SIDE[0]
    _WGRAD_SIDE[0] = bool(flag)
    return old


def wgrad_side_stream_enabled() -> bool:
    return _WGRAD_SIDE[0]


def join_all_side_streams(target) -> None:
    """Make `target` (a stream about to read gradients, e.g. the collective stream) wait for every forked side stream."""
    for key, side in _SIDE_STREAMS.items():
        if _SIDE_DIRTY.get(key):
            target.wait_stream(side)


def set_side_stream_for(stream, side) -> None:
    """Use `side` for the weight gradients forked off `stream` (instead of a private one).  The train step maps each
    discriminator stream to the stream it was itself forked from: that stream idles during the discriminator updates, and a
    fork of a fork does not survive hipStreamEndCapture on ROCm 7.2."""
    _SIDE_STREAMS[stream.cuda_stream] = side


def _fork_side_stream():
    cur = torch.cuda.current_stream()
    key = cur.cuda_stream
    side = _SIDE_STREAMS.get(key)
    if side is None:
        side = _SIDE_STREAMS[key] = torch.cuda.Stream(device=cur.device)
    side.wait_stream(cur)
    _SIDE_DIRTY[key] = True
    return side


def join_side_stream() -> None:
    """Make the current stream wait for the weight-gradient work forked from it (no-op if there is none)."""
    if not torch.cuda.is_available():
        return
    cur = torch.cuda.current_stream()
    key = cur.cuda_stream
    if _SIDE_DIRTY.get(key):
        cur.wait_stream(_SIDE_STREAMS[key])
        _SIDE_DIRTY[key] = False


class ActHandoff:
    """Links a conv whose epilogue applied LeakyReLU (the producer) to the ONE conv that consumes its output: the consumer's
    data-gradient epilogue multiplies by LeakyReLU'(its input) -- which is the producer's activation backward -- and says so
    here, so the producer skips the separate activation-backward pass.  One object per forward call of the pair."""
    __slots__ = ("masked",)

    def __init__(self):
        self.masked = False


class _ConvFn(Function):
    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], kind: str, cache: Optional[dict], wdst, bdst, act: int = 0,
                handoff_out: Optional[ActHandoff] = None, handoff_in: Optional[ActHandoff] = None):
        x = _act(x, "conv input")
        w = _dev(weight.detach(), "conv weight")
        B, Cin, H, W = x.shape
        Cout, Cin_w, kh, kw = w.shape
        if Cin != Cin_w or kh != kw:
            raise L.AganError(f"conv: input has {Cin} channels, weight {tuple(w.shape)}")
        gf, pf, gd, pd, (OH, OW) = conv_geoms(kind, B, Cin, H, W, Cout, kh)
        pe = effective_precision(gf)
        x, odt = _gather_types(gf, pe, x, get_activation_storage())       # 16-bit activation storage where the layer offers it
        out = torch.empty((B, Cout, OH, OW), dtype=_TORCH_OF[odt], device=x.device)
        b = _dev(bias.detach(), "conv bias") if bias is not None else None
        # the amax slot of x: for the fp16-split gather, and for a weight gradient that runs on the fp16-split kernel (f16x3, bf16x6) --
        # taken HERE, where x still is the object its producer registered a slot for
        need_xs = pe == L.PREC_F16X3 or (ctx.needs_input_grad[1] and _needs_amax() and wgrad_effective_precision(gf, pf) == L.PREC_F16X3)
        xs = amax_of(x) if need_xs else None
        _gather(x, packed_weight(w, pf, cache, pe), b, gf, out, kind, "fwd", act, None, pe, xs)
        ctx.x_scale = xs
        if act == L.ACT_NONE:
            ctx.save_for_backward(x, w)
        else:                       # fused LeakyReLU: the backward needs the sign of the output
            ctx.save_for_backward(x, w, out)
        ctx.kind, ctx.has_bias, ctx.cache, ctx.wdst, ctx.bdst, ctx.act = kind, bias is not None, cache, wdst, bdst, act
        ctx.handoff_out = handoff_out if act != L.ACT_NONE else None
        # the consumer can fold the producer's LeakyReLU backward into its dgrad epilogue on the fp32 MFMA path (> 4 channels)
        ctx.handoff_in = handoff_in if (handoff_in is not None and Cin > 4) else None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy: Tensor):
        x, w = ctx.saved_tensors[:2]
        dy = _act(dy, "conv grad")
        if ctx.act != L.ACT_NONE:
            if ctx.handoff_out is not None and ctx.handoff_out.masked:
                ctx.handoff_out.masked = False          # the consumer's dgrad epilogue already applied LeakyReLU'(out)
            else:
                out = _dev(ctx.saved_tensors[2], "conv output")
                dy = _dev(dy, "conv grad")
                dz = torch.empty_like(dy)
                L.call("agan_act_bwd", _p(out), _p(dy), _p(dz), out.numel(), ctx.act, _stream())
                dy = dz
        B, Cin, H, W = x.shape
        Cout, _, kh, kw = w.shape
        gf, pf, gd, pd, _ = conv_geoms(ctx.kind, B, Cin, H, W, Cout, kh)
        dx = dw = db = None
        want_w, want_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        pe_d = effective_precision(gd) if ctx.needs_input_grad[0] else L.PREC_F32
        # weight gradient: the mode the library will run it in (the fp16 split needs its operands' amax slots only then)
        pe_w = wgrad_effective_precision(gf, pf)
        scaled_w = want_w and pe_w == L.PREC_F16X3
        dys = amax_of(dy) if (pe_d == L.PREC_F16X3 or scaled_w) else None      # ONE slot of dy serves both gradients
        side = None
        if _WGRAD_SIDE[0] and want_w and ctx.wdst is not None and (not want_b or ctx.bdst is not None):
            kt = ktable(gf, x.device)                  # (tables are built on the forking stream)
            side = _fork_side_stream()                 # dy is ready on the current stream at this point
            x.record_stream(side)
            dy.record_stream(side)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            if want_w:
                dwbuf, wacc, dw = _grad_out(ctx.wdst, w.shape, x)
                lib = L.load()
                nbytes = lib.agan_conv_wgrad_ws_bytes(byref(gf))
                ws, wsp = _ws(nbytes, x)
                kt = ktable(gf, x.device)
                obs = _OBSERVER[0]
                if obs is not None:
                    obs.begin(ctx.kind, "wgrad", gf, x.element_size(), dy.element_size())
                xs = None
                if scaled_w:
                    xs = ctx.x_scale if ctx.x_scale is not None else amax_of(x)
                xw, dyw = x, dy
                if (xw.dtype != torch.float32 or dyw.dtype != torch.float32) and not lib.agan_conv_wgrad_dt_supported(
                        byref(gf), pf, _PRECISION[0], _dt(xw), _dt(dyw)):
                    xw, dyw = xw.float(), dyw.float()         # a weight gradient without typed storage: widen its operands
                L.call("agan_conv_wgrad_dt", _p(xw), _p(dyw), _p(dwbuf), byref(gf), _p(kt), pf, kh, kw, pe_w, wacc, wsp, nbytes,
                       _stream(), _p(xs), _p(dys if scaled_w else None), _dt(xw), _dt(dyw))
                if obs is not None:
                    obs.end()
            if want_b:
                dbbuf, bacc, db = _grad_out(ctx.bdst, (Cout,), x)
                L.call("agan_bias_grad", _p(_dev(dy, "conv grad")), _p(dbbuf), B, Cout, dy.shape[2] * dy.shape[3], bacc, _stream())
        if ctx.needs_input_grad[0]:
            # dx takes x's storage type where the data-gradient kernel offers it (autograd wants the gradient in the input's dtype)
            dyg, ddt = _gather_types(gd, pe_d, dy, _dt(x))
            dx = torch.empty(x.shape, dtype=_TORCH_OF[ddt], device=x.device)
            mask = x if ctx.handoff_in is not None else None       # x is the producer's LeakyReLU output
            if mask is not None and mask.dtype != dx.dtype:
                mask = mask.to(dx.dtype)
            _gather(dyg, packed_weight(w, pd, ctx.cache, pe_d), None, gd, dx, ctx.kind, "dgrad", L.ACT_NONE, mask, pe_d,
                    dys if pe_d == L.PREC_F16X3 else None)
            if mask is not None:
                ctx.handoff_in.masked = True
        return dx, dw, db, None, None, None, None, None, None, None


# ---- the trainable general conv (include/agan.h: agan_conv2d_train_*): every (kernel, stride, padding) Layers.conv can return ----
_ANY_DESCS = {}


def conv_any_desc(B: int, Cin: int, H: int, W: int, Cout: int, k, stride, padding):
    """-> (descriptor, observer geometry, workspace bytes of forward / data gradient / weight gradient) of a general conv, cached
    like conv_geoms.  Raises outside the library's domain (K 1..5, stride 1..3, padding 0..3 per axis): there is no fallback."""
    key = (B, Cin, H, W, Cout, tuple(k), tuple(stride), tuple(padding))
    hit = _ANY_DESCS.get(key)
    if hit is not None:
        return hit
    (kh, kw), (sh, sw), (ph, pw) = k, stride, padding
    oh, ow = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
    d = L.Conv2dDesc(B, Cin, H, W, Cout, oh, ow, kh, kw, sh, sw, ph, pw, 0, Cin, 0, Cout)
    lib = L.load()
    if not lib.agan_conv2d_train_supported(byref(d)):
        raise L.AganError(f"conv k={k} s={stride} p={padding} on {Cin}x{H}x{W}: {lib.agan_last_error().decode()}")
    g = _geom(B, Cin, H, W, Cout, oh, ow, kh, kw, 1, sh, 1, (-ph, -pw))       # what a launch observer is shown
    hit = _ANY_DESCS[key] = (d, g, tuple(lib.agan_conv2d_train_ws_bytes(byref(d), i) for i in range(3)))
    return hit


class _ConvAnyFn(Function):
    """conv2d(kind="any"): forward, data gradient and weight gradient on the general fp32 MFMA engine (csrc/conv_any.hip).

    fp32 products and fp32 tensors in every precision mode.  Under 16-bit activation storage this conv READS AND WRITES fp32: a
    16-bit input (or incoming gradient) is widened on the way in (_dev), the output and the input gradient are fp32 -- autograd
    casts the latter back to the input's type."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], stride, padding, wdst, bdst):
        ctx.x_dtype = x.dtype
        x = _dev(x, "conv input")
        w = _dev(weight.detach(), "conv weight")
        B, Cin, H, W = x.shape
        Cout, Cin_w, kh, kw = w.shape
        if Cin != Cin_w:
            raise L.AganError(f"conv: input has {Cin} channels, weight {tuple(w.shape)}")
        d, g, nbytes = conv_any_desc(B, Cin, H, W, Cout, (kh, kw), stride, padding)
        b = _dev(bias.detach(), "conv bias") if bias is not None else None
        out = torch.empty((B, Cout, d.OH, d.OW), dtype=torch.float32, device=x.device)
        ws, wsp = _ws(nbytes[0], x)
        obs = _OBSERVER[0]
        if obs is not None:
            obs.begin("any", "fwd", g, 4, 4)
        L.call("agan_conv2d_train_fwd", _p(x), _p(w), _p(b), _p(out), byref(d), wsp, nbytes[0], _stream())
        if obs is not None:
            obs.end()
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.padding, ctx.has_bias, ctx.wdst, ctx.bdst = stride, padding, bias is not None, wdst, bdst
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy: Tensor):
        x, w = ctx.saved_tensors
        dy = _dev(dy, "conv grad")
        B, Cin, H, W = x.shape
        Cout, _, kh, kw = w.shape
        d, g, nbytes = conv_any_desc(B, Cin, H, W, Cout, (kh, kw), ctx.stride, ctx.padding)
        dx = dw = db = None
        want_w, want_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        obs = _OBSERVER[0]
        side = None
        if _WGRAD_SIDE[0] and want_w and ctx.wdst is not None and (not want_b or ctx.bdst is not None):
            side = _fork_side_stream()                 # dy is ready on the current stream at this point
            x.record_stream(side)
            dy.record_stream(side)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            if want_w:
                dwbuf, wacc, dw = _grad_out(ctx.wdst, w.shape, x)
                ws, wsp = _ws(nbytes[2], x)
                if obs is not None:
                    obs.begin("any", "wgrad", g, 4, 4)
                L.call("agan_conv2d_train_wgrad", _p(x), _p(dy), _p(dwbuf), byref(d), wacc, wsp, nbytes[2], _stream())
                if obs is not None:
                    obs.end()
            if want_b:
                dbbuf, bacc, db = _grad_out(ctx.bdst, (Cout,), x)
                L.call("agan_bias_grad", _p(dy), _p(dbbuf), B, Cout, dy.shape[2] * dy.shape[3], bacc, _stream())
        if ctx.needs_input_grad[0]:
            dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            ws, wsp = _ws(nbytes[1], x)
            if obs is not None:
                obs.begin("any", "dgrad", g, 4, 4)
            L.call("agan_conv2d_train_dgrad", _p(dy), _p(w), _p(dx), byref(d), 0, wsp, nbytes[1], _stream())
            if obs is not None:
                obs.end()
            if ctx.x_dtype != torch.float32:
                dx = dx.to(ctx.x_dtype)
        return dx, dw, db, None, None, None, None


def conv_fuses_activation(act: int, cout: int, kind: Optional[str] = None) -> bool:
    """can conv2d apply `act` in its epilogue? (LeakyReLU on the MFMA paths; include/agan.h: agan_conv_gather).  Never for a conv
    of kind "any": the general engine has no activation epilogue."""
    return act == L.ACT_LRELU and cout > 4 and kind != "any"


def conv2d(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, kind: str = "same", cache: Optional[dict] = None,
           wdst=None, bdst=None, act: int = 0, handoff_out: Optional[ActHandoff] = None,
           handoff_in: Optional[ActHandoff] = None, stride=(1, 1), padding=(0, 0)) -> Tensor:
    """conv forward with autograd (dgrad + wgrad kernels).  kind: 'same' | 'down' | 'up' (conv_geoms) or 'any'.
    wdst / bdst: optional flat-gradient destinations of weight / bias (grad_dst(param)).
    act: ACT_LRELU applies the activation in the conv epilogue (see conv_fuses_activation).
    handoff_out / handoff_in: one ActHandoff shared by a fused conv+LeakyReLU and the single conv consuming its output.
    kind 'any': the general trainable conv with the module's `stride` and `padding` (pairs); per axis kernel 1..5, stride 1..3,
    padding 0..3.  fp32 products in every precision mode; under 16-bit activation storage it reads and writes fp32, casting on the
    way in.  No fused activation and no handoff."""
    if kind == "any":
        if act != L.ACT_NONE or handoff_out is not None:
            raise L.AganError("conv2d(kind='any') has no fused activation: run HF.activation / HF.bn_act after it")
        return _ConvAnyFn.apply(x, weight, bias, tuple(stride), tuple(padding), wdst, bdst)
    return _ConvFn.apply(x, weight, bias, kind, cache, wdst, bdst, act, handoff_out, handoff_in)


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, cache: Optional[dict] = None, wdst=None, bdst=None) -> Tensor:
    """nn.Linear as a 1x1 conv on a 1x1 image (generator_submodules.py:36,152)."""
    B, Cin = x.shape
    y = _ConvFn.apply(x.reshape(B, Cin, 1, 1), weight.view(weight.shape[0], Cin, 1, 1), bias, "same", cache, wdst, bdst)
    return y.view(B, weight.shape[0])


# --------------------------------------------------------------------------------------------------------------
# BatchNorm (train mode) + activation
# --------------------------------------------------------------------------------------------------------------
# Batch groups: a discriminator update runs the real and the fake batch through the same weights.  The reference does two
# forward passes (disc_loss.py:55-61), so every BatchNorm sees each batch on its own: batch statistics per pass, two running-
# statistic updates in call order.  `with bn_groups(2)` lets one pass over the concatenated [real; fake] batch reproduce that:
# each BatchNorm call treats the batch axis as `groups` consecutive sub-batches (include/agan.h: agan_bn_train_fwd): statistics,
# running-stat update and normalisation per sub-batch in order; the backward sums gamma/beta gradients over the groups.  The
# convolutions in between simply see twice the pixels -- half the launches, better-filled tiles on the deep 4x4..16x16 layers.
_BN_GROUPS = [1]


@contextlib.contextmanager
def bn_groups(groups: int):
    old = _BN_GROUPS[0]
    _BN_GROUPS[0] = int(groups)
    try:
        yield
    finally:
        _BN_GROUPS[0] = old


class _BnActFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, nbt, training, act, eps, momentum, gdst, bdst, groups):
        x = _act(x, "bn input")
        shape = x.shape
        B, C = shape[0], shape[1]
        HW = x.numel() // (B * C)
        if not training:
            groups = 1
        if B % groups:
            raise L.AganError(f"BatchNorm: batch {B} does not split into {groups} groups")
        Bg = B // groups
        g, b = _dev(gamma.detach(), "bn weight"), _dev(beta.detach(), "bn bias")
        lib = L.load()
        co = C // 2 if act == L.ACT_GLU else C
        # storage types (include/agan.h: agan_bn_*_dt): the output takes the activation storage in force (4-D tensors only); a 16-bit
        # input is read as it stands when the output has the same type, else widened
        odt = get_activation_storage() if HW > 1 else L.DT_F32
        if x.dtype != torch.float32 and _dt(x) != odt:
            x = x.float()
        xdt = _dt(x)
        out = torch.empty((B, co) + tuple(shape[2:]), dtype=_TORCH_OF[odt], device=x.device)
        res = _act(residual, "bn residual") if residual is not None else None
        if res is not None and res.dtype != out.dtype:
            res = res.to(out.dtype)
        if training:
            mean = torch.empty((groups, C), dtype=torch.float32, device=x.device)
            invstd = torch.empty_like(mean)
            nbytes = lib.agan_bn_train_fwd_ws_bytes(Bg, C, HW)
            ws, wsp = _ws(nbytes, x)
            L.call("agan_bn_train_fwd_dt", _p(x), _p(g), _p(b), _p(res), _p(out), _p(mean), _p(invstd), _p(running_mean),
                   _p(running_var), _p(nbt), B, C, HW, float(eps), float(momentum), act, groups, wsp, nbytes, _stream(),
                   _p(_amax_out(out)), xdt, odt)
        else:
            mean = running_mean
            invstd = torch.rsqrt(running_var + eps)
            L.call("agan_bn_act_fwd_dt", _p(x), _p(mean), _p(invstd), _p(g), _p(b), _p(res), _p(out), B, C, HW, act, _stream(),
                   _p(_amax_out(out)), xdt, odt)
        ctx.save_for_backward(x, g, b, mean, invstd)
        ctx.odt = odt
        ctx.act, ctx.training, ctx.has_res, ctx.gdst, ctx.bdst, ctx.groups = act, training, residual is not None, gdst, bdst, groups
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        if not ctx.training:
            raise L.AganError("BatchNorm backward in eval mode is not on the training path")
        x, g, b, mean, invstd = ctx.saved_tensors
        dout = _act(dout, "bn grad")
        if _dt(dout) != ctx.odt:                     # (autograd delivers the output's dtype; a hand-made gradient may not)
            dout = dout.to(_TORCH_OF[ctx.odt])
        B, C = x.shape[0], x.shape[1]
        HW = x.numel() // (B * C)
        groups = ctx.groups
        Bg = B // groups
        dx = torch.empty_like(x)
        # frozen affine parameters (a discriminator inside the generator update): the sums are still needed for dx, but they go
        # to scratch, not into the owner's flat gradient buffer
        dgbuf, gacc, dg = _grad_out(ctx.gdst if ctx.needs_input_grad[1] else None, g.shape, x)
        dbbuf, bacc, db = _grad_out(ctx.bdst if ctx.needs_input_grad[2] else None, b.shape, x)
        if gacc != bacc:
            raise L.AganError("BatchNorm weight/bias gradient destinations out of step")
        nbytes = L.load().agan_bn_act_bwd_ws_bytes(Bg, C, HW)
        ws, wsp = _ws(nbytes, x)
        L.call("agan_bn_act_bwd_dt", _p(x), _p(dout), _p(mean), _p(invstd), _p(g), _p(b), _p(dx), _p(dgbuf), _p(dbbuf), B, C, HW,
               ctx.act, gacc, groups, wsp, nbytes, _stream(), _p(_amax_out(dx)), _dt(x), ctx.odt)
        dres = dout if ctx.has_res else None
        return dx, dg, db, dres, None, None, None, None, None, None, None, None, None, None


def bn_act(x, gamma, beta, running_mean, running_var, nbt, training: bool, act: int, residual=None,
           eps: float = 1e-5, momentum: float = 0.1) -> Tensor:
    """Train-mode BatchNorm + activation (+ residual).  Inside `with bn_groups(G)` the batch axis is G consecutive sub-batches,
    each normalised with its own statistics (see bn_groups above)."""
    return _BnActFn.apply(x, gamma, beta, residual, running_mean, running_var, nbt, training, act, eps, momentum,
                          grad_dst(gamma), grad_dst(beta), _BN_GROUPS[0])


# --------------------------------------------------------------------------------------------------------------
# sentence-conditioned BatchNorm (utilities/layers.py: HipCondBatchNorm2d; include/agan.h: agan_cbn_*)
# --------------------------------------------------------------------------------------------------------------
def _cond_bn_dims(x: Tensor, gamma: Tensor, delta: Tensor, act: int, what: str) -> Tuple[int, int, int]:
    """-> (B, C, HW) of x [B, C, ...] with gamma [C] and delta [B, 2C], or ValueError"""
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"{what}: the input must be [B, C, ...] and not empty, got {tuple(x.shape)}")
    B, C = int(x.shape[0]), int(x.shape[1])
    if act not in (L.ACT_NONE, L.ACT_GLU):
        raise ValueError(f"{what}: activation {act}; the conditional BatchNorm takes ACT_NONE or ACT_GLU")
    if act == L.ACT_GLU and C % 2:
        raise ValueError(f"{what}: GLU needs an even channel count, got {C}")
    if tuple(gamma.shape) != (C,):
        raise ValueError(f"{what}: the weight must be [{C}], got {tuple(gamma.shape)}")
    if tuple(delta.shape) != (B, 2 * C):
        raise ValueError(f"{what}: delta must be [B, 2C] = [{B}, {2 * C}], got {tuple(delta.shape)}")
    return B, C, x.numel() // (B * C)


def cond_bn_act_reference(x: Tensor, gamma: Tensor, beta: Tensor, delta: Tensor, running_mean: Optional[Tensor],
                          running_var: Optional[Tensor], training: bool, act: int, eps: float = 1e-5, momentum: float = 0.1):
    """What cond_bn_act computes, in torch ops, in x's dtype, on any device, differentiable by autograd:

        xhat = (x - mean[c]) / sqrt(var[c] + eps)       batch statistics over (b, p) with the biased variance when `training`,
                                                        else the running statistics
        z = (gamma[c] + delta[b, c]) * xhat + (beta[c] + delta[b, C + c])        out = z (ACT_NONE) or GLU over channel halves

    -> (out, running_mean, running_var): the running statistics after the momentum update with the unbiased variance (the inputs
    themselves, untouched, in eval mode or when they are None)."""
    B, C, HW = _cond_bn_dims(x, gamma, delta, act, "cond_bn_act_reference")
    xs = x.reshape(B, C, HW)
    if training:
        mean = xs.mean(dim=(0, 2))
        var = ((xs - mean.view(1, C, 1)) ** 2).mean(dim=(0, 2))
        if running_mean is not None:
            n = B * HW
            unbiased = var.detach() * (n / (n - 1)) if n > 1 else var.detach()
            running_mean = (1 - momentum) * running_mean + momentum * mean.detach()
            running_var = (1 - momentum) * running_var + momentum * unbiased
    else:
        mean, var = running_mean, running_var
    xhat = (xs - mean.view(1, C, 1)) * torch.rsqrt(var.view(1, C, 1) + eps)
    z = (gamma.view(1, C) + delta[:, :C]).unsqueeze(2) * xhat + (beta.view(1, C) + delta[:, C:]).unsqueeze(2)
    if act == L.ACT_GLU:
        z = z[:, :C // 2] * torch.sigmoid(z[:, C // 2:])
    return z.reshape((B, z.shape[1]) + tuple(x.shape[2:])), running_mean, running_var


class _CondBnActFn(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, delta, running_mean, running_var, nbt, training, act, eps, momentum, gdst, bdst):
        shape = x.shape
        B, C = shape[0], shape[1]
        HW = x.numel() // (B * C)
        g, b = _dev(gamma.detach(), "cond bn weight"), _dev(beta.detach(), "cond bn bias")
        lib = L.load()
        co = C // 2 if act == L.ACT_GLU else C
        out = torch.empty((B, co) + tuple(shape[2:]), dtype=torch.float32, device=x.device)
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=x.device)
            invstd = torch.empty_like(mean)
            nbytes = lib.agan_cbn_train_fwd_ws_bytes(B, C, HW)
            ws, wsp = _ws(nbytes, x)
            L.call("agan_cbn_train_fwd", _p(x), _p(g), _p(b), _p(delta), _p(out), _p(mean), _p(invstd), _p(running_mean),
                   _p(running_var), _p(nbt), B, C, HW, float(eps), float(momentum), act, wsp, nbytes, _stream(), _p(_amax_out(out)))
        else:
            mean = running_mean
            invstd = torch.rsqrt(running_var + eps)
            L.call("agan_cbn_act_fwd", _p(x), _p(mean), _p(invstd), _p(g), _p(b), _p(delta), _p(out), B, C, HW, act, _stream(),
                   _p(_amax_out(out)))
        ctx.save_for_backward(x, g, b, delta, mean, invstd)
        ctx.act, ctx.training, ctx.gdst, ctx.bdst = act, training, gdst, bdst
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        if not ctx.training:
            raise L.AganError("BatchNorm backward in eval mode is not on the training path")
        x, g, b, delta, mean, invstd = ctx.saved_tensors
        dout = _dev(dout, "cond bn grad")
        B, C = x.shape[0], x.shape[1]
        HW = x.numel() // (B * C)
        dx = torch.empty_like(x)
        ddelta = torch.empty_like(delta)
        # (frozen affine parameters: the sums go to scratch, as in _BnActFn)
        dgbuf, gacc, dg = _grad_out(ctx.gdst if ctx.needs_input_grad[1] else None, g.shape, x)
        dbbuf, bacc, db = _grad_out(ctx.bdst if ctx.needs_input_grad[2] else None, b.shape, x)
        if gacc != bacc:
            raise L.AganError("BatchNorm weight/bias gradient destinations out of step")
        nbytes = L.load().agan_cbn_act_bwd_ws_bytes(B, C, HW)
        ws, wsp = _ws(nbytes, x)
        L.call("agan_cbn_act_bwd", _p(x), _p(dout), _p(mean), _p(invstd), _p(g), _p(b), _p(delta), _p(dx), _p(ddelta), _p(dgbuf),
               _p(dbbuf), B, C, HW, ctx.act, gacc, wsp, nbytes, _stream(), _p(_amax_out(dx)))
        return dx, dg, db, ddelta, None, None, None, None, None, None, None, None, None


def cond_bn_act(x, gamma, beta, delta, running_mean, running_var, nbt, training: bool, act: int, eps: float = 1e-5,
                momentum: float = 0.1) -> Tensor:
    """Sentence-conditioned BatchNorm + activation on the HIP kernels (csrc/cond_bn.hip), fp32, with autograd: train-mode BatchNorm
    of x [B, C, ...] whose affine terms are gamma[c] + delta[b, c] and beta[c] + delta[b, C + c], then ACT_NONE or ACT_GLU
    (cond_bn_act_reference states it in torch ops).  delta is a contiguous fp32 [B, 2C] device tensor and receives its gradient
    from autograd; the gamma / beta gradients go to the parameters' flat-gradient slices like bn_act's.  In eval mode the forward
    uses the running statistics and a backward raises.  Not built: `bn_groups` other than 1 and 16-bit activation storage."""
    B, C, HW = _cond_bn_dims(x, gamma, delta, act, "cond_bn_act")
    if _BN_GROUPS[0] != 1:
        raise L.AganError(f"cond_bn_act: bn_groups({_BN_GROUPS[0]}) is in force; the conditional BatchNorm normalises the batch as one group")
    _fp32_only("cond_bn_act", "conditional BatchNorm", x)
    if not delta.is_cuda or delta.dtype != torch.float32 or not delta.is_contiguous():
        raise L.AganError(f"cond_bn_act: delta must be a contiguous float32 [B, 2C] device tensor, got {delta.dtype} on {delta.device}"
                          f"{'' if delta.is_contiguous() else ', not contiguous'}")
    x = _dev(x, "cond bn input")
    return _CondBnActFn.apply(x, gamma, beta, delta, running_mean, running_var, nbt, training, act, eps, momentum,
                              grad_dst(gamma), grad_dst(beta))


# --------------------------------------------------------------------------------------------------------------
# self-attention over the positions of a feature map and the block's gate (utilities/layers.py: SelfAttention2d;
# include/agan.h: agan_self_attn_*, agan_scaled_residual_*)
# --------------------------------------------------------------------------------------------------------------
def _self_attn_dims(q: Tensor, k: Tensor, v: Tensor, what: str) -> Tuple[int, int, int, int, int]:
    """-> (B, N, M, Dk, Dv) of q [B, Dk, N...], k [B, Dk, M...], v [B, Dv, M...], or ValueError"""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() < 3 or t.numel() == 0:
            raise ValueError(f"{what}: {name} must be [B, channels, positions...] and not empty, got {tuple(t.shape)}")
    B, Dk, Dv = int(q.shape[0]), int(q.shape[1]), int(v.shape[1])
    N, M = q.numel() // (B * Dk), v.numel() // (int(v.shape[0]) * Dv)
    if int(k.shape[0]) != B or int(v.shape[0]) != B or int(k.shape[1]) != Dk or k.numel() != B * Dk * M:
        raise ValueError(f"{what}: q {tuple(q.shape)}, k {tuple(k.shape)} and v {tuple(v.shape)} do not fit "
                         f"([B, Dk, N], [B, Dk, M], [B, Dv, M])")
    return B, N, M, Dk, Dv


def self_attention_reference(q: Tensor, k: Tensor, v: Tensor, scale: float = 1.0) -> Tensor:
    """What self_attention computes, in torch ops, in q's dtype, on any device, differentiable by autograd:

        s[b, n, m] = scale * sum_d q[b, d, n] k[b, d, m]      p = softmax over m      o[b, e, n] = sum_m v[b, e, m] p[b, n, m]

    q [B, Dk, N...], k [B, Dk, M...], v [B, Dv, M...] -> o [B, Dv, N...]."""
    B, N, M, Dk, Dv = _self_attn_dims(q, k, v, "self_attention_reference")
    s = scale * torch.bmm(q.reshape(B, Dk, N).transpose(1, 2), k.reshape(B, Dk, M))
    o = torch.bmm(v.reshape(B, Dv, M), torch.softmax(s, dim=2).transpose(1, 2))
    return o.reshape((B, Dv) + tuple(q.shape[2:]))


def _at(t: Tensor, elems: int) -> c_void_p:
    return c_void_p(t.data_ptr() + 4 * elems)


def _self_attn_fwd(q, k, v, o, lse, dims, strides, scale) -> None:
    B, N, M, Dk, Dv = dims
    L.call("agan_self_attn_fwd", q, k, v, _p(o), _p(lse), B, N, M, Dk, Dv, *strides, Dv * N, float(scale), _stream())


def _self_attn_bwd(q, k, v, o, lse, dout, dq, dk, dv, dims, strides, dstrides, scale) -> None:
    B, N, M, Dk, Dv = dims
    nbytes = L.load().agan_self_attn_bwd_ws_bytes(B, N, M, Dk, Dv)
    ws, wsp = _ws(nbytes, o)
    L.call("agan_self_attn_bwd", q, k, v, _p(o), _p(lse), _p(dout), dq, dk, dv, B, N, M, Dk, Dv, *strides, Dv * N, Dv * N, *dstrides,
           float(scale), wsp, nbytes, _stream())


class _SelfAttnFn(Function):
    @staticmethod
    def forward(ctx, q, k, v, scale):
        dims = B, N, M, Dk, Dv = _self_attn_dims(q, k, v, "self_attention")
        o = torch.empty((B, Dv) + tuple(q.shape[2:]), dtype=torch.float32, device=q.device)
        lse = torch.empty((B, N), dtype=torch.float32, device=q.device)
        _self_attn_fwd(_p(q), _p(k), _p(v), o, lse, dims, (Dk * N, Dk * M, Dv * M), scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.dims, ctx.scale = dims, scale
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        B, N, M, Dk, Dv = ctx.dims
        dout = _dev(dout, "self-attention grad")
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        strides = (Dk * N, Dk * M, Dv * M)
        _self_attn_bwd(_p(q), _p(k), _p(v), o, lse, dout, _p(dq), _p(dk), _p(dv), ctx.dims, strides, strides, ctx.scale)
        return dq, dk, dv, None


class _SelfAttnQkvFn(Function):
    """q, k, v are the channel ranges [0, dk), [dk, 2 dk), [2 dk, 2 dk + dv) of one tensor; so are dq, dk, dv of its gradient"""

    @staticmethod
    def forward(ctx, qkv, dk, dv, scale):
        B, C = int(qkv.shape[0]), int(qkv.shape[1])
        N = qkv.numel() // (B * C)
        dims = (B, N, N, dk, dv)
        o = torch.empty((B, dv) + tuple(qkv.shape[2:]), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((B, N), dtype=torch.float32, device=qkv.device)
        _self_attn_fwd(_at(qkv, 0), _at(qkv, dk * N), _at(qkv, 2 * dk * N), o, lse, dims, (C * N,) * 3, scale)
        ctx.save_for_backward(qkv, o, lse)
        ctx.dims, ctx.scale = dims, scale
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, o, lse = ctx.saved_tensors
        B, N, _, dk, dv = ctx.dims
        C = 2 * dk + dv
        dout = _dev(dout, "self-attention grad")
        dqkv = torch.empty_like(qkv)
        strides = (C * N,) * 3
        _self_attn_bwd(_at(qkv, 0), _at(qkv, dk * N), _at(qkv, 2 * dk * N), o, lse, dout, _at(dqkv, 0), _at(dqkv, dk * N),
                       _at(dqkv, 2 * dk * N), ctx.dims, strides, strides, ctx.scale)
        return dqkv, None, None, None


def self_attention(q: Tensor, k: Tensor, v: Tensor, scale: float = 1.0) -> Tensor:
    """Attention of every query position over every key position on the HIP kernels (csrc/self_attn.hip), fp32, with autograd;
    self_attention_reference states it in torch ops.  q [B, Dk, N...], k [B, Dk, M...], v [B, Dv, M...] -> o [B, Dv, N...] with
    Dk <= 64 and Dv <= 128.  Nothing of size N x M is allocated in either direction: the backward keeps q, k, v, o and one
    log-sum-exp per query and recomputes the probabilities."""
    _self_attn_dims(q, k, v, "self_attention")
    _fp32_only("self_attention", "self-attention", q, k, v)
    return _SelfAttnFn.apply(_dev(q, "self-attention q"), _dev(k, "self-attention k"), _dev(v, "self-attention v"), float(scale))


def self_attention_qkv(qkv: Tensor, dk: int, dv: int, scale: float = 1.0) -> Tensor:
    """self_attention(q, k, v) with q, k, v = qkv[:, :dk], qkv[:, dk:2 dk], qkv[:, 2 dk:] of one conv output [B, 2 dk + dv, H, W],
    passed to the kernels by stride: no slice is copied, and the backward returns ONE gradient tensor of qkv's shape that the kernels
    wrote in place (no cat)."""
    if qkv.dim() < 3 or qkv.numel() == 0 or dk < 1 or dv < 1 or int(qkv.shape[1]) != 2 * dk + dv:
        raise ValueError(f"self_attention_qkv: qkv must be [B, 2 dk + dv = {2 * dk + dv}, positions...], got {tuple(qkv.shape)}")
    _fp32_only("self_attention_qkv", "self-attention", qkv)
    return _SelfAttnQkvFn.apply(_dev(qkv, "self-attention qkv"), int(dk), int(dv), float(scale))


def scaled_residual_reference(x: Tensor, y: Tensor, g: Tensor) -> Tensor:
    """What scaled_residual computes, in torch ops: x + g * y with the one-element gate g."""
    return x + g * y


class _ScaledResidualFn(Function):
    @staticmethod
    def forward(ctx, x, y, g, gdst):
        gd = _dev(g.detach(), "scaled_residual gate")
        out = torch.empty_like(x)
        L.call("agan_scaled_residual_fwd", _p(x), _p(y), _p(gd), _p(out), x.numel(), _stream())
        ctx.save_for_backward(y, gd)
        ctx.gdst = gdst
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        y, g = ctx.saved_tensors
        dout = _dev(dout, "scaled_residual grad")
        dy = torch.empty_like(y)
        dgbuf, gacc, dg = _grad_out(ctx.gdst if ctx.needs_input_grad[2] else None, g.shape, y)
        n = y.numel()
        nbytes = L.load().agan_scaled_residual_bwd_ws_bytes(n)
        ws, wsp = _ws(nbytes, y)
        L.call("agan_scaled_residual_bwd", _p(dout), _p(y), _p(g), _p(dy), _p(dgbuf), n, gacc, wsp, nbytes, _stream())
        return dout, dy, dg, None


def scaled_residual(x: Tensor, y: Tensor, g: Tensor) -> Tensor:
    """x + g[0] * y on the HIP kernels with autograd: the gate g (one element) is read on the device, its gradient sum(dout * y)
    goes to the parameter's flat-gradient slice like bn_act's gamma, and the gradient at x is dout itself."""
    if x.shape != y.shape or x.numel() == 0 or g.numel() != 1:
        raise ValueError(f"scaled_residual: x {tuple(x.shape)} and y {tuple(y.shape)} must agree and g must hold one element, "
                         f"got {tuple(g.shape)}")
    _fp32_only("scaled_residual", "self-attention", x, y)
    return _ScaledResidualFn.apply(_dev(x, "scaled_residual x"), _dev(y, "scaled_residual y"), g, grad_dst(g))


class _ActFn(Function):
    @staticmethod
    def forward(ctx, x, act):
        x = _dev(x, "activation input")
        out = torch.empty_like(x)
        L.call("agan_act_fwd", _p(x), _p(out), x.numel(), act, _stream())
        ctx.save_for_backward(out)
        ctx.act = act
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (out,) = ctx.saved_tensors
        dout = _dev(dout, "activation grad")
        dx = torch.empty_like(out)
        L.call("agan_act_bwd", _p(out), _p(dout), _p(dx), out.numel(), ctx.act, _stream())
        return dx, None


def activation(x: Tensor, act: int) -> Tensor:
    return _ActFn.apply(x, act)


class _GluFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = _dev(x, "GLU input")
        B, C = x.shape[0], x.shape[1]
        if C % 2:
            raise AssertionError("channels dont divide 2!")      # utilities/layers.py:22
        HW = x.numel() // (B * C)
        out = torch.empty((B, C // 2) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        L.call("agan_glu_fwd", _p(x), _p(out), B, C, HW, _stream())
        ctx.save_for_backward(x)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        dout = _dev(dout, "GLU grad")
        B, C = x.shape[0], x.shape[1]
        dx = torch.empty_like(x)
        L.call("agan_glu_bwd", _p(x), _p(dout), _p(dx), B, C, x.numel() // (B * C), _stream())
        return dx


def glu(x: Tensor) -> Tensor:
    return _GluFn.apply(x)


# --------------------------------------------------------------------------------------------------------------
# word-context attention (networks/attention.py:25-79)
# --------------------------------------------------------------------------------------------------------------
class _AttentionFn(Function):
    @staticmethod
    def forward(ctx, images, words, weight, mask, scale, wdst):
        # images / context / their gradients keep the activation storage in force (typed kernels: agan_attn_*_dt); words, the
        # projection and the attention map stay fp32
        images, words = _act(images, "attention images"), _dev(words, "attention words")
        if images.dtype != torch.float32 and _dt(images) != get_activation_storage():
            images = images.float()
        w = _dev(weight.detach(), "attention conv1 weight")
        B, C, H, W = images.shape
        Bw, E, T = words.shape
        if Bw != B or tuple(mask.shape) != (B, T):
            raise ValueError(f"attention: images {tuple(images.shape)}, words {tuple(words.shape)}, mask {tuple(mask.shape)}")
        m = mask.to(device=images.device, dtype=torch.int64).contiguous()
        proj = torch.empty((B, C, T), dtype=torch.float32, device=images.device)
        ctxt = torch.empty_like(images)
        attn = torch.empty((B, T, H, W), dtype=torch.float32, device=images.device)
        L.call("agan_attn_fwd_dt", _p(images), _p(words), _p(w), _p(m), float(scale), _p(proj), _p(ctxt), _p(attn),
               B, C, E, T, H * W, _stream(), _dt(images))
        ctx.save_for_backward(images, words, w, proj, attn)
        ctx.scale, ctx.wdst = float(scale), wdst
        ctx.set_materialize_grads(False)     # the attention map usually feeds nothing: no zero-filled 16 MB gradient for it
        return ctxt, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, dctx, dattn):
        images, words, w, proj, attn = ctx.saved_tensors
        B, C, H, W = images.shape
        _, E, T = words.shape
        if dctx is not None:
            dctx = _act(dctx, "attention dctx")
            if dctx.dtype != images.dtype:
                dctx = dctx.to(images.dtype)
        dattn = _dev(dattn, "attention dattn") if dattn is not None else None
        dimages, dwords = torch.empty_like(images), torch.empty_like(words)
        # a frozen projection (requires_grad False) still needs d(proj) for nothing: its gradient goes to scratch, not into the
        # owner's flat buffer (as the conv and BatchNorm paths do)
        dwbuf, wacc, dw = _grad_out(ctx.wdst if ctx.needs_input_grad[2] else None, w.shape, images)
        if not ctx.needs_input_grad[2]:
            dw = None
        nbytes = L.load().agan_attn_bwd_ws_bytes(B, C, T, H * W)
        ws, wsp = _ws(nbytes, images)
        L.call("agan_attn_bwd_dt", _p(images), _p(words), _p(w), _p(proj), _p(attn), _p(dctx), _p(dattn), ctx.scale,
               _p(dimages), _p(dwords), _p(dwbuf), B, C, E, T, H * W, wacc, wsp, nbytes, _stream(), _dt(images))
        return dimages, dwords, dw, None, None, None


def attention(images: Tensor, words: Tensor, conv1_weight: Tensor, mask: Tensor, scaled: bool = True):
    C = images.shape[1]
    scale = 1.0 / math.sqrt(C) if scaled else 1.0
    return _AttentionFn.apply(images, words, conv1_weight, mask, scale, grad_dst(conv1_weight))


# --------------------------------------------------------------------------------------------------------------
# dynamic memory of a refinement stage (networks/memory.py: DynamicMemory; include/agan.h: agan_mem_write_*, agan_mem_read_*)
# --------------------------------------------------------------------------------------------------------------
def _mem_write_dims(U: Tensor, Q: Tensor, what: str) -> Tuple[int, int, int]:
    """-> (B, T, Md) of U [B, T, Md + 1] and Q [B, Md + 1], or ValueError"""
    if U.dim() != 3 or Q.dim() != 2 or U.numel() == 0 or U.shape[2] < 2 or tuple(Q.shape) != (U.shape[0], U.shape[2]):
        raise ValueError(f"{what}: U must be [B, T, memory_dim + 1] and Q [B, memory_dim + 1], got {tuple(U.shape)} and {tuple(Q.shape)}")
    return int(U.shape[0]), int(U.shape[1]), int(U.shape[2]) - 1


def _mem_read_dims(h: Tensor, kv: Tensor, mask: Tensor, rw: Tensor, rb: Tensor, what: str) -> Tuple[int, int, int, int, int]:
    """-> (B, C, T, H, W) of h [B, C, H, W], kv [B, T, 2C], mask [B, T], rw (2C elements) and rb (1 element), or ValueError"""
    if h.dim() != 4 or kv.dim() != 3 or h.numel() == 0 or kv.numel() == 0:
        raise ValueError(f"{what}: h must be [B, C, H, W] and kv [B, T, 2C], got {tuple(h.shape)} and {tuple(kv.shape)}")
    B, C, H, W = (int(s) for s in h.shape)
    T = int(kv.shape[1])
    if int(kv.shape[0]) != B or int(kv.shape[2]) != 2 * C or tuple(mask.shape) != (B, T) or rw.numel() != 2 * C or rb.numel() != 1:
        raise ValueError(f"{what}: h {tuple(h.shape)}, kv {tuple(kv.shape)}, mask {tuple(mask.shape)}, response weight {tuple(rw.shape)} "
                         f"and bias {tuple(rb.shape)} do not fit ([B, C, H, W], [B, T, 2C], [B, T], 2C, 1)")
    return B, C, T, H, W


def memory_write_reference(U: Tensor, Q: Tensor) -> Tensor:
    """What memory_write computes, in torch ops, in U's dtype, on any device, differentiable by autograd:

        g = sigmoid(U[b, t, Md] + Q[b, Md])        m[b, t, d] = relu(U[b, t, d]) g + relu(Q[b, d]) (1 - g)

    U [B, T, Md + 1], Q [B, Md + 1] -> m [B, T, Md]."""
    _, _, Md = _mem_write_dims(U, Q, "memory_write_reference")
    g = torch.sigmoid(U[:, :, Md:] + Q[:, None, Md:])
    return torch.relu(U[:, :, :Md]) * g + torch.relu(Q[:, None, :Md]) * (1 - g)


def memory_read_reference(h: Tensor, kv: Tensor, mask: Tensor, rw: Tensor, rb: Tensor) -> Tuple[Tensor, Tensor]:
    """What memory_read computes, in torch ops, in h's dtype, on any device, differentiable by autograd.  With k = kv[:, :, :C],
    v = kv[:, :, C:] and p a pixel:

        s[t] = sum_c k[b, t, c] h[b, c, p], -inf where mask[b, t] == 0      attn = softmax_t s      o[c] = sum_t v[b, t, c] attn[t]
        z = sum_c (rw[c] h[b, c, p] + rw[C + c] o[c]) + rb      g = sigmoid(z)      r[c] = h[b, c, p] (1 - g) + g o[c]

    h [B, C, H, W], kv [B, T, 2C], mask [B, T], rw 2C elements, rb one -> (x = cat(r, r) [B, 2C, H, W], attn [B, T, H, W])."""
    B, C, T, H, W = _mem_read_dims(h, kv, mask, rw, rb, "memory_read_reference")
    hf = h.reshape(B, C, H * W)
    s = torch.bmm(kv[:, :, :C], hf).masked_fill(mask.to(h.device).view(B, T, 1) == 0, float("-inf"))
    attn = torch.softmax(s, dim=1)
    o = torch.bmm(kv[:, :, C:].transpose(1, 2), attn)
    w = rw.reshape(2 * C)
    z = (w[:C].view(1, C, 1) * hf).sum(dim=1, keepdim=True) + (w[C:].view(1, C, 1) * o).sum(dim=1, keepdim=True) + rb.reshape(1, 1, 1)
    g = torch.sigmoid(z)
    r = hf * (1 - g) + g * o
    return torch.cat((r, r), 1).reshape(B, 2 * C, H, W), attn.reshape(B, T, H, W)


class _MemoryWriteFn(Function):
    @staticmethod
    def forward(ctx, U, Q):
        B, T, Md = _mem_write_dims(U, Q, "memory_write")
        m = torch.empty((B, T, Md), dtype=torch.float32, device=U.device)
        L.call("agan_mem_write_fwd", _p(U), _p(Q), _p(m), B, T, Md, _stream())
        ctx.save_for_backward(U, Q)
        return m

    @staticmethod
    @once_differentiable
    def backward(ctx, dm):
        U, Q = ctx.saved_tensors
        B, T, Md = _mem_write_dims(U, Q, "memory_write")
        dm = _dev(dm, "memory_write grad")
        dU, dQ = torch.empty_like(U), torch.empty_like(Q)
        L.call("agan_mem_write_bwd", _p(U), _p(Q), _p(dm), _p(dU), _p(dQ), B, T, Md, _stream())
        return dU, dQ


def memory_write(U: Tensor, Q: Tensor) -> Tensor:
    """The gated write of the words into the memory on the HIP kernels (csrc/memory.hip), fp32, with autograd; memory_write_reference
    states it in torch ops.  U [B, T, Md + 1] (T <= 64), Q [B, Md + 1] -> m [B, T, Md]."""
    _mem_write_dims(U, Q, "memory_write")
    _fp32_only("memory_write", "memory", U, Q)
    return _MemoryWriteFn.apply(_dev(U, "memory_write U"), _dev(Q, "memory_write Q"))


class _MemoryReadFn(Function):
    @staticmethod
    def forward(ctx, h, kv, mask, rw, rb, wdst, bdst):
        B, C, T, H, W = _mem_read_dims(h, kv, mask, rw, rb, "memory_read")
        w, bias = _dev(rw.detach(), "memory_read response weight"), _dev(rb.detach(), "memory_read response bias")
        m = mask.to(device=h.device, dtype=torch.int64).contiguous()
        x = torch.empty((B, 2 * C, H, W), dtype=torch.float32, device=h.device)
        attn = torch.empty((B, T, H, W), dtype=torch.float32, device=h.device)
        L.call("agan_mem_read_fwd", _p(h), _p(kv), _p(m), _p(w), _p(bias), _p(x), _p(attn), B, C, T, H * W, _stream())
        ctx.save_for_backward(h, kv, m, w, bias, attn)
        ctx.wdst, ctx.bdst = wdst, bdst
        ctx.set_materialize_grads(False)     # the attention map usually feeds nothing: no zero-filled gradient of its size
        return x, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, dx, dattn):
        h, kv, m, w, bias, attn = ctx.saved_tensors
        B, C, H, W = h.shape
        T = kv.shape[1]
        dx = _dev(dx, "memory_read dx") if dx is not None else torch.zeros((B, 2 * C, H, W), dtype=torch.float32, device=h.device)
        dattn = _dev(dattn, "memory_read dattn") if dattn is not None else None
        dh, dkv = torch.empty_like(h), torch.empty_like(kv)
        # a frozen response layer still gets its sums computed: they go to scratch, not into the owner's flat buffer
        dwbuf, wacc, dw = _grad_out(ctx.wdst if ctx.needs_input_grad[3] else None, w.shape, h)
        dbbuf, bacc, db = _grad_out(ctx.bdst if ctx.needs_input_grad[4] else None, bias.shape, h)
        nbytes = L.load().agan_mem_read_bwd_ws_bytes(B, C, T, H * W)
        ws, wsp = _ws(nbytes, h)
        L.call("agan_mem_read_bwd", _p(h), _p(kv), _p(m), _p(w), _p(bias), _p(attn), _p(dx), _p(dattn), _p(dh), _p(dkv), _p(dwbuf),
               _p(dbbuf), B, C, T, H * W, wacc, bacc, wsp, nbytes, _stream())
        return (dh, dkv, None, dw if ctx.needs_input_grad[3] else None, db if ctx.needs_input_grad[4] else None, None, None)


def memory_read(h: Tensor, kv: Tensor, mask: Tensor, rw: Tensor, rb: Tensor) -> Tuple[Tensor, Tensor]:
    """Address, read and respond of the dynamic memory in one HIP pass per direction (csrc/memory.hip), fp32, with autograd;
    memory_read_reference states it in torch ops.  h [B, C, H, W] (C <= 64), kv [B, T, 2C] (keys | values, T <= 64), mask [B, T]
    (0 = ignore the word), rw the response gate's weight (2C elements, any shape) and rb its bias ->
    (x [B, 2C, H, W] = cat(r, r), attn [B, T, H, W]).  The backward keeps the attention map only and recomputes the rest; the
    gradients of rw and rb go to their flat-gradient slices (grad_dst) where the parameters have one."""
    _mem_read_dims(h, kv, mask, rw, rb, "memory_read")
    _fp32_only("memory_read", "memory", h, kv)
    return _MemoryReadFn.apply(_dev(h, "memory_read h"), _dev(kv, "memory_read kv"), mask, rw, rb, grad_dst(rw), grad_dst(rb))


# --------------------------------------------------------------------------------------------------------------
# channel-wise word attention of a refinement stage (networks/attention.py: ChannelAttention; include/agan.h: agan_chan_attn_*)
# --------------------------------------------------------------------------------------------------------------
def _chan_attn_dims(h: Tensor, wt: Tensor, mask: Tensor, what: str) -> Tuple[int, int, int, int, int]:
    """-> (B, C, T, H, W) of h [B, C, H, W], wt [B, T, H * W] and mask [B, T], or ValueError"""
    if h.dim() != 4 or wt.dim() != 3 or h.numel() == 0 or wt.numel() == 0:
        raise ValueError(f"{what}: h must be [B, C, H, W] and wt [B, T, H * W], got {tuple(h.shape)} and {tuple(wt.shape)}")
    B, C, H, W = (int(s) for s in h.shape)
    T = int(wt.shape[1])
    if int(wt.shape[0]) != B or int(wt.shape[2]) != H * W or tuple(mask.shape) != (B, T):
        raise ValueError(f"{what}: h {tuple(h.shape)}, wt {tuple(wt.shape)} and mask {tuple(mask.shape)} do not fit "
                         f"([B, C, H, W], [B, T, H * W], [B, T])")
    return B, C, T, H, W


def _chan_attn_scale(scale: Optional[float], hw: int) -> float:
    return 1.0 / math.sqrt(hw) if scale is None else float(scale)


def channel_attention_reference(h: Tensor, wt: Tensor, mask: Tensor, scale: Optional[float] = None) -> Tuple[Tensor, Tensor]:
    """What channel_attention computes, in torch ops, in h's dtype, on any device, differentiable by autograd.  With p a pixel:

        m[b, c, t] = scale * sum_p h[b, c, p] wt[b, t, p], -inf where mask[b, t] == 0      alpha = softmax_t m
        f[b, c, p] = sum_t alpha[b, c, t] wt[b, t, p]

    h [B, C, H, W], wt [B, T, H * W], mask [B, T], scale None = 1 / sqrt(H * W) -> (f [B, C, H, W], alpha [B, C, T])."""
    B, C, T, H, W = _chan_attn_dims(h, wt, mask, "channel_attention_reference")
    m = torch.bmm(h.reshape(B, C, H * W), wt.transpose(1, 2)) * _chan_attn_scale(scale, H * W)
    alpha = torch.softmax(m.masked_fill(mask.to(h.device).view(B, 1, T) == 0, float("-inf")), dim=2)
    return torch.bmm(alpha, wt).reshape(B, C, H, W), alpha


class _ChannelAttentionFn(Function):
    @staticmethod
    def forward(ctx, h, wt, mask, scale):
        B, C, T, H, W = _chan_attn_dims(h, wt, mask, "channel_attention")
        m = mask.to(device=h.device, dtype=torch.int64).contiguous()
        f = torch.empty_like(h)
        alpha = torch.empty((B, C, T), dtype=torch.float32, device=h.device)
        nbytes = L.load().agan_chan_attn_fwd_ws_bytes(B, C, T, H * W)
        ws, wsp = _ws(nbytes, h)
        L.call("agan_chan_attn_fwd", _p(h), _p(wt), _p(m), scale, _p(alpha), _p(f), B, C, T, H * W, wsp, nbytes, _stream())
        ctx.save_for_backward(h, wt, alpha)
        ctx.scale = scale
        ctx.set_materialize_grads(False)     # alpha usually feeds nothing: no zero-filled gradient for it
        return f, alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, df, dalpha):
        h, wt, alpha = ctx.saved_tensors
        B, C, H, W = h.shape
        T = wt.shape[1]
        need_h, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if (df is None and dalpha is None) or not (need_h or need_w):
            return None, None, None, None
        df = _dev(df, "channel_attention df") if df is not None else torch.zeros_like(h)
        dalpha = _dev(dalpha, "channel_attention dalpha") if dalpha is not None else None
        dh = torch.empty_like(h) if need_h else None          # a NULL destination: the kernel computes nothing for it
        dwt = torch.empty_like(wt) if need_w else None
        nbytes = L.load().agan_chan_attn_bwd_ws_bytes(B, C, T, H * W)
        ws, wsp = _ws(nbytes, h)
        L.call("agan_chan_attn_bwd", _p(h), _p(wt), _p(alpha), _p(df), _p(dalpha), ctx.scale, _p(dh), _p(dwt), B, C, T, H * W, wsp, nbytes,
               _stream())
        return dh, dwt, None, None


def channel_attention(h: Tensor, wt: Tensor, mask: Tensor, scale: Optional[float] = None) -> Tuple[Tensor, Tensor]:
    """Channel-wise word attention on the HIP kernels (csrc/chan_attn.hip), fp32, with autograd; channel_attention_reference states
    it in torch ops.  h [B, C, H, W] (C <= 64), wt [B, T, H * W] (the words seen through the perception layer, T <= 64), mask [B, T]
    (0 = ignore the word), scale None = 1 / sqrt(H * W) -> (f [B, C, H, W], alpha [B, C, T]).  Three launches per direction; nothing of
    the backward is computed for an input that needs no gradient."""
    B, C, T, H, W = _chan_attn_dims(h, wt, mask, "channel_attention")
    _fp32_only("channel_attention", "channel-attention", h, wt)
    return _ChannelAttentionFn.apply(_dev(h, "channel_attention h"), _dev(wt, "channel_attention wt"), mask, _chan_attn_scale(scale, H * W))


def spatial_mean(x: Tensor) -> Tensor:
    """mean over the positions of x [B, C, H, W] -> [B, C] on the HIP kernel (agan_global_avgpool_fwd), fp32.  NOT differentiable:
    the result is detached (the dynamic memory's write gate reads the image through it without a gradient)."""
    xd = _dev(x.detach(), "spatial_mean input")
    if xd.dim() < 3 or xd.numel() == 0:
        raise ValueError(f"spatial_mean: x must be [B, C, positions...] and not empty, got {tuple(x.shape)}")
    B, C = int(xd.shape[0]), int(xd.shape[1])
    y = torch.empty((B, C), dtype=torch.float32, device=xd.device)
    L.call("agan_global_avgpool_fwd", _p(xd), _p(y), B, C, xd.numel() // (B * C), _stream())
    return y


# --------------------------------------------------------------------------------------------------------------
# small heads
# --------------------------------------------------------------------------------------------------------------
class _ReparamFn(Function):
    @staticmethod
    def forward(ctx, mu, logvar, eps):
        mu, logvar, eps = _dev(mu, "mu"), _dev(logvar, "logvar"), _dev(eps, "eps")
        c = torch.empty_like(mu)
        L.call("agan_reparam_fwd", _p(mu), _p(logvar), _p(eps), _p(c), mu.numel(), _stream())
        ctx.save_for_backward(logvar, eps)
        return c

    @staticmethod
    @once_differentiable
    def backward(ctx, dc):
        logvar, eps = ctx.saved_tensors
        dc = _dev(dc, "dc")
        dmu, dlv = torch.empty_like(dc), torch.empty_like(dc)
        L.call("agan_reparam_bwd", _p(logvar), _p(eps), _p(dc), _p(dmu), _p(dlv), dc.numel(), _stream())
        return dmu, dlv, None


def reparametrize(mu, logvar, eps):
    return _ReparamFn.apply(mu, logvar, eps)


class _DiscLossFn(Function):
    @staticmethod
    def forward(ctx, p_real, p_fake):
        p_real, p_fake = _dev(p_real, "D(x)"), _dev(p_fake, "D(G(z))")
        loss = torch.empty((), dtype=torch.float32, device=p_real.device)
        dr, df = torch.empty_like(p_real), torch.empty_like(p_fake)
        L.call("agan_disc_loss", _p(p_real), _p(p_fake), _p(loss), _p(dr), _p(df), p_real.numel(), _stream())
        ctx.save_for_backward(dr, df)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dr, df = ctx.saved_tensors
        return dr * g, df * g


def ns_disc_loss(p_real, p_fake):
    return _DiscLossFn.apply(p_real, p_fake)


class _DiscLossPairedFn(Function):
    """the same loss on one [real; fake] score vector (the paired discriminator pass): no slice views, so autograd does not
    zero-fill and scatter two half gradients"""

    @staticmethod
    def forward(ctx, p):
        p = _dev(p, "D([x; G(z)])")
        n = p.numel() // 2
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        dp = torch.empty_like(p)
        L.call("agan_disc_loss", _p(p[:n]), _p(p[n:]), _p(loss), _p(dp[:n]), _p(dp[n:]), n, _stream())
        ctx.save_for_backward(dp)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return dp * g


def ns_disc_loss_paired(p: Tensor) -> Tensor:
    """NonSaturatingDiscLoss on a score vector whose first half is D(x) and second half D(G(z))"""
    if p.dim() != 1 or p.numel() % 2:
        raise L.AganError("ns_disc_loss_paired: expected a [2B] score vector")
    return _DiscLossPairedFn.apply(p)


class _GenLossFn(Function):
    @staticmethod
    def forward(ctx, p_fake):
        p_fake = _dev(p_fake, "D(G(z))")
        loss = torch.empty((), dtype=torch.float32, device=p_fake.device)
        df = torch.empty_like(p_fake)
        L.call("agan_gen_loss", _p(p_fake), _p(loss), _p(df), p_fake.numel(), _stream())
        ctx.save_for_backward(df)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        return df * g


def ns_gen_loss(p_fake):
    return _GenLossFn.apply(p_fake)


# --------------------------------------------------------------------------------------------------------------
# the text-conditional discriminator head (networks/discriminators.py: COND_DNET; include/agan.h: agan_cond_join_*, agan_cond_disc_loss)
# --------------------------------------------------------------------------------------------------------------
# AttnGAN's jointConv is conv3x3 over cat(h, rep(s)) on the 4x4 code.  The sentence channels are constant over the map, so
#     conv3x3(cat(h, rep(s)), W)[n, c, i, j] = conv3x3(h, W[:, :8df])[n, c, i, j] + sum_{t valid at (i, j)} P[n, c, t]
#     P[n, c, t] = sum_e s[n, e] * W[c, 8df + e, t]
# with t = 3 (di + 1) + (dj + 1) the tap that reads input (i + di, j + dj), valid iff that position lies inside the map.  `cond_join`
# adds the two terms: yi from the library's conv (computed ONCE for [real; fake]), p from its linear (once per caption).
def _tap_mask(dtype, device) -> Tensor:
    """[9, 4, 4]: 1 where tap t is valid at (i, j)"""
    m = torch.zeros(9, 4, 4, dtype=dtype, device=device)
    for t in range(9):
        di, dj = t // 3 - 1, t % 3 - 1
        m[t, max(0, -di):4 - max(0, di), max(0, -dj):4 - max(0, dj)] = 1
    return m


def _cond_join_dims(yi: Tensor, p: Tensor, wrong: bool, what: str) -> Tuple[int, int, int]:
    """-> (B, k, C) of yi [k * B, C, 4, 4] and p [B, C, 9], or ValueError"""
    if yi.dim() != 4 or tuple(yi.shape[2:]) != (4, 4):
        raise ValueError(f"{what}: the image term must be [k * B, C, 4, 4], got {tuple(yi.shape)}")
    if p.dim() != 3 or p.shape[2] != 9 or p.shape[1] != yi.shape[1]:
        raise ValueError(f"{what}: the sentence term must be [B, {yi.shape[1]}, 9], got {tuple(p.shape)}")
    B, C = int(p.shape[0]), int(p.shape[1])
    if B < 1 or C < 1 or yi.shape[0] < B or yi.shape[0] % B:
        raise ValueError(f"{what}: {yi.shape[0]} image rows are not whole groups of the {B} captions")
    if yi.device != p.device:
        raise ValueError(f"{what}: the image term is on {yi.device}, the sentence term on {p.device}")
    if wrong and B < 2:
        raise ValueError(f"{what}: the mismatched pairs (wrong=True) need at least 2 captions")
    return B, int(yi.shape[0]) // B, C


def cond_join_reference(yi: Tensor, p: Tensor, wrong: bool = False) -> Tensor:
    """What cond_join computes, in torch ops, in the operands' dtype, on any device, differentiable by autograd:
    y[n] = yi[n] + S(p[n mod B]) for the k * B rows of yi, and with `wrong` B more rows yi[b] + S(p[(b + 1) mod B]), where
    S(p)[c, i, j] = sum of p[c, t] over the taps valid at (i, j), added in ascending t starting from yi (an invalid tap adds 0)."""
    B, k, C = _cond_join_dims(yi, p, wrong, "cond_join_reference")
    if yi.dtype != p.dtype:
        raise ValueError(f"cond_join_reference: the image term is {yi.dtype}, the sentence term {p.dtype}")
    m = _tap_mask(yi.dtype, yi.device)
    caps, y = p.repeat(k, 1, 1), yi
    if wrong:
        caps, y = torch.cat([caps, p.roll(-1, 0)], dim=0), torch.cat([yi, yi[:B]], dim=0)
    for t in range(9):
        y = y + caps[:, :, t, None, None] * m[t]
    return y


class _CondJoinFn(Function):
    @staticmethod
    def forward(ctx, yi, p, wrong):
        B, C = p.shape[0], p.shape[1]
        k = yi.shape[0] // B
        yi, p = _dev(yi, "cond_join image term"), _dev(p, "cond_join sentence term")
        y = torch.empty(((k + wrong) * B, C, 4, 4), dtype=torch.float32, device=yi.device)
        L.call("agan_cond_join_fwd", _p(yi), _p(p), _p(y), B, k, C, wrong, _stream())
        ctx.dims = (B, k, C, wrong)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        B, k, C, wrong = ctx.dims
        want_yi, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dy = _dev(dy, "cond_join grad")
        dyi = dp = None
        if want_yi and not wrong:
            dyi = dy                     # without wrong rows the image term's gradient IS dy: no launch (the generator update)
        elif want_yi:
            dyi = torch.empty((k * B, C, 4, 4), dtype=torch.float32, device=dy.device)
        if want_p:
            dp = torch.empty((B, C, 9), dtype=torch.float32, device=dy.device)
        if dp is not None or wrong and dyi is not None:
            L.call("agan_cond_join_bwd", _p(dy), _p(dyi if wrong else None), _p(dp), B, k, C, wrong, _stream())
        return dyi, dp, None


def cond_join(yi: Tensor, p: Tensor, wrong: bool = False) -> Tensor:
    """The join of the conditional discriminator head on the HIP kernels (csrc/cond_join.hip), fp32, with autograd.

    yi [k * B, C, 4, 4]: the image term, k consecutive groups of B rows, row n carrying caption n mod B.  p [B, C, 9]: the sentence
    term per caption, channel and tap.  -> y [(k + wrong) * B, C, 4, 4]: rows n < k * B are yi[n] + S(p[n mod B]); with `wrong`, B more
    rows yi[b] + S(p[(b + 1) mod B]) pair the FIRST group's images with the next sample's caption, cyclically (cond_join_reference
    states it in torch ops).  The backward has one summation order and no atomics; only the gradients autograd asks for are
    produced, and the image term's gradient without wrong rows is dy itself.  Works in fp32: 16-bit operands (activation storage)
    are widened on the way in and their gradients cast back.  ValueError on mismatched shapes, devices or dtypes, and for
    wrong=True with fewer than 2 captions."""
    B, k, C = _cond_join_dims(yi, p, wrong, "cond_join")
    for t, name in ((yi, "image"), (p, "sentence")):
        if not t.is_cuda:
            raise ValueError(f"cond_join: the {name} term is on {t.device}; the kernels run on the GPU (cond_join_reference runs anywhere)")
        if t.dtype != torch.float32 and t.dtype not in _DT_OF:
            raise ValueError(f"cond_join: the {name} term is {t.dtype}; expected float32 (or 16-bit activation storage)")
    if yi.dtype != torch.float32:       # autograd casts the gradients back
        yi = yi.float()
    if p.dtype != torch.float32:
        p = p.float()
    return _CondJoinFn.apply(yi, p, bool(wrong))


def _cond_scores(pu: Tensor, pc: Tensor, what: str) -> int:
    if pu.dim() != 1 or pc.dim() != 1 or pu.numel() < 2 or pu.numel() % 2 or pc.numel() * 2 != pu.numel() * 3:
        raise ValueError(f"{what}: expected unconditional scores [2B] of [real; fake] and conditional scores [3B] of [real; fake; wrong], "
                         f"got {tuple(pu.shape)} and {tuple(pc.shape)}")
    if pu.device != pc.device or pu.dtype != pc.dtype:
        raise ValueError(f"{what}: the score vectors differ in device or dtype ({pu.device} {pu.dtype}, {pc.device} {pc.dtype})")
    return pu.numel() // 2


def cond_disc_loss_reference(pu: Tensor, pc: Tensor) -> Tensor:
    """cond_disc_loss in torch ops, in the operands' dtype, on any device."""
    B = _cond_scores(pu, pc, "cond_disc_loss_reference")
    real = (-torch.log(pu[:B] + 1e-8)).mean() + (-torch.log(pc[:B] + 1e-8)).mean()
    fake = ((-torch.log(1 - pu[B:] + 1e-8)).mean() + (-torch.log(1 - pc[B:2 * B] + 1e-8)).mean()
            + (-torch.log(1 - pc[2 * B:] + 1e-8)).mean())
    return real / 2 + fake / 3


class _CondDiscLossFn(Function):
    @staticmethod
    def forward(ctx, pu, pc):
        pu, pc = _dev(pu, "unconditional scores"), _dev(pc, "conditional scores")
        loss = torch.empty((), dtype=torch.float32, device=pu.device)
        dpu, dpc = torch.empty_like(pu), torch.empty_like(pc)
        L.call("agan_cond_disc_loss", _p(pu), _p(pc), _p(loss), _p(dpu), _p(dpc), pu.numel() // 2, _stream())
        ctx.save_for_backward(dpu, dpc)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dpu, dpc = ctx.saved_tensors
        return dpu * g, dpc * g


def cond_disc_loss(pu: Tensor, pc: Tensor) -> Tensor:
    """The discriminator loss of a text-conditional discriminator in ONE launch (loss and both gradients): pu [2B] are the unconditional
    scores of [real; fake], pc [3B] the conditional scores of [real; fake; wrong], all probabilities;
        (m(-log pu_r) + m(-log pc_r)) / 2 + (m(-log(1 - pu_f)) + m(-log(1 - pc_f)) + m(-log(1 - pc_w))) / 3,   m = mean over B
    -- AttnGAN's weights (errD_real: two terms halved; errD_fake + errD_wrong: three terms over 3) on this project's non-saturating
    log terms with their 1e-8 guards, not BCELoss."""
    _cond_scores(pu, pc, "cond_disc_loss")
    if not pu.is_cuda:
        raise ValueError(f"cond_disc_loss: the scores are on {pu.device}; the kernel runs on the GPU (cond_disc_loss_reference runs anywhere)")
    return _CondDiscLossFn.apply(pu, pc)


class _KLFn(Function):
    @staticmethod
    def forward(ctx, mu, logvar):
        mu, logvar = _dev(mu, "mu"), _dev(logvar, "logvar")
        loss = torch.empty((), dtype=torch.float32, device=mu.device)
        dmu, dlv = torch.empty_like(mu), torch.empty_like(logvar)
        L.call("agan_kl_loss", _p(mu), _p(logvar), _p(loss), _p(dmu), _p(dlv), mu.numel(), _stream())
        ctx.save_for_backward(dmu, dlv)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dmu, dlv = ctx.saved_tensors
        return dmu * g, dlv * g


def kl_loss(mu, logvar):
    return _KLFn.apply(mu, logvar)


# --------------------------------------------------------------------------------------------------------------
# DAMSM losses (losses/words_loss.py:29-102, losses/sentence_loss.py:12-50)
# --------------------------------------------------------------------------------------------------------------
def _ids(class_ids, device) -> Optional[Tensor]:
    if class_ids is None:
        return None
    return torch.as_tensor(class_ids).to(device=device, dtype=torch.int64).contiguous()


def _labels(labels, batch: int, device) -> Optional[Tensor]:
    """CE targets for the kernels (words_loss.py:98-99, sentence_loss.py:46-47): an int64 device vector, or None for arange(batch)
    (the kernels' built-in default -- what train.py:104 / _make_match_labels builds, recognised by the `_agan_arange` tag = (batch, tensor version at tagging) so that
    the hot path neither copies nor reads the labels back)."""
    if labels is None:
        return None
    tag = getattr(labels, "_agan_arange", None)
    if tag is not None and tag == (batch, labels._version):      # still the untouched arange _make_match_labels built
        return None
    lab = torch.as_tensor(labels).reshape(-1)
    if lab.numel() != batch:
        raise ValueError(f"labels must have one entry per sample (got {lab.numel()} for a batch of {batch})")
    return lab.to(device=device, dtype=torch.int64).contiguous()


class _FuncAttentionFn(Function):
    @staticmethod
    def forward(ctx, query, context, gamma1, scale):
        q, c = _dev(query, "query"), _dev(context, "context")
        B, D, Lq = q.shape
        ih, iw = c.shape[2], c.shape[3]
        wctx = torch.empty((B, D, Lq), dtype=torch.float32, device=q.device)
        attn = torch.empty((B, Lq, ih, iw), dtype=torch.float32, device=q.device)
        L.call("agan_func_attention_fwd", _p(q), _p(c), gamma1, scale, _p(wctx), _p(attn), B, D, Lq, ih * iw, _stream())
        ctx.save_for_backward(q, c)
        ctx.hp = (gamma1, scale)
        ctx.set_materialize_grads(False)
        return wctx, attn

    @staticmethod
    @once_differentiable
    def backward(ctx, dwctx, dattn):
        q, c = ctx.saved_tensors
        B, D, Lq = q.shape
        S = c.shape[2] * c.shape[3]
        dq, dc = torch.empty_like(q), torch.empty_like(c)
        if dwctx is None and dattn is None:
            return dq.zero_(), dc.zero_(), None, None
        dwctx = _dev(dwctx, "func_attention d(weightedContext)") if dwctx is not None else None
        dattn = _dev(dattn, "func_attention d(attn)") if dattn is not None else None
        L.call("agan_func_attention_bwd", _p(q), _p(c), _p(dwctx), _p(dattn), *ctx.hp, _p(dq), _p(dc), B, D, Lq, S, _stream())
        return dq, dc, None, None


def func_attention(query: Tensor, context: Tensor, gamma1: float = 4.0, scaled: bool = True):
    """The parameter-free DAMSM attention (attention.py:82-120), differentiable like the reference's plain-autograd version.
    Inside the training step it runs fused into the words-loss kernels; this is the standalone entry point."""
    D = query.shape[1]
    return _FuncAttentionFn.apply(query, context, float(gamma1), (1.0 / math.sqrt(D)) if scaled else 1.0)


class _WordsLossFn(Function):
    @staticmethod
    def forward(ctx, feat, wemb, lens, cids, labels, g1, g2, g3, lam):
        feat, wemb = _dev(feat, "img_features"), _dev(wemb, "words_emb")
        B, D = feat.shape[0], feat.shape[1]
        S = feat.numel() // (B * D)
        T = wemb.shape[2]
        loss = torch.empty((), dtype=torch.float32, device=feat.device)
        sim = torch.empty((B, B), dtype=torch.float32, device=feat.device)
        maps = torch.zeros((B, T, S), dtype=torch.float32, device=feat.device)
        save = torch.empty(L.load().agan_words_loss_save_elems(B, D, T, S), dtype=torch.float32, device=feat.device)
        L.call("agan_words_loss_fwd", _p(feat), _p(wemb), _p(lens), _p(cids), _p(labels), g1, g2, g3, lam, _p(loss), _p(sim), _p(maps),
               _p(save), B, D, T, S, _stream())
        ctx.save_for_backward(feat, wemb, lens, save)
        ctx.hp = (g1, g2, g3, lam)
        ctx.mark_non_differentiable(maps, sim)
        return loss, maps, sim

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, _dmaps, _dsim):
        feat, wemb, lens, save = ctx.saved_tensors
        B, D = feat.shape[0], feat.shape[1]
        S = feat.numel() // (B * D)
        T = wemb.shape[2]
        dfeat, dwemb = torch.empty_like(feat), torch.empty_like(wemb)
        dl = dloss.to(torch.float32).contiguous()
        nbytes = L.load().agan_words_loss_bwd_ws_bytes(B, D, T, S)
        ws, wsp = _ws(nbytes, feat)
        L.call("agan_words_loss_bwd", _p(feat), _p(wemb), _p(lens), _p(save), _p(dl), *ctx.hp, _p(dfeat), _p(dwemb),
               B, D, T, S, wsp, nbytes, _stream())
        return dfeat, dwemb, None, None, None, None, None, None, None


def words_loss(feat, wemb, cap_lens, class_ids, gamma1, gamma2, gamma3, wlambda, labels=None):
    if isinstance(cap_lens, Tensor) and cap_lens.is_cuda and cap_lens.dtype == torch.int64:
        lens = cap_lens.contiguous()                       # already resident: no host round trip (HIP-graph capturable)
    else:
        lens = torch.as_tensor(cap_lens).to(device=feat.device, dtype=torch.int64).contiguous()
    return _WordsLossFn.apply(feat, wemb, lens, _ids(class_ids, feat.device), _labels(labels, feat.shape[0], feat.device),
                              float(gamma1), float(gamma2), float(gamma3), float(wlambda))


class _SentLossFn(Function):
    @staticmethod
    def forward(ctx, cnn, rnn, cids, labels, g3, lam, eps):
        cnn, rnn = _dev(cnn, "cnn_code"), _dev(rnn, "rnn_code")
        B, D = cnn.shape
        loss = torch.empty((), dtype=torch.float32, device=cnn.device)
        save = torch.empty(2 * B * B + 2 * B, dtype=torch.float32, device=cnn.device)
        L.call("agan_sent_loss_fwd", _p(cnn), _p(rnn), _p(cids), _p(labels), g3, lam, eps, _p(loss), _p(save), B, D, _stream())
        ctx.save_for_backward(cnn, rnn, save)
        ctx.hp = (g3, lam, eps)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        cnn, rnn, save = ctx.saved_tensors
        B, D = cnn.shape
        dc, dr = torch.empty_like(cnn), torch.empty_like(rnn)
        dl = dloss.to(torch.float32).contiguous()
        L.call("agan_sent_loss_bwd", _p(cnn), _p(rnn), _p(save), _p(dl), *ctx.hp, _p(dc), _p(dr), B, D, _stream())
        return dc, dr, None, None, None, None, None


def sentence_loss(cnn_code, rnn_code, class_ids, gamma3, slambda, eps=1e-8, labels=None):
    return _SentLossFn.apply(cnn_code, rnn_code, _ids(class_ids, cnn_code.device), _labels(labels, cnn_code.shape[0], cnn_code.device),
                             float(gamma3), float(slambda), float(eps))


# --------------------------------------------------------------------------------------------------------------
# word-level discriminator score (include/agan.h: agan_word_corr_*; csrc/word_corr.hip; ControlGAN section 3.2)
# --------------------------------------------------------------------------------------------------------------
def _word_corr_dims(regions: Tensor, words: Tensor, shift, what: str) -> Tuple[int, int, int, int]:
    """-> (B, D, S, T) of regions [B, D, S] (or [B, D, h, w]) and words [B, D, T], or ValueError"""
    if regions.dim() not in (3, 4):
        raise ValueError(f"{what}: regions must be [B, D, S] or [B, D, h, w], got {tuple(regions.shape)}")
    if words.dim() != 3 or words.shape[0] != regions.shape[0] or words.shape[1] != regions.shape[1]:
        raise ValueError(f"{what}: words must be [{regions.shape[0]}, {regions.shape[1]}, T], got {tuple(words.shape)}")
    if words.requires_grad:
        raise ValueError(f"{what}: the words are constants of the score (the text encoder is frozen in the GAN step); detach them")
    if regions.device != words.device:
        raise ValueError(f"{what}: regions are on {regions.device}, words on {words.device}")
    B, D = int(regions.shape[0]), int(regions.shape[1])
    S, T = regions.numel() // max(B * D, 1), int(words.shape[2])
    if B < 1 or D < 1 or S < 1 or T < 1:
        raise ValueError(f"{what}: empty operand (B={B}, D={D}, S={S}, T={T})")
    if isinstance(shift, bool) or not isinstance(shift, int) or not 0 <= shift < B:
        raise ValueError(f"{what}: shift must be an integer in [0, B = {B}), got {shift!r}")
    return B, D, S, T


def word_corr_reference(regions: Tensor, words: Tensor, lens, shift: int = 0, gamma1: float = 4.0, gamma2: float = 5.0,
                        eps: float = 1e-8) -> Tuple[Tensor, Tensor, Tensor]:
    """What word_corr computes, line by line as include/agan.h states it, in torch ops, in the operands' dtype, on any device,
    differentiable by autograd w.r.t. the regions: -> (p [B], r [B, T], g [B, T]).  `lens` is read on the host."""
    B, D, S, T = _word_corr_dims(regions, words, shift, "word_corr_reference")
    if regions.dtype != words.dtype:
        raise ValueError(f"word_corr_reference: regions are {regions.dtype}, words {words.dtype}")
    lens = [int(v) for v in torch.as_tensor(lens).reshape(-1).tolist()]
    if len(lens) != B:
        raise ValueError(f"word_corr_reference: lens must have one entry per caption (got {len(lens)} for {B})")
    regions = regions.reshape(B, D, S)
    ps, rs, gs = [], [], []
    for b in range(B):
        c = (b + shift) % B
        Lc = min(lens[c], T)
        w, n = words[c, :, :Lc].t(), regions[b]                              # w [L, D], n [D, S]
        m = w @ n                                                            # m[l, s] = <w_l, n_s>
        sbar = torch.softmax(m, dim=0)                                       # over the L words
        alpha = torch.softmax(gamma1 * sbar, dim=1)                          # over the S regions
        ctx = alpha @ n.t()                                                  # ctx_l = sum_s alpha[l, s] n_s
        r = (ctx * w).sum(1) / (ctx.norm(dim=1) * w.norm(dim=1)).clamp(min=eps)
        g = torch.softmax(w @ w.mean(0), dim=0)                              # <mean_k w_k, w_l>
        ps.append((g * torch.sigmoid(gamma2 * r)).sum())
        rs.append(torch.nn.functional.pad(r, (0, T - Lc)))
        gs.append(torch.nn.functional.pad(g, (0, T - Lc)))
    return torch.stack(ps), torch.stack(rs), torch.stack(gs)


class _WordCorrFn(Function):
    @staticmethod
    def forward(ctx, regions, words, lens, shift, g1, g2, eps):
        regions, words = _dev(regions, "word_corr regions"), _dev(words, "word_corr words")
        B, D, S = regions.shape
        T = words.shape[2]
        lib = L.load()
        n_save = lib.agan_word_corr_save_elems(B, D, T, S)
        if n_save == 0:
            raise L.AganError(f"word_corr: {lib.agan_last_error().decode()}")
        dev = regions.device
        p = torch.empty(B, dtype=torch.float32, device=dev)
        r = torch.empty((B, T), dtype=torch.float32, device=dev)
        g = torch.empty((B, T), dtype=torch.float32, device=dev)
        save = torch.empty(n_save, dtype=torch.float32, device=dev)
        L.call("agan_word_corr_fwd", _p(regions), _p(words), _p(lens), shift, g1, g2, eps, _p(p), _p(r), _p(g), _p(save), B, D, T, S,
               _stream())
        ctx.save_for_backward(regions, words, lens, save)
        ctx.hp = (shift, g1, g2, eps)
        ctx.mark_non_differentiable(r, g)
        return p, r, g

    @staticmethod
    @once_differentiable
    def backward(ctx, dp, _dr, _dg):
        regions, words, lens, save = ctx.saved_tensors
        B, D, S = regions.shape
        T = words.shape[2]
        shift, g1, g2, eps = ctx.hp
        dregions = torch.empty_like(regions)
        dp = _dev(dp, "word_corr d(p)")
        nbytes = L.load().agan_word_corr_bwd_ws_bytes(B, D, T, S)
        ws, wsp = _ws(nbytes, regions)
        L.call("agan_word_corr_bwd", _p(regions), _p(words), _p(lens), shift, _p(save), _p(dp), g1, g2, eps, _p(dregions), B, D, T, S,
               wsp, nbytes, _stream())
        return dregions, None, None, None, None, None, None


def word_corr(regions: Tensor, words: Tensor, lens, shift: int = 0, gamma1: float = 4.0, gamma2: float = 5.0,
              eps: float = 1e-8) -> Tuple[Tensor, Tensor, Tensor]:
    """The word-level discriminator's score on the HIP kernels (csrc/word_corr.hip), fp32, with autograd: regions [B, D, S] (or
    [B, D, h, w]) and words [B, D, T], lens [B] -> (p [B], r [B, T], g [B, T]); image b is scored against caption (b + shift) mod B
    (include/agan.h states the formulas, word_corr_reference restates them in torch ops).  One launch per direction; a device int64
    `lens` is read by the kernels (no host round trip, HIP-graph capturable).  The gradient reaches the regions from p only: r and
    g are non-differentiable, and the words are constants -- ValueError if they require grad.  ValueError too for CPU tensors
    (word_corr_reference runs anywhere), mismatched shapes and a shift outside [0, B)."""
    B, D, S, T = _word_corr_dims(regions, words, shift, "word_corr")
    if not regions.is_cuda:
        raise ValueError(f"word_corr: the operands are on {regions.device}; the kernels run on the GPU (word_corr_reference runs anywhere)")
    if isinstance(lens, Tensor) and lens.is_cuda and lens.dtype == torch.int64:
        lens = lens.contiguous()                           # already resident: no host round trip (HIP-graph capturable)
    else:
        lens = torch.as_tensor(lens).to(device=regions.device, dtype=torch.int64).contiguous()
    if lens.numel() != B:
        raise ValueError(f"word_corr: lens must have one entry per caption (got {lens.numel()} for {B})")
    return _WordCorrFn.apply(regions.reshape(B, D, S), words, lens.reshape(-1), int(shift), float(gamma1), float(gamma2), float(eps))


# --------------------------------------------------------------------------------------------------------------
# spectral normalisation of a weight (include/agan.h: agan_spectral_*; csrc/spectral.hip; Miyato et al. 2018)
# --------------------------------------------------------------------------------------------------------------
def _spectral_dims(weight: Tensor, u: Tensor, v: Tensor, second: Optional[Tensor], what: str) -> Tuple[int, int, int]:
    """-> (Cout, K0, K1) of weight [Cout, ...] and the optional second column segment [Cout, ...], or ValueError"""
    if weight.dim() < 2 or weight.numel() == 0:
        raise ValueError(f"{what}: the weight must be [Cout, ...] with at least two axes, got {tuple(weight.shape)}")
    cout = int(weight.shape[0])
    k0, k1 = weight.numel() // cout, 0
    if second is not None:
        if second.dim() < 2 or second.numel() == 0 or second.numel() % cout:
            raise ValueError(f"{what}: the second segment must hold {cout} rows, got {tuple(second.shape)}")
        k1 = second.numel() // cout
    if tuple(u.shape) != (cout,) or tuple(v.shape) != (k0 + k1,):
        raise ValueError(f"{what}: u must be [{cout}] and v [{k0 + k1}], got {tuple(u.shape)} and {tuple(v.shape)}")
    if u.requires_grad or v.requires_grad:
        raise ValueError(f"{what}: u and v are state, not parameters")
    for t in (u, v) + (() if second is None else (second,)):
        if t.device != weight.device or t.dtype != weight.dtype:
            raise ValueError(f"{what}: every operand must be {weight.dtype} on {weight.device}, got {t.dtype} on {t.device}")
    return cout, k0, k1


def spectral_weight_reference(weight: Tensor, u: Tensor, v: Tensor, training: bool, second: Optional[Tensor] = None):
    """What spectral_weight computes, as include/agan.h states it and as torch.nn.utils.spectral_norm does with one power iteration,
    in torch ops, in the operands' dtype, on any device, differentiable by autograd with u and v as constants.  `second` [Cout, K1]
    (viewed so): the weight is the row-wise concatenation [weight | second], stored as two tensors.  Training mode writes u' and v
    into `u` and `v`.  -> weight_sn, or (weight_sn, second_sn)."""
    cout, k0, k1 = _spectral_dims(weight, u, v, second, "spectral_weight_reference")
    W = weight.reshape(cout, k0) if second is None else torch.cat([weight.reshape(cout, k0), second.reshape(cout, k1)], dim=1)
    if training:
        with torch.no_grad():
            vn = torch.nn.functional.normalize(torch.mv(W.t(), u), dim=0, eps=1e-12)
            un = torch.nn.functional.normalize(torch.mv(W, vn), dim=0, eps=1e-12)
            u.copy_(un)
            v.copy_(vn)
        u, v = un, vn                                            # this forward's own values: a later iteration moves the buffers
    else:
        u, v = u.clone(), v.clone()
    sigma = torch.dot(u, torch.mv(W, v))
    return weight / sigma if second is None else (weight / sigma, second / sigma)


class _SpectralFn(Function):
    """-> (weight_sn, second_sn or an empty tensor, u', v).  Everything a backward needs -- W_sn, u', v, sigma of THIS forward -- is in
    fresh tensors saved per call: a discriminator runs two forwards before one backward (StandardDiscLoss, batch_pairs = False)."""

    @staticmethod
    def forward(ctx, weight, second, u, v, iterate, wdst, sdst):
        w0 = _dev(weight.detach(), "spectral weight")
        w1 = _dev(second.detach(), "spectral weight (second segment)") if second is not None else None
        cout = w0.shape[0]
        k0, k1 = w0.numel() // cout, (w1.numel() // cout if w1 is not None else 0)
        u, v = _dev(u, "spectral u"), _dev(v, "spectral v")
        lib = L.load()
        wsn0 = torch.empty_like(w0)
        wsn1 = torch.empty_like(w1) if w1 is not None else w0.new_empty(0)
        sigma = torch.empty(1, dtype=torch.float32, device=w0.device)
        if iterate:
            un, vn = torch.empty_like(u), torch.empty_like(v)
        else:
            un, vn = u.clone(), v.clone()
        nbytes = lib.agan_spectral_fwd_ws_bytes(cout, k0, k1)
        ws, wsp = _ws(nbytes, w0)
        L.call("agan_spectral_fwd", _p(w0), _p(w1), _p(u), _p(v), _p(un), _p(vn), _p(sigma), _p(wsn0), _p(wsn1 if w1 is not None else None),
               cout, k0, k1, int(iterate), wsp, nbytes, _stream())
        ctx.save_for_backward(wsn0, wsn1, un, vn, sigma)
        ctx.dims, ctx.wdst, ctx.sdst, ctx.two = (cout, k0, k1), wdst, sdst, w1 is not None
        ctx.mark_non_differentiable(un, vn)
        if w1 is None:
            ctx.mark_non_differentiable(wsn1)
        return wsn0, wsn1, un, vn

    @staticmethod
    @once_differentiable
    def backward(ctx, d0, d1, _du, _dv):
        wsn0, wsn1, un, vn, sigma = ctx.saved_tensors
        cout, k0, k1 = ctx.dims
        d0 = _dev(d0, "spectral d(weight_sn)") if d0 is not None else torch.zeros_like(wsn0)
        dw0buf, acc0, dw0 = _grad_out(ctx.wdst, wsn0.shape, wsn0)
        dw1buf = dw1 = None
        acc1 = 0
        if ctx.two:
            d1 = _dev(d1, "spectral d(second_sn)") if d1 is not None else torch.zeros_like(wsn1)
            dw1buf, acc1, dw1 = _grad_out(ctx.sdst, wsn1.shape, wsn1)
        else:
            d1 = None
        nbytes = L.load().agan_spectral_bwd_ws_bytes(cout, k0, k1)
        ws, wsp = _ws(nbytes, wsn0)
        L.call("agan_spectral_bwd", _p(d0), _p(d1), _p(wsn0), _p(wsn1 if ctx.two else None), _p(un), _p(vn), _p(sigma), _p(dw0buf), _p(dw1buf),
               cout, k0, k1, acc0, acc1, wsp, nbytes, _stream())
        return dw0, dw1, None, None, None, None, None


def spectral_weight(weight: Tensor, u: Tensor, v: Tensor, training: bool, second: Optional[Tensor] = None):
    """weight / sigma on the HIP kernels (csrc/spectral.hip), fp32 in every precision mode, with autograd: sigma is the estimate of the
    largest singular value of weight viewed [Cout, K] that one power iteration from the stored (u, v) gives -- torch.nn.utils.spectral_norm's
    rule (include/agan.h states the formulas, spectral_weight_reference restates them in torch ops).  `training` iterates once and stores
    u' and v back into `u` and `v`; eval mode leaves them.  `second`: the weight is [weight | second] row by row, held in two tensors;
    both are divided by the ONE sigma and (weight_sn, second_sn) comes back.  The result is a FRESH tensor at every call, and the
    backward uses the u', v and sigma of its own forward: two forwards followed by one backward are fine.  The weight gradient goes to
    grad_dst(weight) (grad_dst(second)) where the flat optimiser tagged the parameter.  The consumer must not cache a packed form of the
    result (HF.conv2d / HF.linear with cache=None).  CPU tensors take spectral_weight_reference."""
    _spectral_dims(weight, u, v, second, "spectral_weight")
    if not weight.is_cuda:
        return spectral_weight_reference(weight, u, v, training, second)
    wsn0, wsn1, un, vn = _SpectralFn.apply(weight, second, u, v, bool(training), grad_dst(weight),
                                           grad_dst(second) if second is not None else None)
    if training:
        with torch.no_grad():
            u.copy_(un)
            v.copy_(vn)
    return wsn0 if second is None else (wsn0, wsn1)


# --------------------------------------------------------------------------------------------------------------
# fused Adam on a flat buffer
# --------------------------------------------------------------------------------------------------------------
def adam_step_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step_state: Tensor, lr: float, beta1: float,
               beta2: float, eps: float, grad_scale: float = 1.0) -> None:
    """One fused Adam step over a flat buffer.  `step_state` is the optimiser's 4-element int32 device tensor: the kernel
    advances the step count in it and derives the bias corrections on the device (graph-replay safe)."""
    for t in (param, grad, exp_avg, exp_avg_sq):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise L.AganError("adam_step_: flat contiguous float32 device buffers required")
    if not step_state.is_cuda or step_state.dtype != torch.int32 or step_state.numel() < 4:
        raise L.AganError("adam_step_: step_state must be an int32 device tensor of 4 elements")
    L.call("agan_adam_step", _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), param.numel(), _p(step_state), float(lr),
           float(beta1), float(beta2), float(eps), float(grad_scale), _stream())
    mark_flat_written(param)


# --------------------------------------------------------------------------------------------------------------
# exponential moving average of weights over a segment table (include/agan.h: agan_ema_update; optim.FlatEMA)
# --------------------------------------------------------------------------------------------------------------
_EMA_SEG_DTYPE = [("src", "<u8"), ("dst", "<u8"), ("n", "<i8"), ("first_block", "<i4"), ("reserved", "<i4")]      # include/agan.h: agan_ema_seg


def ema_table(pairs, device) -> Tuple[Tensor, int, int]:
    """(device table, nseg, total_blocks) for `pairs` = [(src address, dst address, floats), ...]: checked and planned on the host
    (agan_ema_plan), one H2D copy."""
    import numpy as np
    pairs = list(pairs)
    segs = np.zeros(len(pairs), dtype=_EMA_SEG_DTYPE)
    for i, (src, dst, n) in enumerate(pairs):
        segs[i] = (int(src), int(dst), int(n), 0, 0)
    total = L.load().agan_ema_plan(c_void_p(segs.ctypes.data), len(pairs))
    if total <= 0:
        L.check(total if total < 0 else L.EINVAL, "agan_ema_plan")
    return torch.from_numpy(segs.view(np.uint8).copy()).to(device), len(pairs), int(total)


def mark_flat_written(flat: Tensor) -> None:
    """A kernel wrote `flat` through its raw pointer: packed copies of its views are stale (what adam_step_ and ema_update_ do after
    their launch; a replayed HIP graph that holds such a launch needs it said once per replay)."""
    rng = _flat_range(flat.data_ptr())
    if rng is not None:
        rng.written()
    else:
        bump_weight_epoch()


def ema_update_(table: Tensor, nseg: int, total_blocks: int, state: Tensor, decay: float, warmup: bool, flat_dst: Tensor) -> None:
    """One averaging update dst += (1 - beta_t) * (src - dst) over every segment of `table` (ema_table).  `state` is the average's
    4-element int32 device tensor: the kernel reads the update count t from it, derives beta_t on the device and advances the
    count (graph-replay safe).  `flat_dst` is the flat buffer among the destinations whose views are conv / linear weights."""
    if not table.is_cuda or table.dtype != torch.uint8 or not table.is_contiguous() or table.numel() < 32 * int(nseg):
        raise L.AganError("ema_update_: the segment table must be a contiguous uint8 device tensor of 32 bytes per segment")
    if not state.is_cuda or state.dtype != torch.int32 or state.numel() < 4:
        raise L.AganError("ema_update_: state must be an int32 device tensor of 4 elements")
    if not flat_dst.is_cuda or flat_dst.dtype != torch.float32 or not flat_dst.is_contiguous():
        raise L.AganError("ema_update_: flat contiguous float32 device buffer required")
    L.call("agan_ema_update", _p(table), int(nseg), int(total_blocks), _p(state), float(decay), int(bool(warmup)), _stream())
    mark_flat_written(flat_dst)


def ema_beta(t: int, decay: float, warmup: bool = True) -> float:
    """beta_t of update number t (0-based), in double as the tick kernel forms it"""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def ema_reference(src: Tensor, dst: Tensor, t: int, decay: float, warmup: bool = True) -> Tensor:
    """float64 oracle of update number t: dst + omb * (src - dst) with the SAME fp32-rounded omb = float32(1 - beta_t) the kernel uses,
    everything else in double.  Returns a new tensor."""
    omb = float(torch.tensor(1.0 - ema_beta(t, decay, warmup), dtype=torch.float64).to(torch.float32))
    d = dst.detach().double()
    return d + omb * (src.detach().double() - d)


# --------------------------------------------------------------------------------------------------------------
# frozen Inception-v3 image-encoder trunk (networks/cnn_encoder.py::CNNEncoder, backend="hip"; eval mode only)
# --------------------------------------------------------------------------------------------------------------
# Each conv's eval-mode BatchNorm folds into its weights and a per-channel bias (w' = w*gamma*invstd, b' = beta - mean*gamma*invstd,
# invstd = 1/sqrt(running_var + eps)), followed by the ReLU epilogue of agan_conv2d_fwd.  The folded weights are packed once per
# direction and cached on the module; a conv is re-folded when any of its five tensors changed -- in-place version bump
# (load_state_dict, an in-place edit) or new storage (.to()): what _stamp shows.  The trunk runs in fp32 in every
# precision mode (agan_conv2d_effective_prec).  The layer plan (which tensors, slices, write/accumulate order) is
# networks/inception_plan.py.
def _conv2d_desc(op, B: int) -> "L.Conv2dDesc":
    d = L.Conv2dDesc()
    d.B, d.Cin, d.IH, d.IW, d.Cout, d.OH, d.OW = B, op.C, op.H, op.W, op.Cout, op.OH, op.OW
    d.KH, d.KW = op.k
    d.SH, d.SW = op.s
    d.PH, d.PW = op.p
    d.in_c0, d.in_ctot, d.out_c0, d.out_ctot = 0, op.C, op.out_c0, op.out_ctot
    return d


_CONV2D_KTABLES = {}


def conv2d_ktable(d: "L.Conv2dDesc", dgrad: int, device) -> Tensor:
    """k-table of a general conv descriptor and direction (agan_conv2d_ktable), built once per (geometry, device)."""
    key = (tuple(getattr(d, n) for n, _ in L.Conv2dDesc._fields_), dgrad, str(device))
    t = _CONV2D_KTABLES.get(key)
    if t is None:
        n = L.load().agan_conv2d_ktable_elems(byref(d), dgrad)
        if n == 0:
            raise L.AganError(f"conv2d: no k-table for this geometry ({L.load().agan_last_error().decode()})")
        t = torch.empty(n, dtype=torch.int32, device=device)
        L.call("agan_conv2d_ktable", byref(d), dgrad, _p(t), _stream())
        _CONV2D_KTABLES[key] = t
    return t


def conv2d_pack(w: Tensor, d: "L.Conv2dDesc", dgrad: int) -> Tensor:
    """pack an OIHW fp32 weight for one direction of a general conv (agan_conv2d_pack_mode picks the layout)"""
    mode = L.load().agan_conv2d_pack_mode(byref(d), dgrad)
    if mode < 0:
        raise L.AganError(f"conv2d: {L.load().agan_last_error().decode()}")
    cout, cin, kh, kw = w.shape
    wk = torch.empty(L.load().agan_packed_weight_bytes(mode, cout, cin, kh, kw, L.PREC_F32), dtype=torch.uint8, device=w.device)
    L.call("agan_pack_weight", _p(w), _p(wk), mode, cout, cin, kh, kw, L.PREC_F32, _stream())
    return wk


def _trunk_layer(module, op, device):
    """(folded bias, packed forward weight, packed data-gradient weight) of one conv of the plan, re-folded when stale"""
    m = module.get_submodule(op.name)
    ts = (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)
    ver = tuple(_stamp(t) for t in ts) + (float(m.bn.eps), str(device))
    cache = module.__dict__.setdefault("_agan_trunk_fold", {})
    was, val = cache.get(op.name, (None, None))
    if was == ver:
        return val
    w, gamma, beta, mean, var = (_dev(t.detach(), f"trunk {op.name}") for t in ts)
    with torch.no_grad():
        scale = gamma * torch.rsqrt(var + m.bn.eps)
        wf = (w * scale.view(-1, 1, 1, 1)).contiguous()
        bf = (beta - mean * scale).contiguous()
    d = _conv2d_desc(op, 1)
    val = (bf, conv2d_pack(wf, d, 0), conv2d_pack(wf, d, 1))
    cache[op.name] = (ver, val)
    return val


def _trunk_forward(image: Tensor, plan, conv_fwd) -> Tuple[Dict[str, Tensor], Dict[int, Tensor]]:
    """the forward walk of the plan shared by both trunk modes: conv_fwd(i, op, src, dst) runs a conv op, the pools / resize / global
    mean run here.  -> (every tensor of the plan by name, max-pool argmax bytes by op index)"""
    B, dev = image.shape[0], image.device
    st = _stream()
    T: Dict[str, Tensor] = {"image": image}
    argmax: Dict[int, Tensor] = {}
    for i, op in enumerate(plan.ops):
        dst = T.get(op.dst)
        if dst is None:
            t = plan.tensors[op.dst]
            dst = T[op.dst] = torch.empty((B, t.C) if op.kind == "gap" else (B, t.C, t.H, t.W), device=dev)
        src = T[op.src]
        if op.kind == "conv":
            conv_fwd(i, op, src, dst)
        elif op.kind == "maxpool":
            am = argmax[i] = torch.empty(B * op.C * op.OH * op.OW, dtype=torch.uint8, device=dev)
            L.call("agan_maxpool3s2_fwd", _p(src), _p(dst), _p(am), B, op.C, op.H, op.W, op.out_c0, op.out_ctot, st)
        elif op.kind == "avgpool":
            L.call("agan_avgpool3s1_fwd", _p(src), _p(dst), B, op.C, op.H, op.W, st)
        elif op.kind == "gap":
            L.call("agan_global_avgpool_fwd", _p(src), _p(dst), B, op.C, op.H * op.W, st)
        else:   # resize
            L.call("agan_resize_bilinear_fwd", _p(src), _p(dst), B, op.C, op.H, op.W, op.OH, op.OW, st)
    return T, argmax


def _trunk_backward(plan, B: int, masks: Dict[str, Tensor], argmax: Dict[int, Tensor], g_feat: Optional[Tensor],
                    g_pooled: Optional[Tensor], conv_bwd) -> Tensor:
    """the reversed walk of the plan shared by both trunk modes -> the image gradient.  conv_bwd(i, op, gy, gx, mask, acc) runs a conv
    op's data gradient: gy is the whole gradient of op.dst (the op reads its slice), gx that of op.src, written (acc 0) or added to."""
    from ..networks.inception_plan import FEATURES, POOLED
    feat = masks[FEATURES]
    dev, st = feat.device, _stream()
    G: Dict[str, Tensor] = {}
    # the external gradient of the Mixed_6e output seeds its buffer (masked by its ReLU); Mixed_7a's ops then add
    G[FEATURES] = torch.empty_like(feat)
    if g_feat is None:
        G[FEATURES].zero_()
    else:
        g_feat = _dev(g_feat, "trunk backward")
        L.call("agan_relu_bwd", _p(feat), _p(g_feat), _p(G[FEATURES]), feat.numel(), 0, st)
    G[POOLED] = torch.zeros(B, plan.tensors[POOLED].C, device=dev) if g_pooled is None else _dev(g_pooled, "trunk backward")
    first_producer = {}
    for i, op in enumerate(plan.ops):
        first_producer.setdefault(op.dst, i)
    for i in range(len(plan.ops) - 1, -1, -1):
        op = plan.ops[i]
        gy = G[op.dst] if first_producer[op.dst] != i else G.pop(op.dst)     # (the last reader of this gradient frees it)
        gx = G.get(op.src)
        if gx is None:
            t = plan.tensors[op.src]
            gx = G[op.src] = torch.empty(B, t.C, t.H, t.W, device=dev)
        mask = masks.get(op.src)
        acc = int(op.accumulate)
        if op.kind == "conv":
            conv_bwd(i, op, gy, gx, mask, acc)
        elif op.kind == "maxpool":
            L.call("agan_maxpool3s2_bwd", _p(gy), _p(argmax[i]), _p(mask), _p(gx), B, op.C, op.H, op.W, op.out_c0, op.out_ctot,
                   acc, st)
        elif op.kind == "avgpool":
            L.call("agan_avgpool3s1_bwd", _p(gy), _p(mask), _p(gx), B, op.C, op.H, op.W, acc, st)
        elif op.kind == "gap":
            L.call("agan_global_avgpool_bwd", _p(gy), _p(mask), _p(gx), B, op.C, op.H * op.W, acc, st)
        else:   # resize: the image is the first and only reader of nothing else -- a plain write
            L.call("agan_resize_bilinear_bwd", _p(gy), _p(gx), B, op.C, op.H, op.W, op.OH, op.OW, st)
    return G["image"]


class _InceptionTrunkFn(Function):
    """image [B,3,H,W] -> (Mixed_6e output [B,768,17,17], pooled Mixed_7c [B,2048]); backward: the image gradient only."""

    @staticmethod
    def forward(ctx, image: Tensor, module, plan):
        image = _dev(image, "inception trunk")
        B, dev, st = image.shape[0], image.device, _stream()

        def conv_fwd(i, op, src, dst):
            d = _conv2d_desc(op, B)
            bias, wk, _ = _trunk_layer(module, op, dev)
            L.call("agan_conv2d_fwd", _p(src), _p(wk), _p(bias), _p(dst), byref(d), _p(conv2d_ktable(d, 0, dev)), L.ACT_RELU, None, 0, st)
        T, argmax = _trunk_forward(image, plan, conv_fwd)
        ctx.module, ctx.plan, ctx.B = module, plan, B
        ctx.masks = {n: T[n] for n, t in plan.tensors.items() if t.relu}      # the ReLU outputs: masks of the backward
        ctx.argmax = argmax
        from ..networks.inception_plan import FEATURES, POOLED
        return T[FEATURES], T[POOLED]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_feat: Optional[Tensor], g_pooled: Optional[Tensor]):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        B, st = ctx.B, _stream()

        def conv_bwd(i, op, gy, gx, mask, acc):
            d = _conv2d_desc(op, B)
            _, _, wkd = _trunk_layer(ctx.module, op, gx.device)
            L.call("agan_conv2d_dgrad", _p(gy), _p(wkd), _p(gx), byref(d), _p(conv2d_ktable(d, 1, gx.device)), _p(mask), acc, None, 0, st)
        gimg = _trunk_backward(ctx.plan, B, ctx.masks, ctx.argmax, g_feat, g_pooled, conv_bwd)
        ctx.masks = ctx.argmax = None
        return gimg, None, None


def inception_trunk(image: Tensor, module) -> Tuple[Tensor, Tensor]:
    """Eval-mode Inception-v3 trunk of `module` (a networks.cnn_encoder.CNNEncoder) on the library's kernels:
    image [B,3,H,W] -> (Mixed_6e output [B,768,17,17], global average of Mixed_7c [B,2048]), differentiable w.r.t. the image."""
    from ..networks.inception_plan import build_plan
    plan = build_plan(image.shape[-2], image.shape[-1])
    return _InceptionTrunkFn.apply(image, module, plan)


# ---- train mode: batch-statistics BatchNorm (CNNEncoder(backend="hip", hip_train=True)) ------------------------------------------
# Each conv runs UNFOLDED (agan_conv2d_fwd, no bias, no activation) into a contiguous raw buffer; agan_bn_relu_slice_fwd takes the batch
# statistics, updates the running ones and writes relu(BN(raw)) into the conv's slice of its destination.  The backward runs
# agan_bn_slice_bwd from the slice of the block gradient (already masked by the ReLU) into a scratch buffer, then the unfolded data
# gradient.  Trunk weights are frozen (no weight gradients); the image gradient is returned.  The unfolded packed weights are cached per
# conv and direction, keyed on the weight's storage and version -- a cache of their own, apart from the eval fold.
def _conv2d_raw_desc(op, B: int) -> "L.Conv2dDesc":
    """the descriptor of a conv that writes all of a contiguous [B, Cout, OH, OW] buffer"""
    d = _conv2d_desc(op, B)
    d.out_c0, d.out_ctot = 0, op.Cout
    return d


def _trunk_train_weight(module, op, dgrad: int, device) -> Tensor:
    """the unfolded conv weight of one conv of the plan, packed for one direction; re-packed when the weight changed"""
    w = module.get_submodule(op.name).conv.weight
    ver = _stamp(w) + (str(device),)
    cache = module.__dict__.setdefault("_agan_trunk_train_w", {})
    was, wk = cache.get((op.name, dgrad), (None, None))
    if was == ver:
        return wk
    wk = conv2d_pack(_dev(w.detach(), f"trunk {op.name}"), _conv2d_raw_desc(op, 1), dgrad)
    cache[(op.name, dgrad)] = (ver, wk)
    return wk


def _bn_buffer(t: Optional[Tensor], dtype, what: str) -> Tensor:
    """a running-statistics buffer the kernel updates in place: it must already be a contiguous device tensor of `dtype`"""
    if t is None or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise L.AganError(f"{what}: running statistics must be contiguous {dtype} device tensors")
    return t


class _InceptionTrunkTrainFn(Function):
    """train-mode trunk: image [B,3,H,W] -> (Mixed_6e output, pooled Mixed_7c); the BatchNorm running statistics of `module` are
    updated; backward: the image gradient only.  `save` False (no_grad, or an image without a gradient) keeps nothing for a backward
    and reuses one raw buffer for every conv."""

    @staticmethod
    def forward(ctx, image: Tensor, module, plan, save: bool):
        image = _dev(image, "inception trunk (train)")
        B, dev, st = image.shape[0], image.device, _stream()
        convs = plan.convs()
        ws_n = max(L.load().agan_bn_relu_slice_fwd_ws_bytes(B, op.Cout, op.OH * op.OW) for op in convs)
        wst, ws = _ws(ws_n, image)
        raws: Dict[int, Tensor] = {}
        stats: Dict[int, Tuple[Tensor, Tensor, Tensor]] = {}
        bumped = []
        if not save:
            raw_scratch = torch.empty(max(B * op.Cout * op.OH * op.OW for op in convs), device=dev)
            stat_scratch = torch.empty(2, max(op.Cout for op in convs), device=dev)

        def conv_fwd(i, op, src, dst):
            bn = module.get_submodule(op.name).bn
            what = f"trunk {op.name}"
            gamma, beta = _dev(bn.weight.detach(), what), _dev(bn.bias.detach(), what)
            rm = _bn_buffer(bn.running_mean, torch.float32, what)
            rv = _bn_buffer(bn.running_var, torch.float32, what)
            nbt = _bn_buffer(bn.num_batches_tracked, torch.int64, what)
            d = _conv2d_raw_desc(op, B)
            HW = op.OH * op.OW
            if save:
                raw = raws[i] = torch.empty(B, op.Cout, op.OH, op.OW, device=dev)
                mean, invstd = torch.empty(op.Cout, device=dev), torch.empty(op.Cout, device=dev)
                stats[i] = (mean, invstd, gamma)
            else:
                raw, mean, invstd = raw_scratch[:B * op.Cout * HW], stat_scratch[0, :op.Cout], stat_scratch[1, :op.Cout]
            L.call("agan_conv2d_fwd", _p(src), _p(_trunk_train_weight(module, op, 0, dev)), None, _p(raw), byref(d),
                   _p(conv2d_ktable(d, 0, dev)), L.ACT_NONE, None, 0, st)
            L.call("agan_bn_relu_slice_fwd", _p(raw), _p(gamma), _p(beta), _p(dst), op.out_c0, op.out_ctot, _p(mean), _p(invstd),
                   _p(rm), _p(rv), _p(nbt), B, op.Cout, HW, float(bn.eps), float(bn.momentum), ws, ws_n, st)
            bumped.extend((rm, rv, nbt))
        T, argmax = _trunk_forward(image, plan, conv_fwd)
        # the kernels wrote the running statistics behind autograd's back: bump their versions (the eval fold keys on them)
        torch.autograd.graph.increment_version(bumped)
        from ..networks.inception_plan import FEATURES, POOLED
        ctx.plan, ctx.B, ctx.module = plan, B, module
        if save:
            # (the Mixed_6e output is also a mask: kept through save_for_backward, as an attribute it would tie the output to its own
            # graph in a reference cycle that only the garbage collector frees)
            ctx.masks = {n: T[n] for n, t in plan.tensors.items() if t.relu and n != FEATURES}
            ctx.save_for_backward(T[FEATURES])
            ctx.argmax, ctx.raws, ctx.stats = argmax, raws, stats
        else:
            ctx.masks = ctx.argmax = ctx.raws = ctx.stats = None
        return T[FEATURES], T[POOLED]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_feat: Optional[Tensor], g_pooled: Optional[Tensor]):
        if not ctx.needs_input_grad[0] or ctx.raws is None:
            return None, None, None, None
        from ..networks.inception_plan import FEATURES
        B, st = ctx.B, _stream()
        feat, = ctx.saved_tensors
        masks = dict(ctx.masks, **{FEATURES: feat})
        convs = ctx.plan.convs()
        dev = feat.device
        ws_n = max(L.load().agan_bn_slice_bwd_ws_bytes(B, op.Cout, op.OH * op.OW) for op in convs)
        wst, ws = _ws(ws_n, feat)
        dz = torch.empty(max(B * op.Cout * op.OH * op.OW for op in convs), device=dev)      # one scratch for every conv

        def conv_bwd(i, op, gy, gx, mask, acc):
            raw = ctx.raws.pop(i)
            mean, invstd, gamma = ctx.stats.pop(i)
            d = _conv2d_raw_desc(op, B)
            L.call("agan_bn_slice_bwd", _p(raw), _p(gy), op.out_c0, op.out_ctot, _p(mean), _p(invstd), _p(gamma), _p(dz),
                   B, op.Cout, op.OH * op.OW, ws, ws_n, st)
            L.call("agan_conv2d_dgrad", _p(dz), _p(_trunk_train_weight(ctx.module, op, 1, dev)), _p(gx), byref(d),
                   _p(conv2d_ktable(d, 1, dev)), _p(mask), acc, None, 0, st)
        gimg = _trunk_backward(ctx.plan, B, masks, ctx.argmax, g_feat, g_pooled, conv_bwd)
        ctx.masks = ctx.argmax = ctx.raws = ctx.stats = None
        return gimg, None, None, None


def inception_trunk_train(image: Tensor, module) -> Tuple[Tensor, Tensor]:
    """Train-mode Inception-v3 trunk of `module` on the library's kernels: batch-statistics BatchNorm (the running statistics are
    updated as torch's train-mode BatchNorm does), same outputs as inception_trunk, differentiable w.r.t. the image.  The trunk's
    parameters must be frozen (no weight gradients)."""
    from ..networks.inception_plan import build_plan
    plan = build_plan(image.shape[-2], image.shape[-1])
    save = torch.is_grad_enabled() and image.requires_grad
    return _InceptionTrunkTrainFn.apply(image, module, plan, save)


# --------------------------------------------------------------------------------------------------------------
# caption encoder (networks/rnn_encoder.py::RNNEncoder, backend="hip"; train and eval mode)
# --------------------------------------------------------------------------------------------------------------
# embedding gather -> (the module's dropout) -> input projection per direction on `linear` (packed W_ih cached per direction by
# packed_weight; fp32: a linear layer is a 1x1 geometry, which every precision mode runs in fp32) -> one recurrence launch
# for both directions (agan_lstm_fwd).  Backward: agan_lstm_bwd (gate gradients) + agan_lstm_wgrad (W_hh, b_hh), the projections'
# own backward (W_ih, b_ih, data) and agan_embedding_bwd.  Nothing is atomic.
class _EmbeddingFn(Function):
    @staticmethod
    def forward(ctx, weight: Tensor, ids: Tensor, T: int):
        w = _dev(weight.detach(), "embedding weight")
        if not ids.is_cuda or ids.dtype != torch.int64 or ids.dim() != 2 or ids.stride(1) != 1:
            raise L.AganError(f"embedding: ids must be a [B, T] int64 device tensor with unit column stride, got {ids.dtype} "
                              f"{tuple(ids.shape)} on {ids.device}")
        B = ids.shape[0]
        V, E = w.shape
        y = torch.empty(B, T, E, device=w.device)
        L.call("agan_embedding_fwd", _p(ids), ids.stride(0), _p(w), _p(y), B, T, V, E, _stream())
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(ids)
        ctx.V = V
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy: Tensor):
        (ids,) = ctx.saved_tensors
        dy = _dev(dy, "embedding grad")
        B, T, E = dy.shape
        dw = torch.empty(ctx.V, E, device=dy.device)
        L.call("agan_embedding_bwd", _p(ids), ids.stride(0), _p(dy), _p(dw), B, T, ctx.V, E, _stream())
        return dw, None, None


def embedding(ids: Tensor, weight: Tensor, T: int) -> Tensor:
    """weight[ids[:, :T]] -> [B, T, E]; an id outside the table gives a zero row (include/agan.h: agan_embedding_fwd)"""
    return _EmbeddingFn.apply(weight, ids, T)


class _LSTMFn(Function):
    """(lens, save, xg_0, W_hh_0, b_hh_0[, xg_1, W_hh_1, b_hh_1]) -> (out [B, T, D*H], hN [B, D*H])"""

    @staticmethod
    def forward(ctx, lens: Tensor, save: bool, *tensors: Tensor):
        D = len(tensors) // 3
        xg = [_dev(t, "lstm input projection") for t in tensors[0::3]]
        whh = [_dev(t.detach(), "lstm weight_hh") for t in tensors[1::3]]
        bhh = [_dev(t.detach(), "lstm bias_hh") for t in tensors[2::3]]
        B, T, G = xg[0].shape
        H = G // 4
        dev = xg[0].device
        out = torch.empty(B, T, D * H, device=dev)
        hN = torch.empty(B, D * H, device=dev)
        gates = torch.empty(D, B, T, G, device=dev) if save else None
        cells = torch.empty(D, B, T, H, device=dev) if save else None
        two = D == 2
        L.call("agan_lstm_fwd", _p(xg[0]), _p(xg[1] if two else None), _p(whh[0]), _p(whh[1] if two else None), _p(bhh[0]),
               _p(bhh[1] if two else None), _p(lens), _p(out), _p(hN), _p(gates), _p(cells), B, T, H, D, _stream())
        if save:
            ctx.save_for_backward(lens, out, gates, cells, *whh)
        ctx.dims = (B, T, H, D)
        return out, hN

    @staticmethod
    @once_differentiable
    def backward(ctx, dout: Optional[Tensor], dhN: Optional[Tensor]):
        lens, out, gates, cells, *whh = ctx.saved_tensors
        B, T, H, D = ctx.dims
        two = D == 2
        dout = _dev(dout, "lstm grad") if dout is not None else None
        dhN = _dev(dhN, "lstm grad") if dhN is not None else None
        dg = torch.empty(D, B, T, 4 * H, device=out.device)
        L.call("agan_lstm_bwd", _p(dout), _p(dhN), _p(whh[0]), _p(whh[1] if two else None), _p(gates), _p(cells), _p(lens), _p(dg[0]),
               _p(dg[1] if two else None), B, T, H, D, _stream())
        need_w = any(ctx.needs_input_grad[3 + 3 * d] or ctx.needs_input_grad[4 + 3 * d] for d in range(D))
        dwhh = dbhh = None
        if need_w:
            dwhh = torch.empty(D, 4 * H, H, device=out.device)
            dbhh = torch.empty(D, 4 * H, device=out.device)
            L.call("agan_lstm_wgrad", _p(dg[0]), _p(dg[1] if two else None), _p(out), _p(dwhh), _p(dbhh), B, T, H, D, _stream())
        grads = []
        for d in range(D):
            grads += [dg[d], dwhh[d] if dwhh is not None else None, dbhh[d] if dbhh is not None else None]
        return (None, None, *grads)


def lstm(xg, whh, bhh, lens: Tensor, save: bool) -> Tuple[Tensor, Tensor]:
    """One LSTM layer over [B, T, 4H] input projections, one per direction (include/agan.h: agan_lstm_fwd).  lens: int32 [B] on
    the device.  save: keep the gates and cells for a backward (False under no_grad or with everything frozen)."""
    args = []
    for x, w, b in zip(xg, whh, bhh):
        args += [x, w, b]
    return _LSTMFn.apply(lens, save, *args)


def image_prep(planes, rows: Optional[Tensor], flip: Optional[Tensor], out=None):
    """Batch preparation from resident uint8 images in ONE launch (include/agan.h: agan_image_prep).

    planes: 1..3 entries, each a uint8 device tensor [n_src, C, H, W] (direct plane) or, after the first, an (H, W) pair: a plane
    resampled from plane 0 (exactly / 2 or / 4, antialiased bilinear).  rows: int32 device [B] (None = 0..B-1), flip: uint8 device [B]
    (None = no mirror).  out: the fp32 [B, C, H, W] tensors to write (None = new ones).  Returns the list of outputs: images in
    [-1, 1], bit-identical to data.batches.scale_255_to_1 on direct planes.  No autograd: images are inputs."""
    planes = list(planes)
    src0 = planes[0] if planes else None
    if not isinstance(src0, Tensor):
        raise L.AganError("image_prep: plane 0 must be a uint8 tensor [n_src, C, H, W]")
    for t, what, dtype in ((src0, "plane 0", torch.uint8), (rows, "rows", torch.int32), (flip, "flip", torch.uint8)):
        if t is not None and not t.is_cuda:
            raise L.AganError(f"image_prep {what}: tensor is on {t.device}; the AttnGAN HIP path runs on an MI355X only (no CPU fallback)")
        if t is not None and (t.dtype != dtype or not t.is_contiguous()):
            raise L.AganError(f"image_prep {what}: expected a contiguous {dtype} tensor, got {t.dtype}")
    if src0.dim() != 4:
        raise L.AganError(f"image_prep plane 0: expected [n_src, C, H, W], got {tuple(src0.shape)}")
    n_src, C = int(src0.shape[0]), int(src0.shape[1])
    B = int(rows.numel()) if rows is not None else (int(out[0].shape[0]) if out is not None else n_src)
    if flip is not None and int(flip.numel()) != B:
        raise L.AganError(f"image_prep flip: {int(flip.numel())} entries for a batch of {B}")
    if out is not None and len(out) != len(planes):
        raise L.AganError(f"image_prep out: {len(out)} tensors for {len(planes)} planes")
    arr = (L.ImagePlane * max(1, len(planes)))()
    outs = []
    for i, p in enumerate(planes):
        if isinstance(p, Tensor):
            if p.device != src0.device or p.dtype != torch.uint8 or not p.is_contiguous() or p.dim() != 4 or tuple(p.shape[:2]) != (n_src, C):
                raise L.AganError(f"image_prep plane {i}: expected a contiguous uint8 [{n_src}, {C}, H, W] tensor on {src0.device}")
            H, W = int(p.shape[2]), int(p.shape[3])
            arr[i].src = p.data_ptr()
        else:
            H, W = (int(v) for v in p)
            arr[i].src = None
        shape = (B, C, H, W)
        o = torch.empty(shape, device=src0.device) if out is None else out[i]
        if o.device != src0.device or o.dtype != torch.float32 or not o.is_contiguous() or tuple(o.shape) != shape:
            raise L.AganError(f"image_prep out[{i}]: expected a contiguous float32 {shape} tensor on {src0.device}")
        arr[i].dst, arr[i].H, arr[i].W = o.data_ptr(), H, W
        outs.append(o)
    L.call("agan_image_prep", arr, len(planes), _p(rows), _p(flip), B, C, n_src, _stream())
    return outs


# --------------------------------------------------------------------------------------------------------------
# differentiable augmentation (augment.py; include/agan.h: agan_diffaug_*)
# --------------------------------------------------------------------------------------------------------------
def _diffaug_bwd(dy: Tensor, u: Tensor, policy: int, q: Optional[Tensor] = None, p: Optional[Tensor] = None) -> Tensor:
    N, C, H, W = dy.shape
    dx = torch.empty_like(dy)
    nbytes = L.load().agan_diffaug_ws_bytes(N, C, H, W)
    ws, wsp = _ws(nbytes, dy)
    if q is None:
        _kmeans_call("agan_diffaug_bwd", _p(dy), _p(u), policy, _p(dx), N, C, H, W, wsp, nbytes, _stream())
    else:
        _kmeans_call("agan_diffaug_gated_bwd", _p(dy), _p(u), _p(q), _p(p), policy, _p(dx), N, C, H, W, wsp, nbytes, _stream())
    return dx


class _DiffAugFn(Function):
    @staticmethod
    def forward(ctx, u, policy, q, p, *xs):
        x0 = xs[0]
        x1 = xs[1] if len(xs) > 1 else None
        n0, C, H, W = x0.shape
        n1 = 0 if x1 is None else int(x1.shape[0])
        y = torch.empty((n0 + n1, C, H, W), dtype=torch.float32, device=x0.device)
        nbytes = L.load().agan_diffaug_ws_bytes(n0 + n1, C, H, W)
        ws, wsp = _ws(nbytes, x0)
        if q is None:
            _kmeans_call("agan_diffaug_fwd", _p(x0), _p(x1), n0, n1, _p(u), policy, _p(y), C, H, W, wsp, nbytes, _stream())
        else:
            _kmeans_call("agan_diffaug_gated_fwd", _p(x0), _p(x1), n0, n1, _p(u), _p(q), _p(p), policy, _p(y), C, H, W, wsp, nbytes,
                         _stream())
        # (p is kept as the tensor it is, not through save_for_backward: the controller advances it in place between the forward
        # and the next step, never between a forward and ITS backward, and a version check would refuse the graph-replayed update)
        if q is None:
            ctx.save_for_backward(u)
        else:
            ctx.save_for_backward(u, q)
        ctx.p = p
        ctx.policy, ctx.sizes = policy, (n0, n1)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        u, q = ctx.saved_tensors if len(ctx.saved_tensors) == 2 else (ctx.saved_tensors[0], None)
        p = ctx.p
        n0, n1 = ctx.sizes
        need = list(ctx.needs_input_grad[4:])
        dy = _dev(dy, "diffaug dy")
        if all(need):                                     # one call over the whole batch, split per source
            dx = _diffaug_bwd(dy, u, ctx.policy, q, p)
            grads = [dx] if n1 == 0 else [dx[:n0], dx[n0:]]
        else:                                             # only the samples of the source that asks
            bounds = [(0, n0), (n0, n0 + n1)]
            grads = [_diffaug_bwd(dy[lo:hi], u[lo:hi], ctx.policy, None if q is None else q[lo:hi], p) if want else None
                     for want, (lo, hi) in zip(need, bounds)]
        return (None, None, None, None, *grads)


def diffaug(xs, u: Tensor, policy: int, q: Optional[Tensor] = None, p: Optional[Tensor] = None) -> Tensor:
    """DiffAugment of include/agan.h (agan_diffaug_fwd; augment.diffaug_reference states it in torch ops) on one [N, C, H, W] tensor
    or a PAIR of equal-shaped ones, whose samples come out concatenated in ONE tensor (the [real; fake] batch of
    NonSaturatingDiscLoss, written by the augmentation itself).  u: [N, 8] uniforms in [0, 1) for all samples of the result, policy:
    the bit mask of augment.parse_policy.  Differentiable in the images: the backward kernel runs for the sources that require grad.

    With `q` [N, 4] (uniforms) and `p` (a ONE-element fp32 device tensor) the gated entries run (agan_diffaug_gated_*): stage k of
    sample n is applied iff its policy bit is set and q[n, k] < p.  p is read by the kernels when they run -- forward and backward read
    the value of THEIR moment -- so a controller may change it in place between steps, inside a captured graph too."""
    xs = (xs,) if isinstance(xs, Tensor) else tuple(xs)
    if not 1 <= len(xs) <= 2:
        raise ValueError(f"diffaug: expected one tensor or a pair, got {len(xs)}")
    xs = tuple(_dev(x, "diffaug x") for x in xs)
    if xs[0].dim() != 4 or any(x.shape != xs[0].shape or x.device != xs[0].device for x in xs):
        raise ValueError(f"diffaug: expected [N, C, H, W] tensors of one shape on one device, got {[tuple(x.shape) for x in xs]}")
    n = sum(int(x.shape[0]) for x in xs)
    u = _dev(u, "diffaug u")
    if u.device != xs[0].device or tuple(u.shape) != (n, 8):
        raise ValueError(f"diffaug: u must be [{n}, 8] on {xs[0].device}, got {tuple(u.shape)} on {u.device}")
    if (q is None) != (p is None):
        raise ValueError("diffaug: q and p come together (the gated form) or not at all")
    if q is not None:
        q = _dev(q, "diffaug q")
        if q.device != xs[0].device or tuple(q.shape) != (n, 4):
            raise ValueError(f"diffaug: q must be [{n}, 4] on {xs[0].device}, got {tuple(q.shape)} on {q.device}")
        if not p.is_cuda or p.device != xs[0].device or p.dtype != torch.float32 or p.numel() != 1:
            raise ValueError(f"diffaug: p must be a one-element float32 tensor on {xs[0].device}, got {p.dtype} {tuple(p.shape)} on {p.device}")
    return _DiffAugFn.apply(u, int(policy), q, p, *xs)


# --------------------------------------------------------------------------------------------------------------
# geometric augmentation (augment.py: geometry_matrices_reference, affine_warp_reference; include/agan.h: agan_geoaug_matrix,
# agan_affine_warp_*)
# --------------------------------------------------------------------------------------------------------------
def geometry_matrices(g: Tensor, geometry: int, p: Optional[Tensor] = None) -> Tensor:
    """M [N, 6] of include/agan.h (agan_geoaug_matrix) from the uniforms g [N, 16] and the stage mask of augment.parse_geometry: ONE
    launch, one thread per sample.  With `p` (a ONE-element fp32 device tensor, read when the kernel runs) stage k of sample n applies
    iff its bit is set and g[n, 8 + k] < p; without it every enabled stage applies."""
    g = _dev(g.detach(), "geometry_matrices g")
    if g.dim() != 2 or g.shape[1] != L.GEOAUG_UNIFORMS or g.shape[0] < 1:
        raise ValueError(f"geometry_matrices: g must be [N, {L.GEOAUG_UNIFORMS}], got {tuple(g.shape)}")
    if p is not None and (not p.is_cuda or p.device != g.device or p.dtype != torch.float32 or p.numel() != 1):
        raise ValueError(f"geometry_matrices: p must be a one-element float32 tensor on {g.device}, got {p.dtype} {tuple(p.shape)} on {p.device}")
    M = torch.empty((g.shape[0], 6), dtype=torch.float32, device=g.device)
    _kmeans_call("agan_geoaug_matrix", _p(g), _p(p), int(geometry), _p(M), int(g.shape[0]), _stream())
    return M


def _affine_warp_bwd(dy: Tensor, M: Tensor) -> Tensor:
    N, C, H, W = dy.shape
    dx = torch.empty_like(dy)
    _kmeans_call("agan_affine_warp_bwd", _p(dy), _p(M), _p(dx), N, C, H, W, _stream())
    return dx


class _AffineWarpFn(Function):
    @staticmethod
    def forward(ctx, M, *xs):
        x0 = xs[0]
        x1 = xs[1] if len(xs) > 1 else None
        n0, C, H, W = x0.shape
        n1 = 0 if x1 is None else int(x1.shape[0])
        y = torch.empty((n0 + n1, C, H, W), dtype=torch.float32, device=x0.device)
        _kmeans_call("agan_affine_warp_fwd", _p(x0), _p(x1), n0, n1, _p(M), _p(y), C, H, W, _stream())
        ctx.save_for_backward(M)
        ctx.sizes = (n0, n1)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        M, = ctx.saved_tensors
        n0, n1 = ctx.sizes
        need = list(ctx.needs_input_grad[1:])
        dy = _dev(dy, "affine_warp dy")
        if all(need):                                     # one call over the whole batch, split per source
            dx = _affine_warp_bwd(dy, M)
            grads = [dx] if n1 == 0 else [dx[:n0], dx[n0:]]
        else:                                             # only the samples of the source that asks
            bounds = [(0, n0), (n0, n0 + n1)]
            grads = [_affine_warp_bwd(dy[lo:hi], M[lo:hi]) if want else None for want, (lo, hi) in zip(need, bounds)]
        return (None, *grads)


def affine_warp(xs, M: Tensor) -> Tensor:
    """The bilinear affine warp of include/agan.h (agan_affine_warp_fwd; augment.affine_warp_reference states it in torch ops) on one
    [N, C, H, W] tensor or a PAIR of equal-shaped ones, whose samples come out concatenated in ONE tensor, as for diffaug.  M: [N, 6]
    = (a, b, tx, c, d, ty) per sample of the result, an output -> source map about the image centre; a tap outside the image reads
    zero.  Differentiable in the images (never in M): the backward is a gather with one summation order and no atomics, run for the
    sources that require grad.  The forward takes any finite matrix; the backward is specified for linear parts that shrink no axis
    below 1/16 (its candidate walk is clamped at 32 outputs either way per axis)."""
    xs = (xs,) if isinstance(xs, Tensor) else tuple(xs)
    if not 1 <= len(xs) <= 2:
        raise ValueError(f"affine_warp: expected one tensor or a pair, got {len(xs)}")
    xs = tuple(_dev(x, "affine_warp x") for x in xs)
    if xs[0].dim() != 4 or any(x.shape != xs[0].shape or x.device != xs[0].device for x in xs):
        raise ValueError(f"affine_warp: expected [N, C, H, W] tensors of one shape on one device, got {[tuple(x.shape) for x in xs]}")
    n = sum(int(x.shape[0]) for x in xs)
    M = _dev(M.detach(), "affine_warp M")
    if M.device != xs[0].device or tuple(M.shape) != (n, 6):
        raise ValueError(f"affine_warp: M must be [{n}, 6] on {xs[0].device}, got {tuple(M.shape)} on {M.device}")
    return _AffineWarpFn.apply(M, *xs)


# --------------------------------------------------------------------------------------------------------------
# the controller of the augmentation probability (augment.py: AdaController; include/agan.h: agan_ada_*)
# --------------------------------------------------------------------------------------------------------------
def _ada_words(t: Tensor, words: int, what: str) -> None:
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < words:
        raise L.AganError(f"{what} must be a contiguous int32 device tensor of at least {words} elements")


def ada_observe_(score: Tensor, slot_view: Tensor, threshold: float = 0.5) -> None:
    """slot_view[0] = #(score > threshold) - #(score < threshold), slot_view[1] = score.numel(), written by one small launch on the
    current stream (include/agan.h: agan_ada_observe).  slot_view: the two int32 words of one discriminator's observation slot."""
    score = _dev(score.detach(), "ada_observe_ score").reshape(-1)
    _ada_words(slot_view, 2, "ada_observe_: the slot")
    if slot_view.device != score.device:
        raise L.AganError(f"ada_observe_: scores on {score.device}, slot on {slot_view.device}")
    _kmeans_call("agan_ada_observe", _p(score), int(score.numel()), float(threshold), _p(slot_view), _stream())


def ada_update_(state: Tensor, nslots: int, interval: int, target: float, rate: float, p_max: float) -> None:
    """One controller call on the 16-word state (include/agan.h: agan_ada_update): fold the observation slots into the window; at the
    end of every `interval`-th call move p (word 4) by count * rate towards r_t > target.  One one-thread launch, no host read."""
    _ada_words(state, L.ADA_STATE_WORDS, "ada_update_: state")
    _kmeans_call("agan_ada_update", _p(state), int(nslots), int(interval), float(target), float(rate), float(p_max), _stream())


# --------------------------------------------------------------------------------------------------------------
# k-means (data/captions.py: kmeans; include/agan.h: agan_kmeans_*)
# --------------------------------------------------------------------------------------------------------------
# One Lloyd iteration is kmeans_assign + kmeans_update.  Device tensors run on the library; a CPU tensor takes the torch restatement
# below, which applies the same rules in float64 (lowest index on a tie, max(0, .) on the distance, out-of-range labels ignored, an
# empty cluster keeps its centroid) and rounds the centroids once to fp32 -- the host-side path of data/captions.py and its tests.
# Neither has autograd: clustering is data preparation.
def _kmeans_call(name: str, *args) -> None:
    """lib.call, with AGAN_EINVAL (a shape outside the documented domain) raised as ValueError"""
    lib = L.load()
    code = getattr(lib, name)(*args)
    if code == L.EINVAL:
        msg = lib.agan_last_error()
        raise ValueError(f"{name}: {msg.decode() if msg else 'bad argument'}")
    L.check(code, name)


def _kmeans_operands(x: Tensor, centroids: Tensor, what: str) -> Tuple[Tensor, Tensor]:
    if x.dim() != 2 or centroids.dim() != 2 or x.shape[1] != centroids.shape[1]:
        raise ValueError(f"{what}: expected x [N, D] and centroids [K, D], got {tuple(x.shape)} and {tuple(centroids.shape)}")
    if centroids.device != x.device:
        raise ValueError(f"{what}: x is on {x.device}, centroids on {centroids.device}")
    for t, n in ((x, "x"), (centroids, "centroids")):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {n} must be float32, got {t.dtype}")
    return x.contiguous(), centroids.contiguous()


def _kmeans_labels(labels: Tensor, x: Tensor, what: str) -> Tensor:
    if labels.dtype != torch.int32 or labels.shape != (x.shape[0],) or labels.device != x.device:
        raise ValueError(f"{what}: labels must be int32 [{x.shape[0]}] on {x.device}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}")
    return labels.contiguous()


_KMEANS_CPU_ROWS = 1 << 14          # rows per float64 score block of the CPU path


def kmeans_assign(x: Tensor, centroids: Tensor, labels: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (labels int32 [N], dist float32 [N], n_changed int32 [1], inertia float64 [1]), all on x's device.

    labels[i] = argmin_c (|c|^2 - 2 x_i.c), the lowest c on a tie; dist[i] = max(0, |x_i|^2 + that score); n_changed = rows whose
    label differs from `labels` (None: every row counts as changed); inertia = sum of dist in float64.  `labels` is not modified."""
    x, centroids = _kmeans_operands(x, centroids, "kmeans_assign")
    N, D = x.shape
    K = centroids.shape[0]
    prev = torch.full((N,), -1, dtype=torch.int32, device=x.device) if labels is None else _kmeans_labels(labels, x, "kmeans_assign")
    if not x.is_cuda:
        if N < 1 or not 1 <= D <= 4096 or not 1 <= K <= 4096 or N * D >= 1 << 31:
            raise ValueError(f"kmeans_assign: N {N}, D {D}, K {K} outside N >= 1, 1 <= D, K <= 4096, N * D < 2^31")
        c64 = centroids.double()
        cn = (c64 * c64).sum(1)
        new = torch.empty(N, dtype=torch.int32)
        dist = torch.empty(N, dtype=torch.float32)
        for s in range(0, N, _KMEANS_CPU_ROWS):
            x64 = x[s:s + _KMEANS_CPU_ROWS].double()
            score = cn.view(1, K) - 2.0 * (x64 @ c64.t())
            best = torch.from_numpy(score.numpy().argmin(axis=1))           # numpy: the first minimum
            d = ((x64 * x64).sum(1) + score.gather(1, best.view(-1, 1)).view(-1)).clamp_(min=0.0)
            new[s:s + _KMEANS_CPU_ROWS] = best.to(torch.int32)
            dist[s:s + _KMEANS_CPU_ROWS] = d.to(torch.float32)
        return new, dist, (new != prev).sum().to(torch.int32).view(1), dist.double().sum().view(1)
    new = prev.clone() if labels is not None else prev
    dist = torch.empty(N, dtype=torch.float32, device=x.device)
    n_changed = torch.empty(1, dtype=torch.int32, device=x.device)
    inertia = torch.empty(1, dtype=torch.float64, device=x.device)
    nbytes = L.load().agan_kmeans_assign_ws_bytes(N, D, K)
    ws, wsp = _ws(nbytes, x)
    _kmeans_call("agan_kmeans_assign", _p(x), _p(centroids), _p(new), _p(dist), _p(n_changed), _p(inertia), N, D, K, wsp, nbytes, _stream())
    return new, dist, n_changed, inertia


def kmeans_update(x: Tensor, labels: Tensor, centroids: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (centroids float32 [K, D], counts int32 [K]): counts[c] = rows with label c, centroids[c] = fp32(float64 mean of those rows);
    a cluster without rows keeps the centroid passed in; a label outside [0, K) is ignored.  `centroids` is not modified."""
    x, centroids = _kmeans_operands(x, centroids, "kmeans_update")
    labels = _kmeans_labels(labels, x, "kmeans_update")
    N, D = x.shape
    K = centroids.shape[0]
    if not x.is_cuda:
        if N < 1 or not 1 <= D <= 4096 or not 1 <= K <= 4096 or N * D >= 1 << 31:
            raise ValueError(f"kmeans_update: N {N}, D {D}, K {K} outside N >= 1, 1 <= D, K <= 4096, N * D < 2^31")
        lab = labels.long()
        ok = (lab >= 0) & (lab < K)
        counts = torch.bincount(lab[ok], minlength=K)
        sums = torch.zeros(K, D, dtype=torch.float64).index_add_(0, lab[ok], x[ok].double())
        mean = (sums / counts.clamp(min=1).view(K, 1).double()).to(torch.float32)
        return torch.where((counts > 0).view(K, 1), mean, centroids), counts.to(torch.int32)
    new = centroids.clone()
    counts = torch.empty(K, dtype=torch.int32, device=x.device)
    nbytes = L.load().agan_kmeans_update_ws_bytes(N, D, K)
    ws, wsp = _ws(nbytes, x)
    _kmeans_call("agan_kmeans_update", _p(x), _p(labels), _p(new), _p(counts), N, D, K, wsp, nbytes, _stream())
    return new, counts


# --------------------------------------------------------------------------------------------------------------
# evaluation reductions (evaluation.py: FeatureMoments, r_precision; include/agan.h: agan_moments_*, agan_retrieval_rank)
# --------------------------------------------------------------------------------------------------------------
# Device tensors run on the library; a CPU tensor takes the float64 torch restatement below with the same rules (upper-triangle state,
# count == 1 -> zero covariance, the clamp of the cosine's denominator, a tie counts against the match, a bad candidate is refused).
# None has autograd: these are measurements.
def _moments_state(sum: Tensor, gram: Tensor, D: int, device, what: str) -> None:
    for t, n, shape in ((sum, "sum", (D,)), (gram, "gram", (D, D))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
            raise ValueError(f"{what}: {n} must be a contiguous float64 {shape} tensor on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def moments_update(x: Tensor, sum: Tensor, gram: Tensor) -> Tuple[Tensor, Tensor]:
    """Adds the rows of x [n, D] float32 to the raw moments IN PLACE and returns them: sum [D] += column sums, gram [D, D] += x^T x on
    and above the diagonal (what lies below the diagonal is unspecified), both float64.  A fresh state is zeros."""
    if x.dim() != 2:
        raise ValueError(f"moments_update: expected x [n, D], got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"moments_update: x must be float32, got {x.dtype}")
    x = x.contiguous()
    n, D = x.shape
    _moments_state(sum, gram, D, x.device, "moments_update")
    if not x.is_cuda:
        if n < 1 or not 1 <= D <= 4096 or n * D >= 1 << 31:
            raise ValueError(f"moments_update: n {n}, D {D} outside n >= 1, 1 <= D <= 4096, n * D < 2^31")
        x64 = x.double()
        sum += x64.sum(0)
        gram += torch.triu(x64.t() @ x64)
        return sum, gram
    nbytes = L.load().agan_moments_update_ws_bytes(n, D)
    ws, wsp = _ws(nbytes, x)
    _kmeans_call("agan_moments_update", _p(x), n, D, _p(sum), _p(gram), wsp, nbytes, _stream())
    return sum, gram


def moments_finish(sum: Tensor, gram: Tensor, count: int) -> Tuple[Tensor, Tensor]:
    """-> (mean [D], cov [D, D]) float64: mean = sum / count, cov = (gram - count mean mean^T) / (count - 1) from the upper triangle of
    gram, mirrored to a matrix that is symmetric bit for bit; count == 1 gives a zero covariance."""
    if sum.dim() != 1:
        raise ValueError(f"moments_finish: expected sum [D], got {tuple(sum.shape)}")
    D, count = sum.shape[0], int(count)
    _moments_state(sum, gram, D, sum.device, "moments_finish")
    if not sum.is_cuda:
        if not 1 <= D <= 4096 or not 1 <= count < 1 << 53:
            raise ValueError(f"moments_finish: D {D}, count {count} outside 1 <= D <= 4096, 1 <= count < 2^53")
        mean = sum / count
        if count == 1:
            return mean, torch.zeros(D, D, dtype=torch.float64)
        upper = torch.triu(gram)
        full = upper + torch.triu(gram, 1).t()
        return mean, (full - count * torch.outer(mean, mean)) / (count - 1)
    mean = torch.empty(D, dtype=torch.float64, device=sum.device)
    cov = torch.empty(D, D, dtype=torch.float64, device=sum.device)
    _kmeans_call("agan_moments_finish", _p(sum), _p(gram), count, D, _p(mean), _p(cov), _stream())
    return mean, cov


_RETRIEVAL_CPU_ROWS = 1 << 10       # queries per float64 block of the CPU path


def retrieval_rank(query: Tensor, bank: Tensor, cand: Tensor, want_scores: bool = False):
    """-> rank int32 [N] (with want_scores: (rank, scores float32 [N, R])), on query's device.

    scores[i][j] = q_i . b_c / max(|q_i| |b_c|, 1e-8) with c = cand[i][j]; column 0 of cand is the match and
    rank[i] = #{ j >= 1 : scores[i][j] >= scores[i][0] }, so a tie counts against the match and rank 0 is a hit.  A candidate outside
    [0, M) raises ValueError: on the device it is refused by the kernel before it is used as an address and reported as a negative
    rank, which this wrapper reads back -- the one synchronisation of the call."""
    if query.dim() != 2 or bank.dim() != 2 or query.shape[1] != bank.shape[1]:
        raise ValueError(f"retrieval_rank: expected query [N, D] and bank [M, D], got {tuple(query.shape)} and {tuple(bank.shape)}")
    if bank.device != query.device or cand.device != query.device:
        raise ValueError(f"retrieval_rank: query is on {query.device}, bank on {bank.device}, cand on {cand.device}")
    for t, n in ((query, "query"), (bank, "bank")):
        if t.dtype != torch.float32:
            raise ValueError(f"retrieval_rank: {n} must be float32, got {t.dtype}")
    N, D = query.shape
    M = bank.shape[0]
    if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[0] != N:
        raise ValueError(f"retrieval_rank: cand must be int32 [{N}, R], got {cand.dtype} {tuple(cand.shape)}")
    R = cand.shape[1]
    query, bank, cand = query.contiguous(), bank.contiguous(), cand.contiguous()
    if not query.is_cuda:
        if N < 1 or M < 1 or not 1 <= D <= 4096 or not 1 <= R <= 1024:
            raise ValueError(f"retrieval_rank: N {N}, M {M}, D {D}, R {R} outside N, M >= 1, 1 <= D <= 4096, 1 <= R <= 1024")
        idx = cand.long()
        if bool(((idx < 0) | (idx >= M)).any()):
            raise ValueError(f"retrieval_rank: a candidate index lies outside [0, {M})")
        b64 = bank.double()
        bn = (b64 * b64).sum(1).sqrt()
        rank = torch.empty(N, dtype=torch.int32)
        scores = torch.empty(N, R, dtype=torch.float32) if want_scores else None
        for s in range(0, N, _RETRIEVAL_CPU_ROWS):
            q = query[s:s + _RETRIEVAL_CPU_ROWS].double()
            c = idx[s:s + _RETRIEVAL_CPU_ROWS]
            dot = (q.unsqueeze(1) * b64[c]).sum(-1)
            sc = dot / ((q * q).sum(1).sqrt().view(-1, 1) * bn[c]).clamp_(min=1e-8)
            rank[s:s + _RETRIEVAL_CPU_ROWS] = (sc[:, 1:] >= sc[:, :1]).sum(1).to(torch.int32)
            if want_scores:
                scores[s:s + _RETRIEVAL_CPU_ROWS] = sc.to(torch.float32)
        return (rank, scores) if want_scores else rank
    rank = torch.empty(N, dtype=torch.int32, device=query.device)
    scores = torch.empty(N, R, dtype=torch.float32, device=query.device) if want_scores else None
    _kmeans_call("agan_retrieval_rank", _p(query), _p(bank), _p(cand), N, M, D, R, _p(scores), _p(rank), _stream())
    if bool((rank < 0).any()):
        raise ValueError(f"retrieval_rank: a candidate index lies outside [0, {M})")
    return (rank, scores) if want_scores else rank


# --------------------------------------------------------------------------------------------------------------
# pairwise-geometry reductions (evaluation.py: manifold_metrics, kernel_distance; include/agan.h: agan_knn_radius, agan_manifold_scan,
# agan_poly_kernel_sum)
# --------------------------------------------------------------------------------------------------------------
# Device tensors run on the library.  A CPU tensor takes the float64 restatement below with the same rules: the row itself is left
# out by index, `<=` against the radius, the lowest index on a tie, the diagonal left out by index.  There a squared distance is the
# float64 sum of squared differences rounded once to float32 -- the value an exact fp32 computation would give -- so a distance
# compared with a radius that IS that distance ties on the CPU as it does on the device.  None has autograd: these are measurements.
_MANIFOLD_CPU_ELEMS = 1 << 24       # float64 elements per block of the CPU paths


def _rows_operand(t: Tensor, name: str, what: str) -> Tensor:
    if t.dim() != 2:
        raise ValueError(f"{what}: expected {name} [n, D], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
    return t.contiguous()


def _rows_in_domain(n: int, D: int) -> bool:
    return n >= 1 and 1 <= D <= 4096 and n * D < 1 << 31


def _pair_d2_blocks(q: Tensor, ref: Tensor):
    """yields (first query row, d2 float64 [rows, n]) over blocks of query rows; d2 holds float32 values"""
    r64 = ref.double()
    rows = max(1, _MANIFOLD_CPU_ELEMS // max(1, ref.shape[0] * ref.shape[1]))
    for s in range(0, q.shape[0], rows):
        diff = q[s:s + rows].double().unsqueeze(1) - r64.unsqueeze(0)
        yield s, (diff * diff).sum(-1).to(torch.float32).double()


def knn_radius(x: Tensor, k: int) -> Tensor:
    """-> rad2 float32 [n] on x's device: the k-th smallest squared distance from row i to the OTHER rows of x [n, D].  The row itself
    is left out by index, so a duplicate row at distance 0 counts as a neighbour.  1 <= k <= 8, n >= k + 1."""
    x = _rows_operand(x, "x", "knn_radius")
    n, D = x.shape
    k = int(k)
    if not 1 <= k <= 8 or n < k + 1 or not _rows_in_domain(n, D):
        raise ValueError(f"knn_radius: n {n}, D {D}, k {k} outside 1 <= k <= 8, n >= k + 1, 1 <= D <= 4096, n * D < 2^31")
    if not x.is_cuda:
        rad2 = torch.empty(n, dtype=torch.float32)
        for s, d2 in _pair_d2_blocks(x, x):
            rows = torch.arange(d2.shape[0])
            d2[rows, s + rows] = float("inf")
            rad2[s:s + d2.shape[0]] = d2.kthvalue(k, dim=1)[0].to(torch.float32)
        return rad2
    rad2 = torch.empty(n, dtype=torch.float32, device=x.device)
    nbytes = L.load().agan_knn_radius_ws_bytes(n, D, k)
    ws, wsp = _ws(nbytes, x)
    _kmeans_call("agan_knn_radius", _p(x), n, D, k, _p(rad2), wsp, nbytes, _stream())
    return rad2


def manifold_scan(q: Tensor, ref: Tensor, rad2: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (count int32 [m], near_d2 float32 [m], near_idx int32 [m]) on q's device, for q [m, D] against ref [n, D]:
    count[i] = #{ j : d2(q_i, ref_j) <= rad2[j] } (all zeros without rad2), near_d2[i] = min_j d2(q_i, ref_j) and near_idx[i] the lowest
    j that attains it."""
    q, ref = _rows_operand(q, "q", "manifold_scan"), _rows_operand(ref, "ref", "manifold_scan")
    m, D = q.shape
    n = ref.shape[0]
    if ref.shape[1] != D or ref.device != q.device:
        raise ValueError(f"manifold_scan: q is {tuple(q.shape)} on {q.device}, ref {tuple(ref.shape)} on {ref.device}")
    if rad2 is not None:
        if rad2.dtype != torch.float32 or tuple(rad2.shape) != (n,) or rad2.device != q.device:
            raise ValueError(f"manifold_scan: rad2 must be float32 [{n}] on {q.device}, got {rad2.dtype} {tuple(rad2.shape)} on {rad2.device}")
        rad2 = rad2.contiguous()
    if not _rows_in_domain(m, D) or not _rows_in_domain(n, D):
        raise ValueError(f"manifold_scan: m {m}, n {n}, D {D} outside m, n >= 1, 1 <= D <= 4096, m * D and n * D < 2^31")
    if not q.is_cuda:
        count = torch.zeros(m, dtype=torch.int32)
        near_d2 = torch.empty(m, dtype=torch.float32)
        near_idx = torch.empty(m, dtype=torch.int32)
        for s, d2 in _pair_d2_blocks(q, ref):
            e = s + d2.shape[0]
            if rad2 is not None:
                count[s:e] = (d2 <= rad2.double().view(1, n)).sum(1).to(torch.int32)
            best = torch.from_numpy(d2.numpy().argmin(axis=1))              # numpy: the first minimum
            near_idx[s:e] = best.to(torch.int32)
            near_d2[s:e] = d2.gather(1, best.view(-1, 1)).view(-1).to(torch.float32)
        return count, near_d2, near_idx
    count = torch.empty(m, dtype=torch.int32, device=q.device)
    near_d2 = torch.empty(m, dtype=torch.float32, device=q.device)
    near_idx = torch.empty(m, dtype=torch.int32, device=q.device)
    nbytes = L.load().agan_manifold_scan_ws_bytes(m, n, D)
    ws, wsp = _ws(nbytes, q)
    _kmeans_call("agan_manifold_scan", _p(q), _p(ref), _p(rad2), m, n, D, _p(count), _p(near_d2), _p(near_idx), wsp, nbytes, _stream())
    return count, near_d2, near_idx


def poly_kernel_sum(x: Tensor, y: Tensor, exclude_diagonal: bool = False) -> Tensor:
    """-> float64 [1] on x's device: sum_ij ((x_i . y_j) / D + 1)^3 over x [n, D] and y [m, D], without the terms i == j when
    exclude_diagonal is set (then n == m; the caller passes y = x)."""
    x, y = _rows_operand(x, "x", "poly_kernel_sum"), _rows_operand(y, "y", "poly_kernel_sum")
    n, D = x.shape
    m = y.shape[0]
    if y.shape[1] != D or y.device != x.device:
        raise ValueError(f"poly_kernel_sum: x is {tuple(x.shape)} on {x.device}, y {tuple(y.shape)} on {y.device}")
    if not _rows_in_domain(n, D) or not _rows_in_domain(m, D) or (exclude_diagonal and n != m):
        raise ValueError(f"poly_kernel_sum: n {n}, m {m}, D {D} outside n, m >= 1, 1 <= D <= 4096, n * D and m * D < 2^31 "
                         f"(n == m with exclude_diagonal)")
    if not x.is_cuda:
        y64 = y.double()
        total = torch.zeros((), dtype=torch.float64)
        rows = max(1, _MANIFOLD_CPU_ELEMS // m)
        for s in range(0, n, rows):
            kv = ((x[s:s + rows].double() @ y64.t()) / D + 1.0) ** 3
            if exclude_diagonal:
                r = torch.arange(kv.shape[0])
                kv[r, s + r] = 0.0
            total += kv.sum()
        return total.view(1)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    nbytes = L.load().agan_poly_kernel_sum_ws_bytes(n, m, D)
    ws, wsp = _ws(nbytes, x)
    _kmeans_call("agan_poly_kernel_sum", _p(x), _p(y), n, m, D, 1 if exclude_diagonal else 0, _p(out), wsp, nbytes, _stream())
    return out


# --------------------------------------------------------------------------------------------------------------
# the Inception Score's reduction (evaluation.py: inception_score; include/agan.h: agan_inception_score)
# --------------------------------------------------------------------------------------------------------------
def inception_split_scores(logits: Tensor, splits: int = 10) -> Tensor:
    """-> float64 [splits, 3] on the device of logits [N, C] float32: per split s of the rows [s N // splits, (s + 1) N // splits) the
    Inception Score exp(Hm - Hc), the label entropy Hm of the split's mean class distribution and the mean conditional entropy Hc of
    its rows (include/agan.h states the arithmetic).  1 <= C <= 4096, N * C < 2^31, 1 <= splits <= min(N, 1024).  A row that holds
    +inf or a NaN, or nothing but -inf, makes its own split's three numbers NaN.  Device tensors run on the library; a CPU tensor takes
    the float64 restatement below.  No autograd: a measurement."""
    if logits.dim() != 2:
        raise ValueError(f"inception_split_scores: expected logits [N, C], got {tuple(logits.shape)}")
    if logits.dtype != torch.float32:
        raise ValueError(f"inception_split_scores: logits must be float32, got {logits.dtype}")
    logits = logits.detach().contiguous()
    N, C = logits.shape
    splits = int(splits)
    if not _rows_in_domain(N, C) or not 1 <= splits <= min(N, 1024):
        raise ValueError(f"inception_split_scores: N {N}, C {C}, splits {splits} outside N >= 1, 1 <= C <= 4096, N * C < 2^31, "
                         f"1 <= splits <= min(N, 1024)")
    if not logits.is_cuda:
        out = torch.empty(splits, 3, dtype=torch.float64)
        zero = torch.zeros((), dtype=torch.float64)
        for s in range(splits):
            x = logits[s * N // splits:(s + 1) * N // splits].double()
            m = x.max(1, keepdim=True)[0]
            logp = x - (m + (x - m).exp().sum(1, keepdim=True).log())
            p = logp.exp()
            hc = -torch.where(p == 0, zero, p * logp).sum(1).mean()
            q = p.mean(0)
            hm = -torch.where(q == 0, zero, q * q.log()).sum()
            out[s, 0], out[s, 1], out[s, 2] = (hm - hc).exp(), hm, hc
        return out
    out = torch.empty(splits, 3, dtype=torch.float64, device=logits.device)
    nbytes = L.load().agan_inception_score_ws_bytes(N, C, splits)
    ws, wsp = _ws(nbytes, logits)
    _kmeans_call("agan_inception_score", _p(logits), N, C, splits, _p(out), wsp, nbytes, _stream())
    return out
