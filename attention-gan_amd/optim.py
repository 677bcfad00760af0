"""Flat-buffer Adam: torch.optim.Adam(lr, betas=(0.5, 0.999)) semantics (train.py:78-80) as ONE fused HIP launch.

All trainable parameters of a module are re-homed as views into a single contiguous fp32 buffer (and their .grad
into a second one).  One optimiser step is then one kernel over the flat buffer, and the data-parallel gradient
exchange (dataparallel.py) all-reduces large contiguous slices instead of hundreds of small tensors -- sized for
288 GB HBM3E and point-to-point xGMI links, not for per-tensor NCCL calls.
"""
from __future__ import annotations

from typing import Dict, Iterable, List

import torch
from torch import Tensor, nn

from .backend import functional as HF


class _FlatHome:
    """Parameters re-homed as views of one flat fp32 buffer that packed-weight caches follow on its own (HF.register_flat)."""

    def _rehome(self, params: List[nn.Parameter], device) -> None:
        """-> self.params, self.offsets, self.numel, self.flat: the buffer holds the parameters' values and every p.data views it"""
        self.params = params
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += (p.numel() + 3) // 4 * 4           # keep every parameter 16-byte aligned inside the buffer
        self.numel = total
        self.flat = torch.zeros(total, dtype=torch.float32, device=device)
        with torch.no_grad():
            for p, o in zip(self.params, self.offsets):
                self.flat[o:o + p.numel()].copy_(p.detach().reshape(-1))
                p.data = self.flat[o:o + p.numel()].view(p.shape)
        if self.flat.is_cuda:
            HF.register_flat(self.flat)        # packed-weight caches follow THIS buffer's writes only

    def __del__(self):
        try:
            HF.unregister_flat(self.flat)
        except Exception:      # interpreter shutdown, or a constructor that raised before the buffer existed
            pass


class FlatAdam(_FlatHome):
    def __init__(self, params: Iterable[nn.Parameter], lr: float = 2e-4, betas=(0.5, 0.999), eps: float = 1e-8):
        params = [p for p in params if p.requires_grad]
        if not params:
            raise ValueError("FlatAdam: no trainable parameters")
        dev, dt = params[0].device, params[0].dtype
        if dt != torch.float32:
            raise ValueError("FlatAdam: float32 parameters only")
        self.lr, self.betas, self.eps = lr, tuple(betas), eps
        self._rehome(params, dev)
        self.grad = torch.zeros(self.numel, dtype=dt, device=dev)
        self.exp_avg = torch.zeros(self.numel, dtype=dt, device=dev)
        self.exp_avg_sq = torch.zeros(self.numel, dtype=dt, device=dev)
        for p, o in zip(self.params, self.offsets):
            p.grad = self.grad[o:o + p.numel()].view(p.shape)
            p._agan_grad_dst = HF.GradDst(self.grad, o, p.numel())   # backward kernels write here directly
        self.step_count = 0
        # device-resident step counter + bias-correction coefficients (see agan_adam_step): advanced by the kernel itself, so a
        # captured HIP graph keeps counting on replay; step_count mirrors it on the host for state_dict()
        self.step_state = torch.zeros(4, dtype=torch.int32, device=dev)

    # -- torch.optim-like surface ---------------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = False) -> None:
        """Start a new backward: drop the per-parameter .grad references and re-arm the first-writer flags.  The flat gradient
        buffer itself is NOT filled with zeros here (376 MB per step at the metric config): the first backward kernel that
        produces a parameter's gradient overwrites its slice, and step() zeroes the slice of any parameter that received no
        gradient at all in this backward (torch.optim.Adam skips such a parameter; a zero gradient keeps the fused update
        branch-free and only decays its moments)."""
        for p in self.params:
            p.grad = None
            p._agan_grad_dst.reset()

    def _rebind(self, indices=None) -> int:
        """Make p.grad the view into the flat buffer (for all parameters, or the given indices); gradients that landed
        elsewhere (a kernel without a flat destination, or autograd cloning instead of adopting) are copied in.
        Returns how many copies were needed."""
        copies = 0
        base = self.grad.data_ptr()
        self.rebind_calls = getattr(self, "rebind_calls", 0) + 1
        it = zip(self.params, self.offsets) if indices is None else ((self.params[i], self.offsets[i]) for i in indices)
        for p, o in it:
            g = p.grad
            if g is not None and g.data_ptr() == base + 4 * o:
                continue
            view = self.grad[o:o + p.numel()].view(p.shape)
            if g is not None:
                dst = p._agan_grad_dst
                if not dst.written:
                    view.copy_(g)             # no kernel wrote the slice: a stock autograd gradient
                    copies += 1
                elif HF.wgrad_side_stream_enabled():
                    # the kernel wrote the slice on a side stream autograd knows nothing about: its copy may have been taken too early
                    raise RuntimeError("FlatAdam: autograd copied a gradient that was written on the weight-gradient side stream")
                elif dst.edges <= 1:
                    # ONE kernel contribution, and autograd holds a tensor of its own: either a clone of that contribution (it clones
                    # instead of adopting the view when something else still references it) or its sum with stock autograd edges
                    # of the same parameter (a tied weight, an op without a flat destination).  In both cases autograd's tensor is
                    # the complete gradient.
                    view.copy_(g)
                    copies += 1
                else:
                    # Several kernel contributions accumulated in the slice.  A clone autograd took once every edge had arrived
                    # equals the slice and is dropped; anything else is a stock autograd edge summed with only PART of the kernel
                    # contributions, which cannot be reconstructed -- refuse rather than train on a wrong gradient.
                    if torch.cuda.is_available() and p.is_cuda and torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("FlatAdam: autograd replaced a gradient with several in-kernel contributions during graph capture")
                    if g.shape != view.shape or not torch.equal(g, view):
                        raise RuntimeError("FlatAdam: a parameter received several in-kernel gradient contributions AND a stock autograd "
                                           "gradient in one backward (tied weight?): unsupported, the sum cannot be recovered")
            elif not p._agan_grad_dst.written:
                view.zero_()                  # no gradient reached this parameter in this backward
            p.grad = view
        self.rebind_copies = getattr(self, "rebind_copies", 0) + copies
        return copies

    def join_and_rebind(self) -> None:
        """Make the flat gradient buffer complete and current on this stream (what step() does first)."""
        HF.join_side_stream()          # weight gradients forked off the current stream (functional.set_wgrad_side_stream)
        self._rebind()

    def named_gradients(self, module) -> Dict[str, Tensor]:
        """{parameter name: view of its slice of the flat gradient buffer} for the trainable parameters of `module`"""
        names = [k for k, p in module.named_parameters() if p.requires_grad]
        return {k: self.grad[o:o + p.numel()].view(p.shape) for k, p, o in zip(names, self.params, self.offsets)}

    def step(self, grad_scale: float = 1.0) -> None:
        self.join_and_rebind()
        self.step_count += 1
        if self.flat.is_cuda:
            HF.adam_step_(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.step_state, self.lr,
                          self.betas[0], self.betas[1], self.eps, grad_scale)
        else:
            raise RuntimeError("FlatAdam.step: parameters are not on an MI355X (no CPU fallback)")

    # -- checkpoint interchange with torch.optim.Adam.state_dict() (reference _save_weights, trainer.py:109-115) --
    def sync_step_count(self) -> int:
        """The device counter is the truth (a replayed HIP graph advances only it): mirror it on the host.  One host sync."""
        if self.step_state.is_cuda:
            self.step_count = int(self.step_state[0].item())
        return self.step_count

    def state_dict(self) -> Dict:
        self.sync_step_count()
        state = {}
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            n = p.numel()
            state[i] = {"step": torch.tensor(float(self.step_count)),
                        "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                        "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone()}
        group = {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: Dict) -> None:
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps = g["lr"], tuple(g["betas"]), g["eps"]
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                st = sd["state"].get(i)
                if st is None:
                    continue
                n = p.numel()
                self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                self.step_count = int(float(st["step"]))
        with torch.no_grad():
            self.step_state.zero_()
            self.step_state[0] = self.step_count


class FlatEMA(_FlatHome):
    """Exponential moving average of a module's weights in a shadow module, as ONE fused HIP launch per update.

    The shadow's trainable parameters are re-homed into a flat buffer of its own with `live_opt`'s order, offsets and padding, so
    the parameter part of an update is one flat-to-flat segment; every floating-point buffer of the live module (BatchNorm running
    statistics) is one more segment into the shadow's buffer of the same name.  Integer buffers (num_batches_tracked) are not
    averaged: shadow_state_dict() copies them from the live module.  Parameters the live optimiser does not own (frozen ones) stay
    as the shadow holds them.  update() does  shadow += (1 - beta_t) * (live - shadow)  with beta_t = min(decay, (1 + t) / (10 + t))
    (warmup) or decay, t counted in device memory (include/agan.h: agan_ema_update).

    The shadow is an inference copy: no gradients, always in eval mode (its train() is pinned to False -- batch statistics would
    depend on the batch), and its packed weights follow the shadow buffer's own epoch (HF.register_flat)."""

    def __init__(self, live_module: nn.Module, shadow_module: nn.Module, live_opt: FlatAdam, decay: float, warmup: bool = True):
        if not 0.0 < float(decay) < 1.0:
            raise ValueError(f"FlatEMA: decay must lie inside (0, 1), got {decay}")
        self.live, self.shadow, self.live_opt = live_module, shadow_module, live_opt
        self.decay, self.warmup = float(decay), bool(warmup)
        live_named = [(k, p) for k, p in live_module.named_parameters() if p.requires_grad]
        if len(live_named) != len(live_opt.params) or any(p is not q for (_, p), q in zip(live_named, live_opt.params)):
            raise ValueError("FlatEMA: live_opt does not hold the trainable parameters of live_module in named_parameters() order")
        if any(p.dtype != torch.float32 for p in shadow_module.parameters()):
            raise ValueError("FlatEMA: float32 parameters only")
        live_all = {k: tuple(p.shape) for k, p in live_module.named_parameters()}
        shadow_all = {k: tuple(p.shape) for k, p in shadow_module.named_parameters()}
        if live_all != shadow_all:
            odd = sorted(k for k in set(live_all) | set(shadow_all) if live_all.get(k) != shadow_all.get(k))
            raise ValueError(f"FlatEMA: the shadow's parameters differ from the live module's in name or shape: {odd[:4]}")
        shadow_params = dict(shadow_module.named_parameters())
        self._rehome([shadow_params[k] for k, _ in live_named], live_opt.flat.device)
        assert self.offsets == live_opt.offsets and self.numel == live_opt.numel, "FlatEMA: the shadow's layout must be the live optimiser's"
        for p in self.params:
            p.grad = None
        for p in shadow_module.parameters():
            p.requires_grad_(False)
        for m in shadow_module.modules():                  # packed copies the original had made of ITS weights
            if isinstance(m.__dict__.get("_packed"), dict):
                m._packed = {}
        cls = type(shadow_module)
        shadow_module.__class__ = type(cls.__name__, (cls,), {"train": lambda self, mode=True: nn.Module.train(self, False),
                                                              "__module__": cls.__module__})
        shadow_module.train(False)
        self.updates = 0
        self.state = torch.zeros(4, dtype=torch.int32, device=self.flat.device)    # [0] update count, [2] fp32 1 - beta_t (device-made)
        self._table = None
        if self.flat.is_cuda:
            self._segments()

    def _buffer_pairs(self):
        """[(live module's buffer dict, shadow module's buffer dict, name)] of every floating-point buffer, checked"""
        shadow_mods = dict(self.shadow.named_modules())
        pairs = []
        for prefix, m in self.live.named_modules():
            for k, b in m._buffers.items():
                if b is None or not b.is_floating_point():
                    continue
                sm = shadow_mods.get(prefix)
                s = sm._buffers.get(k) if sm is not None else None
                name = f"{prefix}.{k}" if prefix else k
                if s is None or s.shape != b.shape:
                    raise ValueError(f"FlatEMA: the shadow has no buffer {name!r} of shape {tuple(b.shape)}")
                if b.dtype != torch.float32 or s.dtype != torch.float32 or not (b.is_contiguous() and s.is_contiguous()) or s.device != b.device:
                    raise ValueError(f"FlatEMA: buffer {name!r} must be contiguous float32 on one device in both modules")
                pairs.append((m._buffers, sm._buffers, k))
        return pairs

    def _segments(self):
        """(device table, nseg, total_blocks).  Built once; before every launch the recorded addresses are compared with the modules'
        buffers of the moment (a .to() or a dtype change reallocates them) and the table is rebuilt when one moved."""
        hit = self._table
        if hit is not None:
            key, pairs = hit[0], hit[1]
            if key[0][0] == self.live_opt.flat.data_ptr() and all(
                    lb[k].data_ptr() == ptrs[0] and sb[k].data_ptr() == ptrs[1] for (lb, sb, k), ptrs in zip(pairs, key[1:])):
                return hit[2:]
        if self.flat.is_cuda and torch.cuda.is_current_stream_capturing():
            raise HF.L.AganError("averaging segment table missing or stale during HIP-graph capture: run a warm-up step first "
                                 "(GanTrainStep.capture does)")
        pairs = self._buffer_pairs()
        key = [(self.live_opt.flat.data_ptr(), self.flat.data_ptr(), self.numel)] + \
              [(lb[k].data_ptr(), sb[k].data_ptr(), lb[k].numel()) for lb, sb, k in pairs]
        self._table = (key, pairs) + HF.ema_table(key, self.flat.device)
        return self._table[2:]

    def update(self) -> None:
        if not self.flat.is_cuda:
            raise RuntimeError("FlatEMA.update: parameters are not on an MI355X (no CPU fallback)")
        table, nseg, total = self._segments()
        self.updates += 1
        HF.ema_update_(table, nseg, total, self.state, self.decay, self.warmup, self.flat)

    def sync_updates(self) -> int:
        """The device counter is the truth (a replayed HIP graph advances only it): mirror it on the host.  One host sync."""
        self.updates = int(self.state[0].item())
        return self.updates

    def copy_from_live(self) -> None:
        """shadow := live (parameters and buffers), update count 0"""
        with torch.no_grad():
            self.shadow.load_state_dict(self.live.state_dict())
            self.state.zero_()
        self.updates = 0

    def shadow_state_dict(self) -> Dict:
        with torch.no_grad():
            shadow = dict(self.shadow.named_buffers())
            for k, b in self.live.named_buffers():
                if not b.is_floating_point() and k in shadow:
                    shadow[k].copy_(b)
        return self.shadow.state_dict()

    def state_dict(self) -> Dict:
        return {"shadow": self.shadow_state_dict(), "decay": self.decay, "warmup": self.warmup, "updates": self.sync_updates()}

    def load_state_dict(self, sd: Dict) -> None:
        """decay and warmup are configuration: the constructor's values stay."""
        with torch.no_grad():
            self.shadow.load_state_dict(sd["shadow"])
            self.updates = int(sd.get("updates", 0))
            self.state.zero_()
            self.state[0] = self.updates
