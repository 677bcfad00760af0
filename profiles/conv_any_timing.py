#!/usr/bin/env python3
"""Times the general trainable conv (HF.conv2d(kind="any"), csrc/conv_any.hip) with device events, alternated runs, median:

  (a) per direction against stock torch on the same device (F.conv2d / conv2d_input / conv2d_weight: MIOpen);
  (b) forward and backward (data + weight gradient) against the tuned kinds at the two shared geometries (3,1,1) and (4,2,1),
      with the general engine forced through kind="any".

    python profiles/conv_any_timing.py > profiles/r08_conv_any_timing.txt
"""
import importlib
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HF = importlib.import_module("attention-gan_amd.backend.functional")

# B, Cin, H, Cout, k, s, p
SHAPES = [(24, 64, 64, 128, 4, 3, 3), (24, 64, 128, 128, 4, 2, 1), (24, 128, 32, 128, 3, 1, 1)]
ROUNDS, WARM = 15, 3


def alternated(fns):
    """median ms of every callable, the callables run in turn ROUNDS times (each between its own pair of events)"""
    ms = [[] for _ in fns]
    for r in range(WARM + ROUNDS):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= WARM:
                ms[i].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


def main():
    dev = "cuda"
    torch.manual_seed(0)
    print(f"{'shape':38s} {'direction':9s} {'any ms':>8s} {'MIOpen ms':>10s} {'ratio':>6s} {'tuned ms':>9s} {'ratio':>6s}")
    for B, cin, H, cout, k, s, p in SHAPES:
        x = torch.randn(B, cin, H, H, device=dev)
        w = torch.randn(cout, cin, k, k, device=dev)
        y = F.conv2d(x, w, None, s, p)
        dy = torch.randn_like(y)
        kind = {(3, 1, 1): "same", (4, 2, 1): "down"}.get((k, s, p))
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        cache = {}

        def lib_fwd(knd, xi, wi):
            return HF.conv2d(xi, wi, None, knd, cache if knd != "any" else None, None, None, 0, None, None, (s, s), (p, p))

        # an output whose graph needs ONE gradient only: the autograd function runs just that direction
        out_d = {knd: lib_fwd(knd, xg, w) for knd in filter(None, ("any", kind))}
        out_w = {knd: lib_fwd(knd, x, wg) for knd in filter(None, ("any", kind))}
        out_b = {knd: lib_fwd(knd, xg, wg) for knd in filter(None, ("any", kind))}
        fns = [lambda: lib_fwd("any", x, w),
               lambda: F.conv2d(x, w, None, s, p),
               lambda: torch.autograd.grad(out_b["any"], (xg, wg), dy, retain_graph=True),
               lambda: (torch.nn.grad.conv2d_input(x.shape, w, dy, s, p), torch.nn.grad.conv2d_weight(x, w.shape, dy, s, p)),
               lambda: torch.autograd.grad(out_d["any"], (xg,), dy, retain_graph=True),
               lambda: torch.nn.grad.conv2d_input(x.shape, w, dy, s, p),
               lambda: torch.autograd.grad(out_w["any"], (wg,), dy, retain_graph=True),
               lambda: torch.nn.grad.conv2d_weight(x, w.shape, dy, s, p)]
        if kind:
            fns += [lambda: lib_fwd(kind, x, w), lambda: torch.autograd.grad(out_b[kind], (xg, wg), dy, retain_graph=True),
                    lambda: torch.autograd.grad(out_d[kind], (xg,), dy, retain_graph=True),
                    lambda: torch.autograd.grad(out_w[kind], (wg,), dy, retain_graph=True)]
        t = alternated(fns)
        name = f"B{B} {cin}->{cout} {H}x{H} k{k} s{s} p{p}"
        tuned = dict(zip(("fwd", "bwd", "dgrad", "wgrad"), t[8:])) if kind else {}
        for label, a, m in (("fwd", t[0], t[1]), ("dgrad", t[4], t[5]), ("wgrad", t[6], t[7]), ("bwd", t[2], t[3])):
            tu = tuned.get(label)
            print(f"{name:38s} {label:9s} {a:8.3f} {m:10.3f} {a / m:6.2f} " + (f"{tu:9.3f} {a / tu:6.2f}" if tu else f"{'-':>9s} {'-':>6s}"))
    print("any: HF.conv2d(kind='any') (fp32 MFMA implicit GEMM; dgrad / wgrad alone: a graph that needs that one gradient; host launch time included); MIOpen: stock torch ops on the "
          "same device; tuned: kinds 'same' / 'down' (Winograd / patch / row planners, fp32 mode).  Medians of 15 alternated runs.")


if __name__ == "__main__":
    main()
