#!/usr/bin/env python3
"""Times one k-means assignment and one centroid update (csrc/kmeans.hip through backend.functional) at N = 200 000 rows against the
plain torch formulation on the same device, with device events around 20 back-to-back calls, alternated windows, medians:

    assign   library: agan_kmeans_assign                         torch: (|c|^2 - 2 X @ C.T).argmin(1)
    update   library: agan_kmeans_update                         torch: zeros(K, D).index_add_(0, labels, X) / bincount

and reports, from the shapes, the assignment's share of the 157.3 TFLOP/s fp32 MFMA peak (2 N K D flops) and the update's bandwidth
(N D 4 bytes: X is read once).  Not run by bench.py.

    python profiles/kmeans_micro.py > profiles/kmeans_micro.txt

`--assign-only` runs nothing but five library assignments per shape: the program to put under `rocprofv3 --kernel-trace --pmc
SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE` for the assignment kernel's MFMA-busy share (busy cycles / (active cycles x 128), the rule of
profiles/README.md), in a run of its own.
"""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HF = importlib.import_module("attention-gan_amd.backend.functional")

N = 200_000
SHAPES = [(k, d) for d in (512, 2048) for k in (9, 300)]
ROUNDS, WARM, CALLS = 15, 3, 20
PEAK_FP32_MFMA = 157.3e12


def alternated(fns):
    """median ms per call of every callable, the callables run in turn ROUNDS times; a timed window is CALLS back-to-back calls between
    one pair of events (20 to 80 ms of device work at the large shapes, 2 ms at the smallest), so that the host's enqueue of a call
    overlaps the device's work on the one before and the figure is device time unless the host is the slower of the two"""
    ms = [[] for _ in fns]
    for r in range(WARM + ROUNDS):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn()
            e1.record()
            e1.synchronize()
            if r >= WARM:
                ms[i].append(e0.elapsed_time(e1) / CALLS)
    return [statistics.median(m) for m in ms]


def main():
    if not torch.cuda.is_available():
        sys.exit("kmeans_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    print(f"{'N':>7s} {'K':>4s} {'D':>5s} | {'assign ms':>9s} {'torch ms':>9s} {'ratio':>6s} {'TFLOP/s':>8s} {'of peak':>7s} | "
          f"{'update ms':>9s} {'torch ms':>9s} {'ratio':>6s} {'TB/s':>6s} | labels equal")
    for K, D in SHAPES:
        c = torch.randn(K, D, generator=g).to(dev)
        x = (c[torch.randint(0, K, (N,), generator=g).to(dev)] + torch.randn(N, D, generator=g).to(dev)).contiguous()
        labels = HF.kmeans_assign(x, c)[0]
        if "--assign-only" in sys.argv[1:]:
            for _ in range(5):
                HF.kmeans_assign(x, c, labels)
            torch.cuda.synchronize()
            continue
        lab64 = labels.long()

        def torch_assign():
            return ((c * c).sum(1).view(1, K) - 2.0 * (x @ c.t())).argmin(1)

        def torch_update():
            sums = torch.zeros(K, D, device=dev).index_add_(0, lab64, x)
            return sums / torch.bincount(lab64, minlength=K).clamp(min=1).view(K, 1)

        same = float((torch_assign() == lab64).float().mean())
        ta, tta, tu, ttu = alternated([lambda: HF.kmeans_assign(x, c, labels), torch_assign, lambda: HF.kmeans_update(x, labels, c), torch_update])
        flops = 2.0 * N * K * D
        print(f"{N:7d} {K:4d} {D:5d} | {ta:9.3f} {tta:9.3f} {ta / tta:6.2f} {flops / ta / 1e9:8.1f} {100 * flops / ta / 1e-3 / PEAK_FP32_MFMA:6.1f}% | "
              f"{tu:9.3f} {ttu:9.3f} {tu / ttu:6.2f} {N * D * 4 / tu / 1e9:6.2f} | {100 * same:.3f}%")
    if "--assign-only" in sys.argv[1:]:
        return
    print("assign / update: backend.functional.kmeans_assign / kmeans_update (workspace allocation and host launch time included); torch: the plain formulation "
          "on the same device (fp32 matmul, argmin, index_add_).  ratio = library / torch.  Per call, from windows of 20 back-to-back calls; medians of 15 alternated windows after 3 warm-up rounds.")


if __name__ == "__main__":
    main()
