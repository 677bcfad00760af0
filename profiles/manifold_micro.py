#!/usr/bin/env python3
"""Times the three pairwise-geometry reductions (csrc/manifold.hip through backend.functional) against the blocked torch formulation on
the same device, with device events around windows of back-to-back calls, alternated windows, medians:

    knn_radius       library: agan_knn_radius                    torch: torch.cdist on row blocks, the diagonal set to inf, kthvalue
    manifold_scan    library: agan_manifold_scan with radii      torch: torch.cdist on row blocks, squared, compared with the radii, sum, min
    poly_kernel_sum  library: agan_poly_kernel_sum               torch: ((x.double() @ y.double().T) / D + 1) ** 3 on row blocks, summed

and reports, from the shapes, the rate of the 2 n m D flops each owes and its share of the 157.3 TFLOP/s fp32 matrix peak; then the
time of one whole evaluation.manifold_metrics and one evaluation.kernel_distance (100 subsets of 1000) on the largest shape.  Not
run by bench.py.

    python profiles/manifold_micro.py > profiles/manifold_micro.txt
"""
import importlib
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HF = importlib.import_module("attention-gan_amd.backend.functional")
EV = importlib.import_module("attention-gan_amd.evaluation")

SHAPES = [(1000, 2048), (5000, 2048), (30_000, 2048)]          # n = m rows, D
K = 3
ROUNDS, WARM = 5, 1
PEAK_FP32_MATRIX = 157.3e12
TORCH_ROW_BLOCK = 2500                                          # rows per block of the torch side: a 2500 x 30000 fp64 block is 600 MB


def alternated(fns, calls):
    """median ms per call of every callable, the callables run in turn ROUNDS times; a timed window is `calls` back-to-back calls between
    one pair of events, so that the host's enqueue of a call overlaps the device's work on the one before"""
    ms = [[] for _ in fns]
    for r in range(WARM + ROUNDS):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            if r >= WARM:
                ms[i].append(e0.elapsed_time(e1) / calls)
    return [statistics.median(m) for m in ms]


def main():
    if not torch.cuda.is_available():
        sys.exit("manifold_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    print(f"library: {os.path.relpath(HF.L.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))}")
    print(f"{'entry':>15s} {'n = m':>6s} {'D':>5s} | {'library ms':>10s} {'torch ms':>9s} {'ratio':>6s} | {'TFLOP/s owed':>12s} {'of peak':>7s} | agreement with torch")
    for n, D in SHAPES:
        x, y = torch.randn(n, D, generator=g).to(dev), (0.2 + torch.randn(n, D, generator=g)).to(dev)
        rad = HF.knn_radius(y, K)

        def torch_knn():
            out = []
            for lo in range(0, n, TORCH_ROW_BLOCK):
                d = torch.cdist(y[lo:lo + TORCH_ROW_BLOCK], y)
                rows = torch.arange(d.shape[0], device=dev)
                d[rows, lo + rows] = float("inf")
                out.append(d.kthvalue(K, dim=1)[0] ** 2)
            return torch.cat(out)

        def torch_scan():
            count, near = [], []
            for lo in range(0, n, TORCH_ROW_BLOCK):
                d2 = torch.cdist(x[lo:lo + TORCH_ROW_BLOCK], y) ** 2
                count.append((d2 <= rad.view(1, -1)).sum(1))
                near.append(d2.min(1)[0])
            return torch.cat(count), torch.cat(near)

        def torch_poly():
            y64, total = y.double(), torch.zeros((), dtype=torch.float64, device=dev)
            for lo in range(0, n, TORCH_ROW_BLOCK):
                total += (((x[lo:lo + TORCH_ROW_BLOCK].double() @ y64.t()) / D + 1.0) ** 3).sum()
            return total

        agree = [f"max rel. radius difference {float(((rad - torch_knn()).abs() / rad).max()):.2e}"]
        count, near, _ = HF.manifold_scan(x, y, rad)
        t_count, t_near = torch_scan()
        agree.append(f"counts equal {100 * float((count == t_count).float().mean()):.2f}%, max rel. nearest difference "
                     f"{float(((near - t_near).abs() / t_near).max()):.2e}")
        agree.append(f"rel. difference {abs(float(HF.poly_kernel_sum(x, y)) - float(torch_poly())) / abs(float(torch_poly())):.2e}")
        calls = 20 if n <= 1000 else 5 if n <= 5000 else 1
        pairs = [("knn_radius", lambda: HF.knn_radius(y, K), torch_knn), ("manifold_scan", lambda: HF.manifold_scan(x, y, rad), torch_scan),
                 ("poly_kernel_sum", lambda: HF.poly_kernel_sum(x, y), torch_poly)]
        owed = 2.0 * n * n * D
        for (name, lib_fn, torch_fn), note in zip(pairs, agree):
            t, tt = alternated([lib_fn, torch_fn], calls)
            print(f"{name:>15s} {n:6d} {D:5d} | {t:10.3f} {tt:9.3f} {t / tt:6.2f} | {owed / t / 1e9:12.1f} {100 * owed / t / 1e-3 / PEAK_FP32_MATRIX:6.1f}% | {note}")
    print(f"library: the backend.functional wrappers (norm pass, contraction, final pass; workspace and output allocation and host launch time "
          f"included), k = {K}.  torch: blocks of {TORCH_ROW_BLOCK} rows; cdist and the comparisons in fp32, the kernel sum in fp64 with its conversions.  "
          f"ratio = library / torch.  owed = 2 n m D flops.  Per call, from windows of 20 (n = 1000), 5 (n = 5000) or 1 call; medians of {ROUNDS} "
          f"alternated windows after {WARM} warm-up round.")

    n, D = SHAPES[-1]
    real, fake = (3.0 + 0.5 * torch.randn(n, D, generator=g)).to(dev), (3.1 + 0.6 * torch.randn(n, D, generator=g)).to(dev)
    for name, fn in (("manifold_metrics(k = 3)", lambda: EV.manifold_metrics(real, fake, k=3)),
                     ("kernel_distance(100 subsets of 1000)", lambda: EV.kernel_distance(real, fake))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        print(f"{name} on {n} real and {n} generated rows of {D}: {(time.perf_counter() - t0) * 1e3:.1f} ms (host clock around one call after one "
              f"warm-up call, read-back included) -> {({k: round(v, 6) for k, v in out.items()})}")


if __name__ == "__main__":
    main()
