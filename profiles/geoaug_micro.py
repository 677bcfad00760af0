#!/usr/bin/env python3
"""Times the geometric augmentation kernels (csrc/geoaug.hip through backend.functional.affine_warp) against torch's own bilinear
warp -- F.affine_grid + F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False) with the equivalent matrix, and its
autograd, whose backward scatters with float atomics -- on the same device, with device events around windows of back-to-back calls,
alternated windows, medians:

    forward      library: agan_affine_warp_fwd (one launch)                 torch: affine_grid + grid_sample
    backward     library: agan_affine_warp_bwd (one launch, a gather)       torch: autograd through grid_sample

at the three image sizes of a batch-48 train step, matrices of all five stages, and reports the library's TB/s of bytes OWED: the
input read once and the output written once, 8 bytes per element.  The `kernels` columns are the two C entries alone on preallocated
buffers; `matrix` is the one launch that builds the 9 * 48 matrices of a step.  Last, the images/s of GanTrainStep.train_epoch in f32
with and without the geometric stages, runs alternated, as a difference against the same tree without the flag.  None of these is a
pass bar.  Not run by bench.py.

    python profiles/geoaug_micro.py > profiles/geoaug_micro.txt
"""
import importlib
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HF = importlib.import_module("attention-gan_amd.backend.functional")
A = importlib.import_module("attention-gan_amd.augment")

SHAPES = [(48, 3, 256, 256), (48, 3, 128, 128), (48, 3, 64, 64)]
GEOMETRY = "xflip,rot90,scale,rotate,aniso"
ROUNDS, WARM, CALLS = 9, 2, 200
EPOCH_STEPS, EPOCH_ROUNDS = 10, 5


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


def theta_of(M, H, W):
    """the [N, 2, 3] matrix of F.affine_grid (normalised coordinates, align_corners=False) that states the same map as M"""
    a, b, tx, c, d, ty = M.unbind(dim=1)
    return torch.stack([torch.stack([a, b * (H / W), 2 * tx], dim=1), torch.stack([c * (W / H), d, 2 * ty], dim=1)], dim=1)


def torch_warp(x, theta):
    return F.grid_sample(x, F.affine_grid(theta, list(x.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)


def raw_calls(x, M):
    """(forward, backward) closures on the C entries with preallocated outputs: the kernels alone"""
    N, C, H, W = x.shape
    y = torch.empty_like(x)
    fwd = lambda: HF.L.call("agan_affine_warp_fwd", HF._p(x), None, N, 0, HF._p(M), HF._p(y), C, H, W, HF._stream())
    bwd = lambda: HF.L.call("agan_affine_warp_bwd", HF._p(x), HF._p(M), HF._p(y), N, C, H, W, HF._stream())
    return fwd, bwd


def main():
    if not torch.cuda.is_available():
        sys.exit("geoaug_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = torch.device("cuda", 0)
    geometry = A.parse_geometry(GEOMETRY)
    g = torch.Generator().manual_seed(0)
    print(f"library: {os.path.relpath(HF.L.LIB_PATH, ROOT)}; geometry {GEOMETRY!r}")
    print(f"{'shape':>18s} | {'fwd ms':>7s} {'torch ms':>9s} {'ratio':>6s} {'TB/s owed':>9s} | {'bwd ms':>7s} {'torch ms':>9s} {'ratio':>6s} {'TB/s owed':>9s} | "
          f"{'kernels fwd':>11s} {'TB/s':>5s} {'bwd':>6s} {'TB/s':>5s} | {'max |lib - torch|':>17s}")
    for shape in SHAPES:
        N, C, H, W = shape
        x = torch.randn(shape, generator=g).to(dev)
        r = torch.randn(shape, generator=g).to(dev)
        M = HF.geometry_matrices(torch.rand(N, 16, generator=g).to(dev), geometry)
        theta = theta_of(M, H, W)
        owed = 8.0 * x.numel()
        xg = x.clone().requires_grad_(True)
        diff = float((HF.affine_warp(x, M) - torch_warp(x, theta)).abs().max())          # the two really state one map

        def lib_bwd():
            xg.grad = None
            HF.affine_warp(xg, M).backward(r)

        def torch_bwd():
            xg.grad = None
            torch_warp(xg, theta).backward(r)

        tf, ttf = alternated([lambda: HF.affine_warp(x, M), lambda: torch_warp(x, theta)], CALLS)
        tfb, ttfb = alternated([lib_bwd, torch_bwd], CALLS)
        tb, ttb = tfb - tf, ttfb - ttf                                 # the backward's own share of forward + backward
        kf, kb = alternated(list(raw_calls(x, M)), CALLS)
        tbs = lambda ms: owed / ms / 1e9
        print(f"{str(list(shape)):>18s} | {tf:7.4f} {ttf:9.4f} {tf / ttf:6.3f} {tbs(tf):9.2f} | {tb:7.4f} {ttb:9.4f} {tb / ttb:6.3f} {tbs(tb):9.2f} | "
              f"{kf:11.4f} {tbs(kf):5.2f} {kb:6.4f} {tbs(kb):5.2f} | {diff:17.2e}")
    gs = torch.rand(9 * SHAPES[0][0], 16, generator=g).to(dev)
    p = torch.full((1,), 0.5, device=dev)
    tm, tmg = alternated([lambda: HF.geometry_matrices(gs, geometry), lambda: HF.geometry_matrices(gs, geometry, p)], CALLS)
    print(f"matrix: {tm:.4f} ms for the {gs.shape[0]} matrices of a batch-{SHAPES[0][0]} step, {tmg:.4f} ms with the gates (one launch, allocation and host time included)")
    print(f"fwd / bwd: backend.functional.affine_warp and its autograd backward (output allocation and host launch time included; bwd = "
          f"[forward + backward] - [forward]); torch: F.affine_grid + F.grid_sample (bilinear, zeros, align_corners=False) with the equivalent "
          f"matrix, and autograd through it.  ratio = library / torch.  kernels: the two C entries alone on preallocated buffers.  TB/s owed = "
          f"8 bytes per element (input read once, output written once) over the time.  Per call, from windows of {CALLS} back-to-back calls; "
          f"medians of {ROUNDS} alternated windows after {WARM} warm-up rounds.")

    # ---- the train step with and without the geometric stages ---------------------------------------------------------------
    import bench
    B = SHAPES[0][0]
    steps = [bench.build(dev, B, HF), bench.build(dev, B, HF)]
    steps[1].geometry = geometry                                       # (bench.build knows no geometry: the attribute is all the constructor sets)
    words, sent, lens, reals = bench.synthetic_batch(dev, B, seed=1)
    batch = (torch.zeros(B, bench.T, dtype=torch.int64), lens, None, reals[0], reals[1], reals[2])
    encoder = lambda w, l: (words, sent)
    rates = [[], []]
    for rnd in range(2 + EPOCH_ROUNDS):
        for i, st in enumerate(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = st.train_epoch([batch] * EPOCH_STEPS, encoder, B)
            torch.cuda.synchronize()
            if rnd >= 2:
                rates[i].append(B * n / (time.perf_counter() - t0))
    off, on = (statistics.median(v) for v in rates)
    print()
    print(f"train_epoch, f32, batch {B}, eager: {off:.1f} images/s without the flag, {on:.1f} images/s with geometry={GEOMETRY!r} ({100 * (on / off - 1):+.2f}%)")
    print(f"(median of {EPOCH_ROUNDS} alternated runs of {EPOCH_STEPS} steps after 2 warm-up runs, wall clock around the epoch with a device "
          f"synchronisation; 9 warped tensors per step in 6 calls = 6 forward launches, plus the 3 backward launches of the generator update, one torch.rand and one matrix launch, in place of 3 torch.cat)")


if __name__ == "__main__":
    main()
