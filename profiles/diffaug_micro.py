#!/usr/bin/env python3
"""Times the augmentation kernels (csrc/diffaug.hip through backend.functional.diffaug) against augment.diffaug_reference -- the same
transform in torch ops -- on the same device, with device events around windows of back-to-back calls, alternated windows, medians:

    forward      library: agan_diffaug_fwd (sum launch + apply launch)          torch: diffaug_reference(x, u, policy)
    backward     library: agan_diffaug_bwd (masked sum launch + apply launch)   torch: autograd through diffaug_reference

at the three image sizes of a batch-48 train step, policy "color,translation,cutout", and reports the library's TB/s of bytes OWED: the
input read twice (once per launch) and the output written once, 12 bytes per element.  A second table times the apply launch's two
load forms on the same data: rows of whole 16-byte chunks (a lane loads the two aligned float4 that cover its four shifted sources)
against the one-pixel-per-lane form (dword loads and stores), which the library takes for a tensor whose base is not 16-byte
aligned -- here a view one float into a larger buffer.  Last, the images/s of GanTrainStep.train_epoch in f32 with and without the
policy, runs alternated.  None of these is a pass bar.  Not run by bench.py.

    python profiles/diffaug_micro.py > profiles/diffaug_micro.txt
"""
import importlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HF = importlib.import_module("attention-gan_amd.backend.functional")
A = importlib.import_module("attention-gan_amd.augment")

SHAPES = [(48, 3, 256, 256), (48, 3, 128, 128), (48, 3, 64, 64)]
POLICY = "color,translation,cutout"
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


def raw_calls(x, u, policy):
    """(forward, backward) closures on the C entries with preallocated output and workspace: the kernels alone"""
    N, C, H, W = x.shape
    nbytes = HF.L.load().agan_diffaug_ws_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(x.numel() + 4, device=x.device)
    y = out[:x.numel()].view_as(x) if x.data_ptr() % 16 == 0 else out[1:1 + x.numel()].view_as(x)     # aligned like its source
    fwd = lambda: HF.L.call("agan_diffaug_fwd", HF._p(x), None, N, 0, HF._p(u), policy, HF._p(y), C, H, W, HF._p(ws), nbytes, HF._stream())
    bwd = lambda: HF.L.call("agan_diffaug_bwd", HF._p(x), HF._p(u), policy, HF._p(y), N, C, H, W, HF._p(ws), nbytes, HF._stream())
    return fwd, bwd


def main():
    if not torch.cuda.is_available():
        sys.exit("diffaug_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = torch.device("cuda", 0)
    policy = A.parse_policy(POLICY)
    g = torch.Generator().manual_seed(0)
    print(f"library: {os.path.relpath(HF.L.LIB_PATH, ROOT)}; policy {POLICY!r}")
    print(f"{'shape':>18s} | {'fwd ms':>7s} {'torch ms':>9s} {'ratio':>6s} {'TB/s owed':>9s} | {'bwd ms':>7s} {'torch ms':>9s} {'ratio':>6s} {'TB/s owed':>9s} | "
          f"{'kernels fwd':>11s} {'TB/s':>5s} {'bwd':>6s} {'TB/s':>5s} | {'one-pixel fwd':>13s} {'TB/s':>5s} {'bwd':>6s} {'TB/s':>5s}")
    for shape in SHAPES:
        x = torch.randn(shape, generator=g).to(dev)
        r = torch.randn(shape, generator=g).to(dev)
        u = torch.rand(shape[0], 8, generator=g).to(dev)
        owed = 12.0 * x.numel()
        xg = x.clone().requires_grad_(True)

        def lib_bwd():
            xg.grad = None
            HF.diffaug(xg, u, policy).backward(r)

        def torch_bwd():
            xg.grad = None
            A.diffaug_reference(xg, u, policy).backward(r)

        tf, ttf = alternated([lambda: HF.diffaug(x, u, policy), lambda: A.diffaug_reference(x, u, policy)], CALLS)
        tfb, ttfb = alternated([lib_bwd, torch_bwd], CALLS)
        tb, ttb = tfb - tf, ttfb - ttf                                 # the backward's own share of forward + backward
        kf, kb = alternated(list(raw_calls(x, u, policy)), CALLS)
        big = torch.empty(x.numel() + 4, device=dev)
        xo = big[1:1 + x.numel()].view_as(x)
        xo.copy_(x)
        of, ob = alternated(list(raw_calls(xo, u, policy)), CALLS)
        tbs = lambda ms: owed / ms / 1e9
        print(f"{str(list(shape)):>18s} | {tf:7.4f} {ttf:9.4f} {tf / ttf:6.3f} {tbs(tf):9.2f} | {tb:7.4f} {ttb:9.4f} {tb / ttb:6.3f} {tbs(tb):9.2f} | "
              f"{kf:11.4f} {tbs(kf):5.2f} {kb:6.4f} {tbs(kb):5.2f} | {of:13.4f} {tbs(of):5.2f} {ob:6.4f} {tbs(ob):5.2f}")
    print(f"fwd / bwd: backend.functional.diffaug and its autograd backward (output and workspace allocation and host launch time included; bwd = "
          f"[forward + backward] - [forward]); torch: augment.diffaug_reference in fp32 and autograd through it.  ratio = library / torch.  "
          f"kernels: the two C entries alone on preallocated buffers.  one-pixel: the same entries on a tensor one float off the 16-byte grid "
          f"(dword loads and stores, one pixel per lane).  TB/s owed = 12 bytes per element (input read by the sum launch and by the apply "
          f"launch, output written once) over the time.  Per call, from windows of {CALLS} back-to-back calls; medians of {ROUNDS} "
          f"alternated windows after {WARM} warm-up rounds.")

    # ---- the train step with and without the policy --------------------------------------------------------------------------
    import bench
    B = SHAPES[0][0]
    steps = [bench.build(dev, B, HF), bench.build(dev, B, HF)]
    steps[1].augment = policy                                          # (bench.build knows no policy: the attribute is all the constructor sets)
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
    print(f"train_epoch, f32, batch {B}, eager: {off:.1f} images/s without augmentation, {on:.1f} images/s with {POLICY!r} ({100 * (on / off - 1):+.2f}%)")
    print(f"(median of {EPOCH_ROUNDS} alternated runs of {EPOCH_STEPS} steps after 2 warm-up runs, wall clock around the epoch with a device "
          f"synchronisation; 9 augmented tensors per step in 6 calls = 12 forward launches, plus 6 backward launches and one torch.rand, in place of 3 torch.cat)")


if __name__ == "__main__":
    main()
