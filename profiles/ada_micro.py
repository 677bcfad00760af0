#!/usr/bin/env python3
"""Times the gated augmentation entries (agan_diffaug_gated_fwd / _bwd, csrc/diffaug.hip) next to the ungated ones of the same build, the
ungated entries of this build next to those of another build of the library (the parent commit's, given with --parent-lib), and
GanTrainStep.train_epoch with `augment` alone and with `ada_target=0.6`.  The method is profiles/diffaug_micro.py's: device events
around windows of 200 back-to-back calls on preallocated buffers, the candidates alternated, medians of 9 windows after 2 warm-up
rounds; the spread printed is (max - min) / median of those 9 windows.  None of these is a pass bar.  Not run by bench.py.

    python profiles/ada_micro.py [--parent-lib path/to/parent/libagan_hip.so] > profiles/ada_micro.txt
"""
import argparse
import ctypes
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
PS = (0.0, 0.5, 1.0)
ROUNDS, WARM, CALLS = 9, 2, 200
EPOCH_STEPS, EPOCH_ROUNDS = 10, 5


def alternated(fns, calls=CALLS):
    """[(median ms per call, spread)] of every callable, the callables run in turn"""
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
    return [(statistics.median(m), (max(m) - min(m)) / statistics.median(m)) for m in ms]


def entries(lib, x, u, policy, q=None, p=None):
    """(forward, backward) closures on `lib`'s C entries with preallocated output and workspace: the kernels alone"""
    N, C, H, W = x.shape
    nbytes = HF.L.load().agan_diffaug_ws_bytes(N, C, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    y = torch.empty_like(x)
    P, st = HF._p, HF._stream

    def check(code):
        if code != 0:
            raise RuntimeError(f"library call failed with {code}")

    if q is None:
        return (lambda: check(lib.agan_diffaug_fwd(P(x), None, N, 0, P(u), policy, P(y), C, H, W, P(ws), nbytes, st())),
                lambda: check(lib.agan_diffaug_bwd(P(x), P(u), policy, P(y), N, C, H, W, P(ws), nbytes, st())), (y, ws))
    return (lambda: check(lib.agan_diffaug_gated_fwd(P(x), None, N, 0, P(u), P(q), P(p), policy, P(y), C, H, W, P(ws), nbytes, st())),
            lambda: check(lib.agan_diffaug_gated_bwd(P(x), P(u), P(q), P(p), policy, P(y), N, C, H, W, P(ws), nbytes, st())), (y, ws))


def parent_library(path):
    lib = ctypes.CDLL(path)
    sig = HF.L._SIGNATURES
    for name in ("agan_diffaug_fwd", "agan_diffaug_bwd"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sig[name]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="another build of libagan_hip.so whose ungated entries are timed next to this build's")
    ap.add_argument("--no-epoch", action="store_true", help="skip the train_epoch comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ada_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = torch.device("cuda", 0)
    policy = A.parse_policy(POLICY)
    lib = HF.L.load()
    g = torch.Generator().manual_seed(0)
    print(f"library: {os.path.relpath(HF.L.LIB_PATH, ROOT)}; policy {POLICY!r}; ms per call (spread of the {ROUNDS} windows)")
    fmt = lambda t: f"{t[0]:7.4f} ({100 * t[1]:4.1f}%)"
    data = []
    print(f"{'shape':>18s} | {'':3s} | {'ungated':>15s} | " + " | ".join(f"{'gated p = ' + str(p):>15s}" for p in PS) + f" | {'copy_':>15s}")
    for shape in SHAPES:
        x = torch.randn(shape, generator=g).to(dev)
        u = torch.rand(shape[0], 8, generator=g).to(dev)
        q = torch.rand(shape[0], 4, generator=g).to(dev)
        data.append((x, u))
        ungated = entries(lib, x, u, policy)
        gated = [entries(lib, x, u, policy, q, torch.tensor([p], device=dev)) for p in PS]
        y = torch.empty_like(x)
        fwd = alternated([ungated[0]] + [e[0] for e in gated] + [lambda: y.copy_(x)])
        bwd = alternated([ungated[1]] + [e[1] for e in gated])
        on = [int((A.gate_masks(q, p).sum(0)).tolist()[0]) for p in PS]
        print(f"{str(list(shape)):>18s} | fwd | " + " | ".join(fmt(t) for t in fwd))
        print(f"{'colour on: ' + '/'.join(map(str, on)) + ' of ' + str(shape[0]):>18s} | bwd | " + " | ".join(fmt(t) for t in bwd))
    print("the C entries alone on preallocated buffers.  copy_: torch's device copy of the same tensor (8 bytes per element).")

    if args.parent_lib:
        parent = parent_library(args.parent_lib)
        print()
        print(f"ungated entries: this build against {os.path.basename(os.path.dirname(os.path.abspath(args.parent_lib)))}/"
              f"{os.path.basename(args.parent_lib)} (the parent commit's build), alternated")
        print(f"{'shape':>18s} | {'':3s} | {'this build':>15s} | {'parent':>15s} | {'this / parent':>13s}")
        for x, u in data:
            mine, theirs = entries(lib, x, u, policy), entries(parent, x, u, policy)
            for tag, k in (("fwd", 0), ("bwd", 1)):
                a, b = alternated([mine[k], theirs[k]])
                print(f"{str(list(x.shape)):>18s} | {tag} | {fmt(a)} | {fmt(b)} | {a[0] / b[0]:13.4f}")
            ya, yb = mine[2][0], theirs[2][0]
            mine[0](), theirs[0]()
            torch.cuda.synchronize()
            print(f"{'':>18s} |     | forward bytes equal: {torch.equal(ya.view(torch.int32), yb.view(torch.int32))}")

    if args.no_epoch:
        return
    # ---- the train step with the policy alone and with adaptation ------------------------------------------------------------
    import bench
    B = SHAPES[0][0]
    steps = [bench.build(dev, B, HF), bench.build(dev, B, HF)]
    for st in steps:
        st.augment = policy                                            # (bench.build knows no policy: the attribute is all the constructor sets)
    steps[1].ada = A.AdaController(dev, len(steps[1].Ds), p=0.0, target=0.6)       # ... and this is all `ada_target=0.6` sets
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
    spread = [(max(v) - min(v)) / statistics.median(v) for v in rates]
    print()
    print(f"train_epoch, f32, batch {B}, eager: {off:.1f} images/s with {POLICY!r} alone (spread {100 * spread[0]:.1f}%), {on:.1f} images/s with "
          f"ada_target=0.6 (spread {100 * spread[1]:.1f}%) ({100 * (on / off - 1):+.2f}%); the controller after the run: {steps[1].ada.sync()}")
    print(f"(median of {EPOCH_ROUNDS} alternated runs of {EPOCH_STEPS} steps after 2 warm-up runs, wall clock around the epoch with a device "
          f"synchronisation; adaptation adds one torch.rand, three observe launches and one update launch per step)")


if __name__ == "__main__":
    main()
