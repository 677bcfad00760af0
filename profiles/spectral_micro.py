#!/usr/bin/env python3
"""Times spectral normalisation of a weight (csrc/spectral.hip through backend.functional.spectral_weight) against the same formulas made
of stock torch ops on the GPU (functional.spectral_weight_reference, autograd for the backward) at real matrices of the metric
configuration's discriminators (df = 64): the first conv 64 x 48, 512 x 4096, the largest 2048 x 16384, 1024 x 18432 and the 1 x 8192
logit head.  Device events around windows of back-to-back calls, the contenders alternated in one process, medians with the range of the
windows (the method of profiles/word_corr_micro.py).  Achieved bytes/s are against the four-pass minimum of a direction (forward: W read
three times, W_sn written once; backward the same count), so forward moves 16 bytes per weight and forward + backward 32.  Then a whole
eager GanTrainStep at bench.py's default workload with norm="batch" and norm="spectral" discriminators, alternated.

    forward:  the call on a leaf weight in training mode (one power iteration; launch time of the host included)
    fwd+bwd:  forward, then torch.autograd.grad for the weight with a gradient at weight_sn

    python profiles/spectral_micro.py     (writes profiles/spectral_micro.txt; --out PATH writes elsewhere; --no-step skips the step)
"""
import importlib
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")

SHAPES = [(64, 48), (512, 4096), (2048, 16384), (1024, 18432), (1, 8192)]
ROUNDS, WARM = 9, 2


def alternated(fns, calls):
    """ms per call of every callable, one list entry per round; the callables run in turn WARM + ROUNDS times, a timed window is `calls`
    back-to-back calls between one pair of events"""
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
    return ms


def fmt(ms):
    return f"{statistics.median(ms):8.4f} [{min(ms):7.4f},{max(ms):8.4f}]"


def apart(a, b):
    return "windows apart" if max(a) < min(b) or max(b) < min(a) else "windows overlap"


def micro(lines, dev):
    g = torch.Generator().manual_seed(0)
    med = statistics.median
    for cout, K in SHAPES:
        w = (torch.randn(cout, K, generator=g) * K ** -0.5).to(dev).requires_grad_(True)
        d = torch.randn(cout, K, generator=g).to(dev)
        u = torch.nn.functional.normalize(torch.randn(cout, generator=g), dim=0).to(dev)
        v = torch.nn.functional.normalize(torch.randn(K, generator=g), dim=0).to(dev)
        ours_f = lambda: HF.spectral_weight(w, u, v, True)
        stock_f = lambda: HF.spectral_weight_reference(w, u, v, True)
        ours_b = lambda: torch.autograd.grad(ours_f(), (w,), d)
        stock_b = lambda: torch.autograd.grad(stock_f(), (w,), d)
        calls = 4 if cout * K > 1 << 22 else 16
        of, sf = alternated([ours_f, stock_f], calls)
        ob, sb = alternated([ours_b, stock_b], calls)
        tb = lambda ms, passes: 4.0 * cout * K * passes / (med(ms) * 1e-3) / 1e12
        lines.append(f"{cout:5d} x {K:5d} ({4 * cout * K / 2 ** 20:7.2f} MiB) | kernels fwd {fmt(of)} ({tb(of, 4):5.2f} TB/s of the 4-pass minimum)  stock torch fwd "
                     f"{fmt(sf)}  x {med(of) / med(sf):6.3f} | kernels f+b {fmt(ob)} ({tb(ob, 8):5.2f} TB/s of 8 passes)  stock torch f+b {fmt(sb)}  "
                     f"x {med(ob) / med(sb):6.3f}   (fwd {apart(of, sf)}, f+b {apart(ob, sb)})")
    lines.append(f"ms per call: median [min, max] of {ROUNDS} alternated windows after {WARM} warm-up rounds, windows of 16 back-to-back calls (4 above "
                 f"16 MiB); fp32, W ~ N(0, K^-1/2), one power iteration per call.  x = kernels / stock (below 1: the kernels are faster).  stock = "
                 f"functional.spectral_weight_reference on the device (mv, normalize, dot, a division; autograd backward).  Back-to-back calls on one "
                 f"matrix: a matrix below the 256 MiB Infinity Cache stays in it from call to call, which a training step's forward does not grant.")


def whole_step(lines, dev):
    import bench
    GEN = importlib.import_module("attention-gan_amd.networks.generator")
    DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
    ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
    TR = importlib.import_module("attention-gan_amd.trainers.trainer")
    batch = bench.WORKLOADS["full3"]["batch"]
    words, sent, lens, reals = bench.synthetic_batch(dev, batch, seed=1234)
    lens = torch.tensor(lens, dtype=torch.int64, device=dev)
    steps = []
    for norm in ("batch", "spectral"):
        torch.manual_seed(0)
        G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND).to(dev)
        Ds = [c(bench.DF, norm=norm).to(dev) for c in (DISC.Disc64, DISC.Disc128, DISC.Disc256)]
        enc = ENC.StandInImageEncoder(bench.EMB).to(dev)
        enc.freeze_all_weights()
        enc.eval()
        steps.append(TR.GanTrainStep(G, Ds, enc))
    run = lambda s: (lambda: s.step(words, sent, lens, None, reals))
    off, on, off2 = alternated([run(steps[0]), run(steps[1]), run(steps[0])], 5)
    med = statistics.median
    base = med(off + off2)
    lines.append("")
    lines.append(f"GanTrainStep, bench.py's default workload (Generator({bench.GF}, {bench.EMB}, {bench.Z}, {bench.COND}), Disc64/128/256({bench.DF}), "
                 f"batch {batch}, fp32, eager, StandInImageEncoder), ms/step median [min, max]: norm=\"batch\" {fmt(off + off2)} "
                 f"({batch / base * 1e3:.1f} images/s); norm=\"spectral\" {fmt(on)} ({batch / med(on) * 1e3:.1f} images/s, x {med(on) / base:.4f}, "
                 f"{med(on) - base:+.3f} ms); the batch step against itself: |median of its first windows - median of its second| = "
                 f"{100 * abs(med(off) - med(off2)) / base:.2f}% (windows of 5 steps, {ROUNDS} alternated rounds after {WARM} warm-up rounds).")


def main():
    if not torch.cuda.is_available():
        sys.exit("spectral_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "spectral_micro.txt")
    lines = [f"library: {os.path.relpath(L.LIB_PATH, os.path.dirname(HERE))}"]
    micro(lines, dev)
    if "--no-step" not in sys.argv:
        whole_step(lines, dev)
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
