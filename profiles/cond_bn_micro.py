#!/usr/bin/env python3
"""Times the sentence-conditioned BatchNorm (csrc/cond_bn.hip through backend.functional.cond_bn_act) against the plain fused
BatchNorm (backend.functional.bn_act, unchanged) at the six up-block shapes of the metric configuration -- gf_dim 32, B = 24, GLU:
512 channels at 8x8 up to 64 channels at 256x256 -- and a whole GanTrainStep at bench.py's default workload with cond_bn off and on.
Device events around windows of back-to-back calls, both contenders alternated in one process, medians -- the method of
profiles/iscore_micro.py.  bn_act is timed TWICE per round (before and after the conditional call): the distance of its two medians
and the range of its windows are the run-to-run spread a ratio has to be read against.

    forward:  the autograd Function's forward on a leaf input (statistics + apply; the workspace allocation and the host's launch time
              included)
    fwd+bwd:  forward, then torch.autograd.grad for x, gamma, beta (and delta): the backward is the difference of the two columns

    python profiles/cond_bn_micro.py            (writes profiles/cond_bn_micro.txt; --out PATH writes elsewhere; --no-step skips the step)

The kernels of both contenders at one shape, in a run of its own (tracing slows the host; DESIGN.md section 22 quotes the medians):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/cond_bn_micro.py --calls-only 64 128
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

B = 24
SHAPES = [("gen1.upsample1", 512, 8), ("gen1.upsample2", 256, 16), ("gen1.upsample3", 128, 32), ("gen1.upsample4", 64, 64),
          ("gen2.upsample", 64, 128), ("gen3.upsample", 64, 256)]          # name, channels of the conv output, map side
ROUNDS, WARM, TRACE_CALLS = 9, 2, 12


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


def spread(a, b):
    """run-to-run spread of one contender timed twice: the distance of its two medians and the range of all its windows, over the median"""
    m = statistics.median(a + b)
    return abs(statistics.median(a) - statistics.median(b)) / m, (max(a + b) - min(a + b)) / m


def operands(C, side, dev, g):
    x = torch.randn(B, C, side, side, generator=g).to(dev).requires_grad_(True)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g)).to(dev).requires_grad_(True)
    delta = (0.3 * torch.randn(B, 2 * C, generator=g)).to(dev).requires_grad_(True)
    rm, rv, nbt = torch.zeros(C, device=dev), torch.ones(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    dout = torch.randn(B, C // 2, side, side, generator=g).to(dev)
    return x, gamma, beta, delta, rm, rv, nbt, dout


def micro(lines, dev):
    g = torch.Generator().manual_seed(0)
    lines.append(f"{'layer':<15s} {'C':>4s} {'HxW':>8s} {'MB of x':>8s} | {'bn_act fwd':>10s} {'cond fwd':>9s} {'ratio':>6s} {'spread':>13s} | "
                 f"{'bn_act f+b':>10s} {'cond f+b':>9s} {'ratio':>6s} {'spread':>13s} | {'bwd ratio':>9s}")
    for name, C, side in SHAPES:
        x, gamma, beta, delta, rm, rv, nbt, dout = operands(C, side, dev, g)

        def bn_fwd():
            return HF.bn_act(x, gamma, beta, rm, rv, nbt, True, L.ACT_GLU)

        def cbn_fwd():
            return HF.cond_bn_act(x, gamma, beta, delta, rm, rv, nbt, True, L.ACT_GLU)

        def bn_both():
            torch.autograd.grad(bn_fwd(), (x, gamma, beta), dout)

        def cbn_both():
            torch.autograd.grad(cbn_fwd(), (x, gamma, beta, delta), dout)
        calls = 40 if side <= 32 else (10 if side <= 128 else 4)
        f0, fc, f1 = alternated([bn_fwd, cbn_fwd, bn_fwd], calls)
        b0, bc, b1 = alternated([bn_both, cbn_both, bn_both], calls)
        med = statistics.median
        fb, fcm, bb, bcm = med(f0 + f1), med(fc), med(b0 + b1), med(bc)
        sf, sb = spread(f0, f1), spread(b0, b1)
        lines.append(f"{name:<15s} {C:4d} {side:>4d}x{side:<3d} {x.numel() * 4 / 1e6:8.1f} | {fb:10.4f} {fcm:9.4f} {fcm / fb:6.3f} "
                     f"{100 * sf[0]:5.1f}% /{100 * sf[1]:5.1f}% | {bb:10.4f} {bcm:9.4f} {bcm / bb:6.3f} {100 * sb[0]:5.1f}% /{100 * sb[1]:5.1f}% | "
                     f"{(bcm - fcm) / (bb - fb):9.3f}")
        del x, dout
    lines.append(f"ms per call, B = {B}, GLU, fp32; windows of 40 (maps up to 32x32), 10 (up to 128x128) or 4 back-to-back calls; medians of {ROUNDS} "
                 f"alternated rounds after {WARM} warm-up rounds; bn_act = both of its windows per round.  ratio = cond / bn_act.  spread = bn_act "
                 f"against itself: |median of its first windows - median of its second| / its range over all windows, over its median.  "
                 f"bwd ratio = (cond f+b - cond fwd) / (bn_act f+b - bn_act fwd).")


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
    for cond_bn in (False, True):
        torch.manual_seed(0)
        G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND, cond_bn=cond_bn).to(dev)
        Ds = [DISC.Disc64(bench.DF).to(dev), DISC.Disc128(bench.DF).to(dev), DISC.Disc256(bench.DF).to(dev)]
        enc = ENC.StandInImageEncoder(bench.EMB).to(dev)
        enc.freeze_all_weights()
        enc.eval()
        steps.append(TR.GanTrainStep(G, Ds, enc))
    off, on = steps
    run = lambda s: (lambda: s.step(words, sent, lens, None, reals))
    a0, c, a1 = alternated([run(off), run(on), run(off)], 5)
    med = statistics.median
    s = spread(a0, a1)
    lines.append("")
    lines.append(f"GanTrainStep, bench.py's default workload (Generator({bench.GF}, {bench.EMB}, {bench.Z}, {bench.COND}), Disc64/128/256({bench.DF}), "
                 f"batch {batch}, fp32, eager): cond_bn off {med(a0 + a1):.3f} ms/step ({batch / med(a0 + a1) * 1e3:.1f} images/s), on {med(c):.3f} ms/step "
                 f"({batch / med(c) * 1e3:.1f} images/s), ratio {med(c) / med(a0 + a1):.4f}; spread of the off step against itself "
                 f"{100 * s[0]:.2f}% / {100 * s[1]:.2f}% (windows of 5 steps, {ROUNDS} alternated rounds after {WARM} warm-up rounds).")


def main():
    if not torch.cuda.is_available():
        sys.exit("cond_bn_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    if "--calls-only" in sys.argv:                  # for a kernel trace: TRACE_CALLS forward + backward calls of both at one shape
        C, side = (int(v) for v in sys.argv[sys.argv.index("--calls-only") + 1:][:2])
        x, gamma, beta, delta, rm, rv, nbt, dout = operands(C, side, dev, torch.Generator().manual_seed(0))
        for _ in range(TRACE_CALLS):
            torch.autograd.grad(HF.bn_act(x, gamma, beta, rm, rv, nbt, True, L.ACT_GLU), (x, gamma, beta), dout)
            torch.autograd.grad(HF.cond_bn_act(x, gamma, beta, delta, rm, rv, nbt, True, L.ACT_GLU), (x, gamma, beta, delta), dout)
        torch.cuda.synchronize()
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "cond_bn_micro.txt")
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
