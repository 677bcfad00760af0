#!/usr/bin/env python3
"""Times the dynamic memory's read (csrc/memory.hip through backend.functional.memory_read) against the path it replaces in a
refinement stage -- backend.functional.attention plus the torch.cat that feeds the residual blocks -- on the same image features, at
the two places of the metric configuration (gf_dim of bench.py, B = 24, T = 18): the 64x64 map of gen2 and the 128x128 map of gen3.
Device events around windows of back-to-back calls, both contenders alternated in one process, medians with the range of the windows
(the method of profiles/cond_bn_micro.py).  Then a whole eager GanTrainStep at bench.py's default workload with the plain generator and
with Generator(memory=True).

    forward:  the call on leaf operands (launch time of the host included); the parent's includes its word projection and the cat
    fwd+bwd:  forward, then torch.autograd.grad for every differentiable operand, with a gradient at x only

    python profiles/memory_micro.py           (writes profiles/memory_micro.txt; --out PATH writes elsewhere; --no-step skips the step)

The kernels of both contenders at one map size, in a run of its own (tracing slows the host):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/memory_micro.py --calls-only 128
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

B, T = 24, 18
MAPS = [64, 128]
ROUNDS, WARM, TRACE_CALLS = 9, 2, 6


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
    return f"{statistics.median(ms):8.3f} [{min(ms):7.3f},{max(ms):8.3f}]"


def operands(C, E, hw, dev, g):
    lens = torch.randint(3, T + 1, (B,), generator=g)
    lens[0] = T
    mask = (torch.arange(T).view(1, T) < lens.view(B, 1)).to(torch.int64).to(dev)
    h = torch.randn(B, C, hw, hw, generator=g).to(dev).requires_grad_(True)
    words = torch.randn(B, E, T, generator=g).to(dev).requires_grad_(True)
    w = (torch.randn(C, E, 1, 1, generator=g) / E ** 0.5).to(dev).requires_grad_(True)
    kv = (torch.relu(torch.randn(B, T, 2 * C, generator=g)) * (2.0 / C ** 0.5)).to(dev).requires_grad_(True)
    rw = (torch.randn(1, 2 * C, 1, 1, generator=g) * 0.3).to(dev).requires_grad_(True)
    rb = torch.randn(1, generator=g).to(dev).requires_grad_(True)
    dx = torch.randn(B, 2 * C, hw, hw, generator=g).to(dev)
    return h, words, w, kv, rw, rb, mask, dx


def contenders(C, E, hw, dev, g):
    h, words, w, kv, rw, rb, mask, dx = operands(C, E, hw, dev, g)

    def parent_fwd():
        ctx, _ = HF.attention(h, words, w, mask)
        return torch.cat((h, ctx), 1)

    def memory_fwd():
        return HF.memory_read(h, kv, mask, rw, rb)[0]
    parent_both = lambda: torch.autograd.grad(parent_fwd(), (h, words, w), dx)
    memory_both = lambda: torch.autograd.grad(memory_fwd(), (h, kv, rw, rb), dx)
    return parent_fwd, memory_fwd, parent_both, memory_both


def micro(lines, dev, C, E):
    g = torch.Generator().manual_seed(0)
    lines.append(f"{'map':<8s} {'C':>3s} {'T':>3s} | {'memory fwd':>26s} {'attention+cat fwd':>26s} {'x':>6s} | {'memory f+b':>26s} "
                 f"{'attention+cat f+b':>26s} {'x':>6s} | {'fwd GB/s memory / parent':>25s} | {'f+b GB/s memory / parent':>25s}")
    for hw in MAPS:
        parent_fwd, memory_fwd, parent_both, memory_both = contenders(C, E, hw, dev, g)
        calls = 8 if hw <= 64 else 3
        mf, pf = alternated([memory_fwd, parent_fwd], calls)
        mb, pb = alternated([memory_both, parent_both], calls)
        med = statistics.median
        n = B * hw * hw
        # algorithmic bytes: memory reads h and writes x and attn; the parent reads h, writes ctx and attn, then the cat reads 2C and
        # writes 2C.  Backward: memory reads h, dx, attn and writes dh; the parent's cat backward reads 2C and writes 2C (two slices made
        # contiguous), its attention backward reads h, dctx, attn and writes dh, and autograd adds the two gradients of h (2C read, C written).
        by_mf, by_pf = 4.0 * n * (C + 2 * C + T), 4.0 * n * (2 * C + T + 4 * C)
        by_mb, by_pb = by_mf + 4.0 * n * (C + 2 * C + T + C), by_pf + 4.0 * n * (4 * C + 3 * C + T + C + 3 * C)
        gb = lambda by, ms: by / (med(ms) * 1e-3) / 1e9
        apart_f = "windows apart" if max(mf) < min(pf) or max(pf) < min(mf) else "windows overlap"
        apart_b = "windows apart" if max(mb) < min(pb) or max(pb) < min(mb) else "windows overlap"
        lines.append(f"{hw}x{hw:<5d} {C:3d} {T:3d} | {fmt(mf)} {fmt(pf)} {med(mf) / med(pf):6.2f} | {fmt(mb)} {fmt(pb)} {med(mb) / med(pb):6.2f} "
                     f"| {gb(by_mf, mf):11.0f} / {gb(by_pf, pf):11.0f} | {gb(by_mb, mb):11.0f} / {gb(by_pb, pb):11.0f}   (fwd {apart_f}, f+b {apart_b})")
    lines.append(f"ms per call: median [min, max] of {ROUNDS} alternated windows after {WARM} warm-up rounds, windows of 8 (64x64) or 3 (128x128) "
                 f"back-to-back calls; B = {B}, fp32, ragged captions of 3..{T} words.  x = memory / parent (below 1: the memory read is faster).  "
                 f"parent = functional.attention (projection of the words included) + torch.cat((h, context), 1).  GB/s = algorithmic bytes over the "
                 f"call time, host launches included: forward 4 (C + 2C + T) per pixel for the memory, 4 (2C + T) + 4 (4C) for the parent.")


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
    for memory in (False, True):
        torch.manual_seed(0)
        G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND, memory=memory).to(dev)
        Ds = [DISC.Disc64(bench.DF).to(dev), DISC.Disc128(bench.DF).to(dev), DISC.Disc256(bench.DF).to(dev)]
        enc = ENC.StandInImageEncoder(bench.EMB).to(dev)
        enc.freeze_all_weights()
        enc.eval()
        steps.append(TR.GanTrainStep(G, Ds, enc))
    run = lambda s: (lambda: s.step(words, sent, lens, None, reals))
    off, mem, off2 = alternated([run(steps[0]), run(steps[1]), run(steps[0])], 5)
    med = statistics.median
    base = med(off + off2)
    lines.append("")
    lines.append(f"GanTrainStep, bench.py's default workload (Generator({bench.GF}, {bench.EMB}, {bench.Z}, {bench.COND}), Disc64/128/256({bench.DF}), "
                 f"batch {batch}, fp32, eager), ms/step median [min, max]: plain {fmt(off + off2)} ({batch / base * 1e3:.1f} images/s); "
                 f"memory=True {fmt(mem)} ({batch / med(mem) * 1e3:.1f} images/s, x {med(mem) / base:.4f}); the plain step against itself: "
                 f"|median of its first windows - median of its second| = {100 * abs(med(off) - med(off2)) / base:.2f}% "
                 f"(windows of 5 steps, {ROUNDS} alternated rounds after {WARM} warm-up rounds).")


def main():
    if not torch.cuda.is_available():
        sys.exit("memory_micro: needs an MI355X (timings on a CPU say nothing about it)")
    import bench
    dev = "cuda"
    C, E = bench.GF, bench.EMB
    if "--calls-only" in sys.argv:                  # for a kernel trace: TRACE_CALLS forward + backward calls of both at one map size
        hw = int(sys.argv[sys.argv.index("--calls-only") + 1])
        _, _, parent_both, memory_both = contenders(C, E, hw, dev, torch.Generator().manual_seed(0))
        for _ in range(TRACE_CALLS):
            memory_both()
            parent_both()
        torch.cuda.synchronize()
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "memory_micro.txt")
    lines = [f"library: {os.path.relpath(L.LIB_PATH, os.path.dirname(HERE))}"]
    micro(lines, dev, C, E)
    if "--no-step" not in sys.argv:
        whole_step(lines, dev)
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
