#!/usr/bin/env python3
"""Times the fused self-attention (csrc/self_attn.hip through backend.functional.self_attention) against the composed torch form --
bmm, softmax, bmm under autograd, stock ATen kernels -- on the same operands, at the two places the block can sit in the metric
configuration (gf_dim 32, B = 24): the 32x32 map (Dk 8, Dv 32, N 1024) and the 64x64 map (Dk 4, Dv 16, N 4096).  Device events around
windows of back-to-back calls, both contenders alternated in one process, medians with the range of the windows -- the method of
profiles/cond_bn_micro.py.  Peak memory of one forward + backward of each is read from torch's allocator.  Then a whole eager
GanTrainStep at bench.py's default workload with self_attn None, 32 and 64.

    forward:  the call on leaf operands (launch time of the host included)
    fwd+bwd:  forward, then torch.autograd.grad for q, k, v

    python profiles/self_attn_micro.py           (writes profiles/self_attn_micro.txt; --out PATH writes elsewhere; --no-step skips the step)

The kernels of both contenders at one shape, in a run of its own (tracing slows the host; DESIGN.md section 23 quotes the medians):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/self_attn_micro.py --calls-only 4 16 4096
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
SHAPES = [("32x32 map", 8, 32, 1024), ("64x64 map", 4, 16, 4096)]          # name, Dk, Dv, N (= M)
ROUNDS, WARM, TRACE_CALLS = 9, 2, 6
PEAK_F32_MFMA = 256 * 4 * 64 * 2.4e9          # FLOP/s: 256 CUs x 4 SIMDs x 64 FLOP per clock x 2.4 GHz


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


def composed(q, k, v):
    p = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=2)
    return torch.bmm(v, p.transpose(1, 2))


def operands(Dk, Dv, N, dev, g):
    q, k, v = (torch.randn(B, d, N, generator=g).to(dev).requires_grad_(True) for d in (Dk, Dk, Dv))
    return q, k, v, torch.randn(B, Dv, N, generator=g).to(dev)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def fmt(ms):
    return f"{statistics.median(ms):8.3f} [{min(ms):7.3f},{max(ms):8.3f}]"


def micro(lines, dev):
    g = torch.Generator().manual_seed(0)
    lines.append(f"{'place':<10s} {'Dk':>3s} {'Dv':>3s} {'N':>5s} | {'fused fwd':>26s} {'composed fwd':>26s} {'x':>6s} | {'fused f+b':>26s} "
                 f"{'composed f+b':>26s} {'x':>6s} | {'peak MB fused / composed':>24s} | {'fused TFLOP/s fwd, f+b':>22s} {'of fp32 MFMA peak':>17s}")
    for name, Dk, Dv, N in SHAPES:
        q, k, v, dout = operands(Dk, Dv, N, dev, g)
        fused_fwd = lambda: HF.self_attention(q, k, v)
        comp_fwd = lambda: composed(q, k, v)
        fused_both = lambda: torch.autograd.grad(HF.self_attention(q, k, v), (q, k, v), dout)
        comp_both = lambda: torch.autograd.grad(composed(q, k, v), (q, k, v), dout)
        err = float((fused_fwd() - comp_fwd()).abs().max())
        assert err < 1e-4, err                                    # the two contenders compute the same thing
        calls = 8 if N <= 1024 else 3
        ff, cf = alternated([fused_fwd, comp_fwd], calls)
        fb, cb = alternated([fused_both, comp_both], calls)
        pf, pc = peak_of(fused_both), peak_of(comp_both)
        med = statistics.median
        # useful arithmetic: S and P.V forward; S, dP, dV, dK, dQ backward (each product once)
        flop_f = 2.0 * B * N * N * (Dk + Dv)
        flop_b = 2.0 * B * N * N * (Dk + Dv + Dv + Dk + Dk)
        tf_f, tf_b = flop_f / (med(ff) * 1e-3), (flop_f + flop_b) / (med(fb) * 1e-3)
        apart = "windows apart" if max(fb) < min(cb) else "WINDOWS OVERLAP"
        lines.append(f"{name:<10s} {Dk:3d} {Dv:3d} {N:5d} | {fmt(ff)} {fmt(cf)} {med(cf) / med(ff):6.2f} | {fmt(fb)} {fmt(cb)} {med(cb) / med(fb):6.2f} "
                     f"| {pf / 1e6:10.1f} / {pc / 1e6:10.1f} | {tf_f / 1e12:10.2f} {tf_b / 1e12:10.2f} {100 * tf_f / PEAK_F32_MFMA:7.1f}% {100 * tf_b / PEAK_F32_MFMA:7.1f}%"
                     f"   ({apart})")
        del q, k, v, dout
    lines.append(f"ms per call: median [min, max] of {ROUNDS} alternated windows after {WARM} warm-up rounds, windows of 8 (N 1024) or 3 (N 4096) "
                 f"back-to-back calls; B = {B}, fp32, scale 1.  x = composed / fused.  composed = torch.bmm, torch.softmax, torch.bmm under autograd.  "
                 f"peak = rise of torch.cuda.max_memory_allocated over one forward + backward.  TFLOP/s = the useful arithmetic (2 B N^2 (Dk + Dv) "
                 f"forward, 2 B N^2 (3 Dk + 2 Dv) backward) over the call time, host launches included; peak = 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz.")


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
    for at in (None, 32, 64):
        torch.manual_seed(0)
        G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND, self_attn=at).to(dev)
        if at is not None:
            with torch.no_grad():
                G.gen1.self_attn.gamma.fill_(0.5)          # an open gate: every kernel of the block does real work
        Ds = [DISC.Disc64(bench.DF).to(dev), DISC.Disc128(bench.DF).to(dev), DISC.Disc256(bench.DF).to(dev)]
        enc = ENC.StandInImageEncoder(bench.EMB).to(dev)
        enc.freeze_all_weights()
        enc.eval()
        steps.append(TR.GanTrainStep(G, Ds, enc))
    run = lambda s: (lambda: s.step(words, sent, lens, None, reals))
    off, a32, a64, off2 = alternated([run(steps[0]), run(steps[1]), run(steps[2]), run(steps[0])], 5)
    med = statistics.median
    base = med(off + off2)
    lines.append("")
    lines.append(f"GanTrainStep, bench.py's default workload (Generator({bench.GF}, {bench.EMB}, {bench.Z}, {bench.COND}), Disc64/128/256({bench.DF}), "
                 f"batch {batch}, fp32, eager), ms/step median [min, max]: self_attn None {fmt(off + off2)} ({batch / base * 1e3:.1f} images/s); "
                 f"32 {fmt(a32)} (x {med(a32) / base:.4f}); 64 {fmt(a64)} (x {med(a64) / base:.4f}); the plain step against itself: "
                 f"|median of its first windows - median of its second| = {100 * abs(med(off) - med(off2)) / base:.2f}% "
                 f"(windows of 5 steps, {ROUNDS} alternated rounds after {WARM} warm-up rounds).")


def main():
    if not torch.cuda.is_available():
        sys.exit("self_attn_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    if "--calls-only" in sys.argv:                  # for a kernel trace: TRACE_CALLS forward + backward calls of both at one shape
        Dk, Dv, N = (int(v) for v in sys.argv[sys.argv.index("--calls-only") + 1:][:3])
        q, k, v, dout = operands(Dk, Dv, N, dev, torch.Generator().manual_seed(0))
        for _ in range(TRACE_CALLS):
            torch.autograd.grad(HF.self_attention(q, k, v), (q, k, v), dout)
            torch.autograd.grad(composed(q, k, v), (q, k, v), dout)
        torch.cuda.synchronize()
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "self_attn_micro.txt")
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
