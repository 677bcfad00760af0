#!/usr/bin/env python3
"""Times the channel-wise word attention (csrc/chan_attn.hip through backend.functional.channel_attention) against the same
formulas made of stock torch ops on the GPU (functional.channel_attention_reference: torch.bmm, softmax, torch.bmm on the same wt, and
autograd for the backward) at the two places of the metric configuration (gf_dim and emb_dim of bench.py, B = 24, T = 18): the
64x64 map of gen2 and the 128x128 map of gen3.  Device events around windows of back-to-back calls, the contenders alternated in one
process, medians with the range of the windows (the method of profiles/memory_micro.py).  The perception layer (functional.linear,
B T = 432 rows -> N outputs, and its weight gradient) is existing code and is timed on its own.  Then a whole eager GanTrainStep at
bench.py's default workload with the plain generator and with Generator(channel_attn=True).

    forward:  the call on leaf operands (launch time of the host included)
    fwd+bwd:  forward, then torch.autograd.grad for h and wt, with a gradient at f only

    python profiles/channel_attn_micro.py     (writes profiles/channel_attn_micro.txt; --out PATH writes elsewhere; --no-step skips the step)
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
    return f"{statistics.median(ms):8.3f} [{min(ms):7.3f},{max(ms):8.3f}]"


def apart(a, b):
    return "windows apart" if max(a) < min(b) or max(b) < min(a) else "windows overlap"


def micro(lines, dev, C, E):
    g = torch.Generator().manual_seed(0)
    med = statistics.median
    lines.append(f"{'map':<8s} {'C':>3s} {'T':>3s} | {'kernels fwd':>26s} {'stock torch fwd':>26s} {'x':>6s} | {'kernels f+b':>26s} "
                 f"{'stock torch f+b':>26s} {'x':>6s} | {'fwd TB/s kernels / stock':>25s} | {'f+b TB/s kernels / stock':>25s}")
    linear = []
    for hw in MAPS:
        n = hw * hw
        lens = torch.randint(3, T + 1, (B,), generator=g)
        lens[0] = T
        mask = (torch.arange(T).view(1, T) < lens.view(B, 1)).to(torch.int64).to(dev)
        h = torch.randn(B, C, hw, hw, generator=g).to(dev).requires_grad_(True)
        words = torch.randn(B, E, T, generator=g).to(dev)
        weight = ((torch.rand(n, E, generator=g) * 2 - 1) / E ** 0.5).to(dev).requires_grad_(True)       # nn.Linear's default init
        rows = words.transpose(1, 2).reshape(B * T, E).contiguous().requires_grad_(True)
        wt = HF.linear(rows, weight).detach().view(B, T, n).requires_grad_(True)
        df = torch.randn(B, C, hw, hw, generator=g).to(dev)
        dwt = torch.randn(B * T, n, generator=g).to(dev)
        ours_f = lambda: HF.channel_attention(h, wt, mask, None)[0]
        stock_f = lambda: HF.channel_attention_reference(h, wt, mask, None)[0]
        ours_b = lambda: torch.autograd.grad(ours_f(), (h, wt), df)
        stock_b = lambda: torch.autograd.grad(stock_f(), (h, wt), df)
        calls = 8 if hw <= 64 else 3
        of, sf = alternated([ours_f, stock_f], calls)
        ob, sb = alternated([ours_b, stock_b], calls)
        # algorithmic bytes per pixel and sample: the score reads h and wt, the read pass reads wt and writes f; the backward reads df
        # and wt for dalpha, then h, df, wt and writes dh and dwt
        by_f = 4.0 * B * n * (2 * C + 2 * T)
        by_b = by_f + 4.0 * B * n * (4 * C + 3 * T)
        tb = lambda by, ms: by / (med(ms) * 1e-3) / 1e12
        lines.append(f"{hw}x{hw:<5d} {C:3d} {T:3d} | {fmt(of)} {fmt(sf)} {med(of) / med(sf):6.2f} | {fmt(ob)} {fmt(sb)} {med(ob) / med(sb):6.2f} "
                     f"| {tb(by_f, of):11.2f} / {tb(by_f, sf):11.2f} | {tb(by_b, ob):11.2f} / {tb(by_b, sb):11.2f}   (fwd {apart(of, sf)}, f+b {apart(ob, sb)})")
        lin_f = lambda: HF.linear(rows, weight)
        lin_b = lambda: torch.autograd.grad(lin_f(), (rows, weight), dwt)
        lf, lb = alternated([lin_f, lin_b], calls)
        linear.append(f"{hw}x{hw}: forward {fmt(lf)}, forward + backward (d rows, d weight) {fmt(lb)}")
    lines.append(f"ms per call: median [min, max] of {ROUNDS} alternated windows after {WARM} warm-up rounds, windows of 8 (64x64) or 3 (128x128) "
                 f"back-to-back calls; B = {B}, fp32, ragged captions of 3..{T} words, scale 1/sqrt(N).  x = kernels / stock (below 1: the kernels are "
                 f"faster).  stock = functional.channel_attention_reference on the device (bmm, masked_fill, softmax, bmm; autograd backward).  TB/s = "
                 f"algorithmic bytes of the KERNELS' plan over the call time, host launches included: forward 4 (2C + 2T) per pixel, backward 4 (4C + 3T); "
                 f"the stock column divides the same bytes by its own time.")
    lines.append(f"perception layer, functional.linear of {B * T} rows x {E} -> N outputs (existing code), ms per call: " + "; ".join(linear))


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
    for on in (False, True):
        torch.manual_seed(0)
        G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND, channel_attn=on).to(dev)
        Ds = [DISC.Disc64(bench.DF).to(dev), DISC.Disc128(bench.DF).to(dev), DISC.Disc256(bench.DF).to(dev)]
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
                 f"batch {batch}, fp32, eager), ms/step median [min, max]: plain {fmt(off + off2)} ({batch / base * 1e3:.1f} images/s); "
                 f"channel_attn=True {fmt(on)} ({batch / med(on) * 1e3:.1f} images/s, x {med(on) / base:.4f}); the plain step against itself: "
                 f"|median of its first windows - median of its second| = {100 * abs(med(off) - med(off2)) / base:.2f}% "
                 f"(windows of 5 steps, {ROUNDS} alternated rounds after {WARM} warm-up rounds).")


def main():
    if not torch.cuda.is_available():
        sys.exit("channel_attn_micro: needs an MI355X (timings on a CPU say nothing about it)")
    import bench
    dev = "cuda"
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "channel_attn_micro.txt")
    lines = [f"library: {os.path.relpath(L.LIB_PATH, os.path.dirname(HERE))}"]
    micro(lines, dev, bench.GF, bench.EMB)
    if "--no-step" not in sys.argv:
        whole_step(lines, dev)
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
