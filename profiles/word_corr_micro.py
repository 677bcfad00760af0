#!/usr/bin/env python3
"""Times the word-level discriminator's score (csrc/word_corr.hip through backend.functional.word_corr) against the same formulas made
of stock torch ops on the GPU (functional.word_corr_reference: a Python loop over the B pairs, autograd for the backward) at the metric
configuration's shapes (B = 24, D = 256, S = 17 x 17 = 289, T = 18, ragged captions).  Device events around windows of back-to-back
calls, the contenders alternated in one process, medians with the range of the windows (the method of profiles/memory_micro.py).  Then
a whole eager GanTrainStep at bench.py's default workload without and with word_disc=WordLevelDisc(EMB), and, to split the difference,
the pieces the module adds timed on their own: the two extra no_grad passes of the image encoder (real and fake 256 x 256 batch) and the
score's launches of one step (discriminator loss: three forward and three backward; generator loss: one of each) with the perception
layer's 1x1 convs.

    forward:  the call on leaf operands (launch time of the host included)
    fwd+bwd:  forward, then torch.autograd.grad for the regions with a gradient at p

    python profiles/word_corr_micro.py     (writes profiles/word_corr_micro.txt; --out PATH writes elsewhere; --no-step skips the step)
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

B, D, S, T = 24, 256, 289, 18
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


def micro(lines, dev):
    g = torch.Generator().manual_seed(0)
    med = statistics.median
    lens = torch.randint(3, T + 1, (B,), generator=g)
    lens[0] = T
    host_lens, dev_lens = lens.tolist(), lens.to(dev)
    regions = (torch.randn(B, D, S, generator=g) * D ** -0.25).to(dev).requires_grad_(True)
    words = (torch.randn(B, D, T, generator=g) * D ** -0.25).to(dev)
    dp = torch.randn(B, generator=g).to(dev)
    for shift in (0, 1):
        ours_f = lambda: HF.word_corr(regions, words, dev_lens, shift)[0]
        stock_f = lambda: HF.word_corr_reference(regions, words, host_lens, shift)[0]
        ours_b = lambda: torch.autograd.grad(ours_f(), (regions,), dp)
        stock_b = lambda: torch.autograd.grad(stock_f(), (regions,), dp)
        of, sf = alternated([ours_f, stock_f], 4)
        ob, sb = alternated([ours_b, stock_b], 4)
        lines.append(f"B {B} D {D} S {S} T {T} shift {shift} | kernels fwd {fmt(of)}  stock torch fwd {fmt(sf)}  x {med(of) / med(sf):6.3f} | "
                     f"kernels f+b {fmt(ob)}  stock torch f+b {fmt(sb)}  x {med(ob) / med(sb):6.3f}   (fwd {apart(of, sf)}, f+b {apart(ob, sb)})")
    lines.append(f"ms per call: median [min, max] of {ROUNDS} alternated windows after {WARM} warm-up rounds, windows of 4 back-to-back calls; fp32, "
                 f"ragged captions of 3..{T} words, N(0, D^-1/2) entries.  x = kernels / stock (below 1: the kernels are faster).  stock = "
                 f"functional.word_corr_reference on the device (a Python loop over the {B} pairs with the lengths on the host; autograd backward).  "
                 f"The kernels: one launch per direction, one workgroup per pair ({B} of the chip's 256 compute units).")


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
        G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND).to(dev)
        Ds = [DISC.Disc64(bench.DF).to(dev), DISC.Disc128(bench.DF).to(dev), DISC.Disc256(bench.DF).to(dev)]
        enc = ENC.StandInImageEncoder(bench.EMB).to(dev)
        enc.freeze_all_weights()
        enc.eval()
        steps.append(TR.GanTrainStep(G, Ds, enc, word_disc=DISC.WordLevelDisc(bench.EMB).to(dev) if on else None))
    run = lambda s: (lambda: s.step(words, sent, lens, None, reals))
    off, on, off2 = alternated([run(steps[0]), run(steps[1]), run(steps[0])], 5)
    med = statistics.median
    base = med(off + off2)
    lines.append("")
    lines.append(f"GanTrainStep, bench.py's default workload (Generator({bench.GF}, {bench.EMB}, {bench.Z}, {bench.COND}), Disc64/128/256({bench.DF}), "
                 f"batch {batch}, fp32, eager, StandInImageEncoder), ms/step median [min, max]: plain {fmt(off + off2)} ({batch / base * 1e3:.1f} images/s); "
                 f"word_disc {fmt(on)} ({batch / med(on) * 1e3:.1f} images/s, x {med(on) / base:.4f}, + {med(on) - base:.3f} ms); the plain step against "
                 f"itself: |median of its first windows - median of its second| = {100 * abs(med(off) - med(off2)) / base:.2f}% "
                 f"(windows of 5 steps, {ROUNDS} alternated rounds after {WARM} warm-up rounds).")
    # the pieces the module adds, timed on their own at the step's shapes
    step = steps[1]
    enc, wd = step.image_encoder, step.word_disc
    fake = torch.rand_like(reals[-1]) * 2 - 1
    wemb = words.detach()

    def encoder_passes():
        with torch.no_grad():
            enc(reals[-1])
            enc(fake)
    with torch.no_grad():
        real_regions, fake_regions = enc(reals[-1])[0], enc(fake)[0]
    fake_leaf = fake_regions.clone().requires_grad_(True)

    def word_level_work():
        step.w_opt.zero_grad()
        step.word_disc_loss.get_loss(wd, fake_regions, real_regions, wemb, lens).backward()
        wd.requires_grad_(False)
        gl = step.word_gen_loss.get_loss(wd, fake_leaf, wemb, lens)
        torch.autograd.grad(gl, (fake_leaf,))
        wd.requires_grad_(True)
    ep, ww = alternated([encoder_passes, word_level_work], 5)
    lines.append(f"of that difference, timed alone (ms per step's worth, same windows): the two extra no_grad encoder passes {fmt(ep)}; the word-level "
                 f"losses of one step -- perception convs, four score forwards and four backwards, the log terms, autograd -- {fmt(ww)}.  The stand-in "
                 f"encoder is three small matrix products; an Inception-v3 encoder's passes cost what profiles/r05_encoder_timing.txt says, twice.")


def main():
    if not torch.cuda.is_available():
        sys.exit("word_corr_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "word_corr_micro.txt")
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
