#!/usr/bin/env python3
"""Times the discriminator-side tail of the text-conditional head (networks/discriminators.py: COND_DNET.jointConv) in two forms, at the
metric configuration (df = 64, nef = 256, batch 24: code [2B, 512, 4, 4], sentences [B, 256]), forward + backward, fp32:

    shared      what the library runs: conv3x3 over the 512 image channels ONCE for [real; fake] (9.4 MB of weights), linear over the
                B captions (4.7 MB), cond_join with the wrong rows, fused BatchNorm + LeakyReLU under bn_groups(3)
    composed    what the library's existing ops would give: per pass torch.cat(h, rep(s)) + HF.conv2d over 8df + nef = 768 channels
                (14 MB of weights) + bn_act, three passes (real, fake, wrong)

Each form is captured into a HIP graph (so that the window holds kernels and no host work) and timed with device events around windows
of back-to-back replays, windows alternated, medians and the spread over the windows; the eager calls are timed the same way.  Then the
images/s of the whole train step with conditional=True and False, eager and captured, runs alternated.  None of these is a pass bar.
Not run by bench.py.

    python profiles/cond_tail_micro.py > profiles/cond_tail_micro.txt
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
L = importlib.import_module("attention-gan_amd.backend.lib")
LAY = importlib.import_module("attention-gan_amd.utilities.layers")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

DF, NEF, B = 64, 256, 24
ROUNDS, WARM, CALLS = 9, 2, 50
STEP_ROUNDS, STEP_WARM, STEPS = 5, 2, 10


def alternated(fns, calls):
    """ms per call of every callable over ROUNDS windows each, the callables run in turn; a window is `calls` back-to-back calls
    between one pair of events"""
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


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    HF.build_pack_tables()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def show(name, ms):
    print(f"  {name:<28s} median {statistics.median(ms):7.4f} ms   min {min(ms):7.4f}   max {max(ms):7.4f}   (spread {100 * (max(ms) - min(ms)) / statistics.median(ms):4.1f}%)")


def tail(dev):
    C = 8 * DF
    torch.manual_seed(0)
    jc = DISC._JointConv(C, NEF).to(dev)
    blk = LAY.Layers.Block3x3_leakRelu(C + NEF, C).to(dev)
    with torch.no_grad():                                   # the same function in both forms
        getattr(blk, "0").weight.copy_(jc.joint_weight())
    g = torch.Generator().manual_seed(0)
    h = torch.randn(2 * B, C, 4, 4, generator=g).to(dev).requires_grad_(True)
    sent = torch.randn(B, NEF, generator=g).to(dev)
    dz = torch.randn(3 * B, C, 4, 4, generator=g).to(dev)
    rep = lambda s: s[:, :, None, None].expand(-1, -1, 4, 4)

    def zero():
        h.grad = None
        for m in (jc, blk):
            for prm in m.parameters():
                prm.grad = None

    def shared_fwd():
        y = HF.cond_join(jc.image(h), jc.sentence(sent).view(B, C, 9), True)
        with HF.bn_groups(3):
            return getattr(jc, "1").fused(y, L.ACT_LRELU)

    def composed_fwd():
        wrong = sent.roll(-1, 0)
        return [blk(torch.cat([x, rep(s)], dim=1)) for x, s in ((h[:B], sent), (h[B:], sent), (h[:B], wrong))]

    def shared():
        zero()
        shared_fwd().backward(dz)

    def composed():
        zero()
        torch.autograd.backward(composed_fwd(), [dz[:B], dz[B:2 * B], dz[2 * B:]])

    # one function: outputs and the code's gradient agree
    shared()
    gs, zs = h.grad.clone(), shared_fwd().detach()
    composed()
    gc, zc = h.grad.clone(), torch.cat([z.detach() for z in composed_fwd()])
    nrel = lambda a, b: float((a - b).norm() / b.norm())
    print(f"shared vs composed on the same weights: output {nrel(zs, zc):.2e}, gradient of the code {nrel(gs, gc):.2e} (norm-relative)")
    print(f"conditional tail, forward + backward, df {DF}, nef {NEF}, B {B}: code [{2 * B}, {C}, 4, 4] -> [{3 * B}, {C}, 4, 4]")
    ge, ce = alternated([shared, composed], CALLS)
    show("shared, eager", ge)
    show("composed, eager", ce)
    gg, cg = alternated([graphed(shared), graphed(composed)], CALLS)
    show("shared, HIP graph", gg)
    show("composed, HIP graph", cg)
    a, b = statistics.median(gg), statistics.median(cg)
    print(f"  HIP graph: shared / composed = {a / b:.3f}; the windows' ranges {'do not overlap' if max(gg) < min(cg) or max(cg) < min(gg) else 'OVERLAP'}")
    fw = alternated([graphed(lambda: shared_fwd()), graphed(lambda: composed_fwd())], CALLS)
    show("shared, forward, HIP graph", fw[0])
    show("composed, forward, HIP graph", fw[1])
    print(f"(per call, from windows of {CALLS} back-to-back calls between device events; {ROUNDS} alternated windows after {WARM} warm-up rounds.  "
          f"HIP graph: the form captured once and replayed, so the window holds its kernels and torch's copies and no host work; eager: "
          f"host launch time included.  Weight gradients go to scratch tensors in both forms.)")


def build(dev, conditional):
    bench = importlib.import_module("bench")
    torch.manual_seed(0)
    G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND).to(dev)
    cd = bench.EMB if conditional else None
    Ds = [DISC.Disc64(bench.DF, cond_dim=cd).to(dev), DISC.Disc128(bench.DF, cond_dim=cd).to(dev), DISC.Disc256(bench.DF, cond_dim=cd).to(dev)]
    enc = ENC.StandInImageEncoder(bench.EMB).to(dev)
    enc.freeze_all_weights()
    enc.eval()
    return TR.GanTrainStep(G, Ds, enc, conditional=conditional)


def steps(dev):
    bench = importlib.import_module("bench")
    words, sent, lens, reals = bench.synthetic_batch(dev, B, seed=1)
    lens = torch.tensor(lens, dtype=torch.int64, device=dev)
    runs, names = [], []
    for conditional in (False, True):
        eager = build(dev, conditional)
        runs.append(lambda st=eager: st.step(words, sent, lens, None, reals))
        names.append(f"conditional={conditional}, eager")
        cap = build(dev, conditional).capture(words, sent, lens, reals)
        runs.append(cap.replay)
        names.append(f"conditional={conditional}, captured")
    rates = [[] for _ in runs]
    for rnd in range(STEP_WARM + STEP_ROUNDS):
        for i, fn in enumerate(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(STEPS):
                fn()
            torch.cuda.synchronize()
            if rnd >= STEP_WARM:
                rates[i].append(B * STEPS / (time.perf_counter() - t0))
    print()
    print(f"train step, f32, 256x256, batch {B}, df {DF}, nef {bench.EMB}: images/s")
    for name, v in zip(names, rates):
        print(f"  {name:<32s} median {statistics.median(v):7.1f}   min {min(v):7.1f}   max {max(v):7.1f}")
    med = [statistics.median(v) for v in rates]
    print(f"  conditional / unconditional: eager {med[2] / med[0]:.3f}, captured {med[3] / med[1]:.3f}")
    print(f"(median of {STEP_ROUNDS} alternated runs of {STEPS} steps after {STEP_WARM} warm-up runs, wall clock around the run with a device "
          f"synchronisation.  The conditional step does strictly more work: per discriminator one more 3x3 conv over [2B] and [B] codes, "
          f"one linear, the join, one BatchNorm over 3B + B codes and one more logit head.)")


def main():
    if not torch.cuda.is_available():
        sys.exit("cond_tail_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = torch.device("cuda", 0)
    print(f"library: {os.path.relpath(L.LIB_PATH, ROOT)}")
    tail(dev)
    steps(dev)


if __name__ == "__main__":
    main()
