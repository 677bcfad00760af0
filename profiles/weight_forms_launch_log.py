#!/usr/bin/env python3
"""Every agan_pack_weight / agan_pack_weights call (name, jobs, layout family) that a fixed sequence makes at the tiny configuration
(gf = df = 8, B = 4, T = 10), in f32 and in bf16: 3 eager steps, capture, 2 replays, a live and an averaged sample, 1 more replay, both
samples again.  Launches recorded into a graph are logged where they are captured; a replay makes no host call.  The output of two
checkouts can be compared with diff.

    python profiles/weight_forms_launch_log.py > profiles/weight_forms_launch_log.txt
"""
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")
L = HF.L

DEV = torch.device("cuda", 0)
GF, DF, EMB, Z, COND, B, T = 8, 8, 32, 16, 16, 4, 10
LOG = []


def logged_call(name, *args, _call=L.call):
    if name == "agan_pack_weight":             # (w, wk, mode, cout, cin, kh, kw, prec, stream)
        LOG.append(f"{name} jobs=1 family={args[7]}")
    elif name == "agan_pack_weights":          # (table, jobs, blocks, prec, stream)
        LOG.append(f"{name} jobs={args[1]} family={args[3]}")
    _call(name, *args)


def phase(title, fn):
    del LOG[:]
    out = fn()
    torch.cuda.synchronize()
    print(f"  {title}: {len(LOG)} pack launches")
    runs = []                                   # equal neighbours as one line
    for line in LOG:
        if runs and runs[-1][0] == line:
            runs[-1][1] += 1
        else:
            runs.append([line, 1])
    for line, n in runs:
        print(f"    {n} x {line}")
    return out


def run(mode):
    print(f"precision {mode}")
    HF.set_precision(L.PRECISIONS[mode])
    torch.manual_seed(3)
    G = GEN.Generator(GF, EMB, Z, COND).to(DEV)
    Ds = [DISC.Disc64(DF).to(DEV), DISC.Disc128(DF).to(DEV), DISC.Disc256(DF).to(DEV)]
    enc = ENC.StandInImageEncoder(EMB).to(DEV)
    enc.freeze_all_weights()
    g = torch.Generator().manual_seed(3)
    words, sent = torch.randn(B, EMB, T, generator=g).to(DEV), torch.randn(B, EMB, generator=g).to(DEV)
    lens = torch.tensor([10, 3, 2, 7], dtype=torch.int64, device=DEV)
    reals = [(torch.rand(B, 3, r, r, generator=g) * 2 - 1).to(DEV) for r in (64, 128, 256)]
    noise, eps = torch.randn(B, Z, generator=g).to(DEV), torch.randn(B, COND, generator=g).to(DEV)
    step = TR.GanTrainStep(G, Ds, enc, seed=3, ema=0.9)

    def samples(tag):
        for name, use_ema in (("live", False), ("averaged", True)):
            phase(f"{name} sample {tag}", lambda: step.generate_images(words, sent, lens, noise=noise, eps=eps, use_ema=use_ema))

    for k in range(3):
        phase(f"eager step {k + 1}", lambda: step.step(words, sent, lens, None, reals))
    graphed = phase("capture (1 warm-up step, then the captured one)", lambda: step.capture(words, sent, lens, reals, warmup=1))
    for k in range(2):
        phase(f"replay {k + 1}", graphed.replay)
    samples("after replay 2")
    phase("replay 3", graphed.replay)
    samples("after replay 3")
    del graphed, step
    HF.set_precision(L.PREC_F32)


if __name__ == "__main__":
    L.call = logged_call
    for mode in ("f32", "bf16"):
        run(mode)
