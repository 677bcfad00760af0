#!/usr/bin/env python3
"""What the averaged generator (GanTrainStep(ema=...), optim.FlatEMA, csrc/ema.hip) costs at the metric configuration (256 x 256,
batch 24, fp32), measured with device events:

  1. the update alone, over the metric generator's flat buffer and BatchNorm statistics --
       warm   windows of back-to-back calls of the C entry (source and destination, 2 x 28 MB, stay in the 256 MiB Infinity Cache),
       cold   single FlatEMA.update() calls, each behind a 1 GiB fill that evicts them -- the state the train step leaves them in,
       host   the wall clock FlatEMA.update() takes to return;
     TB/s of bytes OWED: source read, destination read and written = 12 bytes per float.
  2. the captured train step (GanTrainStep.capture) without and with ema=0.999: two trainers in ONE process, windows of replays
     alternated, median and range of the windows.

On a tree whose GanTrainStep has no `ema` argument (the parent commit) part 1 is skipped and part 2 times two trainers WITHOUT the
average against each other: the same protocol's own spread.  Not a pass bar.  Not run by bench.py.

    python profiles/ema_micro.py > profiles/ema_micro.txt
"""
import importlib
import inspect
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                                                              # noqa: E402  (the metric configuration's constants)

HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

BATCH, DECAY = 24, 0.999
WARM_CALLS, ROUNDS, WARM_ROUNDS, COLD_CALLS = 200, 9, 2, 30
STEP_WINDOW, STEP_ROUNDS, STEP_WARM = 20, 9, 2
HBM_TBS = 6.3                                                                             # achievable HBM3E rate of an MI355X (8 TB/s peak)


def build(dev, ema):
    """bench.build's `full3` trainer, with the average when asked for"""
    torch.manual_seed(0)
    G = GEN.Generator(bench.GF, bench.EMB, bench.Z, bench.COND).to(dev)
    Ds = [DISC.Disc64(bench.DF).to(dev), DISC.Disc128(bench.DF).to(dev), DISC.Disc256(bench.DF).to(dev)]
    enc = ENC.StandInImageEncoder(bench.EMB).to(dev)
    enc.freeze_all_weights()
    enc.eval()
    return TR.GanTrainStep(G, Ds, enc, **({} if ema is None else {"ema": ema}))


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def update_alone(step, dev):
    ema = step.g_ema
    table, nseg, total = ema._segments()
    floats = ema.numel + sum(b.numel() for b in step.G.buffers() if b.is_floating_point())
    owed = 12.0 * floats
    warm = []
    for r in range(WARM_ROUNDS + ROUNDS):
        def window():
            for _ in range(WARM_CALLS):                                                   # the C entry: the tick and the update, no Python around them
                HF.L.call("agan_ema_update", HF._p(table), nseg, total, HF._p(ema.state), ema.decay, int(ema.warmup), HF._stream())
        ms = event_ms(window) / WARM_CALLS
        if r >= WARM_ROUNDS:
            warm.append(ms)
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)                         # 1 GiB
    cold = []
    for r in range(3 + COLD_CALLS):
        flush.fill_(float(r))
        ms = event_ms(ema.update)
        if r >= 3:
            cold.append(ms)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(WARM_CALLS):
        ema.update()
    host = (time.perf_counter() - t0) / WARM_CALLS
    torch.cuda.synchronize()
    w, c = statistics.median(warm), statistics.median(cold)
    print(f"update alone: {nseg} segments ({ema.numel} floats of parameters in one, {nseg - 1} BatchNorm statistics), {total} workgroups of 256, "
          f"{owed / 1e6:.1f} MB owed (12 bytes per float), tick launch included")
    print(f"  warm (Infinity-Cache resident): {w * 1e3:8.2f} us per call  [{min(warm) * 1e3:.2f} .. {max(warm) * 1e3:.2f}]   {owed / w / 1e9:7.2f} TB/s owed; "
          f"median of {ROUNDS} windows of {WARM_CALLS} back-to-back calls")
    print(f"  cold (behind a 1 GiB fill):     {c * 1e3:8.2f} us per call  [{min(cold) * 1e3:.2f} .. {max(cold) * 1e3:.2f}]   {owed / c / 1e9:7.2f} TB/s owed "
          f"= {100 * owed / c / 1e9 / HBM_TBS:.0f} % of the {HBM_TBS} TB/s an MI355X's HBM sustains; median of {COLD_CALLS} single calls, one event pair each "
          f"(the pair's own few us included)")
    print(f"  host: FlatEMA.update() returns after {host * 1e6:.1f} us (address check of {nseg - 1} buffer pairs, two launches; mean of {WARM_CALLS} calls)")


def captured_steps(dev, emas):
    words, sent, lens, reals = bench.synthetic_batch(dev, BATCH, seed=1)
    lens_dev = torch.tensor(lens, dtype=torch.int64, device=dev)
    graphs = []
    for ema in emas:
        step = build(dev, ema)
        graphs.append((step, step.capture(words, sent, lens_dev, reals, warmup=2)))
    ms = [[] for _ in graphs]
    for r in range(STEP_WARM + STEP_ROUNDS):
        for i, (_, graphed) in enumerate(graphs):
            def window():
                for _ in range(STEP_WINDOW):
                    graphed.replay()
            t = event_ms(window) / STEP_WINDOW
            if r >= STEP_WARM:
                ms[i].append(t)
    print(f"captured train step, f32, batch {BATCH}, 256 x 256; ms per step, median [range] of {STEP_ROUNDS} alternated windows of {STEP_WINDOW} replays "
          f"after {STEP_WARM} warm-up rounds:")
    for ema, m in zip(emas, ms):
        print(f"  ema = {str(ema):>5s}: {statistics.median(m):8.3f}  [{min(m):.3f} .. {max(m):.3f}]   {BATCH / statistics.median(m) * 1e3:7.1f} images/s")
    a, b = statistics.median(ms[0]), statistics.median(ms[1])
    print(f"  second - first: {(b - a) * 1e3:+.1f} us per step ({100 * (b / a - 1):+.3f} %)")
    return graphs


def main():
    if not torch.cuda.is_available():
        sys.exit("ema_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = torch.device("cuda", 0)
    has_ema = "ema" in inspect.signature(TR.GanTrainStep.__init__).parameters
    print(f"library: {os.path.relpath(HF.L.LIB_PATH, ROOT)}; GanTrainStep {'has' if has_ema else 'has NO'} `ema` argument")
    graphs = captured_steps(dev, [None, DECAY] if has_ema else [None, None])
    if has_ema:
        print()
        update_alone(graphs[1][0], dev)


if __name__ == "__main__":
    main()
