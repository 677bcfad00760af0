"""What feeding real data costs: ShardBatches (host convert + fp32 copy) vs DeviceShardBatches (resident uint8 + one kernel), B=24.

    python profiles/batch_feed_timing.py [--batch 24] [--reps 20] [--out profiles/r09_batch_feed_timing.txt]

One process, one MI355X, a synthetic three-resolution shard of 22 batches written to a temporary directory.  Reports
  * each loader alone, the two alternated batch by batch, median of --reps after warm-up: host wall time spent inside next(), and
    wall time until the batch is complete on the device (next() + a device synchronisation);
  * agan_image_prep alone, device events around a captured graph of 20 back-to-back launches, per launch, median of --reps replays: three direct planes (the three-resolution shard), with every sample
    mirrored, and img256 + two derived planes (a 256-only shard); achieved GB/s = (bytes read + bytes written) / time;
  * GanTrainStep.train_epoch at the metric configuration (bench.py's full3 build) in f32 and in bf16 with bf16 storage, fed by a fixed
    resident batch, by ShardBatches and by DeviceShardBatches: runs of --reps steps, the three feeds alternated run by run, median
    images/s of the runs after one warm-up run each.
Numbers only; nothing here is a pass bar.
"""
import argparse
import importlib
import itertools
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_batch_feed_timing.txt"))
    args = ap.parse_args()
    B, reps, dev = args.batch, args.reps, torch.device("cuda:0")
    bench = importlib.import_module("bench")
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    LIB = importlib.import_module("attention-gan_amd.backend.lib")
    BT = importlib.import_module("attention-gan_amd.data.batches")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    med = statistics.median
    n_batches = reps + 2
    n = B * n_batches
    rng = np.random.default_rng(0)
    tmp = tempfile.TemporaryDirectory()
    path = os.path.join(tmp.name, "shard.npz")
    images = [rng.integers(0, 256, (n, 3, r, r), dtype=np.uint8) for r in (64, 128, 256)]
    BT.write_shard(path, rng.integers(1, 1000, (n, bench.T)), np.full(n, bench.T), rng.integers(0, 50, n), *images)
    say(f"batch_feed_timing: B={B}, shard of {n} samples ({sum(a.nbytes for a in images) / 1e6:.0f} MB uint8, {n_batches} batches), {torch.cuda.get_device_name(0)}")

    # ---- 1. each loader alone -----------------------------------------------------------------------------------------------------
    host = {"ShardBatches": [], "DeviceShardBatches": []}
    done = {"ShardBatches": [], "DeviceShardBatches": []}
    first = {}
    its = {"ShardBatches": iter(BT.ShardBatches([path], B, device=dev, shuffle=True, seed=0)),
           "DeviceShardBatches": iter(BT.DeviceShardBatches([path], B, dev, shuffle=True, seed=0))}
    for k in range(n_batches):
        for name, it in its.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch = next(it)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if k == 0:
                first[name] = (t2 - t0) * 1e3          # reads the shard (and pins and uploads it)
            if k >= 2:                                  # (the second next() warms the allocators)
                host[name].append((t1 - t0) * 1e3)
                done[name].append((t2 - t0) * 1e3)
            del batch
    say()
    say(f"1. loader alone (median of {len(host['ShardBatches'])}, loaders alternated per batch, device idle before each next())")
    say("   loader               host ms in next()   ms until the batch is complete on the device   first next() of the shard, ms")
    for name in host:
        say(f"   {name:<20} {med(host[name]):>12.3f} {med(done[name]):>24.3f} {first[name]:>40.1f}")
    del its

    # ---- 2. the kernel --------------------------------------------------------------------------------------------------------------
    res = [torch.from_numpy(a).to(dev) for a in images]
    rows = torch.from_numpy(np.sort(rng.permutation(n)[:B]).astype(np.int32)).to(dev)
    ones = torch.ones(B, dtype=torch.uint8, device=dev)
    outs = [torch.empty(B, 3, r, r, device=dev) for r in (256, 128, 64)]
    px = B * 3 * (64 * 64 + 128 * 128 + 256 * 256)
    cases = (("three direct planes", [res[2], res[1], res[0]], None, px + 4 * px),
             ("three direct planes, mirrored", [res[2], res[1], res[0]], ones, px + 4 * px),
             ("img256 + two derived planes", [res[2], (128, 128), (64, 64)], None, B * 3 * 256 * 256 + 4 * px),
             ("img256 + two derived planes, mirrored", [res[2], (128, 128), (64, 64)], ones, B * 3 * 256 * 256 + 4 * px))
    say()
    say(f"2. agan_image_prep alone (device events around a graph of 20 back-to-back launches, per launch, median of {reps} replays; bytes = uint8 read once + fp32 written)")
    say("   case                                      us      MB moved     GB/s")
    CALLS = 20                                          # launches per graph: the host cannot enqueue one as fast as the device runs it
    for name, planes, flip, nbytes in cases:
        HF.image_prep(planes, rows, flip, out=outs)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(CALLS):
                HF.image_prep(planes, rows, flip, out=outs)
        ms = []
        for k in range(reps + 3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            graph.replay()
            e.record()
            torch.cuda.synchronize()
            if k >= 3:
                ms.append(s.elapsed_time(e) / CALLS)
        t = med(ms)
        say(f"   {name:<38} {t * 1e3:>8.1f} {nbytes / 1e6:>10.1f} {nbytes / t / 1e6:>10.0f}")
    del res, outs

    # ---- 3. train_epoch under each feed -------------------------------------------------------------------------------------------
    table = torch.randn(1000, bench.EMB, device=dev, generator=torch.Generator(device=dev).manual_seed(0))

    def text_encoder(words, lengths):
        e = table[words]
        return e.transpose(1, 2), e.mean(1)

    say()
    say(f"3. GanTrainStep.train_epoch, full3 build, runs of {reps} steps, feeds alternated run by run, median images/s of {RUNS} runs after a warm-up run each")
    say("   mode                 fixed resident batch     ShardBatches     DeviceShardBatches")
    for mode, prec, storage in (("f32", "f32", None), ("bf16 --storage bf16", "bf16", "bf16")):
        HF.set_activation_storage(storage)
        HF.set_precision(LIB.PRECISIONS[prec])
        step = bench.build(dev, B, HF)
        fixed = next(iter(BT.ShardBatches([path], B, device=dev, shuffle=True, seed=0)))
        feeds = {"fixed": lambda: [fixed] * reps,
                 "host": lambda: BT.ShardBatches([path], B, device=dev, shuffle=True, seed=0),
                 "device": lambda: BT.DeviceShardBatches([path], B, dev, shuffle=True, seed=0)}
        rate = {k: [] for k in feeds}
        for run in range(RUNS + 1):
            for name, make in feeds.items():
                it = iter(make())
                head = next(it)                         # opening the shard (read, pin, upload) stays outside the timed region
                batches = itertools.chain([head], it)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = step.train_epoch(batches, text_encoder, B, max_batches=reps)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert steps == reps
                if run >= 1:
                    rate[name].append(B * steps / dt)
                for h in (step.d_losses, step.g_losses, step.damsm_losses):
                    h.clear()
        say(f"   {mode:<20} {med(rate['fixed']):>14.1f} {med(rate['host']):>20.1f} {med(rate['device']):>20.1f}")
        say(f"   {'  (min .. max)':<20} {min(rate['fixed']):>8.1f} .. {max(rate['fixed']):<8.1f} {min(rate['host']):>8.1f} .. {max(rate['host']):<8.1f} "
            f"{min(rate['device']):>8.1f} .. {max(rate['device']):<8.1f}")
        del step
    HF.set_activation_storage(None)
    HF.set_precision(LIB.PREC_F32)
    say("   (the first next() of a run, which opens the shard, is outside the timed region: section 1 has its cost; train_epoch reads `lengths`")
    say("    on the host for its batch guard under every feed, which waits for the previous step)")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    tmp.cleanup()


if __name__ == "__main__":
    main()
