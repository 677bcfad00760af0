#!/usr/bin/env python3
"""Times the Inception Score's reduction (csrc/iscore.hip through backend.functional.inception_split_scores) against the float64 torch
statement of the protocol (evaluation.inception_score_reference) on the same device, with device events around windows of back-to-back
calls, alternated windows, medians -- the method of profiles/eval_micro.py:

    library: agan_inception_score (row pass, column pass, class pass, finish; fp32 logits read twice, nothing of size N x C stored)
    torch:   per split: logits.double(), max, exp, sum, log, exp, where, products, means -- float64 passes over an n_s x C matrix

and reports ms per call, the ratio, the bandwidth of the logits read (2 N C 4 bytes over the call's time: a whole-call rate, launch gaps and
the workspace allocation included, not a kernel's share of peak) and the largest relative difference of the two sides' scores.  The
windows call on one tensor again and again: logits and workspace of every shape here fit the 256 MiB Infinity Cache, so those are
cache-resident figures.  The `cold` column is the library's call alone behind a 1 GiB fill that evicts them (the state an evaluation
leaves freshly collected logits in once they pass the cache's size): median of single calls, one event pair each.  Not run by bench.py.

    python profiles/iscore_micro.py            (writes profiles/iscore_micro.txt; --out PATH writes elsewhere)

The kernels of one call, in a run of its own (tracing slows the host; DESIGN.md section 21 quotes the medians of the four kernels):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python profiles/iscore_micro.py --calls-only 30000 1000 10
"""
import importlib
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
HF = importlib.import_module("attention-gan_amd.backend.functional")
EV = importlib.import_module("attention-gan_amd.evaluation")

SHAPES = [(256, 1000, 1), (5000, 200, 10), (30_000, 1000, 10), (50_000, 1000, 10)]          # N, C, splits
ROUNDS, WARM, COLD_CALLS, TRACE_CALLS = 9, 2, 15, 12


def alternated(fns, calls):
    """median ms per call of every callable, the callables run in turn ROUNDS times; a timed window is `calls` back-to-back calls between
    one pair of events, so that the host's enqueue of a call overlaps the device's work on the one before"""
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
    return [statistics.median(m) for m in ms]


def main():
    if not torch.cuda.is_available():
        sys.exit("iscore_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    if "--calls-only" in sys.argv:                  # for a kernel trace: TRACE_CALLS calls of the library at one shape, nothing else
        N, C, S = (int(v) for v in sys.argv[sys.argv.index("--calls-only") + 1:][:3])
        logits = (3.0 * torch.randn(N, C, generator=g)).to(dev)
        for _ in range(TRACE_CALLS):
            HF.inception_split_scores(logits, S)
        torch.cuda.synchronize()
        return
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "iscore_micro.txt")
    flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)                         # 1 GiB
    lines = [f"library: {os.path.relpath(HF.L.LIB_PATH, os.path.dirname(HERE))}",
             f"{'N':>6s} {'C':>5s} {'S':>3s} | {'library ms':>10s} {'torch ms':>9s} {'ratio':>6s} | {'logits read GB/s':>16s} | {'cold ms':>8s} {'GB/s':>7s} | max rel. difference of IS"]
    for N, C, S in SHAPES:
        logits = (3.0 * torch.randn(N, C, generator=g)).to(dev)
        got, ref = HF.inception_split_scores(logits, S), EV.inception_score_reference(logits, S)
        diff = float(((got[:, 0] - ref[:, 0]).abs() / ref[:, 0]).max())
        calls = 50 if N * C <= 1 << 20 else 10
        t, tt = alternated([lambda: HF.inception_split_scores(logits, S), lambda: EV.inception_score_reference(logits, S)], calls)
        cold = []
        for r in range(3 + COLD_CALLS):
            flush.fill_(float(r))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            HF.inception_split_scores(logits, S)
            e1.record()
            e1.synchronize()
            if r >= 3:
                cold.append(e0.elapsed_time(e1))
        c = statistics.median(cold)
        nbytes = 2.0 * N * C * 4
        lines.append(f"{N:6d} {C:5d} {S:3d} | {t:10.4f} {tt:9.3f} {t / tt:6.3f} | {nbytes / t / 1e6:16.1f} | {c:8.4f} {nbytes / c / 1e6:7.1f} | {diff:.2e}")
    lines.append(f"library: backend.functional.inception_split_scores (four launches; the workspace allocation and the host's launch time included; no "
                 f"read-back).  torch: evaluation.inception_score_reference on the same device tensor, float64.  ratio = library / torch.  logits read = "
                 f"2 N C 4 bytes per call over the library's time per call.  Per call, from windows of 50 (N C <= 2^20) or 10 back-to-back calls; "
                 f"medians of {ROUNDS} alternated windows after {WARM} warm-up rounds: the operands stay in the Infinity Cache.  cold: the library's call alone "
                 f"behind a 1 GiB fill, median of {COLD_CALLS} single calls, one event pair each (the pair's own few us included).")
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
