"""Driver for a kernel trace of one DAMSM pretrain batch with both encoders on the library (CNNEncoder(backend="hip", hip_train=True),
RNNEncoder(backend="hip")), B=24, 256x256:

    rocprofv3 --kernel-trace --stats -d OUT -o damsm -- python profiles/damsm_trace.py
    python profiles/damsm_trace.py --summarize OUT/damsm_results.db      (no GPU: reads the trace database)

It runs three steps.  The first packs the trunk's 94 conv weights and the RNN's projections and builds the k-tables; the later ones
are the steady state.  The dispatches of a step are those between two `resize_bilinear_fwd_kernel` launches (the trunk's first
kernel).  Committed result: profiles/r07_damsm_kernel_stats.txt.
"""
import collections
import importlib
import os
import sqlite3
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
    TR = importlib.import_module("attention-gan_amd.trainers.trainer")
    dev = torch.device("cuda:0")
    B, T, vocab, emb = 24, 10, 1000, 256
    torch.manual_seed(0)
    cnn = ENC.CNNEncoder(emb, backend="hip", hip_train=True).to(dev).train()
    rnn = RNN.RNNEncoder(vocabsize=vocab, nhidden=emb, backend="hip").to(dev).train()
    step = TR.DAMSMTrainStep(rnn, cnn)
    caps = torch.randint(1, vocab, (B, T)).to(dev)
    lens = torch.randint(2, T + 1, (B,))
    lens[0] = T
    img = torch.rand(B, 3, 256, 256, device=dev) * 2 - 1
    for _ in range(3):
        out = step.step(caps, lens, None, img)
    torch.cuda.synchronize()
    print("damsm traced:", {k: round(float(v), 4) for k, v in out.items()})


def summarize(db):
    """per-step table of the traced dispatches: code object (libagan_hip or torch / runtime), calls, kernel time, name"""
    c = sqlite3.connect(db)
    uri = dict(c.execute("select id, uri from code_objects"))
    rows = list(c.execute("select name, code_object_id, duration from kernels order by start"))
    starts = [i for i, r in enumerate(rows) if "resize_bilinear_fwd_kernel" in r[0]] + [len(rows)]
    print(f"{len(rows)} dispatches, {len(starts) - 1} steps (split at each resize_bilinear_fwd_kernel, the trunk's first kernel)")
    for k in range(len(starts) - 1):
        part = rows[starts[k]:starts[k + 1]]
        agg = collections.defaultdict(lambda: [0, 0])
        for name, co, dur in part:
            lib = "libagan_hip" if "libagan_hip" in uri.get(co, "") else "torch/rt"
            a = agg[(lib, name.replace("(anonymous namespace)::", "").split("(")[0][:100])]
            a[0] += 1
            a[1] += dur
        tot = sum(a[1] for a in agg.values())
        by_lib = collections.Counter()
        for (lib, _), a in agg.items():
            by_lib[lib] += a[0]
        print(f"\n== step {k + 1}: {len(part)} dispatches, {tot / 1e6:.2f} ms of kernel time; by code object: "
              + ", ".join(f"{l} {n}" for l, n in sorted(by_lib.items())))
        print("   code object   calls  total ms      %  kernel")
        for (lib, name), (n, d) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
            print(f"   {lib:12s} {n:6d} {d / 1e6:9.3f} {100 * d / tot:6.1f}  {name}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        main()
