"""Inception-v3 image-encoder trunk in TRAIN mode (batch-statistics BatchNorm): stock MIOpen vs CNNEncoder(backend="hip",
hip_train=True), B=24, 256x256.

    python profiles/encoder_train_timing.py [--batch 24] [--reps 20]

Reports, in one process, each timed with device events after warm-up, the two paths alternated per repetition (median ms):
  * the train-mode encoder forward with an image that needs no gradient (the DAMSM pretrain case: nothing is saved for the trunk);
  * forward + image gradient;
  * one DAMSMTrainStep (pretrain_damsm.py's batch) with both encoders stock vs both on hip (RNNEncoder(backend="hip") too);
  * the memory the hip trunk keeps for its backward at this batch: from the layer plan, and measured (allocated bytes held by the
    forward's graph).
"""
import argparse
import copy
import gc
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def saved_bytes_from_plan(plan, B):
    """what _InceptionTrunkTrainFn keeps for the backward: raw conv outputs, mean / invstd, every ReLU output, max-pool argmax bytes"""
    raw = sum(B * op.Cout * op.OH * op.OW * 4 + 2 * op.Cout * 4 for op in plan.convs())
    relu = sum(B * t.C * t.H * t.W * 4 for t in plan.tensors.values() if t.relu)
    am = sum(B * op.C * op.OH * op.OW for op in plan.ops if op.kind == "maxpool")
    return raw, relu, am


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    B, dev = args.batch, torch.device("cuda:0")
    bench = importlib.import_module("bench")
    ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
    PLAN = importlib.import_module("attention-gan_amd.networks.inception_plan")
    TR = importlib.import_module("attention-gan_amd.trainers.trainer")

    plan = PLAN.build_plan(256, 256)
    gf_fwd = plan.flops_per_image(backward=False) / 1e9
    raw, relu, am = saved_bytes_from_plan(plan, B)
    print(f"trunk plan: {len(plan.convs())} convs, {gf_fwd:.2f} GF/image forward; saved for the backward at B={B}: raw conv outputs "
          f"{raw / 2**20:.0f} MiB + ReLU outputs {relu / 2**20:.0f} MiB + argmax {am / 2**20:.1f} MiB = {(raw + relu + am) / 2**20:.0f} MiB")

    torch.manual_seed(0)
    enc = ENC.CNNEncoder(bench.EMB).to(dev).train()
    enc.freeze_all_weights()
    x = torch.rand(B, 3, 256, 256, device=dev) * 2 - 1
    xg = x.clone().requires_grad_(True)

    def set_path(b):
        enc.backend, enc.hip_train = b, b == "hip"

    def fwd():
        enc(x)

    def fwd_bwd():
        f, c = enc(xg)
        (f.sum() + c.sum()).backward()

    # memory held by the forward's graph (grad-mode forward with an image gradient) and by the DAMSM-case forward, per path
    for b in ("torch", "hip"):
        set_path(b)
        fwd_bwd()
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        f, c = enc(xg)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated() - base
        del f, c
        gc.collect()
        f, c = enc(x)
        torch.cuda.synchronize()
        held_nog = torch.cuda.memory_allocated() - base
        del f, c
        print(f"  {b:5s}: allocated after a forward that needs the image gradient {held / 2**20:7.0f} MiB, "
              f"without image gradient {held_nog / 2**20:6.1f} MiB")

    times = {(b, k): [] for b in ("torch", "hip") for k in ("fwd", "fwd+dgrad")}
    for b in ("torch", "hip"):                 # warm-up: MIOpen searches, packs, k-tables
        set_path(b)
        for _ in range(3):
            fwd()
            fwd_bwd()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for b in ("torch", "hip"):
            set_path(b)
            times[(b, "fwd")].append(event_ms(fwd))
            times[(b, "fwd+dgrad")].append(event_ms(fwd_bwd))
    print(f"\nencoder at B={B}, 256x256, TRAIN mode (batch statistics; median of {args.reps}, alternated; device events)")
    for k, what in (("fwd", "forward, image needs no gradient (DAMSM)"), ("fwd+dgrad", "forward + image gradient")):
        t, h = statistics.median(times[("torch", k)]), statistics.median(times[("hip", k)])
        gf = gf_fwd * B * (1 if k == "fwd" else 2)
        print(f"  {what:42s} torch {t:7.2f} ms ({gf / t:5.1f} TF/s)   hip {h:7.2f} ms ({gf / h:5.1f} TF/s)   hip/torch {h / t:5.2f}")

    # one DAMSM pretrain batch: words + sentence loss, clip, Adam over the RNN and the image encoder's heads
    g = torch.Generator().manual_seed(0)
    vocab = 1000
    caps = torch.randint(1, vocab, (B, bench.T), generator=g).to(dev)
    lens = torch.randint(2, bench.T + 1, (B,), generator=g)
    lens[0] = bench.T
    torch.manual_seed(1)
    rnn0 = RNN.RNNEncoder(vocabsize=vocab, nhidden=bench.EMB).to(dev).train()
    steps = {}
    for b in ("torch", "hip"):
        rnn, cnn = copy.deepcopy(rnn0), copy.deepcopy(enc)
        rnn.backend = b
        cnn.backend, cnn.hip_train = b, b == "hip"
        steps[b] = TR.DAMSMTrainStep(rnn, cnn)
    st_times = {b: [] for b in steps}
    for b, s in steps.items():
        for _ in range(3):
            s.step(caps, lens, None, x)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for b, s in steps.items():
            st_times[b].append(event_ms(lambda: s.step(caps, lens, None, x)))
    t, h = statistics.median(st_times["torch"]), statistics.median(st_times["hip"])
    print(f"\nDAMSMTrainStep at B={B} (CNNEncoder train mode + bi-LSTM nhidden {bench.EMB}, T={bench.T}; median of {args.reps}, alternated)")
    print(f"  both encoders stock {t:7.2f} ms ({B / t * 1e3:6.1f} img/s)   both on hip {h:7.2f} ms ({B / h * 1e3:6.1f} img/s)   "
          f"hip/torch {h / t:5.2f}")


if __name__ == "__main__":
    main()
