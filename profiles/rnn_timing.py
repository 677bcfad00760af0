"""bi-LSTM caption encoder: backend="torch" (stock embedding + pack + MIOpen LSTM + unpack) vs backend="hip" (the library's kernels),
B=24, T=10, embdim 300, nhidden 256 (128 per direction), bidirectional.

    python profiles/rnn_timing.py [--batch 24] [--reps 50] [--steps 10]

Reports, in one process:
  * the eval-mode forward under no_grad (the frozen encoder of GAN training) and the train-mode forward + backward (DAMSM
    pretraining: all nine parameter gradients), alternated torch / hip per repetition, timed with device events after warm-up
    (median ms);
  * the full metric-config G/D/DAMSM train step that `bench.py --image-encoder inception` builds, plus this encoder run every step
    (bench.py's end_to_end_inception_trunk_plus_lstm line), with each encoder backend, in img/s.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    B, dev = args.batch, torch.device("cuda:0")
    bench = importlib.import_module("bench")
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
    Tn, vocab = bench.T, 5450

    torch.manual_seed(0)
    rnn = RNN.RNNEncoder(vocabsize=vocab, embdim=300, dropprob=0.5, nhidden=256).to(dev)
    g = torch.Generator().manual_seed(0)
    caps = torch.randint(1, vocab, (B, Tn), generator=g).to(dev)
    lens = torch.randint(2, Tn + 1, (B,), generator=g)
    lens[0] = Tn
    wp = torch.randn(B, 256, Tn, device=dev)
    sp = torch.randn(B, 256, device=dev)

    def fwd_eval():
        rnn.eval()
        with torch.no_grad():
            rnn(caps, lens)

    def fwd_bwd_train():
        rnn.train()
        for p in rnn.parameters():
            p.grad = None
        w, s = rnn(caps, lens)
        ((w * wp[:, :, :w.shape[2]]).sum() + (s * sp).sum()).backward()

    cases = (("eval fwd (no_grad)", fwd_eval), ("train fwd+bwd", fwd_bwd_train))
    times = {(b, k): [] for b in ("torch", "hip") for k, _ in cases}
    for b in ("torch", "hip"):                 # warm-up: MIOpen's RNN descriptors, packed W_ih
        rnn.backend = b
        for _ in range(5):
            for _, fn in cases:
                fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for b in ("torch", "hip"):
            rnn.backend = b
            for k, fn in cases:
                times[(b, k)].append(event_ms(fn))
    print(f"bi-LSTM text encoder at B={B}, T={Tn}, embdim 300, nhidden 256 (2 x 128), lengths {lens.tolist()} "
          f"(median of {args.reps}, alternated; device events)")
    for k, _ in cases:
        t, h = statistics.median(times[("torch", k)]), statistics.median(times[("hip", k)])
        print(f"  {k:20s} torch {t:8.3f} ms   hip {h:8.3f} ms   hip/torch {h / t:5.2f}")

    # the metric-config train step with the real trunk + the frozen bi-LSTM (bench.py's end-to-end side line), per RNN backend
    print(f"\nmetric-config train step + Inception trunk (torch) + bi-LSTM, B={B}, {args.steps} timed steps after 3 warm-up")
    words, sent, lens_b, reals = bench.synthetic_batch(dev, B, 0)
    lens_full = torch.full((B,), Tn, dtype=torch.int64, device=dev)
    enc = RNN.RNNEncoder(vocabsize=1000, nhidden=bench.EMB).to(dev).eval()
    enc.freeze_all_weights()
    caps_b = torch.randint(1, 1000, (B, Tn)).to(dev)
    step = bench.build(dev, B, HF, "inception")
    for b in ("torch", "hip"):
        enc.backend = b

        def e2e():
            with torch.no_grad():
                w_e, s_e = enc(caps_b, [Tn] * B)
            return step.step(w_e.contiguous(), s_e.contiguous(), lens_full, None, reals)
        for _ in range(3):
            e2e()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            e2e()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        print(f"  rnn backend={b:5s}  {B / dt:7.1f} img/s  ({dt * 1e3:.1f} ms/step)")


if __name__ == "__main__":
    main()
