"""Inception-v3 image-encoder trunk: backend="torch" (stock MIOpen) vs backend="hip" (the library's kernels), eval mode, B=24, 256x256.

    python profiles/encoder_timing.py [--batch 24] [--reps 20] [--steps 10]

Reports, in one process:
  * the trunk forward and forward + image gradient of each backend, alternated torch / hip per repetition, timed with device events
    after warm-up (median ms);
  * the full metric-config G/D/DAMSM train step that `bench.py --image-encoder inception` builds, plus the frozen bi-LSTM text
    encoder run every step (bench.py's end_to_end_inception_trunk_plus_lstm line), with each backend, in img/s;
  * the algorithmic GF per image of the trunk, from the layer plan (networks/inception_plan.py).
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


def event_ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    B, dev = args.batch, torch.device("cuda:0")
    bench = importlib.import_module("bench")
    ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
    PLAN = importlib.import_module("attention-gan_amd.networks.inception_plan")
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")

    plan = PLAN.build_plan(256, 256)
    gf_fwd = plan.flops_per_image(backward=False) / 1e9
    print(f"trunk plan: {len(plan.convs())} convs, {gf_fwd:.2f} GF/image forward, {2 * gf_fwd:.2f} GF/image forward + data gradient "
          f"({2 * gf_fwd * B:.0f} GF per step at B={B})")

    torch.manual_seed(0)
    enc = ENC.CNNEncoder(bench.EMB).to(dev).eval()
    enc.freeze_all_weights()
    x = torch.rand(B, 3, 256, 256, device=dev) * 2 - 1
    xg = x.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            enc(x)

    def fwd_bwd():
        f, c = enc(xg)
        (f.sum() + c.sum()).backward()

    times = {(b, k): [] for b in ("torch", "hip") for k in ("fwd", "fwd+dgrad")}
    for b in ("torch", "hip"):                 # warm-up: MIOpen searches, folds, k-tables
        enc.backend = b
        for _ in range(3):
            fwd()
            fwd_bwd()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for b in ("torch", "hip"):
            enc.backend = b
            times[(b, "fwd")].append(event_ms(fwd, 1))
            times[(b, "fwd+dgrad")].append(event_ms(fwd_bwd, 1))
    print(f"\ntrunk at B={B}, 256x256, eval mode (median of {args.reps}, alternated; device events)")
    for k in ("fwd", "fwd+dgrad"):
        t, h = statistics.median(times[("torch", k)]), statistics.median(times[("hip", k)])
        gf = gf_fwd * B * (1 if k == "fwd" else 2)
        print(f"  {k:10s} torch {t:8.2f} ms ({gf / t:6.1f} TF/s)   hip {h:8.2f} ms ({gf / h:6.1f} TF/s)   hip/torch {h / t:5.2f}")

    # the metric-config train step with the real trunk + the bi-LSTM (bench.py's end-to-end side line), per backend
    print(f"\nmetric-config train step + Inception trunk + bi-LSTM, B={B}, {args.steps} timed steps after 3 warm-up")
    words, sent, lens, reals = bench.synthetic_batch(dev, B, 0)
    lens_full = torch.full((B,), bench.T, dtype=torch.int64, device=dev)
    rnn = RNN.RNNEncoder(vocabsize=1000, nhidden=bench.EMB).to(dev).eval()
    rnn.freeze_all_weights()
    caps = torch.randint(1, 1000, (B, bench.T)).to(dev)
    for b in ("torch", "hip"):
        step = bench.build(dev, B, HF, "inception")
        step.image_encoder.backend = b

        def e2e():
            with torch.no_grad():
                w_e, s_e = rnn(caps, [bench.T] * B)
            return step.step(w_e.contiguous(), s_e.contiguous(), lens_full, None, reals)
        for _ in range(3):
            e2e()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            e2e()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        print(f"  backend={b:5s}  {B / dt:7.1f} img/s  ({dt * 1e3:.1f} ms/step)")
        del step
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
