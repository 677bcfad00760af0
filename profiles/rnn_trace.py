"""Driver for a kernel trace of the bi-LSTM caption encoder on backend="hip" (B=24, T=10, embdim 300, nhidden 256, bidirectional):

    rocprofv3 --kernel-trace --stats -d OUT -o rnn -- python profiles/rnn_trace.py

Three eval-mode forwards under no_grad (the frozen encoder of GAN training), then three train-mode forward + backward passes (DAMSM
pretraining, dropout 0.5).  The first call of each packs W_ih per direction for the linear engine (once per weight change).  In the
steady state the eval forward is four library launches (embedding gather, two input projections, one recurrence); the train pass adds
torch's dropout, the probe loss and its seed gradient, and the library's backward (recurrence, W_hh reduction, projections,
embedding).  Committed result (a per-dispatch table made from the trace): profiles/r06_rnn_kernel_stats.txt.
"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rnn = RNN.RNNEncoder(5450, embdim=300, nhidden=256, backend="hip").to(dev)
    caps = torch.randint(1, 5450, (24, 10)).to(dev)
    lens = torch.randint(2, 11, (24,))
    rnn.eval()
    with torch.no_grad():
        for _ in range(3):
            w, s = rnn(caps, lens)
    rnn.train()
    for _ in range(3):
        w, s = rnn(caps, lens)
        (w.sum() + s.sum()).backward()
    torch.cuda.synchronize()
    print("rnn traced:", tuple(w.shape), tuple(s.shape), float(rnn.embedding.weight.grad.abs().sum()))


if __name__ == "__main__":
    main()
