"""Driver for a kernel trace of the Inception-v3 trunk on backend="hip" (eval mode, B=24, 256x256), forward + image gradient:

    rocprofv3 --kernel-trace --stats -d OUT -o trunk -- python profiles/encoder_trace.py

It runs the trunk twice.  The first call folds and packs the 94 convs' weights (a handful of torch element-wise kernels per conv,
once per weight change) and builds the k-tables; the second is the steady state, where every kernel launched between the image and
the two outputs and back is one of the library's (libagan_hip.so).  Only the probe loss (two sums) and its seed gradient are
torch's.  Committed result: profiles/r05_encoder_kernel_stats.txt.
"""
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = ENC.CNNEncoder(256, backend="hip").to(dev).eval()
    enc.freeze_all_weights()
    x = (torch.rand(24, 3, 256, 256, device=dev) * 2 - 1).requires_grad_(True)
    for _ in range(2):
        f, c = enc(x)
        (f.sum() + c.sum()).backward()
    torch.cuda.synchronize()
    print("trunk traced:", tuple(f.shape), tuple(c.shape), float(x.grad.abs().sum()))


if __name__ == "__main__":
    main()
