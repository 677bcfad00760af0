#!/usr/bin/env python3
"""Times the two evaluation reductions (csrc/eval.hip through backend.functional) against the plain torch formulation on the same
device, with device events around windows of back-to-back calls, alternated windows, medians:

    moments_update   library: agan_moments_update (sum + upper triangle of the Gram matrix, fp64)   torch: x.double().T @ x.double()
    retrieval_rank   library: agan_retrieval_rank (R gathered rows per query)                       torch: (q[:, None] * bank[cand]).sum(-1)
                                                                                                           with its norms, in query blocks

and reports, from the shapes, the Gram kernel's share of the 78.6 TFLOP/s fp64 matrix peak -- counted on the D (D + 1) / 2 elements it
owes (n D (D + 1) flops), and on the whole tiles it launches -- and the retrieval's gather bandwidth (N R D 4 bytes), to be read
against MI355X's indexed-row rates (5.5-8.6 TB/s for rows served from the Infinity Cache or HBM).  Not run by bench.py.

    python profiles/eval_micro.py > profiles/eval_micro.txt

AGAN_LIB=<variant library> times a build of csrc/eval.hip with another Gram tile (profiles/build_variant.sh NAME "-DAGAN_GRAM_TW=4"
eval.hip); `--tile T` only labels the table with the tile width of the library in use.
"""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HF = importlib.import_module("attention-gan_amd.backend.functional")

MOMENT_SHAPES = [(256, 2048), (4096, 2048), (30_000, 2048)]
RETRIEVAL = (30_000, 30_000, 256, 100)          # N, M, D, R
ROUNDS, WARM = 9, 2
PEAK_FP64_MATRIX = 78.6e12
TORCH_QUERY_BLOCK = 3000                        # queries per block of the torch retrieval: bank[cand] of a block is 307 MB


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
        sys.exit("eval_micro: needs an MI355X (timings on a CPU say nothing about it)")
    dev = "cuda"
    tile = int(sys.argv[sys.argv.index("--tile") + 1]) if "--tile" in sys.argv else 64
    g = torch.Generator().manual_seed(0)
    print(f"library: {HF.L.LIB_PATH} (Gram workgroup tile {tile} x {tile})")
    print(f"{'n':>6s} {'D':>5s} | {'update ms':>9s} {'torch ms':>9s} {'ratio':>6s} | {'TFLOP/s owed':>12s} {'of peak':>7s} {'launched':>9s} {'of peak':>7s} | "
          f"{'workgroups':>10s} | max rel. difference")
    for n, D in MOMENT_SHAPES:
        x = (3.0 + 0.5 * torch.randn(n, D, generator=g)).to(dev)
        s = torch.zeros(D, dtype=torch.float64, device=dev)
        gm = torch.zeros(D, D, dtype=torch.float64, device=dev)

        def torch_moments():
            x64 = x.double()
            return x64.sum(0), x64.t() @ x64

        HF.moments_update(x, s, gm)
        ref = torch_moments()[1]
        diff = float((torch.triu(gm - ref).abs() / ref).max())
        calls = 20 if n <= 4096 else 5
        t, tt = alternated([lambda: HF.moments_update(x, s, gm), torch_moments], calls)
        nt = -(-D // tile)
        wgs = nt * (nt + 1) // 2
        owed, launched = n * D * (D + 1.0), 2.0 * n * wgs * tile * tile
        print(f"{n:6d} {D:5d} | {t:9.3f} {tt:9.3f} {t / tt:6.2f} | {owed / t / 1e9:12.1f} {100 * owed / t / 1e-3 / PEAK_FP64_MATRIX:6.1f}% "
              f"{launched / t / 1e9:9.1f} {100 * launched / t / 1e-3 / PEAK_FP64_MATRIX:6.1f}% | {wgs:10d} | {diff:.2e}")
    print("update: backend.functional.moments_update into a live state (sum pieces, sum, Gram kernel; workspace allocation and host launch time "
          "included); torch: x.double().sum(0) and the FULL x.double().T @ x.double() (2 n D^2 flops, the conversion included).  ratio = library / torch.  "
          f"Per call, from windows of 20 (n <= 4096) or 5 back-to-back calls; medians of {ROUNDS} alternated windows after {WARM} warm-up rounds.")

    N, M, D, R = RETRIEVAL
    q, bank = torch.randn(N, D, generator=g).to(dev), torch.randn(M, D, generator=g).to(dev)
    cand = torch.randint(0, M, (N, R), generator=g).to(torch.int32).to(dev)
    cand64 = cand.long()

    def torch_rank():
        out = []
        for lo in range(0, N, TORCH_QUERY_BLOCK):
            qb, b = q[lo:lo + TORCH_QUERY_BLOCK], bank[cand64[lo:lo + TORCH_QUERY_BLOCK]]
            sc = (qb[:, None] * b).sum(-1) / (qb.norm(dim=1)[:, None] * b.norm(dim=-1)).clamp(min=1e-8)
            out.append((sc[:, 1:] >= sc[:, :1]).sum(1))
        return torch.cat(out)

    def lib_rank():
        rank = torch.empty(N, dtype=torch.int32, device=dev)        # the entry itself: the wrapper's read-back of the verdict would
        HF._kmeans_call("agan_retrieval_rank", HF._p(q), HF._p(bank), HF._p(cand), N, M, D, R, None, HF._p(rank), HF._stream())   # end every window
        return rank

    same = float((lib_rank().long() == torch_rank()).float().mean())
    t, tt = alternated([lib_rank, torch_rank], 5)
    nbytes = N * R * D * 4.0
    print()
    print(f"{'N':>6s} {'M':>6s} {'D':>4s} {'R':>4s} | {'rank ms':>8s} {'torch ms':>9s} {'ratio':>6s} | {'gathered TB/s':>13s} | ranks equal")
    print(f"{N:6d} {M:6d} {D:4d} {R:4d} | {t:8.3f} {tt:9.3f} {t / tt:6.2f} | {nbytes / t / 1e9:13.2f} | {100 * same:.2f}%")
    print(f"rank: agan_retrieval_rank without scores (one launch; the Python wrapper adds one read-back of the ranks); torch: gather, product, sum, norms and "
          f"compare in fp32 over blocks of {TORCH_QUERY_BLOCK} queries.  gathered = N R D 4 bytes of bank rows ({M * D * 4 / 1e6:.0f} MB table).  "
          f"Per call, from windows of 5 back-to-back calls; medians as above.  Ranks differ where two fp32 cosines tie within rounding.")


if __name__ == "__main__":
    main()
