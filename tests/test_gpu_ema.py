"""agan_ema_update on an MI355X against the float64 oracle (backend.functional.ema_reference): segment shapes and alignments with
canaries around every destination, accuracy over 50 updates, the update count advancing on HIP-graph replay, refused arguments.

The bound, per element:  |got - fp64| <= 2^-24 * M * (1 + 6 (1 - beta)) / (1 - beta),  M the largest |src| or |dst| of the segment.
One update rounds src - dst (magnitude <= 2 M), omb * d and the sum (<= M) -- at most three fp32 roundings (the kernel fuses the last
two into one) -- and uses an omb that is itself rounded; an error carried forward is multiplied by beta each update, hence the
geometric sum 1 / (1 - beta).  Taken at beta = 0.9, where it is loosest: 16 * 2^-24 * M."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")

DEV = torch.device("cuda", 0)
BETA = 0.9
BOUND = 2.0 ** -24 * (1 + 6 * (1 - BETA)) / (1 - BETA)          # times M
CANARY = -12345.678
PAD = 8                                                          # floats around every destination (a multiple of 4: keeps the alignment)


class Seg:
    """src and dst views of n floats at the given float offsets from a 16-byte boundary; dst sits inside a canary-filled buffer"""

    def __init__(self, n, g, src_off=0, dst_off=0, scale=1.0):
        self.n, self.scale = n, scale
        self.src_buf = torch.full((n + src_off,), CANARY, device=DEV)
        self.dst_buf = torch.full((n + 2 * PAD + dst_off,), CANARY, device=DEV)
        self.src = self.src_buf[src_off:src_off + n]
        self.lo = PAD + dst_off
        self.dst = self.dst_buf[self.lo:self.lo + n]
        self.src.copy_(torch.randn(n, generator=g) * scale)
        self.dst.copy_(torch.randn(n, generator=g) * scale)
        assert self.src.data_ptr() % 16 == 4 * (src_off % 4) and self.dst.data_ptr() % 16 == 4 * (dst_off % 4)

    def canaries(self):
        return torch.cat([self.dst_buf[:self.lo], self.dst_buf[self.lo + self.n:]])

    def triple(self):
        return (self.src.data_ptr(), self.dst.data_ptr(), self.n)


def _state(t=0):
    s = torch.zeros(4, dtype=torch.int32, device=DEV)
    s[0] = t
    return s


def _update(segs, state, decay=BETA, warmup=True, table=None):
    table = table or HF.ema_table([s.triple() for s in segs], DEV)
    HF.ema_update_(*table, state, decay, warmup, segs[0].dst_buf)
    return table


def test_segments_alignments_and_canaries():
    g = torch.Generator().manual_seed(0)
    segs = [Seg(n, g) for n in (1, 3, 4, 5, 255, 1023, 4097)]
    segs.append(Seg(1027, g, src_off=1, dst_off=1))              # both 4-byte aligned only
    segs.append(Seg(517, g, src_off=0, dst_off=3))               # only dst misaligned
    segs.append(Seg((1 << 20) + 4, g))                           # more workgroups than one, 16-byte path
    segs += [Seg(8, g, dst_off=i % 4) for i in range(70)]        # BatchNorm-sized, every alignment
    T0 = 7
    state = _state(T0)
    src0 = [s.src_buf.clone() for s in segs]
    can0 = [s.canaries().clone() for s in segs]
    dst0 = [s.dst.clone() for s in segs]
    want = [HF.ema_reference(s.src, s.dst, T0, BETA, True) for s in segs]
    M = [float(torch.maximum(s.src.abs().max(), s.dst.abs().max())) for s in segs]
    table, nseg, total = _update(segs, state)
    torch.cuda.synchronize()
    assert nseg == len(segs) == 80 and total >= nseg + 1024
    assert state.tolist()[0] == T0 + 1
    omb = state[2:3].view(torch.float32).item()
    assert omb == float(torch.tensor(1.0 - (1.0 + T0) / (10.0 + T0), dtype=torch.float64).float())
    worst = 0.0
    for i, s in enumerate(segs):
        assert torch.equal(s.src_buf.view(torch.int32), src0[i].view(torch.int32)), f"segment {i}: src changed"
        assert torch.equal(s.canaries().view(torch.int32), can0[i].view(torch.int32)), f"segment {i}: wrote outside [dst, dst + n)"
        err = float((s.dst.double() - want[i]).abs().max())
        worst = max(worst, err / (BOUND * M[i]))
        assert err <= BOUND * M[i], f"segment {i} (n = {s.n}): error {err:.3e} > {BOUND * M[i]:.3e}"
        assert not torch.equal(s.dst, dst0[i]) and not torch.equal(s.dst, s.src), f"segment {i}: not an average"
    print(f"one update, 80 segments: worst error / bound = {worst:.4f}")


def test_accuracy_over_50_updates():
    g = torch.Generator().manual_seed(1)
    shapes = [(4097, 0, 0), (515, 1, 1), (8, 0, 2), (1 << 16, 0, 0)]
    segs = [Seg(n, g, so, do, scale) for scale in (1e-3, 1.0, 1e3) for n, so, do in shapes]
    state = _state()
    ref = [s.dst.double() for s in segs]
    M = [float(s.dst.abs().max()) for s in segs]
    table = None
    for t in range(50):
        for i, s in enumerate(segs):
            s.src.copy_(torch.randn(s.n, generator=g) * s.scale)
            ref[i] = HF.ema_reference(s.src, ref[i], t, BETA, True)
            M[i] = max(M[i], float(s.src.abs().max()), float(ref[i].abs().max()))
        table = _update(segs, state, table=table)
        for i, s in enumerate(segs):
            M[i] = max(M[i], float(s.dst.abs().max()))
    torch.cuda.synchronize()
    assert state.tolist()[0] == 50
    worst = 0.0
    for i, s in enumerate(segs):
        err = float((s.dst.double() - ref[i]).abs().max())
        worst = max(worst, err / (BOUND * M[i]))
        assert err <= BOUND * M[i], f"segment {i} (n = {s.n}, scale {s.scale:g}): error {err:.3e} > {BOUND * M[i]:.3e}"
        assert torch.equal(s.canaries(), torch.full_like(s.canaries(), CANARY))
    print(f"50 updates, decay 0.9 with warm-up: worst error / bound = {worst:.4f}")


def test_update_count_advances_on_graph_replay():
    g = torch.Generator().manual_seed(2)
    seq = [torch.randn(4099, generator=g).to(DEV) for _ in range(6)]

    def fresh():
        gg = torch.Generator().manual_seed(3)
        return [Seg(4099, gg), Seg(8, gg, dst_off=1)], _state()

    segs, state = fresh()
    table = None
    for x in seq:
        segs[0].src.copy_(x)
        table = _update(segs, state, table=table)
    torch.cuda.synchronize()
    want = [s.dst.clone() for s in segs]
    assert state.tolist()[0] == 6

    segs, state = fresh()
    segs[0].src.copy_(seq[0])
    table = _update(segs, state)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _update(segs, state, table=table)
    for x in seq[1:]:
        segs[0].src.copy_(x)
        graph.replay()
    torch.cuda.synchronize()
    assert state.tolist()[0] == 6
    for a, b in zip(segs, want):
        assert torch.equal(a.dst, b)
    # and beta_t did move: six updates at the constant decay give another result
    segs, state = fresh()
    for x in seq:
        segs[0].src.copy_(x)
        table = _update(segs, state, warmup=False)
    assert not torch.equal(segs[0].dst, want[0])


def test_bad_arguments_launch_nothing():
    g = torch.Generator().manual_seed(4)
    seg = Seg(64, g)
    state = _state(5)
    before = seg.dst_buf.clone()
    table = HF.ema_table([seg.triple()], DEV)
    with pytest.raises(L.AganError):
        HF.ema_update_(table[0], 0, table[2], state, BETA, True, seg.dst_buf)                  # nseg = 0
    with pytest.raises(L.AganError):
        HF.ema_table([seg.triple(), (seg.src.data_ptr(), seg.dst.data_ptr(), 0)], DEV)         # a zero-length segment
    with pytest.raises(L.AganError):
        HF.ema_update_(*table, state, 1.0, True, seg.dst_buf)                                  # decay = 1
    with pytest.raises(L.AganError):
        HF.ema_update_(*table, state.cpu(), BETA, True, seg.dst_buf)
    torch.cuda.synchronize()
    assert torch.equal(seg.dst_buf, before) and state.tolist() == [5, 0, 0, 0]
