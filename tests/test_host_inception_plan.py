"""CPU checks of the Inception-v3 trunk's layer plan (networks/inception_plan.py) and of the data-gradient decompositions the general
2-D conv kernels use (include/agan.h: agan_conv2d_dgrad) -- no GPU needed.

* the plan covers every conv / pool / resize of CNNEncoder in execution order, with torch's output shapes, for 64 / 128 / 256 px;
* the branches of every Mixed block tile its output channels [0, Ctot) exactly;
* the 3x3 stride-2 parity decomposition (AGAN_PACK_DGRAD_3x3S2) and the stride-1 flipped-weight gathers with per-axis padding
  (AGAN_PACK_DGRAD_S1) equal torch.nn.grad.conv2d_input bit for bit on dyadic grid operands, applied with plain fp64 torch ops.
"""
import importlib

import pytest
import torch
import torch.nn.functional as F

E = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
P = importlib.import_module("attention-gan_amd.networks.inception_plan")


def _trace_encoder(H):
    """the ops CNNEncoder's stock forward runs, in order, from hooks on the conv modules and patched functional pools"""
    enc = E.CNNEncoder(8).eval().to("meta")
    seen = []
    hooks = [m.register_forward_hook(lambda mod, inp, out, name=name: seen.append(("conv", name, tuple(out.shape))))
             for name, m in enc.named_modules() if isinstance(m, E._ConvBNReLU)]
    orig = (F.max_pool2d, F.avg_pool2d, F.interpolate)

    def mp(x, *a, **k):
        y = orig[0](x, *a, **k)
        seen.append(("maxpool", None, tuple(y.shape)))
        return y

    def ap(x, *a, **k):
        y = orig[1](x, *a, **k)
        seen.append(("avgpool" if y.shape[-1] > 1 else "gap", None, tuple(y.shape)))
        return y

    def rs(x, *a, **k):
        y = orig[2](x, *a, **k)
        seen.append(("resize", None, tuple(y.shape)))
        return y

    E.F.max_pool2d, E.F.avg_pool2d, E.F.interpolate = mp, ap, rs
    try:
        with torch.no_grad():
            enc(torch.zeros(1, 3, H, H, device="meta"))
    finally:
        E.F.max_pool2d, E.F.avg_pool2d, E.F.interpolate = orig
        for h in hooks:
            h.remove()
    return seen


@pytest.mark.parametrize("H", [64, 128, 256])
def test_plan_matches_the_stock_forward(H):
    plan = P.build_plan(H, H)
    seen = _trace_encoder(H)
    got = []
    for op in plan.ops:
        if op.kind == "conv":
            got.append(("conv", op.name, (1, op.Cout, op.OH, op.OW)))
        elif op.kind == "gap":
            got.append(("gap", None, (1, op.C, 1, 1)))
        else:
            got.append((op.kind, None, (1, op.C, op.OH, op.OW)))
    # the same ops with the same output shapes; and the convs in the same order within every branch and block (the plan may run a
    # block's pooling branch at another point than the stock forward does: its branches are independent)
    assert sorted(map(str, got)) == sorted(map(str, seen))
    blocks = lambda ops: [o[1].split(".")[0] for o in ops if o[0] == "conv"]
    assert blocks(got) == blocks(seen)
    for pre in {o[1].rsplit("_", 1)[0] for o in got if o[0] == "conv"}:
        assert [o for o in got if o[0] == "conv" and o[1].rsplit("_", 1)[0] == pre] == \
            [o for o in seen if o[0] == "conv" and o[1].rsplit("_", 1)[0] == pre], pre
    assert len(plan.convs()) == 94


@pytest.mark.parametrize("H", [64, 128, 256])
def test_plan_shapes_equal_torch_shape_rules(H):
    plan = P.build_plan(H, H)
    for op in plan.ops:
        x = torch.empty(1, op.C, op.H, op.W, device="meta")
        if op.kind == "conv":
            y = F.conv2d(x, torch.empty(op.Cout, op.C, *op.k, device="meta"), stride=op.s, padding=op.p)
        elif op.kind == "maxpool":
            y = F.max_pool2d(x, 3, 2)
        elif op.kind == "avgpool":
            y = F.avg_pool2d(x, 3, 1, 1)
        elif op.kind == "gap":
            y = F.avg_pool2d(x, (op.H, op.W))
        else:
            y = F.interpolate(torch.empty(1, op.C, op.H, op.W), size=(P.TRUNK_SIZE, P.TRUNK_SIZE), mode="bilinear", align_corners=False)
        assert tuple(y.shape[-2:]) == (op.OH, op.OW), (op, tuple(y.shape))
        t = plan.tensors[op.dst]
        assert op.out_ctot == t.C and (t.H, t.W) == ((op.OH, op.OW) if op.kind != "gap" else (1, 1)), op
        assert plan.tensors[op.src].C == op.C, op
    assert tuple(plan.tensors[P.FEATURES].__dict__[k] for k in ("C", "H", "W")) == (768, 17, 17)
    assert plan.tensors[P.POOLED].C == 2048


def test_mixed_block_slices_tile_the_output():
    plan = P.build_plan(256, 256)
    sl = P.slices(plan)
    blocks = [n for n in sl if n.startswith("Mixed_") and "." not in n]
    assert len(blocks) == 11
    for name in blocks:
        ranges = sorted(sl[name])
        edge = 0
        for c0, c1 in ranges:
            assert c0 == edge, f"{name}: gap or overlap at channel {edge} ({ranges})"
            edge = c1
        assert edge == plan.tensors[name].C, f"{name}: slices end at {edge} of {plan.tensors[name].C}"
    for name, r in sl.items():          # every other tensor has one producer writing all of it
        if name not in blocks:
            assert r == [(0, plan.tensors[name].C)], name


def test_backward_write_order():
    """every gradient buffer is written once, then added to; the Mixed_6e gradient is seeded by the feature head"""
    plan = P.build_plan(256, 256)
    written = {P.FEATURES}
    for op in reversed(plan.ops):
        assert op.accumulate == (op.src in written), op
        written.add(op.src)
    readers = {}
    for op in plan.ops:
        readers[op.src] = readers.get(op.src, 0) + 1
    assert readers["Mixed_5b"] == 4 and readers["Mixed_6a"] == 4 and readers["Mixed_7b.t_1"] == 2


def test_plan_flops():
    plan = P.build_plan(256, 256)
    f = plan.flops_per_image(backward=False)
    print(f"\nInception-v3 trunk: {f / 1e9:.3f} GF/image forward, {2 * f / 1e9:.3f} GF/image forward + data gradient, "
          f"{len(plan.convs())} convs")
    assert 10e9 < f < 13e9


# ---- data-gradient decompositions on dyadic grids (fp64, plain torch ops) -----------------------------------------------------
def _grid(shape, gen, step):
    return torch.randint(-4, 5, shape, generator=gen).double() * step


def _dgrad_stride1(dy, w, p, ih, iw):
    """the stride-1 data gradient as the library computes it: a forward gather over dy with the flipped weights and padding K-1-P"""
    kh, kw = w.shape[-2:]
    wf = torch.flip(w, dims=(2, 3)).transpose(0, 1)                    # [Cin][Cout][KH][KW], flipped taps (AGAN_PACK_DGRAD_S1)
    ph, pw = kh - 1 - p[0], kw - 1 - p[1]
    dyp = F.pad(dy, (pw, pw, ph, ph))
    B = dy.shape[0]
    dx = torch.zeros(B, w.shape[1], ih, iw, dtype=torch.float64)
    for r in range(kh):
        for s in range(kw):
            win = dyp[:, :, r:r + ih, s:s + iw]                         # [B, Cout, IH, IW]
            dx += torch.einsum("bnyx,cn->bcyx", win, wf[:, :, r, s])
    return dx


def _dgrad_3x3s2(dy, w, ih, iw):
    """the 3x3 stride-2 unpadded data gradient as 4 parity classes of 2x2 taps (AGAN_PACK_DGRAD_3x3S2)"""
    B, cout, oh, ow = dy.shape
    cin = w.shape[1]
    dx = torch.zeros(B, cin, ih, iw, dtype=torch.float64)
    taps = {0: (2, 0), 1: (1, None)}      # class -> weight tap of r = 0, 1 (None: zero-weight padding); dy row = q + OY[cls] + r
    OY = {0: -1, 1: 0}
    for py in (0, 1):
        for px in (0, 1):
            qh, qw = (ih - py + 1) // 2, (iw - px + 1) // 2
            acc = torch.zeros(B, cin, qh, qw, dtype=torch.float64)
            for r in (0, 1):
                for s in (0, 1):
                    th, tw = taps[py][r], taps[px][s]
                    wt = torch.zeros(cout, cin, dtype=torch.float64) if th is None or tw is None else w[:, :, th, tw]
                    rows = torch.arange(qh) + OY[py] + r
                    cols = torch.arange(qw) + OY[px] + s
                    okr, okc = (rows >= 0) & (rows < oh), (cols >= 0) & (cols < ow)
                    win = torch.zeros(B, cout, qh, qw, dtype=torch.float64)
                    win[:, :, okr.nonzero()[:, 0][:, None], okc.nonzero()[:, 0][None, :]] = \
                        dy[:, :, rows[okr][:, None], cols[okc][None, :]]
                    acc += torch.einsum("bnyx,nc->bcyx", win, wt)
            dx[:, :, py::2, px::2] = acc
    return dx


@pytest.mark.parametrize("ih", [299, 35, 17, 8])
def test_dgrad_3x3s2_parity_decomposition_is_exact(ih):
    g = torch.Generator().manual_seed(ih)
    B, cin, cout = 2, 3, 5
    oh = (ih - 3) // 2 + 1
    w, dy = _grid((cout, cin, 3, 3), g, 2.0 ** -3), _grid((B, cout, oh, oh), g, 2.0 ** -1)
    want = torch.nn.grad.conv2d_input((B, cin, ih, ih), w, dy, stride=2, padding=0)
    got = _dgrad_3x3s2(dy, w, ih, ih)
    assert torch.equal(got, want)


@pytest.mark.parametrize("k,p,h", [((3, 3), (1, 1), 35), ((3, 3), (0, 0), 149), ((5, 5), (2, 2), 35), ((1, 7), (0, 3), 17),
                                   ((7, 1), (3, 0), 17), ((1, 3), (0, 1), 8), ((3, 1), (1, 0), 8), ((1, 1), (0, 0), 17)])
def test_dgrad_stride1_flipped_gather_is_exact(k, p, h):
    g = torch.Generator().manual_seed(h * 10 + k[0])
    B, cin, cout = 2, 4, 6
    h = min(h, 40)
    oh, ow = h + 2 * p[0] - k[0] + 1, h + 2 * p[1] - k[1] + 1
    w, dy = _grid((cout, cin) + k, g, 2.0 ** -3), _grid((B, cout, oh, ow), g, 2.0 ** -1)
    want = torch.nn.grad.conv2d_input((B, cin, h, h), w, dy, stride=1, padding=p)
    assert torch.equal(_dgrad_stride1(dy, w, p, h, h), want)
