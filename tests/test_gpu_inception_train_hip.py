"""CNNEncoder(backend="hip", hip_train=True): the TRAIN-mode Inception-v3 trunk on the library's kernels (batch-statistics BatchNorm on
channel slices, csrc/bn_slice.hip) against the stock module in float64 on the CPU, also in .train(): outputs, image gradient, running
statistics; no stock op on the way; run-to-run identity; the forward-only (DAMSM) mode; the eval fold after train-mode passes; the
slice kernels on their own; a whole DAMSM pretrain step.

The BatchNorm buffers and affine parameters are random and non-trivial, as in test_gpu_inception_hip.py.
"""
import copy
import importlib

import pytest
import torch

from helpers import RTOL, probe, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"

E = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")
P = importlib.import_module("attention-gan_amd.networks.inception_plan")


def randomise_bn(enc, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                C = m.num_features
                m.running_mean.copy_(0.2 * torch.randn(C, generator=g))
                m.running_var.copy_(0.5 + torch.rand(C, generator=g))
                m.weight.copy_(0.6 + 0.8 * torch.rand(C, generator=g))
                m.bias.copy_(0.1 * torch.randn(C, generator=g))
    return enc


def make_pair(seed, out_dim=32):
    """(stock CPU encoder in train mode, its hip_train copy on the device)"""
    torch.manual_seed(seed)
    ref = randomise_bn(E.CNNEncoder(out_dim), seed + 1).train()
    hip = copy.deepcopy(ref)
    hip.backend, hip.hip_train = "hip", True
    return ref, hip.to(DEV)


def rel_l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm().clamp(min=1e-30))


def run(enc, x):
    x = x.clone().requires_grad_(True)
    feat, code = enc(x)
    loss = (feat * probe(feat.shape, 0.3).to(feat)).sum() + (code * probe(code.shape, 1.1).to(code)).sum()
    loss.backward()
    return feat.detach(), code.detach(), x.grad


def bn_state(enc):
    return {n: b.detach().clone() for n, b in enc.named_buffers()}


def assert_stats_match(hip, ref, what):
    hs, rs = bn_state(hip), bn_state(ref)
    assert hs.keys() == rs.keys()
    for n, r in rs.items():
        h = hs[n]
        if n.endswith("num_batches_tracked"):
            assert int(h) == int(r), (what, n, int(h), int(r))
        else:
            assert rel_err(h, r) < RTOL, (what, n, rel_err(h, r))


def hip_branches(hip, x):
    """the branch every ReLU of the train-mode HIP trunk took on x and the argmax of every max pool (run on a copy of `hip`: the
    running statistics of `hip` itself are not touched)"""
    class Ctx:
        pass
    ctx = Ctx()
    plan = P.build_plan(x.shape[-2], x.shape[-1])
    ctx.saved_tensors = ()
    ctx.save_for_backward = lambda *t: setattr(ctx, "saved_tensors", t)
    with torch.no_grad():
        f6e, _ = HF._InceptionTrunkTrainFn.forward(ctx, x, copy.deepcopy(hip), plan, True)
    assert ctx.saved_tensors[0] is f6e
    T = dict(ctx.masks, **{P.FEATURES: f6e})
    masks = {op.name: (T[op.dst][:, op.out_c0:op.out_c0 + op.Cout] > 0).cpu() for op in plan.convs()}
    pools = [ctx.argmax[i].view(x.shape[0], op.C, op.OH * op.OW).long().cpu() for i, op in enumerate(plan.ops) if op.kind == "maxpool"]
    return masks, pools


def force_branches(enc, masks, pools):
    """every conv-BN-ReLU of `enc` outputs BN(conv(x)) * mask and every max pool picks the element the HIP path picked (see
    test_gpu_inception_hip.py::force_branches).  The hook runs the train-mode BatchNorm a second time, so `enc`'s running statistics
    are not meaningful afterwards.  -> undo()"""
    F = E.F
    orig = F.max_pool2d
    queue = list(pools)

    def max_pool_at(x, *a, **k):
        t = queue.pop(0).to(x.device)
        B, C, H, W = x.shape
        cols = torch.nn.functional.unfold(x, 3, stride=2).view(B, C, 9, -1)
        y = cols.gather(2, t.unsqueeze(2)).squeeze(2)
        return y.view(B, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1)
    F.max_pool2d = max_pool_at
    hooks = []
    for name, m in enc.named_modules():
        if isinstance(m, E._ConvBNReLU):
            mk = masks[name]
            hooks.append(m.register_forward_hook(lambda mod, inp, out, mk=mk: mod.bn(mod.conv(inp[0])) * mk.to(out.dtype)))

    def undo():
        F.max_pool2d = orig
        for h in hooks:
            h.remove()
        assert not queue, "the stock forward ran fewer max pools than the plan"
    return undo


@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("H", [256, 64])
def test_train_trunk_matches_fp64(B, H):
    ref, hip = make_pair(3 + B)
    g = torch.Generator().manual_seed(H + B)
    x, x2 = (torch.rand(B, 3, H, H, generator=g) * 2 - 1 for _ in range(2))
    ref64 = copy.deepcopy(ref).double()
    forced = copy.deepcopy(ref64)
    masks, pools = hip_branches(hip, x.to(DEV))
    fw, cw, gw = run(ref64, x.double())
    f, c, gx = run(hip, x.to(DEV))
    assert f.shape == (B, 32, 17, 17) and c.shape == (B, 32)
    assert rel_err(f, fw) < RTOL, rel_err(f, fw)
    assert rel_err(c, cw) < RTOL, rel_err(c, cw)
    # the image gradient, differentiating the ReLU and max-pool branches the HIP forward took
    undo = force_branches(forced, masks, pools)
    try:
        fm, cm, gm = run(forced, x.double())
    finally:
        undo()
    print(f"\nB={B} {H}px: features {rel_err(f, fw):.2e}, code {rel_err(c, cw):.2e}, image gradient {rel_l2(gx, gm):.2e} "
          f"(same branches) / {rel_l2(gx, gw):.2e} (free-running fp64)")
    assert rel_err(fm, fw) < RTOL and rel_err(cm, cw) < RTOL
    assert rel_l2(gx, gm) < RTOL, rel_l2(gx, gm)
    # a second forward: the running statistics have moved twice, num_batches_tracked is 2 everywhere
    run(ref64, x2.double())
    run(hip, x2.to(DEV))
    assert_stats_match(hip, ref64, "after two forwards")
    assert int(hip.Mixed_7c.branch_pool.bn.num_batches_tracked) == 2


def test_no_stock_op_runs():
    _, hip = make_pair(21)
    x = (torch.rand(3, 3, 64, 64, device=DEV) * 2 - 1).requires_grad_(True)
    nnf = torch.nn.functional
    saved = nnf.conv2d, nnf.batch_norm, torch.conv2d, torch.batch_norm

    def boom(*a, **k):
        raise AssertionError("a stock convolution / BatchNorm ran")
    nnf.conv2d = nnf.batch_norm = torch.conv2d = torch.batch_norm = boom
    try:
        f, c = hip(x)
        (f.sum() + c.sum()).backward()
        torch.cuda.synchronize()
    finally:
        nnf.conv2d, nnf.batch_norm, torch.conv2d, torch.batch_norm = saved
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert "_agan_trunk_fold" not in hip.__dict__, "train mode must not fold"


def test_run_to_run_identical():
    _, hip = make_pair(9)
    other = copy.deepcopy(hip)
    x = torch.rand(4, 3, 128, 128, device=DEV) * 2 - 1
    a, b = run(hip, x), run(other, x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    sa, sb = bn_state(hip), bn_state(other)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


def test_forward_only_modes_save_nothing_and_update_stats():
    ref, hip = make_pair(17)
    x = torch.rand(3, 3, 64, 64) * 2 - 1
    xd = x.to(DEV)
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        fw, cw = ref64(x.double())
    saving = copy.deepcopy(hip)
    f0, c0, _ = run(saving, xd)                           # the forward that saves for a backward
    t0 = HF.inception_trunk_train(xd.clone().requires_grad_(True), copy.deepcopy(hip))
    # under no_grad, even with an image that requires grad
    h_ng = copy.deepcopy(hip)
    with torch.no_grad():
        f, c = h_ng(xd.clone().requires_grad_(True))
    assert f.grad_fn is None and c.grad_fn is None
    # grad mode on, an image without grad (the DAMSM case): the trunk's outputs carry no graph
    h_ig = copy.deepcopy(hip)
    t6e, tpool = HF.inception_trunk_train(xd, h_ig)
    assert t6e.grad_fn is None and tpool.grad_fn is None
    assert t0[0].grad_fn is not None
    # same kernels in the same order: identical to the saving forward, and within RTOL of fp64
    assert torch.equal(f, f0) and torch.equal(c, c0)
    assert torch.equal(t6e, t0[0].detach()) and torch.equal(tpool, t0[1].detach())
    assert rel_err(f, fw) < RTOL and rel_err(c, cw) < RTOL
    s_sv = bn_state(saving)
    for h in (h_ng, h_ig):
        sh = bn_state(h)
        for n in sh:
            assert torch.equal(sh[n], s_sv[n]), n
    assert_stats_match(h_ng, ref64, "forward only")


def test_eval_after_train_sees_updated_statistics():
    ref, hip = make_pair(29)
    x = torch.rand(2, 3, 64, 64) * 2 - 1
    ref64 = copy.deepcopy(ref).double()
    hip.eval()
    with torch.no_grad():
        hip(x.to(DEV))                   # fills the eval fold cache with the initial statistics
    assert "_agan_trunk_fold" in hip.__dict__
    hip.train()
    for k in range(2):
        xk = torch.rand(2, 3, 64, 64) * 2 - 1
        with torch.no_grad():
            hip(xk.to(DEV))
            ref64(xk.double())
    hip.eval()
    ref64.eval()
    with torch.no_grad():
        f, c = hip(x.to(DEV))
        fw, cw = ref64(x.double())
    assert rel_err(f, fw) < RTOL and rel_err(c, cw) < RTOL, (rel_err(f, fw), rel_err(c, cw))


def test_unsupported_setups_raise():
    _, hip = make_pair(31)
    x = torch.rand(2, 3, 64, 64, device=DEV) * 2 - 1
    hip.Conv2d_4a_3x3.conv.weight.requires_grad_(True)
    with pytest.raises(ValueError):
        hip(x)
    hip.Conv2d_4a_3x3.conv.weight.requires_grad_(False)
    hip.Mixed_5b.branch1x1.bn.momentum = None
    with pytest.raises(ValueError):
        hip(x)
    assert int(hip.Conv2d_1a_3x3.bn.num_batches_tracked) == 0, "a refused call must not have run"


@pytest.mark.parametrize("B,C,HW", [(2, 3, 100), (3, 5, 289), (24, 4, 289), (3, 6, 3025), (4, 7, 5329)],
                         ids=["small-2", "small-8", "small-32", "large-9k", "large-21k"])
def test_slice_kernels_vs_fp64(B, C, HW):
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + HW)
    c0, ctot = 3, C + 5
    eps, mom = 1e-3, 0.1
    x = torch.randn(B, C, HW, generator=g) * 1.7 + 0.6
    gamma, beta = 0.6 + 0.8 * torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g)
    rm, rv = 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    d = {k: v.to(DEV) for k, v in dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv).items()}
    out = torch.full((B, ctot, HW), 7.0, device=DEV)
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    nbt = torch.tensor(5, dtype=torch.int64, device=DEV)
    st = HF._stream()
    lib = L.load()
    wn = lib.agan_bn_relu_slice_fwd_ws_bytes(B, C, HW)
    assert (wn == 0) == (B * HW <= 8192)
    wst, ws = HF._ws(wn, out)
    P_ = HF._p
    L.call("agan_bn_relu_slice_fwd", P_(d["x"]), P_(d["gamma"]), P_(d["beta"]), P_(out), c0, ctot, P_(mean), P_(invstd), P_(d["rm"]),
           P_(d["rv"]), P_(nbt), B, C, HW, eps, mom, ws, wn, st)
    xd = x.double()
    m = xd.mean(dim=(0, 2))
    var = xd.var(dim=(0, 2), unbiased=False)
    n = B * HW
    iw = 1.0 / torch.sqrt(var + eps)
    xh = (xd - m.view(1, -1, 1)) * iw.view(1, -1, 1)
    y = torch.relu(gamma.double().view(1, -1, 1) * xh + beta.double().view(1, -1, 1))
    assert rel_err(out[:, c0:c0 + C], y) < 1e-5
    assert bool((out[:, :c0] == 7.0).all()) and bool((out[:, c0 + C:] == 7.0).all()), "wrote outside its slice"
    assert rel_err(mean, m) < 1e-6 and rel_err(invstd, iw) < 1e-6
    assert rel_err(d["rm"], (1 - mom) * rm.double() + mom * m) < 1e-6
    assert rel_err(d["rv"], (1 - mom) * rv.double() + mom * var * n / (n - 1)) < 1e-6
    assert int(nbt) == 6
    # backward from a slice of a wider gradient
    dy_full = torch.randn(B, ctot, HW, generator=g)
    dx = torch.full((B, C, HW), 7.0, device=DEV)
    wn = lib.agan_bn_slice_bwd_ws_bytes(B, C, HW)
    wst, ws = HF._ws(wn, out)
    dyd = dy_full.to(DEV)
    L.call("agan_bn_slice_bwd", P_(d["x"]), P_(dyd), c0, ctot, P_(mean), P_(invstd), P_(d["gamma"]), P_(dx), B, C, HW, ws, wn, st)
    dy = dy_full[:, c0:c0 + C].double()
    want = (gamma.double() * iw).view(1, -1, 1) * (dy - dy.mean(dim=(0, 2), keepdim=True)
                                                   - xh * (dy * xh).mean(dim=(0, 2), keepdim=True))
    assert rel_err(dx, want) < 1e-5, rel_err(dx, want)
    # the same call again: bit for bit
    dx2 = torch.empty_like(dx)
    L.call("agan_bn_slice_bwd", P_(d["x"]), P_(dyd), c0, ctot, P_(mean), P_(invstd), P_(d["gamma"]), P_(dx2), B, C, HW, ws, wn, st)
    assert torch.equal(dx, dx2)


def test_damsm_step_with_hip_encoders():
    """One DAMSMTrainStep with RNNEncoder(backend="hip") and CNNEncoder(backend="hip", hip_train=True) against the same batch through
    the stock encoders in float64 on the CPU (train mode), the oracle's losses, the RNN clip and torch.optim.Adam: losses, clipped
    gradients, post-step weights and the trunk's running statistics.  (The stock encoders on the device are no yardstick here: at
    this shape the MIOpen train-mode trunk's features are ~4e-2 from float64, the hip trunk's ~5e-5.)"""
    from oracle import attngan_oracle as O   # checker only
    RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
    TR = importlib.import_module("attention-gan_amd.trainers.trainer")
    B, Tn, emb, vocab = 4, 10, 32, 50
    torch.manual_seed(5)
    rnn = RNN.RNNEncoder(vocab, embdim=24, dropprob=0.0, nhidden=emb, backend="hip").to(DEV).train()
    ref, cnn = make_pair(37, emb)
    rnn_c, cnn_c = copy.deepcopy(rnn).cpu().double(), copy.deepcopy(ref).double()
    rnn_c.backend = "torch"
    g = torch.Generator().manual_seed(5)
    caps = torch.randint(0, vocab, (B, Tn), generator=g)
    lens = torch.tensor([10, 7, 2, 10])
    img = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1
    step = TR.DAMSMTrainStep(rnn, cnn)
    out = step.step(caps.to(DEV), lens, None, img.to(DEV))
    torch.cuda.synchronize()
    params_c = list(rnn_c.parameters()) + [p for p in cnn_c.parameters() if p.requires_grad]
    ref_opt = torch.optim.Adam(params_c, lr=2e-3, betas=(0.5, 0.999))
    feats, code = cnn_c(img.double())
    wemb, semb = rnn_c(caps, lens)
    wl, _ = O.words_loss(feats, wemb, torch.arange(B), lens.tolist(), None)
    sl = O.sentence_loss(code, semb, torch.arange(B), None)
    assert rel_err(out["w_loss"], wl) < RTOL, (float(out["w_loss"]), float(wl))
    assert rel_err(out["s_loss"], sl) < RTOL, (float(out["s_loss"]), float(sl))
    ref_opt.zero_grad()
    (wl + sl).backward()
    torch.nn.utils.clip_grad_norm_(rnn_c.parameters(), 0.25)
    named_c = [(n, p) for n, p in list(rnn_c.named_parameters()) + list(cnn_c.named_parameters()) if p.requires_grad]
    named_d = [(n, p) for n, p in list(rnn.named_parameters()) + list(cnn.named_parameters()) if p.requires_grad]
    assert [n for n, _ in named_c] == [n for n, _ in named_d] and any(n.startswith("emb_") for n, _ in named_d)
    for (n, pc), (_, pd) in zip(named_c, named_d):
        assert rel_err(pd.grad, pc.grad) < RTOL, (n, rel_err(pd.grad, pc.grad))
    ref_opt.step()
    flips = total = 0
    for (n, pc), (_, pd) in zip(named_c, named_d):
        # the first Adam step is lr * sign(g): an element may flip only where its gradient is rounding noise of its tensor
        diff = (pd.detach().cpu().double() - pc.detach()).abs()
        off = diff > RTOL * float(pc.detach().abs().max())
        total += pc.numel()
        if int(off.sum()):
            gabs = pc.grad.detach().abs()
            assert float(diff.max()) <= 2.05 * 2e-3 and float(gabs[off].max() / gabs.max()) <= 2 * RTOL, n
            flips += int(off.sum())
    assert flips <= max(2, int(1e-3 * total)), f"{flips} of {total} trainable weights differ from the reference step"
    assert_stats_match(cnn, cnn_c, "DAMSM step")
    assert int(cnn.Conv2d_1a_3x3.bn.num_batches_tracked) == 1
