"""Packed weight forms follow the weights end to end: through a flat buffer registered again at the same address, per buffer when two
optimisers own two modules, and for the LIVE generator across graph replays (tests/test_gpu_ema_step.py checks the averaged one).
Tiny shapes: the cache's logic does not depend on them (tests/test_host_weight_forms.py has it as launch logs)."""
import importlib

import pytest
import torch

from test_gpu_ema_step import DEV, GF, EMB, Z, COND, T, _setup

pytestmark = pytest.mark.gpu

HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
LAYERS = importlib.import_module("attention-gan_amd.utilities.layers")
OPT = importlib.import_module("attention-gan_amd.optim")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")
L = HF.L

PACKS = ("agan_pack_weight", "agan_pack_weights")


@pytest.fixture(params=["f32", "bf16"])
def precision(request):
    HF.set_precision(L.PRECISIONS[request.param])
    try:
        yield request.param
    finally:
        HF.set_precision(L.PREC_F32)


def _modules():
    """a 3x3 "same" conv 16 -> 16 and a linear 16 -> 8 with their inputs; in bf16 their packs are two layout families"""
    torch.manual_seed(11)
    conv, lin = LAYERS.HipConv2d(16, 16, 3, 1, 1, bias=True).to(DEV), LAYERS.HipLinear(16, 8).to(DEV)
    g = torch.Generator().manual_seed(11)
    return conv, lin, torch.randn(2, 16, 8, 8, generator=g).to(DEV), torch.randn(2, 16, generator=g).to(DEV)


def _fresh_caches(*modules):
    for m in modules:
        m._packed = {}


def test_a_flat_buffer_registered_again_is_followed(precision):
    conv, lin, x, xl = _modules()
    opt = OPT.FlatAdam(list(conv.parameters()) + list(lin.parameters()), lr=1e-2)
    opt.zero_grad()
    yc, yl = conv(x), lin(xl)
    first = (yc.detach().clone(), yl.detach().clone())
    (yc.sum() + yl.sum()).backward()
    HF.unregister_flat(opt.flat)
    HF.register_flat(opt.flat)
    opt.step()
    with torch.no_grad():
        second = (conv(x), lin(xl))
        _fresh_caches(conv, lin)
        want = (conv(x), lin(xl))
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, want):
        assert torch.equal(b, c), "stale packed weights after the re-registration"
        assert not torch.equal(a, b)


def test_two_buffers_do_not_stale_each_other(precision, monkeypatch):
    conv, lin, x, xl = _modules()
    opt_c, opt_l = OPT.FlatAdam(conv.parameters(), lr=1e-2), OPT.FlatAdam(lin.parameters(), lr=1e-2)
    opt_c.zero_grad(), opt_l.zero_grad()
    (conv(x).sum() + lin(xl).sum()).backward()
    calls, real_call = [], L.call
    monkeypatch.setattr(L, "call", lambda name, *args: (calls.append(name), real_call(name, *args))[1])

    def packs():
        out = [n for n in calls if n in PACKS]
        calls.clear()
        return out

    with torch.no_grad():
        for opt, module, inp, other, other_inp in ((opt_c, conv, x, lin, xl), (opt_l, lin, xl, conv, x)):
            opt.step()
            packs()
            y_other = other(other_inp)
            assert packs() == [], "the other optimiser's step re-packed this module's weights"
            y = module(inp)
            assert len(packs()) == 1
            _fresh_caches(conv, lin)
            want, want_other = module(inp), other(other_inp)
            packs()
            torch.cuda.synchronize()
            assert torch.equal(y, want) and torch.equal(y_other, want_other)


@pytest.mark.parametrize("how", ["capture", "capture_segments"])
def test_the_live_generator_is_fresh_after_every_replay(how):
    step, d = _setup()
    graphed = getattr(step, how)(d["words"], d["sent"], d["lens"], d["reals"], warmup=1)
    kw = dict(noise=d["noise"], eps=d["eps"])
    graphed.replay()
    s1 = [x.clone() for x in step.generate_images(d["words"], d["sent"], d["lens"], **kw)]
    graphed.replay()
    s2 = step.generate_images(d["words"], d["sent"], d["lens"], **kw)
    torch.manual_seed(99)
    fresh = GEN.Generator(GF, EMB, Z, COND).to(DEV)
    fresh.load_state_dict(step.state_dict()["generator"])
    fresh.eval()
    mask = step._make_mask(d["lens"], T)
    want = step._denormalise_multiple(TR.sample_fakes(fresh, d["words"], d["sent"], mask, step.sample_rng, d["noise"], d["eps"]))
    torch.cuda.synchronize()
    assert len(s1) == len(s2) == len(want) == 3
    for a, b, c in zip(s1, s2, want):
        assert torch.equal(b, c), "the sample after the second replay ran on packs of older weights"
        assert not torch.equal(a, b)
