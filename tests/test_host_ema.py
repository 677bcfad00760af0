"""Host side of the averaged generator (GanTrainStep(ema=...), optim.FlatEMA) on CPU modules at the golden tiny size
(gf = df = 8, EMB 32, Z 16, COND 16): off means absent, the shadow's layout and mode, the checkpoint, the refusals, and the
float64 oracle of one update against a hand-written loop.  No kernel runs here."""
import copy
import importlib

import numpy as np
import pytest
import torch

HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
OPT = importlib.import_module("attention-gan_amd.optim")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

GF, DF, EMB, Z, COND = 8, 8, 32, 16, 16
TODAYS_KEYS = {"generator", "discriminators", "g_optim", "d_optims", "rng", "sample_rng", "rng_world"}


def _step(seed=5, **kw):
    torch.manual_seed(seed)
    G = GEN.Generator(GF, EMB, Z, COND)
    Ds = [DISC.Disc64(DF), DISC.Disc128(DF), DISC.Disc256(DF)]
    return TR.GanTrainStep(G, Ds, None, seed=seed, **kw)


def _same(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_off_means_absent():
    for step in (_step(), _step(ema=None)):
        assert step.G_ema is None and step.g_ema is None
        assert set(step.state_dict()) == TODAYS_KEYS


@pytest.mark.parametrize("decay", [0, 1, -0.1])
def test_decay_outside_the_open_interval_is_refused(decay):
    with pytest.raises(ValueError):
        _step(ema=decay)


def test_shadow_layout_and_mode():
    step = _step(ema=0.9)
    ema, shadow = step.g_ema, step.G_ema
    assert ema.offsets == step.g_opt.offsets and ema.numel == step.g_opt.numel
    base = ema.flat.data_ptr()
    for p, o in zip(ema.params, ema.offsets):
        assert p.data_ptr() == base + 4 * o
    assert not any(p.requires_grad for p in shadow.parameters())
    assert all(p.grad is None for p in shadow.parameters())
    assert not shadow.training
    assert shadow.train() is shadow and not any(m.training for m in shadow.modules())
    assert isinstance(shadow, GEN.Generator)
    # own storage, equal values
    lo, hi = step.g_opt.flat.data_ptr(), step.g_opt.flat.data_ptr() + 4 * step.g_opt.numel
    assert not any(lo <= p.data_ptr() < hi for p in shadow.parameters())
    live_buffers = {b.data_ptr() for b in step.G.buffers()}
    assert not any(b.data_ptr() in live_buffers for b in shadow.buffers())
    assert torch.equal(ema.flat, step.g_opt.flat)
    assert _same(shadow.state_dict(), step.G.state_dict())
    assert step.G.training                                   # the live generator's mode is its own


def test_shadow_with_other_parameters_is_refused():
    torch.manual_seed(0)
    G = GEN.Generator(GF, EMB, Z, COND)
    opt = OPT.FlatAdam(G.parameters())
    with pytest.raises(ValueError):
        OPT.FlatEMA(G, GEN.Generator(GF * 2, EMB, Z, COND), opt, 0.9)          # shapes differ
    with pytest.raises(ValueError):
        OPT.FlatEMA(G, DISC.Disc64(DF), opt, 0.9)                              # names differ
    with pytest.raises(ValueError):
        OPT.FlatEMA(G, GEN.Generator(GF, EMB, Z, COND).double(), opt, 0.9)     # not float32
    with pytest.raises(ValueError):
        OPT.FlatEMA(G, GEN.Generator(GF, EMB, Z, COND), opt, 1.0)


def test_checkpoint_round_trip_keeps_the_average():
    a = _step(ema=0.9)
    with torch.no_grad():                                    # make the shadow differ from the live generator
        a.g_ema.flat.mul_(0.5)
        for b in a.G_ema.buffers():
            if b.is_floating_point():
                b.add_(0.25)
        for b in a.G.buffers():
            if not b.is_floating_point():
                b.fill_(7)
        a.g_ema.state[0] = 3
    sd = copy.deepcopy(a.state_dict())
    assert set(sd) == TODAYS_KEYS | {"generator_ema", "ema"}
    assert sd["ema"] == {"decay": 0.9, "warmup": True, "updates": 3}
    assert set(sd["generator_ema"]) == set(sd["generator"])
    assert all(int(v) == 7 for k, v in sd["generator_ema"].items() if k.endswith("num_batches_tracked"))    # integer buffers: the live ones
    b = _step(seed=9, ema=0.5, ema_warmup=False)
    b.load_state_dict(sd)
    assert _same(b.G_ema.state_dict(), sd["generator_ema"]) and _same(b.G.state_dict(), sd["generator"])
    assert not torch.equal(b.g_ema.flat, b.g_opt.flat)
    assert b.g_ema.sync_updates() == 3 and int(b.g_ema.state[0]) == 3
    assert (b.g_ema.decay, b.g_ema.warmup) == (0.5, False)   # configuration: the constructor's values hold
    again = b.state_dict()
    assert _same(again["generator_ema"], sd["generator_ema"]) and again["ema"]["updates"] == 3


def test_checkpoint_without_the_average_restarts_it_from_the_loaded_generator():
    old = copy.deepcopy(_step(seed=11).state_dict())                           # a run without `ema`: today's keys only
    b = _step(seed=9, ema=0.9)
    with torch.no_grad():
        b.g_ema.state[0] = 4
    assert not torch.equal(b.g_ema.flat, _step(seed=11).g_opt.flat)
    b.load_state_dict(old)
    assert _same(b.G_ema.state_dict(), old["generator"])
    assert torch.equal(b.g_ema.flat, b.g_opt.flat)
    assert b.g_ema.sync_updates() == 0 and int(b.g_ema.state[0]) == 0


def test_use_ema_flags():
    words, sent = torch.zeros(2, EMB, 5), torch.zeros(2, EMB)
    with pytest.raises(ValueError):
        _step().generate_images(words, sent, [5, 3], use_ema=True)
    with pytest.raises(ValueError):
        _step().evaluate([], None, None, 4, use_ema=True)
    with pytest.raises(ValueError):
        _step(ema=0.9).generate_images(words, sent, [5, 3], use_ema=True, train_mode_bn=True)
    with pytest.raises(RuntimeError):
        _step(ema=0.9).g_ema.update()                        # no CPU fallback


def test_segment_plan_is_checked_on_the_host():
    L = HF.L
    table, nseg, total = HF.ema_table([(1 << 20, 2 << 20, 1), (3 << 20, 4 << 20, 4097), ((5 << 20) + 4, 6 << 20, (1 << 20) + 4)], "cpu")
    segs = table.numpy().view(HF._EMA_SEG_DTYPE)
    assert nseg == 3 and list(segs["first_block"]) == [0, 1, 1 + 5] and total == 6 + 1025
    assert list(segs["n"]) == [1, 4097, (1 << 20) + 4]
    for bad in ([], [(1 << 20, 2 << 20, 0)], [(0, 2 << 20, 8)], [(1 << 20, 0, 8)], [(1 << 20, (2 << 20) + 2, 8)]):
        with pytest.raises(L.AganError):
            HF.ema_table(bad, "cpu")
    lib = L.load()
    assert lib.agan_ema_update(None, 1, 1, None, 0.9, 1, None) == L.EINVAL and b"ema_update" in lib.agan_last_error()


@pytest.mark.parametrize("warmup", [True, False])
def test_reference_is_the_recurrence(warmup):
    decay = 0.9
    g = torch.Generator().manual_seed(1)
    dst = torch.randn(37, generator=g)
    want = [float(v) for v in dst]
    got = dst.double()
    for t in range(21):
        src = torch.randn(37, generator=g)
        beta = min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay
        omb = float(np.float32(1.0 - beta))
        want = [d + omb * (float(s) - d) for s, d in zip(src, want)]
        got = HF.ema_reference(src, got, t, decay, warmup)
        assert got.dtype == torch.float64
        assert torch.equal(got, torch.tensor(want, dtype=torch.float64)), t
    assert not torch.equal(got, dst.double())


def test_beta_rule():
    assert HF.ema_beta(0, 0.9) == 0.1 and HF.ema_beta(0, 0.9, warmup=False) == 0.9
    for decay in (0.5, 0.9, 0.999):
        first = next(t for t in range(100000) if (1.0 + t) / (10.0 + t) > decay)
        assert all(HF.ema_beta(t, decay) == (1.0 + t) / (10.0 + t) <= decay for t in range(max(0, first - 50), first))
        assert all(HF.ema_beta(t, decay) == decay for t in range(first, first + 50))
    assert HF.ema_beta(79, 0.9) == 80.0 / 89.0 and HF.ema_beta(81, 0.9) == 0.9          # 82 / 91 is the first ratio above 0.9


def test_segment_table_follows_reallocated_buffers():
    step = _step(ema=0.9)
    ema = step.g_ema
    table, nseg, total = ema._segments()
    assert nseg == 1 + sum(b.is_floating_point() for b in step.G.buffers()) and ema._segments()[0] is table       # built once
    bn = next(m for m in step.G.modules() if "running_mean" in m._buffers)
    bn.running_mean = bn.running_mean.clone()                # what a .to() does to a buffer
    again = ema._segments()
    assert again[0] is not table and again[1:] == (nseg, total)
    bn.running_mean = bn.running_mean.double()
    with pytest.raises(ValueError):
        ema._segments()
