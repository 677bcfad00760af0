"""GanTrainStep with discriminators built with norm="spectral", at the tiny configuration of tests/test_gpu_word_disc_step.py (gf = df = 8,
EMB 32, B = 4, T = 10, StandInImageEncoder), restated here.

The three run modes agree bit for bit over 4 steps (every scalar result, every flat buffer, every u and v), a checkpoint resumes bit for
bit and one taken from norm="batch" discriminators warm-starts, a step on the kernels equals the step with functional.spectral_weight
replaced by its torch statement within the project's 1e-3 -- plain, and with conditional + augment + geometry + ada_target -- and with the
default `norm` a trainer's results are the same bits as one built without ever naming the argument."""
import copy
import importlib

import pytest
import torch

from helpers import RTOL

pytestmark = pytest.mark.gpu

HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

DEV = torch.device("cuda", 0)
GEOMETRY = "xflip,rot90,scale,rotate,aniso"
POLICY = "color,translation,cutout"
GF, DF, EMB, Z, COND, B, T = 8, 8, 32, 16, 16, 4, 10
AUGMENTED = dict(conditional=True, geometry=GEOMETRY, augment=POLICY, augment_p=0.6, ada_target=0.0, ada_interval=2, ada_kimg=0.08)
STEPS = 4


def _setup(seed=3, norm="spectral", conditional=False, **kw):
    torch.manual_seed(seed)
    G = GEN.Generator(GF, EMB, Z, COND).to(DEV)
    cd = EMB if conditional else None
    nk = {} if norm is None else dict(norm=norm)
    Ds = [DISC.Disc64(DF, cond_dim=cd, **nk).to(DEV), DISC.Disc128(DF, cond_dim=cd, **nk).to(DEV), DISC.Disc256(DF, cond_dim=cd, **nk).to(DEV)]
    enc = ENC.StandInImageEncoder(EMB).to(DEV)
    enc.freeze_all_weights()
    g = torch.Generator().manual_seed(seed)
    d = dict(words=torch.randn(B, EMB, T, generator=g).to(DEV), sent=torch.randn(B, EMB, generator=g).to(DEV),
             lens=torch.tensor([10, 3, 2, 7], dtype=torch.int64, device=DEV),
             reals=[(torch.rand(B, 3, r, r, generator=g) * 2 - 1).to(DEV) for r in (64, 128, 256)],
             noise=torch.randn(B, Z, generator=g).to(DEV), eps=torch.randn(B, COND, generator=g).to(DEV),
             aug_u=torch.rand(9, B, 8, generator=g).to(DEV), aug_q=torch.rand(9, B, 4, generator=g).to(DEV),
             aug_g=torch.rand(9, B, 16, generator=g).to(DEV))
    step = TR.GanTrainStep(G, Ds, enc, seed=seed, conditional=conditional, **kw)
    return step, d


def _scalars(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() == 0}


def _flats(step):
    return [o.flat.clone() for o in [step.g_opt] + step.d_opts]


def _states(step):
    """every u and v of the three discriminators"""
    return {f"D{i}.{k}": v.clone() for i, D in enumerate(step.Ds) for k, v in D.state_dict().items() if k.endswith(("_u", "_v"))}


_EAGER = {}


def _eager_run():
    if not _EAGER:
        step, d = _setup()
        first = _states(step)
        for _ in range(STEPS):
            out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        torch.cuda.synchronize()
        _EAGER.update(scalars=_scalars(out), flats=_flats(step), states=_states(step), first=first)
    return _EAGER


@pytest.mark.parametrize("mode", ["graph", "segments"])
def test_eager_graph_and_segments_agree_bit_for_bit(mode):
    """1 warm-up step + STEPS - 1 replays against STEPS eager steps"""
    want = _eager_run()
    assert len(want["states"]) == 2 * (5 + 7 + 9) and all(torch.isfinite(v).all() for v in want["scalars"].values())
    # the iteration ran (the u of a one-row logit head is +-1 and stays)
    assert all(not torch.equal(v, want["first"][k]) for k, v in want["states"].items() if v.numel() > 1)
    step, d = _setup()
    graphed = (step.capture if mode == "graph" else step.capture_segments)(d["words"], d["sent"], d["lens"], d["reals"], warmup=1)
    for _ in range(STEPS - 1):
        out = graphed.replay()
    torch.cuda.synchronize()
    got = _scalars(out)
    assert set(got) == set(want["scalars"])
    for k in want["scalars"]:
        assert torch.equal(got[k], want["scalars"][k]), f"{mode}: loss {k}"
    for i, (a, b) in enumerate(zip(_flats(step), want["flats"])):
        assert torch.equal(a, b), f"{mode}: flat parameter buffer {i}"
    got_states = _states(step)
    for k, v in want["states"].items():
        assert torch.equal(got_states[k], v), f"{mode}: {k}"


def test_checkpoint_resumes_bit_for_bit_and_a_batch_checkpoint_warm_starts():
    a, d = _setup()
    for _ in range(2):
        a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    ckpt = copy.deepcopy(a.state_dict())
    assert not [k for ds in ckpt["discriminators"] for k in ds if "running" in k]
    assert all(any(k.endswith("weight_u") for k in ds) for ds in ckpt["discriminators"])
    b, _ = _setup(seed=77)
    b.load_state_dict(ckpt)
    for _ in range(2):
        out_a = a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        out_b = b.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    sa, sb = _scalars(out_a), _scalars(out_b)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for i, (fa, fb) in enumerate(zip(_flats(a), _flats(b))):
        assert torch.equal(fa, fb), f"flat parameter buffer {i}"
    for (k, va), vb in zip(_states(a).items(), _states(b).values()):
        assert torch.equal(va, vb), k
    # a checkpoint of norm="batch" discriminators: BatchNorm entries ignored, every conv weight and bias loaded, u and v as they were,
    # the discriminators' optimisers fresh
    old, _ = _setup(seed=5, norm="batch")
    old.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    old_ckpt = copy.deepcopy(old.state_dict())
    assert any("running_mean" in k for k in old_ckpt["discriminators"][2])
    c, _ = _setup(seed=78)
    c.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    before = _states(c)
    c.load_state_dict(old_ckpt)
    for i, (D, ds) in enumerate(zip(c.Ds, old_ckpt["discriminators"])):
        sd = D.state_dict()
        for k, v in sd.items():
            if k.endswith("_orig"):
                assert torch.equal(v, ds[k[:-5]]), k
            elif k.endswith(("_u", "_v")):
                assert torch.equal(v, before[f"D{i}.{k}"]), k
            else:
                assert torch.equal(v, ds[k]), k
        o = c.d_opts[i]
        assert o.sync_step_count() == 0 and float(o.exp_avg.abs().max()) == 0 and float(o.exp_avg_sq.abs().max()) == 0
    out = c.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    assert all(torch.isfinite(out[k]) for k in ("d_loss0", "d_loss1", "d_loss2", "g_total"))


@pytest.mark.parametrize("name", ["plain", "conditional+augment+geometry+ada"])
def test_step_equals_the_step_on_the_torch_reference(name, monkeypatch):
    """Two steps against the steps with functional.spectral_weight replaced by spectral_weight_reference in fp32: every scalar and the flat
    gradients under every tag within RTOL (norm-relative for the gradients), and every u and v afterwards.

    Measured on an MI355X: every loss within 2e-6 and the flat gradients within 3e-7 .. 3.4e-6, except "D2" (Disc256), 6.7e-4 plain and
    9.7e-5 augmented.  Both sides are fp32 here and differ only in how sigma is summed, so a pre-activation of Disc256 within rounding of
    the LeakyReLU kink takes one slope with the kernels and the other with the reference (tests/test_gpu_spectral_module.py's docstring;
    one element in 5 * 10^5 moves a layer's gradient by about 1.4e-3 of its norm).  The margin to RTOL is under 2 x and belongs to THIS
    seed and data: another initialisation order or batch moves which element sits at the kink, and a larger figure from "D2" alone, with
    the losses and the other tags where they are, is that and not a kernel."""
    kw = {} if name == "plain" else AUGMENTED

    def run(reference):
        step, d = _setup(**kw)
        grads, calls = {}, []
        step.on_gradients = lambda tag, opt: grads.__setitem__(tag, opt.grad.clone())
        if reference:
            def ref(weight, u, v, training, second=None):
                calls.append(tuple(weight.shape))
                return HF.spectral_weight_reference(weight, u, v, training, second)
            monkeypatch.setattr(HF, "spectral_weight", ref)
        extra = (d["aug_u"], d["aug_q"], d["aug_g"]) if kw else (None, None, None)
        for _ in range(2):
            out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"], *extra)
        torch.cuda.synchronize()
        monkeypatch.undo()
        if reference:    # every normalised layer of the three discriminators went through the replacement, equally often
            layers = (5 + 7 + 9) if not kw else (7 + 9 + 11)
            assert calls and len(calls) % layers == 0, len(calls)
        return _scalars(out), grads, step
    got, got_grads, step = run(False)
    want, want_grads, ref_step = run(True)
    assert set(got_grads) == {"D0", "D1", "D2", "G"} == set(want_grads)
    assert set(got) == set(want)
    for k in want:
        err = abs(float(got[k]) - float(want[k])) / max(abs(float(want[k])), 1e-30)
        print(f"{name}: loss {k}: {float(got[k]):.6f} vs reference {float(want[k]):.6f} (rel {err:.2e})")
        assert err <= RTOL, k
    for tag in want_grads:
        err = float((got_grads[tag].double() - want_grads[tag].double()).norm() / want_grads[tag].double().norm())
        print(f"{name}: gradient {tag}: norm-relative error {err:.2e}")
        assert err <= RTOL, tag
        assert float(got_grads[tag].abs().max()) > 0
    for (k, a), b in zip(_states(step).items(), _states(ref_step).values()):
        err = float((a.double() - b.double()).norm() / b.double().norm())
        assert err <= RTOL, k
    if kw:
        assert step.ada is not None and step.ada.adaptive and step.geometry and step.augment and step.conditional


def test_default_norm_is_the_trainer_of_before():
    """norm left alone, and norm="batch" named: the same bits, the same checkpoint keys, no spectral entry anywhere"""
    a, d = _setup(norm=None)
    b, _ = _setup(norm="batch")
    for _ in range(2):
        out_a = a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        out_b = b.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    sa, sb = _scalars(out_a), _scalars(out_b)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for fa, fb in zip(_flats(a), _flats(b)):
        assert torch.equal(fa, fb)
    assert not _states(a) and not _states(b)
    for da, db in zip(a.state_dict()["discriminators"], b.state_dict()["discriminators"]):
        assert list(da) == list(db) and any("running_mean" in k for k in da)
