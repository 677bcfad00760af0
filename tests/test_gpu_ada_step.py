"""GanTrainStep(augment=..., augment_p=..., ada_target=...) at the tiny configuration of tests/test_gpu_diffaug_step.py (gf = df = 8,
B = 4, T = 10), restated here.  ada_interval = 2 and ada_kimg = 0.08 make a window of 2 steps * 3 discriminators * 4 real images move
p by 24 / (0.08 * 1000 * 3) = 0.1, so p moves within six steps.

The three run modes agree bit for bit (losses, flat parameters, the controller's six words), p follows augment.ada_reference fed
the step's own real scores, a step equals the step on the gated torch oracle, a checkpoint resumes bit for bit with p, and
augment_p = 1 is the step with `augment` alone.

Measured on MI355X (test_step_equals_the_step_on_the_gated_torch_oracle prints every figure): losses within 2.1e-6 relative of the
oracle step, the four flat gradients within 7.8e-7 norm-relative; p went 0.3, 0.3, 0.3, 0.4, 0.4, 0.5 over the six steps."""
import copy
import importlib

import pytest
import torch

from helpers import RTOL

pytestmark = pytest.mark.gpu

A = importlib.import_module("attention-gan_amd.augment")
HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

DEV = torch.device("cuda", 0)
POLICY = "color,translation,cutout"
GF, DF, EMB, Z, COND, B, T = 8, 8, 32, 16, 16, 4, 10
ADA = dict(augment_p=0.3, ada_target=0.0, ada_interval=2, ada_kimg=0.08)
STEPS = 6


def _setup(seed=3, **kw):
    torch.manual_seed(seed)
    G = GEN.Generator(GF, EMB, Z, COND).to(DEV)
    Ds = [DISC.Disc64(DF).to(DEV), DISC.Disc128(DF).to(DEV), DISC.Disc256(DF).to(DEV)]
    enc = ENC.StandInImageEncoder(EMB).to(DEV)
    enc.freeze_all_weights()
    g = torch.Generator().manual_seed(seed)
    d = dict(words=torch.randn(B, EMB, T, generator=g).to(DEV), sent=torch.randn(B, EMB, generator=g).to(DEV),
             lens=torch.tensor([10, 3, 2, 7], dtype=torch.int64, device=DEV),
             reals=[(torch.rand(B, 3, r, r, generator=g) * 2 - 1).to(DEV) for r in (64, 128, 256)],
             noise=torch.randn(B, Z, generator=g).to(DEV), eps=torch.randn(B, COND, generator=g).to(DEV),
             aug_u=torch.rand(9, B, 8, generator=g).to(DEV), aug_q=torch.rand(9, B, 4, generator=g).to(DEV))
    step = TR.GanTrainStep(G, Ds, enc, seed=seed, augment=POLICY, **kw)
    return step, d


def _scalars(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() == 0}


def _flats(step):
    return [o.flat.clone() for o in [step.g_opt] + step.d_opts]


_EAGER = {}


def _eager_run():
    """six eager steps with adaptation, taken once: final losses, flats and state words, p after every step, and every real score"""
    if not _EAGER:
        step, d = _setup(**ADA)
        scores, ps = [], []
        step.on_real_scores = lambda i, s: scores.append((i, s.clone()))
        for _ in range(STEPS):
            out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
            assert out["ada_p"].data_ptr() == step.ada.p.data_ptr()          # the live view
            ps.append(out["ada_p"].clone())
        torch.cuda.synchronize()
        _EAGER.update(scalars=_scalars(out), flats=_flats(step), words=step.ada.state[:6].clone(), ps=[float(p) for p in ps],
                      scores=[(i, s.cpu()) for i, s in scores], rate=step.ada.rate, sync=step.ada.sync())
    return _EAGER


@pytest.mark.parametrize("mode", ["graph", "segments"])
def test_eager_graph_and_segments_agree_bit_for_bit(mode):
    """noise, eps, the uniforms and the gates are drawn INSIDE each form from equally seeded generators, p and the controller's
    window live in device memory: 1 warm-up step + 5 replays against 6 eager steps"""
    want = _eager_run()
    step, d = _setup(**ADA)
    graphed = (step.capture if mode == "graph" else step.capture_segments)(d["words"], d["sent"], d["lens"], d["reals"], warmup=1)
    for _ in range(STEPS - 1):
        out = graphed.replay()
    torch.cuda.synchronize()
    got = _scalars(out)
    assert set(got) == set(want["scalars"]) and "ada_p" not in got           # (ada_p is a one-element view, not a 0-dim loss)
    for k in want["scalars"]:
        assert torch.equal(got[k], want["scalars"][k]), f"{mode}: loss {k}"
    for i, (a, b) in enumerate(zip(_flats(step), want["flats"])):
        assert torch.equal(a, b), f"{mode}: flat parameter buffer {i}"
    assert torch.equal(step.ada.state[:6], want["words"]), f"{mode}: {step.ada.state[:6].tolist()} vs {want['words'].tolist()}"
    assert torch.equal(out["ada_p"].view(torch.int32), want["words"][4:5])
    assert step.ada.sync() == want["sync"]


def test_p_follows_the_reference_fed_the_steps_own_real_scores():
    run = _eager_run()
    assert len(run["scores"]) == 3 * STEPS and all(s.numel() == B for _, s in run["scores"])
    ref = A.ada_new_state(ADA["augment_p"])
    assert run["rate"] == 1.0 / (ADA["ada_kimg"] * 1000.0 * 3)
    trajectory = []
    for k in range(STEPS):
        slots = [None] * 3
        for i, s in run["scores"][3 * k:3 * k + 3]:
            assert slots[i] is None
            slots[i] = A.ada_tally(s)
        A.ada_reference(ref, slots, ADA["ada_interval"], ADA["ada_target"], run["rate"], 1.0)
        trajectory.append(ref["p"])
    print("p after each step:", run["ps"], "r_t at the end:", ref["r_t"])
    assert run["ps"] == trajectory
    assert len(set(trajectory)) > 1, "p never moved: the test checks nothing"
    assert run["sync"] == {"p": ref["p"], "r_t": ref["r_t"], "adjustments": ref["adjustments"]}
    assert run["words"].tolist()[:4] == [ref["sum"], ref["count"], ref["calls"], ref["adjustments"]]


def test_step_equals_the_step_on_the_gated_torch_oracle(monkeypatch):
    def run(oracle):
        step, d = _setup(augment_p=0.5)
        grads = {}
        step.on_gradients = lambda tag, opt: grads.__setitem__(tag, opt.grad.clone())
        if oracle:
            def reference(xs, u, policy, q=None, p=None):
                assert q is not None and p is step.ada.p
                x = xs if isinstance(xs, torch.Tensor) else torch.cat(list(xs), dim=0)
                return A.diffaug_reference(x.float(), u, policy, q, p)
            monkeypatch.setattr(HF, "diffaug", reference)
        out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"], d["aug_u"], d["aug_q"])
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert "ada_p" not in out and "ada" not in step.state_dict()       # a fixed probability: no controller, no checkpoint key
        return _scalars(out), grads, d
    got, got_grads, d = run(False)
    want, want_grads, _ = run(True)
    gates = A.gate_masks(d["aug_q"].reshape(-1, 4), 0.5)
    assert bool(gates.any()) and not bool(gates.all())                       # some stages ran and some did not
    assert set(got_grads) == {"D0", "D1", "D2", "G"} == set(want_grads)
    worst_loss = worst_grad = 0.0
    for k in want:
        err = abs(float(got[k]) - float(want[k])) / max(abs(float(want[k])), 1e-30)
        worst_loss = max(worst_loss, err)
        print(f"loss {k}: {float(got[k]):.6f} vs oracle {float(want[k]):.6f} (rel {err:.2e})")
        assert err <= RTOL, k
    for tag in want_grads:
        err = float((got_grads[tag].double() - want_grads[tag].double()).norm() / want_grads[tag].double().norm())
        worst_grad = max(worst_grad, err)
        print(f"gradient {tag}: norm-relative error {err:.2e}")
        assert err <= RTOL, tag
    print(f"gated step vs oracle: worst loss error {worst_loss:.2e}, worst gradient error {worst_grad:.2e}")


def test_checkpoint_resumes_the_adaptive_run():
    a, d = _setup(**ADA)
    for _ in range(3):                                                      # an odd count: the checkpoint is taken inside a window
        a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    ckpt = copy.deepcopy(a.state_dict())
    assert sorted(ckpt["ada"]) == sorted(A.ADA_WORDS) and ckpt["ada"]["calls"] == 1 and ckpt["ada"]["adjustments"] == 1
    b, _ = _setup(seed=77, **ADA)
    b.load_state_dict(ckpt)
    assert torch.equal(a.ada.state, b.ada.state)
    for _ in range(2):
        out_a = a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        out_b = b.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    sa, sb = _scalars(out_a), _scalars(out_b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for i, (fa, fb) in enumerate(zip(_flats(a), _flats(b))):
        assert torch.equal(fa, fb), f"flat parameter buffer {i}"
    assert torch.equal(a.ada.state, b.ada.state) and a.ada.sync()["adjustments"] == 2
    # a checkpoint without the key: p goes back to its initial value
    del ckpt["ada"]
    b.load_state_dict(ckpt)
    assert b.ada.sync() == {"p": float(torch.tensor(ADA["augment_p"], dtype=torch.float32)), "r_t": 0.0, "adjustments": 0}


def test_probability_one_is_the_step_with_the_policy_alone():
    def run(**kw):
        step, d = _setup(**kw)
        grads = {}
        step.on_gradients = lambda tag, opt: grads.__setitem__(tag, opt.grad.clone())
        extra = (d["aug_q"],) if kw else ()
        out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"], d["aug_u"], *extra)
        torch.cuda.synchronize()
        return _scalars(out), grads, step, d
    want, want_grads, plain, d = run()
    got, got_grads, gated, _ = run(augment_p=1.0)
    assert set(got_grads) == {"D0", "D1", "D2", "G"} == set(want_grads)
    for tag in want_grads:
        assert torch.equal(got_grads[tag], want_grads[tag]), tag
    for k in want:
        assert torch.equal(got[k], want[k]), k
    # the gates are one more draw of 3 * len(Ds) * B * 4 numbers right after aug_u, and none without a probability
    plain.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    gated.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    assert not torch.equal(plain.rng.get_state(), gated.rng.get_state())
    torch.rand(9, B, 4, device=DEV, generator=plain.rng)
    assert torch.equal(plain.rng.get_state(), gated.rng.get_state())
    with pytest.raises(ValueError):
        gated.step(d["words"], d["sent"], d["lens"], None, d["reals"], aug_q=d["aug_q"][:3])
