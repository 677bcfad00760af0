"""GanTrainStep(word_disc=WordLevelDisc(...)) at the tiny configuration of tests/test_gpu_cond_step.py (gf = df = 8, EMB 32, B = 4,
T = 10, StandInImageEncoder), restated here.

The three run modes agree bit for bit (every scalar result, every flat buffer, the word-level discriminator's included), a checkpoint
resumes bit for bit and one without the new keys loads, a step on the kernels equals the step with functional.word_corr replaced by its
fp32 torch statement within the project's 1e-3 -- plain, and with conditional + augment + geometry + ada_target -- the perception layer
moves, and with word_disc=None (the default) nothing new appears anywhere.

Measured on MI355X (test_step_equals_the_step_on_the_torch_reference prints every figure): see that test's docstring."""
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


def _setup(seed=3, word=True, conditional=False, **kw):
    torch.manual_seed(seed)
    G = GEN.Generator(GF, EMB, Z, COND).to(DEV)
    cd = EMB if conditional else None
    Ds = [DISC.Disc64(DF, cond_dim=cd).to(DEV), DISC.Disc128(DF, cond_dim=cd).to(DEV), DISC.Disc256(DF, cond_dim=cd).to(DEV)]
    enc = ENC.StandInImageEncoder(EMB).to(DEV)
    enc.freeze_all_weights()
    g = torch.Generator().manual_seed(seed)
    d = dict(words=torch.randn(B, EMB, T, generator=g).to(DEV), sent=torch.randn(B, EMB, generator=g).to(DEV),
             lens=torch.tensor([10, 3, 2, 7], dtype=torch.int64, device=DEV),
             reals=[(torch.rand(B, 3, r, r, generator=g) * 2 - 1).to(DEV) for r in (64, 128, 256)],
             noise=torch.randn(B, Z, generator=g).to(DEV), eps=torch.randn(B, COND, generator=g).to(DEV),
             aug_u=torch.rand(9, B, 8, generator=g).to(DEV), aug_q=torch.rand(9, B, 4, generator=g).to(DEV),
             aug_g=torch.rand(9, B, 16, generator=g).to(DEV))
    if word:
        kw["word_disc"] = DISC.WordLevelDisc(EMB).to(DEV)
    step = TR.GanTrainStep(G, Ds, enc, seed=seed, conditional=conditional, **kw)
    return step, d


def _scalars(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() == 0}


def _flats(step):
    return [o.flat.clone() for o in [step.g_opt] + step.d_opts + ([step.w_opt] if step.w_opt is not None else [])]


_EAGER = {}


def _eager_run():
    """STEPS eager steps, taken once: final losses and flats"""
    if not _EAGER:
        step, d = _setup()
        for _ in range(STEPS):
            out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        torch.cuda.synchronize()
        _EAGER.update(scalars=_scalars(out), flats=_flats(step))
    return _EAGER


@pytest.mark.parametrize("mode", ["graph", "segments"])
def test_eager_graph_and_segments_agree_bit_for_bit(mode):
    """1 warm-up step + STEPS - 1 replays against STEPS eager steps"""
    want = _eager_run()
    assert {"dw_loss", "gw_loss"} <= set(want["scalars"]) and len(want["flats"]) == 5
    step, d = _setup()
    graphed = (step.capture if mode == "graph" else step.capture_segments)(d["words"], d["sent"], d["lens"], d["reals"], warmup=1)
    if mode == "segments":
        assert graphed.dw_backward is not None and graphed.dw_adam is not None      # the two extra graphs
    for _ in range(STEPS - 1):
        out = graphed.replay()
    torch.cuda.synchronize()
    got = _scalars(out)
    assert set(got) == set(want["scalars"])
    for k in want["scalars"]:
        assert torch.equal(got[k], want["scalars"][k]), f"{mode}: loss {k}"
    for i, (a, b) in enumerate(zip(_flats(step), want["flats"])):
        assert torch.equal(a, b), f"{mode}: flat parameter buffer {i}"
    # the perception layer trained: it has left the identity it started from
    w = step.word_disc.perception.weight.detach().view(EMB, EMB)
    assert float((w - torch.eye(EMB, device=DEV)).abs().max()) > 0
    assert step.w_opt.sync_step_count() == STEPS


def test_checkpoint_resumes_bit_for_bit_and_old_checkpoints_load():
    a, d = _setup()
    for _ in range(2):
        a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    ckpt = copy.deepcopy(a.state_dict())
    assert list(ckpt["word_disc"]) == ["perception.weight"] and "state" in ckpt["word_optim"]
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
    assert torch.equal(a.rng.get_state(), b.rng.get_state())
    # a checkpoint written without the module: everything else loads, the module stays as constructed, its optimiser is fresh
    old = {k: v for k, v in ckpt.items() if k not in ("word_disc", "word_optim")}
    c, _ = _setup(seed=78)
    c.step(d["words"], d["sent"], d["lens"], None, d["reals"])          # (so that "fresh" is not what it already was)
    before = c.word_disc.perception.weight.detach().clone()
    c.load_state_dict(old)
    assert torch.equal(c.word_disc.perception.weight.detach(), before)
    assert c.w_opt.sync_step_count() == 0 and float(c.w_opt.exp_avg.abs().max()) == 0 and float(c.w_opt.exp_avg_sq.abs().max()) == 0
    for k, v in c.G.state_dict().items():
        assert torch.equal(v.cpu(), ckpt["generator"][k].cpu()), k
    out = c.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    assert torch.isfinite(out["dw_loss"]) and torch.isfinite(out["gw_loss"])


@pytest.mark.parametrize("name", ["plain", "conditional+augment+geometry+ada"])
def test_step_equals_the_step_on_the_torch_reference(name, monkeypatch):
    """One step against the step with functional.word_corr replaced by word_corr_reference in fp32: dw_loss, gw_loss (and every other
    scalar) and the flat gradients under the tags "DW" and "G" (and the image discriminators', which the module does not touch), all
    within RTOL, norm-relative for the gradients.  Measured on MI355X, plain and augmented alike: dw_loss within 7.2e-8 of the reference
    step's, gw_loss and every other loss the same bits; the flat gradient under "DW" within 2.8e-7, under "G" within 1.5e-7, the image
    discriminators' the same bits."""
    kw = {} if name == "plain" else AUGMENTED

    def run(reference):
        step, d = _setup(**kw)
        grads, calls = {}, []
        step.on_gradients = lambda tag, opt: grads.__setitem__(tag, opt.grad.clone())
        if reference:
            def corr(regions, words, lens, shift=0, gamma1=4.0, gamma2=5.0, eps=1e-8):
                calls.append((tuple(regions.shape), int(shift)))
                return HF.word_corr_reference(regions.float(), words.float(), lens, shift, gamma1, gamma2, eps)
            monkeypatch.setattr(HF, "word_corr", corr)
        extra = (d["aug_u"], d["aug_q"], d["aug_g"]) if kw else (None, None, None)
        out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"], *extra)
        torch.cuda.synchronize()
        monkeypatch.undo()
        if reference:    # the discriminator loss: real matching, real mismatched, fake; the generator loss: fake
            shape = (B, EMB, 17, 17)
            assert sorted(calls) == sorted([(shape, 0), (shape, 1), (shape, 0), (shape, 0)])
        return _scalars(out), grads, step
    got, got_grads, step = run(False)
    want, want_grads, _ = run(True)
    assert set(got_grads) == {"D0", "D1", "D2", "DW", "G"} == set(want_grads)
    assert set(got) == set(want) and {"dw_loss", "gw_loss"} <= set(got)
    worst_loss = worst_grad = 0.0
    for k in want:
        err = abs(float(got[k]) - float(want[k])) / max(abs(float(want[k])), 1e-30)
        worst_loss = max(worst_loss, err)
        print(f"loss {k}: {float(got[k]):.6f} vs reference {float(want[k]):.6f} (rel {err:.2e})")
        assert err <= RTOL, k
    for tag in want_grads:
        err = float((got_grads[tag].double() - want_grads[tag].double()).norm() / want_grads[tag].double().norm())
        worst_grad = max(worst_grad, err)
        print(f"gradient {tag}: norm-relative error {err:.2e}")
        assert err <= RTOL, tag
    print(f"{name}: step vs reference: worst loss error {worst_loss:.2e}, worst gradient error {worst_grad:.2e}")
    assert float(got_grads["DW"].abs().max()) > 0
    if kw:
        assert step.ada is not None and step.ada.adaptive and step.geometry and step.augment and step.conditional


RESULT_KEYS = ["attn_maps", "d_loss0", "d_loss1", "d_loss2", "fake_imgs", "g_loss0", "g_loss1", "g_loss2", "g_total", "kl", "logvar",
               "mu", "s_loss", "w_loss"]
CKPT_KEYS = ["d_optims", "discriminators", "g_optim", "generator", "rng", "rng_world", "sample_rng"]


def test_default_step_has_no_word_level_entry():
    """word_disc=None: no result key, no checkpoint key, and the same bits as a trainer built without naming the argument"""
    a, d = _setup(word=False)
    assert a.word_disc is None and a.w_opt is None and a.w_buckets is None
    torch.manual_seed(3)
    G = GEN.Generator(GF, EMB, Z, COND).to(DEV)
    Ds = [DISC.Disc64(DF).to(DEV), DISC.Disc128(DF).to(DEV), DISC.Disc256(DF).to(DEV)]
    enc = ENC.StandInImageEncoder(EMB).to(DEV)
    enc.freeze_all_weights()
    b = TR.GanTrainStep(G, Ds, enc, seed=3)                             # the old way
    for _ in range(2):
        out_a = a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        out_b = b.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    assert sorted(out_a) == RESULT_KEYS == sorted(out_b)
    assert sorted(a.state_dict()) == CKPT_KEYS
    for fa, fb in zip(_flats(a), _flats(b)):
        assert torch.equal(fa, fb)
    # with the module the other results keep their names; the two new ones join them
    w, d = _setup()
    assert sorted(w.step(d["words"], d["sent"], d["lens"], None, d["reals"])) == sorted(RESULT_KEYS + ["dw_loss", "gw_loss"])
    assert sorted(w.state_dict()) == sorted(CKPT_KEYS + ["word_disc", "word_optim"])
