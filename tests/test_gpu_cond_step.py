"""GanTrainStep(conditional=True) at the tiny configuration of tests/test_gpu_geoaug_step.py (gf = df = 8, B = 4, T = 10), restated
here, with discriminators built with cond_dim = the sentence embedding's width.

The three run modes agree bit for bit (losses, flat parameters), a checkpoint resumes bit for bit, a step on the kernels equals the
step with functional.cond_join and functional.cond_disc_loss replaced by their fp32 torch statements within the project's 1e-3 --
plain, and with augment + geometry + ada_target -- and with conditional=False (the default) no module, key or result appears.

Measured on MI355X (test_step_equals_the_step_on_the_torch_oracle prints every figure): see that test's docstring."""
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
AUGMENTED = dict(geometry=GEOMETRY, augment=POLICY, augment_p=0.6, ada_target=0.0, ada_interval=2, ada_kimg=0.08)
STEPS = 4


def _setup(seed=3, conditional=True, **kw):
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
    step = TR.GanTrainStep(G, Ds, enc, seed=seed, conditional=conditional, **kw)
    return step, d


def _scalars(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() == 0}


def _flats(step):
    return [o.flat.clone() for o in [step.g_opt] + step.d_opts]


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
    # the head trained: its BatchNorm counted 4 calls per step (real, fake, wrong; fake again in the generator update)
    for D in step.Ds:
        assert int(D.state_dict()["COND_DNET.jointConv.1.num_batches_tracked"]) == 4 * STEPS


def test_checkpoint_resumes_bit_for_bit():
    a, d = _setup()
    for _ in range(2):
        a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    ckpt = copy.deepcopy(a.state_dict())
    assert "conditional" not in ckpt                                    # the head lives in the discriminators' entries: nothing new
    assert all("COND_DNET.jointConv.0.weight" in sd for sd in ckpt["discriminators"])
    b, _ = _setup(seed=77)
    b.load_state_dict(ckpt)
    for _ in range(2):
        out_a = a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        out_b = b.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    sa, sb = _scalars(out_a), _scalars(out_b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for i, (fa, fb) in enumerate(zip(_flats(a), _flats(b))):
        assert torch.equal(fa, fb), f"flat parameter buffer {i}"
    assert torch.equal(a.rng.get_state(), b.rng.get_state())


@pytest.mark.parametrize("name", ["plain", "augment+geometry+ada"])
def test_step_equals_the_step_on_the_torch_oracle(name, monkeypatch):
    """Measured on MI355X, plain and augmented alike: the discriminator losses within 8.8e-8 of the oracle step's and every other loss
    the same bits; the discriminators' flat gradients within 4.1e-8 norm-relative, the generator's within 1.7e-7 (the join's forward is
    the fp32 statement's bits; its backward and the loss kernel sum in another order)."""
    kw = {} if name == "plain" else AUGMENTED

    def run(oracle):
        step, d = _setup(**kw)
        grads, calls = {}, []
        step.on_gradients = lambda tag, opt: grads.__setitem__(tag, opt.grad.clone())
        if oracle:
            def join(yi, p, wrong=False):
                calls.append(("join", tuple(yi.shape), bool(wrong)))
                return HF.cond_join_reference(yi.float(), p.float(), wrong)

            def loss(pu, pc):
                calls.append(("loss", tuple(pu.shape), tuple(pc.shape)))
                return HF.cond_disc_loss_reference(pu, pc)
            monkeypatch.setattr(HF, "cond_join", join)
            monkeypatch.setattr(HF, "cond_disc_loss", loss)
        extra = (d["aug_u"], d["aug_q"], d["aug_g"]) if kw else (None, None, None)
        out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"], *extra)
        torch.cuda.synchronize()
        monkeypatch.undo()
        if oracle:       # per discriminator: one join over [real; fake] with wrong rows, one loss, and one join over the fakes
            c = 8 * DF
            assert sorted(calls) == sorted(3 * [("join", (2 * B, c, 4, 4), True), ("join", (B, c, 4, 4), False), ("loss", (2 * B,), (3 * B,))])
        return _scalars(out), grads, step
    got, got_grads, step = run(False)
    want, want_grads, _ = run(True)
    assert set(got_grads) == {"D0", "D1", "D2", "G"} == set(want_grads)
    assert set(got) == set(want)
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
    print(f"{name}: step vs oracle: worst loss error {worst_loss:.2e}, worst gradient error {worst_grad:.2e}")
    if kw:
        assert step.ada is not None and step.ada.adaptive and step.geometry and step.augment


def _bn(prefix):
    return [f"{prefix}.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]


S16 = (["img_code_s16.0.weight", "img_code_s16.2.weight"] + _bn("img_code_s16.3") + ["img_code_s16.5.weight"] + _bn("img_code_s16.6")
       + ["img_code_s16.8.weight"] + _bn("img_code_s16.9"))
HEAD = ["outlogits.0.weight", "outlogits.0.bias"]
KEYS = [S16 + HEAD,
        S16 + ["img_code_s32.0.weight"] + _bn("img_code_s32.1") + ["img_code_s32_1.0.weight"] + _bn("img_code_s32_1.1") + HEAD,
        S16 + ["img_code_s32.0.weight"] + _bn("img_code_s32.1") + ["img_code_s64.0.weight"] + _bn("img_code_s64.1")
        + ["img_code_s64_1.0.weight"] + _bn("img_code_s64_1.1") + ["img_code_s64_2.0.weight"] + _bn("img_code_s64_2.1") + HEAD]
RESULT_KEYS = ["attn_maps", "d_loss0", "d_loss1", "d_loss2", "fake_imgs", "g_loss0", "g_loss1", "g_loss2", "g_total", "kl", "logvar",
               "mu", "s_loss", "w_loss"]


def test_default_step_has_no_conditional_entry():
    step, d = _setup(conditional=False)
    assert step.conditional is False
    assert type(step.disc_loss).__name__ == "NonSaturatingDiscLoss" and type(step.gen_loss).__name__ == "NonSaturatingGenLoss"
    for D, keys in zip(step.Ds, KEYS):
        assert list(D.state_dict()) == keys
        assert D.COND_DNET is None
    fw = step._gen_forward(d["words"], d["sent"], d["lens"], d["noise"], d["eps"])
    assert fw.sent is None
    out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"])
    torch.cuda.synchronize()
    assert sorted(out) == RESULT_KEYS
    # the conditional step reports the same keys: its terms are inside d_loss* and g_loss*
    cond, d = _setup()
    assert sorted(cond.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"])) == RESULT_KEYS
    with pytest.raises(ValueError, match="conditional=True"):
        TR.GanTrainStep(step.G, step.Ds, None, conditional=True)
