"""The text-conditional discriminators (networks/discriminators.py: Disc64/128/256(df, cond_dim); losses: ConditionalDiscLoss,
ConditionalGenLoss) against AttnGAN's statement of the head, written here in float64 from the module's own state_dict: repeat the
sentence over the 4x4 map, concatenate, conv2d with the joint weight, batch_norm(training), leaky_relu(0.2), the 4x4 stride-4 conv
and sigmoid -- as three separate calls, real, fake, wrong.  df = 8, cond_dim = 32, B = 4, Disc64 on 64x64 images.

Everything is compared norm-relative within helpers.RTOL (1e-3, the project's pin).

Measured on MI355X (the tests print every figure): the figures stand in the tests' docstrings."""
import copy
import importlib

import pytest
import torch
import torch.nn.functional as F

from helpers import RTOL

pytestmark = pytest.mark.gpu

HF = importlib.import_module("attention-gan_amd.backend.functional")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
DL = importlib.import_module("attention-gan_amd.losses.disc_loss")
GL = importlib.import_module("attention-gan_amd.losses.gen_loss")

DEV = torch.device("cuda", 0)
DF, NEF, B = 8, 32, 4
F64 = torch.float64


def _nrel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).norm() / want.norm().clamp_min(1e-300))


def _setup(cls=DISC.Disc64, res=64, b=B, seed=11):
    torch.manual_seed(seed)
    D = cls(DF, cond_dim=NEF).to(DEV)
    g = torch.Generator().manual_seed(seed)
    real = (torch.rand(b, 3, res, res, generator=g) * 2 - 1).to(DEV)
    fake = (torch.rand(b, 3, res, res, generator=g) * 2 - 1).to(DEV)
    sent = torch.randn(b, NEF, generator=g).to(DEV)
    return D, real, fake, sent


# ---- AttnGAN's D_NET64 with COND_DNET in float64, from a state_dict ------------------------------------------------------------
class _Oracle:
    def __init__(self, sd):
        self.p = {k: (v.detach().double() if v.is_floating_point() else v.detach()).cpu().clone() for k, v in sd.items()}
        for k, v in self.p.items():
            if v.is_floating_point() and "running" not in k:
                v.requires_grad_(True)

    def _bn(self, x, key):
        p = self.p
        return F.batch_norm(x, p[key + ".running_mean"], p[key + ".running_var"], p[key + ".weight"], p[key + ".bias"], True, 0.1, 1e-5)

    def features(self, x):
        p = self.p
        x = F.leaky_relu(F.conv2d(x, p["img_code_s16.0.weight"], None, 2, 1), 0.2)
        for conv, bn in ((2, 3), (5, 6), (8, 9)):
            x = F.leaky_relu(self._bn(F.conv2d(x, p[f"img_code_s16.{conv}.weight"], None, 2, 1), f"img_code_s16.{bn}"), 0.2)
        return x

    def uncond(self, h):
        return torch.sigmoid(F.conv2d(h, self.p["outlogits.0.weight"], self.p["outlogits.0.bias"], 4)).view(-1)

    def cond(self, h, s):
        """COND_DNET(h_code, c_code): ONE call, one set of batch statistics"""
        p = self.p
        x = torch.cat([h, s[:, :, None, None].repeat(1, 1, 4, 4)], dim=1)
        x = F.leaky_relu(self._bn(F.conv2d(x, p["COND_DNET.jointConv.0.weight"], None, 1, 1), "COND_DNET.jointConv.1"), 0.2)
        return torch.sigmoid(F.conv2d(x, p["COND_DNET.outlogits.0.weight"], p["COND_DNET.outlogits.0.bias"], 4)).view(-1)

    def disc_loss(self, real, fake, sent):
        hr, hf = self.features(real), self.features(fake)
        pu = torch.cat([self.uncond(hr), self.uncond(hf)])
        wrong = sent[[(b + 1) % sent.shape[0] for b in range(sent.shape[0])]]
        pc = torch.cat([self.cond(hr, sent), self.cond(hf, sent), self.cond(hr, wrong)])        # real, fake, wrong
        return HF.cond_disc_loss_reference(pu, pc), pu, pc


def _module_grads(D):
    """the module's parameter gradients under the state_dict's keys: the joint weight in its concatenated shape"""
    out = {}
    jc = D.COND_DNET.jointConv
    for name, prm in D.named_parameters():
        if name.startswith("COND_DNET.jointConv.image") or name.startswith("COND_DNET.jointConv.sentence"):
            continue
        out[name] = prm.grad
    gs = jc.sentence.weight.grad.view(jc.c, 9, jc.nef).permute(0, 2, 1).reshape(jc.c, jc.nef, 3, 3)
    out["COND_DNET.jointConv.0.weight"] = torch.cat([jc.image.weight.grad, gs], dim=1)
    return out


_RUNS = {}


def _disc_run(batch_pairs):
    """one ConditionalDiscLoss backward on a fresh discriminator: loss, the scores the loss kernel was handed, gradients, buffers"""
    if batch_pairs not in _RUNS:
        D, real, fake, sent = _setup()
        before = copy.deepcopy(D.state_dict())
        crit = DL.ConditionalDiscLoss()
        crit.batch_pairs = batch_pairs
        seen, orig = {}, HF.cond_disc_loss

        def spy(pu, pc):
            seen["pu"], seen["pc"] = pu.detach().clone(), pc.detach().clone()
            return orig(pu, pc)
        HF.cond_disc_loss = spy
        try:
            loss = crit.get_loss(D, fake, real, sent, observe=lambda score: seen.__setitem__("observed", score.clone()))
        finally:
            HF.cond_disc_loss = orig
        loss.backward()
        torch.cuda.synchronize()
        _RUNS[batch_pairs] = dict(loss=loss.detach(), pu=seen["pu"], pc=seen["pc"], observed=seen["observed"], grads={k: v.clone() for k, v in _module_grads(D).items()},
                                  after=copy.deepcopy(D.state_dict()), before=before, data=(real, fake, sent))
    return _RUNS[batch_pairs]


_ORACLE = {}


def _oracle_run():
    if not _ORACLE:
        run = _disc_run(True)
        real, fake, sent = (t.double().cpu() for t in run["data"])
        O = _Oracle(run["before"])
        loss, pu, pc = O.disc_loss(real, fake, sent)
        loss.backward()
        _ORACLE.update(O=O, loss=loss.detach(), pu=pu.detach(), pc=pc.detach())
    return _ORACLE


def test_scores_statistics_and_gradients_against_attngans_statement():
    """Measured on MI355X: scores [real; fake; wrong] 8.0e-8 norm-relative (unconditional 1.4e-7), loss 7.7e-8, running mean / variance of
    jointConv.1 1.3e-7 / 3.4e-8, parameter gradients 1.6e-7 .. 1.2e-6 (the joint weight 5.8e-7)."""
    run, ora = _disc_run(True), _oracle_run()
    O = ora["O"]
    assert run["pc"].shape == (3 * B,) and run["pu"].shape == (2 * B,)
    assert torch.equal(run["observed"], run["pu"][:B])         # `observe` is handed the UNCONDITIONAL real scores
    for what, got, want in (("conditional scores [real; fake; wrong]", run["pc"], ora["pc"]), ("unconditional scores", run["pu"], ora["pu"]),
                            ("loss", run["loss"], ora["loss"])):
        e = _nrel(got, want)
        print(f"{what}: {e:.2e}")
        assert e <= RTOL, what
    # the BatchNorm of the head behaved as three calls in the order real, fake, wrong: running statistics and the counter
    key = "COND_DNET.jointConv.1"
    assert int(run["after"][key + ".num_batches_tracked"]) == int(run["before"][key + ".num_batches_tracked"]) + 3
    assert int(run["after"]["img_code_s16.3.num_batches_tracked"]) == 2
    for stat in (".running_mean", ".running_var"):
        for k in (key, "img_code_s16.9"):
            e = _nrel(run["after"][k + stat], O.p[k + stat])
            print(f"{k + stat}: {e:.2e}")
            assert e <= RTOL, k + stat
    grads = run["grads"]
    assert set(grads) == {k for k, v in O.p.items() if v.requires_grad}
    for k, g in grads.items():
        assert g.shape == O.p[k].shape, k
        e = _nrel(g, O.p[k].grad)
        print(f"gradient {k}: {e:.2e}")
        assert e <= RTOL, k
    assert tuple(grads["COND_DNET.jointConv.0.weight"].shape) == (8 * DF, 8 * DF + NEF, 3, 3)


def test_separate_passes_agree_with_the_paired_path():
    """Measured on MI355X: scores and loss the same bits, gradients within 5.8e-7 (the sums over the passes take another order)."""
    a, b = _disc_run(True), _disc_run(False)
    assert torch.equal(b["observed"], b["pu"][:B])
    for what in ("pu", "pc", "loss"):
        e = _nrel(b[what], a[what])
        print(f"{what}: {e:.2e}")
        assert e <= RTOL, what
    for k in a["grads"]:
        e = _nrel(b["grads"][k], a["grads"][k])
        print(f"gradient {k}: {e:.2e}")
        assert e <= RTOL, k
    for k, v in a["after"].items():
        if "num_batches_tracked" in k:
            assert int(b["after"][k]) == int(v), k
        elif "running" in k:
            assert _nrel(b["after"][k], v) <= RTOL, k


def test_generator_loss_gradient_reaches_the_fake_images():
    """Measured on MI355X: loss 3.6e-8, gradient with respect to the fake images 5.2e-7 norm-relative."""
    D, _, fake, sent = _setup()
    O = _Oracle(D.state_dict())
    D.requires_grad_(False)
    x = fake.clone().requires_grad_(True)
    loss = GL.ConditionalGenLoss().get_loss(D, x, sent)
    loss.backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in D.parameters())
    xo = fake.double().cpu().requires_grad_(True)
    h = O.features(xo)
    want = (-torch.log(O.uncond(h) + 1e-8).mean()) + (-torch.log(O.cond(h, sent.double().cpu()) + 1e-8).mean())
    want.backward()
    e_loss, e_grad = _nrel(loss.detach(), want.detach()), _nrel(x.grad, xo.grad)
    print(f"generator loss: {e_loss:.2e}; gradient with respect to the fake images: {e_grad:.2e}")
    assert e_loss <= RTOL and e_grad <= RTOL
    assert int(D.state_dict()["COND_DNET.jointConv.1.num_batches_tracked"]) == 1


def test_unconditional_path_is_bit_equal():
    D, real, _, _ = _setup()
    plain = D(real)
    D2, _, _, _ = _setup()
    assert torch.equal(plain, D2.uncond(D2.features(real)))
    # and equal to the discriminator built without cond_dim under the same seed (the shared parameters are the same bits)
    torch.manual_seed(11)
    D3 = DISC.Disc64(DF).to(DEV)
    assert torch.equal(plain, D3(real))


def test_scores_depend_on_the_text():
    D, real, fake, sent = _setup()
    D.eval()                                     # (running statistics: no state moves between the calls)
    with torch.no_grad():
        h = D.features(torch.cat([real, fake]))
        pu, pc = D.uncond(h), D.cond(h, sent)
        perm = sent[[1, 2, 3, 0]]
        pu2, pc2 = D.uncond(h), D.cond(h, perm)
        # the wrong rows ARE the real codes under the cyclically next caption
        pw = D.cond(h, sent, wrong=True)
    assert torch.equal(pu, pu2)
    assert not torch.equal(pc, pc2) and float((pc - pc2).abs().max()) > 1e-4
    assert pw.shape == (3 * B,) and torch.equal(pw[:2 * B], pc) and torch.equal(pw[2 * B:], pc2[:B])


@pytest.mark.parametrize("cls,res", [(DISC.Disc128, 128), (DISC.Disc256, 256)])
def test_larger_discriminators_forward_and_backward(cls, res):
    """B = 2: the wrong pair is the swap"""
    D, real, fake, sent = _setup(cls, res, b=2)
    loss = DL.ConditionalDiscLoss().get_loss(D, fake, real, sent)
    loss.backward()
    gl = GL.ConditionalGenLoss().get_loss(D, fake.clone().requires_grad_(True), sent)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(gl)
    for name, prm in D.named_parameters():
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0, name
    assert int(D.state_dict()["COND_DNET.jointConv.1.num_batches_tracked"]) == 4          # real, fake, wrong; fake again
    D.eval()
    with torch.no_grad():
        h = D.features(real)
        assert torch.equal(D.cond(h, sent, wrong=True)[2:], D.cond(h, sent[[1, 0]]))
