"""The rows SURVEY.md §8f lists as "next", each to the same bar as the hot path: sampling (eval-mode generator) against the
oracle, checkpoint/resume reproducing the following step bit for bit, and the DAMSM pre-training step (stock encoders + HIP
losses) against the oracle's losses and torch's own Adam."""
import importlib
import os
import sys

import pytest
import torch

from helpers import RTOL, assert_close, load, sub, T

pytestmark = pytest.mark.gpu
DEV = "cuda"

GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
RNN = importlib.import_module("attention-gan_amd.networks.rnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")
from oracle import attngan_oracle as O   # noqa: E402  (checker only)


def _setup(seed=5):
    torch.manual_seed(seed)
    G = GEN.Generator(4, 16, 8, 8).to(DEV)
    Ds = [DISC.Disc64(4).to(DEV), DISC.Disc128(4).to(DEV), DISC.Disc256(4).to(DEV)]
    enc = ENC.StandInImageEncoder(16).to(DEV)
    enc.freeze_all_weights()
    g = torch.Generator().manual_seed(seed)
    B, Tn = 4, 5
    data = dict(words=torch.randn(B, 16, Tn, generator=g).to(DEV), sent=torch.randn(B, 16, generator=g).to(DEV), lens=[5, 3, 2, 4],
                reals=[(torch.rand(B, 3, r, r, generator=g) * 2 - 1).to(DEV) for r in (64, 128, 256)],
                noise=torch.randn(B, 8, generator=g).to(DEV), eps=torch.randn(B, 8, generator=g).to(DEV))
    return G, Ds, enc, data


def _one(step, d):
    return step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"])


def test_sampling_path_matches_oracle_eval_mode():
    G, Ds, enc, d = _setup()
    step = TR.GanTrainStep(G, Ds, enc)
    _one(step, d)                                              # move the running statistics away from their init
    imgs = step.generate_images(d["words"], d["sent"], d["lens"], d["noise"])
    assert G.training                                          # mode restored
    gp = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    mu, logvar = O.vae_encode(d["sent"].cpu(), gp)
    # the sampler draws its own eps; compare through the deterministic part: feed the module's eps by re-running with mu only
    G.eval()
    with torch.no_grad():
        fakes, _, mu_d, lv_d = G(d["noise"], d["sent"], d["words"], step._make_mask(d["lens"]), d["eps"])
    G.train()
    ref, _, _, _ = O.generator_forward(gp, d["noise"].cpu(), d["sent"].cpu(), d["words"].cpu(), O.make_mask(d["lens"]), d["eps"].cpu(), train=False)
    for i in range(3):
        assert_close(fakes[i], ref[i], RTOL, f"eval-mode fake{i}")
        assert imgs[i].shape == ref[i].shape and float(imgs[i].min()) >= 0.0 and float(imgs[i].max()) <= 1.0
    assert_close(mu_d, mu, RTOL, "mu")


def test_epoch_end_sample_is_train_mode_batchnorm_under_no_grad():
    """train.py:154-158: the epoch-end sample runs the generator under no_grad WITHOUT .eval() on the fixed noise of :105 -- every
    BatchNorm normalises with THIS batch's statistics and pushes them into its running statistics once more.
    generate_images(train_mode_bn=True) against the oracle's train-mode forward: images, and the running statistics afterwards."""
    G, Ds, enc, d = _setup()
    step = TR.GanTrainStep(G, Ds, enc)
    _one(step, d)
    gp = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    fixed = torch.randn(d["noise"].shape, generator=torch.Generator().manual_seed(11)).to(DEV)       # fixed_input, train.py:105
    imgs = step.generate_images(d["words"], d["sent"], d["lens"], fixed, train_mode_bn=True, eps=d["eps"])
    assert G.training and all(not t.requires_grad for t in imgs)
    ref, _, _, _ = O.generator_forward(gp, fixed.cpu(), d["sent"].cpu(), d["words"].cpu(), O.make_mask(d["lens"]), d["eps"].cpu(), train=True)
    for i in range(3):
        assert_close(imgs[i], ref[i] * 0.5 + 0.5, RTOL, f"train-mode sample {i}")            # _denormalise_multiple
    after = G.state_dict()
    moved = 0
    for k, v in gp.items():                                    # the oracle updated gp's running statistics in place
        if "running" in k or "num_batches" in k:
            assert_close(after[k].float(), v.float(), RTOL, k)
            moved += 1
    assert moved > 0
    # and it differs from the eval-mode sample (running statistics) -- the two modes are not interchangeable
    ev = step.generate_images(d["words"], d["sent"], d["lens"], fixed, eps=d["eps"])
    assert float((ev[2] - imgs[2]).abs().max()) > 1e-3


def test_checkpoint_resume_reproduces_next_step():
    G, Ds, enc, d = _setup(7)
    a = TR.GanTrainStep(G, Ds, enc)
    _one(a, d)
    ckpt = {k: (v if not isinstance(v, torch.Tensor) else v.clone()) for k, v in a.state_dict().items()}
    import copy
    ckpt = copy.deepcopy(a.state_dict())
    out_a = _one(a, d)
    G2, Ds2, enc2, _ = _setup(99)                               # different init on purpose
    b = TR.GanTrainStep(G2, Ds2, enc2)
    b.load_state_dict(ckpt)
    out_b = _one(b, d)
    # every kernel of the step reduces in a fixed order (no float atomics), so the resumed step is bit-identical
    for k in ("d_loss0", "d_loss1", "d_loss2", "g_total", "w_loss", "s_loss", "kl"):
        assert float(out_a[k]) == float(out_b[k]), k
    for ma, mb in zip([a.G] + a.Ds, [b.G] + b.Ds):
        for (k, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(va, vb), k


def test_checkpoint_resume_continues_the_noise_stream():
    """With the default noise=None / eps=None the step draws z and eps from GanTrainStep.rng.  The checkpoint carries that
    generator's state: a resumed run continues the sequence (bit-identical next step) instead of replaying steps 0..N from the
    seed, and sampling images mid-training (its own generator) does not shift the training stream."""
    import copy

    def draw(step, d):
        return step.step(d["words"], d["sent"], d["lens"], None, d["reals"])            # noise / eps drawn inside

    G, Ds, enc, d = _setup(7)
    a = TR.GanTrainStep(G, Ds, enc, seed=3)
    draw(a, d)
    ckpt = copy.deepcopy(a.state_dict())
    out_a = draw(a, d)
    G2, Ds2, enc2, _ = _setup(99)
    b = TR.GanTrainStep(G2, Ds2, enc2, seed=3)
    b.load_state_dict(ckpt)
    b.generate_images(d["words"], d["sent"], d["lens"])        # sampling in between must not move the training noise stream
    out_b = draw(b, d)
    for k in ("d_loss0", "d_loss1", "d_loss2", "g_total", "w_loss", "s_loss", "kl"):
        assert float(out_a[k]) == float(out_b[k]), k
    assert torch.equal(out_a["fake_imgs"][2], out_b["fake_imgs"][2])
    # a trainer that restarts the generator from the seed (what an old checkpoint without "rng" gives) replays step 0's noise
    G3, Ds3, enc3, _ = _setup(99)
    c = TR.GanTrainStep(G3, Ds3, enc3, seed=3)
    old = {k: v for k, v in ckpt.items() if k not in ("rng", "sample_rng")}
    c.load_state_dict(old)
    out_c = draw(c, d)
    assert not torch.equal(out_a["fake_imgs"][2], out_c["fake_imgs"][2])


class _FixedDropout(torch.nn.Module):
    """nn.Dropout(p) in training mode with the keep-mask SUPPLIED (inverted dropout: x * keep / (1 - p)), so that the device run and
    the CPU reference run drop the same embedding elements (the stock module draws its mask from a device-specific RNG stream)"""

    def __init__(self, keep, p):
        super().__init__()
        self.register_buffer("keep", keep)
        self.p = p

    def forward(self, x):
        return x * self.keep.to(x.dtype) / (1.0 - self.p)


@pytest.mark.parametrize("dropout", [False, True], ids=["dropout-off", "dropout-0.5-fixed-mask"])
def test_damsm_pretrain_step(dropout):
    """BASELINE configs[0] as written -- pretrain_damsm.py:114-134 on 4 synthetic 64x64 images + 10-token captions (lengths 10, 7, 2,
    10: a full one and the shortest the batch guard lets through) -- with the stock encoders: the HIP losses equal the oracle's on the
    same encoder outputs; the RNN gradient is clipped to a total norm of 0.25 (:132); and the post-step weights of both encoders equal
    torch.optim.Adam(2e-3, (0.5, 0.999)) applied on the CPU to the ORACLE's gradients after the same clip.  Second case: the
    embedding dropout of rnn_encoder.py:83 ACTIVE (p = 0.5, pretrain_damsm.py:66 builds the encoder with its default) with one
    seeded keep-mask handed to both sides."""
    import copy
    torch.manual_seed(3)
    B, Tn, emb, vocab = 4, 10, 32, 50
    rnn = RNN.RNNEncoder(vocab, embdim=24, dropprob=0.0, nhidden=emb).to(DEV)   # (the stock dropout is replaced below when it is on)
    cnn = ENC.StandInImageEncoder(emb).to(DEV)                  # the Inception-shaped trunk obeys the same contract (test below)
    rnn.train()                                                 # (MIOpen's LSTM backward needs training mode)
    rnn_c, cnn_c = copy.deepcopy(rnn).cpu(), copy.deepcopy(cnn).cpu()
    g = torch.Generator().manual_seed(3)
    if dropout:
        keep = (torch.rand(B, Tn, 24, generator=g) >= 0.5)
        assert 0.3 < float(keep.float().mean()) < 0.7
        rnn.dropout, rnn_c.dropout = _FixedDropout(keep.to(DEV), 0.5), _FixedDropout(keep, 0.5)
    step = TR.DAMSMTrainStep(rnn, cnn)
    caps = torch.randint(0, vocab, (B, Tn), generator=g)
    lens = torch.tensor([10, 7, 2, 10])
    img = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1
    out = step.step(caps.to(DEV), lens, None, img.to(DEV))
    # ---- the same step on the CPU: stock encoders, ORACLE losses, torch's clip and Adam ----
    params_c = list(rnn_c.parameters()) + [p for p in cnn_c.parameters() if p.requires_grad]
    ref_opt = torch.optim.Adam(params_c, lr=2e-3, betas=(0.5, 0.999))
    feats, code = cnn_c(img)
    wemb, semb = rnn_c(caps, lens)
    wl, _ = O.words_loss(feats, wemb, torch.arange(B), lens.tolist(), None)
    sl = O.sentence_loss(code, semb, torch.arange(B), None)
    assert_close(out["w_loss"], wl, RTOL, "w_loss")
    assert_close(out["s_loss"], sl, RTOL, "s_loss")
    ref_opt.zero_grad()
    (wl + sl).backward()
    pre = float(torch.nn.utils.clip_grad_norm_(rnn_c.parameters(), 0.25))
    assert pre > 0.25, f"unclipped RNN gradient norm {pre} does not exercise the clip"
    post_hip = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in rnn.parameters() if p.grad is not None)))
    assert abs(post_hip - 0.25) <= 1e-3 * 0.25, f"clipped RNN gradient norm on the device: {post_hip}"
    for (k, pc), (_, pd) in zip(list(rnn_c.named_parameters()) + list(cnn_c.named_parameters()),
                                list(rnn.named_parameters()) + list(cnn.named_parameters())):
        assert_close(pd.grad, pc.grad, RTOL, f"clipped grad {k}")
    ref_opt.step()
    flips = total = 0
    for (k, pc), (_, pd) in zip(list(rnn_c.named_parameters()) + list(cnn_c.named_parameters()),
                                list(rnn.named_parameters()) + list(cnn.named_parameters())):
        diff = (pd.detach().cpu().double() - pc.detach().double()).abs()
        scale = float(pc.detach().abs().max())
        off = diff > RTOL * scale
        total += pc.numel()
        if int(off.sum()):
            # first Adam step is lr * sign(g): an element may flip only where its gradient is rounding noise of its tensor
            gabs = pc.grad.detach().double().abs()
            assert float(diff.max()) <= 2.05 * 2e-3 and float(gabs[off].max() / gabs.max()) <= 2 * RTOL, f"post-step {k}"
            flips += int(off.sum())
    assert flips <= max(2, int(1e-3 * total)), f"{flips} of {total} encoder weights differ from torch.optim.Adam on oracle gradients"


def test_rnn_encoder_vs_reference_golden():
    """f2 on the device (MIOpen LSTM): same fixture as the CPU test in test_host_cpu.py, north_star tolerance."""
    from test_host_cpu import _rnn_vs_golden
    _rnn_vs_golden(DEV, RTOL)


def test_inception_shaped_encoder_contract():
    torch.manual_seed(0)
    m = ENC.CNNEncoder(32).to(DEV).eval()
    x = (torch.rand(2, 3, 64, 64, device=DEV) * 2 - 1).requires_grad_(True)      # any input size is resized to 299 (:75)
    f, c = m(x)
    assert tuple(f.shape) == (2, 32, 17, 17) and tuple(c.shape) == (2, 32)
    (f.sum() + c.sum()).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    trainable = [k for k, p in m.named_parameters() if p.requires_grad]
    assert sorted(trainable) == ["emb_cnn_code.bias", "emb_cnn_code.weight", "emb_features.weight"]


def test_config1_stage1_batch64_vs_oracle():
    """BASELINE.json configs[1]: stage-1 only (CA-net + gen1 + img_out1 + Disc64) at batch 64, forward and backward vs the oracle."""
    torch.manual_seed(1)
    G = GEN.Generator(8, 32, 16, 16).to(DEV)
    D = DISC.Disc64(8).to(DEV)
    g = torch.Generator().manual_seed(1)
    B = 64
    noise, sent, eps = (torch.randn(B, n, generator=g) for n in (16, 32, 16))
    gp = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    dp = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    for k in list(gp) + list(dp):
        pass
    keys = [k for k in gp if k.startswith(("vae.", "gen1.", "img_out1.")) and k.endswith((".weight", ".bias"))]
    for k in keys:
        gp[k].requires_grad_(True)
    mu, logvar = O.vae_encode(sent, gp)
    h = O.gen_initial_stage(noise, O.vae_reparam(mu, logvar, eps), gp, "gen1")
    img_ref = O.gen_make_image(h, gp, "img_out1")
    loss_ref = O.ns_gen_loss(O.disc_forward(dp, img_ref, 64)) + O.kl_loss(mu, logvar)
    grads_ref = dict(zip(keys, torch.autograd.grad(loss_ref, [gp[k] for k in keys])))
    cond, mu_d, lv_d = G.vae(sent.to(DEV), eps.to(DEV))
    img = G.img_out1(G.gen1(noise.to(DEV), cond))
    KL = importlib.import_module("attention-gan_amd.losses.KL_loss").KL_loss
    GL = importlib.import_module("attention-gan_amd.losses.gen_loss").NonSaturatingGenLoss()
    loss = GL.get_loss(D, img) + KL(mu_d, lv_d)
    loss.backward()
    assert_close(img, img_ref, RTOL, "stage-1 image B=64")
    assert_close(loss, loss_ref, RTOL, "loss")
    named = dict(G.named_parameters())
    for k in keys:
        assert_close(named[k].grad, grads_ref[k], RTOL, f"grad {k}")


def test_stage1_only_train_step_vs_oracle():
    """What `bench.py --workload stage1_b64` steps (BASELINE configs[1]): GanTrainStep over Generator1 (CA-net + gen1 + img_out1) and
    ONE discriminator, no DAMSM (train.py:138-143 applies it to the 256x256 image only) -- image, both losses, KL and the weights
    after the two fused Adam steps against the oracle's primitives composed in train.py's order."""
    torch.manual_seed(4)
    gf, df, emb, zd, B = 8, 8, 32, 16, 6
    G = GEN.Generator1(gf, emb, zd, zd).to(DEV)
    D = DISC.Disc64(df).to(DEV)
    g = torch.Generator().manual_seed(4)
    noise, sent, eps = (torch.randn(B, n, generator=g) for n in (zd, emb, zd))
    real = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1
    gp = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    dp = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    step = TR.GanTrainStep(G, [D], None)
    out = step.step(torch.randn(B, emb, 5).to(DEV), sent.to(DEV), [5] * B, None, [real.to(DEV)], noise.to(DEV), eps.to(DEV))
    assert len(out["fake_imgs"]) == 1 and out["attn_maps"] == [] and "w_loss" not in out
    # ---- the oracle, in train.py's order: G forward, D update (real, fake), G update through the UPDATED D + KL ----
    gopt, dopt = O.AdamState(gp), O.AdamState(dp)
    for k in gopt.keys:
        gp[k].requires_grad_(True)
    mu, logvar = O.vae_encode(sent, gp)
    img = O.gen_make_image(O.gen_initial_stage(noise, O.vae_reparam(mu, logvar, eps), gp, "gen1"), gp, "img_out1")
    for k in dopt.keys:
        dp[k].requires_grad_(True)
    dloss = O.ns_disc_loss(O.disc_forward(dp, real, 64), O.disc_forward(dp, img.detach(), 64))
    dopt.apply(dp, dict(zip(dopt.keys, torch.autograd.grad(dloss, [dp[k] for k in dopt.keys]))), 2e-4)
    for k in dopt.keys:
        dp[k].requires_grad_(False)
    gl = O.ns_gen_loss(O.disc_forward(dp, img, 64))
    kl = O.kl_loss(mu, logvar)
    gopt.apply(gp, dict(zip(gopt.keys, torch.autograd.grad(gl + kl, [gp[k] for k in gopt.keys]))), 2e-4)
    assert_close(out["fake_imgs"][0], img, RTOL, "stage-1 image")
    for name, want in (("d_loss0", dloss), ("g_loss0", gl), ("kl", kl), ("g_total", gl + kl)):
        assert_close(out[name], want, RTOL, name)
    # post-step weights: first Adam step is lr * sign(g) -- elements whose gradient is rounding noise may land 2 lr away
    for mod, ref, what in ((G, gp, "G"), (D, dp, "D")):
        flips = total = 0
        for k, v in mod.state_dict().items():
            if not k.endswith((".weight", ".bias")):
                continue
            diff = (v.detach().cpu().double() - ref[k].detach().double()).abs()
            off = diff > RTOL * float(ref[k].detach().abs().max())
            total += diff.numel()
            flips += int(off.sum())
            assert float(diff.max()) <= 2.05 * 2e-4 + RTOL * float(ref[k].detach().abs().max()), f"{what} {k}"
        assert flips <= max(4, int(2e-3 * total)), f"{what}: {flips} of {total} weights off"


def test_config4_stage4_extension_vs_oracle_composition():
    """BASELINE.json configs[4]: 4th stage (512x512) + Disc512, small widths: forward vs the oracle's primitives composed alike."""
    S4 = importlib.import_module("attention-gan_amd.networks.stage4")
    torch.manual_seed(2)
    G = S4.Generator4(4, 16, 8, 8).to(DEV)
    D = S4.Disc512(2).to(DEV)
    g = torch.Generator().manual_seed(2)
    B, Tn = 2, 4
    noise, sent, eps, words = torch.randn(B, 8, generator=g), torch.randn(B, 16, generator=g), torch.randn(B, 8, generator=g), torch.randn(B, 16, Tn, generator=g)
    lens = [4, 2]
    gp = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    dp = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    mask = O.make_mask(lens)
    fakes_ref, _, _, _ = O.generator_forward(gp, noise, sent, words, mask, eps)
    # 4th stage by hand from the oracle primitives
    mu, logvar = O.vae_encode(sent, gp)
    h = O.gen_initial_stage(noise, O.vae_reparam(mu, logvar, eps), {k: v.clone() for k, v in gp.items()}, "gen1")
    gp2 = {k: v.clone() for k, v in gp.items()}
    h = O.gen_initial_stage(noise, O.vae_reparam(mu, logvar, eps), gp2, "gen1")
    for st in ("gen2", "gen3", "gen4"):
        h, _ = O.gen_next_stage(h, words, mask, gp2, st)
    img512_ref = O.gen_make_image(h, gp2, "img_out4")
    y = O.encode_image_by_16times(img512_ref, dp, "img_code_s16")
    for n in ("img_code_s32", "img_code_s64", "img_code_s128"):
        y = O.down_block(y, dp, n)
    for n in ("img_code_s128_1", "img_code_s128_2", "img_code_s128_3"):
        y = O.block3x3_leak(y, dp, n)
    p_ref = torch.sigmoid(torch.nn.functional.conv2d(y, dp["outlogits.0.weight"], dp["outlogits.0.bias"], stride=4)).view(-1)
    fakes, attns, _, _ = G(noise.to(DEV), sent.to(DEV), words.to(DEV), mask.to(DEV), eps.to(DEV))
    assert [tuple(f.shape[-2:]) for f in fakes] == [(64, 64), (128, 128), (256, 256), (512, 512)] and len(attns) == 3
    assert_close(fakes[2], fakes_ref[2], RTOL, "256 image")
    assert_close(fakes[3], img512_ref, RTOL, "512 image")
    p = D(fakes[3])
    assert_close(p, p_ref, RTOL, "Disc512 output")
    p.sum().backward()                                                                     # backward runs through the extension
    assert all(torch.isfinite(q.grad).all() for q in G.parameters() if q.grad is not None)


def _l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@pytest.mark.parametrize("storage", ["f32-storage", "bf16-storage"])
def test_config1_stage1_batch64_bf16(storage):
    """[bf16-storage]: the same stage with conv outputs, BatchNorm inputs / outputs and their gradients STORED in bf16
    (HF.set_activation_storage; include/agan.h AGAN_DT_BF16): one more rounding per stored tensor, same bounds.

    BASELINE.json configs[1] AS WRITTEN: stage-1 only (CA-net + gen1 + img_out1 + Disc64) at the real widths (gf 32, df 64,
    emb 256, z = cond = 100), batch 64, conv operands rounded to bf16 (AGAN_PREC_BF16: v_mfma_f32_32x32x16_bf16, fp32
    accumulate; BatchNorm statistics, GLU, losses and every tensor in HBM stay fp32), against the fp32 CPU oracle.

    Tolerance (documented, not 1e-3): a bf16 operand carries 8 significant bits, so one product is off by ~2^-8 relative and a
    K-term contraction by ~2^-8 / sqrt(K) of its terms' magnitude -- 2..3e-3 of a layer's output maximum (measured per layer in
    test_gpu_parity.py) -- which the six conv layers of the stage-1 generator and BatchNorm's renormalisation carry to ~1e-2
    at the image.  Bounds: image and losses 3e-2 of the maximum; gradients in relative L2 (a LeakyReLU kink that flips under
    the perturbed forward is an O(1) pointwise change, see test_gpu_metric_parity.py) 2.5e-1.  Observed values are printed."""
    L = importlib.import_module("attention-gan_amd.backend.lib")
    KL = importlib.import_module("attention-gan_amd.losses.KL_loss").KL_loss
    GL = importlib.import_module("attention-gan_amd.losses.gen_loss").NonSaturatingGenLoss()
    DL = importlib.import_module("attention-gan_amd.losses.disc_loss").NonSaturatingDiscLoss()
    torch.manual_seed(21)
    G = GEN.Generator(32, 256, 100, 100).to(DEV)
    D = DISC.Disc64(64).to(DEV)
    g = torch.Generator().manual_seed(21)
    B = 64
    noise, sent, eps = (torch.randn(B, n, generator=g) for n in (100, 256, 100))
    real = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1
    gp = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    dp = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    gkeys = [k for k in gp if k.startswith(("vae.", "gen1.", "img_out1.")) and k.endswith((".weight", ".bias"))]
    dkeys = O.trainable_keys(dp)
    for k in gkeys:
        gp[k].requires_grad_(True)
    for k in dkeys:
        dp[k].requires_grad_(True)
    mu, logvar = O.vae_encode(sent, gp)
    img_ref = O.gen_make_image(O.gen_initial_stage(noise, O.vae_reparam(mu, logvar, eps), gp, "gen1"), gp, "img_out1")
    dloss_ref = O.ns_disc_loss(O.disc_forward(dp, real, 64), O.disc_forward(dp, img_ref.detach(), 64))
    dgrads_ref = dict(zip(dkeys, torch.autograd.grad(dloss_ref, [dp[k] for k in dkeys])))
    gloss_ref = O.ns_gen_loss(O.disc_forward(dp, img_ref, 64)) + O.kl_loss(mu, logvar)
    ggrads_ref = dict(zip(gkeys, torch.autograd.grad(gloss_ref, [gp[k] for k in gkeys])))
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    HF.set_precision(L.PREC_BF16)
    HF.set_activation_storage("bf16" if storage == "bf16-storage" else None)
    try:
        cond, mu_d, lv_d = G.vae(sent.to(DEV), eps.to(DEV))
        img = G.img_out1(G.gen1(noise.to(DEV), cond))
        dloss = DL.get_loss(D, img.detach(), real.to(DEV))
        dloss.backward()
        dgr = {k: p.grad.clone() for k, p in D.named_parameters()}
        D.zero_grad()
        D.requires_grad_(False)
        gloss = GL.get_loss(D, img) + KL(mu_d, lv_d)
        gloss.backward()
    finally:
        HF.set_activation_storage(None)
        HF.set_precision(L.PREC_F32)
    e_img = float((img.detach().cpu() - img_ref.detach()).abs().max() / img_ref.detach().abs().max())
    named = dict(G.named_parameters())
    wg = max(_l2(named[k].grad, ggrads_ref[k]) for k in gkeys)
    wd = max(_l2(dgr[k], dgrads_ref[k]) for k in dkeys)
    print(f"configs[1] bf16 B=64 [{storage}]: image max-rel {e_img:.2e} | d_loss {float(dloss):.5f} vs {float(dloss_ref):.5f} | g_loss {float(gloss):.5f} vs "
          f"{float(gloss_ref):.5f} | worst G grad L2 {wg:.2e} | worst D grad L2 {wd:.2e}")
    assert e_img <= 3e-2
    assert abs(float(dloss) - float(dloss_ref)) <= 3e-2 * max(1.0, abs(float(dloss_ref)))
    assert abs(float(gloss) - float(gloss_ref)) <= 3e-2 * max(1.0, abs(float(gloss_ref)))
    assert wg <= 2.5e-1 and wd <= 2.5e-1


# (gf, df, emb, z = cond) -> bounds (image max-rel, image L2, D512 output abs, worst generator-gradient L2 vs the f32 mode)
_CONFIG4_WIDTHS = {
    "toy-gf8-df8": ((8, 8, 32, 16), (2e-1, 5e-2, 5e-2, 5e-1)),
    # observed on MI355X (round 3): image 1.7e-2 max / 2.1e-3 L2, Disc512 output 9.0e-4, gradients 1.7e-1
    "metric-gf32-df64": ((32, 64, 256, 100), (5e-2, 1e-2, 5e-3, 3.5e-1)),
}


@pytest.mark.parametrize("width", list(_CONFIG4_WIDTHS))
def test_config4_stage4_batch8_f16(width):
    """BASELINE.json configs[4] in its arithmetic: the 512x512 fourth stage + Disc512, batch 8, conv operands rounded to fp16
    (AGAN_PREC_F16: v_mfma_f32_32x32x16_f16, fp32 accumulate), at a toy width (fast) and AT THE METRIC WIDTHS (gf 32, df 64,
    emb 256, z = cond = 100: Generator4 9.4 M and Disc512 278 M parameters).  No reference oracle exists for the extension
    (SURVEY.md section 8d C5): the forward (512x512 image AND Disc512's output on it) is held to the oracle's primitives composed
    alike on the CPU, the backward to the fp32 mode of the same HIP path.

    Tolerance: an fp16 operand carries 11 significant bits -> ~3e-4 of a layer's maximum per conv (test_gpu_parity.py), ~1e-2
    after the 25 conv layers up to the 512x512 image; gradients in relative L2 for the LeakyReLU-kink reason.  fp16 also has a
    NARROW RANGE: gradients below 6e-8 flush to zero and below 6e-5 lose bits.  The data gradients of this network at
    initialisation sit around 1e-4..1e-6, inside that band, which is what the L2 bounds below price; a training run at this
    precision would scale the loss (the reference has no such mode to be faithful to).  Observed numbers are printed."""
    S4 = importlib.import_module("attention-gan_amd.networks.stage4")
    L = importlib.import_module("attention-gan_amd.backend.lib")
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    (gf, df, emb, zd), (b_max, b_l2, b_p, b_grad) = _CONFIG4_WIDTHS[width]
    torch.manual_seed(22)
    G = S4.Generator4(gf, emb, zd, zd).to(DEV)
    D = S4.Disc512(df).to(DEV)
    g = torch.Generator().manual_seed(22)
    B, Tn = 8, 10
    noise, sent, eps, words = torch.randn(B, zd, generator=g), torch.randn(B, emb, generator=g), torch.randn(B, zd, generator=g), torch.randn(B, emb, Tn, generator=g)
    lens = [10, 7, 2, 10, 5, 3, 9, 6]
    gp = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    dp = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    mask = O.make_mask(lens)
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 32)))
    with torch.no_grad():
        mu, logvar = O.vae_encode(sent, gp)
        gp2 = {k: v.clone() for k, v in gp.items()}
        h = O.gen_initial_stage(noise, O.vae_reparam(mu, logvar, eps), gp2, "gen1")
        for st in ("gen2", "gen3", "gen4"):
            h, _ = O.gen_next_stage(h, words, mask, gp2, st)
        img512_ref = O.gen_make_image(h, gp2, "img_out4")
        del h
        dp2 = {k: v.clone() for k, v in dp.items()}
        y = O.encode_image_by_16times(img512_ref, dp2, "img_code_s16")
        for n in ("img_code_s32", "img_code_s64", "img_code_s128"):
            y = O.down_block(y, dp2, n)
        for n in ("img_code_s128_1", "img_code_s128_2", "img_code_s128_3"):
            y = O.block3x3_leak(y, dp2, n)
        p_ref = torch.sigmoid(torch.nn.functional.conv2d(y, dp2["outlogits.0.weight"], dp2["outlogits.0.bias"], stride=4)).view(-1)
    res = {}
    for mode in (L.PREC_F32, L.PREC_F16):
        HF.set_precision(mode)
        try:
            G.load_state_dict({k: v.to(DEV) for k, v in gp.items()})          # same running statistics each time
            D.load_state_dict({k: v.to(DEV) for k, v in dp.items()})
            G.zero_grad(); D.zero_grad()
            fakes, _, _, _ = G(noise.to(DEV), sent.to(DEV), words.to(DEV), mask.to(DEV), eps.to(DEV))
            p = D(fakes[3])
            (-torch.log(p + 1e-8).mean()).backward()
            res[mode] = (fakes[3].detach().cpu(), p.detach().cpu(), {k: q.grad.cpu() for k, q in G.named_parameters() if q.grad is not None})
            del fakes, p
        finally:
            HF.set_precision(L.PREC_F32)
    scale = img512_ref.abs().max()
    e32 = float((res[L.PREC_F32][0] - img512_ref).abs().max() / scale)
    e16 = float((res[L.PREC_F16][0] - img512_ref).abs().max() / scale)
    l16 = _l2(res[L.PREC_F16][0], img512_ref)
    p32 = float((res[L.PREC_F32][1] - p_ref).abs().max())
    p16 = float((res[L.PREC_F16][1] - p_ref).abs().max())
    worst = max(_l2(res[L.PREC_F16][2][k], res[L.PREC_F32][2][k]) for k in res[L.PREC_F32][2])
    finite = all(torch.isfinite(v).all() for v in res[L.PREC_F16][2].values())
    print(f"configs[4] 512x512 B=8 [{width}]: image vs oracle max-rel f32-mode {e32:.2e}, f16-mode {e16:.2e} (L2 {l16:.2e}) | "
          f"Disc512 output vs oracle |dp| f32-mode {p32:.2e}, f16-mode {p16:.2e} | worst G grad L2 (f16 vs f32 mode) {worst:.2e} over "
          f"{len(res[L.PREC_F32][2])} tensors")
    # (batch 8: 30 train-mode BatchNorms over few samples and three softmax attentions amplify the 3e-4-per-layer rounding into
    # isolated pixels ~1e-1 off while the image as a whole moves by ~1e-2: bounded in both norms)
    assert e32 <= RTOL and p32 <= RTOL and finite
    assert e16 <= b_max and l16 <= b_l2 and p16 <= b_p
    assert worst <= b_grad


def test_standard_losses_and_upblock_relu():
    """The step-API leftovers of SURVEY.md section 2 #1/#6: StandardGenLoss / StandardDiscLoss (gen_loss.py:21-35, disc_loss.py:26-47)
    and Layers.upBlockReLU (layers.py:71-80) against the oracle's primitives + torch's BCE."""
    LAYERS = importlib.import_module("attention-gan_amd.utilities.layers").Layers
    GLm = importlib.import_module("attention-gan_amd.losses.gen_loss")
    DLm = importlib.import_module("attention-gan_amd.losses.disc_loss")
    torch.manual_seed(31)
    D = DISC.Disc64(8).to(DEV)
    g = torch.Generator().manual_seed(31)
    real, fake = (torch.rand(4, 3, 64, 64, generator=g) * 2 - 1 for _ in range(2))
    labels = torch.rand(4, generator=g) * 0.2 + 0.8
    dp = {k: v.detach().cpu().clone() for k, v in D.state_dict().items()}
    bce = torch.nn.functional.binary_cross_entropy
    dl = DLm.StandardDiscLoss()
    dl.make_labels_for_real_imgs = lambda num_labels, label_smooth=0.8, device="cuda": labels.to(device)     # the reference draws U(0.8, 1)
    got_d = dl.get_loss(D, fake.to(DEV), real.to(DEV))
    pf, pr = O.disc_forward(dp, fake, 64), O.disc_forward(dp, real, 64)            # fake batch first (disc_loss.py:36-44)
    assert_close(got_d, (bce(pf, torch.zeros(4)) + bce(pr, labels)) / 2, RTOL, "StandardDiscLoss")
    got_g = GLm.StandardGenLoss().get_loss(D, fake.to(DEV))
    assert_close(got_g, bce(O.disc_forward(dp, fake, 64), torch.ones(4)), RTOL, "StandardGenLoss")
    got_g.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in D.parameters())
    blk = LAYERS.upBlockReLU(16, 8).to(DEV).train()
    assert set(blk.state_dict()) == {"1.weight", "2.weight", "2.bias", "2.running_mean", "2.running_var", "2.num_batches_tracked"}
    x = torch.randn(3, 16, 8, 8, generator=g)
    p = {k: v.detach().cpu().clone() for k, v in blk.state_dict().items()}
    ref = torch.relu(O.batchnorm_train(O.conv3x3(O.upsample2(x), p["1.weight"]), p, "2"))
    assert_close(blk(x.to(DEV)), ref, RTOL, "upBlockReLU")


def test_hip_graph_replay_equals_eager_steps():
    """The whole step captured as one HIP graph (all streams, four fused Adam updates with device-resident step counters):
    warm-up + capture + replay must land where the same number of eager steps lands."""
    def run(graphed):
        G, Ds, enc, d = _setup(11)
        st = TR.GanTrainStep(G, Ds, enc)
        lens = torch.tensor(d["lens"], dtype=torch.int64, device=DEV)
        if graphed:
            g = st.capture(d["words"], d["sent"], lens, d["reals"], warmup=1, noise=d["noise"], eps=d["eps"])   # 1 warm-up + 1 capture run... 
            out = None
            for _ in range(2):
                out = g.replay()
        else:
            for _ in range(3):                                  # capture itself does not execute: 1 warm-up + 2 replays = 3 steps
                out = st.step(d["words"], d["sent"], lens, None, d["reals"], d["noise"], d["eps"])
        torch.cuda.synchronize()
        return st, {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() == 0}, set(out)
    a, oa, ka = run(False)
    b, ob, kb = run(True)
    assert ka == kb                                              # replay() and step() hand back the same entries
    assert int(a.g_opt.step_state[0]) == int(b.g_opt.step_state[0]) == 3
    # same kernels, same order per stream, no atomics: replay and eager agree bit for bit
    for k in oa:
        assert torch.equal(ob[k], oa[k]), f"loss {k}"
    for ma, mb in zip([a.G] + a.Ds, [b.G] + b.Ds):
        for (k, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(va, vb), k


def test_hip_graph_replay_equals_eager_steps_f16x3():
    """The same in the fp16 split mode: the amax arena (one zero-fill per step, slots handed out in call order) is captured with
    the step, so a replay fills and reads the slots exactly like an eager step does."""
    L = importlib.import_module("attention-gan_amd.backend.lib")
    HF = importlib.import_module("attention-gan_amd.backend.functional")
    HF.set_precision(L.PREC_F16X3)
    try:
        test_hip_graph_replay_equals_eager_steps()
    finally:
        HF.set_precision(L.PREC_F32)


def test_checkpoint_after_graph_replay_resumes_bitwise():
    """A checkpoint taken after HIP-graph replays carries the DEVICE step counter (replays never touch the host one): a fresh
    trainer that loads it and takes one eager step lands bit for bit where the uninterrupted run lands (Adam's bias corrections
    depend on the step number)."""
    import copy
    G, Ds, enc, d = _setup(13)
    a = TR.GanTrainStep(G, Ds, enc)
    lens = torch.tensor(d["lens"], dtype=torch.int64, device=DEV)
    g = a.capture(d["words"], d["sent"], lens, d["reals"], warmup=1, noise=d["noise"], eps=d["eps"])
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ckpt = copy.deepcopy(a.state_dict())
    assert int(a.g_opt.step_state[0]) == 4 and float(ckpt["g_optim"]["state"][0]["step"]) == 4.0
    out_a = a.step(d["words"], d["sent"], lens, None, d["reals"], d["noise"], d["eps"])
    G2, Ds2, enc2, _ = _setup(98)
    b = TR.GanTrainStep(G2, Ds2, enc2)
    b.load_state_dict(ckpt)
    out_b = b.step(d["words"], d["sent"], lens, None, d["reals"], d["noise"], d["eps"])
    torch.cuda.synchronize()
    for k in ("d_loss0", "d_loss1", "d_loss2", "g_total"):
        assert float(out_a[k]) == float(out_b[k]), k
    for ma, mb in zip([a.G] + a.Ds, [b.G] + b.Ds):
        for (k, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(va, vb), k


def test_side_stream_weight_gradients_match_inline():
    """overlap_weight_gradients forks every conv weight/bias gradient onto a side stream (joined by the optimiser step): two
    steps must land bit for bit where the inline path lands (a missed join would show as a stale or torn gradient)."""
    def run(side):
        G, Ds, enc, d = _setup(13)
        st = TR.GanTrainStep(G, Ds, enc)
        st.overlap_weight_gradients = side
        for _ in range(2):
            out = _one(st, d)
        torch.cuda.synchronize()
        return st, out
    a, oa = run(False)
    b, ob = run(True)
    for k in ("d_loss0", "d_loss1", "d_loss2", "g_total"):
        assert float(oa[k]) == float(ob[k]), k
    for ma, mb in zip([a.G] + a.Ds, [b.G] + b.Ds):
        for (k, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(va, vb), k


def test_train_step_is_bit_reproducible():
    """two fresh runs of the same two steps give identical weights: no kernel on the path reduces with float atomics"""
    def run():
        G, Ds, enc, d = _setup(17)
        st = TR.GanTrainStep(G, Ds, enc)
        for _ in range(2):
            _one(st, d)
        torch.cuda.synchronize()
        return st
    a, b = run(), run()
    for ma, mb in zip([a.G] + a.Ds, [b.G] + b.Ds):
        for (k, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(va, vb), k


def test_metric_config_step_properties():
    """BASELINE.json configs[2] at full size (gf 32, df 64, emb 256, T 10, batch 24, 64/128/256 px): the size-independent
    properties next to the oracle comparison of tests/test_gpu_metric_parity.py -- two fresh runs of two steps are bit-identical (no atomics at any size),
    every loss is finite, each discriminator saw 2 BatchNorm batches per D update + 1 per G update (num_batches_tracked = 6
    after two steps), Adam moved no weight by more than ~2 x lr, and the fakes are tanh-bounded."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    HF = importlib.import_module("attention-gan_amd.backend.functional")

    def run():
        step = bench.build(torch.device(DEV), 24, HF)
        before = {(i, k): v.clone() for i, m in enumerate([step.G] + step.Ds) for k, v in m.state_dict().items()
                  if v.dtype == torch.float32 and k.endswith("weight")}
        words, sent, lens, reals = bench.synthetic_batch(torch.device(DEV), 24, seed=5)
        for _ in range(2):
            out = step.step(words, sent, lens, None, reals)
        torch.cuda.synchronize()
        return step, out, before
    a, oa, before = run()
    b, ob, _ = run()
    for k in ("d_loss0", "d_loss1", "d_loss2", "g_total", "w_loss", "s_loss", "kl"):
        assert torch.isfinite(oa[k]).all() and torch.equal(oa[k], ob[k]), k
    for ma, mb in zip([a.G] + a.Ds, [b.G] + b.Ds):
        for (k, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(va, vb), k
    for d in a.Ds:
        nbt = [int(v) for k, v in d.state_dict().items() if k.endswith("num_batches_tracked")]
        assert nbt and all(n == 6 for n in nbt), nbt
    moved = 0.0
    for i, m in enumerate([a.G] + a.Ds):
        for k, v in m.state_dict().items():
            if (i, k) in before:
                moved = max(moved, float((v - before[(i, k)]).abs().max()))
    # Adam (b1 0.5, b2 0.999): |step 1| <= lr; |step 2| <= 1.054 lr (Cauchy-Schwarz on the bias-corrected m / sqrt(v))
    assert 0.0 < moved <= 2 * 2e-4 * 1.05
    for f in oa["fake_imgs"]:
        assert float(f.abs().max()) <= 1.0


def test_paired_discriminator_pass_at_metric_size():
    """Disc256 (df 64) on 24 + 24 images of 256x256: the one-pass [real; fake] update and the reference's two passes
    (disc_loss.py:55-61), against each other and against the CPU oracle.  The two HIP forms take identical LeakyReLU branches
    (same per-group statistics, same arithmetic), so they are compared directly; the oracle differentiates the branches the HIP
    pass took (oracle.LEAKY_MASKS -- see tests/test_gpu_metric_parity.py for why) and every gradient must be within RTOL of
    it, or -- where the real and the fake pass cancel to a small difference -- no further from the fp64 oracle than twice the
    fp32 oracle's own distance."""
    from collections import deque
    from helpers import LeakyMaskRecorder, rel_err
    DL = importlib.import_module("attention-gan_amd.losses.disc_loss").NonSaturatingDiscLoss
    torch.manual_seed(8)
    da, db = DISC.Disc256(64).to(DEV), DISC.Disc256(64).to(DEV)
    db.load_state_dict(da.state_dict())
    p0 = {k: v.detach().cpu().clone() for k, v in da.state_dict().items()}
    gen = torch.Generator().manual_seed(8)
    real = torch.rand(24, 3, 256, 256, generator=gen) * 2 - 1
    fake = torch.rand(24, 3, 256, 256, generator=gen) * 2 - 1
    one, two = DL(), DL()
    two.batch_pairs = False
    with LeakyMaskRecorder([da, db]) as rec:
        la = one.get_loss(da, fake.to(DEV), real.to(DEV))
        lb = two.get_loss(db, fake.to(DEV), real.to(DEV))
    la.backward()
    lb.backward()
    assert_close(la, lb, 1e-6, "loss")
    for (k, ba), (_, bb) in zip(da.named_buffers(), db.named_buffers()):
        if not k.endswith("num_batches_tracked"):
            assert_close(ba, bb, 1e-6, f"buffer {k}")
    # each HIP form against an oracle that differentiates ITS branches (the two forms sum their convolutions in different
    # orders, so a pre-activation within a rounding error of zero may take different sides in them)
    (ia, nb, masks), (ib1, nb1, mreal), (ib2, nb2, mfake) = rec.calls
    assert (ia, nb, ib1, nb1, ib2, nb2) == (0, 48, 1, 24, 1, 24)
    queues = {"one-pass": [m[:24] for m in masks] + [m[24:] for m in masks], "two-pass": list(mreal) + list(mfake)}
    flips = sum(int((a != b).sum()) for a, b in zip(queues["one-pass"], queues["two-pass"]))
    print(f"LeakyReLU branches that differ between the one-pass and the two-pass form: {flips}")

    def oracle(dt, form):
        p = {k: (v.to(dt, copy=True) if v.is_floating_point() else v.clone()) for k, v in p0.items()}
        keys = O.trainable_keys(p)
        for k in keys:
            p[k].requires_grad_(True)
        O.LEAKY_MASKS = deque(queues[form])
        O.LEAKY_STATS = stats = []
        try:
            loss = O.ns_disc_loss(O.disc_forward(p, real.to(dt), 256), O.disc_forward(p, fake.to(dt), 256))
            assert not O.LEAKY_MASKS
        finally:
            O.LEAKY_MASKS = O.LEAKY_STATS = None
        # the imposed branches may differ from the oracle's own x > 0 only on a few elements within rounding of zero
        print(O.check_leaky_stats(stats, 1e-5, 1e-5, f"kink sync {form} {str(dt)[6:]}"))      # observed: 20 of 1e8, |x| <= 1.1e-6 max|x|
        return loss.detach(), dict(zip(keys, torch.autograd.grad(loss, [p[k] for k in keys]))), p
    ref = {form: (oracle(torch.float32, form), oracle(torch.float64, form)) for form in queues}
    l32, _, p32 = ref["one-pass"][0]
    assert_close(la, l32, RTOL, "loss vs oracle")
    for k, ba in da.named_buffers():
        if not k.endswith("num_batches_tracked"):
            assert_close(ba, p32[k], RTOL, f"buffer {k} vs oracle")
    rows, bad = [], []
    for (k, pa), (_, pb) in zip(da.named_parameters(), db.named_parameters()):
        for form, p in (("one-pass", pa), ("two-pass", pb)):
            g32, g64 = ref[form][0][1], ref[form][1][1]
            e32 = rel_err(g32[k], g64[k])
            ed, e64 = rel_err(p.grad, g32[k]), rel_err(p.grad, g64[k])
            ok = ed <= RTOL or e64 <= 2.0 * e32
            rows.append(f"{k:28s} {form:8s} vs-f32 {ed:8.2e} vs-f64 {e64:8.2e} (f32 oracle vs f64 {e32:8.2e}) {'ok' if ok else 'FAIL'}")
            if not ok:
                bad.append(rows[-1])
    print("\n" + "\n".join(rows))
    assert not bad, "\n".join(bad)
