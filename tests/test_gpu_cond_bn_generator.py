"""The sentence-conditioned BatchNorm through the layers, the generator and GanTrainStep (utilities/layers.py: HipCondBatchNorm2d;
networks/generator.py: cond_bn=True), at Generator(4, 16, 10, 10), B = 3, T = 5 and Disc64/128/256(4), within helpers.RTOL of float64
CPU oracles made of stock ops: nearest x2 -> F.conv2d -> functional.cond_bn_act_reference with GLU for one up block, and the
repository's CPU oracle (oracle/attngan_oracle.py) with that block in place of its up_block for the whole generator."""
import copy
import importlib

import pytest
import torch
import torch.nn.functional as F

from helpers import RTOL, assert_close, rel_err
from oracle import attngan_oracle as O

pytestmark = pytest.mark.gpu

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")
LAY = importlib.import_module("attention-gan_amd.utilities.layers")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

DEV = torch.device("cuda", 0)
GF, DF, EMB, Z, COND, B, T = 4, 4, 16, 10, 10, 3, 5
LENS = [5, 2, 3]


# ------------------------------------------------------------------------------------------------------------------ oracles
def up_block_oracle(x, p, prefix, condition):
    """nearest x2 -> conv3x3 -> conditional BatchNorm (batch statistics) -> GLU, in the operands' dtype"""
    y = F.conv2d(O.upsample2(x), p[prefix + ".1.weight"], None, 1, 1)
    delta = F.linear(condition, p[prefix + ".2.cond.weight"])
    return HF.cond_bn_act_reference(y, p[prefix + ".2.weight"], p[prefix + ".2.bias"], delta, None, None, True, L.ACT_GLU)[0]


def generator_oracle(p, noise, sent, words, mask, eps, cond_path=True):
    """oracle.generator_forward with up_block_oracle for every up block; cond_path=False cuts the gradient that reaches the CA-net
    through the conditional BatchNorms (the values are the same)"""
    mu, logvar = O.vae_encode(sent, p)
    cond = O.vae_reparam(mu, logvar, eps)
    code = cond if cond_path else cond.detach()
    x = F.linear(torch.cat((noise, cond), 1), p["gen1.fc.0.weight"])
    x = O.glu(O.batchnorm_train(x, p, "gen1.fc.1", update_running=False))
    h = x.view(-1, x.shape[1] // 16, 4, 4)
    for i in (1, 2, 3, 4):
        h = up_block_oracle(h, p, f"gen1.upsample{i}", code)
    imgs = [O.gen_make_image(h, p, "img_out1")]
    for g, o in (("gen2", "img_out2"), ("gen3", "img_out3")):
        ctx, _ = O.attention_module(h, words, p[g + ".attention.conv1.weight"], mask)
        x = torch.cat((h, ctx), 1)
        for i in range(2):
            x = O.res_block(x, p, f"{g}.residual.{i}", True)
        h = up_block_oracle(x, p, g + ".upsample", code)
        imgs.append(O.gen_make_image(h, p, o))
    return imgs


def params64(module):
    return {k: (v.detach().double().cpu().clone().requires_grad_(v.dtype.is_floating_point and not k.endswith(("running_mean", "running_var")))
                if v.dtype.is_floating_point else v.detach().cpu().clone()) for k, v in module.state_dict().items()}


def gen_inputs(seed=5):
    g = torch.Generator().manual_seed(seed)
    noise, sent, words = torch.randn(B, Z, generator=g), torch.randn(B, EMB, generator=g), torch.randn(B, EMB, T, generator=g)
    eps = torch.randn(B, COND, generator=g)
    noise[1] = noise[0]                                   # samples 0 and 1: equal noise, different sentences
    return noise, sent, words, O.make_mask(LENS), eps


def randomise_cond_weights(module, seed=9, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if k.endswith("2.cond.weight"):
                v.copy_((torch.randn(v.shape, generator=g) * scale).to(v.device))


# ---------------------------------------------------------------------------------------------------------- single up block
def test_up_block_vs_float64_oracle():
    torch.manual_seed(11)
    blk = LAY.Layers.upBlock(8, 4, cond_dim=COND)
    randomise_cond_weights(blk)
    with torch.no_grad():                                  # (affine terms off their 1 / 0 initialisation)
        getattr(blk, "2").weight.uniform_(0.5, 1.5)
        getattr(blk, "2").bias.normal_(0, 0.2)
    blk = blk.to(DEV).train()
    g = torch.Generator().manual_seed(12)
    x, cond = torch.randn(B, 8, 6, 6, generator=g), torch.randn(B, COND, generator=g)
    dout = torch.randn(B, 4, 12, 12, generator=g)
    xd, cd = x.to(DEV).requires_grad_(True), cond.to(DEV).requires_grad_(True)
    out = blk(xd, cd)
    assert tuple(out.shape) == (B, 4, 12, 12)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    p = params64(blk)
    x64, c64 = x.double().requires_grad_(True), cond.double().requires_grad_(True)
    want = up_block_oracle(x64, {"blk." + k: v for k, v in p.items()}, "blk", c64)
    want.backward(dout.double())
    assert_close(out, want, RTOL, "out")
    assert_close(xd.grad, x64.grad, RTOL, "dx")
    assert_close(cd.grad, c64.grad, RTOL, "dcondition")
    for k in ("1.weight", "2.weight", "2.bias", "2.cond.weight"):
        got = dict(blk.named_parameters())[k].grad
        assert got is not None and p[k].grad is not None, k
        assert_close(got, p[k].grad, RTOL, f"d {k}")
    # the running statistics moved as the plain BatchNorm's do
    bn = getattr(blk, "2")
    assert int(bn.num_batches_tracked) == 1 and bool((bn.running_mean != 0).any())
    with pytest.raises(ValueError, match="condition"):
        blk(xd)


def test_eval_mode_uses_the_running_statistics_and_its_backward_raises():
    torch.manual_seed(13)
    blk = LAY.Layers.upBlock(8, 4, cond_dim=COND)
    randomise_cond_weights(blk)
    bn = getattr(blk, "2")
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    blk = blk.to(DEV).eval()
    g = torch.Generator().manual_seed(14)
    x, cond = torch.randn(B, 8, 6, 6, generator=g), torch.randn(B, COND, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    out = blk(xd, cond.to(DEV))
    p = {k: v.detach().double().cpu() for k, v in blk.state_dict().items()}
    y = F.conv2d(O.upsample2(x.double()), p["1.weight"], None, 1, 1)
    want = HF.cond_bn_act_reference(y, p["2.weight"], p["2.bias"], F.linear(cond.double(), p["2.cond.weight"]), p["2.running_mean"],
                                    p["2.running_var"], False, L.ACT_GLU)[0]
    assert_close(out, want, RTOL, "eval out")
    assert int(bn.num_batches_tracked) == 0
    with pytest.raises(L.AganError, match="eval mode"):
        out.sum().backward()


# ---------------------------------------------------------------------------------------------------------- whole generator
def _pair(seed=7):
    """(unconditional generator, conditional generator with the same weights and zero cond weights), on the device, train mode"""
    torch.manual_seed(seed)
    plain = GEN.Generator(GF, EMB, Z, COND)
    cond = GEN.Generator(GF, EMB, Z, COND, cond_bn=True)
    report = cond.load_state_dict(plain.state_dict(), strict=False)          # the warm start
    assert len(report.missing_keys) == 6 and not report.unexpected_keys
    return plain.to(DEV).train(), cond.to(DEV).train()


def _run(G, inputs):
    noise, sent, words, mask, eps = (t.to(DEV) for t in inputs)
    return G(noise, sent, words, mask, eps)


def test_zero_cond_weights_reproduce_the_unconditional_generator():
    """The conditional forward apply is bn_act's arithmetic on gamma + delta, beta + delta (make_affine / norm_of of csrc/bn_common.h) and
    its statistics are bn_act's bit for bit; zero cond weights give delta = 0, so the images -- and the running statistics -- are the
    unconditional generator's bits, not merely within RTOL of them."""
    plain, cond = _pair()
    inputs = gen_inputs()
    want, got = _run(plain, inputs)[0], _run(cond, inputs)[0]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        assert_close(a, b, RTOL, f"image {i}")
        assert torch.equal(a, b), f"image {i}: max |conditional - unconditional| = {float((a - b).detach().abs().max()):.3e}"
    ps, cs = plain.state_dict(), cond.state_dict()
    for k in ps:
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(cs[k], ps[k]), k


def test_generator_vs_float64_oracle_and_the_gradient_through_cond():
    _, cond = _pair()
    randomise_cond_weights(cond)
    inputs = gen_inputs()
    imgs = _run(cond, inputs)[0]
    probes = [torch.cos(torch.arange(im.numel(), dtype=torch.float64) * 0.37 + i).view(im.shape) for i, im in enumerate(imgs)]
    sum((im * pr.float().to(DEV)).sum() for im, pr in zip(imgs, probes)).backward()
    torch.cuda.synchronize()
    # samples 0 and 1 share the noise and differ in the sentence
    assert bool((inputs[0][0] == inputs[0][1]).all())
    for i, im in enumerate(imgs):
        assert rel_err(im[0], im[1]) > 10 * RTOL, f"image {i}: samples with different sentences came out alike"
    # the cond weights act: the same generator with them at zero gives other images
    _, zero = _pair()
    for i, (a, b) in enumerate(zip(imgs, _run(zero, inputs)[0])):
        assert rel_err(a, b) > 10 * RTOL, f"image {i}: the cond weights changed nothing"

    def oracle(cond_path):
        p = params64(cond)
        noise, sent, words, mask, eps = inputs
        out = generator_oracle(p, noise.double(), sent.double(), words.double(), mask, eps.double(), cond_path)
        sum((im * pr).sum() for im, pr in zip(out, probes)).backward()
        return out, p
    want, p = oracle(True)
    for i, (a, b) in enumerate(zip(imgs, want)):
        assert_close(a, b, RTOL, f"image {i}")
    named = dict(cond.named_parameters())
    for k in ("vae.fc.weight", "vae.fc.bias", "gen1.fc.0.weight", "gen1.upsample1.2.cond.weight", "gen1.upsample4.2.cond.weight",
              "gen2.upsample.2.cond.weight", "gen3.upsample.2.cond.weight", "gen3.upsample.2.weight", "gen1.upsample2.2.bias"):
        assert_close(named[k].grad, p[k].grad, RTOL, f"d {k}")
    # that gradient includes the path through the conditional BatchNorms: without it the oracle's own gradient is far away
    _, cut = oracle(False)
    gap = rel_err(cut["vae.fc.weight"].grad, p["vae.fc.weight"].grad)
    print(f"d vae.fc.weight: HIP vs oracle {rel_err(named['vae.fc.weight'].grad, p['vae.fc.weight'].grad):.3e}; "
          f"oracle without the cond path vs with it {gap:.3e}")
    assert gap > 10 * RTOL, "the probe does not tell the two gradients apart"


# ------------------------------------------------------------------------------------------------------------- GanTrainStep
STEPS = 3


def _setup(seed=3, **kw):
    torch.manual_seed(seed)
    G = GEN.Generator(GF, EMB, Z, COND, cond_bn=True).to(DEV)
    Ds = [DISC.Disc64(DF).to(DEV), DISC.Disc128(DF).to(DEV), DISC.Disc256(DF).to(DEV)]
    enc = ENC.StandInImageEncoder(EMB).to(DEV)
    enc.freeze_all_weights()
    g = torch.Generator().manual_seed(seed)
    d = dict(words=torch.randn(B, EMB, T, generator=g).to(DEV), sent=torch.randn(B, EMB, generator=g).to(DEV),
             lens=torch.tensor(LENS, dtype=torch.int64, device=DEV),
             reals=[(torch.rand(B, 3, r, r, generator=g) * 2 - 1).to(DEV) for r in (64, 128, 256)])
    return TR.GanTrainStep(G, Ds, enc, seed=seed, **kw), d


def _scalars(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() == 0}


def _cond_slices(step):
    """(key, offset, numel) of every cond weight inside the generator's flat buffers"""
    out = []
    for k, p in step.G.named_parameters():
        if k.endswith("2.cond.weight"):
            dst = HF.grad_dst(p)
            assert dst is not None, f"{k} is not in the flat optimiser"
            out.append((k, dst.offset, dst.numel))
    assert len(out) == 6
    return out


_EAGER = {}


def _eager_run():
    """STEPS eager steps, taken once: the first step's generator gradient, the final losses, flat parameters and flat gradient"""
    if not _EAGER:
        step, d = _setup()
        grads = []
        step.on_gradients = lambda tag, opt: grads.append(opt.grad.clone()) if tag == "G" else None
        for _ in range(STEPS):
            out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        torch.cuda.synchronize()
        _EAGER.update(scalars=_scalars(out), flat=step.g_opt.flat.clone(), grad=step.g_opt.grad.clone(), first_grad=grads[0],
                      slices=_cond_slices(step), d_flats=[o.flat.clone() for o in step.d_opts])
    return _EAGER


def test_eager_step_trains_the_cond_weights():
    run = _eager_run()
    for k, v in run["scalars"].items():
        assert bool(torch.isfinite(v)), k
    for k, off, n in run["slices"]:
        g = run["first_grad"][off:off + n]
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), f"{k}: no gradient in the flat buffer"
        assert bool((run["flat"][off:off + n] != 0).any()), f"{k}: still zero after {STEPS} steps"


@pytest.mark.parametrize("mode", ["graph", "segments"])
def test_eager_graph_and_segments_agree_bit_for_bit(mode):
    """1 warm-up step + STEPS - 1 replays against STEPS eager steps: losses, the generator's flat gradient and every flat parameter"""
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
    assert bool((want["grad"] != 0).any())
    assert torch.equal(step.g_opt.grad, want["grad"]), f"{mode}: generator gradient"
    assert torch.equal(step.g_opt.flat, want["flat"]), f"{mode}: generator parameters"
    for i, (a, b) in enumerate(zip(step.d_opts, want["d_flats"])):
        assert torch.equal(a.flat, b), f"{mode}: discriminator {i} parameters"


def test_the_averaged_generator_follows_the_cond_weights():
    step, d = _setup(ema=0.999)
    keys = [k for k in step.G_ema.state_dict() if k.endswith("2.cond.weight")]
    assert len(keys) == 6 and all(not bool(step.G_ema.state_dict()[k].any()) for k in keys)
    step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    live, avg = step.G.state_dict(), step.G_ema.state_dict()
    for k in keys:
        assert bool((live[k] != 0).any()), f"{k}: the live weight did not move"
        assert bool((avg[k] != 0).any()), f"{k}: the averaged weight did not move"


def test_checkpoint_round_trip_reproduces_the_next_step():
    a, d = _setup()
    for _ in range(2):
        a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    ckpt = copy.deepcopy(a.state_dict())
    b, _ = _setup(seed=77)
    b.load_state_dict(ckpt)
    for k, v in a.G.state_dict().items():
        assert torch.equal(v, b.G.state_dict()[k]), k
    assert sum(k.endswith("2.cond.weight") for k in b.G.state_dict()) == 6
    out_a = a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    out_b = b.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    sa, sb = _scalars(out_a), _scalars(out_b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.g_opt.flat, b.g_opt.flat) and torch.equal(a.g_opt.grad, b.g_opt.grad)
    for i, (oa, ob) in enumerate(zip(a.d_opts, b.d_opts)):
        assert torch.equal(oa.flat, ob.flat), f"discriminator {i}"
