"""GanTrainStep(geometry=...) at the tiny configuration of tests/test_gpu_ada_step.py (gf = df = 8, B = 4, T = 10), restated here: the
geometric warp alone, and in front of DiffAugment's stages with an adapting probability (ada_interval = 2 and ada_kimg = 0.08 move p
by 0.1 per window, as there).

The three run modes agree bit for bit (losses, flat parameters, the controller's words), a checkpoint resumes bit for bit, a step on
the kernels equals the step with functional.affine_warp replaced by the fp32 torch statement within the project's 1e-3, and with
geometry=None nothing is drawn.

Measured on MI355X (test_step_equals_the_step_on_the_torch_oracle prints every figure), geometry alone and geometry + DiffAugment at
p = 0.6 alike: every loss and the three discriminators' flat gradients EQUAL the oracle step's (the forward kernel performs the fp32
statement's operations in its order, so the warped images are the same bits), the generator's flat gradient is within 1.5e-7
norm-relative (the backward's summation order differs from autograd's)."""
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
GEOMETRY = "xflip,rot90,scale,rotate,aniso"
POLICY = "color,translation,cutout"
GF, DF, EMB, Z, COND, B, T = 8, 8, 32, 16, 16, 4, 10
CONFIGS = {"geometry": dict(geometry=GEOMETRY),
           "geometry+augment+ada": dict(geometry=GEOMETRY, augment=POLICY, augment_p=0.6, ada_target=0.0, ada_interval=2, ada_kimg=0.08)}
STEPS = 4


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
             aug_u=torch.rand(9, B, 8, generator=g).to(DEV), aug_q=torch.rand(9, B, 4, generator=g).to(DEV),
             aug_g=torch.rand(9, B, 16, generator=g).to(DEV))
    step = TR.GanTrainStep(G, Ds, enc, seed=seed, **kw)
    return step, d


def _scalars(out):
    return {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor) and v.dim() == 0}


def _flats(step):
    return [o.flat.clone() for o in [step.g_opt] + step.d_opts]


_EAGER = {}


def _eager_run(name):
    """STEPS eager steps, taken once per configuration: final losses, flats and the controller's words"""
    if name not in _EAGER:
        step, d = _setup(**CONFIGS[name])
        for _ in range(STEPS):
            out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
        torch.cuda.synchronize()
        _EAGER[name] = dict(scalars=_scalars(out), flats=_flats(step), words=None if step.ada is None else step.ada.state[:6].clone())
    return _EAGER[name]


@pytest.mark.parametrize("mode", ["graph", "segments"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_eager_graph_and_segments_agree_bit_for_bit(name, mode):
    """every uniform -- the geometric stages' too -- is drawn INSIDE each form from equally seeded generators, and the matrix launch
    reads p from device memory: 1 warm-up step + STEPS - 1 replays against STEPS eager steps"""
    want = _eager_run(name)
    step, d = _setup(**CONFIGS[name])
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
    if want["words"] is not None:
        assert torch.equal(step.ada.state[:6], want["words"]), f"{mode}: {step.ada.state[:6].tolist()} vs {want['words'].tolist()}"
        assert step.ada.sync()["adjustments"] == STEPS // 2


@pytest.mark.parametrize("name", list(CONFIGS))
def test_checkpoint_resumes_bit_for_bit(name):
    a, d = _setup(**CONFIGS[name])
    for _ in range(3):
        a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    ckpt = copy.deepcopy(a.state_dict())
    assert "geometry" not in ckpt and ("ada" in ckpt) == (a.ada is not None)       # the stages are configuration, not checkpoint content
    b, _ = _setup(seed=77, **CONFIGS[name])
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


@pytest.mark.parametrize("name", ["geometry", "geometry+augment+p"])
def test_step_equals_the_step_on_the_torch_oracle(name, monkeypatch):
    kw = dict(geometry=GEOMETRY) if name == "geometry" else dict(geometry=GEOMETRY, augment=POLICY, augment_p=0.6)

    def run(oracle):
        step, d = _setup(**kw)
        grads, calls = {}, []
        step.on_gradients = lambda tag, opt: grads.__setitem__(tag, opt.grad.clone())
        if oracle:
            def reference(xs, M):
                x = xs if isinstance(xs, torch.Tensor) else torch.cat(list(xs), dim=0)
                calls.append(tuple(x.shape))
                return A.affine_warp_reference(x.float(), M)
            monkeypatch.setattr(HF, "affine_warp", reference)
        extra = (d["aug_u"], d["aug_q"]) if "augment" in kw else (None, None)
        out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"], d["noise"], d["eps"], *extra, d["aug_g"])
        torch.cuda.synchronize()
        monkeypatch.undo()
        if oracle:                                      # nine tensors: [real; fake] and fake again, per discriminator
            assert sorted(calls) == sorted([(2 * B, 3, r, r) for r in (64, 128, 256)] + [(B, 3, r, r) for r in (64, 128, 256)])
        return _scalars(out), grads, step, d
    got, got_grads, step, d = run(False)
    want, want_grads, _, _ = run(True)
    # the matrices the step used: the stages were at work, and with a probability some gates were open and some shut
    g = d["aug_g"].reshape(-1, 16)
    M = HF.geometry_matrices(g, step.geometry, None if step.ada is None else step.ada.p)
    assert not bool((M == torch.tensor([1.0, 0, 0, 0, 1, 0], device=DEV)).all())
    if step.ada is not None:
        gates = A.geometry_gates(g, step.ada.p)
        assert bool(gates.any()) and not bool(gates.all()) and not torch.equal(M, HF.geometry_matrices(g, step.geometry))
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
    print(f"{name}: step vs oracle: worst loss error {worst_loss:.2e}, worst gradient error {worst_grad:.2e}")


def test_without_geometry_nothing_is_drawn():
    plain, d = _setup()
    assert plain.geometry == 0
    fw = plain._gen_forward(d["words"], d["sent"], d["lens"], None, None)
    assert fw.aug_m is None and fw.aug_u is None and fw.aug_q is None
    assert plain._augmenter(fw, 0, 2) is None
    # the generator stands where two randn draws leave it, as before
    twin = torch.Generator(device=DEV)
    twin.manual_seed(3 * 1000003)
    torch.randn(B, Z, device=DEV, generator=twin)
    torch.randn(B, COND, device=DEV, generator=twin)
    assert torch.equal(plain.rng.get_state(), twin.get_state())
    # an aug_g handed to a step without geometry is ignored, not drawn from
    fw = plain._gen_forward(d["words"], d["sent"], d["lens"], d["noise"], d["eps"], None, None, d["aug_g"])
    assert fw.aug_m is None and torch.equal(plain.rng.get_state(), twin.get_state())
    # with geometry: one more draw of 3 * len(Ds) * B * 16 numbers, the last of the step's
    geo, _ = _setup(geometry=GEOMETRY)
    fw = geo._gen_forward(d["words"], d["sent"], d["lens"], None, None)
    assert tuple(fw.aug_m.shape) == (9, B, 6) and fw.aug_u is None and fw.aug_q is None
    assert not torch.equal(geo.rng.get_state(), twin.get_state())
    g = torch.rand(9, B, 16, device=DEV, generator=twin)
    assert torch.equal(geo.rng.get_state(), twin.get_state())
    assert torch.equal(fw.aug_m.view(-1, 6), HF.geometry_matrices(g.view(-1, 16), 31))
    with pytest.raises(ValueError):
        geo.step(d["words"], d["sent"], d["lens"], None, d["reals"], aug_g=d["aug_g"][:3])


def test_probability_needs_a_policy_or_geometry():
    torch.manual_seed(0)
    G = GEN.Generator(GF, EMB, Z, COND).to(DEV)
    Ds = [DISC.Disc64(DF).to(DEV)]
    with pytest.raises(ValueError, match="augment_p and ada_target need a non-empty augment policy"):
        TR.GanTrainStep(G, Ds, None, augment_p=0.5)
    with pytest.raises(ValueError, match="augment_p and ada_target need a non-empty augment policy"):
        TR.GanTrainStep(G, Ds, None, ada_target=0.5, geometry="")
    with pytest.raises(ValueError):
        TR.GanTrainStep(G, Ds, None, geometry="flip")
    step = TR.GanTrainStep(G, Ds, None, geometry="xflip", augment_p=0.5)
    assert step.ada is not None and step.augment == 0 and step.geometry == A.XFLIP
