"""The channel-wise word attention inside trainers.GanTrainStep, which needed no change for it: Generator(4, 16, 10, 10,
channel_attn=True) with Disc64/128/256(4), B = 3.  Eager steps, capture() replays and capture_segments() replays agree bit for bit;
a repeated step from the same state is bit-identical; a checkpoint round trip reproduces the next step; the averaged generator
follows the perception weights; both new parameters have a slice in the flat optimiser and a gradient after one step."""
import copy
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu

HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
ENC = importlib.import_module("attention-gan_amd.networks.cnn_encoder")
TR = importlib.import_module("attention-gan_amd.trainers.trainer")

DEV = torch.device("cuda", 0)
GF, DF, EMB, Z, COND, B, T = 4, 4, 16, 10, 10, 3, 5
LENS = [5, 2, 3]
STEPS = 3
KEYS = ("gen2.channel_attn.perception.weight", "gen3.channel_attn.perception.weight")


def _setup(seed=3, **kw):
    torch.manual_seed(seed)
    G = GEN.Generator(GF, EMB, Z, COND, channel_attn=True).to(DEV)
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


def _slices(step):
    """(key, offset, numel) of the perception weights inside the generator's flat buffers"""
    named = dict(step.G.named_parameters())
    out = []
    for k in KEYS:
        dst = HF.grad_dst(named[k])
        assert dst is not None, f"{k} is not in the flat optimiser"
        assert dst.numel == named[k].numel()
        out.append((k, dst.offset, dst.numel))
    return out


_EAGER = {}


def _eager_run():
    """STEPS eager steps, taken once: the generator gradient of every step, the final losses, flat parameters and flat gradient"""
    if not _EAGER:
        step, d = _setup()
        grads = []
        step.on_gradients = lambda tag, opt: grads.append(opt.grad.clone()) if tag == "G" else None
        flats = [step.g_opt.flat.clone()]
        for _ in range(STEPS):
            out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
            flats.append(step.g_opt.flat.clone())
        torch.cuda.synchronize()
        _EAGER.update(scalars=_scalars(out), flat=step.g_opt.flat.clone(), grad=step.g_opt.grad.clone(), grads=grads, flats=flats,
                      slices=_slices(step), d_flats=[o.flat.clone() for o in step.d_opts])
    return _EAGER


def test_both_new_parameters_have_a_flat_slice_and_a_gradient_after_one_step():
    run = _eager_run()
    for k, v in run["scalars"].items():
        assert bool(torch.isfinite(v)), k
    assert [n for _, _, n in run["slices"]] == [64 * 64 * EMB, 128 * 128 * EMB]
    spans = sorted((off, off + n) for _, off, n in run["slices"])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "slices overlap"
    for k, off, n in run["slices"]:
        g0 = run["grads"][0][off:off + n]
        assert bool(torch.isfinite(g0).all()) and bool((g0 != 0).any()), f"{k}: no gradient in the first step"
        assert not torch.equal(run["flats"][1][off:off + n], run["flats"][0][off:off + n]), f"{k}: the first step did not move it"


def test_the_gradient_buckets_hold_the_new_slices_whole():
    """the bucket plan of data parallelism sees ordinary parameters: each perception weight lies inside exactly one bucket, and the
    buckets tile the flat gradient"""
    DP = importlib.import_module("attention-gan_amd.dataparallel")
    step, _ = _setup()
    buckets = DP.GradBuckets(step.g_opt, bucket_bytes=1 << 18)            # smaller than either weight: they open buckets of their own
    assert buckets.bounds[0][0] == 0 and buckets.bounds[-1][1] == step.g_opt.numel
    assert all(a[1] == b[0] for a, b in zip(buckets.bounds, buckets.bounds[1:]))
    index = {id(p): i for i, p in enumerate(step.g_opt.params)}
    named = dict(step.G.named_parameters())
    for k, off, n in _slices(step):
        lo, hi = buckets.bounds[buckets.param_bucket[index[id(named[k])]]]
        assert lo <= off and off + n <= hi, f"{k}: [{off}, {off + n}) is not inside its bucket [{lo}, {hi})"
    assert sum(buckets.counts) == len(step.g_opt.params)


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


def test_the_same_step_from_the_same_state_is_bit_identical():
    want = _eager_run()
    step, d = _setup()
    for _ in range(STEPS):
        out = step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    got = _scalars(out)
    for k in want["scalars"]:
        assert torch.equal(got[k], want["scalars"][k]), k
    assert torch.equal(step.g_opt.grad, want["grad"]) and torch.equal(step.g_opt.flat, want["flat"])


def test_the_averaged_generator_follows_the_perception_weights():
    step, d = _setup(ema=0.999)
    before = {k: step.G_ema.state_dict()[k].clone() for k in KEYS}
    for _ in range(2):
        step.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    avg = step.G_ema.state_dict()
    for k in KEYS:
        assert not torch.equal(avg[k], before[k]), f"{k}: the averaged weight did not move"


def test_checkpoint_round_trip_reproduces_the_next_step():
    a, d = _setup()
    for _ in range(2):
        a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    ckpt = copy.deepcopy(a.state_dict())
    b, _ = _setup(seed=77)
    b.load_state_dict(ckpt)
    for k, v in a.G.state_dict().items():
        assert torch.equal(v, b.G.state_dict()[k]), k
    assert all(k in b.G.state_dict() for k in KEYS)
    out_a = a.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    out_b = b.step(d["words"], d["sent"], d["lens"], None, d["reals"])
    torch.cuda.synchronize()
    sa, sb = _scalars(out_a), _scalars(out_b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.g_opt.flat, b.g_opt.flat) and torch.equal(a.g_opt.grad, b.g_opt.grad)
    for i, (oa, ob) in enumerate(zip(a.d_opts, b.d_opts)):
        assert torch.equal(oa.flat, ob.flat), f"discriminator {i}"
