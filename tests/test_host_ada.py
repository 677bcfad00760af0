"""CPU-side tests of adaptive discriminator augmentation: the gated transform in torch ops (augment.diffaug_reference with q and p:
the oracle of tests/test_gpu_ada.py), the controller in Python integers and doubles (augment.ada_reference: the oracle of
agan_ada_update), the C ABI's argument checks (which return before any device work) and GanTrainStep's constructor checks."""
import ctypes
import importlib
import math
import struct

import pytest
import torch

A = importlib.import_module("attention-gan_amd.augment")
L = importlib.import_module("attention-gan_amd.backend.lib")

SHAPE = (8, 3, 9, 12)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(seed=0, shape=SHAPE, dtype=torch.float64):
    g = _gen(seed)
    x = torch.randn(shape, generator=g, dtype=dtype)
    x[0, 0, 0, 0] = -0.0
    u = torch.rand(shape[0], 8, generator=g, dtype=torch.float32)
    return x, u


def _q_for_masks(p=0.5):
    """q [8, 4] such that sample n passes exactly the gates of the bits of n at probability p"""
    q = torch.empty(8, 4, dtype=torch.float32)
    for n in range(8):
        for k in range(3):
            q[n, k] = 0.25 * p if n >> k & 1 else min(1.5 * p, 0.999)
    q[:, 3] = 0.0                                                      # reserved: must not matter
    return q


@pytest.mark.parametrize("policy", range(8))
def test_p_one_is_the_ungated_function_and_p_zero_the_identity(policy):
    x, u = _case(policy)
    q = torch.rand(8, 4, generator=_gen(50 + policy))
    assert torch.equal(A.diffaug_reference(x, u, policy, q, 1.0), A.diffaug_reference(x, u, policy))
    y0 = A.diffaug_reference(x, u, policy, q, 0.0)
    assert torch.equal(y0, x) and math.copysign(1.0, float(y0[0, 0, 0, 0])) == -1.0
    assert torch.equal(A.diffaug_reference(x, u, policy, q, float("nan")), x)          # a NaN p gates everything off
    assert torch.equal(A.diffaug_reference(x, u, policy, q, torch.tensor([1.0])), A.diffaug_reference(x, u, policy))
    with pytest.raises(ValueError):
        A.diffaug_reference(x, u, policy, q)
    with pytest.raises(ValueError):
        A.diffaug_reference(x, u, policy, q[:, :3], 0.5)


@pytest.mark.parametrize("policy", [7, 5, 3, 6])
def test_every_gate_mask_equals_the_policy_masked_per_sample(policy):
    x, u = _case(10 + policy)
    x.requires_grad_(True)
    r = torch.randn(SHAPE, generator=_gen(20 + policy), dtype=torch.float64)
    q = _q_for_masks(0.5)
    assert A.gate_masks(q, 0.5).tolist() == [[bool(n >> k & 1) for k in range(3)] for n in range(8)]
    y = A.diffaug_reference(x, u, policy, q, 0.5)
    grad, = torch.autograd.grad((y * r).sum(), x)
    for n in range(8):
        xn = x[n:n + 1].detach().clone().requires_grad_(True)
        yn = A.diffaug_reference(xn, u[n:n + 1], policy & n)
        gn, = torch.autograd.grad((yn * r[n:n + 1]).sum(), xn, allow_unused=True)
        gn = torch.zeros_like(xn) if gn is None else gn
        if policy & n & A.COLOR:                                        # the colour sums may be taken in another order: 1e-14
            assert float((y[n:n + 1] - yn).detach().abs().max()) <= 1e-14 and float((grad[n:n + 1] - gn).abs().max()) <= 1e-14
        else:                                                           # gathers and selections only: the same bits
            assert torch.equal(y[n:n + 1].detach(), yn.detach()), n
            assert torch.equal(grad[n:n + 1], gn), n


def test_the_compare_is_an_fp32_compare():
    p = 0.3
    p32 = struct.unpack("<f", struct.pack("<f", p))[0]
    below = float(torch.nextafter(torch.tensor(p32, dtype=torch.float32), torch.tensor(0.0)))
    q = torch.tensor([[p32, below, 0.0, 0.0]], dtype=torch.float32)
    assert A.gate_masks(q, p).tolist() == [[False, True, True]]          # q == p is off, the fp32 below p is on
    assert A.gate_masks(q.double(), torch.tensor([p32])).tolist() == [[False, True, True]]


# ---- the controller -------------------------------------------------------------------------------------------------------------
def _f32(v):
    return struct.unpack("<f", struct.pack("<f", v))[0]


def test_all_positive_scores_raise_p_by_count_times_rate_and_all_negative_lower_it():
    rate = 1.0 / 4096                                                   # a power of two: every step below is exact in fp32
    st = A.ada_new_state(0.25)
    up = [A.ada_tally(torch.full((16,), 0.9)), A.ada_tally(torch.full((16,), 0.7))]
    assert up == [(16, 16), (16, 16)]
    for w in range(3):
        A.ada_reference(st, up, 1, 0.6, rate, 1.0)
        assert st["p"] == 0.25 + (w + 1) * 32 * rate and st["r_t"] == 1.0 and st["adjustments"] == w + 1
        assert (st["sum"], st["count"], st["calls"]) == (0, 0, 0)
    down = [A.ada_tally(torch.full((16,), 0.1)), None]
    for w in range(2):
        A.ada_reference(st, down, 1, 0.6, rate, 1.0)
        assert st["p"] == 0.25 + 96 * rate - (w + 1) * 16 * rate and st["r_t"] == -1.0


def test_clamping_target_hit_and_empty_window():
    st = A.ada_new_state(0.01)
    A.ada_reference(st, [(-8, 8)], 1, 0.6, 0.01, 0.5)
    assert st["p"] == 0.0 and st["adjustments"] == 1
    st = A.ada_new_state(0.45)
    A.ada_reference(st, [(8, 8)], 1, 0.6, 0.01, 0.5)
    assert st["p"] == 0.5
    st = A.ada_new_state(0.25)
    A.ada_reference(st, [(4, 8)], 1, 0.5, 0.01, 1.0)                    # r == target: sgn(0) = 0
    assert st["p"] == 0.25 and st["r_t"] == 0.5 and st["adjustments"] == 1
    st = A.ada_new_state(0.25)
    st["r_t"] = 0.125
    for slots in ([None], [(0, 0)], []):
        A.ada_reference(st, slots, 1, 0.5, 0.01, 1.0)                   # nothing observed: p, r_t and the adjustment count stay
        assert st == {"sum": 0, "count": 0, "calls": 0, "adjustments": 0, "p": 0.25, "r_t": 0.125}


def test_nan_scores_count_in_the_denominator_only():
    score = torch.tensor([0.9, float("nan"), 0.1, 0.9, 0.5, float("nan"), 0.7, 0.51])
    assert A.ada_tally(score) == (3, 8)                                 # 4 above, 1 below, one equal, two NaN
    st = A.ada_new_state(0.0)
    A.ada_reference(st, [A.ada_tally(score)], 1, 0.0, 1.0 / 64, 1.0)
    assert st["r_t"] == 0.375 and st["p"] == 8.0 / 64


def test_interval_counts_calls_across_windows():
    st = A.ada_new_state(0.5)
    seen = []
    for call in range(7):
        A.ada_reference(st, [(2, 4), (-1, 4)], 3, 0.0, 1.0 / 1024, 1.0)
        seen.append((st["sum"], st["count"], st["calls"], st["adjustments"], st["p"]))
    assert seen[0] == (1, 8, 1, 0, 0.5) and seen[1] == (2, 16, 2, 0, 0.5)
    assert seen[2] == (0, 0, 0, 1, 0.5 + 24.0 / 1024) and seen[5] == (0, 0, 0, 2, 0.5 + 48.0 / 1024)
    assert seen[6][:4] == (1, 8, 1, 2)
    assert st["r_t"] == 0.125
    # p and r_t are kept as fp32 values
    st = A.ada_new_state(0.1)
    assert st["p"] == _f32(0.1)
    A.ada_reference(st, [(1, 3)], 1, 0.6, 1e-3, 1.0)
    assert st["r_t"] == _f32(1.0 / 3.0) and st["p"] == _f32(_f32(0.1) - 3 * 1e-3)


def test_controller_rate_and_validation():
    c = A.AdaController(torch.device("cpu"), 3, p=0.2, target=0.6, interval=4, kimg=500.0)
    assert c.rate == 1.0 / (500.0 * 1000.0 * 3) and c.adaptive
    assert c.state.dtype == torch.int32 and c.state.numel() == 16 == L.ADA_STATE_WORDS
    assert float(c.p) == _f32(0.2) and c.p.data_ptr() == c.state.data_ptr() + 4 * L.ADA_P_WORD
    assert c.slot(2).data_ptr() == c.state.data_ptr() + 4 * (L.ADA_SLOT_WORD + 4)
    assert c.sync() == {"p": _f32(0.2), "r_t": 0.0, "adjustments": 0}
    sd = c.state_dict()
    assert sorted(sd) == sorted(A.ADA_WORDS)
    sd.update(p=0.75, adjustments=5, sum=-3, count=9, calls=1, r_t=-0.5)
    c.state[8:].fill_(7)
    c.load_state_dict(sd)
    assert c.state_dict() == sd and float(c.p) == 0.75 and int(c.state[6:].abs().sum()) == 0
    assert not A.AdaController(torch.device("cpu"), 3, p=0.2).adaptive
    for kw in (dict(p=1.5), dict(p=-0.1), dict(p_max=0.0), dict(p_max=1.5), dict(p=0.6, p_max=0.5), dict(interval=0), dict(kimg=0.0),
               dict(target=2.0)):
        with pytest.raises(ValueError):
            A.AdaController(torch.device("cpu"), 3, **kw)
    with pytest.raises(ValueError):
        A.AdaController(torch.device("cpu"), 5)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_arguments_before_any_launch():
    """Every refusal comes before device work, so it can be checked without a GPU (pointers are never followed)."""
    lib = L.load()
    p = ctypes.c_void_p(4096)                                           # a non-null token
    ok = dict(x0=p, x1=None, n0=2, n1=0, u=p, q=p, p=p, policy=7, y=p, C=3, H=8, W=8, ws=p, ws_bytes=1 << 20)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.agan_diffaug_gated_fwd(a["x0"], a["x1"], a["n0"], a["n1"], a["u"], a["q"], a["p"], a["policy"], a["y"], a["C"], a["H"],
                                          a["W"], a["ws"], a["ws_bytes"], None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.agan_diffaug_gated_bwd(a["x0"], a["u"], a["q"], a["p"], a["policy"], a["y"], a["n0"], a["C"], a["H"], a["W"], a["ws"],
                                          a["ws_bytes"], None)

    need = lib.agan_diffaug_ws_bytes(2, 3, 8, 8)
    for call in (fwd, bwd):
        for kw in (dict(q=None), dict(p=None), dict(C=0), dict(C=5), dict(H=0), dict(W=-1), dict(n0=0), dict(policy=8), dict(policy=-1),
                   dict(x0=None), dict(u=None), dict(y=None), dict(ws=None), dict(n0=1 << 20, C=4, H=32, W=16)):
            assert call(**kw) == L.EINVAL, kw
            assert lib.agan_last_error()
        assert call(ws_bytes=need - 1) == L.EWORKSPACE
    assert fwd(n1=-1, x1=p) == L.EINVAL

    def update(state=p, nslots=3, interval=4, target=0.6, rate=1e-6, p_max=1.0):
        return lib.agan_ada_update(state, nslots, interval, target, rate, p_max, None)

    for kw in (dict(state=None), dict(nslots=0), dict(nslots=5), dict(interval=0), dict(rate=-1e-9), dict(rate=float("nan")),
               dict(p_max=0.0), dict(p_max=1.0001), dict(p_max=float("nan")), dict(target=float("nan"))):
        assert update(**kw) == L.EINVAL, kw
        assert lib.agan_last_error()
    for args in ((None, 4, 0.5, p), (p, 4, 0.5, None), (p, 0, 0.5, p), (p, 4, float("nan"), p)):
        assert lib.agan_ada_observe(*args, None) == L.EINVAL, args


# ---- GanTrainStep's constructor ---------------------------------------------------------------------------------------------------
def test_trainer_refuses_a_probability_without_a_policy():
    """The checks come first in the constructor: nothing of the (tiny, host-side) modules is touched before they raise."""
    TR = importlib.import_module("attention-gan_amd.trainers.trainer")
    G = torch.nn.Linear(2, 2)
    Ds = [torch.nn.Linear(2, 1) for _ in range(3)]
    for kw in (dict(augment_p=0.5), dict(ada_target=0.6), dict(augment="", ada_target=0.6), dict(augment=None, augment_p=1.0)):
        with pytest.raises(ValueError, match="augment"):
            TR.GanTrainStep(G, Ds, **kw)
    for kw in (dict(augment_p=1.5), dict(augment_p=-0.5), dict(ada_target=0.6, ada_p_max=0.0), dict(ada_target=0.6, ada_interval=0),
               dict(ada_target=0.6, ada_kimg=0.0), dict(ada_target=0.6, augment_p=0.8, ada_p_max=0.5), dict(ada_target=3.0)):
        with pytest.raises(ValueError, match="AdaController"):
            TR.GanTrainStep(G, Ds, augment="color,cutout", **kw)
