"""The gated augmentation kernels (agan_diffaug_gated_*, backend.functional.diffaug with q and p) against the gated
augment.diffaug_reference, and the controller kernels (agan_ada_observe / agan_ada_update) against augment.ada_tally / ada_reference.

Shapes: eight samples, so that every one of the eight gate masks occurs in ONE call (sample n passes the gates of the bits of n);
[8, 3, 5, 7] and [8, 1, 5, 7] take the one-pixel path, [8, 3, 8, 12] and [8, 4, 24, 40] the 16-byte path, [9, 3, 64, 64] needs three
partial sums per sample, and [8, 3, 8, 12] once more from a base one float off the 16-byte grid (one-pixel path with W % 4 == 0).

A sample whose colour gate is off is only moved: it must EQUAL the oracle, -0.0 included.  With colour on the bound is DESIGN.md
section 15's: |y - ref64| <= 64 * 2^-24 (max|x| + 0.5) and |dx - ref64| <= 64 * 2^-24 max|dy| per sample.  Measured on MI355X over
all of these (the checks print every figure): at most 0.052 of the forward bound and 0.050 of the backward bound.
"""
import ctypes
import importlib
import struct

import pytest
import torch

pytestmark = pytest.mark.gpu

A = importlib.import_module("attention-gan_amd.augment")
HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")

DEV = torch.device("cuda", 0)
SHAPES = [(8, 3, 5, 7), (8, 1, 5, 7), (8, 3, 8, 12), (8, 4, 24, 40), (9, 3, 64, 64)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
BOUND = 64 * 2.0 ** -24
P = 0.5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mask_q(N, p=P):
    """q [N, 4]: sample n passes exactly the gates of the bits of n % 8 at probability p"""
    q = torch.empty(N, 4)
    for n in range(N):
        for k in range(3):
            q[n, k] = 0.25 * p if n >> k & 1 else 1.5 * p
    q[:, 3] = 0.0
    return q


def _case(shape, seed, off_grid=False):
    """(x, r, u) on the device, -0.0 among x and r; off_grid: both start one float past a 16-byte boundary"""
    g = _gen(seed)
    n = 1
    for s in shape:
        n *= s
    out = []
    for _ in range(2):
        flat = torch.randn(n + 1, generator=g)
        flat[1], flat[n] = -0.0, -0.0
        t = flat.to(DEV)
        t = t[1:].view(shape) if off_grid else t[1:].clone().view(shape)
        assert (t.data_ptr() % 16 != 0) == off_grid
        out.append(t)
    return out[0], out[1], torch.rand(shape[0], 8, generator=g).to(DEV)


def _p(value):
    return torch.tensor([value], dtype=torch.float32, device=DEV)


def _both(x, u, policy, r, q=None, p=None):
    """(y, dx) of the kernels for upstream gradient r"""
    x = x.detach().requires_grad_(True)
    y = HF.diffaug(x, u, policy, q, p)
    y.backward(r)
    return y.detach(), x.grad


def _ref(x, u, policy, r, q=None, p=None):
    x = x.detach().clone().requires_grad_(True)
    y = A.diffaug_reference(x, u, policy, q, p)
    y.backward(r)
    return y.detach(), x.grad


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_against_the_oracle(x, r, u, q, p, policy):
    """colour-off samples equal the fp32 oracle; colour-on samples stay inside the bound against the float64 oracle"""
    y, dx = _both(x, u, policy, r, q, p)
    y32, dx32 = _ref(x, u, policy, r, q, p)
    y64, dx64 = _ref(x.double().cpu(), u.cpu(), policy, r.double().cpu(), q.cpu(), p.cpu())
    colour = (A.gate_masks(q, p)[:, 0] & bool(policy & A.COLOR)).cpu()
    off = ~colour
    assert torch.equal(y[off.to(DEV)], y32[off.to(DEV)]), "forward, colour-off samples"
    assert torch.equal(dx[off.to(DEV)], dx32[off.to(DEV)]), "backward, colour-off samples"
    if bool(colour.any()):
        lim_y = BOUND * (x.abs().amax(dim=(1, 2, 3)).cpu().double() + 0.5)
        lim_dx = BOUND * r.abs().amax(dim=(1, 2, 3)).cpu().double()
        err_y = (y.cpu().double() - y64).abs().amax(dim=(1, 2, 3))
        err_dx = (dx.cpu().double() - dx64).abs().amax(dim=(1, 2, 3))
        print(f"gated diffaug {tuple(x.shape)} policy {policy}: forward {float((err_y / lim_y)[colour].max()):.4f} of the bound, "
              f"backward {float((err_dx / lim_dx)[colour].max()):.4f}")
        assert bool((err_y <= lim_y)[colour].all()), f"forward: {err_y.tolist()} > {lim_y.tolist()}"
        assert bool((err_dx <= lim_dx)[colour].all()), f"backward: {err_dx.tolist()} > {lim_dx.tolist()}"
    return y, dx


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_p_zero_moves_the_bits_and_p_one_is_the_ungated_call(shape):
    x, r, u = _case(shape, sum(shape))
    q = torch.rand(shape[0], 4, generator=_gen(1)).to(DEV)
    for policy in (7, 6, 1):
        for p in (0.0, float("nan")):
            y, dx = _both(x, u, policy, r, q, _p(p))
            assert torch.equal(_bits(y), _bits(x)) and torch.equal(_bits(dx), _bits(r)), (policy, p)
        y, dx = _both(x, u, policy, r, q, _p(1.0))
        y_u, dx_u = _both(x, u, policy, r)
        assert torch.equal(_bits(y), _bits(y_u)) and torch.equal(_bits(dx), _bits(dx_u)), policy
    assert int((_bits(x) == -2 ** 31).sum()) >= 1                          # -0.0 was among the inputs


@pytest.mark.parametrize("policy", [7, 5, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_gate_mask_in_one_call(shape, policy):
    x, r, u = _case(shape, sum(shape) + policy)
    q = _mask_q(shape[0]).to(DEV)
    assert A.gate_masks(q, P)[:8].tolist() == [[bool(n >> k & 1) for k in range(3)] for n in range(8)]
    y, dx = _check_against_the_oracle(x, r, u, q, _p(P), policy)
    assert torch.equal(_bits(y[0]), _bits(x[0])) and torch.equal(_bits(dx[0]), _bits(r[0]))      # sample 0: every gate off
    # random gates at another probability
    _check_against_the_oracle(x, r, u, torch.rand(shape[0], 4, generator=_gen(2)).to(DEV), _p(0.3), policy)


def test_a_base_one_float_off_the_16_byte_grid():
    shape = (8, 3, 8, 12)
    x, r, u = _case(shape, 5, off_grid=True)
    q = _mask_q(8).to(DEV)
    y, dx = _check_against_the_oracle(x, r, u, q, _p(P), 7)
    ya, dxa = _both(x.clone(), u, 6, r.clone(), q, _p(P))                  # without colour both access paths give the same bits
    yo, dxo = _both(x, u, 6, r, q, _p(P))
    assert torch.equal(_bits(ya), _bits(yo)) and torch.equal(_bits(dxa), _bits(dxo))


@pytest.mark.parametrize("shape", [(8, 3, 5, 7), (8, 3, 8, 12)], ids=["pixel", "vec"])
def test_edge_of_the_compare(shape):
    """q == p is off, the fp32 just below p is on"""
    x, r, u = _case(shape, 7)
    p32 = float(torch.tensor(0.3, dtype=torch.float32))
    below = float(torch.nextafter(torch.tensor(p32, dtype=torch.float32), torch.tensor(0.0)))
    q = torch.full((shape[0], 4), p32)
    q[1::2, :3] = below
    q = q.to(DEV)
    y, dx = _check_against_the_oracle(x, r, u, q, _p(p32), 7)
    y_u, dx_u = _both(x, u, 7, r)
    assert torch.equal(_bits(y[0::2]), _bits(x[0::2])) and torch.equal(_bits(dx[0::2]), _bits(r[0::2]))
    assert torch.equal(_bits(y[1::2]), _bits(y_u[1::2])) and torch.equal(_bits(dx[1::2]), _bits(dx_u[1::2]))


@pytest.mark.parametrize("shape", [(4, 3, 5, 7), (4, 3, 8, 12), (3, 3, 64, 64)], ids=["pixel", "vec", "partials"])
def test_pair_form_with_different_gates_in_the_halves(shape):
    N = shape[0]
    g = _gen(sum(shape) + 300)
    a0, b0 = torch.randn(shape, generator=g).to(DEV), torch.randn(shape, generator=g).to(DEV)
    u = torch.rand(2 * N, 8, generator=g).to(DEV)
    r = torch.randn((2 * N,) + shape[1:], generator=g).to(DEV)
    q = torch.cat([torch.full((N, 4), 0.1), _mask_q(N)]).to(DEV)     # first half: every gate on; second: masks 0..N-1
    p = _p(P)
    whole = torch.cat([a0, b0]).requires_grad_(True)
    y_cat = HF.diffaug(whole, u, 7, q, p)
    y_cat.backward(r)
    y_u, _ = _both(torch.cat([a0, b0]), u, 7, r)
    assert torch.equal(_bits(y_cat[:N]), _bits(y_u[:N])) and torch.equal(_bits(y_cat[N]), _bits(b0[0]))
    a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    y = HF.diffaug((a, b), u, 7, q, p)
    assert torch.equal(_bits(y), _bits(y_cat))
    y.backward(r)
    assert torch.equal(_bits(a.grad), _bits(whole.grad[:N])) and torch.equal(_bits(b.grad), _bits(whole.grad[N:]))
    for first in (True, False):                                          # one source asks: its samples' gates go with it
        a, b = a0.clone().requires_grad_(first), b0.clone().requires_grad_(not first)
        HF.diffaug((a, b), u, 7, q, p).backward(r)
        want, idle = (a, b) if first else (b, a)
        assert idle.grad is None
        assert torch.equal(_bits(want.grad), _bits(whole.grad[:N] if first else whole.grad[N:]))


def _raw(name, *args):
    return getattr(L.load(), name)(*args)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_calls_give_the_same_bytes_with_a_poisoned_workspace(shape):
    """... which also shows that the partial sums of a sample whose colour gate is off are never read"""
    N, C, H, W = shape
    x, r, u = _case(shape, sum(shape) + 400)
    q, p = _mask_q(N).to(DEV), _p(P)
    nbytes = L.load().agan_diffaug_ws_bytes(N, C, H, W)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    st = HF._stream()
    outs = []
    for fill in (float("nan"), 1e30):
        y, dx = torch.empty_like(x), torch.empty_like(x)
        ws.fill_(fill)
        assert _raw("agan_diffaug_gated_fwd", _ptr(x), None, N, 0, _ptr(u), _ptr(q), _ptr(p), 7, _ptr(y), C, H, W, _ptr(ws), nbytes, st) == 0
        ws.fill_(fill)
        assert _raw("agan_diffaug_gated_bwd", _ptr(r), _ptr(u), _ptr(q), _ptr(p), 7, _ptr(dx), N, C, H, W, _ptr(ws), nbytes, st) == 0
        outs.append((y, dx))
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0])) and torch.equal(_bits(outs[0][1]), _bits(outs[1][1]))
    assert bool(torch.isfinite(outs[0][0]).all()) and bool(torch.isfinite(outs[0][1]).all())
    y_f, dx_f = _both(x, u, 7, r, q, p)                                   # and they are what the autograd bridge returns
    assert torch.equal(_bits(outs[0][0]), _bits(y_f)) and torch.equal(_bits(outs[0][1]), _bits(dx_f))


def test_p_is_read_on_the_device_when_the_kernel_runs():
    """one gated call captured into a graph; p changed in place; the replay follows the new p without a re-capture"""
    shape = (8, 3, 8, 12)
    x, r, u = _case(shape, 9)
    q, p = _mask_q(8).to(DEV), _p(0.0)
    want = {v: _both(x, u, 7, r, q, _p(v))[0] for v in (0.0, P, 1.0)}
    assert not torch.equal(want[0.0], want[P]) and not torch.equal(want[P], want[1.0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        HF.diffaug(x, u, 7, q, p)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y = HF.diffaug(x, u, 7, q, p)
    for v in (P, 1.0, 0.0, P):
        p.fill_(v)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(want[v])), v


def test_argument_checks():
    N, C, H, W = 2, 3, 8, 8
    x = torch.zeros(N, C, H, W, device=DEV)
    u, q, p = torch.rand(N, 8, device=DEV), torch.rand(N, 4, device=DEV), _p(0.5)
    with pytest.raises(ValueError):
        HF.diffaug(x, u, 7, q)                                            # q without p
    with pytest.raises(ValueError):
        HF.diffaug(x, u, 7, q[:, :3], p)
    with pytest.raises(ValueError):
        HF.diffaug(x, u, 7, q, torch.zeros(2, device=DEV))
    with pytest.raises(ValueError):
        HF.diffaug(x, u, 7, q, p.cpu())
    with pytest.raises(ValueError):
        HF.diffaug(x, u, 7, q, p.double())


# ---- the controller -------------------------------------------------------------------------------------------------------------
def _f32_bits(v):
    return struct.unpack("<i", struct.pack("<f", v))[0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_observe_counts_in_integers(n):
    g = _gen(n)
    score = torch.rand(n, generator=g)
    score[torch.rand(n, generator=g) < 0.2] = 0.5                          # equal to the threshold: neither above nor below
    score[torch.rand(n, generator=g) < 0.1] = float("nan")
    if n >= 63:
        score[0], score[1], score[n - 1] = float("nan"), 0.5, 0.75
    state = torch.full((16,), 12345, dtype=torch.int32, device=DEV)
    for i, (s, thr) in enumerate(((score, 0.5), (score, 0.25), (-score, -0.5), (torch.ones(n), 0.5))):
        HF.ada_observe_(s.to(DEV), state[8 + 2 * i:10 + 2 * i], thr)
    got = state.cpu().tolist()
    assert got[:8] == [12345] * 8                                         # written, not accumulated, and nothing else touched
    for i, (s, thr) in enumerate(((score, 0.5), (score, 0.25), (-score, -0.5), (torch.ones(n), 0.5))):
        assert tuple(got[8 + 2 * i:10 + 2 * i]) == A.ada_tally(s, thr), (i, thr)
    assert tuple(got[14:16]) == (n, n)
    assert got[8] == -got[12]


@pytest.mark.parametrize("nslots,interval", [(1, 1), (2, 2), (3, 4), (4, 2), (3, 1), (4, 4)])
def test_forty_updates_equal_the_reference(nslots, interval):
    """integer words equal, p and r_t equal as fp32 bits; p moves both ways and meets both clamps"""
    g = _gen(10 * nslots + interval)
    target, rate, p_max = 0.1, 1.0 / 97.0, 0.8
    ctl = A.AdaController(DEV, nslots, p=0.3, target=target, interval=interval, kimg=1.0, p_max=p_max)
    ctl.rate = rate
    ref = A.ada_new_state(0.3)
    seen = []
    for call in range(40):
        lean = 0.8 if call < 14 else (0.2 if call < 32 else 0.5)          # mostly above, then mostly below, then mixed
        slots = []
        for i in range(nslots):
            if float(torch.rand((), generator=g)) < 0.25 or call in (20, 21, 22, 23):
                slots.append(None)                                        # this discriminator did not observe (calls 20..23: nobody did)
                continue
            n = int(torch.randint(1, 40, (), generator=g))
            score = (torch.rand(n, generator=g) < lean).float() * 0.8 + 0.1
            score[torch.rand(n, generator=g) < 0.1] = float("nan")
            ctl.observe(i, score.to(DEV))
            slots.append(A.ada_tally(score))
        ctl.update()
        A.ada_reference(ref, slots, interval, target, rate, p_max)
        words = ctl.state.cpu().tolist()
        assert words[:4] == [ref["sum"], ref["count"], ref["calls"], ref["adjustments"]], call
        assert words[4] == _f32_bits(ref["p"]) and words[5] == _f32_bits(ref["r_t"]), (call, ref)
        assert words[6:] == [0] * 10, call                                # reserved words untouched, slots emptied
        seen.append(ref["p"])
    assert ctl.state_dict() == ref and ctl.sync() == {"p": ref["p"], "r_t": ref["r_t"], "adjustments": ref["adjustments"]}
    assert max(seen) == struct.unpack("<f", struct.pack("<f", p_max))[0] and min(seen) == 0.0
    assert 1 <= ref["adjustments"] <= (36 if interval == 1 else 40 // interval)      # (calls 20..23 are empty windows of interval 1)
