"""CPU tests of the self-attention block (include/agan.h: agan_self_attn_*, agan_scaled_residual_*; backend/functional.py:
self_attention_reference, scaled_residual_reference; utilities/layers.py: SelfAttention2d; networks/generator.py: self_attn): the C ABI
declares and exports the entry points and they refuse bad arguments before any device is touched; the torch references equal a hand
composition in float64 and their autograd gradients equal the closed-form formulas; a generator built with the block under a seed has
every parameter of the plain one and exactly three keys more."""
import importlib
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
SUB = importlib.import_module("attention-gan_amd.networks.generator_submodules")
S4 = importlib.import_module("attention-gan_amd.networks.stage4")
LAY = importlib.import_module("attention-gan_amd.utilities.layers")

NAMES = ["agan_self_attn_fwd", "agan_self_attn_bwd_ws_bytes", "agan_self_attn_bwd", "agan_self_attn_last_launch",
         "agan_scaled_residual_fwd", "agan_scaled_residual_bwd_ws_bytes", "agan_scaled_residual_bwd"]
P = 1                       # a non-null dummy pointer value: validation must fail before it is used
BIG = 1 << 40               # a workspace size that is never the reason for a refusal
NEW_KEYS = {"gen1.self_attn.qkv.weight", "gen1.self_attn.proj.weight", "gen1.self_attn.gamma"}


def test_header_binding_and_makefile_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "agan.h")).read()
    declared = set(re.findall(r"\b(agan_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
    makefile = open(os.path.join(ROOT, "attention-gan_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "self_attn.hip" in srcs
    lib = L.load()
    assert lib.agan_version() == L.ABI_VERSION == 101
    assert re.search(r"#define AGAN_VERSION 101\b", header)


FWD_PTRS = ["q", "k", "v", "o", "lse"]
BWD_PTRS = ["q", "k", "v", "o", "lse", "dout", "dq", "dk", "dv"]
FWD_STRIDES = ["q_bs", "k_bs", "v_bs", "o_bs"]
BWD_STRIDES = ["q_bs", "k_bs", "v_bs", "o_bs", "do_bs", "dq_bs", "dk_bs", "dv_bs"]


def rows_of(name, B, N, M, Dk, Dv):
    """rows x row length of the operand whose batch stride is `name`"""
    return {"q_bs": Dk * N, "k_bs": Dk * M, "v_bs": Dv * M, "o_bs": Dv * N, "do_bs": Dv * N, "dq_bs": Dk * N, "dk_bs": Dk * M,
            "dv_bs": Dv * M}[name]


def fwd(lib, B, N, M, Dk, Dv, scale=1.0, **kw):
    ptrs = [kw.get(n, P) for n in FWD_PTRS]
    strides = [kw.get(n, max(rows_of(n, B, N, M, Dk, Dv), 0)) for n in FWD_STRIDES]
    return lib.agan_self_attn_fwd(*ptrs, B, N, M, Dk, Dv, *strides, scale, None)


def bwd(lib, B, N, M, Dk, Dv, scale=1.0, ws=P, ws_bytes=BIG, **kw):
    ptrs = [kw.get(n, P) for n in BWD_PTRS]
    strides = [kw.get(n, max(rows_of(n, B, N, M, Dk, Dv), 0)) for n in BWD_STRIDES]
    return lib.agan_self_attn_bwd(*ptrs, B, N, M, Dk, Dv, *strides, scale, ws, ws_bytes, None)


ENTRIES = [("self_attn_fwd", fwd), ("self_attn_bwd", bwd)]
# (B, N, M, Dk, Dv): each dimension < 1, Dk = 65, Dv = 129, B * N * max(Dk, Dv) and B * M * max(Dk, Dv) at 2^31
BAD = [(0, 64, 64, 4, 16), (-1, 64, 64, 4, 16), (2, 0, 64, 4, 16), (2, -3, 64, 4, 16), (2, 64, 0, 4, 16), (2, 64, -1, 4, 16),
       (2, 64, 64, 0, 16), (2, 64, 64, -4, 16), (2, 64, 64, 4, 0), (2, 64, 64, 4, -16), (2, 64, 64, 65, 16), (2, 64, 64, 4, 129),
       (1 << 10, 1 << 17, 64, 4, 16), (1 << 10, 64, 1 << 17, 16, 4)]


@pytest.mark.parametrize("dims", BAD, ids=[str(d) for d in BAD])
@pytest.mark.parametrize("name,entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entries_refuse_bad_shapes(name, entry, dims):
    lib = L.load()
    assert entry(lib, *dims) == L.EINVAL
    assert name.encode() in lib.agan_last_error()
    assert lib.agan_self_attn_bwd_ws_bytes(*dims) == 0
    if name == "self_attn_bwd":
        assert entry(lib, *dims, ws_bytes=0) == L.EINVAL              # not "workspace": the shape is refused first
    assert lib.agan_self_attn_last_launch(None, 0) == 0                # nothing was launched


@pytest.mark.parametrize("name,entry", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entries_refuse_a_scale_that_is_not_finite(name, entry):
    lib = L.load()
    for scale in (float("nan"), float("inf"), -float("inf")):
        assert entry(lib, 2, 64, 48, 4, 16, scale=scale) == L.EINVAL
        assert name.encode() + b": scale" in lib.agan_last_error()


@pytest.mark.parametrize("which", FWD_STRIDES)
def test_fwd_refuses_a_short_batch_stride(which):
    lib = L.load()
    dims = (2, 64, 48, 4, 16)
    assert fwd(lib, *dims, **{which: rows_of(which, *dims) - 1}) == L.EINVAL
    assert b"self_attn_fwd: batch stride" in lib.agan_last_error()


@pytest.mark.parametrize("which", BWD_STRIDES)
def test_bwd_refuses_a_short_batch_stride(which):
    lib = L.load()
    dims = (2, 64, 48, 4, 16)
    assert bwd(lib, *dims, **{which: rows_of(which, *dims) - 1}) == L.EINVAL
    assert b"self_attn_bwd: batch stride" in lib.agan_last_error()
    assert bwd(lib, *dims, ws_bytes=0, **{which: rows_of(which, *dims) - 1}) == L.EINVAL


@pytest.mark.parametrize("missing", FWD_PTRS)
def test_fwd_refuses_null_pointers(missing):
    lib = L.load()
    assert fwd(lib, 2, 64, 48, 4, 16, **{missing: None}) == L.EINVAL
    assert b"self_attn_fwd: null pointer" in lib.agan_last_error()


@pytest.mark.parametrize("missing", BWD_PTRS + ["ws"])
def test_bwd_refuses_null_pointers(missing):
    lib = L.load()
    assert bwd(lib, 2, 64, 48, 4, 16, **{missing: None}) == L.EINVAL
    assert b"self_attn_bwd: null pointer" in lib.agan_last_error()


def test_workspace_size_and_a_short_workspace():
    lib = L.load()
    assert lib.agan_self_attn_bwd_ws_bytes(2, 64, 48, 4, 16) == 2 * 64 * 4               # delta: one float per query
    assert lib.agan_self_attn_bwd_ws_bytes(3, 33, 31, 3, 5) == (3 * 33 * 4 + 15) // 16 * 16
    need = lib.agan_self_attn_bwd_ws_bytes(24, 4096, 4096, 4, 16)
    assert need == 24 * 4096 * 4
    for short in (0, need - 1):
        assert bwd(lib, 24, 4096, 4096, 4, 16, ws_bytes=short) == L.EWORKSPACE
        msg = lib.agan_last_error()
        assert b"self_attn_bwd: workspace" in msg and str(need).encode() in msg
    assert lib.agan_self_attn_last_launch(None, 0) == 0


def test_the_gate_entries_refuse_bad_arguments():
    lib = L.load()
    assert lib.agan_scaled_residual_fwd(P, P, P, P, 0, None) == L.EINVAL
    assert b"scaled_residual_fwd" in lib.agan_last_error()
    for i in range(4):
        ptrs = [P] * 4
        ptrs[i] = None
        assert lib.agan_scaled_residual_fwd(*ptrs, 64, None) == L.EINVAL
        assert b"scaled_residual_fwd: null pointer" in lib.agan_last_error()
    assert lib.agan_scaled_residual_bwd_ws_bytes(0) == 0
    assert lib.agan_scaled_residual_bwd(P, P, P, P, P, 0, 0, P, BIG, None) == L.EINVAL
    assert lib.agan_scaled_residual_bwd(P, P, P, P, P, 0, 0, P, 0, None) == L.EINVAL
    assert b"scaled_residual_bwd" in lib.agan_last_error()
    for i in range(5):
        ptrs = [P] * 5
        ptrs[i] = None
        assert lib.agan_scaled_residual_bwd(*ptrs, 64, 0, P, BIG, None) == L.EINVAL
        assert b"scaled_residual_bwd: null pointer" in lib.agan_last_error()
    assert lib.agan_scaled_residual_bwd(P, P, P, P, P, 64, 0, None, BIG, None) == L.EINVAL
    # one fp64 partial per workgroup of 1024 elements, at most 1024 workgroups
    assert lib.agan_scaled_residual_bwd_ws_bytes(1) == 16
    assert lib.agan_scaled_residual_bwd_ws_bytes(4097) == 5 * 8 + 8
    assert lib.agan_scaled_residual_bwd_ws_bytes(1 << 30) == 1024 * 8
    need = lib.agan_scaled_residual_bwd_ws_bytes(300000)
    for short in (0, need - 1):
        assert lib.agan_scaled_residual_bwd(P, P, P, P, P, 300000, 0, P, short, None) == L.EWORKSPACE
        assert b"scaled_residual_bwd: workspace" in lib.agan_last_error()
    assert lib.agan_self_attn_last_launch(None, 0) == 0


# ------------------------------------------------------------------------------------------------------- the torch references
def hand(q, k, v, scale):
    """the issue's formulas with explicit loops over the batch, in the operands' dtype -> (o, p)"""
    B, Dk, N = q.shape
    os_, ps = [], []
    for b in range(B):
        s = scale * (q[b].t() @ k[b])                                  # [N, M]
        e = torch.exp(s - s.max(dim=1, keepdim=True).values)
        p = e / e.sum(dim=1, keepdim=True)
        os_.append(v[b] @ p.t())                                       # [Dv, N]
        ps.append(p)
    return torch.stack(os_), torch.stack(ps)


@pytest.mark.parametrize("dims,scale", [((2, 5, 7, 3, 4), 1.0), ((3, 16, 9, 1, 2), 0.4), ((1, 1, 6, 2, 3), -1.5)])
def test_self_attention_reference_and_its_gradients(dims, scale):
    B, N, M, Dk, Dv = dims
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(s, generator=g, dtype=torch.float64, requires_grad=True) for s in ((B, Dk, N), (B, Dk, M), (B, Dv, M)))
    do = torch.randn((B, Dv, N), generator=g, dtype=torch.float64)
    o = HF.self_attention_reference(q, k, v, scale)
    o_hand, p = hand(q.detach(), k.detach(), v.detach(), scale)
    assert o.shape == (B, Dv, N) and o.dtype == torch.float64
    assert (o - o_hand).abs().max().item() < 1e-12
    dq, dk, dv = torch.autograd.grad(o, (q, k, v), do)
    delta = (do * o_hand).sum(dim=1)                                   # [B, N]
    dp = do.transpose(1, 2) @ v.detach()                               # [B, N, M]
    ds = p * (dp - delta.unsqueeze(2))
    assert (dq - scale * (k.detach() @ ds.transpose(1, 2))).abs().max().item() < 1e-12
    assert (dk - scale * (q.detach() @ ds)).abs().max().item() < 1e-12
    assert (dv - do @ p).abs().max().item() < 1e-12


def test_self_attention_reference_takes_maps_and_refuses_misfits():
    q, k, v = torch.randn(2, 3, 4, 5), torch.randn(2, 3, 2, 3), torch.randn(2, 6, 2, 3)
    o = HF.self_attention_reference(q, k, v, 0.5)
    assert o.shape == (2, 6, 4, 5) and o.dtype == torch.float32
    flat = HF.self_attention_reference(q.reshape(2, 3, 20), k.reshape(2, 3, 6), v.reshape(2, 6, 6), 0.5)
    assert torch.equal(o.reshape(2, 6, 20), flat)
    with pytest.raises(ValueError):
        HF.self_attention_reference(q, torch.randn(2, 4, 2, 3), v)
    with pytest.raises(ValueError):
        HF.self_attention_reference(q, k, torch.randn(2, 6, 7))
    with pytest.raises(L.AganError):
        HF.self_attention(q, k, v)                                     # no CPU fallback


def test_scaled_residual_reference_and_its_gradients():
    g0 = torch.Generator().manual_seed(5)
    x, y = (torch.randn((3, 4, 5), generator=g0, dtype=torch.float64, requires_grad=True) for _ in range(2))
    g = torch.tensor([0.7], dtype=torch.float64, requires_grad=True)
    do = torch.randn((3, 4, 5), generator=g0, dtype=torch.float64)
    out = HF.scaled_residual_reference(x, y, g)
    assert (out - (x.detach() + 0.7 * y.detach())).abs().max().item() < 1e-12
    dx, dy, dg = torch.autograd.grad(out, (x, y, g), do)
    assert torch.equal(dx, do)
    assert (dy - 0.7 * do).abs().max().item() < 1e-12
    assert abs(dg.item() - (do * y.detach()).sum().item()) < 1e-12


# ------------------------------------------------------------------------------------------------------- construction
def test_the_block_has_three_keys_and_starts_closed():
    blk = LAY.SelfAttention2d(64)
    assert (blk.dk, blk.dv) == (8, 32)
    sd = blk.state_dict()
    assert set(sd) == {"qkv.weight", "proj.weight", "gamma"}
    assert sd["qkv.weight"].shape == (48, 64, 1, 1) and sd["proj.weight"].shape == (64, 32, 1, 1)
    assert sd["gamma"].shape == (1,) and sd["gamma"].item() == 0.0
    small = LAY.SelfAttention2d(4)
    assert (small.dk, small.dv) == (1, 2)


@pytest.mark.parametrize("at", [32, 64])
def test_generator_with_the_block_keeps_every_plain_parameter(at):
    torch.manual_seed(7)
    plain = GEN.Generator(4, 16, 10, 10).state_dict()
    torch.manual_seed(7)
    gen = GEN.Generator(4, 16, 10, 10, self_attn=at)
    sd = gen.state_dict()
    assert set(sd) - set(plain) == NEW_KEYS and set(plain) <= set(sd)
    for key, value in plain.items():
        assert torch.equal(sd[key], value), key
    assert sd["gen1.self_attn.gamma"].item() == 0.0
    channels = 8 if at == 32 else 4
    assert sd["gen1.self_attn.qkv.weight"].shape[1] == channels and sd["gen1.self_attn.proj.weight"].shape[0] == channels
    assert sd["gen1.self_attn.qkv.weight"].abs().sum().item() > 0 and sd["gen1.self_attn.proj.weight"].abs().sum().item() > 0
    report = gen.load_state_dict(plain, strict=False)
    assert set(report.missing_keys) == NEW_KEYS and not report.unexpected_keys


def test_other_generators_and_refusals():
    with pytest.raises(ValueError):
        GEN.Generator(4, 16, 10, 10, self_attn=16)
    with pytest.raises(ValueError):
        GEN.Generator1(4, 16, 10, 10, self_attn=128)
    with pytest.raises(ValueError):
        SUB.GenInitialStage(64, 10, 10, self_attn=0)
    assert len(GEN.Generator(32, 256, 100, 100).state_dict()) == 97
    for cls in (GEN.Generator1, S4.Generator4):
        torch.manual_seed(7)
        plain = cls(4, 16, 10, 10).state_dict()
        torch.manual_seed(7)
        sd = cls(4, 16, 10, 10, self_attn=64).state_dict()
        assert set(sd) - set(plain) == NEW_KEYS
        assert all(torch.equal(sd[key], value) for key, value in plain.items())
    stage = SUB.GenInitialStage(64, 10, 10, self_attn=32)
    assert stage.self_attn.channels == 8 and set(k for k in stage.state_dict() if k.startswith("self_attn.")) == \
        {"self_attn.qkv.weight", "self_attn.proj.weight", "self_attn.gamma"}
    assert SUB.GenInitialStage(64, 10, 10).self_attn is None
