"""CPU tests of the channel-wise word attention (include/agan.h: agan_chan_attn_*; backend/functional.py:
channel_attention_reference; networks/attention.py: ChannelAttention; networks/generator.py: channel_attn): the C ABI declares and
exports the entry points and they refuse bad arguments before any device is touched; the torch reference equals a hand-written
per-channel loop in float64 and its autograd gradients equal the closed forms; a channel-attention generator has exactly the new
keys at the wider channel plan and the plain generator is untouched."""
import importlib
import math
import os
import re

import pytest
import torch

from channel_attn_cases import channel_attention_oracle, mask_of, stage_input_oracle
from oracle import attngan_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")
GEN = importlib.import_module("attention-gan_amd.networks.generator")
SUB = importlib.import_module("attention-gan_amd.networks.generator_submodules")
S4 = importlib.import_module("attention-gan_amd.networks.stage4")
ATT = importlib.import_module("attention-gan_amd.networks.attention")

NAMES = ["agan_chan_attn_fwd_ws_bytes", "agan_chan_attn_fwd", "agan_chan_attn_bwd_ws_bytes", "agan_chan_attn_bwd"]
P = 1                       # a non-null dummy pointer value: validation must fail before it is used
BIG = 1 << 40               # a workspace size that is never the reason for a refusal


def test_header_binding_and_makefile_declare_the_entry_points():
    header = open(os.path.join(ROOT, "include", "agan.h")).read()
    declared = set(re.findall(r"\b(agan_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS, name
    makefile = open(os.path.join(ROOT, "attention-gan_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "chan_attn.hip" in srcs
    lib = L.load()
    assert lib.agan_version() == L.ABI_VERSION == 101
    assert re.search(r"#define AGAN_VERSION 101\b", header)


# ------------------------------------------------------------------------------------------------------------- refusals
F_PTRS = ["h", "wt", "mask", "alpha", "f"]
B_PTRS = ["h", "wt", "alpha", "df", "dalpha_out", "dh", "dwt"]


def fwd(lib, B, C, T, HW, ws=P, ws_bytes=BIG, **kw):
    a = {n: kw.get(n, P) for n in F_PTRS}
    return lib.agan_chan_attn_fwd(a["h"], a["wt"], a["mask"], 0.5, a["alpha"], a["f"], B, C, T, HW, ws, ws_bytes, None)


def bwd(lib, B, C, T, HW, ws=P, ws_bytes=BIG, **kw):
    a = {n: kw.get(n, P) for n in B_PTRS}
    return lib.agan_chan_attn_bwd(a["h"], a["wt"], a["alpha"], a["df"], a["dalpha_out"], 0.5, a["dh"], a["dwt"], B, C, T, HW, ws,
                                  ws_bytes, None)


ENTRIES = [("chan_attn_fwd", fwd, F_PTRS), ("chan_attn_bwd", bwd, B_PTRS)]
# (B, C, T, HW): each dimension < 1, C = 65, T = 65, B * C * HW at 2^31 (2^10 * 2^4 * 2^17), B * T * HW at 2^31, B = 65536
BAD = [(0, 4, 5, 36), (-3, 4, 5, 36), (2, 0, 5, 36), (2, -4, 5, 36), (2, 4, 0, 36), (2, 4, -5, 36), (2, 4, 5, 0), (2, 4, 5, -36),
       (2, 65, 5, 36), (2, 4, 65, 36), (1 << 10, 16, 5, 1 << 17), (1 << 10, 1, 16, 1 << 17), (1 << 16, 1, 1, 1)]


@pytest.mark.parametrize("dims", BAD, ids=[str(d) for d in BAD])
@pytest.mark.parametrize("name,entry,_", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entries_refuse_bad_shapes(name, entry, _, dims):
    lib = L.load()
    assert entry(lib, *dims) == L.EINVAL
    assert lib.agan_last_error().startswith(name.encode() + b":")
    assert lib.agan_chan_attn_fwd_ws_bytes(*dims) == 0 and lib.agan_chan_attn_bwd_ws_bytes(*dims) == 0
    assert entry(lib, *dims, ws_bytes=0) == L.EINVAL                  # not "workspace": the shape is refused first


def test_the_largest_shapes_below_the_limits_pass_validation():
    """one element under 2^31 is a shape, not a refusal: the size queries answer (nothing is launched by a query)"""
    lib = L.load()
    assert lib.agan_chan_attn_fwd_ws_bytes(1 << 10, 16, 5, (1 << 17) - 1) > 0
    assert lib.agan_chan_attn_bwd_ws_bytes(1 << 10, 1, 16, (1 << 17) - 1) > 0
    assert lib.agan_chan_attn_fwd_ws_bytes(65535, 1, 1, 1) == 65535 * 4
    assert lib.agan_chan_attn_fwd_ws_bytes(2, 64, 64, 49) == 2 * 1 * 64 * 64 * 4


@pytest.mark.parametrize("name,entry,ptrs", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_entries_refuse_null_pointers(name, entry, ptrs):
    lib = L.load()
    dims = (2, 4, 5, 36)
    for missing in ptrs + ["ws"]:
        if missing == "dalpha_out":                                 # optional: NULL is no gradient at the returned alpha
            assert entry(lib, *dims, dalpha_out=None, h=None) == L.EINVAL
            continue
        if missing in ("dh", "dwt"):                                # one of the two may be NULL (that gradient is not wanted) ...
            assert entry(lib, *dims, **{missing: None}, ws_bytes=0) == L.EWORKSPACE     # ... so validation goes on to the workspace
            continue
        assert entry(lib, *dims, **{missing: None}) == L.EINVAL, missing
        assert lib.agan_last_error() == name.encode() + b": null pointer", missing
    if name == "chan_attn_bwd":                                     # ... but not both
        assert entry(lib, *dims, dh=None, dwt=None) == L.EINVAL
        assert lib.agan_last_error() == b"chan_attn_bwd: null pointer"


def test_workspace_sizes_and_a_short_workspace():
    lib = L.load()
    # forward: one [C, T] score slab per sample and workgroup of 256 pixels; backward: a dalpha slab each, and scale * dm [B, C, T]
    assert lib.agan_chan_attn_fwd_ws_bytes(3, 4, 5, 36) == 3 * 1 * 20 * 4
    assert lib.agan_chan_attn_bwd_ws_bytes(3, 4, 5, 36) == (3 * 1 * 20 + 3 * 20) * 4
    assert lib.agan_chan_attn_fwd_ws_bytes(3, 64, 17, 324) == 3 * 2 * 64 * 17 * 4
    assert lib.agan_chan_attn_fwd_ws_bytes(3, 8, 33, 256) == 3 * 1 * 8 * 33 * 4
    for entry, query in ((fwd, lib.agan_chan_attn_fwd_ws_bytes), (bwd, lib.agan_chan_attn_bwd_ws_bytes)):
        need = query(24, 32, 18, 128 * 128)
        assert need == (24 * 64 * 32 * 18 + (24 * 32 * 18 if entry is bwd else 0)) * 4
        name = b"chan_attn_fwd" if entry is fwd else b"chan_attn_bwd"
        for short in (0, need - 1):
            assert entry(lib, 24, 32, 18, 128 * 128, ws_bytes=short) == L.EWORKSPACE
            msg = lib.agan_last_error()
            assert msg.startswith(name + b": workspace") and str(need).encode() in msg


def test_the_function_has_no_cpu_fallback_and_checks_shapes():
    h, wt, mask = torch.randn(2, 3, 4, 4), torch.randn(2, 5, 16), torch.ones(2, 5, dtype=torch.int64)
    with pytest.raises(L.AganError):
        HF.channel_attention(h, wt, mask, None)
    for fn in (HF.channel_attention, HF.channel_attention_reference):
        with pytest.raises(ValueError):
            fn(h, wt[:, :, :-1], mask, None)                        # wt is not H * W long
        with pytest.raises(ValueError):
            fn(h, wt, mask[:, :-1], None)
        with pytest.raises(ValueError):
            fn(h, wt[:1], mask, None)
        with pytest.raises(ValueError):
            fn(h.reshape(2, 3, 16), wt, mask, None)


# ------------------------------------------------------------------------------------------------------- the torch reference
def _case():
    B, C, T, H, W = 2, 3, 4, 2, 3
    g0 = torch.Generator().manual_seed(17)
    mk = lambda *s: torch.randn(*s, generator=g0, dtype=torch.float64)      # noqa: E731
    return mk(B, C, H, W), mk(B, T, H * W), mask_of([T, 2], T), mk(B, C, H, W), mk(B, C, T)


@pytest.mark.parametrize("scale", [None, 1.0, 0.37])
def test_channel_attention_reference_equals_a_per_channel_loop(scale):
    h, wt, mask, _, _ = _case()
    B, C, H, W = h.shape
    T, N = wt.shape[1], H * W
    f, alpha = HF.channel_attention_reference(h, wt, mask, scale)
    assert f.shape == (B, C, H, W) and alpha.shape == (B, C, T) and f.dtype == torch.float64
    s = 1.0 / math.sqrt(N) if scale is None else scale
    hf = h.reshape(B, C, N)
    for b in range(B):
        for c in range(C):
            m = [s * sum(float(hf[b, c, p]) * float(wt[b, t, p]) for p in range(N)) if int(mask[b, t]) else -math.inf for t in range(T)]
            mx = max(m)
            e = [math.exp(v - mx) for v in m]
            a = [v / sum(e) for v in e]
            for t in range(T):
                assert abs(float(alpha[b, c, t]) - a[t]) < 1e-12
            for p in range(N):
                assert abs(float(f.reshape(B, C, N)[b, c, p]) - sum(a[t] * float(wt[b, t, p]) for t in range(T))) < 1e-12
    assert float(alpha[1, :, 2:].abs().max()) == 0.0                 # masked words get exactly zero


@pytest.mark.parametrize("with_dalpha", [False, True])
def test_channel_attention_reference_gradients_equal_the_closed_forms(with_dalpha):
    h, wt, mask, df, dalpha_out = _case()
    B, C, H, W = h.shape
    T, N = wt.shape[1], H * W
    scale = 0.6
    leaves = [t.clone().requires_grad_(True) for t in (h, wt)]
    f, alpha = HF.channel_attention_reference(leaves[0], leaves[1], mask, scale)
    outs, gouts = ((f, alpha), (df, dalpha_out)) if with_dalpha else ((f,), (df,))
    dh, dwt = torch.autograd.grad(outs, leaves, gouts)
    a, hf, dff = alpha.detach(), h.reshape(B, C, N), df.reshape(B, C, N)
    dalpha = torch.bmm(dff, wt.transpose(1, 2))                      # [B, C, T]
    if with_dalpha:
        dalpha = dalpha + dalpha_out
    dm = a * (dalpha - (a * dalpha).sum(dim=2, keepdim=True))
    want_dh = scale * torch.bmm(dm, wt)                              # [B, C, N]
    want_dwt = torch.bmm(a.transpose(1, 2), dff) + scale * torch.bmm(dm.transpose(1, 2), hf)
    assert float(want_dh.abs().max()) > 0 and float(want_dwt.abs().max()) > 0
    assert (dh.reshape(B, C, N) - want_dh).abs().max().item() < 1e-12
    assert (dwt - want_dwt).abs().max().item() < 1e-12
    assert float(dm[1, :, 2:].abs().max()) == 0.0                    # a masked word takes no score gradient


def test_a_single_live_word_is_read_back_for_every_channel():
    h, wt, _, _, _ = _case()
    B, C, H, W = h.shape
    T = wt.shape[1]
    f, alpha = HF.channel_attention_reference(h, wt, mask_of([1, T], T), None)
    assert torch.equal(alpha[0, :, 0], torch.ones(C, dtype=torch.float64)) and float(alpha[0, :, 1:].abs().max()) == 0.0
    for c in range(C):
        assert torch.equal(f[0, c].reshape(-1), wt[0, 0])
    # a sample with every word masked gives NaN, as the other attention modules do
    f, alpha = HF.channel_attention_reference(h, wt, mask_of([0, T], T), None)
    assert bool(torch.isnan(alpha[0]).all()) and bool(torch.isnan(f[0]).all()) and bool(torch.isfinite(f[1]).all())


def test_the_oracle_composition_is_linear_then_reference_then_cat():
    g0 = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g0, dtype=torch.float64)      # noqa: E731
    images, context, words, weight, mask = mk(2, 3, 4, 4), mk(2, 3, 4, 4), mk(2, 6, 5), mk(16, 6), mask_of([5, 3], 5)
    f, alpha = channel_attention_oracle(images, words, mask, weight)
    wt = torch.einsum("pe,bet->btp", weight, words)
    f2, alpha2 = HF.channel_attention_reference(images, wt, mask, 0.25)       # None = 1 / sqrt(16)
    assert (f - f2).abs().max().item() < 1e-12 and (alpha - alpha2).abs().max().item() < 1e-12
    x, _ = stage_input_oracle(images, context, words, mask, weight)
    assert x.shape == (2, 9, 4, 4) and torch.equal(x[:, :3], images) and torch.equal(x[:, 3:6], context) and torch.equal(x[:, 6:], f)


# ------------------------------------------------------------------------------------------------------- module and generators
def test_the_module_has_one_parameter_and_refuses_a_wrong_map_size():
    mod = ATT.ChannelAttention(8, 16, 6)
    sd = mod.state_dict()
    assert list(sd) == ["perception.weight"] and sd["perception.weight"].shape == (36, 16)
    assert mod.scale is None and ATT.ChannelAttention(8, 16, 6, scale=1).scale == 1.0
    for bad in (0, -4, 2.5, "6", True):
        with pytest.raises(ValueError):
            ATT.ChannelAttention(8, 16, bad)
    mod.apply_mask(torch.ones(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="6 x 6"):
        mod(torch.randn(2, 8, 4, 4), torch.randn(2, 16, 3))
    with pytest.raises(ValueError, match="6 x 6"):
        mod(torch.randn(2, 8, 6, 4), torch.randn(2, 16, 3))
    with pytest.raises(L.AganError):
        mod(torch.randn(2, 8, 6, 6), torch.randn(2, 16, 3))          # the right size: no CPU fallback


def test_a_channel_attention_generator_has_exactly_the_new_keys_at_width_three():
    torch.manual_seed(7)
    plain = GEN.Generator(4, 16, 10, 10).state_dict()
    torch.manual_seed(7)
    gen = GEN.Generator(4, 16, 10, 10, channel_attn=True)
    sd = gen.state_dict()
    assert set(sd) - set(plain) == {"gen2.channel_attn.perception.weight", "gen3.channel_attn.perception.weight"}
    assert set(plain) - set(sd) == set()
    assert sd["gen2.channel_attn.perception.weight"].shape == (64 * 64, 16)
    assert sd["gen3.channel_attn.perception.weight"].shape == (128 * 128, 16)
    assert "gen2.attention.conv1.weight" in sd and "gen3.attention.conv1.weight" in sd
    assert isinstance(gen.gen2.channel_attn, ATT.ChannelAttention) and gen.gen2.channel_attn.hw == 64 and gen.gen3.channel_attn.hw == 128
    # residual blocks and the up block are those of width 3 gf = 12: the shapes a stand-alone stage of that plan has
    want = SUB.GenNextStage(4, 16, 2, channel_attn_hw=64).state_dict()
    seen = 0
    for stage in ("gen2", "gen3"):
        for k, v in sd.items():
            if k.startswith((stage + ".residual.", stage + ".upsample.")):
                assert v.shape == want[k[len(stage) + 1:]].shape, k
                seen += 1
    assert seen > 0
    assert sd["gen2.residual.0.block.0.weight"].shape[1] == 12 and plain["gen2.residual.0.block.0.weight"].shape[1] == 8
    assert sd["gen2.upsample.1.weight"].shape[1] == 12 and sd["gen2.upsample.1.weight"].shape[0] == 2 * 4
    for k in plain:                                                  # everything else keeps its shape
        if not k.startswith(("gen2.residual.", "gen2.upsample.", "gen3.residual.", "gen3.upsample.")):
            assert sd[k].shape == plain[k].shape, k
    # what was built before gen2 has the plain generator's values under one seed
    for k in plain:
        if k.startswith(("vae.", "gen1.", "img_out1.")):
            assert torch.equal(sd[k], plain[k]), k
    with pytest.raises(RuntimeError):
        gen.load_state_dict(plain, strict=False)                    # a plain checkpoint does not load: the shapes differ


def test_generator4_and_the_combinations():
    sd4 = S4.Generator4(4, 16, 10, 10, channel_attn=True).state_dict()
    assert {k for k in sd4 if "channel_attn" in k} == {f"gen{i}.channel_attn.perception.weight" for i in (2, 3, 4)}
    assert sd4["gen4.channel_attn.perception.weight"].shape == (256 * 256, 16)
    both = GEN.Generator(4, 16, 10, 10, cond_bn=True, self_attn=32, channel_attn=True).state_dict()
    assert "gen2.upsample.2.cond.weight" in both and "gen1.self_attn.gamma" in both and "gen3.channel_attn.perception.weight" in both
    assert both["gen2.upsample.2.cond.weight"].shape[1] == 10
    with pytest.raises(ValueError, match="channel plan"):
        GEN.Generator(4, 16, 10, 10, memory=True, channel_attn=True)
    with pytest.raises(ValueError, match="channel plan"):
        S4.Generator4(4, 16, 10, 10, memory=True, channel_attn=True)
    with pytest.raises(ValueError, match="channel plan"):
        SUB.GenNextStage(4, 16, 2, memory=True, channel_attn_hw=64)
    with pytest.raises(TypeError):
        GEN.Generator1(4, 16, 10, 10, channel_attn=True)             # no refinement stage, no such argument


def test_the_plain_generator_is_untouched():
    torch.manual_seed(7)
    a = GEN.Generator(4, 16, 10, 10)
    torch.manual_seed(7)
    b = GEN.Generator(4, 16, 10, 10, channel_attn=False)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert set(sa) == set(O.make_generator_params(4, 16, 10, 10))       # the reference's keys, as the oracle lists them
    assert not hasattr(a.gen2, "channel_attn") and not any("channel_attn" in k for k in sa)
    assert [n for n, _ in a.named_modules() if "channel_attn" in n] == []
    assert len(GEN.Generator(32, 256, 100, 100).state_dict()) == 97
    torch.manual_seed(7)
    p4 = S4.Generator4(4, 16, 10, 10).state_dict()
    torch.manual_seed(7)
    q4 = S4.Generator4(4, 16, 10, 10, channel_attn=False).state_dict()
    assert list(p4) == list(q4) and all(torch.equal(p4[k], q4[k]) for k in p4) and not any("channel_attn" in k for k in p4)
    # the memory generator is the parent's as well
    torch.manual_seed(7)
    m1 = GEN.Generator(4, 16, 10, 10, memory=True).state_dict()
    torch.manual_seed(7)
    m2 = GEN.Generator(4, 16, 10, 10, memory=True, channel_attn=False).state_dict()
    assert list(m1) == list(m2) and all(torch.equal(m1[k], m2[k]) for k in m1)


def test_the_default_scale_keeps_the_softmax_soft_at_initialisation():
    """the numbers behind `scale=None`: float64, the generator's own perception weights at the 64 x 64 stage"""
    B, T = 3, 5
    meds = {None: [], 1.0: []}
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        gen = GEN.Generator(4, 16, 10, 10, channel_attn=True)
        weight = gen.gen2.channel_attn.perception.weight.detach().double()
        g0 = torch.Generator().manual_seed(seed)
        images = torch.randn(B, 4, 64, 64, generator=g0, dtype=torch.float64)
        words = torch.randn(B, 16, T, generator=g0, dtype=torch.float64)
        for scale in meds:
            _, alpha = channel_attention_oracle(images, words, mask_of([T] * B, T), weight, scale)
            meds[scale].append(float(alpha.amax(dim=2).median()))
            if scale is None:
                assert float(alpha.amax(dim=2).max()) < 0.9
    assert max(meds[None]) < 0.6 and min(meds[1.0]) > 0.9, meds
