"""CPU tests of spectral normalisation (Miyato et al. 2018): the plain-torch statement (backend.functional.spectral_weight_reference,
which CPU tensors take) against torch.nn.utils.spectral_norm, the holders' state_dict interchange with torch's modules, the warm start
from a plain `weight`, the joint conv's one sigma over [image | sentence], the discriminators' norm="spectral" mode (same initial weights
as norm="batch" under a seed, no BatchNorm key, refusal of other values), the default modules' unchanged keys, and the argument checks
of the C entries (agan_spectral_*), which answer before any device is touched."""
import importlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn

L = importlib.import_module("attention-gan_amd.backend.lib")
HF = importlib.import_module("attention-gan_amd.backend.functional")
LAY = importlib.import_module("attention-gan_amd.utilities.layers")
DISC = importlib.import_module("attention-gan_amd.networks.discriminators")
S4 = importlib.import_module("attention-gan_amd.networks.stage4")

F64 = torch.float64


def _close(a, b, tol=1e-12):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("kind", ["conv", "linear"])
def test_reference_equals_torch_spectral_norm_in_float64(kind):
    """three training forwards, then an eval forward: outputs, u, v and weight_orig.grad"""
    torch.manual_seed(5)
    if kind == "conv":
        ours = LAY.HipConv2d(5, 7, 3, 1, 1, True, spectral=True).double()
        theirs = torch.nn.utils.spectral_norm(nn.Conv2d(5, 7, 3, padding=1)).double()
        x = torch.randn(2, 5, 6, 6, dtype=F64)
        run = lambda m, w: F.conv2d(x, w, m.bias, padding=1)
    else:
        ours = LAY.HipLinear(11, 4, spectral=True).double()
        theirs = torch.nn.utils.spectral_norm(nn.Linear(11, 4)).double()
        x = torch.randn(3, 11, dtype=F64)
        run = lambda m, w: F.linear(x, w, m.bias)
    assert sorted(ours.state_dict()) == sorted(theirs.state_dict()) == ["bias", "weight_orig", "weight_u", "weight_v"]
    theirs.load_state_dict(ours.state_dict(), strict=True)
    g = torch.randn_like(run(ours, ours.weight_orig))
    for it in range(4):
        training = it < 3
        ours.train(training), theirs.train(training)
        ours.zero_grad(), theirs.zero_grad()
        ya = run(ours, HF.spectral_weight_reference(ours.weight_orig, ours.weight_u, ours.weight_v, training))
        yb = theirs(x)
        (ya * g).sum().backward()
        (yb * g).sum().backward()
        assert _close(ya, yb), it
        assert _close(ours.weight_u, theirs.weight_u) and _close(ours.weight_v, theirs.weight_v), it
        assert _close(ours.weight_orig.grad, theirs.weight_orig.grad), it
    # CPU tensors take the reference through the public entry too
    a = HF.spectral_weight(ours.weight_orig, ours.weight_u, ours.weight_v, False)
    assert torch.equal(a, HF.spectral_weight_reference(ours.weight_orig, ours.weight_u, ours.weight_v, False))


def test_two_forwards_then_one_backward_use_their_own_u_and_v():
    """the second training forward moves the buffers; the first forward's graph must keep its own"""
    torch.manual_seed(1)
    w = torch.randn(4, 6, dtype=F64, requires_grad=True)
    u = F.normalize(torch.randn(4, dtype=F64), dim=0)
    v = F.normalize(torch.randn(6, dtype=F64), dim=0)
    d = torch.randn(4, 6, dtype=F64)
    u1, v1 = u.clone(), v.clone()
    a = HF.spectral_weight_reference(w, u1, v1, True)
    HF.spectral_weight_reference(w, u1, v1, True)
    (a * d).sum().backward()
    u2, v2 = u.clone(), v.clone()
    w2 = w.detach().clone().requires_grad_(True)
    (HF.spectral_weight_reference(w2, u2, v2, True) * d).sum().backward()
    assert torch.equal(w.grad, w2.grad)


def test_state_dict_interchange_with_torch_both_ways():
    torch.manual_seed(2)
    ours = LAY.HipConv2d(3, 8, 4, 2, 1, False, spectral=True)
    theirs = torch.nn.utils.spectral_norm(nn.Conv2d(3, 8, 4, 2, 1, bias=False))
    assert abs(float(ours.weight_u.norm()) - 1) < 1e-6 and abs(float(ours.weight_v.norm()) - 1) < 1e-6
    theirs.load_state_dict(ours.state_dict(), strict=True)
    for k, v in ours.state_dict().items():
        assert torch.equal(theirs.state_dict()[k], v), k
    torch.manual_seed(3)
    other = torch.nn.utils.spectral_norm(nn.Conv2d(3, 8, 4, 2, 1, bias=False))
    ours.load_state_dict(other.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    lin = LAY.HipLinear(6, 5, spectral=True)
    tl = torch.nn.utils.spectral_norm(nn.Linear(6, 5))
    tl.load_state_dict(lin.state_dict(), strict=True)
    lin.load_state_dict(tl.state_dict(), strict=True)
    assert lin.weight_v.shape == (6,) and lin.weight_u.shape == (5,)


def test_warm_start_from_a_plain_weight():
    torch.manual_seed(4)
    plain = LAY.HipConv2d(3, 8, 4, 2, 1, True)
    sn = LAY.HipConv2d(3, 8, 4, 2, 1, True, spectral=True)
    u, v = sn.weight_u.clone(), sn.weight_v.clone()
    sn.load_state_dict(plain.state_dict(), strict=True)
    assert torch.equal(sn.weight_orig, plain.weight) and torch.equal(sn.bias, plain.bias)
    assert torch.equal(sn.weight_u, u) and torch.equal(sn.weight_v, v)


def test_default_holders_are_unchanged():
    torch.manual_seed(6)
    a = LAY.HipConv2d(3, 8, 4, 2, 1, True)
    torch.manual_seed(6)
    b = nn.Conv2d(3, 8, 4, 2, 1)
    assert list(a.state_dict()) == ["weight", "bias"] and torch.equal(a.weight, b.weight) and torch.equal(a.bias, b.bias)
    assert list(LAY.HipLinear(4, 3).state_dict()) == ["weight", "bias"]
    for cls in (DISC.Disc64, DISC.Disc128, DISC.Disc256):
        for cd in (None, 16):
            keys = list(cls(4, cond_dim=cd).state_dict())
            assert not [k for k in keys if k.endswith(("_orig", "_u", "_v"))], keys
    assert not [k for k in S4.Disc512(2).state_dict() if k.endswith(("_orig", "_u", "_v"))]


@pytest.mark.parametrize("cls", [DISC.Disc64, DISC.Disc128, DISC.Disc256])
@pytest.mark.parametrize("cond_dim", [None, 16])
def test_spectral_and_batch_hold_the_same_initial_weights(cls, cond_dim):
    torch.manual_seed(9)
    a = cls(4, cond_dim=cond_dim)
    torch.manual_seed(9)
    b = cls(4, cond_dim=cond_dim, norm="spectral")
    sa, sb = a.state_dict(), b.state_dict()
    assert not [k for k in sb if "running_mean" in k or "num_batches_tracked" in k]
    assert b.supports_batch_groups
    convs = [k for k in sa if k.endswith(".weight") and k.rsplit(".", 1)[0] + ".running_mean" not in sa]
    assert convs
    for k in convs:
        assert torch.equal(sa[k], sb[k + "_orig"]), k
        u, v = sb[k + "_u"], sb[k + "_v"]
        assert u.shape == (sa[k].shape[0],) and v.shape == (sa[k][0].numel(),)
        assert abs(float(u.norm()) - 1) < 1e-5 and abs(float(v.norm()) - 1) < 1e-5
    for k in sa:
        if k.endswith(".bias") and k.rsplit(".", 1)[0] + ".running_mean" not in sa:
            assert torch.equal(sa[k], sb[k]), k
    want = {k + s for k in convs for s in ("_orig", "_u", "_v")} | {k for k in sa if k.endswith(".bias") and k.rsplit(".", 1)[0] + ".running_mean" not in sa}
    assert set(sb) == want
    if cond_dim is not None:
        assert {"COND_DNET.jointConv.0.weight_orig", "COND_DNET.jointConv.0.weight_u", "COND_DNET.jointConv.0.weight_v",
                "COND_DNET.outlogits.0.weight_orig", "COND_DNET.outlogits.0.bias"} <= set(sb)
    assert {"outlogits.0.weight_orig", "outlogits.0.weight_u", "outlogits.0.weight_v", "outlogits.0.bias"} <= set(sb)


def test_disc512_spectral_and_bad_norm_values():
    torch.manual_seed(9)
    a = S4.Disc512(2)
    torch.manual_seed(9)
    b = S4.Disc512(2, norm="spectral")
    assert torch.equal(a.state_dict()["img_code_s128_3.0.weight"], b.state_dict()["img_code_s128_3.0.weight_orig"])
    assert not [k for k in b.state_dict() if "running" in k]
    for cls in (DISC.Disc64, DISC.Disc128, DISC.Disc256, S4.Disc512):
        for bad in ("instance", None, "Spectral", True):
            with pytest.raises(ValueError, match="norm"):
                cls(2, norm=bad)
    with pytest.raises(ValueError, match="norm"):
        LAY.Layers.downBlock(4, 8, norm="layer")


def test_warm_start_of_a_spectral_discriminator_from_a_batch_checkpoint():
    torch.manual_seed(10)
    a = DISC.Disc128(4, cond_dim=16)
    torch.manual_seed(11)
    b = DISC.Disc128(4, cond_dim=16, norm="spectral")
    before = {k: v.clone() for k, v in b.state_dict().items()}
    b.load_state_dict(a.state_dict())
    sa, sb = a.state_dict(), b.state_dict()
    for k in sb:
        if k.endswith("_orig"):
            assert torch.equal(sb[k], sa[k[:-5]]), k
        elif k.endswith(("_u", "_v")):
            assert torch.equal(sb[k], before[k]), k
        else:
            assert torch.equal(sb[k], sa[k]), k


def test_joint_conv_is_the_spectral_norm_of_attngans_layer():
    """sigma and u equal torch's on the concatenated AttnGAN-layout weight; the saved v is in AttnGAN's column order; save -> load
    round-trips bit for bit"""
    torch.manual_seed(12)
    c, nef = 8, 5
    D = DISC.Disc64(1, cond_dim=nef, norm="spectral").double()
    jc = D.COND_DNET.jointConv
    assert jc.c == c and not hasattr(jc, "1")
    theirs = torch.nn.utils.spectral_norm(nn.Conv2d(c + nef, c, 3, padding=1, bias=False)).double()
    sd = {k[len("COND_DNET.jointConv.0."):]: v for k, v in D.state_dict().items() if k.startswith("COND_DNET.jointConv.0.")}
    assert sorted(sd) == ["weight_orig", "weight_u", "weight_v"] and sd["weight_orig"].shape == (c, c + nef, 3, 3)
    theirs.load_state_dict(sd, strict=True)
    for _ in range(3):
        wi, ws = jc.weights_sn()
        x = torch.randn(1, c + nef, 4, 4, dtype=F64)
        theirs(x)
        ours = torch.cat([wi, ws.view(c, 9, nef).permute(0, 2, 1).reshape(c, nef, 3, 3)], dim=1)
        assert _close(ours, theirs.weight)
        assert _close(jc.weight_u, theirs.weight_u)
        assert _close(D.state_dict()["COND_DNET.jointConv.0.weight_v"], theirs.weight_v)
        sigma_ours = float(jc.image.weight.flatten()[0] / wi.flatten()[0])
        sigma_theirs = float(theirs.weight_orig.flatten()[0] / theirs.weight.flatten()[0])
        assert abs(sigma_ours - sigma_theirs) <= 1e-12 * abs(sigma_theirs)
    torch.manual_seed(13)
    E = DISC.Disc64(1, cond_dim=nef, norm="spectral").double()
    E.load_state_dict(D.state_dict(), strict=True)
    for k, v in D.state_dict().items():
        assert torch.equal(E.state_dict()[k], v), k
    assert torch.equal(E.COND_DNET.jointConv.weight_v, jc.weight_v) and torch.equal(E.COND_DNET.jointConv.sentence.weight, jc.sentence.weight)


def test_fifty_iterations_reach_the_top_singular_value():
    torch.manual_seed(14)
    conv = LAY.HipConv2d(6, 9, 3, 1, 1, False, spectral=True)
    for _ in range(50):
        w = conv.weight_sn()
    top = float(torch.linalg.svdvals(w.detach().reshape(9, -1).double())[0])
    assert abs(top - 1) < 1e-3, top
    conv.eval()
    u = conv.weight_u.clone()
    assert torch.equal(conv.weight_sn(), w) and torch.equal(conv.weight_u, u)


def test_python_refusals():
    w = torch.randn(3, 4)
    u, v = torch.randn(3), torch.randn(4)
    with pytest.raises(ValueError, match="u must be"):
        HF.spectral_weight(w, v, u, True)
    with pytest.raises(ValueError, match="second segment"):
        HF.spectral_weight(w, u, torch.randn(9), True, second=torch.randn(5, 1))
    with pytest.raises(ValueError, match="at least two axes"):
        HF.spectral_weight(torch.randn(3), u, v, True)
    with pytest.raises(ValueError, match="state"):
        HF.spectral_weight(w, u.requires_grad_(True), v, True)


def test_c_entries_refuse_before_touching_the_device():
    lib = L.load()
    p = 64                                                            # (never dereferenced: every call below is refused first)
    fwd = lambda cout, k0, k1, it=1, w1=p, ws=p, n=1 << 30, v=p, uo=p: lib.agan_spectral_fwd(p, w1, p, v, uo, p, p, p, w1, cout, k0, k1, it, ws, n, None)
    bwd = lambda cout, k0, k1, d1=p, ws=p, n=1 << 30: lib.agan_spectral_bwd(p, d1, p, d1, p, p, p, p, d1, cout, k0, k1, 0, 0, ws, n, None)
    for shape in ((0, 4, 0), (4, 0, 0), (4, 4, -1), (-1, 4, 0), (1 << 16, 1 << 15, 0), (1 << 15, 1 << 15, 1 << 15)):
        assert fwd(*shape) == L.EINVAL and b"spectral_fwd" in lib.agan_last_error()
        assert bwd(*shape) == L.EINVAL and b"spectral_bwd" in lib.agan_last_error()
        assert lib.agan_spectral_fwd_ws_bytes(*shape) == 0 and b"spectral_fwd_ws_bytes" in lib.agan_last_error()
        assert lib.agan_spectral_bwd_ws_bytes(*shape) == 0 and b"spectral_bwd_ws_bytes" in lib.agan_last_error()
    assert fwd(8, 8, 0, it=2) == L.EINVAL and b"iterate" in lib.agan_last_error()
    assert fwd(8, 8, 8, w1=None) == L.EINVAL and b"null" in lib.agan_last_error()
    assert fwd(8, 8, 0, it=0, v=None) == L.EINVAL and fwd(8, 8, 0, uo=None) == L.EINVAL
    assert bwd(8, 8, 8, d1=None) == L.EINVAL and b"spectral_bwd" in lib.agan_last_error()
    assert lib.agan_spectral_fwd(None, p, p, p, p, p, p, p, p, 8, 8, 0, 1, p, 1 << 30, None) == L.EINVAL
    # the seam: 64 x 128 needs no workspace, 64 x 129 does; a short or missing one is refused
    assert lib.agan_spectral_fwd_ws_bytes(64, 128, 0) == 0 and lib.agan_spectral_bwd_ws_bytes(64, 128, 0) == 0
    nf, nb = lib.agan_spectral_fwd_ws_bytes(64, 129, 0), lib.agan_spectral_bwd_ws_bytes(64, 129, 0)
    assert nf > 0 and nb > 0
    assert fwd(64, 129, 0, n=nf - 1) == L.EWORKSPACE and b"spectral_fwd" in lib.agan_last_error()
    assert fwd(64, 129, 0, ws=None, n=nf) == L.EWORKSPACE
    assert bwd(64, 129, 0, n=nb - 1) == L.EWORKSPACE and b"spectral_bwd" in lib.agan_last_error()
    assert bwd(64, 129, 0, ws=None, n=nb) == L.EWORKSPACE
