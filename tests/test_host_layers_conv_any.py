"""`Layers.conv(in_channels, out_channels, in_hw, out_hw)` builds for every (kernel, stride, padding) triple the reference's search can
return, with the reference's choice (tests/golden/l1_layers_conv.npz, written by tests/golden/make_golden_layers_conv.py from the
reference's own `Layers.conv`).  Needs no GPU: construction only."""
import importlib
import os

import numpy as np
import pytest
import torch

LAY = importlib.import_module("attention-gan_amd.utilities.layers")
HF = importlib.import_module("attention-gan_amd.backend.functional")
L = importlib.import_module("attention-gan_amd.backend.lib")

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "l1_layers_conv.npz"), allow_pickle=False)
ROWS = [tuple(int(v) for v in p) + tuple(int(v) for v in c) for p, c in zip(Z["pairs"], Z["conv"])]

TRIPLES = [(1, 1, 3), (1, 2, 3), (1, 3, 3), (2, 1, 3), (2, 2, 3), (2, 3, 3), (3, 1, 0), (3, 1, 1), (3, 1, 2), (3, 1, 3), (3, 2, 3), (3, 3, 3),
           (4, 1, 0), (4, 1, 1), (4, 1, 2), (4, 1, 3), (4, 2, 0), (4, 2, 1), (4, 2, 2), (4, 2, 3), (4, 3, 0), (4, 3, 1), (4, 3, 2), (4, 3, 3)]


def test_fixture_covers_the_24_triples_in_order():
    assert [r[2:5] for r in ROWS] == TRIPLES


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"{r[0]}to{r[1]}-k{r[2]}s{r[3]}p{r[4]}")
def test_layers_conv_builds_with_the_reference_choice(row):
    in_hw, out_hw, k, s, p, has_bias = row
    torch.manual_seed(3)
    m = LAY.Layers.conv(4, 6, in_hw, out_hw)
    assert isinstance(m, torch.nn.Conv2d) and isinstance(m, LAY.HipConv2d)
    assert m.kernel_size == (k, k) and m.stride == (s, s) and m.padding == (p, p)
    assert (m.bias is not None) == bool(has_bias)
    assert (m.in_channels, m.out_channels) == (4, 6)
    assert m.kind == {(3, 1, 1): "same", (4, 2, 1): "down"}.get((k, s, p), "any")
    assert set(m.state_dict()) == {"weight"}
    # nn.Conv2d's init and RNG consumption
    torch.manual_seed(3)
    ref = torch.nn.Conv2d(4, 6, kernel_size=k, stride=s, padding=p, bias=False)
    assert torch.equal(m.weight, ref.weight)


def test_layers_conv_of_the_issue_example_builds():
    m = LAY.Layers.conv(64, 64, 8, 4)
    assert (m.kernel_size, m.stride, m.padding, m.kind) == ((4, 4), (3, 3), (3, 3), "any")


def test_outside_the_domain_still_raises_and_tuned_kinds_keep_their_route():
    for k, s, p in ((7, 1, 0), (7, 2, 3), (6, 1, 0), (3, 4, 1), (3, 1, 4)):
        with pytest.raises(NotImplementedError):
            LAY.HipConv2d(4, 4, k, s, p, False)
    assert LAY.HipConv2d(4, 4, 3, 1, 1, False).kind == "same"
    assert LAY.HipConv2d(4, 4, 1, 1, 0, True).kind == "same"
    assert LAY.HipConv2d(4, 4, 5, 1, 2, False).kind == "same"
    assert LAY.HipConv2d(4, 4, 4, 2, 1, True).kind == "down"
    assert LAY.HipConv2d(4, 4, 3, 1, 1, False, kind="up").kind == "up"
    assert LAY.HipConv2d(4, 4, 5, 2, 0, True).kind == "any"


def test_fused_activation_is_never_chosen_for_kind_any():
    assert HF.conv_fuses_activation(L.ACT_LRELU, 64) is True                  # the two-argument call keeps its meaning
    assert HF.conv_fuses_activation(L.ACT_LRELU, 4) is False
    assert HF.conv_fuses_activation(L.ACT_LRELU, 64, "down") is True
    assert HF.conv_fuses_activation(L.ACT_LRELU, 64, "any") is False
