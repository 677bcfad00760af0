#!/usr/bin/env python3
"""Generate tests/golden/l1_layers_conv.npz: what the REFERENCE's `Layers.conv(in_channels, out_channels, in_hw, out_hw)` returns
for one (in_hw, out_hw) pair per (kernel, stride, padding) triple its search can produce.

Run in the build container only (the GPU box has no /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_layers_conv.py

The reference module is imported read-only from /root/reference; nothing of its source is copied.  The file holds integers only:
`pairs` [24, 2] = (in_hw, out_hw) and `conv` [24, 4] = (kernel_size, stride, padding, has_bias) of the returned nn.Conv2d, both axes
of which are equal by construction (asserted here).
"""
import os
import sys

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from utilities.layers import Layers                                        # noqa: E402

PAIRS = [(1, 7), (15, 11), (28, 12), (1, 6), (14, 10), (26, 11), (10, 8), (6, 6), (2, 4), (1, 5), (1, 3), (24, 10),
         (11, 8), (7, 6), (3, 4), (1, 4), (18, 8), (12, 6), (6, 4), (2, 3), (5, 1), (3, 1), (1, 1), (1, 2)]


def main():
    rows = []
    for in_hw, out_hw in PAIRS:
        m = Layers.conv(4, 6, in_hw, out_hw)
        for name in ("kernel_size", "stride", "padding"):
            a, b = getattr(m, name)
            assert a == b, (name, a, b)
        rows.append((m.kernel_size[0], m.stride[0], m.padding[0], int(m.bias is not None)))
    assert len(set(r[:3] for r in rows)) == len(PAIRS), "the pairs no longer hit distinct triples"
    np.savez(os.path.join(OUT, "l1_layers_conv.npz"), pairs=np.asarray(PAIRS, dtype=np.int64), conv=np.asarray(rows, dtype=np.int64))
    for p, r in zip(PAIRS, rows):
        print(p, "->", r)


if __name__ == "__main__":
    main()
