#!/usr/bin/env python3
"""Host cost of packed_weight's hit path (a fresh entry of a registered flat buffer) in two checkouts of this repository, measured
in ONE process with the checkouts alternated: timeit, 20 000 calls x 5 repeats each.  The library is stubbed and the tensors are
CPU tensors (tests/test_host_weight_forms.py does the same), so this is host Python only and needs no GPU.

    python profiles/weight_forms_host.py PARENT_CHECKOUT BRANCH_CHECKOUT > profiles/weight_forms_host.txt
"""
import importlib.util
import os
import sys
import timeit

import torch

CALLS, REPEATS = 20000, 5


def load(root, name):
    """the package of the checkout at `root` under the module name `name` -> its backend.functional"""
    pkg = os.path.join(root, "attention-gan_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module(name + ".backend.functional")


class StubLib:
    agan_packed_weight_bytes = staticmethod(lambda mode, cout, cin, kh, kw, prec: 64)
    agan_pack_job_blocks_prec = staticmethod(lambda mode, cout, cin, kh, kw, prec: 1)


def hit_path(HF):
    HF.L.load, HF.L.call, HF._stream = (lambda: StubLib), (lambda name, *args: None), (lambda: None)
    flat = torch.zeros(128)
    HF.register_flat(flat)
    w, cache = flat[:36].view(1, 4, 3, 3), {}
    HF.packed_weight(w, 0, cache, 0)
    return (lambda: HF.packed_weight(w, 0, cache, 0)), flat


def main():
    names = ("parent", "branch")
    fns = {n: hit_path(load(os.path.abspath(root), "agan_" + n)) for n, root in zip(names, sys.argv[1:3])}
    us = {n: [] for n in names}
    for n in names:
        timeit.timeit(fns[n][0], number=CALLS)                  # warm-up
    for _ in range(REPEATS):
        for n in names:
            us[n].append(timeit.timeit(fns[n][0], number=CALLS) / CALLS * 1e6)
    print(f"packed_weight on a fresh entry, us per call: {CALLS} calls x {REPEATS} repeats, parent and branch alternated in one process")
    for n in names:
        print(f"{n}: " + " ".join(f"{v:.3f}" for v in us[n]) + f"   best {min(us[n]):.3f}  spread {max(us[n]) - min(us[n]):.3f}")
    print(f"branch best - parent best = {min(us['branch']) - min(us['parent']):+.3f} us "
          f"(allowed: the parent's spread, {max(us['parent']) - min(us['parent']):.3f} us)")


if __name__ == "__main__":
    main()
