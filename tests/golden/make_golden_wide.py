#!/usr/bin/env python3
"""Golden fixtures of the mini-batch modules at embedding widths above 64 (`minibatch_wide128.npz`, `minibatch_wide200.npz`).

Same recipe, same reference classes and same keys as `make_golden.py::mini_module_case` (the D = 64 / D = 32 fixtures
`minibatch_small` / `minibatch_dense`), called at d = 128 and d = 200.  Like `make_golden.py` it runs only where the reference
tree is mounted; the fixtures are data only.  D = 256 has no reference fixture (four copies of a 256 x 256 weight exceed the
size limit of a committed file): the float64 oracle covers it.

    python tests/golden/make_golden_wide.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import make_golden  # noqa: E402


def main():
    if not os.path.isdir(make_golden.REF):
        sys.exit("reference tree not present; golden fixtures can only be regenerated in the build container")
    make_golden.torch.set_num_threads(8)
    make_golden._stub_third_party()
    sys.path.insert(0, os.path.join(make_golden.REF, "src"))
    make_golden.mini_module_case("wide128", n=600, n_entries=3000, f=17, d=128, seed=5, n_norm=40, n_ano=10,
                                 kind="powerlaw", k_steps=6, self_loop_frac=0.05)
    make_golden.mini_module_case("wide200", n=150, n_entries=3000, f=9, d=200, seed=8, n_norm=24, n_ano=6,
                                 kind="er", k_steps=3, self_loop_frac=1.0)


if __name__ == "__main__":
    main()
