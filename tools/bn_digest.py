#!/usr/bin/env python
"""One digest per (entry point, case, output tensor) of msml_amd/csrc/bn.hip, to compare two builds of the library bit
for bit:

    MSML_LIB=<other build> python tools/bn_digest.py a.txt ; python tools/bn_digest.py b.txt ; cmp a.txt b.txt

The calls are the ones tests/test_gpu_bn.py and tests/test_gpu_bn_eval_bwd.py make: the `reduce`, `apply`, `rows`,
`lattice` and `big` tables of tests/bn_cases.py and the tables of tests/bn_eval_cases.py, f32 and bf16, both protocols,
the row-protocol _next / _s2 / _next_s2 forms and msml_bn_fin_bwd_apply with every next / add combination.  Every output
buffer of every call is hashed right after the call (accumulator outputs included: their f64 sums of f32 partials are
exact, so they do not depend on the order of the atomic adds).  The f64 comparisons of those tests are not repeated here."""
import hashlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msml_amd import _lib  # noqa: E402
from tests import bn_cases as B, bn_eval_cases as E  # noqa: E402
from tests.test_gpu_bn import Device as BnDevice  # noqa: E402
from tests.test_gpu_bn_eval_bwd import Device as EvalDevice  # noqa: E402

LINES = []


class NoReport(B.Report):
    def check(self, *a, **k):
        return 0.0

    def exact(self, *a, **k):
        return True


def recording(base, case):
    class Rec(base):
        def call(self, name, *args):
            outs = [buf for buf, _ in self.bufs if any(lo == buf.data_ptr() for lo, _ in self.pending)]
            super().call(name, *args)
            self.n = getattr(self, "n", 0) + 1
            for i, buf in enumerate(outs):
                h = hashlib.sha1(buf.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]
                LINES.append("%s %s call%d out%d %s %s" % (name, case.name, self.n, i, tuple(buf.shape), h))
    return Rec()


def main(path):
    t0 = time.time()
    rep = NoReport()
    for c in B.case_table("reduce"):
        B.check_reduce_case(recording(BnDevice, c), c, rep, "cuda")
    for c in B.case_table("apply") + B.case_table("big"):
        B.check_apply_case(recording(BnDevice, c), c, rep, "cuda")
        torch.cuda.empty_cache()
    for c in B.case_table("rows") + B.case_table("lattice"):
        B.check_rows_case(recording(BnDevice, c), c, rep, "cuda")
    for c in B.case_table("lattice"):
        B.check_lattice_fwd(recording(BnDevice, c), c, rep, "cuda")
    for c in E.case_table("normal") + E.case_table("lattice"):
        E.check_eval_case(recording(EvalDevice, c), c, rep, "cuda")
    for dt in ("f32", "bf16"):
        for n in (8, 8 * 255, 8 * (768 * 256 + 5)):
            c = B.Case("add-n%d-%s" % (n, dt), n // 8, 8, dt, False, False, False, False, "normal", None, "add")
            d = B.draw(c, "cuda")
            recording(BnDevice, c).add(d["x"], d["dy"])
    with open(path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    names = sorted({ln.split()[0] for ln in LINES})
    print("%s: %d digests of %d entry points (%s) from %s in %.0f s"
          % (path, len(LINES), len(names), ", ".join(names), _lib.LIBPATH, time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1])
