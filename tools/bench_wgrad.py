#!/usr/bin/env python
"""Strip weight-gradient kernel (wgrad_halo.hip) per launch, on COLD operands: every launch reads another (dY, X) set
of a rotation larger than L2 and the Infinity Cache, as inside the training step.  Device events around each launch,
median over the launches after one warm-up rotation.

  python tools/bench_wgrad.py                         the library in the tree
  python tools/bench_wgrad.py --libs a.so,b.so        A/B: the libraries interleaved, --rounds rounds, one fresh
                                                      process per library and round (MSML_LIB selects the library)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (label, N, Cin, Cout, H, W, layers per launch)
SHAPES = [("256->256 @14x14 x4", 256, 256, 256, 14, 14, 4), ("128->128 @28x28 x4", 256, 128, 128, 28, 28, 4),
          ("256->512 @14x14 x1", 256, 256, 512, 14, 14, 1), ("64->64 @56x56 x4", 256, 64, 64, 56, 56, 4)]


def measure(launches):
    import torch
    sys.path.insert(0, ROOT)
    from msml_amd import _lib
    out = {}
    for label, n, cin, cout, h, w, group in SHAPES:
        group = min(group, _lib.value("msml_conv_wgrad_group_max", cout, cin, cout, cin, n, h, w, h, w, 3, 3, 1, 1, 1))
        set_bytes = group * n * h * w * (cin + cout) * 2
        nset = max(3, int(1.2e9 / set_bytes))
        us = [[torch.randn(n, h, w, cout, device="cuda").bfloat16() for _ in range(group)] for _ in range(nset)]
        vs = [[torch.randn(n, h, w, cin, device="cuda").bfloat16() for _ in range(group)] for _ in range(nset)]
        dws = [torch.zeros(cout, cin, 3, 3, device="cuda") for _ in range(group)]
        ws = torch.empty(_lib.value("msml_conv_wgrad_workspace", cout, cin, n, h, w, 3, 3), dtype=torch.uint8, device="cuda")
        arr = ctypes.c_void_p * group
        pd = arr(*[t.data_ptr() for t in dws])
        args = [(arr(*[t.data_ptr() for t in us[k]]), arr(*[t.data_ptr() for t in vs[k]])) for k in range(nset)]

        def launch(k):
            _lib.call("msml_conv_wgrad_group", args[k][0], args[k][1], pd, group, cout, cin, cout, cin, cin, 0, n, h, w,
                      h, w, 3, 3, 1, 1, 1, 0, ws, ws.numel(), _lib.BF16)
        for k in range(nset):
            launch(k)
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for i, (e0, e1) in enumerate(ev):
            e0.record()
            launch(i % nset)
            e1.record()
        torch.cuda.synchronize()
        us_med = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3
        out[label] = {"us": us_med, "tflops": 2.0 * group * n * h * w * cin * cout * 9 / us_med * 1e-6}
        del us, vs, args
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child or not a.libs:
        res = measure(a.launches)
        if a.child:
            print("RESULT " + json.dumps(res), flush=True)
        else:
            for k, v in res.items():
                print("%-22s %8.1f us  %6.0f TFLOP/s (launch + reduce)" % (k, v["us"], v["tflops"]))
        return
    libs = a.libs.split(",")
    print("%-22s %5s " % ("shape", "round") + " ".join("%16s" % os.path.basename(x)[:16] for x in libs), flush=True)
    for r in range(a.rounds):
        row = []
        for lib in libs:
            env = dict(os.environ, MSML_LIB=os.path.abspath(lib))
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--launches", str(a.launches)],
                               env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=300).stdout
            row.append(json.loads([x for x in o.splitlines() if x.startswith("RESULT ")][-1][7:]))
        for label, *_ in SHAPES:
            print("%-22s %5d " % (label, r) + " ".join("%13.1f us" % x[label]["us"] for x in row), flush=True)


if __name__ == "__main__":
    main()
