#!/usr/bin/env python
"""Microbenchmark of msml_bn_eval_act_bwd (backward through a frozen BatchNorm + PReLU, bf16) at the ires50 batch-256 maps,
without and with the parameter-gradient sums, beside the training-mode backward msml_bn_act_bwd_acc at the same shapes
and a `copy_` that moves the same bytes (the eval backward streams dy, x -> dx: three tensors; the copy reads and writes
1.5 tensors each).  Device events around INNER back-to-back calls, WARMUP untimed rounds, the contenders alternate inside
every round and the median round is reported, so that clock and cache state are shared.  Buffers are reused between
rounds: the small maps (7 x 7, 14 x 14) stay in the last-level cache, as they largely do in a training step.

    python tools/bench_bn_eval_bwd.py [--rounds 15] [--inner 10]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from msml_amd import _lib, ops  # noqa: E402

SHAPES = [(256 * 112 * 112, 64), (256 * 56 * 56, 64), (256 * 28 * 28, 128), (256 * 14 * 14, 256), (256 * 7 * 7, 512)]
WARMUP = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda")
    slower = []
    print("%-16s %10s %10s %10s %10s | %8s %8s" % ("M x C", "eval", "eval+sums", "train acc", "copy", "eval/cp", "sums/cp"))
    for m, c in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(m + c)
        dy = torch.randn(m, c, device=dev, generator=g).bfloat16()
        x = torch.randn(m, c, device=dev, generator=g).bfloat16()
        dx = torch.empty_like(x)
        coef = torch.rand(4, c, device=dev, generator=g) + 0.5
        alpha = torch.rand(c, device=dev, generator=g) * 0.3
        pg = torch.zeros(3, c, device=dev)
        rows = _lib.value("msml_bn_eval_act_bwd_rows", m, c)
        ws = torch.empty(rows * 3 * c, device=dev)
        n15 = m * c * 3 // 2
        src, dst = torch.empty(n15, device=dev, dtype=torch.bfloat16).normal_(), torch.empty(n15, device=dev, dtype=torch.bfloat16)

        def ev_plain():
            _lib.call("msml_bn_eval_act_bwd", dy, x, coef[0], coef[1], alpha, None, None, None, dx, None, None, None, None, 0,
                      m, c, None, 0, _lib.BF16)

        def ev_sums():
            _lib.call("msml_bn_eval_act_bwd", dy, x, coef[0], coef[1], alpha, coef[2], coef[3], None, dx, None, pg[0], pg[1],
                      pg[2], 0, m, c, ws, ws.numel(), _lib.BF16)

        def train_acc():
            _lib.call("msml_bn_act_bwd_acc", dy, x, coef[0], coef[1], alpha, coef[2], coef[3], None, None, dx, None, pg[0],
                      pg[1], pg[2], 0, m, c, ops.stats_acc(c, dev, 3), _lib.BF16)

        def copy():
            dst.copy_(src)

        fns = (ev_plain, ev_sums, train_acc, copy)
        times = [[] for _ in fns]
        for r in range(WARMUP + a.rounds):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                if r >= WARMUP:
                    times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
        t = [statistics.median(v) for v in times]
        print("%9d x %-4d %8.1f us %8.1f us %8.1f us %8.1f us | %7.0f%% %7.0f%%"
              % (m, c, t[0], t[1], t[2], t[3], 100.0 * t[3] / t[0], 100.0 * t[3] / t[1]))
        if t[0] > t[2] or t[1] > t[2]:
            slower.append((m, c))
    print("eval backward slower than msml_bn_act_bwd_acc at:", slower if slower else "no shape")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
