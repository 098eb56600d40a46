"""Time the fused top-k search (msml_amd.identify.search_topk, csrc/search.hip) on synthetic unit-norm rows at two
sizes, f32 and f64, against the plain route on the same device: chunked torch.matmul + torch.topk with a running merge.

    ijbc_gallery1   19 593 probes x 1 772 gallery rows, E = 512, k = 10 (the first IJB-C 1:N gallery)
    large_gallery    3 530 probes x 1 000 000 gallery rows (the MegaFace distractor set), E = 512, k = 10

Per size and dtype, after a warm-up, --reps timed repeats with the two routes ALTERNATING (device events, median):
the library call alone (`kernel_ms`: search + merge launches on preallocated buffers), `search_topk` as called from
Python (input checks and allocations included) and the torch route.  TFLOP/s = 2 P G E / time; `of_f32_matrix_peak` is
that over the device's f32 matrix rate (157.3 TFLOP/s), for f64 too: a yardstick, not that type's own peak.  The
workspace bytes are reported next to the P x G matrix the torch route would need unchunked.  Results of the two routes
are compared at the timed size.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_ident.py [--reps 5] [--large-gallery 1000000] [--out profiles/ident_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import _lib, identify  # noqa: E402
from msml_amd._lib import call, value  # noqa: E402

F32_MATRIX_PEAK = 157.3e12
CHUNK_BYTES = 1 << 30          # score chunk of the torch route


def unit_rows(n, e, dtype, gen):
    x = torch.randn(n, e, generator=gen, device="cuda", dtype=torch.float32).to(dtype)
    return x / x.norm(dim=1, keepdim=True)


def torch_route(p, g, k):
    """The k best of p @ g.T without the whole matrix: column chunks, topk per chunk, merged with the running list.
    torch.topk leaves the order of ties open; on random rows there are none."""
    cols = max(k, CHUNK_BYTES // (p.shape[0] * p.element_size()))
    best_s = best_i = None
    for c0 in range(0, g.shape[0], cols):
        s, i = torch.topk(p @ g[c0:c0 + cols].T, min(k, g.shape[0] - c0), dim=1)
        i += c0
        if best_s is not None:
            s, i = torch.cat([best_s, s], 1), torch.cat([best_i, i], 1)
            s, o = torch.topk(s, k, dim=1)
            i = torch.gather(i, 1, o)
        best_s, best_i = s, i
    return best_s, best_i


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def case(name, P, G, E, k, dtype, reps, gen):
    p, g = unit_rows(P, E, dtype, gen), unit_rows(G, E, dtype, gen)
    splits = value("msml_search_topk_splits", P, G, k)
    nbytes = value("msml_search_topk_workspace", P, k, splits)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device="cuda")
    sc = torch.empty(P, k, dtype=dtype, device="cuda")
    ix = torch.empty(P, k, dtype=torch.int32, device="cuda")
    dt = identify._DT[dtype]
    routes = {
        "kernel": lambda: call("msml_search_topk", p, P, g, G, E, k, splits, dt, sc, ix, ws, nbytes),
        "search_topk": lambda: identify.search_topk(p, g, k, dtype=dtype),
        "torch": lambda: torch_route(p, g, k),
    }
    for fn in routes.values():                               # warm-up of every route at the timed shape
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in routes}
    for _ in range(reps):
        for n, fn in routes.items():
            ms[n].append(event_ms(fn))
    ts, ti = torch_route(p, g, k)
    same = float((ti == ix.long()).double().mean())
    err = float((ts - sc).abs().max())
    flop = 2.0 * P * G * E
    row = {"case": name, "dtype": str(dtype).replace("torch.", ""), "P": P, "G": G, "E": E, "k": k, "splits": splits,
           "workspace_bytes": int(nbytes), "full_matrix_bytes": int(P) * int(G) * p.element_size(),
           "index_equal_to_torch_route": round(same, 6), "max_score_diff_to_torch_route": err}
    for n in routes:
        med = float(np.median(ms[n]))
        row[n + "_ms"] = round(med, 3)
        row[n + "_ms_min_max"] = [round(min(ms[n]), 3), round(max(ms[n]), 3)]
        row[n + "_TFLOPs"] = round(flop / (med * 1e-3) / 1e12, 2)
    row["kernel_of_f32_matrix_peak"] = round(flop / (row["kernel_ms"] * 1e-3) / F32_MATRIX_PEAK, 3)
    row["torch_over_kernel"] = round(row["torch_ms"] / row["kernel_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--large-gallery", type=int, default=1000000)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for dtype in (torch.float32, torch.float64):
        rows.append(case("ijbc_gallery1", 19593, 1772, a.e, a.k, dtype, a.reps, gen))
        rows.append(case("large_gallery", 3530, a.large_gallery, a.e, a.k, dtype, a.reps, gen))
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "f32_matrix_peak_TFLOPs": F32_MATRIX_PEAK / 1e12,
           "torch_route_chunk_bytes": CHUNK_BYTES, "cases": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
