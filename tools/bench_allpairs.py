"""Time all-pairs verification (msml_amd.allpairs.all_pairs_roc, csrc/allpairs.hip) at the size of the MegaFace list:
3 530 probes x 1 000 000 gallery rows, E = 512, FAR targets 1e-6 .. 1e-3, f32 and f64, on synthetic rows (unit-norm,
a few rows per subject), against what a user would write today on the same device: chunked torch.matmul with a running
top-(a + 1) list of the impostor scores for the thresholds (one list for the largest target; the others read their
position in it), then a second chunked matmul that compares every score with the thresholds.

Per dtype, after a warm-up, --reps timed repeats with the routes ALTERNATING (device events, median):
    first_hist_ms     one histogram pass over all keys (range (0, 0), 2^12 bins): nearly every lane hits one bin
    deep_hist_ms      one histogram pass at the second level (the ranges the first walk step gives the targets)
    collect_ms        one collecting pass of the range the first target ends in
    count_ms          one count pass with the thresholds found
    all_pairs_roc_ms  the whole call as made from Python (host walk, syncs and allocations included), and `passes`
    torch_ms          the torch route
--passes-only leaves the torch route out (to time another build of the library, selected with MSML_LIB).  Results of
the two routes are compared at the timed size.  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_allpairs.py [--reps 5] [--gallery 1000000] [--passes-only] [--out profiles/allpairs_bench.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import _lib, allpairs  # noqa: E402

FARS = (1e-6, 1e-5, 1e-4, 1e-3)
CHUNK_BYTES = 1 << 30          # score chunk of the torch route
ROWS_PER_SUBJECT = 4           # of the synthetic gallery; every probe row is one more row of a gallery subject


def make_rows(P, G, E, dtype, gen):
    """Gallery: G / 4 subjects, 4 noisy unit rows each; probes: noisy rows of the first P subjects."""
    n_sub = max(P, G // ROWS_PER_SUBJECT)
    centers = torch.randn(n_sub, E, generator=gen, device="cuda", dtype=torch.float32)
    gs = torch.arange(G, device="cuda") % n_sub
    ps = torch.arange(P, device="cuda")

    def rows(sub):
        x = centers[sub] + 1.5 * torch.randn(sub.numel(), E, generator=gen, device="cuda", dtype=torch.float32)
        return (x / x.norm(dim=1, keepdim=True)).to(dtype)
    return rows(ps), ps.cpu().numpy(), rows(gs), gs.cpu().numpy()


def torch_route(p, pc, g, gc, positions):
    """Thresholds by a running descending list of the max(positions) + 1 largest impostor scores, counts by a second
    pass.  pc / gc: subject codes on the device."""
    k = max(positions) + 1
    cols = max(1, CHUNK_BYTES // (p.shape[0] * p.element_size()))
    best = None
    for c0 in range(0, g.shape[0], cols):
        s = p @ g[c0:c0 + cols].T
        s.masked_fill_(pc[:, None] == gc[None, c0:c0 + cols], -math.inf)
        s = torch.topk(s.reshape(-1), min(k, s.numel())).values
        best = s if best is None else torch.topk(torch.cat([best, s]), min(k, best.numel() + s.numel())).values
    thr = best[torch.tensor(positions, device=p.device)]
    gen = torch.zeros(len(positions), dtype=torch.int64, device=p.device)
    imp = torch.zeros_like(gen)
    for c0 in range(0, g.shape[0], cols):
        s = p @ g[c0:c0 + cols].T
        same = pc[:, None] == gc[None, c0:c0 + cols]
        for t in range(len(positions)):
            above = s > thr[t]
            gen[t] += (above & same).sum()
            imp[t] += (above & ~same).sum()
    return thr, gen, imp


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def case(P, G, E, dtype, reps, gen, passes_only):
    p, ps, g, gs = make_rows(P, G, E, dtype, gen)
    pcode, gcode, n_gen, n_imp = allpairs.subject_codes(ps, gs)
    pc, gc = torch.from_numpy(pcode).cuda(), torch.from_numpy(gcode).cuda()
    be = allpairs.HipBackend(p, pc, g, gc, dtype)
    width = 32 if dtype == torch.float32 else 64
    positions = [int(math.floor(f * n_imp)) for f in FARS]
    res = allpairs.all_pairs_roc(p, ps, g, gs, fars=FARS, dtype=dtype)                 # also the warm-up
    # the ranges of the second level and the range the first target is collected from, by the walk's own first steps
    first = be.hist([(0, 0)], allpairs.BINS_LOG2)[0][::-1].cumsum()
    deep = sorted({(4095 - int(np.searchsorted(first, a, side="right")), allpairs.BINS_LOG2) for a in positions})
    deep = deep[:allpairs.HIST_BINS >> allpairs.BINS_LOG2]
    key0 = int(allpairs.score_keys(res["thresholds"][:1].astype(allpairs._NP[dtype]))[0])
    rng0 = (key0 >> (width - 2 * allpairs.BINS_LOG2), 2 * allpairs.BINS_LOG2)
    routes = {
        "first_hist": lambda: be.hist([(0, 0)], allpairs.BINS_LOG2),
        "deep_hist": lambda: be.hist(deep, allpairs.BINS_LOG2),
        "collect": lambda: be.collect(rng0),
        "count": lambda: be.count(res["thresholds"]),
        "all_pairs_roc": lambda: allpairs.all_pairs_roc(p, ps, g, gs, fars=FARS, dtype=dtype),
    }
    if not passes_only:
        routes["torch"] = lambda: torch_route(p, pc, g, gc, positions)
    for fn in routes.values():                               # warm-up of every route at the timed shape
        fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in routes}
    for _ in range(reps):
        for n, fn in routes.items():
            ms[n].append(event_ms(fn))
    row = {"dtype": str(dtype).replace("torch.", ""), "P": P, "G": G, "E": E, "fars": list(FARS), "splits": be.splits,
           "n_genuine": n_gen, "n_impostor": n_imp, "passes": res["passes"], "deep_hist_ranges": len(deep),
           "collected_keys": int(be.collect(rng0).size), "thresholds": res["thresholds"].tolist(),
           "far_count": res["far_count"].tolist(), "tar": res["tar"].tolist(),
           "full_matrix_bytes": int(P) * int(G) * p.element_size()}
    for n in routes:
        row[n + "_ms"] = round(float(np.median(ms[n])), 3)
        row[n + "_ms_min_max"] = [round(min(ms[n]), 3), round(max(ms[n]), 3)]
    if not passes_only:
        thr, tgen, timp = torch_route(p, pc, g, gc, positions)
        row["max_threshold_diff_to_torch_route"] = float((thr.double().cpu() - torch.from_numpy(res["thresholds"])).abs().max())
        row["far_count_torch_route"] = timp.tolist()
        row["tar_count_equal_to_torch_route"] = bool((tgen.cpu().numpy() == res["tar_count"]).all())
        row["torch_over_all_pairs_roc"] = round(row["torch_ms"] / row["all_pairs_roc_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--probes", type=int, default=3530)
    ap.add_argument("--gallery", type=int, default=1000000)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--passes-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for name in a.dtypes.split(","):
        rows.append(case(a.probes, a.gallery, a.e, {"f32": torch.float32, "f64": torch.float64}[name], a.reps, gen,
                         a.passes_only))
        torch.cuda.empty_cache()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "library": os.path.basename(_lib.LIBPATH),
           "torch_route_chunk_bytes": CHUNK_BYTES, "cases": rows}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
