"""Time the template-verification chain at IJB-C size on synthetic data: 469 375 images x (512 | 512) f32,
23 124 templates, 15 658 489 pairs.  Every device stage is timed with events after a warm-up (median of --reps),
with the bytes it must move and the GB/s that makes; the same stages of the numpy / sklearn restatement
(tests/ijb_cases.py) on the host CPUs are the baseline (--no-cpu skips them, --cpu-pairs limits the pair stage and
scales its time).  Prints one JSON line; `--out FILE` also writes it.

    python tools/bench_ijb.py [--images N --templates T --pairs P --e E] [--reps 5] [--no-cpu] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from msml_amd import ijb  # noqa: E402
from msml_amd._lib import call, value  # noqa: E402
from tests import ijb_cases as C  # noqa: E402

COPY_RATE = 6.29e12        # bytes / s, the device's measured copy rate (read + write)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def stage(name, ms, nbytes, note=""):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"stage": name, "ms": round(ms, 3), "bytes": int(nbytes), "GB/s": round(gbs, 1),
            "of_copy_rate": round(gbs * 1e9 / COPY_RATE, 3), "note": note}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=469375)
    ap.add_argument("--templates", type=int, default=23124)
    ap.add_argument("--pairs", type=int, default=15658489)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-pairs", type=int, default=2000000)
    ap.add_argument("--out")
    a = ap.parse_args()
    n, t, p, e = a.images, a.templates, a.pairs, a.e
    g = torch.Generator(device="cuda").manual_seed(1)
    feats = torch.randn(n, 2 * e, generator=g, device="cuda")
    face = torch.rand(n, generator=g, device="cuda") * 0.8 + 0.2
    tid = (torch.rand(n, generator=g, device="cuda", dtype=torch.float64) ** 3 * t).long().clamp_(max=t - 1)
    tid[:t] = torch.randperm(t, generator=g, device="cuda")
    templates = (tid * 3 + 11).cpu().numpy()
    medias = torch.randint(0, 40, (n,), generator=g, device="cuda").cpu().numpy()
    # the protocol's pair file lists p1 in long runs
    p1 = (torch.randint(0, t, (p,), generator=g, device="cuda").sort()[0] * 3 + 11)
    p2 = (torch.randint(0, t, (p,), generator=g, device="cuda") * 3 + 11)
    label = (torch.rand(p, generator=g, device="cuda") < 0.001).to(torch.uint8)

    t0 = time.perf_counter()
    lay = ijb.segment_layout(templates, medias)
    layout_ms = (time.perf_counter() - t0) * 1e3
    rows = []
    out = {}

    def pool():
        out["tf"], out["ut"] = ijb.template_features(feats, templates, medias, face, layout=lay)
    ms = timed(pool, a.reps)
    rows.append(stage("template_pool", ms, n * 2 * e * 4 + n * 8 + t * e * 8 * 3, "read once; host call included"))
    tf, ut = out["tf"], out["ut"]
    r1, r2 = ijb.template_rows(ut, p1), ijb.template_rows(ut, p2)
    score = torch.empty(p, dtype=torch.float64, device="cuda")
    ms = timed(lambda: call("msml_template_pair_score", tf, t, e, r1, r2, p, score), a.reps)
    rows.append(stage("template_pair_score", ms, p * (2 * e * 8 + 16),
                      "bytes REQUESTED by the waves (two rows per pair); the matrix is %d MB" % (t * e * 8 // 10 ** 6)))
    rows[-1]["unique_bytes"] = int(t * e * 8 + p * 16)
    ms = timed(lambda: ijb.template_rows(ut, p1), a.reps)
    rows.append(stage("template_rows (torch.searchsorted, one list)", ms, p * 12, "plumbing"))
    srt = {}

    def sort():
        srt["s"], idx = torch.sort(score, descending=True)
        srt["y"] = label[idx].contiguous()
    ms = timed(sort, a.reps)
    rows.append(stage("torch.sort + label gather", ms, p * (8 + 8 + 8 + 1 + 1), "plumbing; ideal single pass"))
    ss, ys = srt["s"], srt["y"]
    blk = torch.empty(value("msml_roc_blocks", p), 2, dtype=torch.int32, device="cuda")
    ms = timed(lambda: call("msml_roc_block_counts", ss, ys, p, blk), a.reps)
    rows.append(stage("roc_block_counts", ms, p * 9))
    tab = blk.cpu().numpy().astype(np.int64)
    k = int(tab[:, 1].sum())
    off = torch.from_numpy((np.cumsum(tab, 0) - tab).astype(np.int32)).cuda()
    tps, fps = (torch.empty(k, dtype=torch.int32, device="cuda") for _ in range(2))
    ms = timed(lambda: call("msml_roc_points", ss, ys, p, off, tps, fps), a.reps)
    rows.append(stage("roc_points", ms, p * 9 + k * 8))
    tgt = torch.tensor(ijb.FPRS, dtype=torch.float64, device="cuda")
    keep = torch.empty(k, dtype=torch.uint8, device="cuda")
    part = torch.empty(value("msml_roc_reduce_blocks", k), 2 + 2 * len(ijb.FPRS), dtype=torch.int64, device="cuda")
    ms = timed(lambda: call("msml_roc_reduce", tps, fps, k, tgt, len(ijb.FPRS), keep, part), a.reps)
    rows.append(stage("roc_reduce", ms, k * 9 + part.numel() * 8))
    ms = timed(lambda: ijb.roc_table(score, label), a.reps)
    rows.append(stage("roc_table (sort, 3 kernels, host tables)", ms, p * 44))
    ms = timed(lambda: ijb.evaluate_templates(feats, templates, medias, p1, p2, label, faceness=face), 2)
    res = {"device": torch.cuda.get_device_name(0), "images": n, "templates": t, "pairs": p, "E": e, "roc_points": k,
           "max_rows": lay.max_rows, "segment_layout_host_ms": round(layout_ms, 1),
           "evaluate_templates_end_to_end_ms": round(ms, 1), "stages": rows}
    if not a.no_cpu:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        cpu = {}
        f_h, face_h, sc_h, lab_h = feats.cpu().numpy(), face.cpu().numpy(), score.cpu().numpy(), label.cpu().numpy()
        p1_h, p2_h = p1.cpu().numpy(), p2.cpu().numpy()
        t0 = time.perf_counter()
        tn, ut_r, _ = C.pool_ref(C.input_feats(f_h, face_h), templates, medias)
        cpu["pool_s"] = round(time.perf_counter() - t0, 2)
        q = min(p, a.cpu_pairs)
        t0 = time.perf_counter()
        C.scores_ref(tn, ut_r, p1_h[:q], p2_h[:q])
        cpu["pair_scores_s"] = round((time.perf_counter() - t0) * p / q, 2)
        cpu["pair_scores_measured_on_pairs"] = q
        t0 = time.perf_counter()
        C.roc_ref(sc_h, lab_h)
        cpu["roc_table_s"] = round(time.perf_counter() - t0, 2)
        cpu["threads"] = torch.get_num_threads()
        res["cpu_restatement"] = cpu
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
