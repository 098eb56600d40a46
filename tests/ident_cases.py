"""Shared by tests/test_ident_cpu.py, tests/test_gpu_ident.py and tools/bench_ident.py: a numpy restatement of the
1:N identification path (msml_amd/identify.py, csrc/search.hip) and the seeded case generators.

`topk_ref` is the f64 `p @ g.T` followed by np.lexsort((arange(G), -s)).  `metrics_ref` works from the FULL score
matrix (mate rank = number of gallery rows that come before the mate in that order), so it does not share the top-k
route with the code under test.  There is no reference script for these metrics: they restate the NIST open-set
definitions with the tie rule of msml_amd.identify."""
import math

import numpy as np

# (P, G, E, k, splits) of the f64 edge-shape test; None = the library's default split count
EDGE_SHAPES = [(1, 1, 4, 1, 1), (1, 10, 8, 10, 1), (63, 64, 4, 5, 1), (65, 65, 36, 10, 2), (130, 200, 512, 32, 1),
               (130, 200, 512, 32, 3), (130, 200, 512, 32, 7), (200, 333, 128, 20, None)]
END_TO_END = dict(seed=7, n_probe=130, n_gallery=300, e=128, mated=0.6, noise=3.5)


def scores_full(probe, gallery):
    return np.asarray(probe, np.float64) @ np.asarray(gallery, np.float64).T


def topk_ref(probe, gallery, k, full=None):
    """(scores [P][k] f64, index [P][k] int32): descending score, ties by ascending gallery row; -0.0 ties with 0.0."""
    s = scores_full(probe, gallery) if full is None else full
    g = s.shape[1]
    idx = np.stack([np.lexsort((np.arange(g), -(row + 0.0)))[:k] for row in s])      # + 0.0: -0.0 becomes 0.0
    return np.take_along_axis(s, idx, 1), idx.astype(np.int32)


def min_gap(full, k):
    """Smallest gap between consecutive reference scores among each row's first k + 1 (k when the row has no more)."""
    s = -np.sort(-full, axis=1)[:, :k + 1]
    return float(np.diff(-s, axis=1).min()) if s.shape[1] > 1 else float("inf")


def mate_rows_ref(probe_subjects, gallery_subjects):
    where = {int(s): i for i, s in enumerate(gallery_subjects)}
    return np.array([where.get(int(s), -1) for s in probe_subjects], np.int32)


def metrics_ref(full, mate, k, ranks=(1, 5, 10), fpirs=(0.01, 0.1)):
    """From the full P x G score matrix.  Returns the dict of identify.identification_metrics as plain numpy."""
    full = np.asarray(full, np.float64)
    mate = np.asarray(mate, np.int64)
    p, g = full.shape
    mated = mate >= 0
    rank = np.full(p, -1, np.int64)
    rows = np.arange(g)
    for i in np.flatnonzero(mated):
        sm = full[i, mate[i]]
        rank[i] = min(k, int(((full[i] > sm) | ((full[i] == sm) & (rows < mate[i]))).sum()))
    n_mated, n_non = int(mated.sum()), int((~mated).sum())
    cmc_count = np.array([int((rank[mated] < r).sum()) for r in ranks], np.int64)
    top1 = full.max(1)
    u = -np.sort(-top1[~mated])
    thr, tp, fa = [], [], []
    for f in fpirs:
        tau = u[int(math.floor(f * n_non))]
        thr.append(tau)
        fa.append(int((u > tau).sum()))
        tp.append(int((mated & (rank == 0) & (top1 > tau)).sum()))
    tp, fa = np.array(tp, np.int64), np.array(fa, np.int64)
    return {"mate_rank": rank.astype(np.int32), "n_mated": n_mated, "n_nonmated": n_non, "cmc": cmc_count / n_mated,
            "cmc_count": cmc_count, "thresholds": np.array(thr, np.float64), "tpir": tp / n_mated, "tpir_count": tp,
            "fpir_achieved": fa / max(n_non, 1)}


def distractor_ranks_ref(probe, mate, distractors, k):
    full = scores_full(probe, distractors)
    ms = (np.asarray(probe, np.float64) * np.asarray(mate, np.float64)).sum(1)
    return np.minimum((full > ms[:, None]).sum(1), k).astype(np.int32), ms


def unit_rows(rng, n, e):
    x = rng.standard_normal((n, e))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def integer_rows(rng, n, e, lo=-4, hi=4):
    """Exact in f32 and f64 products and sums: many ties."""
    return rng.integers(lo, hi + 1, (n, e)).astype(np.float64)


def make_identification(seed, n_probe, n_gallery, e, mated, noise):
    """One gallery row per subject (sparse shuffled ids); a share `mated` of the probes is its subject's gallery row
    plus noise * standard normal per channel / sqrt(e) before normalisation, the others are subjects the gallery does
    not hold.  Returns probe, probe_subjects, gallery, gallery_subjects."""
    rng = np.random.default_rng(seed)
    gallery = unit_rows(rng, n_gallery, e)
    ids = rng.choice(np.arange(5, 50 * (n_gallery + n_probe)), n_gallery + n_probe, replace=False).astype(np.int64)
    g_sub, spare = ids[:n_gallery], ids[n_gallery:]
    is_mated = rng.random(n_probe) < mated
    row = rng.integers(0, n_gallery, n_probe)
    probe = np.where(is_mated[:, None], gallery[row], 0.0) + noise / np.sqrt(e) * rng.standard_normal((n_probe, e))
    probe /= np.linalg.norm(probe, axis=1, keepdims=True)
    p_sub = np.where(is_mated, g_sub[row], spare)
    return probe, p_sub, gallery, g_sub
