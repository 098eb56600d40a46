"""Shared by tests/test_allpairs_cpu.py and tests/test_gpu_allpairs.py: a numpy restatement of the all-pairs
verification path (msml_amd/allpairs.py, csrc/allpairs.hip) and the seeded case generators.

`allpairs_ref` works from the FULL f64 score matrix: it masks, sorts and counts, and shares nothing with the radix
route of the code under test.  `radix_select_ref` restates the selection on keys, `NumpyBackend` serves the three
passes of msml_amd.allpairs from a stored score matrix so that the host side of the walk runs without a GPU.  There is
no reference script for these figures: the rule (a = floor(f * n_impostor), tau = u[a] of the descending impostor
scores, a score equal to tau is rejected) is the one msml_amd.identify uses for FPIR."""
import math

import numpy as np

from tests.ident_cases import integer_rows, unit_rows  # noqa: F401  (re-exported for the tests)

INT_SHAPES = [(1, 2, 4), (63, 64, 4), (65, 65, 36), (70, 75, 128), (130, 200, 512)]      # (P, G, E)
INT_FARS = (0.0, 1e-3, 1e-2, 1e-1)
REAL_CONFIGS = [dict(seed=11, n_subjects=120, e=128, noise=3.5), dict(seed=12, n_subjects=60, e=512, noise=3.0)]
REAL_FARS = (0.0, 1e-3, 1e-2, 1e-1)


def key32(x):
    """f32 scores -> uint32 keys: all bits of a negative flipped, the sign bit of a non-negative set; -0.0 as 0.0."""
    b = (np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000))


def key64(x):
    b = (np.asarray(x, np.float64) + 0.0).view(np.uint64)
    return np.where(b & np.uint64(1 << 63), b ^ np.uint64(0xFFFFFFFFFFFFFFFF), b ^ np.uint64(1 << 63))


def pair_masks(probe_subjects, gallery_subjects, symmetric):
    """(genuine, impostor) boolean [P][G]; symmetric: only i < j."""
    ps, gs = np.asarray(probe_subjects), np.asarray(probe_subjects if symmetric else gallery_subjects)
    same = ps[:, None] == gs[None, :]
    pair = np.triu(np.ones(same.shape, bool), 1) if symmetric else np.ones(same.shape, bool)
    return same & pair, ~same & pair


def allpairs_ref(full, probe_subjects, gallery_subjects, fars, symmetric):
    """From the full f64 P x G score matrix.  Returns the dict of allpairs.all_pairs_roc (without `passes`)."""
    full = np.asarray(full, np.float64) + 0.0
    gen_m, imp_m = pair_masks(probe_subjects, gallery_subjects, symmetric)
    gen, u = full[gen_m], -np.sort(-full[imp_m])
    thr, fa, ta = [], [], []
    for f in fars:
        tau = u[int(math.floor(f * u.size))]
        thr.append(tau)
        fa.append(int((u > tau).sum()))
        ta.append(int((gen > tau).sum()))
    fa, ta = np.array(fa, np.int64), np.array(ta, np.int64)
    return {"n_genuine": int(gen.size), "n_impostor": int(u.size), "fars": tuple(fars),
            "thresholds": np.array(thr, np.float64), "far_count": fa, "tar_count": ta, "far_achieved": fa / u.size,
            "tar": ta / gen.size}


def threshold_margin(full, probe_subjects, gallery_subjects, thresholds, symmetric):
    """Smallest distance of any pair's reference score from a threshold, the scores equal to it left out."""
    gen_m, imp_m = pair_masks(probe_subjects, gallery_subjects, symmetric)
    s = np.asarray(full, np.float64)[gen_m | imp_m]
    d = np.abs(s[:, None] - np.asarray(thresholds)[None, :])
    return float(d[d > 0].min())


def radix_select_ref(keys, a, width, b=12, cap=1):
    """The key at 0-based position `a` of the descending order of `keys` (uint32 / uint64, width 32 / 64) by radix:
    narrow by b bits per level while the range holds more than `cap` keys and is not a single key, then sort what is
    left.  Returns (key, number of keys greater than it, levels)."""
    keys = np.asarray(keys)
    inside, bits, above, levels = keys, 0, 0, 0
    while bits < width and inside.size > cap:
        step = min(b, width - bits)
        digit = ((inside >> inside.dtype.type(width - bits - step)) & inside.dtype.type((1 << step) - 1)).astype(np.int64)
        count = np.bincount(digit, minlength=1 << step)
        d = (1 << step) - 1
        while above + count[d] <= a:
            above += int(count[d])
            d -= 1
        inside, bits, levels = inside[digit == d], bits + step, levels + 1
    key = np.sort(inside)[::-1][a - above]
    return int(key), above + int((inside > key).sum()), levels


class NumpyBackend:
    """The three passes of msml_amd.allpairs from a stored score matrix in f32 or f64 (its dtype picks the key width).
    `log` lists the calls."""

    def __init__(self, scores, probe_subjects, gallery_subjects, symmetric):
        scores = np.asarray(scores)
        assert scores.dtype in (np.float32, np.float64)
        gen_m, imp_m = pair_masks(probe_subjects, gallery_subjects, symmetric)
        self.gen, self.imp = scores[gen_m].astype(np.float64), scores[imp_m]
        self.width = 32 if scores.dtype == np.float32 else 64
        self.keys = key32(self.imp) if self.width == 32 else key64(self.imp)
        self.log = []

    def _inside(self, rng):
        prefix, bits = rng
        if bits == 0:
            return self.keys
        return self.keys[(self.keys >> self.keys.dtype.type(self.width - bits)) == self.keys.dtype.type(prefix)]

    def hist(self, ranges, bits):
        self.log.append(("hist", tuple(ranges), bits))
        out = np.zeros((len(ranges), 1 << bits), np.int64)
        for i, rng in enumerate(ranges):
            k = self._inside(rng)
            digit = (k >> k.dtype.type(self.width - rng[1] - bits)) & k.dtype.type((1 << bits) - 1)
            out[i] = np.bincount(digit.astype(np.int64), minlength=1 << bits)
        return out

    def collect(self, rng):
        self.log.append(("collect", rng))
        return np.sort(self._inside(rng))[::-1]

    def count(self, thresholds):
        self.log.append(("count", tuple(thresholds)))
        imp = self.imp.astype(np.float64)
        return (np.array([(self.gen > t).sum() for t in thresholds], np.int64),
                np.array([(imp > t).sum() for t in thresholds], np.int64))


def make_verification(seed, n_subjects, e, noise, max_rows=3):
    """1 .. max_rows unit rows per subject around a unit centre (noise * standard normal per channel / sqrt(e) before
    normalisation), sparse shuffled subject ids, rows in random order.  Returns rows [n][e], subject ids [n]."""
    rng = np.random.default_rng(seed)
    centers = unit_rows(rng, n_subjects, e)
    cnt = rng.integers(1, max_rows + 1, n_subjects)
    sub = np.repeat(np.arange(n_subjects), cnt)
    x = centers[sub] + noise / np.sqrt(e) * rng.standard_normal((len(sub), e))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    ids = rng.choice(np.arange(5, 50 * n_subjects), n_subjects, replace=False)
    perm = rng.permutation(len(sub))
    return x[perm], ids[sub][perm].astype(np.int64)


def split_rows(x, ids):
    """The asymmetric split: the first n * 2 // 5 rows are probes, the others the gallery."""
    n = len(x) * 2 // 5
    return x[:n], ids[:n], x[n:], ids[n:]


def integer_case(seed, p, g, e, n_subjects=None):
    """Integer rows (exact scores in f32 and f64, many ties) with subjects drawn so that genuine pairs exist."""
    rng = np.random.default_rng(seed)
    n_subjects = n_subjects or max(1, min(p, g) // 3)
    probe, gallery = integer_rows(rng, p, e), integer_rows(rng, g, e)     # |partial sums| <= 16 e < 2^24: exact in f32
    ps, gs = rng.integers(0, n_subjects, p) * 7 + 3, rng.integers(0, n_subjects, g) * 7 + 3
    ps[0] = gs[0]                                           # at least one genuine pair
    if (ps[:, None] == gs[None, :]).all():
        gs[-1] = gs[0] + 7                                  # ... and one impostor pair
    return probe, ps.astype(np.int64), gallery, gs.astype(np.int64)
