"""All-pairs verification on the HIP path: exact TAR @ FAR over EVERY probe x gallery comparison, without the P x G
score matrix.

The MegaFace list writer of the reference (datasets/benchmarks/get_list.py:138-208) prepares two protocols: rank-1
identification against the distractors (msml_amd.identify) and verification, TAR at FAR = 1e-6 over all probe x gallery
pairs; the masked-face challenges use the same all-pairs figure.  The reference ships no evaluator for it, so there is
NO reference script to follow: the rule below is the one identify.identification_metrics uses for FPIR.

Pairs.  With a gallery every (p, g) is a pair; `gallery=None` is the symmetric mode: the pairs (i, j), i < j, among the
probe rows.  A pair is genuine when its two subject ids are equal, an impostor otherwise; a gallery may hold several
rows of a subject.  The score of a pair is the inner product of the two rows, -0.0 counted as 0.0, with the bits
`identify.search_topk` gives that pair for the same `dtype`.

Rule for a target f (0 <= f < 1): u = the impostor scores in descending order, a = floor(f * n_impostor), tau = u[a];
far_count = #{impostor > tau}, tar_count = #{genuine > tau}.  A score equal to tau is rejected, so far_count <= a.

Selection without the matrix.  A score maps to an order-preserving unsigned key of W = 32 (f32) or 64 (f64) bits: all
bits of a negative flipped, the sign bit of a non-negative set.  u[a] is found by a radix select on the keys:
  1. a histogram pass counts the impostors of up to HIST_BINS >> b ranges (prefix, prefix_bits) into 2^b bins each by
     the key's next b bits (b = BINS_LOG2, less at the last level);
  2. the host walks a target's bins from the top to the one that holds position a, adds the bins above it to the
     target's count of impostors above, and narrows the range; targets whose ranges coincide share a histogram;
  3. a target stops when its range is a single key, or holds at most `collect_cap` impostors: a collecting pass then
     fetches the scores of the range, they are sorted on the device and tau is read at position a - above;
  4. a count pass (`all_pairs_counts`) compares every score with the thresholds; its impostor counts must equal the
     ones the walk gave (RuntimeError otherwise).
All counters are integers and the order in which scores arrive does not matter, so the result depends neither on
`collect_cap`, `splits`, the bins per pass nor on the run.

* `all_pairs_roc(...)`: thresholds, counts and rates for FAR targets.
* `all_pairs_counts(...)`: genuine / impostor pairs above caller-given thresholds.
* `subject_codes(...)`: host side: dense int32 codes over both id sets and the exact pair counts.
* `score_keys`, `key_score`: the key of a score and back.

The passes come from a backend: by default the HIP library (csrc/allpairs.hip); any object with `hist(ranges, bits)`,
`collect(range)` and `count(thresholds)` serves (see HipBackend), which is how the tests run the walk without a GPU.
A backend that also has `collect_many(ranges)` is asked once for all ranges: HipBackend collects them in one pass.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, value
from .ijb import _ids

BINS_LOG2 = 12            # bins of a range per histogram pass: 2^12
HIST_BINS = 8192          # bins of one pass (the workgroup's LDS histogram): ranges per pass = HIST_BINS >> bits
MAX_TARGETS = 16          # FAR targets / thresholds of one call
HIST, COLLECT, COUNT = 0, 1, 2          # MSML_ALLPAIRS_*
_DT = {torch.float32: _lib.F32, torch.float64: _lib.F64}
_NP = {torch.float32: np.float32, torch.float64: np.float64}


def score_keys(scores):
    """numpy f32 / f64 scores -> uint32 / uint64 keys that order as the scores do (-0.0 as 0.0)."""
    s = np.ascontiguousarray(scores) + 0.0
    if s.dtype == np.float32:
        b = s.view(np.uint32)
        return np.where(b >> np.uint32(31), ~b, b | np.uint32(1 << 31))
    if s.dtype != np.float64:
        raise ValueError("score_keys: scores are %s" % s.dtype)
    b = s.view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))


def key_score(key, width):
    """The score of a key of `width` (32 / 64) bits as a Python float: the f32 / f64 value widened exactly."""
    key, top = int(key), 1 << (width - 1)
    bits = key ^ top if key & top else ~key & ((1 << width) - 1)
    if width == 32:
        return float(np.array([bits], np.uint32).view(np.float32)[0])
    return float(np.array([bits], np.uint64).view(np.float64)[0])


def subject_codes(probe_subjects, gallery_subjects=None):
    """Host side (numpy, no GPU).  One integer subject id per row -> (probe_code int32 [P], gallery_code int32 [G] or
    None, n_genuine, n_impostor): dense codes over the union of both id sets, and the exact pair counts as Python ints
    (they may exceed 2^32).  gallery_subjects=None: the symmetric mode, pairs i < j among the probe rows."""
    ps = _ids(probe_subjects, "probe_subjects")
    if gallery_subjects is None:
        _, code = np.unique(ps, return_inverse=True)
        c = np.bincount(code.reshape(-1)).astype(np.int64)
        gen = int((c * (c - 1) // 2).sum())
        return code.reshape(-1).astype(np.int32), None, gen, ps.size * (ps.size - 1) // 2 - gen
    gs = _ids(gallery_subjects, "gallery_subjects")
    uniq, code = np.unique(np.concatenate([ps, gs]), return_inverse=True)
    pc, gc = code.reshape(-1)[:ps.size], code.reshape(-1)[ps.size:]
    gen = int(np.dot(np.bincount(pc, minlength=uniq.size).astype(np.int64),
                     np.bincount(gc, minlength=uniq.size).astype(np.int64)))
    return pc.astype(np.int32), gc.astype(np.int32), gen, ps.size * gs.size - gen


def _checked_rows(a, name):
    """Shape and value checks of a row set WHERE IT LIVES (numpy or any tensor): nothing is copied to the device."""
    if isinstance(a, torch.Tensor):
        if a.is_complex() or a.dtype == torch.bool:
            raise ValueError("%s: dtype %s is not numeric" % (name, a.dtype))
    else:
        a = np.asarray(a)
        if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError("%s: dtype %s is not numeric" % (name, a.dtype))
    if a.ndim != 2 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("%s must be [rows][E], got %s" % (name, tuple(a.shape)))
    if a.shape[1] % 4:
        raise ValueError("%s: embedding size %d is not a multiple of 4" % (name, a.shape[1]))
    if a.shape[0] >= 2 ** 31 - 1:
        raise ValueError("%s: %d rows do not fit int32" % (name, a.shape[0]))
    return a


def _finite(a, name):
    ok = bool(torch.isfinite(a).all()) if isinstance(a, torch.Tensor) else bool(np.isfinite(a).all())
    if not ok:
        raise ValueError("%s holds NaN or infinity" % name)


class HipBackend:
    """The three passes on the device (msml_allpairs_pass).  p / g: [P][E] / [G][E] CUDA tensors in `dtype`, pcode /
    gcode their int32 subject codes on the device; g is None in the symmetric mode."""

    def __init__(self, p, pcode, g, gcode, dtype, splits=None, collect_cap=1 << 20):
        self.p, self.pcode, self.dtype = p, pcode, dtype
        self.symmetric = g is None
        self.g, self.gcode = (p, pcode) if g is None else (g, gcode)
        self.P, self.E = p.shape
        self.G = self.g.shape[0]
        self.splits = value("msml_allpairs_splits", self.P, self.G) if splits is None else int(splits)
        if not 1 <= self.splits <= 65535:
            raise ValueError("all_pairs: splits=%d outside 1..65535" % self.splits)
        self.cap = max(1, min(int(collect_cap), self.P * self.G))

    def _pass(self, mode, n_ranges=0, prefix=None, bits=None, bins_log2=0, hist=None, cand=None, cand_count=None,
              cap=0, thr=None, n_thr=0, counts=None):
        # prefix / bits / thr: numpy arrays the library reads on the host during the call
        call("msml_allpairs_pass", self.p, self.P, self.pcode, self.g, self.G, self.gcode, self.E, _DT[self.dtype],
             int(self.symmetric), mode, n_ranges, prefix.ctypes.data if prefix is not None else None,
             bits.ctypes.data if bits is not None else None, bins_log2, hist, cand, cand_count, cap,
             thr.ctypes.data if thr is not None else None, n_thr, counts, self.splits)

    def hist(self, ranges, bits):
        """ranges: at most HIST_BINS >> bits (prefix, prefix_bits) -> int64 [len(ranges)][1 << bits]: the impostors of
        every range by the next `bits` bits of their key."""
        prefix = np.array([r[0] for r in ranges], np.uint64)
        pbits = np.array([r[1] for r in ranges], np.int32)
        out = torch.zeros(len(ranges), 1 << bits, dtype=torch.int64, device=self.p.device)
        self._pass(HIST, len(ranges), prefix, pbits, bits, hist=out)
        return out.cpu().numpy()

    def collect_many(self, ranges):
        """One pass for at most 16 ranges (prefix, prefix_bits): per range the keys of the impostors inside it, sorted
        descending (numpy)."""
        prefix = np.array([r[0] for r in ranges], np.uint64)
        pbits = np.array([r[1] for r in ranges], np.int32)
        cand = torch.empty(len(ranges), self.cap, dtype=self.dtype, device=self.p.device)
        n = torch.zeros(len(ranges), dtype=torch.int64, device=self.p.device)
        self._pass(COLLECT, len(ranges), prefix, pbits, cand=cand, cand_count=n, cap=self.cap)
        n = n.cpu().tolist()
        if max(n) > self.cap:
            raise RuntimeError("all_pairs: a range holds %d impostors, the collecting buffer %d" % (max(n), self.cap))
        return [score_keys(torch.sort(cand[i, :c], descending=True).values.cpu().numpy()) for i, c in enumerate(n)]

    def collect(self, rng):
        """The keys of the impostors inside rng = (prefix, prefix_bits), sorted descending (numpy)."""
        return self.collect_many([rng])[0]

    def count(self, thresholds):
        """thresholds: f64 -> (genuine_above, impostor_above), int64 [T] each: pairs with score > threshold."""
        thr = np.ascontiguousarray(thresholds, np.float64)
        out = torch.zeros(2, thr.size, dtype=torch.int64, device=self.p.device)
        self._pass(COUNT, thr=thr, n_thr=thr.size, counts=out)
        out = out.cpu().numpy()
        return out[0], out[1]


def _prepare(name, probe, probe_subjects, gallery, gallery_subjects, dtype, splits, backend, collect_cap=1 << 20):
    """Every check that needs no launch, the subject codes, and the backend.  -> (backend, n_genuine, n_impostor)."""
    if dtype not in _DT:
        raise ValueError("%s: dtype %s is not torch.float32 or torch.float64" % (name, dtype))
    if (gallery is None) != (gallery_subjects is None):
        raise ValueError("%s: gallery and gallery_subjects come together (neither: the symmetric mode)" % name)
    p = _checked_rows(probe, name + ": probe")
    g = None if gallery is None else _checked_rows(gallery, name + ": gallery")
    if g is not None and g.shape[1] != p.shape[1]:
        raise ValueError("%s: probe rows hold %d channels, gallery rows %d" % (name, p.shape[1], g.shape[1]))
    pcode, gcode, n_gen, n_imp = subject_codes(probe_subjects, gallery_subjects)
    if pcode.size != p.shape[0] or (g is not None and gcode.size != g.shape[0]):
        raise ValueError("%s: one subject id per probe row and per gallery row" % name)
    if n_gen == 0 or n_imp == 0:
        raise ValueError("%s: %d genuine and %d impostor pairs: needs both" % (name, n_gen, n_imp))
    _finite(p, name + ": probe")
    if g is not None:
        _finite(g, name + ": gallery")
    if backend is None:
        from .identify import _rows                 # to the device and to `dtype` as search_topk converts its inputs
        p = _rows(p, dtype, name + ": probe")
        pcode = torch.from_numpy(pcode).to(p.device)
        if g is not None:
            g = _rows(g, dtype, name + ": gallery").to(p.device)
            gcode = torch.from_numpy(gcode).to(p.device)
        backend = HipBackend(p, pcode, g, gcode, dtype, splits, collect_cap)
    return backend, n_gen, n_imp


def _select(backend, width, n_impostor, positions, collect_cap, bins_log2=BINS_LOG2):
    """The radix walk.  positions: 0-based places in the descending impostor order.  -> (keys, above, passes): per
    target the key at its position and the number of impostor keys greater than it."""
    T = len(positions)
    prefix, bits, above, inside = [0] * T, [0] * T, [0] * T, [n_impostor] * T
    passes = 0
    while True:
        active = [t for t in range(T) if bits[t] < width and inside[t] > collect_cap]
        if not active:
            break
        depth = bits[active[0]]                     # the active targets have all narrowed at every level so far
        assert all(bits[t] == depth for t in active)
        b = min(bins_log2, width - depth)
        ranges = sorted({(prefix[t], depth) for t in active})
        per_pass = max(1, HIST_BINS >> b)
        table = {}
        for i in range(0, len(ranges), per_pass):
            chunk = ranges[i:i + per_pass]
            h = np.asarray(backend.hist(chunk, b)).astype(np.int64)
            passes += 1
            if h.shape != (len(chunk), 1 << b):
                raise RuntimeError("all_pairs: histogram of shape %s for %d ranges of %d bins" % (h.shape, len(chunk), 1 << b))
            table.update(zip(chunk, h))
        for t in active:
            desc = table[(prefix[t], depth)][::-1]  # from the top bin down
            cum = np.cumsum(desc)
            if int(cum[-1]) != inside[t]:
                raise RuntimeError("all_pairs: range (%#x, %d) holds %d impostors, its histogram %d"
                                   % (prefix[t], depth, inside[t], int(cum[-1])))
            k = int(np.searchsorted(cum, positions[t] - above[t], side="right"))    # the first bin with cum > position
            above[t] += int(cum[k - 1]) if k else 0
            inside[t] = int(desc[k])
            prefix[t] = (prefix[t] << b) | ((1 << b) - 1 - k)
            bits[t] = depth + b
    keys = [0] * T
    todo = sorted({(prefix[t], bits[t]) for t in range(T) if bits[t] < width})
    if todo and hasattr(backend, "collect_many"):   # one pass for all ranges
        collected = dict(zip(todo, backend.collect_many(todo)))
        passes += 1
    else:
        collected = {rng: backend.collect(rng) for rng in todo}
        passes += len(todo)
    for t in range(T):
        if bits[t] == width:                        # a single key: every impostor of the range equals it
            keys[t] = prefix[t]
            continue
        rng = (prefix[t], bits[t])
        ks = np.asarray(collected[rng])
        if ks.size != inside[t] or (ks.size > 1 and bool((ks[:-1] < ks[1:]).any())):
            raise RuntimeError("all_pairs: range (%#x, %d) holds %d impostors, %d were collected (or not sorted)"
                               % (rng[0], rng[1], inside[t], ks.size))
        keys[t] = int(ks[positions[t] - above[t]])
        if bits[t] and keys[t] >> (width - bits[t]) != prefix[t]:
            raise RuntimeError("all_pairs: key %#x lies outside its range (%#x, %d)" % (keys[t], rng[0], rng[1]))
        above[t] += int(np.count_nonzero(ks > ks.dtype.type(keys[t])))
    return keys, above, passes


@torch.no_grad()
def all_pairs_counts(probe, probe_subjects, gallery=None, gallery_subjects=None, thresholds=(), dtype=torch.float64,
                     splits=None, backend=None):
    """probe [P][E], gallery [G][E] (None: symmetric mode), one integer subject id per row; numpy or CUDA tensors,
    converted to `dtype` (torch.float32 / torch.float64) as search_topk converts them.  Returns a dict: `n_genuine`,
    `n_impostor` (Python ints), `thresholds` (f64 numpy) and `genuine_above` / `impostor_above` (int64 numpy [T]): the
    pairs whose score, widened to f64, is > the threshold.  At most 16 thresholds; none gives empty arrays and no pass.
    ValueError as all_pairs_roc, and for a NaN threshold."""
    thr = np.array([float(t) for t in thresholds], np.float64)
    if thr.size > MAX_TARGETS:
        raise ValueError("all_pairs_counts: %d thresholds, at most %d" % (thr.size, MAX_TARGETS))
    if np.isnan(thr).any():
        raise ValueError("all_pairs_counts: a threshold is NaN")
    backend, n_gen, n_imp = _prepare("all_pairs_counts", probe, probe_subjects, gallery, gallery_subjects, dtype, splits,
                                     backend)
    gen = imp = np.zeros(0, np.int64)
    if thr.size:
        gen, imp = (np.asarray(c).astype(np.int64) for c in backend.count(thr))
    return {"n_genuine": n_gen, "n_impostor": n_imp, "thresholds": thr, "genuine_above": gen, "impostor_above": imp}


@torch.no_grad()
def all_pairs_roc(probe, probe_subjects, gallery=None, gallery_subjects=None, fars=(1e-6, 1e-5, 1e-4, 1e-3),
                  dtype=torch.float64, collect_cap=1 << 20, splits=None, backend=None):
    """TAR @ FAR over all pairs by the rule of the module text.  Inputs as all_pairs_counts.  fars: at most 16 targets
    in [0, 1).  collect_cap: a range with at most this many impostors is fetched and sorted instead of narrowed further
    (>= 1); splits: ranges the gallery columns are cut into (None: msml_allpairs_splits); neither changes the result.
    Returns a dict:

    n_genuine, n_impostor    Python ints
    fars                     the targets
    thresholds               f64 numpy: tau, exactly the f32 / f64 score widened
    far_count, tar_count     int64 numpy: #{impostor > tau}, #{genuine > tau}
    far_achieved, tar        f64 numpy: the counts over n_impostor / n_genuine
    passes                   kernel passes over the P x G tiles (histogram + collecting + the count pass)

    ValueError before any launch for non-finite rows, E % 4 != 0, row counts that do not fit int32, an id count that
    does not match the rows, gallery_subjects without gallery or the reverse, no genuine or no impostor pair, a target
    outside [0, 1), more than 16 targets, another dtype, collect_cap < 1.  RuntimeError when the count pass disagrees
    with the walk."""
    fars = [float(f) for f in fars]
    if len(fars) > MAX_TARGETS:
        raise ValueError("all_pairs_roc: %d targets, at most %d" % (len(fars), MAX_TARGETS))
    if any(not 0.0 <= f < 1.0 for f in fars):
        raise ValueError("all_pairs_roc: FAR targets %s outside [0, 1)" % (fars,))
    collect_cap = int(collect_cap)
    if collect_cap < 1:
        raise ValueError("all_pairs_roc: collect_cap=%d" % collect_cap)
    backend, n_gen, n_imp = _prepare("all_pairs_roc", probe, probe_subjects, gallery, gallery_subjects, dtype, splits,
                                     backend, collect_cap)
    width = 32 if dtype == torch.float32 else 64
    positions = [min(int(math.floor(f * n_imp)), n_imp - 1) for f in fars]
    keys, above, passes = _select(backend, width, n_imp, positions, collect_cap)
    thr = np.array([key_score(k, width) for k in keys], np.float64)
    far_count = np.array(above, np.int64)
    tar_count = np.zeros(0, np.int64)
    if fars:
        gen, imp = (np.asarray(c).astype(np.int64) for c in backend.count(thr))
        passes += 1
        if not np.array_equal(imp, far_count):
            raise RuntimeError("all_pairs_roc: the count pass finds %s impostors above the thresholds, the radix walk %s"
                               % (imp.tolist(), far_count.tolist()))
        tar_count = gen
    return {"n_genuine": n_gen, "n_impostor": n_imp, "fars": tuple(fars), "thresholds": thr, "far_count": far_count,
            "tar_count": tar_count, "far_achieved": far_count / n_imp, "tar": tar_count / n_gen, "passes": passes}
