"""1:N identification on the HIP path: gallery search, rank-k accuracy (CMC) and the open-set rates TPIR @ FPIR.

The reference prepares identification lists and ships no evaluator for them: datasets/benchmarks/get_list.py:138-208
writes the MegaFace list (1 000 000 distractors under label 9999 plus FaceScrub probe / mate pairs), :100-135 the AR
list; IJB-C has an official 1:N part (two galleries, one probe set) on the template features msml_amd.ijb pools.  There
is therefore NO reference script to follow here: the metrics below are the NIST open-set definitions (FRVT 1:N: FPIR =
share of non-mated searches with a candidate above the threshold, TPIR = share of mated searches whose mate is first
and above it) with the tie rules stated at each function.

* `search_topk(probe, gallery, k)`: for every probe row the k largest inner products with the gallery rows, in
  descending score, ties by ascending gallery row (csrc/search.hip).  The P x G score matrix is never stored: the
  workspace is splits * P * k entries.  The result has the same bits for every `splits` and in every run.
* `mate_rows(probe_subjects, gallery_subjects)`: host side: the gallery row of every probe's subject, or -1.
* `identification_metrics(topk_scores, topk_index, mate)`: mate ranks, CMC, thresholds, TPIR and achieved FPIR.
* `identify(...)` chains the three; `identify_templates(...)` gathers template rows first (one IJB-C gallery per
  call: the protocol's figure is the mean over its two galleries, which the caller takes).
* `distractor_ranks(probe, mate, distractors)`: the MegaFace protocol: each (probe, mate) pair against G distractors.

Inputs may be numpy arrays or CUDA tensors, as in msml_amd.ijb; scores and indices stay on the device, the small
tables come back as numpy.
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, value
from .ijb import _dev, _ids, template_rows

KMAX = 32
_DT = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _rows(a, dtype, name):
    if not isinstance(a, torch.Tensor):
        a = np.asarray(a)
        if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError("%s: dtype %s is not numeric" % (name, a.dtype))
    elif a.is_complex() or a.dtype == torch.bool:
        raise ValueError("%s: dtype %s is not numeric" % (name, a.dtype))
    a = _dev(a, dtype)
    if a.dim() != 2 or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("%s must be [rows][E], got %s" % (name, tuple(a.shape)))
    if not bool(torch.isfinite(a).all()):
        raise ValueError("%s holds NaN or infinity" % name)
    return a


@torch.no_grad()
def search_topk(probe, gallery, k=10, splits=None, dtype=torch.float64):
    """probe [P][E], gallery [G][E] -> (scores [P][k] in `dtype`, index [P][k] int32), both on the device: for every
    probe row the k largest <probe row, gallery row>, descending, ties by ascending gallery row (-0.0 == 0.0): the order
    of np.lexsort((arange(G), -s)).  dtype: torch.float64 (f64 MFMA) or torch.float32; the inputs are converted to it.
    splits: ranges the gallery is cut into (None: msml_search_topk_splits); the result does not depend on it.
    ValueError for non-finite inputs, shapes that do not match, another dtype, k outside 1..32, k > G, E % 4 != 0."""
    if dtype not in _DT:
        raise ValueError("search_topk: dtype %s is not torch.float32 or torch.float64" % (dtype,))
    k = int(k)
    if not 1 <= k <= KMAX:
        raise ValueError("search_topk: k=%d outside 1..%d" % (k, KMAX))
    p, g = _rows(probe, dtype, "search_topk: probe"), _rows(gallery, dtype, "search_topk: gallery")
    if g.device != p.device:
        g = g.to(p.device)
    P, E = p.shape
    G = g.shape[0]
    if g.shape[1] != E:
        raise ValueError("search_topk: probe rows hold %d channels, gallery rows %d" % (E, g.shape[1]))
    if E % 4:
        raise ValueError("search_topk: embedding size %d is not a multiple of 4" % E)
    if k > G:
        raise ValueError("search_topk: k=%d exceeds the %d gallery rows" % (k, G))
    if P >= 2 ** 31 - 1 or G >= 2 ** 31 - 1:
        raise ValueError("search_topk: %d x %d rows do not fit int32" % (P, G))
    splits = value("msml_search_topk_splits", P, G, k) if splits is None else int(splits)
    if not 1 <= splits <= 65535:
        raise ValueError("search_topk: splits=%d outside 1..65535" % splits)
    scores = torch.empty(P, k, dtype=dtype, device=p.device)
    index = torch.empty(P, k, dtype=torch.int32, device=p.device)
    nbytes = value("msml_search_topk_workspace", P, k, splits)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device) if nbytes else None
    call("msml_search_topk", p, P, g, G, E, k, splits, _DT[dtype], scores, index, ws, nbytes)
    return scores, index


def mate_rows(probe_subjects, gallery_subjects):
    """Host side (numpy, no GPU).  int32 [P]: the gallery row whose subject id equals the probe's, -1 when the gallery
    does not hold the subject (a non-mated probe).  A gallery with a repeated subject is refused with ValueError (the
    IJB-C galleries hold one template per subject), and so are ids that are not integers."""
    ps, gs = _ids(probe_subjects, "probe_subjects"), _ids(gallery_subjects, "gallery_subjects")
    if gs.size == 0:
        raise ValueError("mate_rows: empty gallery")
    order = np.argsort(gs, kind="stable")
    sg = gs[order]
    dup = np.flatnonzero(sg[1:] == sg[:-1])
    if dup.size:
        raise ValueError("mate_rows: subject %d has more than one gallery row" % sg[dup[0]])
    pos = np.minimum(np.searchsorted(sg, ps), sg.size - 1)
    return np.where(sg[pos] == ps, order[pos], -1).astype(np.int32)


def _cpu_or_dev(a, dtype=None):
    """numpy -> CPU tensor; tensors stay where they are."""
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None and a.dtype != dtype:
        a = a.to(dtype)
    return a


@torch.no_grad()
def identification_metrics(topk_scores, topk_index, mate, ranks=(1, 5, 10), fpirs=(0.01, 0.1)):
    """topk_scores / topk_index [P][k]: search_topk's result (CPU or CUDA tensors, or numpy); mate [P]: mate_rows'
    result.  Returns a dict:

    mate_rank       int32 [P] (on the scores' device): -1 for a non-mated probe; the 0-based position of the mate in
                    the probe's list; k when the mate is not within the first k
    n_mated, n_nonmated
    cmc             numpy f64 [len(ranks)]: #{mated: mate_rank < r} / n_mated;  cmc_count: the numerators
    thresholds, tpir, fpir_achieved
                    numpy f64 [len(fpirs)].  For a target f (0 <= f < 1): u = the top-1 scores of the non-mated probes
                    sorted descending, a = floor(f * n_nonmated), tau = u[a]; fpir_achieved = #{u > tau} / n_nonmated
                    (at most f; smaller when scores tie with tau); tpir = #{mated: mate_rank == 0 and top-1 score >
                    tau} / n_mated.  tpir_count: the numerators

    ValueError when max(ranks) > k, when there is no mated probe, for a target outside [0, 1), and when fpirs is not
    empty and there is no non-mated probe.  fpirs=() evaluates the closed set only."""
    s = _cpu_or_dev(topk_scores)
    idx = _cpu_or_dev(topk_index).to(s.device)
    m = _cpu_or_dev(mate).to(s.device).reshape(-1).to(torch.int64)
    if s.dim() != 2 or idx.shape != s.shape or s.shape[0] == 0 or s.shape[1] == 0 or m.numel() != s.shape[0]:
        raise ValueError("identification_metrics: scores %s, index %s and %d mates do not match"
                         % (tuple(s.shape), tuple(idx.shape), m.numel()))
    if not s.dtype.is_floating_point:
        raise ValueError("identification_metrics: scores are %s" % s.dtype)
    P, k = s.shape
    ranks = [int(r) for r in ranks]
    fpirs = [float(f) for f in fpirs]
    if ranks and (min(ranks) < 1 or max(ranks) > k):
        raise ValueError("identification_metrics: ranks %s outside 1..k=%d" % (ranks, k))
    if any(not 0.0 <= f < 1.0 for f in fpirs):
        raise ValueError("identification_metrics: FPIR targets %s outside [0, 1)" % (fpirs,))
    mated = m >= 0
    hit = idx.to(torch.int64) == m[:, None]                       # a list names a gallery row at most once
    pos = torch.where(hit.any(1), hit.to(torch.int32).argmax(1), torch.full_like(m, k))
    mate_rank = torch.where(mated, pos, torch.full_like(m, -1)).to(torch.int32)
    n_mated = int(mated.sum())
    n_non = P - n_mated
    if n_mated == 0:
        raise ValueError("identification_metrics: no mated probe")
    if fpirs and n_non == 0:
        raise ValueError("identification_metrics: FPIR targets need non-mated probes")
    mr = mate_rank[mated]
    cmc_count = np.array([int((mr < r).sum()) for r in ranks], np.int64)
    top1 = s[:, 0].to(torch.float64)
    thr, tp, fa = [], [], []
    if fpirs:
        u = torch.sort(top1[~mated], descending=True).values
        first = top1[mated][mr == 0]
        for f in fpirs:
            tau = u[int(math.floor(f * n_non))]
            thr.append(float(tau))
            fa.append(int((u > tau).sum()))
            tp.append(int((first > tau).sum()))
    tp, fa = np.array(tp, np.int64), np.array(fa, np.int64)
    return {"mate_rank": mate_rank, "n_mated": n_mated, "n_nonmated": n_non, "ranks": tuple(ranks),
            "fpirs": tuple(fpirs), "cmc": cmc_count / n_mated, "cmc_count": cmc_count,
            "thresholds": np.array(thr, np.float64), "tpir": tp / n_mated, "tpir_count": tp,
            "fpir_achieved": fa / max(n_non, 1)}


@torch.no_grad()
def identify(probe, probe_subjects, gallery, gallery_subjects, ranks=(1, 5, 10), fpirs=(0.01, 0.1), k=None,
             splits=None, dtype=torch.float64):
    """search_topk, mate_rows and identification_metrics in a row.  probe [P][E] with one subject id per row, gallery
    [G][E] with one row per subject.  k defaults to max(ranks).  Returns the metrics dict plus `topk_scores`,
    `topk_index` (device) and `mate` (numpy)."""
    ranks = tuple(int(r) for r in ranks)
    if k is None:
        if not ranks:
            raise ValueError("identify: needs ranks or k")
        k = max(ranks)
    mate = mate_rows(probe_subjects, gallery_subjects)
    n_p = probe.shape[0] if hasattr(probe, "shape") else len(probe)
    n_g = gallery.shape[0] if hasattr(gallery, "shape") else len(gallery)
    if mate.size != n_p or np.asarray(_ids(gallery_subjects, "gallery_subjects")).size != n_g:
        raise ValueError("identify: one subject id per probe row and per gallery row")
    sc, idx = search_topk(probe, gallery, k, splits, dtype)
    out = identification_metrics(sc, idx, mate, ranks, fpirs)
    out.update(topk_scores=sc, topk_index=idx, mate=mate)
    return out


@torch.no_grad()
def identify_templates(template_feats, unique_templates, gallery_templates, gallery_subjects, probe_templates,
                       probe_subjects, ranks=(1, 5, 10), fpirs=(0.01, 0.1), k=None, splits=None, dtype=torch.float64):
    """identify on rows of pooled template features (ijb.template_features' result): gallery_templates /
    probe_templates name the template id of every gallery / probe entry, *_subjects their subject ids; ValueError for a
    template id without images (ijb.template_rows).  IJB-C 1:N has two galleries searched by one probe set: call this
    once per gallery and average the figures; that mean is the caller's."""
    tf = _dev(template_feats)
    if tf.dim() != 2 or tf.shape[0] != len(unique_templates):
        raise ValueError("template_feats %s does not match %d templates" % (tuple(tf.shape), len(unique_templates)))
    g_rows = template_rows(unique_templates, gallery_templates, tf.device).to(torch.int64)
    p_rows = template_rows(unique_templates, probe_templates, tf.device).to(torch.int64)
    return identify(tf[p_rows], probe_subjects, tf[g_rows], gallery_subjects, ranks, fpirs, k, splits, dtype)


@torch.no_grad()
def distractor_ranks(probe, mate, distractors, k=10, splits=None, dtype=torch.float64):
    """The MegaFace list of datasets/benchmarks/get_list.py:138-208: P (probe, mate) feature rows [P][E] each, searched
    against distractors [G][E].  rank[p] = #{top-k distractor scores > <probe_p, mate_p>}, capped at k by construction:
    0 means the mate beats every distractor.  The mate score is a plain row-wise f64 dot product in torch; it may differ
    from the score the kernel would give the same pair in its last bits (another summation order), which matters only
    for a distractor that ties with the mate to that precision.  Returns a dict: `rank` int32 [P] (device), `rank1` =
    mean(rank == 0), `mate_scores` f64 [P], `topk_scores`, `topk_index`."""
    p = _rows(probe, torch.float64, "distractor_ranks: probe")
    m = _rows(mate, torch.float64, "distractor_ranks: mate")
    if m.shape != p.shape:
        raise ValueError("distractor_ranks: probe %s and mate %s differ" % (tuple(p.shape), tuple(m.shape)))
    sc, idx = search_topk(probe if dtype != torch.float64 else p, distractors, k, splits, dtype)
    ms = (p * m.to(p.device)).sum(1)
    rank = (sc.to(torch.float64) > ms[:, None]).sum(1).to(torch.int32)
    return {"rank": rank, "rank1": float((rank == 0).double().mean()), "mate_scores": ms, "topk_scores": sc,
            "topk_index": idx}
