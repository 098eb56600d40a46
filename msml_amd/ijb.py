"""Template verification (IJB-B / IJB-C) on the HIP path: eval/qeval_ijbc.py of the reference.

* `segment_layout(templates, medias)`: host side, once per protocol file: the image rows ordered by (template id,
  media id, row) with the media and template offsets the pooling kernel walks, and `unique_templates`.
* `template_features(...)`: flip sum, detector-score weighting (qeval_ijbc.py:484-502), media mean, template sum
  and L2 normalisation (`image2template_feature`, :303-337) in one read of the image features.
* `pair_scores(...)`: cosine of every listed template pair (`verification`, :343-369).
* `roc_table(scores, labels)`: the TPR @ FPR table and the AUC (:565-585) of `roc_curve(label, score)`.
* `evaluate_templates(...)` chains them.

Inputs may be numpy arrays or CUDA tensors; features and scores stay on the device, the small tables come back as
numpy.  Sums are f64 in a fixed order: two runs give the same bits.

Where this differs from the reference on purpose: `verification` maps a pair id that is not a template id to row 0
(or fails with an IndexError beyond the largest id); `pair_scores` raises ValueError for every such id.
"""
import collections

import numpy as np
import torch

from ._lib import call, value

FPRS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)

SegmentLayout = collections.namedtuple(
    "SegmentLayout", "order media_start template_media_start unique_templates launch max_rows")


def _ids(a, name):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 1:
        a = a.reshape(-1)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must be integers, got %s" % (name, a.dtype))
    return a.astype(np.int64)


def segment_layout(templates, medias):
    """Host side (numpy, no GPU).  templates / medias: one id per image row, any order, any integers.

    order                  [N] int32   rows sorted by (template id, media id, row): np.unique's ascending order of
                                       both ids, rows of one media in their original order
    media_start            [M+1] int32 positions in `order` where a (template, media) group starts; a media id used
                                       by two templates makes one group in each, as np.where(templates == uqt)
                                       followed by np.unique(face_medias) does
    template_media_start   [T+1] int32 first group of each template
    unique_templates       [T] int64   np.unique(templates): row t of the pooled features
    launch                 [T] int32   templates by falling row count (largest first, ties by ascending row)
    max_rows               int         rows of the largest template
    """
    templates, medias = _ids(templates, "templates"), _ids(medias, "medias")
    n = templates.size
    if n == 0:
        raise ValueError("segment_layout: no images")
    if medias.size != n:
        raise ValueError("segment_layout: %d template ids but %d media ids" % (n, medias.size))
    if n >= 2 ** 31 - 1:
        raise ValueError("segment_layout: %d rows do not fit int32 offsets" % n)
    order = np.lexsort((medias, templates))                     # stable: equal keys keep the row order
    ts, ms = templates[order], medias[order]
    new_t = np.r_[True, ts[1:] != ts[:-1]]
    new_m = new_t | np.r_[True, ms[1:] != ms[:-1]]
    media_start = np.r_[np.flatnonzero(new_m), n]
    t_pos = np.flatnonzero(new_t)
    tms = np.r_[(np.cumsum(new_m) - 1)[t_pos], media_start.size - 1]
    rows = np.diff(np.r_[t_pos, n])
    launch = np.argsort(-rows, kind="stable")
    i32 = np.int32
    return SegmentLayout(order.astype(i32), media_start.astype(i32), tms.astype(i32), ts[t_pos].copy(),
                         launch.astype(i32), int(rows.max()))


def _dev(a, dtype=None, device=None):
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not a.is_cuda:
        a = a.to(device if device is not None else "cuda")
    if dtype is not None and a.dtype != dtype:
        a = a.to(dtype)
    return a.contiguous()


@torch.no_grad()
def template_features(img_feats, templates, medias, faceness=None, flip_sum=True, layout=None, single=False):
    """img_feats [N][2E] f32 (embedding | embedding of the flipped image, the layout forward_db produces): the halves
    are summed with flip_sum=True, the first half alone is used with flip_sum=False (use_flip_test of the reference).
    single=True: img_feats is [N][E], no flip half.  faceness [N] or None (use_detector_score).  layout: a
    segment_layout(templates, medias) to reuse.  Returns (template_feats [T][E] f64 on the device, L2-normalised,
    unique_templates [T] numpy)."""
    lay = layout if layout is not None else segment_layout(templates, medias)
    x = img_feats
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0):
        x = _dev(img_feats, torch.float32)                       # rows of a wider device buffer are read in place
    if x.dim() != 2 or x.shape[0] != lay.order.size:
        raise ValueError("img_feats %s does not hold one row per template id (%d)" % (tuple(x.shape), lay.order.size))
    width = x.shape[1]
    if single:
        if flip_sum:
            raise ValueError("single=True features have no flip half to sum")
        e = width
    else:
        if width % 2:
            raise ValueError("img_feats width %d is not two halves" % width)
        e = width // 2
    if e % 4:
        raise ValueError("embedding size %d is not a multiple of 4" % e)
    face = None
    if faceness is not None:
        face = _dev(faceness, torch.float32, x.device).reshape(-1)
        if face.numel() != x.shape[0]:
            raise ValueError("faceness holds %d scores for %d rows" % (face.numel(), x.shape[0]))
    t = lay.unique_templates.size
    out = torch.empty(t, e, dtype=torch.float64, device=x.device)
    call("msml_template_pool", x, x.shape[0], x.stride(0), e, 1 if flip_sum else 0, face, _dev(lay.order, None, x.device),
         _dev(lay.media_start, None, x.device), _dev(lay.template_media_start, None, x.device),
         _dev(lay.launch, None, x.device), t, out)
    return out, lay.unique_templates


@torch.no_grad()
def template_rows(unique_templates, ids, device="cuda"):
    """Row of every template id (template2id of qeval_ijbc.py:350-352) as int32 on the device; ValueError for an id
    that is not in unique_templates."""
    ut = _dev(_ids(unique_templates, "unique_templates"), None, device)
    if isinstance(ids, torch.Tensor) and ids.is_cuda:
        p = ids.reshape(-1).to(torch.int64)
    else:
        p = _dev(_ids(ids, "pair ids"), None, device)
    if ut.numel() == 0:
        raise ValueError("no templates")
    row = torch.searchsorted(ut, p).clamp_(max=ut.numel() - 1)
    bad = ut[row] != p
    if bool(bad.any()):
        raise ValueError("pair list names template id %d, which has no images" % int(p[bad][0]))
    return row.to(torch.int32)


@torch.no_grad()
def pair_scores(template_feats, unique_templates, p1, p2):
    """score[i] = <template_feats[row(p1[i])], template_feats[row(p2[i])]> -> [P] f64 on the device."""
    tn = _dev(template_feats, torch.float64)
    if tn.dim() != 2 or tn.shape[0] != len(unique_templates):
        raise ValueError("template_feats %s does not match %d templates" % (tuple(tn.shape), len(unique_templates)))
    if tn.shape[1] % 2:
        raise ValueError("embedding size %d is odd" % tn.shape[1])
    r1, r2 = template_rows(unique_templates, p1, tn.device), template_rows(unique_templates, p2, tn.device)
    if r1.numel() != r2.numel() or r1.numel() == 0:
        raise ValueError("pair lists hold %d and %d ids" % (r1.numel(), r2.numel()))
    score = torch.empty(r1.numel(), dtype=torch.float64, device=tn.device)
    call("msml_template_pair_score", tn, tn.shape[0], tn.shape[1], r1, r2, r1.numel(), score)
    return score


@torch.no_grad()
def roc_points(scores, labels, fprs=()):
    """roc_curve(labels, scores) (drop_intermediate=True) on the device.  Returns a dict:
    fps, tps       int32 device tensors: the counts of ALL distinct-score points, descending score
    keep           uint8 device tensor: 1 where roc_curve keeps the point
    n_points       len(fpr) of roc_curve: the kept points plus the origin it prepends
    n_pos, n_neg   label counts
    auc            trapezoid area over the kept points (exact integer area / (n_pos * n_neg))
    nearest        per target FPR the index into fps / tps of the kept point nearest to it, -1 for the origin
                   (ties: the later point of the ascending curve)"""
    s = _dev(scores, torch.float64).reshape(-1)
    y = _dev(labels, None, s.device).reshape(-1)
    n = s.numel()
    if n == 0 or y.numel() != n:
        raise ValueError("roc: %d scores and %d labels" % (n, y.numel()))
    if n >= 2 ** 31 - 1:
        raise ValueError("roc: %d scores do not fit int32 counts" % n)
    if not bool(torch.isfinite(s).all()):
        raise ValueError("roc: scores hold NaN or infinity")
    fprs = [float(f) for f in fprs]
    if len(fprs) > 16:
        raise ValueError("roc: at most 16 target FPRs")
    ss, idx = torch.sort(s, descending=True)
    ys = (y != 0).to(torch.uint8)[idx].contiguous()
    nb = value("msml_roc_blocks", n)
    blk = torch.empty(nb, 2, dtype=torch.int32, device=s.device)
    call("msml_roc_block_counts", ss, ys, n, blk)
    tab = blk.cpu().numpy().astype(np.int64)                     # the small table between the two passes
    n_pos, k = (int(v) for v in tab.sum(0))
    n_neg = n - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("roc: needs both labels (%d positives, %d negatives)" % (n_pos, n_neg))
    off = torch.from_numpy((np.cumsum(tab, 0) - tab).astype(np.int32)).to(s.device)
    tps = torch.empty(k, dtype=torch.int32, device=s.device)
    fps = torch.empty(k, dtype=torch.int32, device=s.device)
    call("msml_roc_points", ss, ys, n, off, tps, fps)
    nt = len(fprs)
    tgt = torch.tensor(fprs, dtype=torch.float64, device=s.device) if nt else None
    keep = torch.empty(k, dtype=torch.uint8, device=s.device)
    part = torch.empty(value("msml_roc_reduce_blocks", k), 2 + 2 * nt, dtype=torch.int64, device=s.device)
    call("msml_roc_reduce", tps, fps, k, tgt, nt, keep, part)
    part = part.cpu().numpy()
    area2 = sum(int(v) for v in part[:, 1].view(np.uint64))
    nearest = []
    for j, f in enumerate(fprs):
        d = np.ascontiguousarray(part[:, 2 + 2 * j]).view(np.float64)
        kk = part[:, 3 + 2 * j]
        dmin = d.min()
        best = int(kk[d == dmin].max())
        nearest.append(-1 if abs(0.0 - f) < dmin else best)      # the origin comes first: it loses every tie
    return {"fps": fps, "tps": tps, "keep": keep, "n_points": int(part[:, 0].sum()) + 1, "n_pos": n_pos,
            "n_neg": n_neg, "auc": area2 / (2 * n_pos * n_neg), "nearest": nearest}


def roc_table(scores, labels, fprs=FPRS):
    """(tprs [len(fprs)] numpy f64, auc): TPR of the roc_curve point nearest to every target FPR, and the AUC."""
    r = roc_points(scores, labels, fprs)
    near = np.asarray(r["nearest"], np.int64)
    tp = r["tps"][torch.from_numpy(np.maximum(near, 0)).to(r["tps"].device)].cpu().numpy().astype(np.float64)
    tp[near < 0] = 0.0
    return tp / r["n_pos"], r["auc"]


def _mean_scores(score_list):
    """score = first; score += each other; score /= count (qeval_ijbc.py:536-548)."""
    total = None
    for s in score_list:
        s = _dev(s, torch.float64).reshape(-1)
        total = s.clone() if total is None else total.add_(s)
    return total / len(score_list)


@torch.no_grad()
def evaluate_templates(img_feats, templates, medias, p1, p2, label, faceness=None, flip_sum=True, fprs=FPRS,
                       scores=None, single=False):
    """The chain of qeval_ijbc.py: pooled template features, pair scores, TPR @ FPR table and AUC.  img_feats may be a
    list of feature arrays (the reference's 10 repeats under random occlusion): their scores are averaged.  scores: a
    score array or a list of them computed earlier; pooling and scoring are skipped then.  Returns a dict with
    `scores` (device), `tprs`, `auc`, `fprs`, and `template_feats` / `unique_templates` of the last pooling."""
    out = {"fprs": tuple(fprs), "template_feats": None, "unique_templates": None}
    if scores is None:
        feats = img_feats if isinstance(img_feats, (list, tuple)) else [img_feats]
        lay = segment_layout(templates, medias)
        scores = []
        for f in feats:
            tf, ut = template_features(f, templates, medias, faceness, flip_sum, lay, single)
            scores.append(pair_scores(tf, ut, p1, p2))
            out["template_feats"], out["unique_templates"] = tf, ut
    elif not isinstance(scores, (list, tuple)):
        scores = [scores]
    if not scores:
        raise ValueError("evaluate_templates: no scores")
    out["scores"] = _mean_scores(scores)
    out["tprs"], out["auc"] = roc_table(out["scores"], label, fprs)
    return out
