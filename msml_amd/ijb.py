"""Template verification (IJB-B / IJB-C) on the HIP path: eval/qeval_ijbc.py of the reference.

* `segment_layout(templates, medias)`: host side, once per protocol file: the image rows ordered by (template id,
  media id, row) with the media and template offsets the pooling kernel walks, and `unique_templates`.
* `template_features(...)`: flip sum, detector-score weighting (qeval_ijbc.py:484-502), media mean, template sum
  and L2 normalisation (`image2template_feature`, :303-337) in one read of the image features.
* `pair_scores(...)`: cosine of every listed template pair (`verification`, :343-369).
* `roc_table(scores, labels)`: the TPR @ FPR table and the AUC (:565-585) of `roc_curve(label, score)`.
* `evaluate_templates(...)` chains them.
* `align_matrices` / `pack_images` / `align_faces` / `pair_inputs` / `eval_inputs` / `align_and_embed`: the step in
  front of them, `Embedding.get` and `get_image_feature` (:145-187, :242-297): the 5-point similarity estimate on the
  host, then warp, colour swap, block occlusion, mirror and normalisation on the device (csrc/align.hip), from decoded
  images and landmarks to the `[N][2E]` features.

Inputs may be numpy arrays or CUDA tensors; features and scores stay on the device, the small tables come back as
numpy.  Sums are f64 in a fixed order: two runs give the same bits.

Where this differs from the reference on purpose: `verification` maps a pair id that is not a template id to row 0
(or fails with an IndexError beyond the largest id); `pair_scores` raises ValueError for every such id.
"""
import collections

import numpy as np
import torch

from . import packed
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


# ---------------------------------------------------------------------------------------------------------------------
# Step 2 of the script, Embedding.get + the staging of get_image_feature (qeval_ijbc.py:145-187, 257-293): transform
# estimate on the host, warp / colour swap / block occlusion / mirror / normalisation on the device (csrc/align.hip).

def _dst_points():
    """The `src` table of qeval_ijbc.py:90-96 as the script builds it: float32, +8 on x in float32."""
    p = np.array([[30.2946, 51.6963], [65.5318, 51.5014], [48.0252, 71.7366], [33.5493, 92.3655], [62.7299, 92.2041]],
                 dtype=np.float32)
    p[:, 0] += 8.0
    return p.astype(np.float64)


def align_matrices(landmarks, out_size=112):
    """Host side (numpy f64, no GPU): the 2 x 3 matrix tform.params[0:2] of SimilarityTransform.estimate(landmark5,
    src) (qeval_ijbc.py:158-160) of every image, [N][2][3] float64.

    landmarks [N][5][2] or [N][68][2] (one image: [5][2] / [68][2]); 68 points are reduced as :149-155 do, in the
    dtype they come in.  The estimate is skimage's _umeyama with scale, batched: covariance dst_demean.T @ src_demean
    / n, SVD, the det < 0 sign fix, the rank cases, scale = (S . d) / src_demean.var(0).sum().  The destination points
    are those of a 112 x 112 crop; out_size scales them (112 leaves them as they are).  ValueError naming the row for
    non-finite landmarks and for points that all coincide (rank 0, where skimage returns NaN)."""
    lm = np.asarray(landmarks)
    if lm.ndim == 2:
        lm = lm[None]
    if lm.ndim != 3 or lm.shape[1] not in (5, 68) or lm.shape[2] != 2 or lm.shape[0] == 0:
        raise ValueError("landmarks %s are not [N][5][2] or [N][68][2]" % (tuple(lm.shape),))
    if not np.issubdtype(lm.dtype, np.floating):
        lm = lm.astype(np.float64)
    if lm.shape[1] == 68:
        lm = np.stack([(lm[:, 36] + lm[:, 39]) / 2, (lm[:, 42] + lm[:, 45]) / 2, lm[:, 30], lm[:, 48], lm[:, 54]], 1)
    src = lm.astype(np.float64)
    bad = np.flatnonzero(~np.isfinite(src).all((1, 2)))
    if bad.size:
        raise ValueError("landmarks of row %d are not finite" % bad[0])
    dst = _dst_points() * (float(out_size) / 112.0)
    n, num = src.shape[0], src.shape[1]
    src_mean, dst_mean = src.mean(1), dst.mean(0)
    sd, dd = src - src_mean[:, None], dst - dst_mean
    a = np.matmul(dd.T[None], sd) / num                          # [N][2][2]
    u, s, vt = np.linalg.svd(a)
    rank = (s > s.max(1, keepdims=True) * (2 * np.finfo(np.float64).eps)).sum(1)
    bad = np.flatnonzero(rank == 0)
    if bad.size:
        raise ValueError("landmarks of row %d coincide: no similarity transform (rank 0)" % bad[0])
    d = np.ones((n, 2))
    d[np.linalg.det(a) < 0, 1] = -1.0
    # rank 1: U @ V when det(U) det(V) > 0, else the last sign is -1 for the rotation (the scale keeps d)
    dr = d.copy()
    low = rank == 1
    if low.any():
        pos = np.linalg.det(u) * np.linalg.det(vt) > 0
        dr[low & pos] = 1.0
        dr[low & ~pos, 1] = -1.0
    rot = np.matmul(u * dr[:, None, :], vt)
    scale = (s * d).sum(1) / sd.var(1).sum(1)
    m = np.empty((n, 2, 3))
    m[:, :, 2] = dst_mean - scale[:, None] * np.matmul(rot, src_mean[:, :, None])[:, :, 0]
    m[:, :, :2] = rot * scale[:, None, None]
    return m


pack_images = packed.pack_images


def invert_matrices(matrices):
    """[N][2][3] forward maps (src -> dst) -> [N][6] f64 inverse maps, in cv2.warpAffine's order of operations."""
    m = np.array(matrices, dtype=np.float64).reshape(-1, 6)
    if not np.isfinite(m).all():
        raise ValueError("transform %d is not finite" % np.flatnonzero(~np.isfinite(m).all(1))[0])
    det = m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3]
    with np.errstate(divide="ignore"):
        det = np.where(det != 0, 1.0 / det, 0.0)
    a11, a22 = m[:, 4] * det, m[:, 0] * det
    m[:, 0], m[:, 1], m[:, 3], m[:, 4] = a11, m[:, 1] * -det, m[:, 3] * -det, a22
    b1 = -m[:, 0] * m[:, 2] - m[:, 1] * m[:, 5]
    b2 = -m[:, 3] * m[:, 2] - m[:, 4] * m[:, 5]
    m[:, 2], m[:, 5] = b1, b2
    return m


def _out_hw(out_size):
    if isinstance(out_size, (int, np.integer)):
        return int(out_size), int(out_size)
    oh, ow = out_size
    return int(oh), int(ow)


@torch.no_grad()
def align_faces(buf, meta, matrices, out_size=112, bgr=True):
    """cv2.warpAffine(img, M, (s, s), borderValue=0.0) + cvtColor(BGR2RGB) (qeval_ijbc.py:161-164) of every packed
    source in one launch (msml_align_warp) -> uint8 [N][s][s][3] on the device.  buf / meta: pack_images' result (buf
    on the host or already on the device); matrices [N][2][3]: align_matrices' result; out_size: s or (h, w);
    bgr=False leaves the channel order alone.  meta is checked on the host against buf.numel() before anything is
    uploaded (packed.check)."""
    mt = packed.check(buf, meta, "align_faces")
    n = mt.shape[0]
    minv = invert_matrices(matrices)
    if minv.shape[0] != n:
        raise ValueError("align_faces: %d matrices for %d images" % (minv.shape[0], n))
    oh, ow = _out_hw(out_size)
    src = buf if buf.is_cuda else buf.to("cuda", non_blocking=True)
    dst = torch.empty(n, oh, ow, 3, dtype=torch.uint8, device=src.device)
    call("msml_align_warp", src, _dev(mt, None, src.device), _dev(minv, None, src.device), dst, n, oh, ow,
         1 if bgr else 0)
    return dst


@torch.no_grad()
def pair_inputs(faces, desc=None):
    """faces uint8 [N][H][W][3] RGB on the device, desc: data.draw's descriptors (kinds none / block) or None ->
    f32 [2N][3][H][W]: row 2i the normalised face with its block painted black, row 2i + 1 its mirror
    (msml_align_pairs): the batch Embedding.get and forward_db hand to the model (qeval_ijbc.py:181-192)."""
    if not (isinstance(faces, torch.Tensor) and faces.is_cuda and faces.dtype == torch.uint8 and faces.dim() == 4
            and faces.shape[3] == 3 and faces.is_contiguous()):
        raise ValueError("pair_inputs: faces must be a contiguous uint8 [N][H][W][3] tensor on the device")
    n, h, w, _ = faces.shape
    if desc is not None:
        if not (desc.is_cuda and desc.dtype == torch.int32 and tuple(desc.shape) == (n, 64) and desc.is_contiguous()):
            raise ValueError("pair_inputs: desc must be int32 [%d][64] on the device" % n)
        kind = desc[:, 0]
        if bool(((kind != 0) & (kind != 3)).any()):
            raise ValueError("pair_inputs: only block (3) and none (0) descriptors are supported")
    out = torch.empty(2 * n, 3, h, w, dtype=torch.float32, device=faces.device)
    call("msml_align_pairs", faces, desc, out, n, h, w)
    return out


@torch.no_grad()
def eval_inputs(faces, seed=1, offset=0, lo=0, hi=1):
    """RandomBlock(lo, hi) (the script's --lo / --hi, qeval_ijbc.py:166-173) on every aligned face, then pair_inputs.
    lo = hi = None skips the occlusion.  The block's size and place come from the project's counter-based generator
    (data.draw(mode="block"): a function of seed and offset + row, as in the training pipeline), NOT from numpy's
    global RNG as in the reference: the same (seed, offset) gives the same blocks on any batch split, and no run
    reproduces the reference's draws."""
    if lo is None and hi is None:
        return pair_inputs(faces, None)
    from . import data
    if faces.shape[1] != faces.shape[2]:
        raise ValueError("eval_inputs: RandomBlock needs square faces, got %d x %d" % (faces.shape[1], faces.shape[2]))
    desc = data.draw(faces.shape[0], seed, offset, mode="block", lo=int(lo), hi=int(hi), flip=False,
                     size=faces.shape[1], device=faces.device)
    return pair_inputs(faces, desc)


@torch.no_grad()
def align_and_embed(model, images, landmarks, batch=64, lo=0, hi=1, seed=1, out_size=112):
    """get_image_feature (qeval_ijbc.py:242-297) without its per-image loop: images (a list of cv2.imread results) and
    their landmarks ([N][5][2] or [N][68][2]) -> img_feats [N][2E] f32 on the device, embedding | embedding of the
    mirrored face, which evaluate_templates takes as it is.  `batch` images per launch: packed, uploaded, warped,
    occluded + mirrored + normalised, embedded.  Image i draws its block from (seed, i) whatever the batch size (the
    project's counter-based generator, not numpy's global RNG: see eval_inputs)."""
    n = len(images)
    m = align_matrices(landmarks, out_size)
    if m.shape[0] != n:
        raise ValueError("align_and_embed: %d images but %d landmark sets" % (n, m.shape[0]))
    batch = max(1, int(batch))
    out = None
    for i0 in range(0, n, batch):
        i1 = min(n, i0 + batch)
        buf, meta = pack_images(images[i0:i1])
        faces = align_faces(buf, meta, m[i0:i1], out_size)
        f = model(eval_inputs(faces, seed, i0, lo, hi))
        if isinstance(f, (tuple, list)):
            f = f[0]
        f = f.float().reshape(i1 - i0, -1)
        if out is None:
            out = torch.empty(n, f.shape[1], dtype=torch.float32, device=f.device)
        out[i0:i1] = f
    return out
