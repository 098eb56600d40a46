"""Verification on the HIP path: the embedding protocol and the pair metrics of the reference
(eval/verification.py:239-306 `test`, :54-199 `calculate_roc` / `calculate_val` / `evaluate`;
eval/qeval_mxnet.py:326-390 uses the same orig + flip sum).

* `extract_embeddings(model, x)`: embeddings of the batch and of its horizontal flip, summed (the
  reference normalises after the sum, verification.py:299-301).
* `evaluate(embeddings, issame)`: 10-fold accuracy over the 0..4 / 0.01 threshold grid and TAR @ FAR 1e-3
  over the 0..4 / 0.001 grid.  The reference makes nrof_thresholds x nrof_folds boolean passes over all
  pairs in numpy; here ONE kernel computes the f64 pair distances and ONE builds a [fold][same][threshold]
  histogram (integer atomics, deterministic), from which every confusion-matrix entry of every threshold
  and fold is a prefix sum -- the remaining arithmetic is on a table of a few thousand integers.
* `eval_pairs` / `extract_sum` / `occlusion_sweep`: test.py itself (eval/qeval_mxnet.py:486-600) -- the model inputs
  of one extraction in one launch (msml_eval_pairs), the orig + mirror feature sum, and the loop over occlusion
  levels and repeats that prints the paper's table.
* `eval_pair_masks` / `segmentation_sweep`: the same loop for the segmentation branch -- the ground-truth masks of
  eval_pairs' rows and the pixel / blob scores of `final_seg` against them (msml_amd/segeval.py).
"""
import numpy as np
import torch

from ._lib import call

def slinear_first_order(x, y, xq):
    """interp1d(x, y, kind='slinear')(xq) as scipy 1.5.4 (the reference's pin, requirements.txt:100)
    evaluates it when x holds duplicates -- far_train is a step function, so it always does: interp1d
    sorts x with a stable argsort and builds the degree-1 B-spline on the knots [x0, x..., xn] without
    the strictly-increasing check newer scipy applies (>= 1.10 raises 'Expect x to not have
    duplicates').  Empty knot intervals are skipped, so the value at xq interpolates between the LAST
    sample of the run x[j] <= xq and the first sample of the next run."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    order = np.argsort(x, kind="mergesort")
    x, y = x[order], y[order]
    j = int(np.searchsorted(x, xq, side="right")) - 1
    j = min(max(j, 0), len(x) - 2)
    while j > 0 and x[j + 1] == x[j]:
        j -= 1
    if x[j + 1] == x[j]:
        return float(y[j])
    return float(y[j] + (y[j + 1] - y[j]) * (xq - x[j]) / (x[j + 1] - x[j]))


@torch.no_grad()
def extract_embeddings(model, x, normalize=False):
    """(B, E) f64: model(x) + model(flip(x)) summed in float64 like the reference, which stores both passes in
    float64 arrays (verification.py:283,299); normalize=True returns the f32 L2-normalised rows instead (:300, on
    device) for callers that only need cosines."""
    f1 = model(x)[0]
    f2 = model(x.flip(3))[0]
    out = f1.double() + f2.double()
    if normalize:
        from . import functional as Fh
        out = Fh.normalize(out.float())
    return out


def pair_saliency(model, a, b, flip=False):
    """Which pixels drive a match: (cos, da, db) for the image batches a, b (B, C, H, W) -- cos (B,) the cosine of the
    embeddings of a[i] and b[i] (flip=True: of the orig + mirror sums, as extract_embeddings), da / db its gradient for
    each image batch (the stems' msml_stem_bwd_data in bf16 mode).  Runs the model in eval mode (BatchNorm statistics
    untouched) and puts every module's mode back; no host synchronisation.  torch.autograd.grad on the images: a
    parameter's .grad is left alone unless it is a FlatSGD arena view, which the backward kernels add into directly --
    freeze the parameters (requires_grad_(False)) for a map without that and at less cost."""
    from . import functional as Fh
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.enable_grad():
            xs = [t.detach().requires_grad_(True) for t in (a, b)]
            emb = [model(x)[0] + model(x.flip(3))[0] if flip else model(x)[0] for x in xs]
            cos = (Fh.normalize(emb[0].float()) * Fh.normalize(emb[1].float())).sum(1)
            da, db = torch.autograd.grad(cos.sum(), xs)
    finally:
        for m, mode in modes:
            m.training = mode
    return cos.detach(), da, db


@torch.no_grad()
def pair_cosine(emb):
    """Cosine of every pair (rows 2i, 2i+1) of summed embeddings: 1 - dist / 2 with the f64 distance of
    the normalised rows."""
    return 1.0 - pair_sqdist(emb) / 2.0


@torch.no_grad()
def pair_sqdist(emb):
    """emb: (2 * n_pairs, E) f32 or f64 (extract_embeddings) on the GPU, NOT normalised -> (n_pairs,) f64 squared
    distances of the L2-normalised rows (sklearn.preprocessing.normalize + np.sum(np.square(diff), 1))."""
    f64 = emb.dtype == torch.float64
    emb = emb.contiguous() if f64 else emb.float().contiguous()
    n2, e = emb.shape
    assert n2 % 2 == 0 and emb.is_cuda
    dist = torch.empty(n2 // 2, dtype=torch.float64, device=emb.device)
    call("msml_pair_sqdist_f64" if f64 else "msml_pair_sqdist", emb, n2 // 2, e, dist)
    return dist


def _fold_hist(dist, issame, thresholds, nfolds):
    n = dist.numel()
    thr = torch.as_tensor(np.asarray(thresholds, np.float64), device=dist.device)
    same = torch.as_tensor(np.asarray(issame).astype(np.uint8), device=dist.device)
    hist = torch.empty(nfolds, 2, thr.numel() + 1, dtype=torch.int32, device=dist.device)
    call("msml_pair_hist", dist, same, n, thr, thr.numel(), nfolds, hist)
    return hist.cpu().numpy().astype(np.int64)


def _counts(hist):
    """accept[f][s][k] = pairs of test fold f with issame == s and dist < thr[k]; tot[f][s]."""
    acc = np.cumsum(hist, axis=2)[:, :, :-1]
    tot = hist.sum(axis=2)
    return acc, tot


def evaluate(emb, issame, nrof_folds=10, far_target=1e-3):
    """emb: (2 * n_pairs, E) summed (orig + flip) embeddings on the GPU.  Returns the reference's
    `evaluate` tuple (tpr, fpr, accuracy, val, val_std, far) -- verification.py:181-199."""
    issame = np.asarray(issame).astype(bool)
    dist = pair_sqdist(emb)
    n = dist.numel()
    assert len(issame) == n
    # ---- calculate_roc (:54-107): thresholds 0..4 step 0.01 ----
    thr = np.arange(0, 4, 0.01)
    acc, tot = _counts(_fold_hist(dist, issame, thr, nrof_folds))          # test-fold counts
    tp, fp = acc[:, 1], acc[:, 0]                                          # [fold][thr]
    n_same, n_diff = tot[:, 1:2], tot[:, 0:1]
    all_tp, all_fp = tp.sum(0, keepdims=True), fp.sum(0, keepdims=True)
    tr_tp, tr_fp = all_tp - tp, all_fp - fp                                # train = all folds but f
    tr_same, tr_diff = n_same.sum() - n_same, n_diff.sum() - n_diff
    acc_train = (tr_tp + (tr_diff - tr_fp)) / (tr_same + tr_diff)
    best = np.argmax(acc_train, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        tprs = np.where(n_same > 0, tp / np.maximum(n_same, 1), 0.0)
        fprs = np.where(n_diff > 0, fp / np.maximum(n_diff, 1), 0.0)
    size = (n_same + n_diff)[:, 0]
    f = np.arange(nrof_folds)
    accuracy = (tp[f, best] + (n_diff[:, 0] - fp[f, best])) / size
    tpr, fpr = tprs.mean(0), fprs.mean(0)
    # ---- calculate_val (:125-163): thresholds 0..4 step 0.001, FAR target ----
    thr2 = np.arange(0, 4, 0.001)
    acc2, tot2 = _counts(_fold_hist(dist, issame, thr2, nrof_folds))
    tp2, fp2 = acc2[:, 1], acc2[:, 0]
    s2, d2 = tot2[:, 1:2], tot2[:, 0:1]
    far_train = (fp2.sum(0, keepdims=True) - fp2) / (d2.sum() - d2)
    val = np.zeros(nrof_folds)
    far = np.zeros(nrof_folds)
    d_host = None
    for k in range(nrof_folds):
        if np.max(far_train[k]) >= far_target:
            t = slinear_first_order(far_train[k], thr2, far_target)
        else:
            t = 0.0
        # the interpolated threshold is not on the grid: count the test fold directly (a few hundred pairs)
        if d_host is None:
            d_host = dist.cpu().numpy()
            base, rem = n // nrof_folds, n % nrof_folds
            starts = np.cumsum([0] + [base + (1 if i < rem else 0) for i in range(nrof_folds)])
        sl = slice(starts[k], starts[k + 1])
        pred = np.less(d_host[sl], t)
        val[k] = float(np.sum(pred & issame[sl])) / float(np.sum(issame[sl]))
        far[k] = float(np.sum(pred & ~issame[sl])) / float(np.sum(~issame[sl]))
    return tpr, fpr, accuracy, float(np.mean(val)), float(np.std(val)), float(np.mean(far))


@torch.no_grad()
def pair_cosdist(emb):
    """emb: (2 * n_pairs, E) f32 or f64 on the GPU, NOT normalised -> (n_pairs,) f64 cosine DISTANCES of rows 2i,
    2i + 1: sklearn.preprocessing.normalize then scipy's cdist(..., metric='cosine') (qeval_mxnet.py:419,426-430)."""
    f64 = emb.dtype == torch.float64
    emb = emb.contiguous() if f64 else emb.float().contiguous()
    n2, e = emb.shape
    assert n2 % 2 == 0 and emb.is_cuda
    dist = torch.empty(n2 // 2, dtype=torch.float64, device=emb.device)
    call("msml_pair_cosdist_f64" if f64 else "msml_pair_cosdist", emb, n2 // 2, e, dist)
    return dist


def _rank(sorted_asc, queries, strict):
    out = torch.empty(queries.numel(), dtype=torch.int32, device=queries.device)
    call("msml_rank_count", sorted_asc, sorted_asc.numel(), queries, queries.numel(), 1 if strict else 0, out)
    return out.cpu().numpy().astype(np.int64)


@torch.no_grad()
def roc_accuracy_tarfar(emb, issame):
    """`Verification.start_verification` of the reference (eval/qeval_mxnet.py:422-483), which test.py prints for
    every occlusion level: returns (acc, tarfar[5]).

    emb: (2 * n_pairs, E) embeddings on the GPU (rows 2i, 2i + 1 form pair i), issame: n_pairs booleans.  The
    reference's own conventions are kept:
    * its label is 0 for a SAME pair and 1 for a different one (qeval_mxnet.py:550-551), and roc_curve runs on the
      cosine DISTANCE with label 1 as the positive class; acc = tpr[argmin |tpr - (1 - fpr)|] over the points
      roc_curve keeps, the first minimum;
    * neg_cnt = pos_cnt = n_pairs // 2 whatever the real counts are, and the loops index the first n_pairs // 2
      entries of each list, so the reference raises unless both lists are at least that long.  Precondition here:
      exactly as many same as different pairs (n_pairs even); ValueError otherwise;
    * tarfar[k] for FAR <= 1e-1 .. 1e-4: thresholds are the different-pair distances T with
      #(different < T) / neg_cnt <= FAR (strict <), the value is the largest #(same <= T) / pos_cnt (<=);
      the fifth entry (1e-5) stays 0.
    The two O(n^2) Python loops are two rank queries on the sorted distances (msml_rank_count)."""
    from . import ijb
    issame = np.asarray(issame).astype(bool).reshape(-1)
    dist = pair_cosdist(emb)
    n = dist.numel()
    if len(issame) != n:
        raise ValueError("roc_accuracy_tarfar: %d pairs but %d labels" % (n, len(issame)))
    cnt = n // 2
    if n % 2 or int(issame.sum()) != cnt:
        raise ValueError("roc_accuracy_tarfar: the reference needs as many same as different pairs "
                         "(%d same, %d different)" % (int(issame.sum()), n - int(issame.sum())))
    label = (~issame).astype(np.uint8)                                    # 0: same
    r = ijb.roc_points(dist, label)
    keep = r["keep"].bool()
    fpr = np.r_[0, r["fps"][keep].cpu().numpy()] / r["n_neg"]
    tpr = np.r_[0, r["tps"][keep].cpu().numpy()] / r["n_pos"]
    acc = float(tpr[np.argmin(np.abs(tpr - (1 - fpr)))])
    lab = torch.from_numpy(label).to(dist.device)
    pos_sorted = torch.sort(dist[lab == 0])[0]
    neg_sorted = torch.sort(dist[lab == 1])[0]
    far = _rank(neg_sorted, neg_sorted, True) / cnt                       # ascending with the threshold
    tarfar = np.zeros(5)
    thr_idx = [int(np.flatnonzero(far <= fv)[-1]) for fv in (1e-1, 1e-2, 1e-3, 1e-4)]   # far[0] == 0 always qualifies
    thr = neg_sorted[torch.tensor(thr_idx, device=dist.device)].contiguous()
    tarfar[:4] = _rank(pos_sorted, thr, False) / cnt
    return acc, tarfar


# ---------------------------------------------------------------------------------------------- test.py
FILLS = {"black": 0, "white": 1, "gauss": 2}        # --fill_type (rand_occ.py:25-72)
PROTOCOLS = {"BB": 0, "NB": 1}                      # _load_one_input's protocol (qeval_mxnet.py:184-187)
LEVELS = tuple((lo, lo + 1) for lo in range(0, 100, 10))      # lo_list / hi_list of qeval_mxnet.py:528-529


def pairs_file_order(files_by_identity):
    """The flat order read_pairs_txt indexes: identities sorted, the files of each sorted (qeval_folder.py:43-49 sorts
    the files; the identity order is this function's): [(identity, file)]."""
    return [(ident, f) for ident in sorted(files_by_identity) for f in sorted(files_by_identity[ident])]


def read_pairs_txt(lines, files_by_identity):
    """The pair list of eval/qeval_folder.py:52-73 (MFR2 / RMFRD pairs.txt) without its file I/O.  lines: the lines of the
    file; files_by_identity: {identity: [file names]}.  A line of 3 words `name i j` is a SAME pair of one identity, a
    line of 4 words `name1 i name2 j` a DIFFERENT pair; i, j count from 1 into the SORTED file list of the identity.
    Returns (pairs int64 [P][2], rows of pairs_file_order(files_by_identity); issame bool [P]).  ValueError naming the
    line for another word count, an unknown identity or an index outside the identity's list."""
    first, n = {}, 0
    for ident in sorted(files_by_identity):
        first[ident] = (n, len(files_by_identity[ident]))
        n += len(files_by_identity[ident])
    pairs, issame = [], []
    for k, line in enumerate(lines):
        words = line.strip().split(" ")
        if len(words) == 3:
            names, idx = (words[0], words[0]), (words[1], words[2])
        elif len(words) == 4:
            names, idx = (words[0], words[2]), (words[1], words[3])
        else:
            raise ValueError("read_pairs_txt: line %d has %d words, not 3 or 4" % (k, len(words)))
        row = []
        for name, i in zip(names, idx):
            if name not in first:
                raise ValueError("read_pairs_txt: line %d names the unknown identity %r" % (k, name))
            try:
                i = int(i)
            except ValueError:
                raise ValueError("read_pairs_txt: line %d: %r is not an index" % (k, i)) from None
            if not 1 <= i <= first[name][1]:
                raise ValueError("read_pairs_txt: line %d: index %d outside 1..%d of %r" % (k, i, first[name][1], name))
            row.append(first[name][0] + i - 1)
        pairs.append(row)
        issame.append(len(words) == 3)
    return np.array(pairs, np.int64).reshape(-1, 2), np.array(issame, bool)


def list_folder(root):
    """The directory walk of eval/qeval_folder.py:42-47: {identity: [file names, sorted]} for every sub-directory of
    root (the identity) and every regular file in it.  An identity without files keeps its empty list."""
    import os
    out = {}
    for ident in sorted(os.listdir(root)):
        sub = os.path.join(root, ident)
        if os.path.isdir(sub):
            out[ident] = sorted(f for f in os.listdir(sub) if os.path.isfile(os.path.join(sub, f)))
    return out


def load_folder(root, device="cuda", progressive=False):
    """The file I/O read_pairs_txt leaves out (qeval_folder.py:42-49, Image.open(...).convert('RGB') of every file of
    every identity): -> (files_by_identity, buf, meta), the images decoded on the device (imageio.decode_images: JPEG
    and PNG files, mixed freely) in pairs_file_order -- row k of meta is the image read_pairs_txt's index k names.
    ValueError naming the file for one that cannot be decoded.  progressive=True: progressive JPEG files decode too."""
    import os
    from . import imageio
    files = list_folder(root)
    order = pairs_file_order(files)
    if not order:
        raise ValueError("load_folder: no files under %r" % (root,))
    blobs = []
    for ident, f in order:
        with open(os.path.join(root, ident, f), "rb") as fh:
            blobs.append(fh.read())
    try:
        buf, meta = imageio.decode_images(blobs, order="rgb", strict=True, device=device, progressive=progressive)
    except imageio.DecodeError as e:
        raise ValueError("load_folder: %s: %s" % (os.path.join(*order[e.index]), e)) from None
    return files, buf, meta


def save_folder(root, names, images, order="rgb", **options):
    """The writing twin of load_folder, the layout eval/align_dataset.py:52-75 produces: image k goes to
    root/<identity>/<file> for names[k] = (identity, file) or "identity/file", its format taken from the file's suffix as
    PIL.Image.save takes it (imageio.save_images: .png files are PNG, .jpg / .jpeg files JPEG with `options` = quality,
    sampling, restart, filter).  images: uint8 [N, H, W, 3] on the device or the packed (buf, meta).  -> the paths."""
    import os
    from . import imageio
    pairs = [tuple(n.split("/", 1)) if isinstance(n, str) else tuple(n) for n in names]
    if any(len(p) != 2 or not p[0] or not p[1] or "/" in p[1] or os.sep in p[1] for p in pairs):
        raise ValueError("save_folder: names are (identity, file) pairs or 'identity/file' strings")
    for ident in sorted({p[0] for p in pairs}):
        os.makedirs(os.path.join(root, ident), exist_ok=True)
    return imageio.save_images(images, [os.path.join(root, i, f) for i, f in pairs], order, **options)


def _no_block(lo, hi):
    return (lo is None and hi is None) or (lo == 0 and hi == 1)


@torch.no_grad()
def eval_pairs(src, seed=1, index0=0, lo=0, hi=1, fill="black", protocol="BB", out_size=None, gray=False,
               use_norm=True):
    """The 2N model inputs of N decoded faces as test.py builds them (_load_one_input, qeval_mxnet.py:173-189, and the
    normalisation of :319-324), in one launch (msml_eval_pairs).  src: uint8 [N][H][W][3] RGB on the device, one size
    per call -> f32 [2N][1 or 3][oh][ow]: row 2i is image i, row 2i + 1 its mirrored copy, each: mirror, CenterCrop
    to out_size (None: the source size, an int, or (h, w) -- the reference's cfg.out_size is (w, h)) with torchvision's
    zero padding and half-to-even origin, Grayscale when `gray`, RandomBlock(lo, hi, fill), ToTensor, and
    sub_(0.5).div_(0.5) when `use_norm`.  protocol "NB" occludes only images whose global index index0 + i is even.
    lo = hi = None, or (0, 1), gives no block.

    Deliberate difference from the reference, as in ijb.eval_inputs: the block's size and place come from the
    project's counter-based generator (data.draw(mode="block", size=ow)), the row of image g = index0 + i with mirror
    bit f at counter 2 g + f -- the mirrored copy draws a block of its own, as test.py's second pass does -- and the
    gauss fill's normals from the same generator keyed by (seed, 2 g + f, block row, block column, channel), NOT from
    numpy's global RNG: a batch split does not change the result, and no run reproduces test.py's draws."""
    if fill not in FILLS:
        raise ValueError("eval_pairs: fill %r is not one of %s" % (fill, sorted(FILLS)))
    if protocol not in PROTOCOLS:
        raise ValueError("eval_pairs: protocol %r is not one of %s" % (protocol, sorted(PROTOCOLS)))
    if protocol == "NB" and gray:
        raise ValueError("eval_pairs: the NB protocol has no gray form (the reference puts a 3-channel tensor into "
                         "the 1-channel batch there and raises)")
    if (lo is None) != (hi is None):
        raise ValueError("eval_pairs: lo and hi are both None or both integers")
    if not _no_block(lo, hi) and not 0 <= int(lo) < int(hi) <= 101:
        raise ValueError("eval_pairs: block range [%r, %r) outside 0..101" % (lo, hi))
    if int(index0) < 0:
        raise ValueError("eval_pairs: index0 = %r" % (index0,))
    if not (isinstance(src, torch.Tensor) and src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3
            and src.shape[0] >= 1):
        raise ValueError("eval_pairs: src must be a uint8 [N][H][W][3] tensor")
    if not src.is_contiguous():
        raise ValueError("eval_pairs: src must be contiguous")
    from . import data
    n, h, w, _ = src.shape
    oh, ow = data._out_hw(out_size, h, w)
    if ow % 4 or not (4 <= h <= 256 and 4 <= w <= 256 and 4 <= oh <= 256 and 4 <= ow <= 256):
        raise ValueError("eval_pairs: source %d x %d -> output %d x %d: sizes 4..256, output width a multiple of 4"
                         % (h, w, oh, ow))
    if not src.is_cuda:
        raise ValueError("eval_pairs: src must be on the device")
    desc = None
    if not _no_block(lo, hi):
        desc = data.draw(2 * n, seed, 2 * int(index0), mode="block", lo=int(lo), hi=int(hi), flip=False, size=ow,
                         device=src.device)
    out = torch.empty(2 * n, 1 if gray else 3, oh, ow, dtype=torch.float32, device=src.device)
    call("msml_eval_pairs", src, n, h, w, desc, out, oh, ow, int(bool(gray)), int(bool(use_norm)), FILLS[fill],
         PROTOCOLS[protocol], int(seed), int(index0))
    return out


@torch.no_grad()
def extract_sum(model, src, batch=256, index0=0, **eval_pairs_kwargs):
    """start_extract (qeval_mxnet.py:285-397) without its per-image loops: [N][E] f32 on the device, embedding of
    eval_pairs' row 2i + embedding of row 2i + 1 (features_flip + features, :390).  `batch` images (2 * batch model
    rows) per step; a model that returns a tuple gives its first entry (:333).  Nothing here waits for the device."""
    n = src.shape[0]
    batch = max(1, int(batch))
    out = None
    for i0 in range(0, n, batch):
        i1 = min(n, i0 + batch)
        f = model(eval_pairs(src[i0:i1], index0=int(index0) + i0, **eval_pairs_kwargs))
        if isinstance(f, (tuple, list)):
            f = f[0]
        f = f.float().reshape(2 * (i1 - i0), -1)
        if out is None:
            out = torch.empty(n, f.shape[1], dtype=torch.float32, device=f.device)
        torch.add(f[0::2], f[1::2], out=out[i0:i1])
    return out


def sweep_seed(seed, level, repeat):
    """The generator seed of repeat `repeat` of level number `level` (its position in `levels`) of a sweep started with
    `seed`: (seed + 0x9E3779B97F4A7C15 * (1024 * level + repeat + 1)) mod 2^63 -- a function of the three alone, so a
    level's draws do not depend on which other levels, or how many repeats, the sweep runs."""
    return (int(seed) + 0x9E3779B97F4A7C15 * (1024 * int(level) + int(repeat) + 1)) % (1 << 63)


def occlusion_sweep(model, src, issame, levels=LEVELS, repeats=10, seed=1, batch=256, fill="black", protocol="BB",
                    out_size=None, gray=False, use_norm=True, nrof_folds=10):
    """The loop of test.py (qeval_mxnet.py:539-600) over block-occlusion levels: per level `repeats` extractions with
    fresh blocks (one for the levels (0, 1) and (100, 101), :556), each through `evaluate` (mean of the 10-fold
    accuracies, :566-569) and `roc_accuracy_tarfar` (:571-573), averaged over the repeats in f64 in the reference's
    order of additions (:569, :573-576).  src: uint8 [2 * n_pairs][H][W][3] on the device (load_bin's images in order),
    issame: n_pairs booleans.  Returns {"levels", "avg_acc" [L], "tarfar" [L][5]} -- the three rows test.py prints --
    and the per-repeat values "acc" (L lists), "roc_acc" (L lists), "tarfar_runs" (L arrays [repeats][5]).

    Repeat r of level number k draws with sweep_seed(seed, k, r).  As in eval_pairs the draws come from the project's
    counter-based generator, not numpy's global RNG (np.random.seed(1), :499): no run reproduces test.py's blocks."""
    levels = [(int(lo), int(hi)) for lo, hi in levels]
    res = {"levels": levels, "avg_acc": [], "tarfar": np.zeros((len(levels), 5)), "acc": [], "roc_acc": [],
           "tarfar_runs": []}
    for k, (lo, hi) in enumerate(levels):
        reps = 1 if (lo, hi) in ((0, 1), (100, 101)) else int(repeats)
        avg_acc, accs, rocs, runs = 0.0, [], [], []
        for r in range(reps):
            emb = extract_sum(model, src, batch=batch, seed=sweep_seed(seed, k, r), lo=lo, hi=hi, fill=fill,
                              protocol=protocol, out_size=out_size, gray=gray, use_norm=use_norm)
            accuracy = evaluate(emb, issame, nrof_folds)[2]
            acc2 = float(np.mean(accuracy))
            roc_acc, tarfar = roc_accuracy_tarfar(emb, issame)
            avg_acc += acc2
            res["tarfar"][k] += tarfar
            accs.append(acc2)
            rocs.append(roc_acc)
            runs.append(tarfar)
        res["avg_acc"].append(avg_acc / reps)
        res["tarfar"][k] /= reps
        res["acc"].append(accs)
        res["roc_acc"].append(rocs)
        res["tarfar_runs"].append(np.stack(runs))
    return res


@torch.no_grad()
def load_bin(path, image_size, device="cuda"):
    """eval/verification.py:202-236: read a verification `.bin` (a pickle of (JPEG byte strings, issame)) and decode it
    on the device (jpeg.decode_batch, bit-exact with mx.image.imdecode) -> ([data, flipped], issame): two f32
    [2P, 3, H, W] tensors on the device holding the pixel values 0..255 as the reference does, the second mirrored
    along the width.  image_size: (H, W).  A decoded width other than image_size[0] raises NotImplementedError: the
    reference then calls mx.image.resize_short, a cv2 resize that is not restated here."""
    import pickle
    from . import jpeg
    with open(path, "rb") as f:
        try:
            bins, issame = pickle.load(f)
        except UnicodeDecodeError:
            f.seek(0)
            bins, issame = pickle.load(f, encoding="bytes")
    n = len(issame) * 2
    batch = jpeg.pack_jpegs([bytes(b) for b in bins[:n]])
    for i, d in enumerate(batch.descriptors):
        if d.status == 0 and d.width != image_size[0]:
            raise NotImplementedError("load_bin: image %d is %d pixels wide, not %d: the reference resizes it with "
                                      "mx.image.resize_short (cv2), which is not restated" % (i, d.width, image_size[0]))
    faces = jpeg.decode_batch(batch, size=(int(image_size[0]), int(image_size[1])), order="rgb", strict=True,
                              device=device)
    data = faces.permute(0, 3, 1, 2).float().contiguous()
    return [data, data.flip(3).contiguous()], issame


# ---------------------------------------------------------------------------------------------- the mask branch
@torch.no_grad()
def eval_pair_masks(n, h, w, seed=1, index0=0, lo=0, hi=1, protocol="BB", out_size=None, device="cuda"):
    """The ground-truth masks of the 2n rows eval_pairs builds from n source images of h x w with the same arguments:
    uint8 [2n][oh][ow] on the device, 0 inside the row's block and 1 elsewhere (the `msk` convention of data.augment).
    The same data.draw(2n, seed, 2 * index0, mode="block", ..., size=ow) descriptors and the same rectangle words (kind,
    x0, y0, w, h; cropped at the border) as msml_eval_pairs reads, the same NB rule (images with an odd global index
    index0 + i stay clean) and the same refusals.  lo = hi = None, or (0, 1), gives all ones.  A few torch operations on
    the descriptors, no synchronisation."""
    if protocol not in PROTOCOLS:
        raise ValueError("eval_pair_masks: protocol %r is not one of %s" % (protocol, sorted(PROTOCOLS)))
    if (lo is None) != (hi is None):
        raise ValueError("eval_pair_masks: lo and hi are both None or both integers")
    if not _no_block(lo, hi) and not 0 <= int(lo) < int(hi) <= 101:
        raise ValueError("eval_pair_masks: block range [%r, %r) outside 0..101" % (lo, hi))
    if int(index0) < 0:
        raise ValueError("eval_pair_masks: index0 = %r" % (index0,))
    if int(n) < 1:
        raise ValueError("eval_pair_masks: n = %r" % (n,))
    from . import data
    n, h, w = int(n), int(h), int(w)
    oh, ow = data._out_hw(out_size, h, w)
    if ow % 4 or not (4 <= h <= 256 and 4 <= w <= 256 and 4 <= oh <= 256 and 4 <= ow <= 256):
        raise ValueError("eval_pair_masks: source %d x %d -> output %d x %d: sizes 4..256, output width a multiple of 4"
                         % (h, w, oh, ow))
    if _no_block(lo, hi):
        return torch.ones(2 * n, oh, ow, dtype=torch.uint8, device=device)
    desc = data.draw(2 * n, seed, 2 * int(index0), mode="block", lo=int(lo), hi=int(hi), flip=False, size=ow,
                     device=device)
    kind, bx, by, bw, bh = (desc[:, k].view(-1, 1, 1) for k in range(5))
    ys = torch.arange(oh, dtype=torch.int32, device=desc.device).view(1, oh, 1)
    xs = torch.arange(ow, dtype=torch.int32, device=desc.device).view(1, 1, ow)
    inside = (kind == 3) & (ys >= by) & (ys < by + bh) & (xs >= bx) & (xs < bx + bw)
    if protocol == "NB":
        g = int(index0) + torch.arange(2 * n, device=desc.device) // 2
        inside &= (g % 2 == 0).view(-1, 1, 1)
    return (~inside).to(torch.uint8)


@torch.no_grad()
def segmentation_sweep(model, src, levels=LEVELS, repeats=10, seed=1, batch=256, fill="black", protocol="BB",
                       out_size=None, gray=False, use_norm=True, tau=0.5, min_area=1, connectivity=8, cap=1024):
    """occlusion_sweep's loop for the OTHER output of the model: did the segmentation branch find the block?  The same
    levels, the same repeat rule (one extraction for (0, 1) and (100, 101)) and the same sweep_seed(seed, k, r) seeds, so the
    two tables line up row for row.  Every eval_pairs batch goes through the model; its `final_seg` (the second output)
    is scored against eval_pair_masks of the same arguments: segeval.mask_counts (pixels) and segeval.blob_totals (blobs
    of `connectivity`, at most `cap` per mask, found / false alarm at `tau`).  src: uint8 [N][H][W][3] on the device.

    Returns {"levels", "metrics": per level segeval.metrics_from_counts of the counts pooled over its repeats, "blobs": per
    level the blob_detection dict of the totals pooled over its repeats, "counts": per level int64 [repeats][4],
    "metrics_runs" / "blobs_runs": per level the lists of per-repeat dicts}.  A row with more than `cap` components in
    either mask (the salt-and-pepper output of an untrained branch) is left out of the blob totals and counted in the
    dict's "n_overflow" instead of ending the sweep; a labelling status other than 0 raises RuntimeError as in
    blob_detection.  ValueError for a model without a second output (use_osb=False) or whose final_seg is not
    [rows][2][oh][ow] of the input's size.
    The host waits for the device once per level, after its last launch."""
    from . import segeval
    levels = [(int(lo), int(hi)) for lo, hi in levels]
    res = {"levels": levels, "metrics": [], "blobs": [], "counts": [], "metrics_runs": [], "blobs_runs": []}
    n, h, w = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    batch = max(1, int(batch))
    for k, (lo, hi) in enumerate(levels):
        reps = 1 if (lo, hi) in ((0, 1), (100, 101)) else int(repeats)
        pix = torch.zeros(reps, 4, dtype=torch.int64, device=src.device)
        blob = torch.zeros(reps, 5, dtype=torch.int64, device=src.device)
        bad = []
        for r in range(reps):
            s = sweep_seed(seed, k, r)
            for i0 in range(0, n, batch):
                i1 = min(n, i0 + batch)
                x = eval_pairs(src[i0:i1], seed=s, index0=i0, lo=lo, hi=hi, fill=fill, protocol=protocol,
                               out_size=out_size, gray=gray, use_norm=use_norm)
                out = model(x)
                if not isinstance(out, (tuple, list)) or len(out) < 2 or out[1] is None:
                    raise ValueError("segmentation_sweep: the model returns no final_seg (use_osb=False?)")
                seg = out[1]
                if seg.dim() != 4 or seg.shape[0] != x.shape[0] or seg.shape[1] != 2 or seg.shape[2:] != x.shape[2:]:
                    raise ValueError("segmentation_sweep: final_seg is %s for inputs %s" % (tuple(seg.shape), tuple(x.shape)))
                if seg.dtype not in (torch.float32, torch.bfloat16):
                    seg = seg.float()
                seg = seg.contiguous()
                gt = eval_pair_masks(i1 - i0, h, w, seed=s, index0=i0, lo=lo, hi=hi, protocol=protocol, out_size=out_size,
                                     device=src.device)
                segeval.mask_counts(seg, gt, total=pix[r])
                totals, over, failed = segeval.blob_totals(seg, gt, tau, min_area, connectivity, cap)
                blob[r, :4] += (totals * (~over).view(-1, 1)).sum(0)
                blob[r, 4] += over.sum()
                bad.append((2 * i0, failed))
        for row0, failed in bad:                                # the level's first wait for the device
            segeval.raise_if_failed(failed, row0)
        pix_h, blob_h = pix.cpu().numpy(), blob.cpu().numpy()
        res["counts"].append(pix_h)
        res["metrics"].append(segeval.metrics_from_counts(pix_h.sum(0)))
        res["blobs"].append(_blob_dict(blob_h.sum(0)))
        res["metrics_runs"].append([segeval.metrics_from_counts(c) for c in pix_h])
        res["blobs_runs"].append([_blob_dict(t) for t in blob_h])
    return res


def _blob_dict(t):
    from . import segeval
    d = segeval.detection_from_totals(t[:4])
    d["n_overflow"] = int(t[4])
    return d
