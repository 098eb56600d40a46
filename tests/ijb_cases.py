"""Shared by tests/test_ijb_cpu.py, tests/test_gpu_ijb.py, tools/make_golden_ijb.py and tools/bench_ijb.py: the
seeded synthetic template-verification set, and a vectorised numpy / sklearn restatement of the three reference
functions the goldens were recorded from (image2template_feature and verification of eval/qeval_ijbc.py,
Verification.start_verification of eval/qeval_mxnet.py).  The restatement sums in another order than the reference's
loops, so it agrees with them to rounding, not to the bit; counts and tables agree exactly."""
import numpy as np

FPRS = (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1)
GOLDEN_SET = dict(seed=7, n_img=6000, e=64, n_tmpl=500, n_ident=120, noise=1.2, n_pairs=30000)
GOLDEN_PAIRS = dict(seed=11, n_pairs=600, e=64, noise=4.0)


def tolerance(max_rows, e):
    """Absolute bound on template features and pair scores: f64 sums of at most max_rows (pooling) + e (norm, dot)
    terms bounded by the row norm, taken in another order; 8 is the margin."""
    return 8.0 * (max_rows + e) * 2.0 ** -53


def make_set(seed, n_img, e, n_tmpl, n_ident, noise, n_pairs):
    """n_pairs is an upper bound (duplicates are dropped).  Images of n_ident identities in n_tmpl templates with
    sparse unsorted ids; media ids are shared by one to about
    six images of a template and reused between templates; a fifth of the pairs are same-identity, p1 in long runs."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((n_ident, e))
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    tmpl_ids = rng.choice(np.arange(3, 40 * n_tmpl), n_tmpl, replace=False).astype(np.int64)
    tmpl_ident = np.r_[np.arange(n_ident), rng.integers(0, n_ident, n_tmpl - n_ident)] if n_tmpl >= n_ident \
        else rng.integers(0, n_ident, n_tmpl)
    # very uneven templates: a few take most images, every template has at least one
    weight = rng.pareto(1.5, n_tmpl) + 0.05
    t_of_img = np.r_[rng.permutation(n_tmpl), rng.choice(n_tmpl, n_img - n_tmpl, p=weight / weight.sum())]
    t_of_img = t_of_img[rng.permutation(n_img)]
    templates = tmpl_ids[t_of_img]
    rows = np.bincount(t_of_img, minlength=n_tmpl)
    medias = (rng.integers(0, 1 << 30, n_img) % np.maximum(1, (rows[t_of_img] + 2) // 3)).astype(np.int64) * 7 + 100
    ident = tmpl_ident[t_of_img]
    quality = rng.uniform(0.3, 1.0, (n_img, 1))
    orig = centers[ident] * quality + noise / np.sqrt(e) * rng.standard_normal((n_img, e))
    flip = orig + 0.3 * noise / np.sqrt(e) * rng.standard_normal((n_img, e))
    img_feats = np.concatenate([orig, flip], 1).astype(np.float32)
    faceness = rng.uniform(0.2, 1.0, n_img).astype(np.float32)
    # pairs
    n_same = n_pairs // 5
    a = rng.integers(0, n_tmpl, n_pairs)
    b = rng.integers(0, n_tmpl, n_pairs)
    by_ident = [np.flatnonzero(tmpl_ident == i) for i in range(n_ident)]
    for k in range(n_same):
        b[k] = rng.choice(by_ident[tmpl_ident[a[k]]])
    # no template against itself and no pair twice (in either order): such scores tie exactly or to an ulp, and
    # whether two scores one ulp apart count as one ROC point must not decide a test
    _, first = np.unique(np.minimum(a, b) * n_tmpl + np.maximum(a, b), return_index=True)
    first = first[a[first] != b[first]]
    a, b = a[first], b[first]
    o = np.argsort(a, kind="stable")
    a, b = a[o], b[o]
    label = (tmpl_ident[a] == tmpl_ident[b]).astype(np.int64)
    return {"img_feats": img_feats, "faceness": faceness, "templates": templates, "medias": medias,
            "p1": tmpl_ids[a], "p2": tmpl_ids[b], "label": label}


def make_pairs(seed, n_pairs, e, noise):
    """Embeddings of n_pairs pairs (rows 2i, 2i + 1), exactly half of them same-identity, shuffled."""
    rng = np.random.default_rng(seed)
    issame = np.zeros(n_pairs, bool)
    issame[rng.permutation(n_pairs)[:n_pairs // 2]] = True
    a = rng.standard_normal((n_pairs, e))
    other = rng.standard_normal((n_pairs, e))
    b = np.where(issame[:, None], a, other) + noise * rng.standard_normal((n_pairs, e)) * rng.uniform(0.2, 1, (n_pairs, 1))
    emb = np.empty((2 * n_pairs, e), np.float32)
    emb[0::2], emb[1::2] = a, b
    return emb, issame


# ---------------------------------------------------------------------------------------------------------------------
def input_feats(img_feats, faceness=None, flip_sum=True, single=False, dtype=np.float64):
    """What get_template_features hands to image2template_feature (flip sum or first half, times the detector score),
    computed in `dtype`."""
    x = np.asarray(img_feats).astype(dtype)
    if not single:
        e = x.shape[1] // 2
        x = x[:, :e] + x[:, e:] if flip_sum else x[:, :e]
    if faceness is not None:
        x = x * np.asarray(faceness).astype(dtype)[:, None]
    return x


def pool_ref(x, templates, medias):
    """image2template_feature, vectorised: (L2-normalised template features f64, unique_templates, max rows)."""
    templates, medias = np.asarray(templates), np.asarray(medias)
    ut, t_inv = np.unique(templates, return_inverse=True)
    um, m_inv = np.unique(medias, return_inverse=True)
    key = t_inv.astype(np.int64) * um.size + m_inv
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    count = np.diff(np.r_[start, ks.size])
    means = np.add.reduceat(np.asarray(x, np.float64)[order], start, axis=0) / count[:, None]
    t_of_media = ks[start] // um.size
    t_start = np.flatnonzero(np.r_[True, t_of_media[1:] != t_of_media[:-1]])
    tf = np.add.reduceat(means, t_start, axis=0)
    norm = np.sqrt(np.einsum("ij,ij->i", tf, tf))
    norm[norm == 0] = 1.0
    return tf / norm[:, None], ut, int(np.bincount(t_inv).max())


def scores_ref(tn, ut, p1, p2, batch=100000):
    """verification, vectorised per batch."""
    r1, r2 = np.searchsorted(ut, p1), np.searchsorted(ut, p2)
    assert (ut[r1] == p1).all() and (ut[r2] == p2).all()
    out = np.empty(len(r1))
    for i in range(0, len(r1), batch):
        out[i:i + batch] = np.einsum("ij,ij->i", tn[r1[i:i + batch]], tn[r2[i:i + batch]])
    return out


def roc_ref(scores, label, fprs=FPRS):
    """The TPR @ FPR table of qeval_ijbc.py:565-585: (tprs, auc, number of roc_curve points, kept fps, kept tps)."""
    from sklearn.metrics import auc, roc_curve
    fpr, tpr, _ = roc_curve(label, scores)
    area = auc(fpr, tpr)
    n_pos, n_neg = int(np.sum(np.asarray(label) != 0)), int(np.sum(np.asarray(label) == 0))
    rf, rt = fpr[::-1], tpr[::-1]
    tprs = []
    for x in fprs:
        d = np.abs(rf - x)
        tprs.append(rt[np.flatnonzero(d == d.min())[0]])       # the smallest index of the reversed curve wins a tie
    return (np.asarray(tprs), float(area), len(fpr), np.rint(fpr[1:] * n_neg).astype(np.int64),
            np.rint(tpr[1:] * n_pos).astype(np.int64))


def start_verification_ref(emb, issame):
    """Verification.start_verification, its two counting loops as searches in sorted arrays: (acc, tarfar[5])."""
    import sklearn.preprocessing
    from sklearn.metrics import roc_curve
    f = sklearn.preprocessing.normalize(np.asarray(emb, np.float64))
    a, b = f[0::2], f[1::2]
    dist = 1.0 - np.clip(np.einsum("ij,ij->i", a, b) / (np.sqrt(np.einsum("ij,ij->i", a, a)) *
                                                        np.sqrt(np.einsum("ij,ij->i", b, b))), -1.0, 1.0)
    gt = np.where(np.asarray(issame, bool), 0, 1)
    fpr, tpr, _ = roc_curve(gt, dist)
    acc = tpr[np.argmin(np.abs(tpr - (1 - fpr)))]
    cnt = len(dist) // 2
    pos, neg = np.sort(dist[gt == 0]), np.sort(dist[gt == 1])
    assert len(pos) == cnt and len(neg) == cnt
    far = np.searchsorted(neg, neg, side="left") / cnt
    tarfar = np.zeros(5)
    for k, fv in enumerate((1e-1, 1e-2, 1e-3, 1e-4)):
        t = neg[np.flatnonzero(far <= fv)[-1]]
        tarfar[k] = np.searchsorted(pos, t, side="right") / cnt
    return float(acc), tarfar
