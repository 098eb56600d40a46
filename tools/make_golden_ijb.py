"""Record the template-verification golden (tests/golden/g11_ijb.npz) from the reference's own functions.

Needs the reference checkout (first argument, default ../reference next to this repository); runs on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ijb.py [REFERENCE_ROOT]

eval/qeval_ijbc.py and eval/qeval_mxnet.py are programs, not modules (module-level argparse, cv2, mxnet, menpo), so
they are parsed with `ast` and ONLY image2template_feature, verification and the method
Verification.start_verification are compiled, in a namespace that supplies np, sklearn.preprocessing, cdist,
roc_curve, auc and a do-nothing plt.  Nothing of their text is written anywhere.  The TPR @ FPR table of
qeval_ijbc.py:565-585 is module-level code there; it is sklearn's roc_curve / auc plus a nearest-point pick, stated
here.  Inputs come from tests/ijb_cases.py by seed; the file holds seeds, sizes and results only:

  tn, ut, scores        the two reference functions on FLOAT64 inputs (the pin)
  f32_diff              largest difference of features / scores to the same functions on the float32 inputs the
                        reference script really feeds them (recorded for DESIGN.md, not asserted)
  tprs, auc, n_points   the table of the raw scores; *_r2 the same for the scores rounded to two decimals
  sv_acc, sv_tarfar     start_verification on GOLDEN_PAIRS

The set must be STABLE: the table is recomputed with every score moved by +tol and by -tol (tests/ijb_cases.py
tolerance) and with the restated scores; if an entry changes nothing is written -- pick another seed.
"""
import ast
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
OUT = os.path.join(ROOT, "tests", "golden", "g11_ijb.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

from tests import ijb_cases as C  # noqa: E402


class _Plt:
    def __getattr__(self, name):
        return lambda *a, **k: None


def namespace():
    import sklearn.preprocessing
    from scipy.spatial.distance import cdist
    from sklearn.metrics import auc, roc_curve
    return {"np": np, "sklearn": sklearn, "cdist": cdist, "roc_curve": roc_curve, "auc": auc, "plt": _Plt(), "os": os}


def reference_functions():
    ns = namespace()
    tree = ast.parse(open(os.path.join(REF, "eval", "qeval_ijbc.py")).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("image2template_feature", "verification")]
    assert len(keep) == 2
    exec(compile(ast.Module(body=keep, type_ignores=[]), "qeval_ijbc", "exec"), ns)
    tree = ast.parse(open(os.path.join(REF, "eval", "qeval_mxnet.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Verification"][0]
    meth = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "start_verification"]
    assert len(meth) == 1
    exec(compile(ast.Module(body=meth, type_ignores=[]), "qeval_mxnet", "exec"), ns)
    return ns["image2template_feature"], ns["verification"], ns["start_verification"]


def table(scores, label):
    """qeval_ijbc.py:565-585 with roc_curve / auc of sklearn: nearest point of the reversed curve, first on a tie."""
    from sklearn.metrics import auc, roc_curve
    fpr, tpr, _ = roc_curve(label, scores)
    area = auc(fpr, tpr)
    fpr, tpr = np.flipud(fpr), np.flipud(tpr)
    tprs = [tpr[min(range(len(fpr)), key=lambda i: (abs(fpr[i] - x), i))] for x in C.FPRS]
    return np.asarray(tprs), float(area), len(fpr)


class _Task:
    pass


if __name__ == "__main__":
    pool, verify, start_verification = reference_functions()
    s = C.make_set(**C.GOLDEN_SET)
    quiet = contextlib.redirect_stdout(io.StringIO())
    rec = {}
    with quiet:
        tn, ut = pool(C.input_feats(s["img_feats"], s["faceness"]), s["templates"], s["medias"])
        scores = verify(tn, ut, s["p1"], s["p2"])
        tn32, _ = pool(C.input_feats(s["img_feats"], s["faceness"], dtype=np.float32), s["templates"], s["medias"])
        scores32 = verify(tn32, ut, s["p1"], s["p2"])
    rec["tn"], rec["ut"], rec["scores"] = tn, ut, scores
    rec["f32_diff"] = np.array([np.abs(tn32 - tn).max(), np.abs(scores32 - scores).max()])
    tn_r, ut_r, max_rows = C.pool_ref(C.input_feats(s["img_feats"], s["faceness"]), s["templates"], s["medias"])
    tol = C.tolerance(max_rows, C.GOLDEN_SET["e"])
    rec["max_rows"] = np.int64(max_rows)
    label = s["label"]
    tprs, area, npts = table(scores, label)
    rec["tprs"], rec["auc"], rec["n_points"] = tprs, np.float64(area), np.int64(npts)
    r2 = np.round(scores, 2)
    rec["tprs_r2"], rec["auc_r2"], rec["n_points_r2"] = (np.asarray(v) for v in table(r2, label))
    # stability proof
    restated = C.scores_ref(tn_r, ut_r, s["p1"], s["p2"])
    assert np.abs(restated - scores).max() <= tol and np.abs(tn_r - tn).max() <= tol, "restatement outside the bound"
    for name, moved in (("+tol", scores + tol), ("-tol", scores - tol), ("restated", restated)):
        t2, _, n2 = table(moved, label)
        if not np.array_equal(t2, tprs) or n2 != npts:
            sys.exit("unstable set (%s): %r vs %r, %d vs %d points -- pick another seed" % (name, t2, tprs, n2, npts))
    gap = np.diff(np.sort(scores))
    print("tprs", tprs, "auc", area, "points", npts, "| r2:", rec["tprs_r2"], rec["n_points_r2"])
    print("smallest score gap %.3e (ties %d), tol %.3e, max rows %d, f32 diff %r" %
          (gap[gap > 0].min(), int((gap == 0).sum()), tol, max_rows, rec["f32_diff"]))
    # start_verification
    emb, issame = C.make_pairs(**C.GOLDEN_PAIRS)
    import sklearn.preprocessing
    task = _Task()
    task.feature = sklearn.preprocessing.normalize(emb.astype(np.float64))   # Verification._prepare, on f64
    task.ground_truth_label = [0 if v else 1 for v in issame]      # qeval_mxnet.py:550-551
    task.save_path = os.devnull
    with quiet:
        acc, tarfar = start_verification(task)
    rec["sv_acc"], rec["sv_tarfar"] = np.float64(acc), np.asarray(tarfar)
    acc_r, tarfar_r = C.start_verification_ref(emb, issame)
    assert acc_r == acc and np.array_equal(tarfar_r, tarfar), (acc_r, acc, tarfar_r, tarfar)
    print("start_verification", acc, tarfar)
    np.savez_compressed(OUT, **rec)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
