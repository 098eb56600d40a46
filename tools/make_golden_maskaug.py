"""Writes tests/golden/g12_maskaug.npz: the reference's _add_gauss_to_mask on small inputs, with every random draw logged.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_maskaug.py [REFERENCE_ROOT]

datasets/load_dataset.py imports mxnet, torchvision and cv2 at module level, so the two methods this golden is about,
FaceByRandOccMask._add_gauss_to_mask (:203-280) and FaceByRandOccMask._get_gauss (:282-339), are cut out of its syntax tree
and run with numpy and torch alone, `self` being a plain namespace with out_size, is_gray and _get_gauss.  The run is
seeded with np.random.seed(s); np.random.randint / random / uniform / randn are wrapped for its duration so that every
value drawn is logged in order (a randn array is logged as one entry and stored beside the log).  Nothing of the
reference's text goes into the file: it holds the seeds, the inputs, the draws and the outputs.

Cases: the three transform types, both signs of light and of block, gray 128 x 128 and RGB 112 x 112 -- for each the
first seed whose draws give the wanted type and sign.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
OUT = os.path.join(ROOT, "tests", "golden", "g12_maskaug.npz")
# (type, sign or None, gray, size); type 0 light, 1 noise, 2 block as tests/maskaug_cases.py
CASES = [(0, 1, False, 112), (0, -1, True, 128), (1, None, False, 112), (1, None, True, 128), (2, 1, True, 128),
         (2, -1, False, 112)]


def reference_methods():
    tree = ast.parse(open(os.path.join(REF, "datasets", "load_dataset.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "FaceByRandOccMask"][0]
    keep = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("_add_gauss_to_mask", "_get_gauss")]
    assert len(keep) == 2
    for n in keep:
        n.decorator_list = []                      # _get_gauss is a staticmethod: called through the namespace below
    ns = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=keep, type_ignores=[]), "load_dataset", "exec"), ns)
    return ns["_add_gauss_to_mask"], ns["_get_gauss"]


class Logged:
    """np.random.{randint, random, uniform, randn} logged for the duration of a `with`."""
    NAMES = ("randint", "random", "uniform", "randn")

    def __enter__(self):
        self.log, self.arrays, self.saved = [], [], {n: getattr(np.random, n) for n in self.NAMES}
        for name, fn in self.saved.items():
            setattr(np.random, name, self.wrap(name, fn))
        return self

    def wrap(self, name, fn):
        def logged(*a, **k):
            v = fn(*a, **k)
            if np.ndim(v):
                self.arrays.append(np.array(v, np.float64))
                self.log.append((name, 0.0))
            else:
                self.log.append((name, float(v)))
            return v
        return logged

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(np.random, name, fn)


def inputs(gray, size, seed):
    """A blocky face (8 x 8 tiles, so the file stays small) in [0, 1] and a mask plane as the Resize leaves it: 255 on the
    face, 0 on the lower face, a ramp with values on both sides of 128 (127, 128, 129 among them) along the edge."""
    rng = np.random.RandomState(1000 + seed)
    c = 1 if gray else 3
    tiles = rng.randint(0, 256, (c, size // 8, size // 8)).astype(np.uint8)
    face = np.kron(tiles, np.ones((1, 8, 8), np.uint8))
    y, x = np.mgrid[0:size, 0:size]
    depth = np.minimum(np.minimum(y - size // 2, (size - 4) - y), np.minimum(x - size // 5, (size - size // 5) - x))
    mask = np.clip(255 - depth * 42, 0, 255).astype(np.uint8)
    mask[size // 2 + 3, size // 5 + 10:size // 5 + 13] = [127, 128, 129]
    return face, mask


def run(fn, gauss, gray, size, seed):
    face, mask = inputs(gray, size, seed)
    me = types.SimpleNamespace(out_size=(size, size), is_gray=gray, _get_gauss=gauss)
    np.random.seed(seed)
    with Logged() as lg:
        out_face, out_mask = fn(me, torch.from_numpy(face.astype(np.float32) / np.float32(255.0)), mask, True)
    assert isinstance(out_face, torch.Tensor) and out_face.dtype == torch.float32 and out_mask.dtype == torch.int32
    return face, mask, lg, out_face.numpy(), out_mask.numpy()


def main():
    fn, gauss = reference_methods()
    out = {"cases": np.array(len(CASES))}
    for i, (ty, sign, gray, size) in enumerate(CASES):
        for seed in range(1000):
            face, mask, lg, of, om = run(fn, gauss, gray, size, seed)
            tt = int(lg.log[0][1])
            got = 0 if tt >= 7 else (1 if tt >= 5 else 2)
            vals = [v for _, v in lg.log]
            s = None if got == 1 else int(vals[6 if got == 0 else 5]) * 2 - 1
            if got == ty and s == sign and (got != 1 or sum(vals[-3:]) in (1, 2)):
                break
        else:
            raise SystemExit("no seed for case %d" % i)
        p = "c%d_" % i
        out.update({p + "seed": np.array(seed), p + "gray": np.array(gray), p + "size": np.array(size), p + "face": face,
                    p + "mask": mask, p + "log_names": np.array([n for n, _ in lg.log]),
                    p + "log_vals": np.array(vals, np.float64), p + "out_face": of, p + "out_mask": om})
        if lg.arrays:
            assert len(lg.arrays) == 1
            out[p + "randn"] = lg.arrays[0]
        print("case", i, "type", ty, "sign", sign, "gray", gray, "size", size, "seed", seed, "draws", len(vals),
              "face", of.shape, of.dtype, "range", float(of.min()), float(of.max()))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
