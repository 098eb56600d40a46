"""Writes the MTCNN fixtures of the detector tests: tests/golden/mtcnn_{pnet,rnet,onet}.npz (the reference's three weight
sets as plain f32 arrays under its parameter names; O-Net's features.conv5.weight split row-wise over two files so that no
file exceeds 1 MiB) and tests/golden/g13_mtcnn.npz (inputs, every intermediate and the results of the reference).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_mtcnn.py [REFERENCE_ROOT]

Runs with the reference as the working directory, because get_nets.py loads its weights by relative path.  PNet / RNet /
ONet, box_utils and first_stage are imported as they are (the package's __init__ is bypassed: it pulls in plotting code);
eval/preprocess/mtcnn.py imports cv2 at module level, so MTCNN.detect_faces is cut out of its syntax tree and run with
`self` a plain namespace holding the three nets.  Nothing of the reference's text goes into the files.

Inputs: a 300 x 170 composite on a (90, 110, 130) background holding datasets/3d_tools/samples/Tom_Hanks_54745.png at
(5, 20), datasets/augment/375_face.jpg resized to 80 x 80 at (125, 60) and datasets/augment/Dan_Kellner_0001.jpg resized
to 70 x 70 at (222, 10); and the 112 x 112 375_face.jpg alone.  Runs: min_face_size 24.5 and 32 on both (keys c24_, c32_,
f24_, f32_; mfs_small / mfs_large hold the two values), and the pyramid alone at min_face_size 20 and 64 on the composite
(c20_, c64_).  The small size is 24.5 and not 20: of 20, 20.5, 21, ... 32 it is the first at which this layout meets all
four conditions below on both images (at 20 an overlap inside one scale equals 0.5 exactly and a rounded value lies
0.0045 from a half-integer); 32 meets them as it is.

The intermediates are logged from the cut detect_faces itself (drive(): wrappers around the functions it calls, forward
hooks on the nets).  Every run is made twice, in f32 as the reference runs and with the nets cast to f64 and
torch.FloatTensor, through which the reference uploads its inputs, giving f64.  floor_{pnet,rnet,onet,final} are
max |f32 - f64| per output kind over all runs.  tests/mtcnn_cases.py is run beside it and must give the same box lists;
its trace gives the margins, which are asserted (and stored as margin_*): probabilities >= 1e-3 from their threshold,
overlaps >= 1e-3 from theirs, rounded values >= 1e-2 from a half-integer, no NMS call with equal scores among more than
16 boxes."""
import ast
import importlib
import math
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference"))
GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT = 1 << 20
THR, NMS_THR, FACTOR = [0.6, 0.7, 0.8], [0.7, 0.7, 0.7], 0.707
MFS_SMALL, MFS_LARGE = 24.5, 32.0


def reference():
    os.chdir(REF)
    sys.path.insert(0, REF)
    pkg = "eval.preprocess.mtcnn_pytorch.src"
    parts = pkg.split(".")
    for i in range(1, len(parts) + 1):                       # bare packages: no __init__ is executed
        name = ".".join(parts[:i])
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, *parts[:i])]
        sys.modules[name] = m
    nets = importlib.import_module(pkg + ".get_nets")
    box = importlib.import_module(pkg + ".box_utils")
    first = importlib.import_module(pkg + ".first_stage")
    tree = ast.parse(open(os.path.join(REF, "eval", "preprocess", "mtcnn.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MTCNN"][0]
    fn = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "detect_faces"]
    ns = {"np": np, "torch": torch, "device": torch.device("cpu"), "run_first_stage": first.run_first_stage, "nms": box.nms,
          "calibrate_box": box.calibrate_box, "get_image_boxes": box.get_image_boxes,
          "convert_to_square": box.convert_to_square}
    exec(compile(ast.Module(body=fn, type_ignores=[]), "mtcnn", "exec"), ns)
    first.device = torch.device("cpu")
    return nets, (ns["detect_faces"], ns)


def images():
    bg = Image.new("RGB", (300, 170), (90, 110, 130))
    a = Image.open(os.path.join(REF, "datasets/3d_tools/samples/Tom_Hanks_54745.png")).convert("RGB")
    b = Image.open(os.path.join(REF, "datasets/augment/375_face.jpg")).convert("RGB")
    c = Image.open(os.path.join(REF, "datasets/augment/Dan_Kellner_0001.jpg")).convert("RGB")
    bg.paste(a, (5, 20))
    bg.paste(b.resize((80, 80)), (125, 60))
    bg.paste(c.resize((70, 70)), (222, 10))
    face = b if b.size == (112, 112) else b.resize((112, 112))
    return np.asarray(bg, np.uint8).copy(), np.asarray(face, np.uint8).copy()


HEADS = {"pnet": ("conv4_1", "conv4_2"), "rnet": ("conv5_1", "conv5_2"), "onet": ("conv6_1", "conv6_2", "conv6_3")}


def as_double(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def drive(ref, nets3, img_u8, min_face_size, double=False):
    """One run of the cut detect_faces with everything that passes through it logged: the names it calls
    (run_first_stage, nms, calibrate_box, get_image_boxes) are wrapped in its namespace for the duration, and forward
    hooks on the nets' head layers and inputs log the raw outputs and the crops.  double: the nets are the f64 copies and
    torch.FloatTensor, through which the reference uploads its inputs, gives f64 for the duration."""
    cut, ns = ref
    log = {"scale": [], "nms": [], "calibrate": [], "boxes": [], "in": {}, "head": {}}
    saved = {k: ns[k] for k in ("run_first_stage", "nms", "calibrate_box", "get_image_boxes")}

    def first_stage(image, net, scale, threshold):
        log["scale"].append(scale)
        return saved["run_first_stage"](image, net, scale=scale, threshold=threshold)

    def nms(boxes, *a, **k):
        keep = saved["nms"](boxes, *a, **k)
        log["nms"].append((np.array(boxes), list(keep)))
        return keep

    def calibrate(bboxes, offsets):
        log["calibrate"].append(np.hstack([np.array(bboxes), np.array(offsets, dtype=np.float64)]))
        return saved["calibrate_box"](bboxes, offsets)

    def image_boxes(bounding_boxes, img, size=24):
        out = saved["get_image_boxes"](bounding_boxes, img, size=size)
        log["boxes"].append(np.array(bounding_boxes))          # as the call leaves them: clipped to the image
        return out

    hooks = []
    for name, net in zip(("pnet", "rnet", "onet"), nets3):
        for head in HEADS[name]:
            hooks.append(getattr(net, head).register_forward_hook(
                lambda m, i, o, key=head: log["head"].setdefault(key, []).append(o.detach().numpy().copy())))
        hooks.append(net.register_forward_pre_hook(
            lambda m, i, key=name: log["in"].setdefault(key, []).append(i[0].detach().numpy().copy())))
    float_tensor = torch.FloatTensor
    ns.update(run_first_stage=first_stage, nms=nms, calibrate_box=calibrate, get_image_boxes=image_boxes)
    if double:
        torch.FloatTensor = as_double
    try:
        me = types.SimpleNamespace(pnet=nets3[0], rnet=nets3[1], onet=nets3[2])
        boxes, landmarks = cut(me, Image.fromarray(img_u8), min_face_size, THR, NMS_THR, FACTOR)
    finally:
        torch.FloatTensor = float_tensor
        ns.update(saved)
        for h in hooks:
            h.remove()
    image = Image.fromarray(img_u8)
    rec = {"scales": np.array(log["scale"], np.float64)}
    for li, s in enumerate(log["scale"]):
        size = (math.ceil(image.size[0] * s), math.ceil(image.size[1] * s))
        rec["level%d" % li] = np.asarray(image.resize(size, Image.BILINEAR), np.uint8)
        assert log["in"]["pnet"][li].shape[2:] == rec["level%d" % li].shape[:2]
        rec["pnet_a%d" % li], rec["pnet_b%d" % li] = log["head"]["conv4_1"][li][0], log["head"]["conv4_2"][li][0]
    assert len(log["nms"]) == 3 and len(log["calibrate"]) == 3 and len(log["boxes"]) == 2
    rec["boxes1"], rec["boxes2"] = log["calibrate"][0], log["calibrate"][1][:, :5]
    rec["boxes1r"], rec["boxes2r"] = log["boxes"]
    for key, name in (("crops24", "rnet"), ("crops48", "onet")):
        rec[key] = np.round(log["in"][name][0] / 0.0078125 + 127.5).astype(np.uint8).transpose(0, 2, 3, 1)
    rec["rnet_cls"], rec["rnet_off"] = log["head"]["conv5_1"][0], log["head"]["conv5_2"][0]
    rec["onet_cls"], rec["onet_off"], rec["onet_lm"] = (log["head"][k][0] for k in HEADS["onet"])
    rec["boxes3"], rec["landmarks"] = boxes, landmarks
    return rec


KINDS = {"pnet": ("pnet_a", "pnet_b"), "rnet": ("rnet_cls", "rnet_off"), "onet": ("onet_cls", "onet_off", "onet_lm"),
         "final": ("boxes3", "landmarks")}


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mtcnn_cases as mc
    nets, ref = reference()
    n32 = [nets.PNet().eval(), nets.RNet().eval(), nets.ONet().eval()]
    n64 = [nets.PNet().eval().double(), nets.RNet().eval().double(), nets.ONet().eval().double()]
    os.makedirs(GOLD, exist_ok=True)
    weights = []
    for name, net in zip(("pnet", "rnet", "onet"), n32):
        params = {k: v.detach().numpy().astype(np.float32) for k, v in net.named_parameters()}
        weights.append(params)
        files = [dict(params)]
        path = os.path.join(GOLD, "mtcnn_%s.npz" % name)
        np.savez(path, **files[0])
        if os.path.getsize(path) > LIMIT:
            os.remove(path)
            big = "features.conv5.weight"
            w = files[0].pop(big)
            half = w.shape[0] // 2
            files[0][big + ".part0"] = w[:half]
            files.append({big + ".part1": w[half:]})
            for i, f in enumerate(files):
                path = os.path.join(GOLD, "mtcnn_%s_%d.npz" % (name, i))
                np.savez(path, **f)
                assert os.path.getsize(path) <= LIMIT, path
        print(name, "written")
    composite, face = images()
    out = {"composite": composite, "face": face}
    floors = {k: 0.0 for k in KINDS}
    trace = {}
    out["mfs_small"], out["mfs_large"] = np.array(MFS_SMALL), np.array(MFS_LARGE)
    for tag, img, mfs in (("c24", composite, MFS_SMALL), ("c32", composite, MFS_LARGE), ("f24", face, MFS_SMALL),
                          ("f32", face, MFS_LARGE)):
        r32 = drive(ref, n32, img, mfs)
        r64 = drive(ref, n64, img, mfs, double=True)
        assert r32["pnet_a0"].dtype == np.float32 and r64["pnet_a0"].dtype == np.float64
        rec = {}
        b_mc, l_mc, dropped = mc.detect_faces(img, weights, mfs, THR, NMS_THR, FACTOR, np.float64, trace, rec)
        assert dropped == 0, tag
        for k in ("boxes1", "boxes1r", "boxes2", "boxes2r", "boxes3"):
            assert r32[k].shape == rec[k].shape == r64[k].shape, (tag, k, r32[k].shape, rec[k].shape)
            assert np.array_equal(r32[k][:, :4], rec[k][:, :4]) or k == "boxes3", (tag, k)
        for k, v in r32.items():
            if k.startswith("level") or k.startswith("crops"):
                assert np.array_equal(v, rec[k]), (tag, k)
        for kind, prefixes in KINDS.items():
            for k in r32:
                if k.rstrip("0123456789") in prefixes:
                    floors[kind] = max(floors[kind], float(np.abs(r32[k].astype(np.float64) - r64[k]).max()))
        for k, v in r32.items():
            out["%s_%s" % (tag, k)] = v
        out["%s_boxes3_f64" % tag], out["%s_landmarks_f64" % tag] = r64["boxes3"], r64["landmarks"]
        print(tag, "levels", len(r32["scales"]), "boxes", [len(r32[k]) for k in ("boxes1", "boxes2", "boxes3")])
    for tag, mfs in (("c20_", 20.0), ("c64_", 64.0)):
        for k, v in drive(ref, n32, composite, mfs).items():
            if k == "scales" or k.startswith("level"):
                out[tag + k] = v
        for li, s in enumerate(out[tag + "scales"]):
            sh, sw = mc.level_size(composite.shape[0], composite.shape[1], s)
            assert np.array_equal(mc.resize(composite, sw, sh), out[tag + "level%d" % li]), (tag, li)
    print("margins", trace, "floors", floors)
    assert trace["prob"] >= 1e-3 and trace["overlap"] >= 1e-3 and trace["round"] >= 1e-2 and trace.get("ties", 0) <= 16
    for k, v in floors.items():
        out["floor_" + k] = np.array(v)
    for k in ("prob", "overlap", "round"):
        out["margin_" + k] = np.array(trace[k])
    out["margin_ties"] = np.array(trace.get("ties", 0))
    path = os.path.join(GOLD, "g13_mtcnn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= LIMIT


if __name__ == "__main__":
    main()
