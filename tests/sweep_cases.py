"""Shared by tests/test_sweep_cpu.py, tests/test_gpu_sweep.py and tools/bench_sweep.py: an independent restatement (PIL
and numpy, no import of msml_amd.verification) of the model inputs of test.py -- _load_one_input of
eval/qeval_mxnet.py:173-189 with the transform of :97-101 / :544-547 and the normalisation of :319-324 -- and the case
table the tests run on.

* `crop_origin(d)` / `center_crop_geometry(insz, outsz)`   torchvision's CenterCrop arithmetic for one axis
* `center_crop(img, oh, ow)`       the same on a PIL image: ImageOps.expand with zeros, then Image.crop
* `normals(seed, row, bh, bw, c)`  the gauss fill's standard normals: the counter-based generator of csrc/evalin.hip
* `f_paste_byte(v)`                the byte Image.paste stores for a mode-F block value in an L image (the stated rule;
                                   tests/test_sweep_cpu.py checks it against PIL)
* `block_image(...)`               the occluder image exactly as rand_occ.py:52-64 constructs it
* `reference_rows(src, desc, ...)` every output row with PIL itself: Image.fromarray, transpose(FLIP_LEFT_RIGHT),
                                   pad + crop, convert('L'), Image.paste of the block image, then the f32 steps

torchvision is not installed where this was written.  The arithmetic restated here is that of
torchvision.transforms.functional.center_crop as its source reads since 0.10:

    if crop_width > image_width or crop_height > image_height:
        padding_ltrb = [
            (crop_width - image_width) // 2 if crop_width > image_width else 0,
            (crop_height - image_height) // 2 if crop_height > image_height else 0,
            (crop_width - image_width + 1) // 2 if crop_width > image_width else 0,
            (crop_height - image_height + 1) // 2 if crop_height > image_height else 0,
        ]
        img = pad(img, padding_ltrb, fill=0)
        ...
    crop_top = int(round((image_height - crop_height) / 2.0))
    crop_left = int(round((image_width - crop_width) / 2.0))
    return crop(img, crop_top, crop_left, crop_height, crop_width)

It has NOT been compared with a torchvision build, and not with the 0.8.2 of the reference's requirements.txt:120 in
particular; msml_amd/data.py load_occluder_sets already restates CenterCrop the same way.
"""
import numpy as np
from PIL import Image, ImageOps

from oracle import occ as O

f32 = np.float32
FLIP = getattr(getattr(Image, "Transpose", Image), "FLIP_LEFT_RIGHT")
GAUSS_SALT = 0x6761757373
FILLS = ("black", "white", "gauss")
NEAR = 1e-6                       # |z * 255 - nearest integer| below which the gauss byte may fall either way

# (source H, source W, out h, out w, gray, norm): the table of the issue this file was written for
CASES = ((112, 112, 112, 112, 0, 1),      # identity geometry
         (112, 112, 128, 128, 1, 0),      # pad 8 / 8, the LightCNN recipe
         (113, 115, 128, 128, 1, 0),      # odd pad 7 / 8 and 6 / 7
         (112, 112, 112, 96, 0, 1),       # crop on one axis, non-square block range
         (117, 115, 112, 112, 0, 1),      # crop differences 5 and 3 (half to even), mirror-then-crop
         (20, 12, 16, 16, 0, 0))          # pad one axis and crop the other, tiny rows
LEVELS = ((0, 1), (10, 11), (90, 91))


def crop_origin(d):
    """int(round(d / 2.0)) with Python's round: half to even."""
    return int(round(d / 2.0))


def center_crop_geometry(insz, outsz):
    """(zeros in front, zeros behind, crop origin in the padded axis) of CenterCrop for one axis."""
    if outsz > insz:
        return (outsz - insz) // 2, (outsz - insz + 1) // 2, 0
    return 0, 0, crop_origin(insz - outsz)


def center_crop(img, oh, ow):
    w, h = img.size
    l, r, left = center_crop_geometry(w, ow)
    t, b, top = center_crop_geometry(h, oh)
    if l or r or t or b:
        img = ImageOps.expand(img, border=(l, t, r, b), fill=0)
    return img.crop((left, top, left + ow, top + oh))


def _mix(z):
    """splitmix64 on a uint64 array (oracle.occ._mix for arrays)."""
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def normals(seed, row, bh, bw, channels):
    """[bh][bw][channels] f64 standard normals of output row `row` = 2 * (global image index) + mirrored."""
    with np.errstate(over="ignore"):
        key = O._mix((O._mix((seed + GAUSS_SALT) & O.M64) + row) & O.M64)
        ry, rx, c = np.meshgrid(np.arange(bh, dtype=np.uint64), np.arange(bw, dtype=np.uint64),
                                np.arange(channels, dtype=np.uint64), indexing="ij")
        r = _mix(np.uint64(key) + ((ry * np.uint64(256) + rx) * np.uint64(4) + c))
    u1 = ((r >> np.uint64(32)).astype(np.float64) + 1.0) * (1.0 / 4294967296.0)
    u2 = (r & np.uint64(0xFFFFFFFF)).astype(np.float64) * (1.0 / 4294967296.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def f_paste_byte(v):
    """What Image.paste stores in an L image for the value v of a mode-F block: v as f32; <= 0 -> 0, >= 255 -> 255,
    else truncated."""
    v = np.asarray(v, np.float64).astype(f32)
    return np.where(v <= 0, 0, np.where(v >= 255, 255, np.trunc(v))).astype(np.uint8)


def block_image(fill, mode, bh, bw, z=None):
    """rand_occ.py:52-64 (a bh x bw block; the reference's is square).  z: normals(...) for the gauss fill."""
    if fill == "black":
        return Image.fromarray(np.zeros([bh, bw], dtype=np.uint8))
    if fill == "white":
        return Image.fromarray(np.ones([bh, bw], dtype=np.uint8) * 255)
    if mode == "L":
        return Image.fromarray(z[:, :, 0] * 255)                     # float64 -> a mode-F image
    # (z * 255).astype(np.uint8) as numpy does it on x86-64: truncate toward zero, wrap modulo 256
    return Image.fromarray((z * 255).astype(np.int64).astype(np.uint8))


def near_integer(z):
    v = z * 255
    return np.abs(v - np.rint(v)) < NEAR


def to_tensor(img, norm):
    a = np.asarray(img, np.uint8)
    a = a[:, :, None] if a.ndim == 2 else a
    v = a.astype(f32) / f32(255.0)
    if norm:
        v = v - f32(0.5)
        v = v / f32(0.5)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def reference_rows(src, desc, oh, ow, gray=0, norm=1, fill="black", protocol="BB", seed=1, index0=0):
    """src [N][H][W][3] uint8, desc [2N][64] int32 (kinds 0 / 3) or None -> (rows [2N][C][oh][ow] f32, near [same shape]
    bool: the gauss pixels whose z * 255 lies within NEAR of an integer, block pixels drawn)."""
    n = src.shape[0]
    ch = 1 if gray else 3
    out = np.empty((2 * n, ch, oh, ow), f32)
    near = np.zeros(out.shape, bool)
    drawn = 0
    for i in range(n):
        g = index0 + i
        for f in (0, 1):
            img = Image.fromarray(src[i])
            if f:
                img = img.transpose(FLIP)
            img = center_crop(img, oh, ow)
            if protocol == "NB" and g % 2:
                assert not gray
                out[2 * i + f] = to_tensor(img, norm)
                continue
            if gray:
                img = img.convert("L")
            d = None if desc is None else desc[2 * i + f]
            if d is not None and int(d[0]) != 0:
                assert int(d[0]) == 3
                x0, y0, bw, bh = (int(v) for v in d[1:5])
                z = normals(seed, 2 * g + f, bh, bw, ch) if fill == "gauss" else None
                img = img.copy()
                img.paste(block_image(fill, img.mode, bh, bw, z), (x0, y0))
                if z is not None:
                    y1, x1 = min(y0 + bh, oh), min(x0 + bw, ow)
                    near[2 * i + f, :, y0:y1, x0:x1] = near_integer(z)[:y1 - y0, :x1 - x0].transpose(2, 0, 1)
                    drawn += z.size
            out[2 * i + f] = to_tensor(img, norm)
    return out, near, drawn


def faces(h, w, seed):
    """5 images of random bytes, one all 255, one all 0."""
    a = np.random.default_rng(seed).integers(0, 256, (7, h, w, 3), dtype=np.uint8)
    a[5], a[6] = 255, 0
    return a


def draw(n, seed, index0, lo, hi, ow):
    """The 2n block descriptors of images index0 .. index0 + n - 1: counter 2 g + f, block range of an ow-wide square."""
    return O.draw(seed, 2 * index0, 2 * n, ow, ow, 2, lo, hi, flip=False)
