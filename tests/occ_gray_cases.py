"""Shared by tests/test_occ_gray_cpu.py and tests/test_gpu_occ_gray.py: the CPU restatement of the gray / resized /
unnormalised output of the device input pipeline (msml_occ_draw_out / msml_occ_apply_out, msml_amd/csrc/occ.hip).

What the reference's FaceByRandOccMask.__getitem__ does with is_gray / out_size / use_norm
(datasets/load_dataset.py:86-139,179,183-201), in its order:
  occlude the RGB face at the source size (oracle.occ: draw, inside, paste -- unchanged)
  -> convert('L')                          rgb_to_l: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
  -> transforms.Resize(out_size)           resize_bilinear: Image.resize((w, h), BILINEAR) of face, 0 / 255 mask, clean face
  -> flip                                  in output coordinates
  -> ToTensor, _add_gauss_to_face          oracle.occ.light_map at the OUTPUT size, / max
  -> Msk2Tenser                            mask != 255 -> 0, else 1
  -> Normalize(0.5, 0.5) only with use_norm
The two new stages are written from Pillow's documented arithmetic (Convert.c's L24 weights; Resample.c's
precompute_coeffs + normalize_coeffs_8bpc + the two 8-bit passes with the triangle filter) as oracle/occ.py does for
bicubic, and tests/test_occ_gray_cpu.py pins them BIT FOR BIT to PIL itself -- the library the reference calls.
"""
import numpy as np

from oracle import occ as oo

f32 = np.float32
# (gray, out_size, use_norm) of the GPU tests; out_size an int or (h, w)
SWITCHES = [(True, 128, False), (True, 112, True), (False, 128, True), (False, (112, 96), False), (True, 96, False)]


def out_hw(out_size, h, w):
    if out_size is None:
        return h, w
    if isinstance(out_size, int):
        return out_size, out_size
    return int(out_size[0]), int(out_size[1])


def rgb_to_l(rgb):
    """PIL convert('L') of an RGB uint8 array (..., 3): ITU-R 601-2 luma in 16-bit fixed point, rounded."""
    a = rgb.astype(np.uint32)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def bilinear_coeffs(insz, outsz):
    """precompute_coeffs + normalize_coeffs_8bpc of Pillow's Resample.c for the triangle filter (support 1):
    [(first tap, taps, [22-bit fixed-point coefficients])] per output coordinate."""
    scale = insz / outsz
    fscale = max(scale, 1.0)
    support = 1.0 * fscale
    ss = 1.0 / fscale
    rows = []
    for xx in range(outsz):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        cnt = min(int(center + support + 0.5), insz) - xmin
        k = []
        for x in range(cnt):
            v = abs((x + xmin - center + 0.5) * ss)
            k.append(1.0 - v if v < 1.0 else 0.0)
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        rows.append((xmin, cnt, [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in k]))
    return rows


def _pass(a, axis, outsz):
    a = np.moveaxis(a, axis, 0)
    if a.shape[0] == outsz:                        # ImagingResample: an axis that keeps its size is skipped
        return np.moveaxis(a, 0, axis)
    out = np.empty((outsz,) + a.shape[1:], np.uint8)
    for xx, (xmin, cnt, k) in enumerate(bilinear_coeffs(a.shape[0], outsz)):
        acc = np.full(a.shape[1:], 1 << 21, np.int64)
        for j in range(cnt):
            acc += a[xmin + j].astype(np.int64) * k[j]
        out[xx] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize_bilinear(a, oh, ow):
    """Image.fromarray(a).resize((ow, oh), Image.BILINEAR) for a uint8 (h, w) or (h, w, c) array: horizontal pass,
    uint8 intermediate, vertical pass."""
    return _pass(_pass(a, 1, ow), 0, oh)


def draw(seed, offset, n, h, w, mode, lo=0, hi=36, flip=True, sets=(), out_size=None):
    """oracle.occ.draw with the light centre drawn over the output size (words 9, 10; same draw indices)."""
    desc = oo.draw(seed, offset, n, h, w, mode, lo, hi, flip, sets=sets)
    oh, ow = out_hw(out_size, h, w)
    for i in range(n):
        c = np.array([f32(ow) * oo.unif(oo.u32(seed, offset + i, 9)), f32(oh) * oo.unif(oo.u32(seed, offset + i, 10))], f32)
        desc[i, 9:11] = c.view(np.int32)
    return desc


def occlude(face, d, sets=()):
    """The occluded uint8 face (h, w, 3) and the 0 (occluded) / 255 'L' mask at the source size, with oracle.occ."""
    h, w, _ = face.shape
    pix = face.copy()
    occ = oo.inside(d, h, w)
    if d[0] >= oo.OCC_GLASSES:
        occ = oo.paste(pix, d, sets)
    elif d[0] == oo.OCC_BLOCK:
        pix[occ] = 0
    elif d[0] != oo.OCC_NONE:
        pix[occ] = d[5:8].astype(np.uint8)
    return pix, np.where(occ, 0, 255).astype(np.uint8)


def stages_u8(face, d, sets, gray, oh, ow):
    """(face, mask, clean) as uint8 after occlusion, convert('L'), resize and flip: (oh, ow, C), (oh, ow), (oh, ow, C)."""
    pix, m = occlude(face, d, sets)
    clean = face
    if gray:
        pix, clean = rgb_to_l(pix)[..., None], rgb_to_l(clean)[..., None]
    pix, m, clean = resize_bilinear(pix, oh, ow), resize_bilinear(m, oh, ow), resize_bilinear(clean, oh, ow)
    if d[8]:
        pix, m, clean = pix[:, ::-1], m[:, ::-1], clean[:, ::-1]
    return pix, m, clean


def apply(src, desc, light=True, want_ori=True, sets=(), gray=False, out_size=None, use_norm=True):
    """src: (n, h, w, 3) uint8 -> img (n, C, oh, ow) f32, msk (n, oh, ow) int64, ori (n, C, oh, ow) f32 or None."""
    n, h, w, _ = src.shape
    oh, ow = out_hw(out_size, h, w)
    ch = 1 if gray else 3
    img = np.empty((n, ch, oh, ow), f32)
    ori = np.empty((n, ch, oh, ow), f32) if want_ori else None
    msk = np.empty((n, oh, ow), np.int64)
    for i in range(n):
        d = desc[i]
        pix, m, clean = stages_u8(src[i], d, sets, gray, oh, ow)
        t = pix.astype(f32) / f32(255.0)           # ToTensor
        if light:
            t = t * oo.light_map(d, oh, ow)[:, :, None]
            t = t / t.max()
        c = clean.astype(f32) / f32(255.0)
        if use_norm:
            t, c = (t - f32(0.5)) / f32(0.5), (c - f32(0.5)) / f32(0.5)
        img[i] = t.transpose(2, 0, 1)
        if want_ori:
            ori[i] = c.transpose(2, 0, 1)
        msk[i] = np.where(m != 255, 0, 1)
    return img, msk, ori


def synthetic_sets(seed=3):
    """Stand-ins for the reference's occluder folders, in the shapes its constructors preload (two glasses folders
    80 x 40, scarves 90 x 90, objects 55 x 55) with transparent, faint (alpha <= 10), translucent and opaque regions."""
    rng = np.random.default_rng(seed)

    def entries(num, h, w):
        a = rng.integers(0, 256, (num, h, w, 4), dtype=np.uint8)
        u = rng.random((num, h, w))
        a[..., 3] = np.where(u < 0.35, 0, np.where(u < 0.45, rng.integers(1, 11, (num, h, w)), a[..., 3]))
        a[:, h // 4:h // 2, w // 4:w // 2, 3] = 255
        return a
    return [("glasses", entries(5, 40, 80)), ("glasses", entries(3, 40, 80)), ("scarf", entries(4, 90, 90)),
            ("object", entries(6, 55, 55))]


def oracle_sets(sets):
    return [(oo.KIND_OF[k], a) for k, a in sets]
