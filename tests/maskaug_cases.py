"""Shared by tests/test_maskaug_cpu.py and tests/test_gpu_maskaug.py: the numpy restatement of the facial-mask branch of
the device input pipeline (msml_occ_draw_mask / msml_occ_apply_mask, msml_amd/csrc/occ.hip).

What the reference does for a mask sample (FaceByRandOccMask.__getitem__ with mask_flag, datasets/load_dataset.py:
113-139,167-177, and _add_gauss_to_mask :203-280 with _get_gauss :282-339), in its order:
  rendered face -> convert('L') when gray -> Resize -> flip -> ToTensor, light, / max       (occ_gray_cases, unchanged)
  mask plane    -> Resize -> flip -> value <= 128 ? 0 : 255; the returned mask is // 255     binarise
  the float16 offset on the mask pixels inside the rectangle                                 offset_map, mask_light
  face - offset in f32, not clamped                                                          add_gauss_to_mask
  Normalize only with use_norm
Every function takes the random draws as ARGUMENTS (a dict, see draws_from_log / draws_from_desc), so the same code is
checked bit for bit against the reference's own run (tests/golden/g12_maskaug.npz, tools/make_golden_maskaug.py) and
then serves as the reference of the device, whose draws come from its descriptors.
"""
import numpy as np

from oracle import occ as oo
from tests import occ_gray_cases as G

f16, f32 = np.float16, np.float32
OCC_MASK = 8
LIGHT, NOISE, BLOCK = 0, 1, 2
# draw indices of msml_occ_draw_mask (0-13 and 16-45 belong to the occluders)
K_FLAG, K_TYPE, K_LX, K_RX, K_LY, K_RY, K_SIGN, K_CX, K_CY, K_RAD, K_JIT = 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56
NOISE_DOMAIN = 0x6D61736B
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------ _add_gauss_to_mask with the draws as arguments
def type_of(trans_type):
    """:233,:244: >= 7 Gaussian light, 5-6 Gaussian noise, <= 4 block."""
    return LIGHT if trans_type >= 7 else (NOISE if trans_type >= 5 else BLOCK)


def binarise(m_u8):
    """:210-212: the resized mask, <= 128 -> 0 (occluded), else 255."""
    return np.where(m_u8 <= 128, 0, 255).astype(np.uint8)


def gauss_patch(dr):
    """_get_gauss(lx, ly, rx, ry, (), ()) and :238, as an f32 (ry - ly, rx - lx) array: relative coordinate minus absolute
    centre in f64, truncated through int16; int16 squares; f32 distance; exp(-0.5 d^2 / f32(r^2)) in f32."""
    rw, rh = dr["rx"] - dr["lx"], dr["ry"] - dr["ly"]
    ix = (np.arange(rw) - float(dr["cx"])).astype(np.int16)
    iy = (np.arange(rh) - float(dr["cy"])).astype(np.int16)
    dist = np.sqrt((ix[None, :] ** 2 + iy[:, None] ** 2).astype(f32))
    g = np.exp(f32(-0.5) * (dist * dist) / f32(float(dr["radius"]) ** 2))
    return (g - f32(0.5)) * f32(2) * f32(0.4) * f32(dr["sign"])


def offset_map(dr, h, w, step=0):
    """rescale_map (:226, :240, :245) or block_map (:253-255): float16 (h, w), zero outside the rectangle.  step = -1 / +1
    moves every light / noise value one float16 step down / up (the envelope of the GPU test)."""
    m = np.zeros((h, w), f16)
    if dr["type"] == LIGHT:
        patch = gauss_patch(dr).astype(f16)
    elif dr["type"] == NOISE:
        patch = np.asarray(dr["noise"]).astype(f16)
    else:
        patch = np.full((dr["ry"] - dr["ly"], dr["rx"] - dr["lx"]), dr["sign"], f16)
    if step and dr["type"] != BLOCK:
        patch = np.nextafter(patch, f16(np.inf * step))
    m[dr["ly"]:dr["ry"], dr["lx"]:dr["rx"]] = patch
    return m


def mask_light(dr, bin_u8, gray, step=0):
    """msk_light of :229-268: float16 (3, h, w), or (h, w) when gray."""
    h, w = bin_u8.shape
    one = (bin_u8 == 0).astype(f16)                     # :230: 1 on the mask, 0 on the face
    m = offset_map(dr, h, w, step)
    l = np.zeros((3, h, w), f16)
    for c in range(3):
        if dr["type"] == BLOCK or dr["jitter"][c]:      # :256 no jitter on the block; :261
            l[c] = one * m
    if gray:                                            # :265-267, every operation rounded to float16
        l = (f16(0.2989) * l[0] + f16(0.5870) * l[1] + f16(0.1140) * l[2]) / f16(3)
    return l


def add_gauss_to_mask(face, m_u8, gray, dr, step=0):
    """face: f32 (C, h, w) after _add_gauss_to_face; m_u8: the resized, flipped mask plane.  -> (face - msk_light in f32,
    int32 (h, w) mask 0 occluded / 1 clean)."""
    b = binarise(m_u8)
    l = mask_light(dr, b, gray, step)
    return face - l.astype(f32), (b // 255).astype(np.int32)


def draws_from_log(names, vals, randn=None):
    """The reference's own draws, logged in order by tools/make_golden_maskaug.py, as the dict the functions above take."""
    it = iter(zip([str(n) for n in names], [float(v) for v in vals]))

    def take(kind):
        n, v = next(it)
        assert n == kind, (n, kind)
        return v
    tt = int(take("randint"))
    dr = {"type": type_of(tt), "ly": 1, "ry": 111, "sign": 1, "jitter": (1, 1, 1)}
    dr["lx"] = 40 + int(take("randint"))
    dr["rx"] = 100 + int(take("randint"))
    if dr["type"] == LIGHT:
        dr["cx"] = dr["lx"] + (dr["rx"] - dr["lx"]) * take("random")
        dr["cy"] = dr["ly"] + (dr["ry"] - dr["ly"]) * take("random")
        dr["radius"] = take("uniform")
        dr["sign"] = int(take("randint")) * 2 - 1
    elif dr["type"] == NOISE:
        assert take("randn") == 0.0                    # the array itself travels beside the log
        dr["noise"] = randn
    else:
        dr["ly"] = 40 + int(take("randint"))
        dr["ry"] = 100 + int(take("randint"))
        dr["sign"] = int(take("randint")) * 2 - 1
    if dr["type"] != BLOCK:
        dr["jitter"] = tuple(int(take("randint")) for _ in range(3))
    assert next(it, None) is None
    return dr


# ------------------------------------------------------------------ the device's draws
def _mix(z):
    """splitmix64 on uint64 arrays (wrapping)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def noise_key(seed, img):
    """mix(mix(seed + 'mask') + image index): words 28 (low) and 29 (high) of a mask descriptor."""
    with np.errstate(over="ignore"):
        return _mix(_mix(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + np.uint64(NOISE_DOMAIN)) + np.uint64(img))


def normals(key, xs, ys):
    """occ_mask_normal: the float16 standard normal of output pixels (xs, ys) under `key`.  r = mix(key + y * 65536 + x);
    Box-Muller in f32 from two 24-bit uniforms, u1 = ((r >> 40) + 1) / 2^24 in (0, 1], u2 = ((r >> 8) & 0xFFFFFF) / 2^24."""
    xs, ys = np.asarray(xs, np.uint64), np.asarray(ys, np.uint64)
    with np.errstate(over="ignore"):
        r = _mix(np.uint64(key) + ys * np.uint64(65536) + xs)
    u1 = ((r >> np.uint64(40)) + np.uint64(1)).astype(f32) * f32(1.0 / 16777216.0)
    u2 = ((r >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(f32) * f32(1.0 / 16777216.0)
    rad = np.sqrt(f32(-2.0) * np.log(u1))
    ang = f32(6.2831854820251465) * u2
    return (rad * np.cos(ang)).astype(f16)


def flagged(seed, img, p_mask):
    return p_mask > 0 and bool(oo.unif(oo.u32(seed, img, K_FLAG)) < f32(p_mask))


def mask_words(seed, img):
    """Words 16-29 of a mask descriptor (msml_occ_draw_mask), from draws 47-58."""
    ri = lambda k, a, b: oo.randint(oo.u32(seed, img, k), a, b)
    un = lambda k: oo.unif(oo.u32(seed, img, k))
    ty = type_of(ri(K_TYPE, 0, 11))
    lx, rx, ly, ry = 40 + ri(K_LX, -20, 21), 100 + ri(K_RX, -20, 11), 1, 111
    if ty == BLOCK:
        ly, ry = 40 + ri(K_LY, -20, 20), 100 + ri(K_RY, -20, 10)
    rw, rh = rx - lx, ry - ly
    edge = max(rw, rh)
    rlo, rhi = int(edge / 1.5), int(edge * 1.5)
    fl = np.array([f32(lx) + f32(f32(rw) * un(K_CX)), f32(ly) + f32(f32(rh) * un(K_CY)),
                   f32(rlo) + f32(f32(rhi - rlo) * un(K_RAD))], f32)
    key = int(noise_key(seed, img))
    w = np.zeros(14, np.int64)
    w[:9] = [ty, lx, ly, rx, ry, ri(K_SIGN, 0, 2) * 2 - 1] + [ri(K_JIT + c, 0, 2) for c in range(3)]
    w[9:12] = fl.view(np.int32)
    w[12:14] = [key & 0xFFFFFFFF, key >> 32]
    return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def draw(seed, offset, n, h, w, mode, lo=0, hi=36, flip=True, sets=(), out_size=None, p_mask=0.0):
    """msml_occ_draw_mask: occ_gray_cases.draw for the samples that are not flagged; a flagged one keeps flip and light
    (words 8-11), has kind 8, zeros in words 1-7 and 12-15, and the mask's words from 16 on."""
    desc = G.draw(seed, offset, n, h, w, mode, lo, hi, flip, sets=sets, out_size=out_size)
    for i in range(n):
        if flagged(seed, offset + i, p_mask):
            keep = desc[i, 8:12].copy()
            desc[i] = 0
            desc[i, 0] = OCC_MASK
            desc[i, 8:12] = keep
            desc[i, 16:30] = mask_words(seed, offset + i)
    return desc


def draws_from_desc(d):
    """The dict of the functions above from a mask descriptor; the noise is regenerated from the key of words 28-29."""
    fl = d[25:28].view(f32)
    dr = {"type": int(d[16]), "lx": int(d[17]), "ly": int(d[18]), "rx": int(d[19]), "ry": int(d[20]), "sign": int(d[21]),
          "jitter": tuple(int(v) for v in d[22:25]), "cx": fl[0], "cy": fl[1], "radius": fl[2]}
    if dr["type"] == NOISE:
        key = (int(d[29]) & 0xFFFFFFFF) << 32 | (int(d[28]) & 0xFFFFFFFF)
        ys, xs = np.mgrid[dr["ly"]:dr["ry"], dr["lx"]:dr["rx"]]
        dr["noise"] = normals(key, xs, ys)
    return dr


def mask_sample(masked, mask, d, light, gray, oh, ow, use_norm, steps=(0,)):
    """One mask sample of the device: masked (h, w, 3) uint8, mask (h, w) uint8, d its descriptor -> [img (C, oh, ow) f32
    for every step of `steps`], msk (oh, ow) int64."""
    pix = G.rgb_to_l(masked)[..., None] if gray else masked
    pix, m = G.resize_bilinear(pix, oh, ow), G.resize_bilinear(mask, oh, ow)
    if d[8]:
        pix, m = pix[:, ::-1], m[:, ::-1]
    t = pix.astype(f32) / f32(255.0)
    if light:
        t = t * oo.light_map(d, oh, ow)[:, :, None]
        t = t / t.max()
    face, dr, outs = np.ascontiguousarray(t.transpose(2, 0, 1)), draws_from_desc(d), []
    for step in steps:
        out, om = add_gauss_to_mask(face, m, gray, dr, step)
        outs.append((out - f32(0.5)) / f32(0.5) if use_norm else out)
    return outs, om.astype(np.int64)


def apply(src, masked, mask, desc, light=True, sets=(), gray=False, out_size=None, use_norm=True, rows=None, steps=(0,)):
    """The whole batch: occ_gray_cases.apply, then the mask samples whose row exists rewritten (a mask sample without a
    render is the clean sample).  -> ([img for every step of `steps`], msk, ori); steps (0, -1, 1) gives the restatement
    and its float16 envelope."""
    n, h, w, _ = src.shape
    oh, ow = G.out_hw(out_size, h, w)
    is_mask = desc[:, 0] == OCC_MASK
    plain = desc.copy()
    plain[is_mask, 0] = oo.OCC_NONE
    img, msk, ori = G.apply(src, plain, light, True, sets, gray, out_size, use_norm)
    imgs = [img.copy() for _ in steps]
    for i in np.nonzero(is_mask)[0]:
        r = i if rows is None else int(rows[i])
        if 0 <= r < masked.shape[0]:
            outs, msk[i] = mask_sample(masked[r], mask[r], desc[i], light, gray, oh, ow, use_norm, steps)
            for dst, out in zip(imgs, outs):
                dst[i] = out
    return imgs, msk, ori


def synthetic_renders(src, seed=5):
    """Stand-ins for mask_out.rec / mask.rec of the faces `src` (n, h, w, 3): the lower face recoloured, and a mask plane
    with a ramp through 128 along the edge."""
    rng = np.random.RandomState(seed)
    n, h, w, _ = src.shape
    top = rng.randint(h // 2, h // 2 + h // 8, (n, 1, 1))
    left = rng.randint(w // 6, w // 4, (n, 1, 1))
    y, x = np.arange(h).reshape(1, h, 1), np.arange(w).reshape(1, 1, w)
    depth = np.minimum(np.minimum(y - top, (h - 6) - y), np.minimum(x - left, (w - left) - x))
    alpha = np.clip(depth / 3.0, 0.0, 1.0)
    colour = rng.randint(0, 256, (n, 1, 1, 3))
    masked = np.rint(src * (1 - alpha[..., None]) + colour * alpha[..., None]).astype(np.uint8)
    mask = np.rint(255.0 * (1 - alpha)).astype(np.uint8)
    return masked, mask


# (seed, offset, n) of the GPU tests; tests/test_maskaug_cpu.py asserts that with p_mask = 1 they cover the three types,
# both signs of light and of block, a jitter pattern of all zeros and one with a channel kept
GPU_DRAWS = (1234, 5000, 32)


def coverage(seed, offset, n):
    """{(type, sign)} of light and block, and the jitter patterns of light / noise, over n mask samples."""
    signs, jit, types = set(), set(), set()
    for i in range(n):
        w = mask_words(seed, offset + i)
        types.add(int(w[0]))
        if w[0] != NOISE:
            signs.add((int(w[0]), int(w[5])))
        if w[0] != BLOCK:
            jit.add(tuple(int(v) for v in w[6:9]))
    return types, signs, jit
