"""Device input pipeline: H2D double buffering with DataLoaderX semantics and
occlusion synthesis / flip / Gaussian light / normalisation on the GPU (csrc/occ.hip).

At 7 000 images/s per GPU (56 000 on a node) the reference's per-sample PIL / OpenCV augmentation
(FaceByRandOccMask.__getitem__, datasets/load_dataset.py:101-139; 32 workers, config.py:29) is the next
bottleneck: here the host only hands over decoded uint8 faces (37.6 KB per image, 9.6 MB per batch of
256 -- 0.15 ms of PCIe Gen5) and labels; everything else runs on the device in two kernels per batch.

* `augment(src_u8, seed, offset, mode)`   -- (img, msk, ori) from a uint8 batch already on the device.
* `DeviceLoaderX(source, device, ...)`    -- datasets/dataloaderx.py:40-66 semantics: a background thread
  pulls host batches, the next batch is copied on a side stream from pinned memory and augmented there
  while the current step runs, `__next__` makes the compute stream wait for that stream.
* `gray=True, out_size=128, use_norm=False` on `augment` / `DeviceLoaderX` -- the reference's is_gray / out_size /
  use_norm switches (load_dataset.py:86-139,179; the LightCNN recipe, config.py:99-102): occlusion at the source size,
  convert('L'), bilinear Resize of face, mask and clean face, flip, light at the output size, no Normalize -- one
  kernel, bit for bit in the integer part (msml_occ_apply_out).
* `p_mask=0.2` on `draw` / `augment` / `DeviceLoaderX` with `masked=`, `mask=` (and `rows=`) -- the facial-mask branch of
  the mix (load_dataset.py:113,167-177 and _add_gauss_to_mask :203-280): flagged samples take the caller's rendered face
  and mask plane through Resize, flip and light, binarise the mask at <= 128 and change the mask pixels by Gaussian
  light, Gaussian noise or a block (msml_occ_draw_mask + the overlay msml_occ_apply_mask).  `mask_flags` is the same
  draw on the host, for the record reader.  With p_mask = 0 (the default) nothing is launched that was not before.
* `SynthFaceSource`                        -- stand-in for the record reader: a pool of random uint8 faces in
  pinned host memory (no dataset travels with this repo).
"""
import queue
import threading

import torch

from ._lib import call
from .jpeg import JpegBatch

# "train": the asset-free mix {rect, ellipse, polygon, none}; "ms1m" / "casia": the reference's full mixes with the
# texture occluders (load_dataset.py:155-163), which need an OccluderAtlas; "glasses" / "scarf" / "object": one class.
MODES = {"train": 0, "rect": 1, "block": 2, "none": 3, "polygon": 4, "ms1m": 5, "casia": 6, "glasses": 7, "scarf": 8,
         "object": 9}
DESC_WORDS = 64
KINDS = {"glasses": 5, "scarf": 6, "object": 7}
META_WORDS, RT_WORDS = 16, 10


def resample_table(insz, outsz, filter="bicubic"):
    """Pillow's resampling coefficients for one axis (resample.pillow_coeffs) as csrc/occ.hip reads them: int32
    [outsz][10] = first tap, taps, up to 8 coefficients in 22-bit fixed point.  "bicubic" is what Image.resize -- the
    call of rand_occ.py:375,466,562 -- uses by default; "bilinear" (the triangle filter, support 1) is
    transforms.Resize on a PIL image (load_dataset.py:117-120)."""
    import numpy as np
    from .resample import pillow_coeffs
    xmin, cnt, fixed = pillow_coeffs(insz, outsz, filter)
    if fixed.shape[1] > RT_WORDS - 2:
        raise ValueError("resample_table: %d -> %d needs %d taps (at most %d)"
                         % (insz, outsz, cnt[np.argmax(cnt > RT_WORDS - 2)], RT_WORDS - 2))
    tab = np.zeros((outsz, RT_WORDS), np.int32)
    tab[:, 0], tab[:, 1], tab[:, 2:2 + fixed.shape[1]] = xmin, cnt, fixed
    return tab


class OccluderAtlas:
    """Texture occluders on the device.  sets: [(kind, rgba)], kind in {'glasses', 'scarf', 'object'}, rgba a uint8
    array / tensor [num, h0, w0, 4] preloaded as the reference's constructors do (load_occluder_sets reads the
    reference's folders).  Holds the atlas bytes, the set table and the resampling tables for every size a sample
    can draw at image size `size` (rand_occ.py:371-374, 464-465, 560-561)."""

    def __init__(self, sets, size=112, device="cuda"):
        import numpy as np
        if not 1 <= len(sets) <= 16:
            raise ValueError("OccluderAtlas: 1..16 occluder sets")
        self.size = size
        blobs, meta, dirs, tabs = [], np.zeros((len(sets), META_WORDS), np.int32), [], []
        off, rt_off, self.patch_bytes, self.lds_bytes = 0, 0, 0, 0
        cache = {}

        def table_dir(insz, lo, hi):
            nonlocal rt_off
            base = len(dirs)
            for out in range(lo, hi + 1):
                key = (insz, out)
                if key not in cache:
                    cache[key] = rt_off
                    tabs.append(resample_table(insz, out).reshape(-1))
                    rt_off += out * RT_WORDS
                dirs.append(cache[key])
            return base
        for i, (kind, rgba) in enumerate(sets):
            a = np.ascontiguousarray(rgba.cpu().numpy() if torch.is_tensor(rgba) else rgba, dtype=np.uint8)
            if a.ndim != 4 or a.shape[3] != 4 or a.shape[0] < 1:
                raise ValueError("OccluderAtlas: set %d must be [num, h0, w0, 4] uint8" % i)
            num, h0, w0, _ = a.shape
            k = KINDS[kind]
            if k == 5:                                   # the glasses scale with the image (rand_occ.py:371-372)
                bw, bh, lo, hi = size * (w0 / 120.0), size * (h0 / 120.0), 1 / 1.1, 1.1
            elif k == 6:
                bw, bh, lo, hi = float(w0), float(h0), 1 / 1.1, 1.0
            else:
                bw, bh, lo, hi = float(w0), float(h0), 1.0, 2.0
            wmin, wmax = max(int(bw * lo) - 1, 1), int(bw * hi) + 1
            hmin, hmax = max(int(bh * lo) - 1, 1), int(bh * hi) + 1
            meta[i, :11] = [off, num, h0, w0, k, wmin, wmax, hmin, hmax, table_dir(w0, wmin, wmax),
                            table_dir(h0, hmin, hmax)]
            blobs.append(a.reshape(-1))
            off += a.size
            self.patch_bytes = max(self.patch_bytes, hmax * wmax * 4, h0 * w0 * 4)
            self.lds_bytes = max(self.lds_bytes, (h0 * w0 + h0 * wmax) * 4)
        if self.lds_bytes > 160 * 1024:
            raise ValueError("OccluderAtlas: an occluder set needs %d bytes of LDS (160 KB available)" % self.lds_bytes)
        self.nsets = len(sets)
        self.atlas = torch.from_numpy(np.concatenate(blobs)).to(device)
        self.meta = torch.from_numpy(meta).to(device)
        self.dir = torch.tensor(dirs, dtype=torch.int32, device=device)
        self.rtab = torch.from_numpy(np.concatenate(tabs)).to(device)


def load_occluder_sets(root):
    """Preload the reference's occluder folders at run time, from the USER's checkout (nothing is copied into this
    package): `root` = <reference>/datasets/augment/occluder.  Same order and arithmetic as the training mix of
    datasets/load_dataset.py:72-85: RandomGlassesList(glasses_crop, eleglasses_crop) with RandomGlasses.__init__
    (rand_occ.py:345-366: RGBA, resize to 80 x 40), RandomScarf (:441-462: 90 x 90), RandomRealObject (:531-556:
    rescale by max(w / 55, h / 55), centre crop to 55 x 55)."""
    import os
    import numpy as np
    from PIL import Image

    def folder(name, fn):
        d = os.path.join(root, name)
        return np.stack([fn(Image.open(os.path.join(d, f)).convert("RGBA")) for f in os.listdir(d)])

    def fixed(w, h):
        return lambda im: np.array(im.resize((w, h)), dtype=np.uint8)

    def center_crop(im, w=55, h=55):
        fw, fh = im.size
        ratio = max(fw / w, fh / h)
        im = im.resize((int(fw / ratio), int(fh / ratio)))
        # torchvision CenterCrop((55, 55)): pad evenly with zeros when smaller, then crop around the centre
        iw, ih = im.size
        if iw < w or ih < h:
            pl, pt = (w - iw) // 2 if iw < w else 0, (h - ih) // 2 if ih < h else 0
            canvas = Image.new("RGBA", (max(w, iw), max(h, ih)), (0, 0, 0, 0))
            canvas.paste(im, (pl, pt))
            im = canvas
            iw, ih = im.size
        top, left = int(round((ih - h) / 2.0)), int(round((iw - w) / 2.0))
        return np.array(im.crop((left, top, left + w, top + h)), dtype=np.uint8)

    return [("glasses", folder("glasses_crop", fixed(80, 40))), ("glasses", folder("eleglasses_crop", fixed(80, 40))),
            ("scarf", folder("scarf_crop", fixed(90, 90))), ("object", folder("object_train", center_crop))]


def _out_hw(out_size, h, w):
    """out_size as transforms.Resize takes it here: None (the source size), an int (square) or (h, w)."""
    if out_size is None:
        return h, w
    if isinstance(out_size, int):
        return out_size, out_size
    oh, ow = out_size
    return int(oh), int(ow)


_OUT_TABLES = {}      # (device, source size, output size) -> the bilinear table of that axis on the device


def _out_table(insz, outsz, device):
    if insz == outsz:
        return None                                  # ImagingResample skips an axis that keeps its size
    key = (str(device), insz, outsz)
    if key not in _OUT_TABLES:
        _OUT_TABLES[key] = torch.from_numpy(resample_table(insz, outsz, "bilinear")).to(device)
    return _OUT_TABLES[key]


_M64 = (1 << 64) - 1
MASK_FLAG_DRAW = 46       # the draw index of the mask flag (csrc/occ.hip: 0-13 and 16-45 belong to the occluders)
MASK_MIN_HW = (111, 110)  # the reference's rectangle (y < 111, x < 110) is in output pixels and is not scaled


def _mix(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def mask_flags(seed, offset, n, p_mask):
    """Which of the images offset .. offset + n - 1 are facial-mask samples under `seed`: bool [n], the draw of
    msml_occ_draw_mask on the host (occ_unif(occ_u32(seed, image, 46)) < p_mask in f32).  A record reader fetches the
    mask_out / mask records of these indices only and builds `rows` from them."""
    import numpy as np
    out = np.zeros(n, bool)
    if p_mask <= 0:
        return out
    base = _mix(int(seed) & _M64)
    pm = np.float32(p_mask)
    for i in range(n):
        u = (_mix((base + (int(offset) + i) * 64 + MASK_FLAG_DRAW) & _M64) >> 32) & 0xFFFFFFFF
        out[i] = np.float32(u >> 8) * np.float32(1.0 / 16777216.0) < pm
    return out


def _check_mask_args(p_mask, masked, mask, rows, n, h, w, oh, ow):
    """The host-side refusals of the facial-mask branch, before any launch."""
    if not 0.0 <= p_mask <= 1.0:
        raise ValueError("p_mask = %r is not a probability" % (p_mask,))
    if (masked is None) != (mask is None):
        raise ValueError("masked and mask come together")
    if p_mask > 0 and masked is None:
        raise ValueError("p_mask > 0 needs the rendered faces (masked) and their masks (mask)")
    if p_mask > 0 and (oh < MASK_MIN_HW[0] or ow < MASK_MIN_HW[1]):
        raise ValueError("the facial-mask branch needs an output of at least %d x %d (got %d x %d): the reference's "
                         "rectangle is not scaled with the size" % (MASK_MIN_HW + (oh, ow)))
    if masked is None:
        return
    m = masked.shape[0]
    if masked.dtype != torch.uint8 or tuple(masked.shape) != (m, h, w, 3):
        raise ValueError("masked must be uint8 [M, %d, %d, 3], got %s %s" % (h, w, masked.dtype, tuple(masked.shape)))
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (m, h, w):
        raise ValueError("mask must be uint8 [%d, %d, %d], got %s %s" % (m, h, w, mask.dtype, tuple(mask.shape)))
    if rows is None:
        if m != n:
            raise ValueError("without rows, masked / mask hold one render per sample (%d), got %d" % (n, m))
    elif rows.dtype != torch.int32 or tuple(rows.shape) != (n,):
        raise ValueError("rows must be int32 [%d], got %s %s" % (n, rows.dtype, tuple(rows.shape)))


def draw(n, seed, offset, mode="train", lo=0, hi=36, flip=True, size=112, device="cuda", atlas=None, out_size=None,
         p_mask=0.0):
    """Per-image occlusion / flip / light descriptors (msml_occ_draw[_tex]), int32 [n, 64] on the device.  out_size:
    the size the light is added at (msml_occ_draw_out: the light centre is uniform over the OUTPUT image).  p_mask > 0:
    msml_occ_draw_mask -- an image is a facial-mask sample (kind 8) with that probability (the reference: 0.2)."""
    if p_mask > 0:
        oh, ow = _out_hw(out_size, size, size)
        if p_mask > 1.0:
            raise ValueError("p_mask = %r is not a probability" % (p_mask,))
        if oh < MASK_MIN_HW[0] or ow < MASK_MIN_HW[1]:
            raise ValueError("the facial-mask branch needs an output of at least %d x %d (got %d x %d)"
                             % (MASK_MIN_HW + (oh, ow)))
    desc = torch.empty(n, DESC_WORDS, dtype=torch.int32, device=device)
    if MODES[mode] >= 5:
        if atlas is None:
            raise ValueError("mode %r needs an OccluderAtlas (texture occluders come from the caller's assets)" % mode)
        if atlas.size != size:
            raise ValueError("OccluderAtlas was built for %d-pixel images" % atlas.size)
    if p_mask > 0:
        tex = MODES[mode] >= 5
        call("msml_occ_draw_mask", int(seed), int(offset), n, size, size, oh, ow, MODES[mode], lo, hi, int(flip),
             atlas.meta if tex else None, atlas.nsets if tex else 0, float(p_mask), desc)
    elif out_size is not None:
        oh, ow = _out_hw(out_size, size, size)
        tex = MODES[mode] >= 5
        call("msml_occ_draw_out", int(seed), int(offset), n, size, size, oh, ow, MODES[mode], lo, hi, int(flip),
             atlas.meta if tex else None, atlas.nsets if tex else 0, desc)
    elif MODES[mode] >= 5:
        call("msml_occ_draw_tex", int(seed), int(offset), n, size, size, MODES[mode], lo, hi, int(flip), atlas.meta,
             atlas.nsets, desc)
    else:
        call("msml_occ_draw", int(seed), int(offset), n, size, size, MODES[mode], lo, hi, int(flip), desc)
    return desc


def apply(src, desc, light=True, want_ori=True, atlas=None, gray=False, out_size=None, use_norm=True, masked=None,
          mask=None, rows=None):
    """src: (N, H, W, 3) uint8 on the device -> img (N,3,H,W) f32, msk (N,H,W) int64, ori or None.  atlas: the
    OccluderAtlas the descriptors were drawn with (texture kinds are resampled per sample, then pasted).
    gray / out_size / use_norm: the reference's is_gray / out_size / use_norm (msml_occ_apply_out) -- img and ori
    (N, 1 or 3, oh, ow), in [0, 1] without the normalisation, msk (N, oh, ow); desc drawn with the same out_size.
    masked (M, H, W, 3) uint8, mask (M, H, W) uint8 (any gray value; <= 128 after the resize is the mask), rows int32
    (N) or None (M == N): the renders of the facial-mask samples (kind 8 of draw(..., p_mask=...)); sample n takes row
    rows[n], and a row outside 0 .. M - 1 leaves it the clean sample (msml_occ_apply_mask, an overlay on img and msk)."""
    n, h, w, c = src.shape
    assert c == 3 and src.dtype == torch.uint8 and src.is_cuda and src.is_contiguous()
    oh, ow = _out_hw(out_size, h, w)
    if masked is not None or mask is not None:
        _check_mask_args(1.0, masked, mask, rows, n, h, w, oh, ow)      # (the overlay may run: the size check applies)
        assert masked.is_cuda and mask.is_cuda and masked.is_contiguous() and mask.is_contiguous()
        assert rows is None or (rows.is_cuda and rows.is_contiguous())
    out_form = gray or out_size is not None or not use_norm
    if out_form:
        ch = 1 if gray else 3
        img = torch.empty(n, ch, oh, ow, dtype=torch.float32, device=src.device)
        ori = torch.empty(n, ch, oh, ow, dtype=torch.float32, device=src.device) if want_ori else None
        msk = torch.empty(n, oh, ow, dtype=torch.int64, device=src.device)
        patch, stride = None, 0
        if atlas is not None:
            patch, stride = torch.empty(n, atlas.patch_bytes, dtype=torch.uint8, device=src.device), atlas.patch_bytes
            call("msml_occ_resize", atlas.atlas, atlas.meta, atlas.dir, atlas.rtab, desc, patch, stride, n,
                 atlas.lds_bytes)
        call("msml_occ_apply_out", src, desc, patch, stride, _out_table(w, ow, src.device),
             _out_table(h, oh, src.device), img, msk, ori, n, h, w, oh, ow, int(gray), int(use_norm), int(light))
    else:
        img = torch.empty(n, 3, h, w, dtype=torch.float32, device=src.device)
        ori = torch.empty(n, 3, h, w, dtype=torch.float32, device=src.device) if want_ori else None
        msk = torch.empty(n, h, w, dtype=torch.int64, device=src.device)
        if atlas is not None:
            patch = torch.empty(n, atlas.patch_bytes, dtype=torch.uint8, device=src.device)
            call("msml_occ_resize", atlas.atlas, atlas.meta, atlas.dir, atlas.rtab, desc, patch, atlas.patch_bytes, n,
                 atlas.lds_bytes)
            call("msml_occ_apply_tex", src, desc, patch, atlas.patch_bytes, img, msk, ori, n, h, w, int(light))
        else:
            call("msml_occ_apply", src, desc, img, msk, ori, n, h, w, int(light))
    if masked is not None:
        call("msml_occ_apply_mask", masked, mask, rows, masked.shape[0], desc, _out_table(w, ow, src.device),
             _out_table(h, oh, src.device), img, msk, n, h, w, oh, ow, int(gray), int(use_norm), int(light))
    return img, msk, ori


def augment(src, seed, offset, mode="train", lo=0, hi=36, flip=True, light=True, want_ori=True, atlas=None, gray=False,
            out_size=None, use_norm=True, p_mask=0.0, masked=None, mask=None, rows=None):
    """draw + apply.  p_mask > 0 needs masked / mask (and takes rows); with p_mask = 0 they are not looked at and the
    launches are those of a call without them."""
    n, h, w, _ = src.shape
    _check_mask_args(p_mask, masked, mask, rows, n, h, w, *_out_hw(out_size, h, w))
    if p_mask <= 0:
        masked = mask = rows = None
    desc = draw(n, seed, offset, mode, lo, hi, flip, h, src.device, atlas, out_size, p_mask)
    return apply(src, desc, light, want_ori, atlas if MODES[mode] >= 5 else None, gray, out_size, use_norm, masked, mask,
                 rows) + (desc,)


class SynthFaceSource:
    """Endless host-side source of (uint8 faces [B,112,112,3] in pinned memory, int64 labels [B]): `pool`
    distinct batches are generated once and cycled, as a record reader with a warm page cache would.
    masks=True: (faces, masked, mask, labels) -- stand-ins for the mask_out / mask records of every face: the lower face
    recoloured in one colour per sample, and a mask plane that is 0 there and 255 on the face with a three-pixel ramp
    between them, so that values on both sides of 128 meet the binarisation."""

    def __init__(self, batch, num_classes, steps=None, pool=4, seed=1, size=112, masks=False):
        self.batch, self.steps = batch, steps
        self.pool = []
        for i in range(pool):
            g = torch.Generator().manual_seed(seed + 977 * i)
            faces = torch.randint(0, 256, (batch, size, size, 3), generator=g, dtype=torch.uint8)
            labels = torch.randint(0, num_classes, (batch,), generator=g)
            item = (faces, labels)
            if masks:
                item = (faces,) + self._renders(faces, g) + (labels,)
            if torch.cuda.is_available():
                item = tuple(t.pin_memory() for t in item)
            self.pool.append(item)

    @staticmethod
    def _renders(faces, g):
        b, size = faces.shape[0], faces.shape[1]
        top = torch.randint(size // 2, size // 2 + size // 8, (b, 1, 1), generator=g).float()
        left = torch.randint(size // 6, size // 4, (b, 1, 1), generator=g).float()
        y = torch.arange(size).float().view(1, size, 1)
        x = torch.arange(size).float().view(1, 1, size)
        depth = torch.minimum(torch.minimum(y - top, (size - 6.0) - y), torch.minimum(x - left, (size - left) - x))
        alpha = (depth / 3.0).clamp(0.0, 1.0)                                  # 0 on the face, 1 well inside the mask
        colour = torch.randint(0, 256, (b, 1, 1, 3), generator=g).float()
        masked = (faces.float() * (1.0 - alpha[..., None]) + colour * alpha[..., None]).round().to(torch.uint8)
        mask = (255.0 * (1.0 - alpha)).round().to(torch.uint8)
        return masked.contiguous(), mask.contiguous()

    def __iter__(self):
        i = 0
        while self.steps is None or i < self.steps:
            yield self.pool[i % len(self.pool)]
            i += 1


class _Background(threading.Thread):
    """BackgroundGenerator of datasets/dataloaderx.py:12-37: a daemon thread fills a bounded queue."""

    def __init__(self, generator, device_index, max_prefetch=6):
        super().__init__(daemon=True)
        self.queue = queue.Queue(max_prefetch)
        self.generator = generator
        self.device_index = device_index
        self.start()

    def run(self):
        torch.cuda.set_device(self.device_index)
        for item in self.generator:
            self.queue.put(item)
        self.queue.put(None)

    def __next__(self):
        item = self.queue.get()
        if item is None:
            raise StopIteration
        return item


class DeviceLoaderX:
    """for img, msk, ori, label in DeviceLoaderX(source, local_rank, seed=...): ...

    Batch k+1 is copied (non_blocking, pinned -> HBM) and augmented on `self.stream` while the caller
    trains on batch k; `__next__` first makes the current stream wait for `self.stream`
    (dataloaderx.py:60-66).  The random draws of batch k are keyed by (seed, k * batch + image index):
    reproducible whatever the timing.

    p_mask > 0 (the reference: 0.2): the source yields (faces, masked, mask, label) or (faces, masked, mask, rows, label)
    -- the renders of the facial-mask samples, one per face or packed with rows[n] the render of face n (-1: none; see
    mask_flags) -- and they go over on the side stream with the faces.

    A source of compressed records (jpeg.RecordFaceSource) yields JpegBatch objects in place of the uint8 tensors; they
    are decoded on the side stream in front of augment, and after every `__next__` `self.jpeg_status` is the int32 [B]
    status tensor of the batch just returned (0 = decoded)."""

    def __init__(self, source, local_rank=0, seed=1, mode="train", lo=0, hi=36, flip=True, light=True,
                 want_ori=True, max_prefetch=6, atlas=None, gray=False, out_size=None, use_norm=True, p_mask=0.0):
        self.source, self.local_rank = source, local_rank
        self.stream = torch.cuda.Stream(local_rank)
        self.atlas = atlas                   # OccluderAtlas for the "ms1m" / "casia" mixes (texture occluders)
        self.cfg = (seed, mode, lo, hi, flip, light, want_ori)
        self.out = (gray, out_size, use_norm)   # the reference's is_gray / out_size / use_norm (LightCNN: True, 128, False)
        self.p_mask = p_mask
        self.jpeg_status = None              # JpegBatch sources: the status int32 [B] of the batch __next__ returned last
        self._status = None
        self.max_prefetch = max_prefetch
        self.count = 0
        self.batch = None

    def __iter__(self):
        self.iter = _Background(iter(self.source), self.local_rank, self.max_prefetch)
        self.count = 0
        self.preload()
        return self

    def preload(self):
        try:
            host = next(self.iter)
        except StopIteration:
            self.batch = None
            return
        seed, mode, lo, hi, flip, light, want_ori = self.cfg
        faces, label = host[0], host[-1]
        if self.p_mask > 0 and len(host) not in (4, 5):
            raise ValueError("p_mask > 0: the source must yield (faces, masked, mask[, rows], label)")
        status = None
        with torch.cuda.stream(self.stream):
            if isinstance(faces, JpegBatch):     # compressed records (jpeg.RecordFaceSource): decoded here, on the side stream
                src, extra, status = self._decode(host)
                lab = label.to(device=self.local_rank, non_blocking=True)
            else:
                src = faces.to(device=self.local_rank, non_blocking=True)
                lab = label.to(device=self.local_rank, non_blocking=True)
                extra = ()
                if self.p_mask > 0:              # masked, mask and, when the renders are packed, rows
                    extra = tuple(t.to(device=self.local_rank, non_blocking=True) for t in host[1:-1])
            img, msk, ori, _ = augment(src, seed, self.count * src.shape[0], mode, lo, hi, flip, light, want_ori,
                                       self.atlas, *self.out, self.p_mask, *extra)
        self.count += 1
        self.batch = (img, msk, ori, lab, src) + extra
        self._status = status                # of self.batch, and its last element: __next__ stream-records it with the rest
        if status is not None:
            self.batch += (status,)

    def _decode(self, host):
        """host: (JpegBatch, label) or (JpegBatch, JpegBatch of mask_out, JpegBatch of mask, rows, label) -> the faces
        uint8 [B, H, W, 3], (masked, mask, rows) or (), and the batch's status int32 [B] on the device: 0, or why
        face n -- or, where that is 0, the render rows[n] points at -- was not decoded (jpeg.STATUS).  A record the
        parser refused, face or render, is an error here, before anything is launched."""
        from . import jpeg
        faces = host[0]
        bad = faces.status.nonzero()[0]
        if bad.size:
            raise ValueError("DeviceLoaderX: record %d of the batch: %s" % (bad[0], faces.descriptors[bad[0]].reason))
        size = faces.sizes[0]
        dev = torch.device("cuda", self.local_rank)
        src, status = jpeg.decode_batch(faces, size=size, strict=False, device=dev)
        extra = ()
        if self.p_mask > 0:
            masked, mask, rst = jpeg.decode_renders(host[1], host[2], size, dev)
            rows = host[3].to(device=dev, non_blocking=True)
            extra = (masked, mask, rows)
            of_face = torch.where(rows >= 0, rst[rows.clamp(0, rst.shape[0] - 1).long()], torch.zeros_like(status))
            status = torch.where(status != 0, status, of_face)
        return src, extra, status

    def __next__(self):
        cur = torch.cuda.current_stream()
        cur.wait_stream(self.stream)
        batch = self.batch
        if batch is None:
            raise StopIteration
        for t in batch:                      # produced on the side stream, consumed on this one
            if t is not None:
                t.record_stream(cur)
        # the status of THIS batch (0 = decoded; see _decode), ordered on the current stream like its images; reading
        # it on the host is the caller's synchronisation, the loader makes none
        self.jpeg_status = self._status
        self.preload()
        return batch[:4]
