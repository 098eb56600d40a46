"""Write tests/golden/g19_png_enc.npz: the SOURCE arrays of the PNG encoder's tests (there are no expected bytes: the
files are checked by reading them back).  The four 112 x 112 faces decoded from g15_jpeg.npz's streams with Pillow (convert('RGB'); the fourth is a gray stream), the
decoded arrays of g17_png.npz's 8-bit gray / RGB / RGBA streams in their own mode, and the synthetic shapes of
tests/png_enc_cases.py."""
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from msml_amd import png                     # noqa: E402
from tests import png_cases, png_enc_cases   # noqa: E402


def main():
    out = {}
    z = np.load(os.path.join(ROOT, "tests", "golden", "g15_jpeg.npz"), allow_pickle=False)
    offs, faces = z["stream_offsets"], 0
    for i, name in enumerate(str(s) for s in z["names"]):
        if faces < 4 and name.startswith("face") and bool(z["supported"][i]) and tuple(z["shapes"][i][:2]) == (112, 112):
            data = z["streams"][offs[i]:offs[i + 1]].tobytes()
            out["face%d" % faces] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            faces += 1
    assert faces == 4
    mode_of = {0: "L", 2: "RGB", 6: "RGBA"}
    for c in png_cases.load_golden()[0]:
        d = png.parse_png(c["data"])
        if c["supported"] and d.status == 0 and d.depth == 8 and d.colour_type in mode_of and d.trns is None:
            out["png_" + c["name"]] = np.ascontiguousarray(c[mode_of[d.colour_type]])
    out.update(png_enc_cases.synthetic())
    path = png_enc_cases.GOLDEN
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
