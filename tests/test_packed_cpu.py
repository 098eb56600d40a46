"""CPU tests of the packed image form (msml_amd/packed.py): the layout rule, the host check every consumer of a caller's
(buf, meta) goes through, and the front of mtcnn_align and detect_faces.  Nothing here needs the library."""
import numpy as np
import pytest
import torch

from msml_amd import ijb, packed


def test_layout_rounds_pitches_and_accumulates_offsets():
    widths = np.array([1, 2, 3, 5, 8], np.int64)
    heights = np.array([3, 1, 4, 2, 5], np.int64)
    for channels in (1, 3, 4):
        meta, total = packed.layout(heights, widths, channels)
        assert meta.dtype == np.int64 and meta.shape == (5, 4) and meta.flags["C_CONTIGUOUS"]
        end = 0
        for (off, h, w, pitch), hh, ww in zip(meta, heights, widths):
            row = ww * channels
            assert (h, w) == (hh, ww) and pitch % 4 == 0 and row <= pitch < row + 4
            assert off == end
            end = off + h * pitch
        assert total == end
    meta, total = packed.layout([7], [5])                       # three channels unless told otherwise
    assert meta.tolist() == [[0, 7, 5, 16]] and total == 112


def test_layout_is_what_the_consumers_accept():
    meta, total = packed.layout([3, 1, 4, 2, 5], [1, 2, 3, 5, 8])
    buf = torch.zeros(total, dtype=torch.uint8)
    got = packed.check(buf, meta, "align_faces")
    assert got.dtype == np.int64 and got.flags["C_CONTIGUOUS"] and got.tolist() == meta.tolist()
    assert packed.check(buf, torch.from_numpy(meta), "align_faces").tolist() == meta.tolist()
    with pytest.raises(ValueError, match="align_faces: meta row 4"):
        packed.check(buf[:total - 1], meta, "align_faces")      # the pitch's padding counts: 3 W = 24 is the pitch here
    # pack_images' tight rows pass too, and keep their layout
    imgs = [np.full((2, 3, 3), 7, np.uint8), np.full((1, 1, 3), 9, np.uint8)]
    pbuf, pmeta = ijb.pack_images(imgs)
    assert pmeta.tolist() == [[0, 2, 3, 9], [20, 1, 1, 3]] and pbuf.numel() == 24
    assert packed.check(pbuf, pmeta, "x").tolist() == pmeta.tolist()


def test_check_refuses_every_row_that_is_not_an_image_inside_the_buffer():
    good = [8, 5, 7, 24]                                        # ends at 8 + 4 * 24 + 21 = 125
    buf = torch.zeros(125, dtype=torch.uint8)
    assert packed.check(buf, [good], "who").tolist() == [good]
    bad = {"negative offset": [-4, 5, 7, 24], "offset not a multiple of 4": [6, 5, 7, 24], "pitch < 3 W": [8, 5, 7, 20],
           "pitch >= 2^31": [8, 5, 7, 2 ** 31], "H = 0": [8, 0, 7, 24], "W = 0": [8, 5, 0, 24],
           "H = 32768": [8, 32768, 7, 24], "W = 32768": [8, 5, 32768, 3 * 32768]}
    for name, row in bad.items():
        with pytest.raises(ValueError, match="who: meta row 1 "):
            packed.check(torch.zeros(2 ** 20, dtype=torch.uint8), [good, row], "who")
    with pytest.raises(ValueError, match=r"who: meta row 0 \(offset 8, 5 x 7, pitch 24\) does not describe an image inside "
                                         "the 124-byte buffer"):
        packed.check(buf[:124], [good], "who")                  # the last row one byte past the buffer
    for meta in (np.zeros((0, 4), np.int64), np.zeros((2, 3), np.int64), np.zeros((1, 4), np.float32), np.zeros(4, np.int64)):
        with pytest.raises(ValueError, match="who: meta must be \\[N\\]\\[4\\] integers"):
            packed.check(buf, meta, "who")
    for b in (torch.zeros(125, dtype=torch.int8), torch.zeros(5, 25, dtype=torch.uint8), torch.zeros(250, dtype=torch.uint8)[::2],
              np.zeros(125, np.uint8)):
        with pytest.raises(ValueError, match="who: buf must be a contiguous 1-D uint8 tensor"):
            packed.check(b, [good], "who")


def test_sources_checks_a_callers_pair_and_packs_a_list():
    imgs = [np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3), np.full((1, 5, 3), 9, np.uint8)]
    buf, meta = packed.sources(imgs, "detect_faces")
    assert meta.tolist() == ijb.pack_images(imgs)[1].tolist() and buf.numel() == 36
    same_buf, same = packed.sources((buf, meta), "detect_faces")
    assert same_buf is buf and same.tolist() == meta.tolist()
    past = meta.copy()
    past[1, 1] = 2                                              # a second row that the buffer does not hold
    with pytest.raises(ValueError, match="detect_faces: meta row 1"):
        packed.sources((buf, past), "detect_faces")
    with pytest.raises(ValueError, match="pack_images"):
        packed.sources([], "detect_faces")


def test_meta_on_device_takes_a_fitting_tensor_and_uploads_the_rest():
    cpu = torch.device("cpu")
    meta, _ = packed.layout([2, 3], [4, 5])
    t = torch.from_numpy(meta)
    assert packed.meta_on_device(t, 2, cpu, "decode_into") is t
    up = packed.meta_on_device(meta.tolist(), 2, cpu, "decode_into")
    assert up.dtype == torch.int64 and up.tolist() == meta.tolist()
    with pytest.raises(ValueError, match=r"decode_into: meta must be \[3\]\[4\]"):
        packed.meta_on_device(meta, 3, cpu, "decode_into")
    for wrong in (t.to(torch.int32), t[:1], t.t().contiguous().t()):
        with pytest.raises(ValueError, match="decode_into: a meta tensor must be contiguous int64"):
            packed.meta_on_device(wrong, 2, cpu, "decode_into")
    u = packed.uniform_meta(3, 2, 5, 3, cpu)
    assert u.tolist() == [[0, 2, 5, 15], [30, 2, 5, 15], [60, 2, 5, 15]] and packed.uniform_meta(3, 2, 5, 3, cpu) is u
