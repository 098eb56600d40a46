"""LightCNN-29v2 FRB, host side (no GPU): construction through MSML, the reference's state-dict layout (keys and
shapes recorded from the reference in tests/golden/g10_lightcnn_eval.npz), the arguments that must raise, and the gray
occlusion helper."""
import numpy as np
import pytest
import torch

from msml_amd import synthetic
from msml_amd.backbones import MSML
from tests.helpers import load

PEER_OFF = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}


def lightcnn_msml(**kw):
    args = dict(fm_params=(3, 2, "sigmoid", "mul"), header_type="Softmax", peer_params=dict(PEER_OFF))
    args.update(kw)
    return MSML("lightcnn", "unet", (1, 1, 1, 1), 1000, **args)


def test_lightcnn_msml_builds_with_the_reference_shapes():
    m = lightcnn_msml()
    assert (m.input_size, m.gray, m.dim_feature) == (128, True, 256)
    assert m.heights == (64, 32, 16, 8) and m.f_channels == (48, 96, 192, 128)
    assert tuple(m.osb.conv1.weight.shape) == (64, 1, 3, 3)
    assert tuple(m.osb.deconv1.weight.shape) == (8, 18, 4, 4)
    assert m.frb.drop.p == 0.0
    # FM bottleneck widths (fmoperator.py:38-39 of the reference)
    assert [m.frb.fm_ops[i].res_block[0].conv1.out_channels for i in range(4)] == [24, 48, 128, 64]


def test_lightcnn_state_dict_matches_the_reference():
    g = load("g10_lightcnn_eval.npz")
    sd = lightcnn_msml().state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(d) for d in t.shape) for t in sd.values()] == [str(s) for s in g["shapes"]]
    assert sum(t.numel() for k, t in sd.items() if k.startswith("frb.") and "num_batches" not in k) > 11_000_000
    # strict round trip
    m2 = lightcnn_msml()
    m2.load_state_dict(sd, strict=True)


def test_lightcnn_without_osb_and_fm_builds():
    m = MSML("lightcnn", "unet", (0, 0, 0, 0), 10, use_osb=False)
    assert m.frb.fc.out_features == 256


@pytest.mark.parametrize("header", ["Softmax", "AMArcFace", "AMCosFace"])
def test_lightcnn_headers_take_256(header):
    m = lightcnn_msml(header_type=header)
    assert m.classification.weight.shape[-1] == 256 or m.classification.weight.shape[0] == 256


def test_lightcnn_pretrained_raises():
    with pytest.raises(NotImplementedError, match="load_state_dict"):
        lightcnn_msml(frb_pretrained=True)


def test_lightcnn_peer_raises():
    with pytest.raises(NotImplementedError, match="LightCNN teacher"):
        lightcnn_msml(peer_params={"use_ori": True, "use_conv": True, "mask_trans": "conv"})


def test_lightcnn_split_bf16_eval_raises():
    m = lightcnn_msml(fp16=True).eval()
    m.eval_precision = "bf16x3"

    class FakeCuda(torch.Tensor):       # passes the device check without a GPU
        @property
        def is_cuda(self):
            return True
    x = torch.zeros(1, 1, 128, 128).as_subclass(FakeCuda)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp16=False.*bf16"):
        m(x)


def test_rect_occlusion_rgb_unchanged_and_gray():
    x = synthetic.images(3, seed=5)
    a, ma = synthetic.rect_occlusion(x, seed=7)
    # the draws of the 3-channel version, restated: ratio, width, position, then one colour per channel
    rng = np.random.RandomState(7)
    b = x.clone()
    mb = torch.ones(3, 112, 112, dtype=torch.int64)
    for i in range(3):
        ratio = rng.randint(0, 36) * 0.01
        area = int(112 * 112 * ratio)
        ow = rng.randint(int(112 * ratio) + 1, 113)
        oh = int(area / ow)
        ox = rng.randint(0, 112 - ow + 1)
        oy = rng.randint(0, 112 - oh + 1)
        for c in range(3):
            b[i, c, oy:oy + oh, ox:ox + ow] = rng.randint(0, 256) / 255.0 * 2.0 - 1.0
        mb[i, oy:oy + oh, ox:ox + ow] = 0
    assert torch.equal(a, b) and torch.equal(ma, mb)
    g = synthetic.gray_images(2)
    assert g.shape == (2, 1, 128, 128) and float(g.min()) >= 0.0 and float(g.max()) <= 1.0
    go, gm = synthetic.rect_occlusion(g, seed=1)
    assert go.shape == g.shape and gm.shape == (2, 128, 128)
    assert torch.equal(go[:, 0][gm == 1], g[:, 0][gm == 1])
