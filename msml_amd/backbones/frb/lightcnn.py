"""Face Recognition Branch: LightCNN-29v2 with Feature-Masking hooks, on the HIP path.

Mirrors backbones/frb/lightcnn.py of the reference (mfm :25-39, group :41-50, resblock :53-66,
network_29layers_v2 :145-237, lightcnn29 :258-306): same module / parameter names (state dicts
interchange, `strict=True`), same default initialisation; forward runs on NHWC tensors through
libmsml_hip.so.  Every mfm is one conv kernel with the max in its epilogue (msml_conv2d_mfm), the
max + avg pool one element-wise kernel (msml_pool2_fwd).  The peer teacher (use_ori) is out of scope
and raises, as backbones/peer does.
"""
import torch
from torch import nn

from ... import functional as Fh
from ..._lib import F32

__all__ = ["lightcnn29", "network_29layers_v2", "mfm", "group", "resblock"]


class mfm(nn.Module):
    """Conv2d(in, 2*out) + max over the two halves (lightcnn.py:25-39; the Linear variant, type 0, is unused by v2)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, padding=1, type=1):
        super().__init__()
        if type != 1:
            raise NotImplementedError("msml_amd: the Linear mfm (type 0) is not used by LightCNN-29v2")
        self.out_channels = out_channels
        self.filter = nn.Conv2d(in_channels, 2 * out_channels, kernel_size=kernel_size, stride=stride,
                                padding=padding)

    def forward(self, x, residual=None):
        return Fh.mfm_conv(self.filter, self.out_channels, x, residual)


class group(nn.Module):
    """mfm 1x1 (in -> in) then mfm k x k (in -> out) (lightcnn.py:41-50)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding):
        super().__init__()
        self.conv_a = mfm(in_channels, in_channels, 1, 1, 0)
        self.conv = mfm(in_channels, out_channels, kernel_size, stride, padding)

    def forward(self, x):
        return self.conv(self.conv_a(x))


class resblock(nn.Module):
    """mfm3x3(mfm3x3(x)) + x (lightcnn.py:53-66); the add is conv2's epilogue."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv1 = mfm(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.conv2 = mfm(in_channels, out_channels, kernel_size=3, stride=1, padding=1)

    def forward(self, x):
        xa, xb = Fh.fanout2(x)           # x feeds conv1 and the residual: one gradient sum, no autograd add
        return self.conv2(self.conv1(xa), residual=xb)


class network_29layers_v2(nn.Module):
    def __init__(self, block, layers, fm_ops, dim_feature=256, dropout=0., peer_params: dict = None):
        super().__init__()
        peer_params = peer_params or {}
        self.conv1 = mfm(1, 48, 5, 1, 2)
        self.block1 = self._make_layer(block, layers[0], 48, 48)
        self.group1 = group(48, 96, 3, 1, 1)
        self.block2 = self._make_layer(block, layers[1], 96, 96)
        self.group2 = group(96, 192, 3, 1, 1)
        self.block3 = self._make_layer(block, layers[2], 192, 192)
        self.group3 = group(192, 128, 3, 1, 1)
        self.block4 = self._make_layer(block, layers[3], 128, 128)
        self.group4 = group(128, 128, 3, 1, 1)
        self.fc = nn.Linear(8 * 8 * 128, dim_feature)
        self.drop = nn.Dropout(p=dropout, inplace=True)
        assert len(fm_ops) == 4
        self.fm_ops = nn.ModuleList(fm_ops)
        self.peer = None
        self.header_type = str(peer_params.get("header_type", "")).lower()
        if peer_params.get("use_ori"):
            # (lightcnn.py:186-193: a Softmax header takes the LightCNN teacher, any other raises)
            if "softmax" not in self.header_type:
                raise ValueError("Error type of lightcnn, cannot decide peer network.")
            from ..peer import lightcnn29_v2
            self.peer = lightcnn29_v2().requires_grad_(False)

    @staticmethod
    def _make_layer(block, num_blocks, in_channels, out_channels):
        return nn.Sequential(*[block(in_channels, out_channels) for _ in range(num_blocks)])

    def forward(self, x, segs, ori=None, wait_segs=None, dtype=F32):
        """x: NCHW f32 gray image (B, 1, 128, 128); segs: [seg3, seg2, seg1, seg0] NHWC 18-channel maps (detached);
        wait_segs: event after which `segs` are valid; dtype: storage of the maps (F32 or BF16).
        Returns (feature (B, dim) f32, kd)."""
        if ori is not None:
            raise TypeError("'NoneType' object is not callable: `ori` given but no peer network was built "
                            "(peer_params.use_ori False)")
        x = Fh.mfm_stem(self.conv1.filter, 48, x.float().contiguous(), dtype)
        stages = ((self.block1, self.group1), (self.block2, self.group2),
                  (self.block3, self.group3, self.block4, self.group4))
        x = Fh.pool2(x)
        if wait_segs is not None:
            torch.cuda.current_stream().wait_event(wait_segs)
        x, _ = self.fm_ops[0](x, segs[0], None)
        for k, mods in enumerate(stages):
            for m in mods:
                x = m(x)
            x = Fh.pool2(x)
            x, _ = self.fm_ops[k + 1](x, segs[k + 1], None)
        # flatten(C,H,W) + Linear(8192, dim): skinny GEMM on the NHWC-ordered operand (lightcnn.py:232-233)
        n, h, w, c = x.shape
        wview = self.fc.weight.view(self.fc.out_features, c, h, w)
        y = Fh.flat_fc(x, wview, self.fc.bias, self.fc.weight)
        if self.drop.p > 0 and self.training:
            y = Fh.dropout(y, self.drop.p)
        return Fh.to_vec(y, self.fc.out_features), 0.0


def lightcnn29(fm_ops, pretrained=True, dim_feature=256, dropout=0., peer_params=None):
    """lightcnn.py:258-306.  pretrained=False, the branch train.py takes, drops `dropout` (Dropout(p=0)) exactly as the
    reference does; the pretrained checkpoint is not shipped: load it with load_state_dict."""
    if pretrained:
        raise NotImplementedError("msml_amd: pretrained FRB weights are loaded via load_state_dict")
    return network_29layers_v2(resblock, [1, 2, 3, 4], fm_ops=fm_ops, dim_feature=dim_feature,
                               peer_params=peer_params)
