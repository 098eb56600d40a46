"""MSML on the MI355X HIP path: drop-in for backbones/msml.py of the reference.

Same constructor (msml.py:20-33), same forward(x, label=None, ori=None) (msml.py:150-174):
training returns (final_cls, final_seg, kd), eval returns (feature, final_seg); state-dict keys
are `frb.*`, `osb.*`, `classification.*` exactly as the reference's.

`fp16` selects the compute mode of the whole net: False -> exact-f32 MFMA (parity mode, matches
the reference's fp32 results to rounding), True -> bf16 operands with f32 accumulation
(the reference's autocast analogue; see DESIGN.md for the measured error).
"""
import os

import torch
import torch.nn as nn

from .. import functional as Fh
from .._lib import BF16, F32
from ..headers import AMArcFace, AMCosFace, Softmax
from .fm import FMCnn, FMNone
from .frb import iresnet18, iresnet34, iresnet50, iresnet100, lightcnn29
from .osb import unet

__all__ = ["MSML"]


class MSML(nn.Module):
    frb_type_list = ("lightcnn", "iresnet18", "iresnet34", "iresnet50", "iresnet100")
    osb_type_list = ("unet",)
    head_type_list = ("Softmax", "AMArcFace", "AMCosFace")

    def __init__(self, frb_type: str, osb_type: str, fm_layers: tuple, num_classes: int,
                 fp16: bool = False, frb_pretrained: bool = False,
                 fm_params: tuple = (3, 2, "tanh", "add"), header_type: str = "Softmax",
                 header_params: tuple = (64.0, 0.5, 0.0, 0.0), dropout: float = 0.,
                 use_osb: bool = True, peer_params: dict = None):
        super().__init__()
        assert len(fm_layers) == 4
        # shapes per FRB family (msml.py:47-58)
        self.lightcnn = "lightcnn" in frb_type
        if self.lightcnn:
            self.input_size, self.gray = 128, True
            self.heights = (64, 32, 16, 8)
            self.f_channels = (48, 96, 192, 128)
            self.dim_feature = 256
        elif "iresnet" in frb_type:
            self.input_size, self.gray = 112, False
            self.heights = (56, 28, 14, 7)
            self.f_channels = (64, 128, 256, 512)
            self.dim_feature = 512
        else:
            raise ValueError("FRB type error")
        if "unet" not in osb_type:
            raise ValueError("OSB type error")
        self.s_channels = (18, 18, 18, 18)
        peer_params = dict(peer_params or {})
        peer_params["header_type"] = header_type
        kernel_size, num_res, act, arith = fm_params
        fm_ops = []
        for i in range(4):
            if fm_layers[i] == 0:
                fm_ops.append(FMNone())
            elif fm_layers[i] == 1:
                fm_ops.append(FMCnn(self.heights[i], self.heights[i], self.f_channels[i], kernel_size,
                                    num_res, act, arith, peer_params))
            else:
                raise ValueError("FM Operators type error")
        self.fm_ops = fm_ops          # plain list, like the reference (registered under frb)
        ctor = None
        if self.lightcnn:
            ctor = lightcnn29
        for key, fn in (("100", iresnet100), ("18", iresnet18), ("34", iresnet34), ("50", iresnet50)):
            if ctor is None and key in frb_type:
                ctor = fn
                break
        if ctor is None:
            raise ValueError("IResNet type {} not found".format(frb_type))
        self.frb = ctor(self.fm_ops, pretrained=frb_pretrained, dropout=dropout,
                        peer_params=peer_params)
        self.osb = unet(backbone="r18", gray=self.gray, input_size=self.input_size)
        self.num_classes = num_classes
        assert header_type in self.head_type_list
        s, m, a, k = header_params
        if "Softmax" in header_type:
            self.classification = Softmax(self.dim_feature, num_classes, device_id=None)
        elif "AMCosFace" in header_type:
            self.classification = AMCosFace(self.dim_feature, num_classes, device_id=None, s=s, m=m,
                                            a=a, k=k)
        else:
            self.classification = AMArcFace(self.dim_feature, num_classes, device_id=None, s=s, m=m,
                                            a=a, k=k)
        self.fp16 = fp16
        self.classification.fp16 = fp16
        self.use_osb = use_osb
        # Inference precision with fp16=True: "bf16x3" = split-bf16 operands (hi + lo, three bf16 MFMAs
        # per product, csrc/x3.hip) -- embeddings within 1e-3 and mask indices bit-exact against the f32
        # reference, the outputs the north-star tolerances are stated for; "bf16" = plain bf16 operands,
        # ~3x the throughput at ~5e-3 embedding error.  Training with fp16=True is always bf16.
        self.eval_precision = os.environ.get("MSML_EVAL_PRECISION", "bf16x3")
        self.x3_chunk = 256

    def forward(self, x, label=None, ori=None):
        if not x.is_cuda:
            raise RuntimeError("msml_amd.MSML runs on an MI355X only (no CPU path); got a CPU tensor")
        if self.lightcnn and self.fp16 and not self.training and not torch.is_grad_enabled() \
                and self.eval_precision not in ("bf16",):
            raise NotImplementedError("msml_amd: split-bf16 (%r) inference is not built for the LightCNN FRB; use "
                                      "fp16=False (exact f32, what the reference evaluates with) or "
                                      "eval_precision='bf16'" % (self.eval_precision,))
        from .. import ops
        if (self.fp16 and not self.training and not torch.is_grad_enabled() and self.eval_precision == "bf16x3"
                and x.shape[0] > self.x3_chunk):
            # split-bf16 maps hold 6 B per element: a 112 x 112 x 64-channel map of more than ~440 images
            # passes the 2 GiB range of a buffer descriptor.  Images are independent in eval mode, so
            # the batch is processed in chunks (bit-identical results, see the batch-composition test).
            def part(t, i):                  # label / ori travel with their images
                return None if t is None else t[i:i + self.x3_chunk]
            outs = [self.forward(x[i:i + self.x3_chunk], part(label, i), part(ori, i))
                    for i in range(0, x.shape[0], self.x3_chunk)]
            # (use_osb=False returns (feature, None): pass a None output through)
            return tuple(None if t[0] is None else torch.cat(t) for t in zip(*outs))
        ops.PACKS.refresh_if_stale()      # one batched repack after a FlatSGD step
        ops.DEFER_BN_COUNTERS = True      # num_batches_tracked: one foreach add per forward
        try:
            return self._forward(x, label, ori)
        finally:
            ops.DEFER_BN_COUNTERS = False
            ops.flush_bn_counters()

    def _forward(self, x, label, ori):
        from .. import ops
        # bf16: the stems unfold the raw image themselves (im2col + 1x1 conv); f32: padded NHWC
        x3 = (self.fp16 and not self.training and not torch.is_grad_enabled()
              and self.eval_precision == "bf16x3")
        xh = Fh.RawImage(x.float(), x3=x3) if self.fp16 else Fh.to_nhwc(x, F32)
        if ori is not None:
            ori = Fh.RawImage(ori.float()) if self.fp16 else Fh.to_nhwc(ori, F32)
        if self.lightcnn:
            return self._forward_lightcnn(x, xh, label, ori)
        side = ops.OSB_STREAM
        if not self.use_osb:                      # msml.py:159-161: no masks (FMNone stages only)
            feature, kd = self.frb(xh, (None, None, None, None), ori)
            if self.training:
                if label is None:
                    return feature, None, kd
                return self.classification(feature, label) + kd, None, kd
            return feature, None
        if side is None:
            seg_list = self.osb(xh)                # [seg0, seg1, seg2, seg3, seg5]
            osb_done = None
        else:
            # OSB on its own stream: its forward overlaps the FRB stem / layer1, its backward
            # (autograd replays nodes on their forward stream) the whole FRB backward
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            xh.record_stream(side)
            with torch.cuda.stream(side):
                seg_list = self.osb(xh)
                osb_done = side.record_event()
            for t_ in seg_list:
                t_.record_stream(main)
        final_seg = seg_list[4]
        segs = [seg_list[3], seg_list[2], seg_list[1], seg_list[0]]
        feature, kd = self.frb(xh, segs, ori, wait_segs=osb_done)
        if self.training:
            if label is None:
                # head-less training return for the PartialFC path (train.py:283): the reference's
                # dead op2 branch calls backbone(img) and feeds the embedding to PartialFC.
                return feature, final_seg, kd
            final_cls = self.classification(feature, label) + kd
            return final_cls, final_seg, kd
        return feature, final_seg

    def _forward_lightcnn(self, x, xh, label, ori):
        """_forward for the LightCNN FRB: its mfm stem unfolds the raw gray image itself (msml_stem_im2col, 5x5 -> 32
        patches), the OSB takes the stem input it takes for IResNet (xh)."""
        from .. import ops
        dtype = BF16 if self.fp16 else F32
        if not self.use_osb:
            feature, kd = self.frb(x, (None, None, None, None), ori, dtype=dtype)
            if self.training:
                if label is None:
                    return feature, None, kd
                return self.classification(feature, label) + kd, None, kd
            return feature, None
        side = ops.OSB_STREAM
        if side is None:
            seg_list = self.osb(xh)
            osb_done = None
        else:
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            xh.record_stream(side)
            with torch.cuda.stream(side):
                seg_list = self.osb(xh)
                osb_done = side.record_event()
            for t_ in seg_list:
                t_.record_stream(main)
        final_seg = seg_list[4]
        segs = [seg_list[3], seg_list[2], seg_list[1], seg_list[0]]
        feature, kd = self.frb(x, segs, ori, wait_segs=osb_done, dtype=dtype)
        if self.training:
            if label is None:
                return feature, final_seg, kd
            return self.classification(feature, label) + kd, final_seg, kd
        return feature, final_seg
