"""smoke(): one small pass of the hot path on cuda:0 checked against the CPU oracle.

Eval forward of ires18-MSML (f32 parity mode) on 2 synthetic occluded faces: embeddings within
1e-3 rel of the oracle, occlusion-mask indices bit-exact; then one bf16 training step
(forward + backward + fused clip/SGD) to exercise the backward kernels; then one fixture JPEG decoded on the device,
bit-exact with the pixels Pillow recorded."""
import torch


def run():
    assert torch.cuda.is_available(), "smoke() needs a GPU"
    from msml_amd import _lib, functional as Fh, synthetic
    from msml_amd.backbones import MSML
    from msml_amd.optim import FlatSGD, reference_param_groups
    from msml_amd.tricks.consensus_loss import StructureConsensuLossFunction
    from oracle import model as om
    from oracle.fill import fill_module
    _lib.load()
    peer = {"use_ori": False, "use_conv": False, "mask_trans": "conv", "use_decoder": False}
    kw = dict(fm_params=(3, 2, "sigmoid", "mul"), header_type="AMArcFace",
              header_params=(64.0, 0.48, 0.0, 0.0))
    m = fill_module(MSML("iresnet18", "unet", (1, 1, 1, 1), 100, peer_params=peer, **kw)).cuda().eval()
    o = fill_module(om.MSML("iresnet18", "unet", (1, 1, 1, 1), 100, **kw)).eval()
    x, msk = synthetic.rect_occlusion(synthetic.images(2, 1), 1)
    with torch.no_grad():
        f_ref, seg_ref = o(x)
        f, seg = m(x.cuda())
    err = ((f.cpu() - f_ref).norm() / f_ref.norm()).item()
    same = torch.equal(Fh.mask_index(seg).cpu().long(), om.mask_index(seg_ref))
    assert err < 1e-3 and same, (err, same)
    # one bf16 training step (seeded: the reference's default init is random)
    torch.manual_seed(0)
    t = MSML("iresnet18", "unet", (1, 1, 1, 1), 100, fp16=True, peer_params=peer, **kw).cuda().train()
    opt = FlatSGD(reference_param_groups(t, 2, 1), 0.9, 5e-4, 5.0)
    label = synthetic.labels(2, 100, 1).cuda()
    opt.zero_grad()
    cls, seg, _ = t(x.cuda(), label)
    loss = torch.nn.functional.cross_entropy(cls, label) + \
        StructureConsensuLossFunction(10.0, 5.0)(seg, msk.cuda(), msk.cuda())
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and torch.isfinite(opt.grad_norm()).item()
    _jpeg()
    print("smoke ok: eval feature rel err %.2e, masks bit-exact, train loss %.4f grad-norm %.3f"
          % (err, loss.item(), opt.grad_norm().item()))


def _jpeg():
    import os
    import numpy as np
    from msml_amd import jpeg
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                             "g15_jpeg.npz"), allow_pickle=False)
    i = [str(s) for s in z["names"]].index("face0_112x112_420_q95_r3")
    data = z["streams"][z["stream_offsets"][i]:z["stream_offsets"][i + 1]].tobytes()
    want = z["pixels"][z["pixel_offsets"][i]:z["pixel_offsets"][i + 1]].reshape(112, 112, 3)
    got = jpeg.decode_batch([data], size=(112, 112))[0].cpu().numpy()
    assert np.array_equal(got, want), "JPEG decode differs from libjpeg's pixels"
    z = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                             "g16_jpeg_enc.npz"), allow_pickle=False)
    i = [str(s) for s in z["names"]].index("uniform0_112x112_420_q75_r0")
    src = z["sources"][z["source_offsets"][i]:z["source_offsets"][i + 1]].reshape(1, 112, 112, 3)
    want = z["streams"][z["stream_offsets"][i]:z["stream_offsets"][i + 1]].tobytes()
    import torch
    assert jpeg.encode_batch(torch.from_numpy(src).cuda()).to_bytes() == [want], "JPEG encode differs from libjpeg's bytes"
