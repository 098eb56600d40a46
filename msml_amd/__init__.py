"""MSML on AMD Instinct (gfx950): the model, heads, optimizer and data path over libmsml_hip.so."""


def freeze_batchnorm(module, affine=True):
    """Freeze every BatchNorm under `module` (itself included): eval mode, so the forward normalises with the running
    statistics and leaves them (and num_batches_tracked) untouched, and the backward treats them as constants; with
    affine=True the weight and bias also stop receiving gradients (requires_grad_(False)).  Returns the number of
    BatchNorms frozen.

    As in torch, the mode is a flag of the module: a later `module.train()` (or `model.train()` on a parent) puts the
    BatchNorms back into training mode -- call freeze_batchnorm again after it.  requires_grad stays as set here."""
    from torch.nn.modules.batchnorm import _BatchNorm
    n = 0
    for m in module.modules():
        if isinstance(m, _BatchNorm):
            m.eval()
            if affine:
                for p in (m.weight, m.bias):
                    if p is not None:
                        p.requires_grad_(False)
            n += 1
    return n
