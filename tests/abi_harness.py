"""Memory hygiene of the direct C-ABI tests (tests/test_gpu_bn.py, tests/test_gpu_head.py, tests/test_gpu_ew.py) without a
sanitizer: every output lives between two guard bands of a sentinel, outputs are pre-filled with NaN (an element the
kernel does not write fails the comparison), every input is cloned before the call and compared after it."""
import torch

from msml_amd import _lib

GUARD = 64
SENTINEL = -1232.0            # exact in bf16, f32 and f64
DTC = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


class GuardedDevice:
    """out(): a guarded output buffer; call(): the entry point through msml_amd._lib.call with the checks above."""
    name = "device"

    def __init__(self):
        self.bufs = []            # every guarded buffer of this case: (buffer, payload elements)
        self.pending = []         # allocated since the last call: the outputs of the next one

    def out(self, shape, dtype, init=None):
        n = 1
        for s in shape:
            n *= s
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        v = buf[GUARD:GUARD + n].view(shape)
        if init is None:
            v.fill_(float("nan"))
        elif torch.is_tensor(init):
            v.copy_(init)
        else:
            v.fill_(init)
        self.bufs.append((buf, n))
        self.pending.append((buf.data_ptr(), buf.data_ptr() + buf.numel() * buf.element_size()))
        return v

    def call(self, name, *args):
        def is_out(a):
            return any(lo <= a.data_ptr() < hi for lo, hi in self.pending)
        ins = [(a, a.clone()) for a in args if torch.is_tensor(a) and not is_out(a)]
        _lib.call(name, *args)
        for a, c in ins:
            assert torch.equal(a.contiguous().view(torch.uint8), c.contiguous().view(torch.uint8)), "%s modified an input" % name
        for buf, n in self.bufs:
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all()), \
                "%s wrote outside an output buffer" % name
        self.pending = []

