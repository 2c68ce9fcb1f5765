"""The diagnostic two-pass step kernel (MODE 2, ``ecg_tiny_step_grads_twice``: every workgroup computes its sample
twice, the second time over the LDS the first pass left behind) writes the same gradient rows as the production
step kernel, bit for bit: every sum of a pass runs in a fixed order and every pass rewrites the pads it reads.

MODE 2 only exists at 8 waves, so the production kernel is forced to 8 waves as well (same per-sample summation
order).  Window lengths: 8 (less than one 16-step tile), 33 (one step into the second tile pair), 100 (four pairs).
"""
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

pytestmark = pytest.mark.gpu

B, NC = 3, 2
CONFIGS = {"fp32": ("fp32", False), "bf16_lds": ("bf16", False), "bf16_prefrag": ("bf16", True)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("L", [8, 33, 100])
def test_two_pass_rows_equal_single_pass_rows(L, config):
    from crossscale_ecg.ops import _lib
    from crossscale_ecg.ops.fused_tiny import labels_int32, new_wprep, prec_id, slab_stride, tiny_step_grads
    precision, prefrag = CONFIGS[config]
    dev = torch.device("cuda:0")
    torch.manual_seed(L)
    model = TinyECG(num_classes=NC).to(dev)
    flat = model.flatten_parameters()
    x = torch.randn(B, L, device=dev)
    y32 = labels_int32(torch.randint(0, NC, (B,), device=dev), NC)
    stride = slab_stride(NC)
    # both slabs start from the same sentinel, so the columns neither kernel writes compare equal too
    once = torch.full((B, stride), -7.0, device=dev)
    twice = torch.full((B, stride), -7.0, device=dev)
    wprep = new_wprep(dev) if prefrag else None
    lib = _lib.kernels()
    prev = lib.ecg_tiny_force_waves(8)
    try:
        tiny_step_grads(flat, x, y32, None, B, NC, slab=once, precision=precision, prefrag=prefrag, wprep=wprep)
        st = lib.ecg_tiny_step_grads_twice(x.data_ptr(), L, x.stride(0), None, y32.data_ptr(), flat.data_ptr(), NC,
                                           twice.data_ptr(), stride, B, 1.0 / B, prec_id(precision),
                                           _lib.ptr(wprep), _lib.stream_ptr(dev))
        _lib.check(st, "ecg_tiny_step_grads_twice")
        torch.cuda.synchronize()
    finally:
        lib.ecg_tiny_force_waves(prev)
    P = num_params(NC)  # columns [0, P): gradients, column P: loss
    assert torch.isfinite(once[:, :P + 1]).all()
    assert (once[:, P] > 0).all(), "the loss column still holds the sentinel: nothing was written"
    assert torch.equal(once.view(torch.int32), twice.view(torch.int32)), (once - twice).abs().max().item()
