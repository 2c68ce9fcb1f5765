"""The operand-exact TinyECG reference (models/tiny_ecg_ref.py) on its own, without a GPU: its algebra against float64
autograd, its noise floor on exactly the cases of tests/test_tiny_operand_exact_gpu.py (the number the bounds of that
file are set from), that the bound has teeth against the two classic seam defects of a tiled kernel, and exact zeros."""
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from crossscale_ecg.models.tiny_ecg_ref import (INTERMEDIATES, logit_error, row_errors, row_tensors, split_params,
                                                tiny_ecg_reference)

import tiny_operand_cases as tc


@pytest.mark.parametrize("L", [8, 33, 100])
@pytest.mark.parametrize("nc", [2, 5, 16])
def test_algebra_equals_float64_autograd(L, nc):
    g = torch.Generator(device="cpu").manual_seed(100 * L + nc)
    torch.manual_seed(nc)
    model = TinyECG(num_classes=nc)
    x, y = torch.randn(tc.B, L, generator=g), torch.randint(0, nc, (tc.B,), generator=g)
    ref = tiny_ecg_reference(tc.flat_of(model), x, y, 1.0 / tc.B, nc, rounding=None)
    rows, logits = tc.autograd_rows(model, x, y, 1.0 / tc.B, torch.float64)
    errs = row_errors(ref.rows, rows, nc)
    print(", ".join(f"{n} {e:.2e}" for n, e in errs.items()), f"logits {logit_error(ref.logits, logits):.2e}")
    assert ref.rows.dtype == torch.float64 and ref.rows.shape == (tc.B, num_params(nc) + 1)
    assert max(errs.values()) < 1e-10 and logit_error(ref.logits, logits) < 1e-10
    assert torch.equal(ref.rows[:, -1], ref.loss) and set(ref.inter) == set(INTERMEDIATES)


def test_row_layout_is_param_layout():
    names = [n for n, _ in row_tensors(5)]
    assert names == [n for n, _ in TinyECG(5).named_parameters()] + ["loss"]
    assert row_tensors(5)[-1][1] == slice(num_params(5), num_params(5) + 1)


def test_rounding_points_are_bf16_values():
    c = tc.grad_case(33, 2)
    for name in ("h1", "dh1"):
        t = c["ref"].inter[name]
        assert torch.equal(t, t.to(torch.bfloat16).to(t.dtype)), name
    assert set(c["ref"].inter["m"].unique().tolist()) <= {0.0, 1.0}
    # bf16 rounding is what separates it from autograd: percents, not the noise floor
    plain = tiny_ecg_reference(c["flat"], c["x"], c["y"], 1.0 / tc.B, 2, rounding=None)
    assert max(row_errors(c["ref"].rows, plain.rows, 2).values()) > 1e-3


def _check_bound(floor, recorded, bound):
    """``bound`` is 10 x the recorded floor (rounded up to two digits) and <= 1e-3, and the floor measured now is the
    recorded one.  The floor is a few float32 ulps, so the summation order of the host's CPU library (its ISA path,
    its thread count) moves it a little: within a factor of 1.5 either way it counts as the same floor."""
    assert 10 * recorded <= bound <= 10 * 1.05 * recorded and bound <= 1e-3
    assert recorded / 1.5 <= floor <= recorded * 1.5, f"measured floor {floor:.3g}, recorded {recorded:.3g}"


def test_noise_floor_sets_the_bound():
    """The reference in float32 against the reference in float64 on exactly the GPU file's bf16 cases."""
    floors = tc.bf16_floor()
    for k, v in floors.items():
        print(k, f"{v:.3g}")
    floor = max(floors.values())
    print(f"bf16 reference floor {floor:.3g}: REF_BOUND = 10 x floor = {10 * floor:.3g}, set to {tc.REF_BOUND:.3g}")
    assert len(floors) == len(tc.GRAD_CASES) + 1 + len(tc.LOGIT_CASES)
    assert floor <= tc.SEED_FLOOR_MAX
    _check_bound(floor, tc.REF_FLOOR, tc.REF_BOUND)


def test_fp32_noise_floor_sets_the_bound():
    """float32 autograd against float64 autograd on exactly the GPU file's fp32 cases."""
    floors = tc.f32_floor()
    for k, v in floors.items():
        print(k, f"{v:.3g}")
    floor = max(floors.values())
    print(f"fp32 floor {floor:.3g}: REF_BOUND_F32 = 10 x floor = {10 * floor:.3g}, set to {tc.REF_BOUND_F32:.3g}")
    _check_bound(floor, tc.REF_FLOOR_F32, tc.REF_BOUND_F32)
    for c in tc.F32_CASES:  # the reference the fp32 kernels are compared with is float64 autograd
        case = tc.f32_case(*c)
        rows, logits = case["autograd64"]
        assert max(row_errors(case["ref"].rows, rows, c[1]).values()) < 1e-10


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


@pytest.mark.parametrize("nc", [2, 5])
def test_bound_has_teeth(nc):
    """Defect A: h1 at one time step replaced by its neighbour.  Defect B: one conv2 dgrad tap dropped at the last
    time step.  At the largest L of the GPU cases, each moves a tensor of every sample's row by > 3 x REF_BOUND."""
    L = max(tc.GRAD_L)
    c = tc.grad_case(L, nc)
    ref = c["ref"]
    args = (c["flat"], c["x"], c["y"], 1.0 / tc.B, nc)
    h1 = ref.inter["h1"].clone()
    h1[:, :, L // 2] = h1[:, :, L // 2 - 1]
    a = tiny_ecg_reference(*args, replace={"h1": h1})
    w2b = _bf16(split_params(c["flat"], nc)[2])
    w2g = _bf16(w2b[None] * ref.inter["g"][:, :, None, None])
    dh1 = ref.inter["dh1"].clone()
    tap = torch.einsum("bo,boi->bi", ref.inter["m"][:, :, L - 2], w2g[:, :, :, 3])  # dh1[L-1] <- m[L-2], k = 3
    dh1[:, :, L - 1] = _bf16(dh1[:, :, L - 1] - tap) * (ref.inter["h1"][:, :, L - 1] > 0)
    b = tiny_ecg_reference(*args, replace={"dh1": dh1})
    for what, bad in (("A", a), ("B", b)):
        for s in range(tc.B):
            e = max(row_errors(bad.rows[s:s + 1], ref.rows[s:s + 1], nc).values())
            print(f"defect {what} nc={nc} sample {s}: {e:.3g}")
            if what == "B" and not tap[s].any():
                continue  # (no active conv2 output at L - 2: the dropped tap carries nothing for this sample)
            assert e > 3 * tc.REF_BOUND, (what, s, e)
    assert not torch.equal(b.rows[:, :128], ref.rows[:, :128]) and torch.equal(b.rows[:, 128:], ref.rows[:, 128:])


def test_exact_zeros():
    """The recorder's "zeros" inputs: zero conv1 bias and a run of exact-zero windows (exact zero pre-activations of
    both convolutions), -0.0: relu'(0) = 0, finite rows, and the algebra still equals autograd's."""
    c = tc.grad_case(100, 2, "zeros")
    x, ref = c["x"], c["ref"]
    assert (x[:, 15:58] == 0).all() and torch.signbit(x[0, 58:62]).all() and (x[0, 58:62] == 0).all()
    assert torch.isfinite(ref.rows).all() and torch.isfinite(ref.logits).all()
    # conv1 sees only zeros at t in [18, 55): pre-activation exactly 0 -> h1 = 0 and relu'(h1) = 0
    assert (ref.inter["h1"][:, :, 18:55] == 0).all() and (ref.inter["dh1"][:, :, 18:55] == 0).all()
    assert (ref.inter["dh1"] != 0).any()
    # conv2 there is its bias alone, zero on the even channels: relu'(0) = 0; the odd ones follow their bias's sign
    b2 = split_params(c["flat"], 2)[3]
    assert (ref.inter["m"][:, ::2, 20:53] == 0).all()
    assert torch.equal(ref.inter["m"][:, 1::2, 20:53], (_bf16(b2[1::2]) > 0).double()[None, :, None].expand(tc.B, 8, 33))
    model = tc.zeros_weights(2)
    plain = tiny_ecg_reference(c["flat"], x, c["y"], 1.0 / tc.B, 2, rounding=None)
    rows, logits = tc.autograd_rows(model, x, c["y"], 1.0 / tc.B, torch.float64)
    assert max(row_errors(plain.rows, rows, 2).values()) < 1e-10
