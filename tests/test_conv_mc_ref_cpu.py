"""The pieces of tests/test_conv_mc_exact_gpu.py proved without a kernel (tests/conv_mc_cases.py): the float64
references equal torch autograd in float64, an fp32 emulation of a correct kernel stays inside the derived per-element
bound on every case of the GPU file's table (a slice of the samples where a case is large), its rounding-flip share sets
``FLIP_CAP``, and three injected defects each break the bound."""
import functools

import pytest
import torch
import torch.nn.functional as F

import conv_mc_cases as cc

SHAPES = [  # B, L, Cin, Cout, K, stride, pad
    (2, 9, 3, 4, 3, 2, 1),
    (3, 8, 2, 5, 3, 2, 1),   # (L + 2p - K) % 2 != 0
    (2, 7, 4, 3, 1, 2, 0),
    (2, 8, 4, 3, 1, 2, 0),
    (3, 11, 3, 2, 5, 1, 2),
    (2, 6, 2, 2, 3, 1, 0),
    (2, 10, 3, 3, 5, 2, 1),
]


def _draw(B, L, Cin, Cout, K, s, p):
    g = torch.Generator().manual_seed(B * 100 + L)
    x = torch.randn(B, L, Cin, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Cout, K, Cin, generator=g, dtype=torch.float64, requires_grad=True)
    Lo = (L + 2 * p - K) // s + 1
    dy = torch.randn(B, Lo, Cout, generator=g, dtype=torch.float64)
    y = F.conv1d(x.transpose(1, 2), w.permute(0, 2, 1), None, stride=s, padding=p).transpose(1, 2)
    return x, w, dy, y, Lo


@pytest.mark.parametrize("shape", SHAPES)
def test_conv_reference_equals_autograd(shape):
    B, L, Cin, Cout, K, s, p = shape
    x, w, dy, y, Lo = _draw(*shape)
    torch.testing.assert_close(cc.conv_nlc(x.detach(), w.detach(), s, p, 1, Lo), y.detach(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES)
def test_data_grad_as_dilated_conv_equals_autograd(shape):
    """Conv-transpose written as the kernel's call: dilated input, flipped taps, pad K-1-p."""
    B, L, Cin, Cout, K, s, p = shape
    x, w, dy, y, Lo = _draw(*shape)
    dx, = torch.autograd.grad(y, x, dy)
    w_d = w.detach().flip(1).permute(2, 1, 0).contiguous()  # [Cin][K][Cout]
    torch.testing.assert_close(cc.conv_nlc(dy, w_d, 1, K - 1 - p, s, L), dx, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES)
def test_weight_grad_reference_equals_autograd(shape):
    B, L, Cin, Cout, K, s, p = shape
    x, w, dy, y, Lo = _draw(*shape)
    dw, = torch.autograd.grad(y, w, dy)
    ref, S = cc.wgrad_ref(dy, x.detach(), K, s, p)
    torch.testing.assert_close(ref, dw, rtol=1e-12, atol=1e-12)
    want = torch.nn.grad.conv1d_weight(x.detach().transpose(1, 2), (Cout, Cin, K), dy.transpose(1, 2), stride=s,
                                       padding=p).permute(0, 2, 1)
    torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-12)
    assert (S >= ref.abs() - 1e-12).all()


def test_masks_equal_relu_backward():
    """``add * (add_mask > 0)`` and ``v * (smask > 0)`` are ReLU's backward in torch, at +0.0, -0.0 and negatives too;
    the three mask sources of the generated operands are one mask."""
    c = cc.FWD_CASES[0]
    o = cc.fwd_operands(c)
    for name in ("add_mask", "smask"):
        m = o[name]
        bits = m.view(torch.int16)
        assert (m < 0).any() and (bits == 0).any() and (bits == -32768).any()  # negatives, +0.0 and -0.0 present
        assert 0.3 < (m <= 0).double().mean().item() < 0.7
        a = m.double().requires_grad_(True)
        g, = torch.autograd.grad(torch.relu(a), a, o["add"].double())
        assert torch.equal(g, torch.where(m > 0, o["add"].double(), 0.0))
    acc = torch.ones(o["add"].shape, dtype=torch.float64)
    v, e = cc.fwd_reference(acc, acc, 1, add=o["add"], add_mask=o["add_mask"])
    assert torch.equal(v, 1.0 + torch.where(o["add_mask"] > 0, o["add"].double(), 0.0))
    keeps = [cc.bnb_keep(cc.variant_args(n, o)[4]) for n in ("bnb_smask", "bnb_bits", "bnb_mscale")]
    assert torch.equal(keeps[0], keeps[1]) and torch.equal(keeps[0], keeps[2])
    # the recomputed mask in plain fp32 arithmetic (torch's CPU addcmul) agrees wherever it is not a rounding tie
    f32 = torch.clamp(torch.addcmul(o["mshift"], o["sz"].float(), o["mscale"]), min=0).bfloat16() > 0
    assert (f32 != keeps[2]).double().mean().item() < 1e-3


def test_correct_rounding_needs_two_to_minus_eight():
    """The unit roundoff of bf16 is 2^-8: the correctly rounded reference itself exceeds 2^-9 |v| and never 2^-8 |v|."""
    v = torch.linspace(1.0, 2.0, 100001, dtype=torch.float64)
    rel = ((cc.to_bf16(v).double() - v).abs() / v).max().item()
    assert 2.0 ** -9 < rel <= 2.0 ** -8 == cc.U16


def _cpu_B(c):
    """Samples of the CPU slice: at least 3 (or all), about 1500 output rows."""
    return min(c.B, max(3, 1500 // c.Lout))


@functools.lru_cache(maxsize=None)
def _cpu_case(i):
    c = cc.FWD_CASES[i]
    o = cc.fwd_operands(c, B=_cpu_B(c))
    acc = cc.conv_nlc(o["x"].double(), o["w"].double(), c.stride, c.pad, c.in_dil, c.Lout)
    S = cc.conv_nlc(o["x"].double().abs(), o["w"].double().abs(), c.stride, c.pad, c.in_dil, c.Lout)
    return c, o, acc, S


def _run(i, variant, defect=None):
    c, o, acc, S = _cpu_case(i)
    bias, add, add_mask, relu, bnb, stats = cc.variant_args(variant, o)
    v, e = cc.fwd_reference(acc, S, c.K * c.Cin, bias, add, add_mask, relu, bnb)
    y, st = cc.emulate_fwd(c, o, bias, add, add_mask, relu, bnb, defect)
    r = cc.check_fwd(y, v, e)
    r["stats"] = cc.check_stats(st, y, bnb) if stats else 0.0
    return r


def test_emulation_inside_bound_and_flip_share():
    worst, share, nn = 0.0, 0.0, 0
    for i, c in enumerate(cc.FWD_CASES):
        for variant in cc.VARIANTS:
            r = _run(i, variant)
            assert r["finite"] and r["ratio"] <= 1.0 and r["outside"] == 0 and r["stats"] <= 1.0, (c.name, variant, r)
            worst, share, nn = max(worst, r["ratio"], r["stats"]), max(share, r["flips"]), nn + r["not_neighbour"]
    print(f"fp32 emulation: worst ratio to the bound {worst:.3f}, largest flip share {share:.3e}, "
          f"elements further than one bf16 step from bf16(v): {nn}")
    assert share <= cc.FLIP_SHARE <= 1.25 * share + 1e-5, share  # the constant is the measurement, rounded up
    cap = min(10 * cc.FLIP_SHARE, 1e-2)
    assert abs(cc.FLIP_CAP - cap) <= 0.05 * cap


@pytest.mark.parametrize("defect,variant", [("boundary", "plain"), ("mask_ge", "add_mask"),
                                            ("smean_d", "bnb_szd"), ("smean_d", "bnb_szd_add_mask_smask")])
def test_injected_defect_breaks_the_bound(defect, variant):
    broken = []
    for i, c in enumerate(cc.FWD_CASES):
        r = _run(i, variant, defect)
        if r["ratio"] > 1.0 or r["outside"] > 0 or r["stats"] > 1.0:
            broken.append(c.name)
    print(f"{defect}: breaks the bound on {len(broken)} of {len(cc.FWD_CASES)} cases")
    assert broken
    if defect != "boundary":  # (a K = 1 pad-0 conv reads no row outside its sample)
        assert len(broken) == len(cc.FWD_CASES)


@pytest.mark.parametrize("kernel", cc.WG_KERNELS)
def test_weight_grad_emulation_inside_bound(kernel):
    worst = 0.0
    for c in cc.wgrad_cases(kernel):
        dy, x = cc.wgrad_operands(c)
        ref, S = cc.wgrad_ref(dy, x, c.K, c.stride, c.pad)
        d = dy.float().reshape(-1, c.Cout)
        got = torch.stack([d.T @ xk.reshape(-1, c.Cin) for xk in cc._taps(x.float(), c.K, c.stride, c.pad, 1, c.Lout)], 1)
        e = S * (cc.C_MFMA * c.B * c.Lout * cc.U32)
        worst = max(worst, ((got.double() - ref).abs() / e.clamp_min(1e-300)).max().item())
    print(f"{kernel}: fp32 emulation worst ratio to the bound {worst:.3f}")
    assert worst <= 1.0
