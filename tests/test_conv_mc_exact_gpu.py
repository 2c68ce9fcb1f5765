"""Every kernel family of csrc/kernels/conv1d_mc.hip per element against float64 (tests/conv_mc_cases.py: reference,
derived bound, case tables; tests/test_conv_mc_ref_cpu.py proves those pieces without a kernel).

Each forward / data-grad case asserts the kernel the host dispatch reports for it (``conv_mc.fwd_kernel``), runs all
ten epilogue variants through ``conv_mc.fwd_ex_raw`` and checks every stored element against conditions (1) and (2) of
conv_mc_cases, every statistics column summed over the partial rows against its own bound, the rounding-flip share
against ``FLIP_CAP``, and that the three mask sources of the BatchNorm-backward mode give bitwise the same output.
Each weight-gradient family (``conv_mc.wgrad_kernel``) runs stride 1 and 2, K in {1, 3, 5}, every valid pad, 1, 3 and
the default split count, row counts that are no multiple of 64, Lout < 8 and splits whose last slice is empty or short.

Not covered: the register-staged fallbacks the dispatch takes only when an operand lies beyond the LDS-DMA loops' 32-bit
buffer offsets (above 2 GiB) - ``reg_BMxBN`` forward tiles of undilated convs and the register-staged 128x128 and
256x256 weight-gradient tiles.  (The register-staged forward loop itself runs here through the strided data-grads with
``set_dma_dilated(False)``.)

Observed on an MI355X (worst ratio to the bound over the family's cases and variants: elements / statistics columns;
largest flip share), from profiles/r23/conv_mc_exact_gpu_tests.txt:
forward / data-grad family | runs (cases x variants) | worst element ratio | worst statistics ratio | largest flip share | elements beyond one bf16 step of bf16(v)
  dma_64x64        50   0.967   0.101   9.38e-05   6
  dma_128x128      40   0.993   0.000   8.53e-05   252
  dma_128x64       10   0.981   0.000   6.18e-05   106
  dma_mt_128x64    20   0.992   0.000   6.18e-05   163
  dma_256x256      10   0.992   0.000   3.73e-05   258
  dma_256x128      10   0.993   0.000   3.64e-05   151
  tap128           30   0.962   0.067   8.43e-05   50
  tap64c           20   0.982   0.081   8.13e-05   16
  tap64            30   0.981   0.081   1.41e-04   123
  dgrad_s2_64      30   0.965   0.072   8.27e-05   11
  dgrad_s2_128     30   0.976   0.053   1.30e-04   10
  reg_64x64        20   0.963   0.044   0.00e+00   0
  reg_128x128      20   0.993   0.000   3.98e-05   93
weight-gradient family | cases | worst element ratio
  ts             12 cases  0.012
  dma2           87 cases  0.028
  reg_128x64     87 cases  0.021
  reg_64x128     87 cases  0.027
  reg_64x64      83 cases  0.024
  dma_256x256    87 cases  0.030
The element ratio is the final bf16 rounding (at most 1 for a correctly rounded value); the interval condition held for
every element.  The statistics and weight-gradient bounds grow with the number of summed rows and a correct kernel uses a
few per cent of them (0.000 at 8k-65k rows): they detect structural errors (a dropped row, a swapped mean), not small ones.
"""
import pytest
import torch

import crossscale_ecg  # noqa: F401
import conv_mc_cases as cc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_BNB_ORDER = ("smask", "sz", "smean", "srstd", "szd", "smean_d", "srstd_d", "mscale", "mshift")


class _Toggles:
    """Apply (setter name, value) pairs of ops.conv_mc and restore the previous settings on exit."""

    def __init__(self, toggles):
        self.toggles, self.prev = toggles, []

    def __enter__(self):
        from crossscale_ecg.ops import conv_mc
        for name, val in self.toggles:
            self.prev.append((name, int(getattr(conv_mc, name)(val))))
        return self

    def __exit__(self, *exc):
        from crossscale_ecg.ops import conv_mc
        for name, val in reversed(self.prev):
            getattr(conv_mc, name)(val)
        return False


def _bnb_list(bnb):
    if bnb is None:
        return None, 0
    lst = [bnb.get(k) for k in _BNB_ORDER]
    if "smask_bits" in bnb:
        lst[0] = bnb["smask_bits"]
        return lst, 2
    return lst, 0


@pytest.mark.parametrize("case", cc.FWD_CASES, ids=[c.name for c in cc.FWD_CASES])
def test_forward_family_per_element(case):
    from crossscale_ecg.ops import conv_mc
    c = case
    o = cc.fwd_operands(c, DEV)
    acc = cc.conv_nlc(o["x"].double(), o["w"].double(), c.stride, c.pad, c.in_dil, c.Lout)
    S = cc.conv_nlc(o["x"].double().abs(), o["w"].double().abs(), c.stride, c.pad, c.in_dil, c.Lout)
    shape = (c.B, c.Lin, c.Cin, c.Lout, c.Cout, c.K, c.stride, c.pad, c.in_dil)
    failures, outs = [], {}
    with _Toggles(c.toggles):
        for variant in cc.VARIANTS:
            bias, add, add_mask, relu, bnb, stats = cc.variant_args(variant, o)
            assert conv_mc.fwd_kernel(*shape, stats=stats) == c.kernel
            lst, bits = _bnb_list(bnb)
            _, y, st = conv_mc.fwd_ex_raw(o["x"], o["w"], c.stride, c.pad, c.Lout, c.in_dil, bias, add, add_mask,
                                          relu | bits, lst, stats)
            torch.cuda.synchronize()
            v, e = cc.fwd_reference(acc, S, c.K * c.Cin, bias, add, add_mask, relu, bnb)
            r = cc.check_fwd(y, v, e)
            r["stats"] = 0.0
            if stats:
                assert st.shape == (3 if bnb is not None and "szd" in bnb else 2, conv_mc.stat_rows(*shape), c.Cout)
                r["stats"] = cc.check_stats(st, y, bnb)
            print(f"EXACT fwd | {c.kernel} | {c.name} | {variant} | ratio {r['ratio']:.3f} | stats {r['stats']:.3f} | "
                  f"flips {r['flips']:.2e} | beyond one step {r['not_neighbour']}")
            if not (r["finite"] and r["ratio"] <= 1.0 and r["outside"] == 0 and r["stats"] <= 1.0
                    and r["flips"] <= cc.FLIP_CAP):
                failures.append((variant, r))
            outs[variant] = y
    assert not failures, failures
    assert torch.equal(outs["bnb_smask"], outs["bnb_bits"]) and torch.equal(outs["bnb_smask"], outs["bnb_mscale"])


def test_unsupported_epilogues_are_bad_arguments():
    """An input pre-activation together with the BatchNorm-backward mode, and a fused tail without partial rows, are
    rejected (status 1, nothing launched) on the kernels that take a pre-activation."""
    from crossscale_ecg.ops import _lib, conv_mc
    lib = conv_mc._lib_k()
    for B, L, Cin, Cout, kernel in ((3, 37, 64, 64, "tap64"), (3, 37, 64, 128, "tap128")):
        c = cc._fwd("bad", kernel, B, L, Cin, Cout, 3, 1, 1)
        o = cc.fwd_operands(c, DEV)
        assert conv_mc.fwd_kernel(B, L, Cin, L, Cout, 3, 1, 1, 1, stats=True) == kernel and conv_mc.pre_act_ok(B, L, Cin, Cout)
        y = torch.empty(B, L, Cout, dtype=torch.bfloat16, device=DEV)
        stats = torch.zeros(2, conv_mc.stat_rows(B, L, Cin, L, Cout), Cout, device=DEV)
        sc, sh = torch.ones(Cin, device=DEV), torch.zeros(Cin, device=DEV)
        pa = (_lib.C.c_void_p * 3)(sc.data_ptr(), sh.data_ptr(), None)
        bnb = (_lib.C.c_void_p * 9)(*[_lib.ptr(o.get(k)) if k in ("smask", "sz", "smean", "srstd") else None
                                      for k in _BNB_ORDER])
        args = (B, L, Cin, L, Cout, 3, 1, 1, 1, 0)
        st = lib.ecg_conv1d_nlc_fwd_pa(o["x"].data_ptr(), o["w"].data_ptr(), None, y.data_ptr(), stats.data_ptr(), None,
                                       None, *args, bnb, None, pa, _lib.stream_ptr(y.device))
        assert st == 1
        st = lib.ecg_conv1d_nlc_fwd_pa(o["x"].data_ptr(), o["w"].data_ptr(), None, y.data_ptr(), None, None, None, *args,
                                       None, stats.data_ptr(), None, _lib.stream_ptr(y.device))  # a tail, no stats
        assert st == 1
        st, _, _ = conv_mc.fwd_ex_raw(o["x"], o["w"], 1, 1, L, add_mask=o["add_mask"], check=False)  # mask, no add
        assert st == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("kernel", cc.WG_KERNELS)
def test_weight_gradient_family_per_element(kernel):
    from crossscale_ecg.ops import conv_mc
    cases = cc.wgrad_cases(kernel)
    worst, failures, seen_empty, seen_multi = 0.0, [], False, False
    with _Toggles(cases[0].toggles):
        for c in cases:
            shape = (c.B, c.L, c.Cin, c.Lout, c.Cout, c.K, c.stride, c.pad)
            splits = c.splits if c.splits is not None else conv_mc.wgrad_default_splits(*shape)
            assert conv_mc.wgrad_kernel(splits, *shape) == kernel, (c, conv_mc.wgrad_kernel(splits, *shape))
            R = c.B * c.Lout
            chunks = (R + 63) // 64
            cps = (chunks + splits - 1) // splits
            seen_empty |= (splits - 1) * cps >= chunks
            seen_multi |= c.splits is None and splits > 1
            dy, x = cc.wgrad_operands(c, DEV)
            part = conv_mc.wgrad_parts_raw(dy, x, c.K, c.stride, c.pad, splits)
            dw = conv_mc.wgrad_raw(dy, x, c.K, c.stride, c.pad, splits)
            torch.cuda.synchronize()
            ref, S = cc.wgrad_ref(dy, x, c.K, c.stride, c.pad)
            e = S * (cc.C_MFMA * R * cc.U32)
            got = part.double().sum(0).view(c.Cout, c.K, c.Cin)
            err = (got - ref).abs()
            ratio = torch.where(e > 0, err / e, torch.where(err > 0, float("inf"), 0.0)).max().item()
            worst = max(worst, ratio)
            ok = (part.shape[0] == splits and bool(torch.isfinite(part).all()) and ratio <= 1.0
                  and bool(((dw.double() - got).abs() <= (splits + 1) * cc.U32 * part.double().abs().sum(0).view_as(got)
                            ).all()))
            if not ok:
                failures.append((c, ratio))
    print(f"EXACT wgrad | {kernel} | {len(cases)} cases | worst ratio {worst:.3f}")
    assert not failures, failures
    assert seen_empty and (seen_multi or kernel == "reg_64x64")
