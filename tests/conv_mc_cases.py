"""What tests/test_conv_mc_ref_cpu.py and tests/test_conv_mc_exact_gpu.py share: the float64 references of the NLC conv
entry points (``ecg_conv1d_nlc_fwd_pa`` with its whole epilogue, ``ecg_conv1d_nlc_wgrad``), the per-element bound derived
below, an fp32 emulation of a correct kernel, the operand generator and the case tables.  A plain module (pytest puts
this directory on ``sys.path``); every function works on whatever device its operands live on.

Reference.  All arithmetic in float64 on the bf16 operand values exactly as stored.  ``acc = conv(x, w; stride, pad,
in_dil)`` (``in_dil > 1``: the input is read zero-inserted, as ``load_a_fwd`` does), ``v = acc + bias + add * (add_mask >
0)``, BatchNorm-backward mode ``v = v * mask`` with the mask from ``smask > 0``, from the bits of ``smask_bits`` or from
``bf16(max(fma(sz, mscale, mshift), 0)) > 0``, then the optional ReLU.  The last mask is an operand, not a result, so it
is formed as the kernel forms it: the fma is exact in float64 up to one rounding (a bf16 times an fp32 has 32
significant bits), and a rounding to fp32 and to bf16 changes neither its sign nor whether it is zero.  The statistics
are taken from the kernel's own stored bf16 output ``y``: forward mode ``sum y, sum y^2``; backward mode ``sum y,
sum y * (sz - smean) * srstd`` and, with ``szd``, ``sum y * (szd - smean_d) * srstd_d``.  The weight gradient is
``dw[co, k, ci] = sum_(b,t) dy[b, t, co] * x[b, t * stride + k - pad, ci]``.

Bound, derived and not measured.  A correct kernel stores ``bf16(f)`` with ``f`` an fp32 value: a sum of ``n`` terms
(``n = Kw * Cin``, + 1 for a bias, + 1 for an added tensor), each product of two bf16 values exact in fp32.  Any order
of fp32 additions of n terms misses the exact sum by at most ``(n - 1) * 2^-24 * S`` to first order, ``S`` the sum of
the terms' absolute values (the same conv of ``|x|`` and ``|w|``, plus ``|bias| + |add|``); the MFMA's internal
summation of a 32-step block is unspecified, so the bound takes twice that: ``|f - v| <= e = C_MFMA * n * 2^-24 * S``
with ``C_MFMA = 2``.  Masking and ReLU do not widen it (``|max(f, 0) - max(v, 0)| <= |f - v|``; a masked element is
exactly zero, and its ``e`` is zero).  Rounding to bf16 is monotone and within ``2^-8`` relative (8 significant bits: steps of
``2^-7`` relative, half a step just above a power of two is ``2^-8``), hence for every stored element

    (1)  |got - v| <= 2^-8 * (|v| + e) + e
    (2)  bf16(v - e) <= got <= bf16(v + e)

(``2^-8``, not ``2^-9``, is the unit roundoff of bf16: ``bf16(v)`` itself, the correctly rounded reference, misses
``v`` by up to ``2^-8 |v|`` - tests/test_conv_mc_ref_cpu.py::test_correct_rounding_needs_two_to_minus_eight.  (2) is
the tightest condition a correctly rounding kernel can be held to, and it is asserted on every element.)

(2) implies (1) and is what "``v_bf16`` or a bf16 neighbour of it" has to mean once cancellation makes ``e`` larger than
half a bf16 step of ``v``: there an fp32 sum that is right to within a few of its own ulps lies several bf16 steps
from ``v_bf16`` (about 1e-4 of the elements of a 192-term conv have ``|v| < 1e-4 S``; the fp32 emulation below shows
them too, ``not_neighbour`` in ``check_fwd``'s result).  Where ``e`` is at most half a step, (2) allows ``v_bf16`` and
one neighbour only.  Both are asserted on every element; the share of elements that differ from ``v_bf16`` at all
(rounding flips) is capped by ``FLIP_CAP``.  The fp32 weight gradient is not rounded again: ``|got - dw| <= e`` with
``n = B * Lout``.  A statistics column, summed over the partial rows, is an fp32 sum of ``n`` = rows terms, each term
computed with up to three fp32 roundings: ``|got - ref| <= e`` with ``S = sum |terms|`` (``C_MFMA * n >= n + 2`` covers
the terms' own roundings).  These two bounds grow with ``n`` (a weight gradient over thousands of rows, a statistics
column over 65k rows: 0.8 % of ``sum |terms|``) and a correct kernel uses a few per cent of them: they detect
structural errors - a dropped or doubled row, a swapped mean, a wrong slice - not small ones.

``FLIP_SHARE`` is the largest share of elements at which the fp32 emulation differs from ``v_bf16`` over the forward
case table (tests/test_conv_mc_ref_cpu.py measures it and asserts ``FLIP_CAP == min(10 x FLIP_SHARE, 1 %)`` to two
digits).  The cap is a condition; (1) and (2) are what has teeth.
"""
import dataclasses
from typing import Dict, Optional, Tuple

import torch

C_MFMA = 2.0
U32 = 2.0 ** -24
U16 = 2.0 ** -8   # unit roundoff of bf16 (8 significant bits): half a step of 2^-7 relative
FLIP_SHARE = 1.8e-3   # measured: tests/test_conv_mc_ref_cpu.py::test_emulation_inside_bound_and_flip_share
FLIP_CAP = 1e-2       # min(10 x FLIP_SHARE, 1 %)


# ------------------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class FwdCase:
    name: str
    kernel: str          # what conv_mc.fwd_kernel must report
    B: int
    Lin: int
    Cin: int
    Cout: int
    K: int
    stride: int
    pad: int
    in_dil: int
    Lout: int
    toggles: Tuple[Tuple[str, int], ...] = ()   # (conv_mc setter name, value), restored by the test
    seed: int = 0

    @property
    def M(self):
        return self.B * self.Lout


def _fwd(name, kernel, B, L, Cin, Cout, K, s, p, toggles=(), seed=0):
    return FwdCase(name, kernel, B, L, Cin, Cout, K, s, p, 1, (L + 2 * p - K) // s + 1, tuple(toggles), seed)


def _dgrad(name, kernel, B, L, Cin_f, Cout_f, K, s, p, toggles=(), seed=0):
    """The data-grad call of the forward conv (B, L, Cin_f -> Cout_f, K, s, p): dy [B, Lo, Cout_f] read with input
    dilation s, flipped taps (the weight is random anyway), pad K-1-p, output length L, Cin_f output channels."""
    Lo = (L + 2 * p - K) // s + 1
    return FwdCase(name, kernel, B, Lo, Cout_f, Cin_f, K, 1, K - 1 - p, s, L, tuple(toggles), seed)


_NO_TAP64 = (("set_tap64", 0),)
_TAP2 = (("set_tap_shared", 2), ("set_tap64", 0))
_PHASE = (("set_tap_s2", 0),)
_PHASE_REG = (("set_tap_s2", 0), ("set_dma_dilated", 0))

# M = B * Lout thresholds of pick_fwd_tile (mt128 = ceil(M / 128), mt256 = ceil(M / 256)):
#   128x128: Cout % 128 == 0 and mt128 * Cout/128 >= 256        -> Cout 512: M >= 63 * 128 + 1 = 8065
#   128x64 : mt128 * Cout/64 >= 512                              -> Cout 320: M >= 102 * 128 + 1 = 13057 (515 tiles > 512
#            workgroup slots: the multi-tile kernel unless set_multi_tile(0))
#   128x64 multi-tile mode 2: Cout == 128 and 2 * mt128 > 512    -> M >= 256 * 128 + 1 = 32769
#   256x256: Cout % 256 == 0 and mt256 * Cout/256 >= 512         -> Cout 512: M >= 255 * 256 + 1 = 65281
#   256x128: family 2, Cout % 128 == 0, mt256 * Cout/128 >= 512  -> Cout 384: M >= 170 * 256 + 1 = 43521
# Every M below leaves a ragged last tile and every Lout is no multiple of 16 (a sample boundary inside a fragment).
FWD_CASES = [
    _fwd("64x64 one ragged tile, s2", "dma_64x64", 2, 9, 64, 64, 3, 2, 1),
    _fwd("64x64 two tiles, K5", "dma_64x64", 3, 37, 64, 192, 5, 1, 2),
    _fwd("64x64 s2 odd remainder", "dma_64x64", 3, 34, 128, 128, 1, 2, 0),
    _fwd("128x128 K1 s2 odd remainder", "dma_128x128", 37, 438, 64, 512, 1, 2, 0),
    _fwd("128x128 K3 s2 odd remainder", "dma_128x128", 37, 438, 128, 512, 3, 2, 1),
    _fwd("128x64 one tile per workgroup", "dma_128x64", 53, 247, 64, 320, 3, 1, 1, (("set_multi_tile", 0),)),
    _fwd("128x64 multi-tile", "dma_mt_128x64", 53, 247, 64, 320, 3, 1, 1),
    _fwd("128x64 multi-tile mode 2", "dma_mt_128x64", 131, 502, 64, 128, 1, 2, 0, (("set_multi_tile", 2),)),
    _fwd("256x256", "dma_256x256", 257, 255, 64, 512, 1, 1, 0),
    _fwd("256x128", "dma_256x128", 173, 253, 64, 384, 1, 1, 0, (("set_tile_family", 2),)),
    _fwd("tap128 L=2", "tap128", 7, 2, 128, 256, 3, 1, 1),
    _fwd("tap128 ragged", "tap128", 3, 37, 64, 128, 3, 1, 1),
    _fwd("tap128 multi-tile", "tap128", 300, 63, 128, 128, 3, 1, 1),
    _fwd("tap64c L=2", "tap64c", 7, 2, 64, 64, 3, 1, 1, _TAP2),
    _fwd("tap64c multi-tile", "tap64c", 40, 125, 64, 64, 3, 1, 1, _TAP2),
    _fwd("tap64 L=2", "tap64", 7, 2, 64, 64, 3, 1, 1),
    _fwd("tap64 ragged", "tap64", 3, 37, 64, 64, 3, 1, 1),
    _fwd("tap64 persistent", "tap64", 700, 125, 64, 64, 3, 1, 1),
    _dgrad("dgrad_s2_64 L=2", "dgrad_s2_64", 5, 3, 64, 128, 3, 2, 1),
    _dgrad("dgrad_s2_64 ragged even", "dgrad_s2_64", 3, 126, 64, 128, 3, 2, 1),
    _dgrad("dgrad_s2_64 multi-tile", "dgrad_s2_64", 64, 125, 64, 128, 3, 2, 1),
    _dgrad("dgrad_s2_128 L=2 even", "dgrad_s2_128", 5, 4, 128, 64, 3, 2, 1),
    _dgrad("dgrad_s2_128 even", "dgrad_s2_128", 2, 30, 256, 512, 3, 2, 1),
    _dgrad("dgrad_s2_128 multi-tile odd", "dgrad_s2_128", 37, 63, 128, 256, 3, 2, 1),
    _dgrad("phase 64x64 K3 odd", "dma_64x64", 2, 9, 64, 64, 3, 2, 1, _PHASE),
    _dgrad("phase 64x64 K1 even", "dma_64x64", 3, 8, 64, 64, 1, 2, 0, _PHASE),
    _dgrad("phase 128x128 K1 odd", "dma_128x128", 37, 219, 512, 64, 1, 2, 0, _PHASE),
    _dgrad("phase 128x128 K3 even", "dma_128x128", 37, 220, 512, 64, 3, 2, 1, _PHASE),
    _dgrad("phase reg 64x64 K3 odd", "reg_64x64", 2, 9, 64, 64, 3, 2, 1, _PHASE_REG),
    _dgrad("phase reg 64x64 K1 even", "reg_64x64", 3, 8, 64, 64, 1, 2, 0, _PHASE_REG),
    _dgrad("phase reg 128x128 K1 odd", "reg_128x128", 37, 219, 512, 64, 1, 2, 0, _PHASE_REG),
    _dgrad("phase reg 128x128 K3 even", "reg_128x128", 37, 220, 512, 64, 3, 2, 1, _PHASE_REG),
]

VARIANTS = ("plain", "bias_relu", "stats", "add", "add_mask", "bnb_smask", "bnb_bits", "bnb_mscale", "bnb_szd",
            "bnb_szd_add_mask_smask")


@dataclasses.dataclass(frozen=True)
class WgCase:
    kernel: str
    B: int
    L: int
    Cin: int
    Cout: int
    K: int
    stride: int
    pad: int
    splits: Optional[int]   # None: the default plan
    toggles: Tuple[Tuple[str, int], ...] = ()

    @property
    def Lout(self):
        return (self.L + 2 * self.pad - self.K) // self.stride + 1


_WG_FAMILIES = {  # kernel: (Cin, Cout, toggles)
    "dma2": (128, 128, ()),
    "reg_128x64": (64, 128, ()),
    "reg_64x128": (128, 64, ()),
    "reg_64x64": (64, 64, ()),
    "dma_256x256": (256, 256, (("set_tile_family", 2),)),
}
_WG_KP = [(1, 0), (3, 0), (3, 1), (3, 2), (5, 0), (5, 1), (5, 2)]


def wgrad_cases(kernel: str):
    """The weight-gradient cases of one kernel family.  Shapes: (3, ~70 output rows) - 4 row chunks of 64, the last
    ragged, so 3 splits leave the last slice empty; (5 samples, Lout < 8); one shape with 5 chunks (3 splits: a short
    last slice) and one whose default plan has several splits.  Stride 2 lengths alternate the parity of L + 2p - K."""
    if kernel == "ts":  # stride-1 pad-1 3-tap, Lout >= 8, at most 64 channels
        shapes = [(3, 70), (5, 8), (4, 75), (64, 125)]
        return [WgCase("ts", B, L, 64, 64, 3, 1, 1, sp) for B, L in shapes for sp in (1, 3, None)]
    Cin, Cout, tog = _WG_FAMILIES[kernel]
    out = []
    for s in (1, 2):
        for i, (K, p) in enumerate(_WG_KP):
            if kernel == "reg_64x64" and (K, s, p) == (3, 1, 1):
                lens = [(5, 7)]  # Lout < 8: the only stride-1 pad-1 3-tap shape the tap-shared kernel leaves
            else:
                lo = 70
                L70 = (lo - 1) * s + K - 2 * p + (i % 2 if s == 2 else 0)
                L7 = (7 - 1) * s + K - 2 * p + ((i + 1) % 2 if s == 2 else 0)
                lens = [(3, L70), (5, L7)]
            for B, L in lens:
                for sp in (1, 3, None):
                    out.append(WgCase(kernel, B, L, Cin, Cout, K, s, p, sp, tog))
    out.append(WgCase(kernel, 4, 75 * 2, Cin, Cout, 3, 2, 1, 3, tog))       # 5 chunks over 3 splits: short last slice
    out.append(WgCase(kernel, 64, 125 * 2 + 1, Cin, Cout, 3, 2, 1, None, tog))  # default plan with several splits
    if kernel != "reg_64x64":
        out.append(WgCase(kernel, 64, 125, Cin, Cout, 3, 1, 1, None, tog))
    return out


WG_KERNELS = ("ts",) + tuple(_WG_FAMILIES)


# --------------------------------------------------------------------------------------------------- operands
def _bf16_randn(shape, gen, device, scale=1.0):
    return (torch.randn(shape, generator=gen, device=device) * scale).bfloat16()


def _mask_like(shape, gen, device):
    """bf16 values, about half of them <= 0: negatives, +0.0 and -0.0 among them."""
    m = torch.randn(shape, generator=gen, device=device)
    r = torch.rand(shape, generator=gen, device=device)
    m = torch.where((m <= 0) & (r < 0.25), torch.zeros_like(m), m)
    m = torch.where((m <= 0) & (r >= 0.25) & (r < 0.5), -torch.zeros_like(m), m)
    return m.bfloat16()


def fwd_operands(c: FwdCase, device="cpu", B: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Seeded operands of one forward case (``B``: fewer samples - a slice of the rows for the CPU).  ``smask`` is the
    activation ``bf16(max(fma(sz, mscale, mshift), 0))`` with its zeros replaced by negatives, +0.0 and -0.0, and
    ``smask_bits`` its ``> 0`` bits, so that the three mask sources describe one mask."""
    B = c.B if B is None else B
    g = torch.Generator(device=device).manual_seed(1000 + c.seed)
    out_shape = (B, c.Lout, c.Cout)
    o = dict(
        x=_bf16_randn((B, c.Lin, c.Cin), g, device),
        w=_bf16_randn((c.Cout, c.K, c.Cin), g, device, (c.K * c.Cin) ** -0.5),
        bias=torch.randn(c.Cout, generator=g, device=device),
        add=_bf16_randn(out_shape, g, device),
        add_mask=_mask_like(out_shape, g, device),
        sz=_bf16_randn(out_shape, g, device),
        szd=_bf16_randn(out_shape, g, device),
        smean=torch.randn(c.Cout, generator=g, device=device) * 0.3,
        srstd=torch.rand(c.Cout, generator=g, device=device) + 0.5,
        smean_d=torch.randn(c.Cout, generator=g, device=device) * 0.3 + 1.0,
        srstd_d=torch.rand(c.Cout, generator=g, device=device) + 1.5,
        mscale=(torch.rand(c.Cout, generator=g, device=device) + 0.5)
        * torch.where(torch.rand(c.Cout, generator=g, device=device) < 0.25, -1.0, 1.0),
        mshift=torch.randn(c.Cout, generator=g, device=device) * 0.3,
    )
    keep = mask_from_sz(o["sz"], o["mscale"], o["mshift"])
    act = torch.clamp(o["sz"].double() * o["mscale"].double() + o["mshift"].double(), min=0).float().bfloat16()
    r = torch.rand(out_shape, generator=g, device=device)
    off = -torch.randn(out_shape, generator=g, device=device).abs() - 2.0 ** -100  # dropped: negative, +0.0 or -0.0
    off = torch.where(r < 1 / 3, torch.zeros_like(off), torch.where(r < 2 / 3, -torch.zeros_like(off), off))
    o["smask"] = torch.where(keep, act, off.bfloat16())
    assert torch.equal(o["smask"] > 0, keep)
    o["smask_bits"] = pack_bits(keep)
    return o


def mask_from_sz(sz, mscale, mshift):
    """``bf16(max(fma(sz, mscale, mshift), 0)) > 0`` as the kernel forms it (module docstring)."""
    f = (sz.double() * mscale.double() + mshift.double()).float()  # fp32 fma: one rounding of the exact value
    return torch.clamp(f, min=0).bfloat16() > 0


def pack_bits(keep):
    """Byte i holds element 8 i + e in bit e (FwdArgs::smask_bits)."""
    k = keep.reshape(-1, 8).to(torch.int32)
    wgt = (2 ** torch.arange(8, device=keep.device, dtype=torch.int32))
    return (k * wgt).sum(1).to(torch.uint8)


def wgrad_operands(c: WgCase, device="cpu"):
    g = torch.Generator(device=device).manual_seed(2000 + c.B * 131 + c.L * 7 + c.K + c.stride + c.pad)
    return (_bf16_randn((c.B, c.Lout, c.Cout), g, device), _bf16_randn((c.B, c.L, c.Cin), g, device))


# ------------------------------------------------------------------------------------------------- references
def _taps(x, K, stride, pad, in_dil, Lout, leak=False):
    """The K operand row sets of the conv: [K][B, Lout, Cin], row t of tap k = x_dilated[t * stride + k - pad] or zero.
    ``leak`` (an injected defect): a position outside the sample reads the neighbouring sample's row instead."""
    B, Lin, Cin = x.shape
    Ld = (Lin - 1) * in_dil + 1
    need = (Lout - 1) * stride + K  # padded positions 0 .. need-1  <->  dilated positions -pad .. need-1-pad
    if leak:
        flat = torch.zeros(B * Ld + 2 * need + 2 * pad, Cin, dtype=x.dtype, device=x.device)
        body = torch.zeros(B, Ld, Cin, dtype=x.dtype, device=x.device)
        body[:, ::in_dil] = x
        flat[need + pad:need + pad + B * Ld] = body.reshape(B * Ld, Cin)
        idx = (torch.arange(B, device=x.device)[:, None] * Ld + torch.arange(Lout, device=x.device)[None] * stride
               + need)  # + k: flat row of (b, t, k)
        return [flat[idx + k] for k in range(K)]
    xp = torch.zeros(B, max(need, pad + Ld), Cin, dtype=x.dtype, device=x.device)
    xp[:, pad:pad + Ld:in_dil] = x
    return [xp[:, k:k + (Lout - 1) * stride + 1:stride] for k in range(K)]


def conv_nlc(x, w, stride, pad, in_dil, Lout, leak=False):
    """Plain tap loop in the operands' dtype: x [B, Lin, Cin], w [Cout, K, Cin] -> [B, Lout, Cout]."""
    acc = None
    for k, xk in enumerate(_taps(x, w.shape[1], stride, pad, in_dil, Lout, leak)):
        t = xk @ w[:, k, :].T
        acc = t if acc is None else acc + t
    return acc


def wgrad_ref(dy, x, K, stride, pad):
    """dw [Cout, K, Cin] float64 and the same sum of absolute values."""
    Lout = dy.shape[1]
    d, xs = dy.double().reshape(-1, dy.shape[2]), x.double()
    dw = torch.stack([d.T @ xk.reshape(-1, x.shape[2]) for xk in _taps(xs, K, stride, pad, 1, Lout)], 1)
    S = torch.stack([d.abs().T @ xk.reshape(-1, x.shape[2]) for xk in _taps(xs.abs(), K, stride, pad, 1, Lout)], 1)
    return dw, S


def variant_args(variant: str, o: Dict[str, torch.Tensor]):
    """(bias, add, add_mask, relu bit, bnb dict or None, stats) of an epilogue variant."""
    bnb = None
    if variant.startswith("bnb"):
        bnb = dict(sz=o["sz"], smean=o["smean"], srstd=o["srstd"])
        if variant == "bnb_bits":
            bnb["smask_bits"] = o["smask_bits"]
        elif variant == "bnb_mscale":
            bnb.update(mscale=o["mscale"], mshift=o["mshift"])
        else:
            bnb["smask"] = o["smask"]
        if "szd" in variant:
            bnb.update(szd=o["szd"], smean_d=o["smean_d"], srstd_d=o["srstd_d"])
    add = o["add"] if variant in ("add", "add_mask", "bnb_szd_add_mask_smask") else None
    add_mask = o["add_mask"] if variant in ("add_mask", "bnb_szd_add_mask_smask") else None
    bias = o["bias"] if variant == "bias_relu" else None
    return bias, add, add_mask, int(variant == "bias_relu"), bnb, variant == "stats" or bnb is not None


def bnb_keep(bnb):
    if "mscale" in bnb:
        return mask_from_sz(bnb["sz"], bnb["mscale"], bnb["mshift"])
    if "smask_bits" in bnb:
        b = bnb["smask_bits"].to(torch.int32)
        e = torch.arange(8, device=b.device, dtype=torch.int32)
        return ((b[:, None] >> e) & 1).bool().reshape(bnb["sz"].shape)
    if "smask" in bnb:
        return bnb["smask"] > 0
    return None


def fwd_reference(acc, S, n_conv, bias=None, add=None, add_mask=None, relu=0, bnb=None):
    """(v, e) in float64 from the float64 conv ``acc`` and its absolute-value twin ``S`` (module docstring)."""
    v, s, n = acc.clone(), S.clone(), n_conv
    if bias is not None:
        v += bias.double()
        s += bias.double().abs()
        n += 1
    if add is not None:
        a = add.double() if add_mask is None else torch.where(add_mask > 0, add.double(), 0.0)
        v += a
        s += a.abs()
        n += 1
    e = s * (C_MFMA * n * U32)
    keep = bnb_keep(bnb) if bnb is not None else None
    if keep is not None:
        v, e = torch.where(keep, v, 0.0), torch.where(keep, e, 0.0)
    if relu:
        v = torch.clamp(v, min=0)
    return v, e


def to_bf16(v64):
    return v64.float().bfloat16()


def _bf16_ord(t):
    """bf16 bit patterns as integers ordered like the values (+0 and -0 both 0)."""
    b = t.view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def check_fwd(got, v, e):
    """Conditions (1) and (2) of the module docstring on every element of the stored bf16 ``got``.  Returns a dict:
    ``ratio`` = worst |got - v| / bound (1), ``outside`` = elements outside interval (2), ``flips`` = share of elements
    that differ from bf16(v), ``not_neighbour`` = elements further than one bf16 step from bf16(v)."""
    g = got.double()
    bound = U16 * (v.abs() + e) + e
    err = (g - v).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, float("inf"), 0.0)).max().item()
    slack = v.abs() * 2.0 ** -22  # the float64 -> fp32 -> bf16 conversion rounds twice: step outwards first
    lo, hi = to_bf16(v - e - slack).double(), to_bf16(v + e + slack).double()
    outside = int(((g < lo) | (g > hi)).sum().item())
    vb = to_bf16(v)
    steps = (_bf16_ord(got) - _bf16_ord(vb)).abs()
    return dict(ratio=ratio, outside=outside, flips=(steps != 0).double().mean().item(),
                not_neighbour=int((steps > 1).sum().item()), finite=bool(torch.isfinite(got).all().item()))


def stats_reference(y, bnb=None, swap_mean_d=False):
    """Float64 statistics columns [2 or 3, Cout] of the stored bf16 output ``y`` and their term-magnitude sums.
    ``swap_mean_d`` (an injected defect): ``smean`` where the third column needs ``smean_d``."""
    C = y.shape[-1]
    yd = y.double().reshape(-1, C)
    if bnb is None:
        terms = [yd, yd * yd]
    else:
        terms = [yd, yd * (bnb["sz"].double().reshape(-1, C) - bnb["smean"].double()) * bnb["srstd"].double()]
        if "szd" in bnb:
            mu = bnb["smean"] if swap_mean_d else bnb["smean_d"]
            terms.append(yd * (bnb["szd"].double().reshape(-1, C) - mu.double()) * bnb["srstd_d"].double())
    return torch.stack([t.sum(0) for t in terms]), torch.stack([t.abs().sum(0) for t in terms])


def check_stats(stats, y, bnb=None):
    """Worst |sum over partial rows - reference| / e over the statistics columns (module docstring); inf if the
    partial rows are not finite."""
    ref, S = stats_reference(y, bnb)
    n = y.numel() // y.shape[-1]
    e = S * (C_MFMA * n * U32)
    err = (stats.double().sum(1) - ref).abs()
    if stats.shape[0] != ref.shape[0] or not torch.isfinite(stats).all():
        return float("inf")
    return torch.where(e > 0, err / e, torch.where(err > 0, float("inf"), 0.0)).max().item()


# -------------------------------------------------------------------------------------------- fp32 emulation
def emulate_fwd(c: FwdCase, o, bias=None, add=None, add_mask=None, relu=0, bnb=None, defect=None):
    """What a correct kernel computes, in fp32: fp32 matmuls of the bf16 operands per tap, the epilogue in fp32 in the
    kernel's order, rounding to bf16; the statistics columns in fp32 from the rounded values.  ``defect``: None,
    ``"boundary"`` (a row outside the sample reads the neighbouring sample), ``"mask_ge"`` (``>= 0`` for ``> 0`` in the
    add mask) or ``"smean_d"`` (``smean`` for ``smean_d`` in the third statistic)."""
    v = conv_nlc(o["x"].float(), o["w"].float(), c.stride, c.pad, c.in_dil, c.Lout, leak=defect == "boundary")
    if bias is not None:
        v = v + bias
    if add is not None:
        if add_mask is None:
            v = v + add.float()
        else:
            m = add_mask.float() >= 0 if defect == "mask_ge" else add_mask.float() > 0
            v = v + torch.where(m, add.float(), 0.0)
    keep = bnb_keep(bnb) if bnb is not None else None
    if keep is not None:
        v = torch.where(keep, v, 0.0)
    if relu:
        v = torch.clamp(v, min=0)
    y = v.bfloat16()
    yf = y.float().reshape(-1, c.Cout)
    if bnb is None:
        cols = [yf.sum(0), (yf * yf).sum(0)]
    else:
        cols = [yf.sum(0), (yf * (bnb["sz"].float().reshape(-1, c.Cout) - bnb["smean"]) * bnb["srstd"]).sum(0)]
        if "szd" in bnb:
            mu = bnb["smean"] if defect == "smean_d" else bnb["smean_d"]
            cols.append((yf * (bnb["szd"].float().reshape(-1, c.Cout) - mu) * bnb["srstd_d"]).sum(0))
    return y, torch.stack(cols)[:, None, :]
