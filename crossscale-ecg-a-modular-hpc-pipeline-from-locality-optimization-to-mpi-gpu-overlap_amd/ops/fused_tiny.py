"""Fused TinyECG training / inference on gfx950 (Python side of csrc/kernels/tiny_ecg_step.hip).

Each workgroup computes one sample's forward+backward out of LDS.  The bf16 kernels keep no copy of the window
there: every wave builds its conv1 operand in registers from bounded loads of the window row in global memory
(the fp32 kernel stages the window in LDS for its VALU conv1).  ``FusedTinyTrainer`` runs a whole FedAvg
local round as two launches per step (gradient slab, then slab reduction + SGD), captured into one native hipGraph
and replayed with a single ``hipGraphLaunch`` per round.  (A one-launch step with an in-kernel reduction tree and a
persistent one-launch round were measured slower on MI355X and removed in round 5: profiles/r4/tiny_phase_diag.txt.)

Reference semantics per step: Module_3/TRUE_FL_M3/part3_fedavg_overlap_mpi_gpu.py:103-132
(train_step_G0/G1), batches as Module_3/shard_dataset.py:118-136, optimizer SGD(lr=1e-2, momentum=0.9).
Differences: bf16 MFMA operands with fp32 accumulation (AMP numerics without a GradScaler), the loss is
accumulated on the device and read once per round (the reference syncs + ``loss.item()`` every step).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib
from ..models.tiny_ecg import TinyECG, num_params
from ..data.dataset import DeviceIndexSampler
from ..utils.philox import mix64
from .tiny_eval import EvalResult, TinyEvaluator, evaluate_torch, tiny_evaluate  # noqa: F401  (evaluation: ops/tiny_eval.py)


PRECISION = {"bf16": 0, "fp32": 1}


def prec_id(precision: str) -> int:
    if precision not in PRECISION:
        raise ValueError(f"precision must be one of {list(PRECISION)}, got {precision!r}")
    return PRECISION[precision]


def new_wprep(device) -> torch.Tensor:
    """Device buffer for the prepared-fragment image (bf16 conv operands of the flat weights, MFMA lane order).
    Zero-initialised: the K-padding slots are never written by the SGD epilogue that keeps the image current."""
    return torch.zeros(_lib.kernels().ecg_tiny_wprep_bytes(), dtype=torch.uint8, device=device)


def _wprep_ptr(precision: str, prefrag: bool, device, wprep: Optional[torch.Tensor] = None):
    """Prepared fragments (PF) are the bf16 default; ``prefrag=False`` builds the conv operands in LDS every step.
    Both paths are bitwise identical (csrc/kernels/tiny_ecg_step.hip WP_* comment)."""
    if precision != "bf16" or not prefrag:
        return None, None
    w = new_wprep(device) if wprep is None else wprep
    return w.data_ptr(), w


def slab_stride(num_classes: int) -> int:
    return (num_params(num_classes) + 1 + 63) // 64 * 64


def _check_dataset(x: torch.Tensor, y: Optional[torch.Tensor], num_classes: int):
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1:
        raise ValueError(f"dataset must be a CUDA float32 [N, L] tensor with unit stride, got "
                         f"{x.dtype} {tuple(x.shape)} stride {x.stride()} on {x.device}")
    if y is not None:
        if y.dtype != torch.int32 or y.dim() != 1 or y.shape[0] != x.shape[0] or y.device != x.device:
            raise ValueError("labels must be int32 [N] on the dataset's device")


def _check_idx(idx: torch.Tensor, B: int, N: int, device):
    if idx.dtype != torch.int32 or idx.numel() < B or idx.device != device or not idx.is_contiguous():
        raise ValueError("idx must be a contiguous int32 device tensor with >= B entries")


def labels_int32(y: torch.Tensor, num_classes: int) -> torch.Tensor:
    y32 = y.to(torch.int32).contiguous()
    if y32.numel():
        lo, hi = int(y32.min()), int(y32.max())
        if lo < 0 or hi >= num_classes:
            raise ValueError(f"labels must be in [0, {num_classes}), got [{lo}, {hi}]")
    return y32


def tiny_forward(flat_params: torch.Tensor, x: torch.Tensor, idx: Optional[torch.Tensor], batch: int,
                 num_classes: int = 2, precision: str = "bf16", prefrag: bool = True) -> torch.Tensor:
    """Logits [batch, C] of TinyECG for windows ``x[idx[b]]`` (or ``x[b]`` when idx is None).  ``prefrag``: build
    the prepared-fragment image first and run the PF kernel (bf16 only)."""
    _check_dataset(x, None, num_classes)
    if idx is not None:
        _check_idx(idx, batch, x.shape[0], x.device)
    elif batch > x.shape[0]:
        raise ValueError("batch larger than dataset")
    out = torch.empty((batch, num_classes), dtype=torch.float32, device=x.device)
    lib = _lib.kernels()
    wp, _keep = _wprep_ptr(precision, prefrag, x.device)
    st = lib.ecg_tiny_forward(x.data_ptr(), x.shape[1], x.stride(0), _lib.ptr(idx), flat_params.data_ptr(),
                              num_classes, out.data_ptr(), batch, prec_id(precision), wp, _lib.stream_ptr(x.device))
    _lib.check(st, "ecg_tiny_forward")
    return out


def tiny_step_grads(flat_params: torch.Tensor, x: torch.Tensor, y32: torch.Tensor, idx: Optional[torch.Tensor],
                    batch: int, num_classes: int = 2, slab: Optional[torch.Tensor] = None,
                    precision: str = "bf16", prefrag: bool = True,
                    wprep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-sample gradient slab [batch, stride] (loss in column P) of one fused step (no update).  ``prefrag``:
    rebuild the prepared-fragment image (``wprep``, or a temporary) from the weights and run the PF kernel."""
    _check_dataset(x, y32, num_classes)
    if idx is not None:
        _check_idx(idx, batch, x.shape[0], x.device)
    stride = slab_stride(num_classes)
    if slab is None:
        slab = torch.empty((batch, stride), dtype=torch.float32, device=x.device)
    lib = _lib.kernels()
    wp, _keep = _wprep_ptr(precision, prefrag, x.device, wprep)
    st = lib.ecg_tiny_step_grads(x.data_ptr(), x.shape[1], x.stride(0), _lib.ptr(idx), y32.data_ptr(),
                                 flat_params.data_ptr(), num_classes, slab.data_ptr(), stride, batch,
                                 1.0 / batch, prec_id(precision), wp, _lib.stream_ptr(x.device))
    _lib.check(st, "ecg_tiny_step_grads")
    return slab


# ``FusedTinyTrainer(prepack=...)``: what a round does with the dataset packed once (TinyRound.prepack).  The default
# is set by measurement (profiles/r15/tiny_prepacked.txt: 9.76-9.81 us/step unpacked, 9.58-9.64 gather, 9.45-9.52
# direct); ECG_TINY_PREPACK=none|gather|direct overrides it for a process (A/B runs of an unchanged driver), an
# explicit argument overrides both.  A caller that sets ``gather=`` or ``pack=`` itself asks for that gather-based
# round and its buffers, so the default then is "none".
PREPACK_DEFAULT = "direct"
# Largest share of the device's free memory the packed shard may take (it is about 0.52 of the fp32 shard at L = 500);
# above it the trainer keeps the unpacked path.  A quarter leaves the 64 GB resident runs (33 GB packed, 288 GB HBM)
# their packed copy and refuses it where the shard itself already fills half of what is free.
PREPACK_SHARE = 0.25


def _prepack_variant(prepack, explicit_gather: bool = False) -> str:
    if prepack is None:
        prepack = "none" if explicit_gather else os.environ.get("ECG_TINY_PREPACK") or PREPACK_DEFAULT
    if prepack is True:
        prepack = "gather" if PREPACK_DEFAULT == "none" else PREPACK_DEFAULT  # (the cheaper form if none is default)
    if prepack is False:
        prepack = "none"
    if prepack not in _lib.PREPACK:
        raise ValueError(f"prepack must be a bool or one of {list(_lib.PREPACK)}, got {prepack!r}")
    return prepack


def pack_dataset(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The windows ``x`` [N, L] as packed bf16 rows [N, ldb]: 4 zeros, bf16(x[n]), zeros up to ldb = L rounded up to
    32, plus 8 - the rows the packed step kernel reads (csrc/kernels/tiny_ecg_step.hip kPackLead).  Every element of
    ``out``, pads included, is written."""
    _check_dataset(x, None, 0)
    lib = _lib.kernels()
    N, L = x.shape
    ldb = lib.ecg_tiny_pack_halfs(L, 1)
    if out is None:
        out = torch.empty((N, ldb), dtype=torch.bfloat16, device=x.device)
    if out.shape != (N, ldb) or out.dtype != torch.bfloat16 or not out.is_contiguous() or out.device != x.device:
        raise ValueError(f"packed rows must be a contiguous bfloat16 [{N}, {ldb}] tensor on the dataset's device")
    _lib.check(lib.ecg_tiny_pack_dataset(x.data_ptr(), x.stride(0), N, L, out.data_ptr(), _lib.stream_ptr(x.device)),
               "ecg_tiny_pack_dataset")
    return out


def check_dp_args(dp_clip: float, dp_noise: float) -> None:
    if not dp_clip >= 0.0 or not dp_noise >= 0.0:
        raise ValueError(f"dp_clip and dp_noise must be >= 0, got {dp_clip} and {dp_noise}")
    if dp_noise > 0.0 and dp_clip == 0.0:
        raise ValueError("dp_noise > 0 needs a clip norm (dp_clip > 0): the noise is scaled by it")


def check_prox_args(prox_mu: float, dp_clip: float = 0.0) -> None:
    if not prox_mu >= 0.0:
        raise ValueError(f"prox_mu must be >= 0, got {prox_mu}")
    if prox_mu > 0.0 and dp_clip > 0.0:
        raise ValueError("FedProx (prox_mu > 0) is not combined with DP-SGD (dp_clip > 0): the DP reduce has no "
                         "proximal term")


def dp_reduce_slab(slab: torch.Tensor, dp_clip: float, dp_noise: float, dp_seed: int, dp_step: torch.Tensor,
                   num_classes: int = 2):
    """DP-SGD sum of a gradient slab without an update: returns (grad [P], loss_sum [1], clip factors [B]) where
    ``grad = sum_b c_b * slab[b] + dp_noise * dp_clip / B * z(dp_seed, t)``, ``t`` the value of ``dp_step`` (int64
    device word) before the call; the call advances it by one.  The loss column is neither clipped nor noised."""
    P = num_params(num_classes)
    grad = torch.empty(P, dtype=torch.float32, device=slab.device)
    loss = torch.zeros(1, dtype=torch.float32, device=slab.device)
    scale = torch.empty(slab.shape[0], dtype=torch.float32, device=slab.device)
    st = _lib.kernels().ecg_slab_reduce_dp_sgd(
        slab.data_ptr(), slab.shape[0], slab.stride(0), P, None, None, grad.data_ptr(), loss.data_ptr(), 0.0, 0.0, 0.0,
        0, 0, None, dp_clip, dp_noise, int(dp_seed) & (2 ** 64 - 1), scale.data_ptr(), dp_step.data_ptr(),
        _lib.stream_ptr(slab.device))
    _lib.check(st, "ecg_slab_reduce_dp_sgd")
    return grad, loss, scale


def dp_noise(P: int, seed: int, t: int, device) -> torch.Tensor:
    """Diagnostic: the standard normals z [P] the DP reduce draws for (seed, step t)."""
    z = torch.empty(P, dtype=torch.float32, device=device)
    st = _lib.kernels().ecg_dp_noise(z.data_ptr(), P, int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1),
                                     _lib.stream_ptr(z.device))
    _lib.check(st, "ecg_dp_noise")
    return z


def reduce_slab(slab: torch.Tensor, num_classes: int = 2):
    """Sum a gradient slab: returns (grad [P], loss_sum [1]) without applying an update."""
    P = num_params(num_classes)
    grad = torch.empty(P, dtype=torch.float32, device=slab.device)
    loss = torch.zeros(1, dtype=torch.float32, device=slab.device)
    lib = _lib.kernels()
    st = lib.ecg_slab_reduce_sgd(slab.data_ptr(), slab.shape[0], slab.shape[1], P, None, None, grad.data_ptr(),
                                 loss.data_ptr(), 0.0, 0.0, 0.0, 0, 0, None, _lib.stream_ptr(slab.device))
    _lib.check(st, "ecg_slab_reduce_sgd")
    return grad, loss


class FusedTinyTrainer:
    """Single-GPU local trainer for TinyECG on the fused HIP step (one FL client).

    ``model`` is flattened in place: its parameters become views of ``self.params`` so that
    ``state_dict()`` / FedAvg collectives operate on the very buffer the kernels update.

    ``prefrag`` / ``gather`` (bf16 only): prepared fragments - a round's first step builds its conv operands in LDS
    (the weights may have been rewritten since: FedAvg, broadcast, checkpoint) and its SGD epilogue rewrites the
    whole image, which every later step of the round reads; ``gather`` (needs ``prefrag``) - every step's windows
    and labels are gathered into a contiguous ping-pong buffer inside the previous step's reduce launch, so the
    step kernel reads row b without the dependent idx -> window load (csrc/kernels/tiny_ecg_step.hip GatherArgs).
    Measured: step kernel 7.76 -> 7.52 us and step period 12.35 -> 12.08 us under the kernel tracer (medians of
    687 steps), bench K=500 11.17 -> 11.06 us/step (profiles/r3/tiny_gather_ab.txt).

    ``pack`` (needs ``gather``): the gather also writes every window as a packed bf16 row - zero pads on both sides
    standing in for the conv padding - into a second ping-pong buffer ``xbg``, and the gathered steps run the step
    kernel variant that loads its conv1 operand from those rows (one 16-byte load and a one-element shift per time
    step instead of 7 floats, 7 conversions and the edge handling).  The operand is bitwise the same, so
    ``pack=False`` - the round exactly as it was, ``xg`` rows into the unpacked kernel - gives identical results.
    ``xg`` is written either way.

    ``prepack`` (needs ``pack``): the dataset does not change for the life of a trainer, so its packed form is built
    once, at construction (``xpk``, [N, ldb] bf16: about half the fp32 shard again), instead of being converted,
    padded and copied as fp32 on every step.  ``"gather"``: the gather blocks copy packed rows ``xpk[idx[b]]`` into
    ``xbg`` - 16 bytes per thread, fewer blocks, no fp32 read, no conversion, and no ``xg``, which is neither allocated
    nor written.  ``"direct"``: no gather at all - the packed step kernel loads ``idx[b]`` itself and reads its row
    from ``xpk`` (no ``xg`` / ``yg`` / ``xbg``); this is the fastest form measured and the default.  ``"none"`` /
    False: the round as above.  None: ``PREPACK_DEFAULT`` (or ECG_TINY_PREPACK) - but "none" for a caller that
    passes ``gather=`` or ``pack=``, who asks for that gather-based round and its buffers; True: the default form.
    Results are bitwise the same in every form.  Callers that rewrite ``x`` in place call ``repack()``.  If the packed shard would take more than
    ``prepack_share`` of the device's free memory, or its allocation fails, the trainer keeps the unpacked path:
    ``prepack`` is then ``"none"`` and ``prepack_fallback`` says why (None otherwise).  Measurements:
    profiles/r15/tiny_prepacked.txt.

    DP-SGD (``dp_clip`` > 0): every step clips each sample's gradient to l2 norm ``dp_clip`` and adds Gaussian noise
    of standard deviation ``dp_noise * dp_clip`` to their sum before the 1/B mean - two launches on the reduce side
    (clip factors, then the clipped and noised reduce + SGD), the step kernel unchanged.  The noise is Philox
    (``utils/philox.py``) keyed by ``dp_seed`` (default: a mix of ``seed``) and a 64-bit step counter kept on the
    device (``dp_step``; host mirror ``dp_steps``), so graph replays, enqueued rounds and the torch backend draw the
    same values.  The training loss is summed unclipped and un-noised: it is not private.

    FedProx (``prox_mu`` > 0; Li et al., "Federated Optimization in Heterogeneous Networks"): the local objective gains
    ``prox_mu / 2 * |w - w_start|^2``, ``w_start`` the weights the round started from, so every step's gradient gains
    ``prox_mu * (w - w_start)`` in the reduce kernel's SGD epilogue (``slab_reduce_prox_sgd_kernel``; it passes through
    momentum like any other gradient).  The round's first launch copies the weights into ``prox_anchor``, a tensor this
    trainer owns and only ever writes in place (captured graphs hold its address), so a replayed graph re-anchors every
    round and there is no state to save.  Not combined with DP-SGD.  ``prox_mu == 0``: the launches of before.
    """

    def __init__(self, model: TinyECG, x_gpu: torch.Tensor, y_gpu: torch.Tensor, batch_size: int,
                 steps_per_round: int, lr: float = 1e-2, momentum: float = 0.9, weight_decay: float = 0.0,
                 nesterov: bool = False, seed: Optional[int] = None, use_graph: Optional[bool] = None,
                 precision: str = "bf16", prefrag: bool = True, gather: Optional[bool] = None,
                 pack: Optional[bool] = None,
                 prepack=None, prepack_share: float = PREPACK_SHARE,
                 dp_clip: float = 0.0, dp_noise: float = 0.0, dp_seed: Optional[int] = None, prox_mu: float = 0.0):
        check_prox_args(prox_mu, dp_clip)
        self.device = x_gpu.device
        self.precision = precision
        self.prec = prec_id(precision)
        self.model = model
        self.nc = model.num_classes
        self.params = model.flat if model.flat is not None else model.flatten_parameters()
        if self.params.device != self.device:
            raise ValueError("model and dataset must be on the same device")
        self.P = num_params(self.nc)
        self.x = x_gpu.contiguous()
        self.y32 = labels_int32(y_gpu, self.nc)
        _check_dataset(self.x, self.y32, self.nc)
        self.B = int(batch_size)
        self.S = int(steps_per_round)
        self.lr, self.momentum, self.wd, self.nesterov = float(lr), float(momentum), float(weight_decay), bool(nesterov)
        self.stride = slab_stride(self.nc)
        self.mom = torch.zeros_like(self.params)
        self.slab = torch.empty((self.B, self.stride), dtype=torch.float32, device=self.device)
        self.loss_acc = torch.zeros(1, dtype=torch.float32, device=self.device)
        # batches of the NEXT round are drawn into idx_stage while the current round computes; a round reads the
        # staged table in place and the two tables then swap, so idx_table holds what the last round read
        self.idx_table = torch.zeros((self.S, self.B), dtype=torch.int32, device=self.device)
        self.idx_stage = torch.zeros((self.S, self.B), dtype=torch.int32, device=self.device)
        self._staged: Optional[int] = None  # rows staged for the next round (None: nothing staged)
        self._loss_steps = 0  # steps accumulated in loss_acc since its last reset
        self.sampler = DeviceIndexSampler(self.x.shape[0], self.B, self.device, seed=seed)
        # a round = one hipGraph replay, or (ECG_TINY_GRAPH=0) the same kernels enqueued from a C++ loop
        self.use_graph = (os.environ.get("ECG_TINY_GRAPH", "1") != "0") if use_graph is None else bool(use_graph)
        self._graphs = {}  # (n_steps, table pointer) -> native hipGraphExec handle
        self.steps_done = 0
        self._evaluator: Optional[TinyEvaluator] = None  # evaluate(): buffers allocated on first use
        lib = _lib.kernels()
        L = self.x.shape[1]
        smem = lib.ecg_tiny_smem_bytes(L, self.prec)
        if smem > 160 * 1024:
            raise ValueError(f"window length {L} too long for the fused kernel ({smem} B LDS)")
        self.prefrag = bool(prefrag) and precision == "bf16"
        self.wprep = new_wprep(self.device) if self.prefrag else None
        explicit_gather = gather is not None or pack is not None
        self.gather = (True if gather is None else bool(gather)) and self.prefrag
        self.pack = (True if pack is None else bool(pack)) and self.gather
        self.prepack_share = float(prepack_share)
        self.prepack, self.prepack_fallback = _prepack_variant(prepack, explicit_gather) if self.pack else "none", None
        self.xpk = None
        if self.prepack != "none":
            self._alloc_prepacked()
        self.xg = self.yg = self.xbg = None
        if self.gather and self.prepack != "direct":
            self.yg = torch.zeros(2 * self.B, dtype=torch.int32, device=self.device)
            if self.prepack == "none":
                self.xg = torch.zeros(lib.ecg_tiny_gather_floats(L, self.B), dtype=torch.float32, device=self.device)
            if self.pack:
                self.xbg = torch.zeros(lib.ecg_tiny_gather_halfs(L, self.B), dtype=torch.bfloat16,
                                       device=self.device)
        check_dp_args(dp_clip, dp_noise)
        self.dp_clip, self.dp_noise = float(dp_clip), float(dp_noise)
        self.dp = self.dp_clip > 0.0
        self.dp_seed = (mix64(0 if seed is None else seed) if dp_seed is None else int(dp_seed)) & (2 ** 64 - 1)
        self.dp_steps = 0  # host mirror of dp_step, counted like steps_done
        self.dp_scale = self.dp_step = None
        if self.dp:
            self.dp_scale = torch.zeros(self.B, dtype=torch.float32, device=self.device)
            self.dp_step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.prox_mu = float(prox_mu)
        self.prox_anchor = torch.zeros_like(self.params) if self.prox_mu > 0.0 else None
        # the native description of a round; ``idx`` and ``steps`` are set per round (_round_of)
        self._round = _lib.TinyRound(
            X=self.x.data_ptr(), ldx=self.x.stride(0), Y=self.y32.data_ptr(), params=self.params.data_ptr(),
            mom=self.mom.data_ptr(), slab=self.slab.data_ptr(), loss_acc=self.loss_acc.data_ptr(),
            wprep=_lib.ptr(self.wprep), xg=_lib.ptr(self.xg), yg=_lib.ptr(self.yg), L=L, nc=self.nc,
            slab_stride=self.stride, B=self.B, lr=self.lr, momentum=self.momentum, wd=self.wd,
            nesterov=int(self.nesterov), prec=self.prec, dp_clip=self.dp_clip, dp_sigma=self.dp_noise,
            dp_seed=self.dp_seed, dp_scale=_lib.ptr(self.dp_scale), dp_step=_lib.ptr(self.dp_step),
            xbg=_lib.ptr(self.xbg), xpk=_lib.ptr(self.xpk), prepack=_lib.PREPACK[self.prepack])
        if self.prox_mu > 0.0:  # (all-zero fields otherwise: the round then issues the launches it always issued)
            r = self._round
            r.prox_mu, r.prox_anchor, r.prox_snapshot = self.prox_mu, self.prox_anchor.data_ptr(), 1

    def _alloc_prepacked(self) -> None:
        """Allocate and fill the packed shard, or record why not and keep the unpacked path."""
        N, L = self.x.shape
        need = 2 * _lib.kernels().ecg_tiny_pack_halfs(L, N)
        free, _total = torch.cuda.mem_get_info(self.device)
        if need > self.prepack_share * free:
            self.prepack_fallback = (f"packed shard of {need} B exceeds {self.prepack_share:g} of the {free} B free")
        else:
            try:
                self.xpk = torch.empty((N, need // (2 * N)), dtype=torch.bfloat16, device=self.device)
            except torch.cuda.OutOfMemoryError as e:
                self.prepack_fallback = f"allocation of {need} B failed: {e}"
        if self.xpk is None:
            self.prepack = "none"
        else:
            self.repack()

    def repack(self) -> None:
        """Rebuild the packed shard from ``self.x`` (enqueued on the current stream): call it after rewriting the
        windows in place.  Without a packed shard there is nothing to do."""
        if self.xpk is not None:
            pack_dataset(self.x, self.xpk)

    # ------------------------------------------------------------------ graph management
    def _round_of(self, n: int, table: torch.Tensor):
        r = self._round
        r.idx, r.steps = table.data_ptr(), n
        return C.byref(r)

    def _graph_for(self, n: int, table: torch.Tensor) -> C.c_void_p:
        """Graph of an n-step round reading ``table`` in place (one per size and index buffer)."""
        key = (n, table.data_ptr())
        g = self._graphs.get(key)
        if g is None:
            g = C.c_void_p()
            torch.cuda.synchronize(self.device)
            _lib.check(_lib.kernels().ecg_tiny_round_capture(C.byref(g), self._round_of(n, table)),
                       "ecg_tiny_round_capture")
            self._graphs[key] = g
        return g

    def close(self):
        graphs, self._graphs = getattr(self, "_graphs", {}), {}
        for g in graphs.values():
            if g.value:
                _lib.kernels().ecg_round_graph_destroy(g)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ execution
    def prepare(self, sizes) -> None:
        """Draw the sampler's first permutation block, then capture, upload and warm every round graph whose step
        count is in ``sizes`` (on both index buffers), so a later round of that size only replays.  The warm-up
        replay is rolled back (weights, momentum, loss, staged batches and the DP step counter are restored): it
        leaves the training state exactly as it found it."""
        self.sampler.prime()
        if not self.use_graph:
            return
        lib = _lib.kernels()
        sizes = [self._check_n(n) for n in sizes]
        state = (self.params, self.mom, self.loss_acc, self.idx_stage, self.idx_table)
        if self.dp:
            state += (self.dp_step,)
        snap = [t.clone() for t in state]
        stream = _lib.stream_ptr(self.device)
        for n in sizes:
            for table in (self.idx_stage, self.idx_table):
                g = self._graph_for(n, table)
                _lib.check(lib.ecg_round_graph_upload(g, stream), "ecg_round_graph_upload")
                _lib.check(lib.ecg_round_graph_launch(g, stream), "ecg_round_graph_launch")
        for t, v in zip(state, snap):
            t.copy_(v)
        torch.cuda.synchronize(self.device)

    def _check_n(self, n_steps: Optional[int]) -> int:
        n = self.S if n_steps is None else int(n_steps)
        if not 0 < n <= self.S:
            raise ValueError(f"n_steps must be in [1, {self.S}]")
        return n

    def stage(self, n_steps: Optional[int] = None) -> None:
        """Draw the next round's ``n_steps`` batches into the staging table (enqueued on the current stream: it
        runs after the rounds already enqueued, none of which reads this table)."""
        n = self._check_n(n_steps)
        self.sampler.fill(self.idx_stage[:n])
        self._staged = n

    def prepare_round(self, n_steps: Optional[int] = None, reset_loss: bool = True) -> None:
        """Batch preparation of a round (unless ``launch_round(..., next_n=n)`` already staged it); reads no
        weights, so it can run while the previous round's FedAvg all-reduce is in flight (``--overlap tail``)."""
        n = self._check_n(n_steps)
        if reset_loss:
            self.loss_acc.zero_()
            self._loss_steps = 0
        if self._staged != n:
            if self._staged is not None:
                raise RuntimeError(f"{self._staged} rows are staged for the next round, not {n}")
            self.stage(n)

    def take_staged(self, n_steps: Optional[int] = None) -> torch.Tensor:
        """Consume the batches staged for an ``n_steps`` round and count its steps: returns the table whose first
        ``n_steps`` rows the round reads in place.  The two tables swap: that table is now ``idx_table`` and the
        other one receives the next staging."""
        n = self._check_n(n_steps)
        if self._staged != n:
            raise RuntimeError("launch_round without prepare_round: no batches staged for this round")
        self._staged = None
        self.idx_table, self.idx_stage = self.idx_stage, self.idx_table
        self.steps_done += n
        self._loss_steps += n
        if self.dp:
            self.dp_steps += n
        return self.idx_table

    def run_round(self, n_steps: Optional[int] = None, reset_loss: bool = True, next_n: Optional[int] = None) -> None:
        """Enqueue ``n_steps`` (default ``steps_per_round``) local SGD steps on the current stream (async);
        ``next_n``: also stage the following round's batches behind this round."""
        self.prepare_round(n_steps, reset_loss)
        self.launch_round(n_steps, next_n)

    def launch_round(self, n_steps: Optional[int] = None, next_n: Optional[int] = None) -> None:
        """The round's SGD steps on the staged batches (one graph replay, or the same launches enqueued one by
        one), then optionally stage the next round."""
        n = self._check_n(n_steps)
        table = self.take_staged(n)
        stream = _lib.stream_ptr(self.device)
        if self.use_graph:
            _lib.check(_lib.kernels().ecg_round_graph_launch(self._graph_for(n, table), stream),
                       "ecg_round_graph_launch")
        else:
            _lib.check(_lib.kernels().ecg_tiny_round_enqueue(self._round_of(n, table), stream),
                       "ecg_tiny_round_enqueue")
        if next_n is not None:
            self.stage(next_n)

    def evaluate(self, x: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None) -> EvalResult:
        """Loss / accuracy / confusion matrix of the CURRENT weights, in this trainer's precision, on windows ``x``
        with labels ``y`` (default: its own training windows).  Enqueued on the current stream behind whatever
        rounds are in flight; reads the weights only (its own prepared-fragment image, scratch and output record are
        allocated on first use - a round's ``wprep`` is not touched), so the training state is left as it was.  The
        returned record's metric tensors are reused by the next ``evaluate``."""
        if (x is None) != (y is None):
            raise ValueError("evaluate takes both windows and labels, or neither")
        if x is None:
            x, y32 = self.x, self.y32
        else:
            y32 = y if y.dtype == torch.int32 else labels_int32(y, self.nc)
        if self.precision != "bf16":
            return tiny_evaluate(self.params, x, y32, None, self.nc, self.precision)
        if self._evaluator is None:
            self._evaluator = TinyEvaluator(self.device, self.nc)
        return self._evaluator.run(self.params, x, y32)

    def avg_loss(self) -> float:
        """Mean per-step loss since the last reset (synchronises)."""
        return float(self.loss_acc.item()) / (self.B * max(1, self._loss_steps))

    def reset_momentum(self):
        self.mom.zero_()

    def set_dp_steps(self, n: int) -> None:
        """Continue the noise stream at step ``n`` (checkpoint resume)."""
        self.dp_steps = int(n)
        if self.dp:
            self.dp_step.fill_(int(n))
