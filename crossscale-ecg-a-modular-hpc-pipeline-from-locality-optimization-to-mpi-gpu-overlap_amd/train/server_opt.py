"""Server optimizers on a cohort round's averaged client delta (Reddi et al., "Adaptive Federated Optimization").

With Delta the averaged, clipped, noised client delta of a round (``train/cohort.py`` states it), server state ``m`` and
``v`` (fp32, kept across rounds; ``m = 0`` and, for the three adaptive rules, ``v = tau^2`` at construction - the
paper's ``v_{-1} >= tau^2``), no bias correction, everything in fp32:

* ``sgdm`` (FedAvgM):  ``m = b1 m + Delta``,                ``g += eta m``
* ``adagrad``:         ``m = b1 m + (1 - b1) Delta``,       ``v = v + Delta^2``
* ``adam``:            ``m`` as adagrad,                    ``v = b2 v + (1 - b2) Delta^2``
* ``yogi``:            ``m`` as adagrad,                    ``v = v - (1 - b2) Delta^2 sign(v - Delta^2)``, sign(0) = 0
* adagrad, adam, yogi: ``g += eta m / (sqrt(v) + tau)`` with the new ``m`` and ``v``

``eta`` is the server step size ``server_lr``.  This is the definition that ``cohort_server_opt_kernel`` and, from
Delta on, ``server_step_kernel`` of csrc/kernels/tiny_ecg_close.hip implement; ``server_opt_step`` is its torch form
(the eager reference and the CPU path).  ``SERVER_SCOPES`` names where the step is taken: per rank on the rank's own
Delta, or once ("global") on the all-reduced mean of the ranks' Deltas.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

SERVER_OPTS = ("none", "sgdm", "adagrad", "adam", "yogi")
SERVER_OPT_IDS = {name: i for i, name in enumerate(SERVER_OPTS)}  # EcgTinyCohortRound's server_opt
ADAPTIVE = ("adagrad", "adam", "yogi")
BETA1, BETA2, TAU = 0.9, 0.99, 1e-3
# Where the server step is taken.  "rank": inside every rank's round, on that rank's delta (a driver of several ranks
# then averages the stepped weights: exact for the linear rules only).  "global": the round stops at the delta, the
# driver averages the ranks' deltas, and every rank takes the same step on the average (``apply_server_step``).
SERVER_SCOPES = ("rank", "global")


def check_server_scope(scope: str) -> str:
    if scope not in SERVER_SCOPES:
        raise ValueError(f"unknown server scope {scope!r}: one of {', '.join(SERVER_SCOPES)}")
    return scope


def check_server_opt(opt: str, beta1: float = BETA1, beta2: float = BETA2, tau: float = TAU) -> int:
    """The id of ``opt``; raises on an unknown name and, with an optimizer on, on betas outside [0, 1) or tau <= 0."""
    if opt not in SERVER_OPT_IDS:
        raise ValueError(f"unknown server optimizer {opt!r}: one of {', '.join(SERVER_OPTS)}")
    if opt != "none":
        if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
            raise ValueError("server_beta1 and server_beta2 must be in [0, 1)")
        if opt in ADAPTIVE and not tau > 0.0:
            raise ValueError("server_tau must be > 0")
    return SERVER_OPT_IDS[opt]


def server_opt_init(opt: str, numel: int, tau: float, device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(m, v) as a run starts: zeros and (adaptive rules) fp32(tau)^2; (zeros, None) for sgdm, (None, None) for none."""
    if opt == "none":
        return None, None
    m = torch.zeros(numel, dtype=torch.float32, device=device)
    if opt not in ADAPTIVE:
        return m, None
    t = torch.tensor(tau, dtype=torch.float32, device=device)
    return m, (t * t).expand(numel).clone()


def server_opt_step(opt: str, g: torch.Tensor, delta: torch.Tensor, m: torch.Tensor, v: Optional[torch.Tensor],
                    eta: float, b1: float, b2: float, tau: float, dtype: torch.dtype = torch.float32):
    """One server step in fp32: ``(g_new, m_new, v_new)`` (``v_new`` is ``v`` for sgdm); the inputs are not written.
    ``dtype=torch.float64`` evaluates the same rules in float64 on the fp32 constants (a reference for tests)."""
    if opt not in SERVER_OPT_IDS or opt == "none":
        raise ValueError(f"server_opt_step: no rule for {opt!r}")
    c = lambda s: torch.tensor(s, dtype=torch.float32, device=g.device).to(dtype)  # noqa: E731  (rounded once, to fp32)
    g, delta, m = g.to(dtype), delta.to(dtype), m.to(dtype)
    eta, b1, b2, tau, one = c(eta), c(b1), c(b2), c(tau), c(1.0)
    if opt == "sgdm":
        m = b1 * m + delta
        return g + eta * m, m, v
    m = b1 * m + (one - b1) * delta
    v, d2 = v.to(dtype), delta * delta
    if opt == "adagrad":
        v = v + d2
    elif opt == "adam":
        v = b2 * v + (one - b2) * d2
    else:
        v = v - (one - b2) * d2 * torch.sign(v - d2)
    return g + (eta * m) / (torch.sqrt(v) + tau), m, v
