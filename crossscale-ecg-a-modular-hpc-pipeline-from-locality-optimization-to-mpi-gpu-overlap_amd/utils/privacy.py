"""Privacy accountant for DP-SGD: Renyi differential privacy (RDP) of the sampled Gaussian mechanism.

Per step, at every integer order alpha = 2..256, the RDP of the Gaussian mechanism with noise multiplier sigma applied
to a Poisson sample of rate q is the exact binomial sum of Mironov, Talwar and Zhang, "Renyi Differential Privacy of
the Sampled Gaussian Mechanism" (2019), section 3.3:

    rdp(alpha) = 1/(alpha-1) * ln sum_{k=0..alpha} C(alpha,k) (1-q)^(alpha-k) q^k exp((k^2 - k) / (2 sigma^2))

RDP composes additively over steps, and converts to (epsilon, delta)-DP with
``epsilon = min_alpha [ rdp(alpha) + ln(1/delta) / (alpha - 1) ]`` (Mironov 2017, proposition 3).

THIS IS THE POISSON-SUBSAMPLING BOUND.  It assumes every step draws its batch by including each record independently
with probability q.  The samplers of this project draw fixed-size batches from epoch permutations, as the reference
does; with ``sample_rate = batch / n_train`` the figure reported here is the commonly quoted approximation for such
training loops, not a proof for this sampler.
"""
from __future__ import annotations

import math
from typing import Iterable, Sequence

import numpy as np

ORDERS = tuple(range(2, 257))


def rdp_step(noise_multiplier: float, sample_rate: float, alpha: int) -> float:
    """RDP at integer order ``alpha`` >= 2 of one step of the sampled Gaussian mechanism."""
    sigma, q, a = float(noise_multiplier), float(sample_rate), int(alpha)
    if a < 2 or a != alpha:
        raise ValueError("alpha must be an integer >= 2")
    if not 0.0 <= q <= 1.0:
        raise ValueError("sample_rate must be in [0, 1]")
    if q == 0.0:
        return 0.0
    if sigma <= 0.0:
        return math.inf
    if q == 1.0:
        return a / (2.0 * sigma * sigma)
    k = np.arange(a + 1, dtype=np.float64)
    log_binom = np.array([math.lgamma(a + 1) - math.lgamma(i + 1) - math.lgamma(a - i + 1) for i in range(a + 1)])
    terms = log_binom + (a - k) * math.log1p(-q) + k * math.log(q) + (k * k - k) / (2.0 * sigma * sigma)
    m = float(terms.max())
    return (m + math.log(float(np.exp(terms - m).sum()))) / (a - 1)


def rdp(noise_multiplier: float, sample_rate: float, steps: int, orders: Sequence[int] = ORDERS) -> np.ndarray:
    """RDP of ``steps`` composed steps at every order of ``orders``."""
    return np.array([steps * rdp_step(noise_multiplier, sample_rate, a) for a in orders], dtype=np.float64)


def epsilon_from_rdp(rdp_values: Iterable[float], delta: float, orders: Sequence[int] = ORDERS) -> float:
    if not 0.0 < delta < 1.0:
        raise ValueError("delta must be in (0, 1)")
    return min(float(r) + math.log(1.0 / delta) / (a - 1) for r, a in zip(rdp_values, orders))


def epsilon(noise_multiplier: float, sample_rate: float, steps: int, delta: float) -> float:
    """epsilon of (epsilon, delta)-DP after ``steps`` DP-SGD steps with noise multiplier ``noise_multiplier`` at
    Poisson sampling rate ``sample_rate`` (see the module docstring for what that assumes); ``inf`` without noise."""
    if steps < 0:
        raise ValueError("steps must be >= 0")
    if not 0.0 < delta < 1.0:
        raise ValueError("delta must be in (0, 1)")
    if noise_multiplier <= 0.0:
        return math.inf
    if steps == 0:
        return 0.0
    return epsilon_from_rdp(rdp(noise_multiplier, sample_rate, steps), delta)
