"""``utils/privacy.py``: the RDP accountant of the sampled Gaussian mechanism against a closed form (q = 1), a float64
quadrature of the Renyi divergence it bounds, monotonicity, and the no-noise case."""
import math

import numpy as np
import pytest

import crossscale_ecg  # noqa: F401
from crossscale_ecg.utils import privacy


def test_full_batch_matches_closed_form():
    """sample_rate = 1: the plain Gaussian mechanism, rdp(alpha) = alpha / (2 sigma^2) per step."""
    for sigma, steps, delta in ((1.0, 1, 1e-5), (0.8, 100, 1e-5), (2.5, 1000, 1e-6)):
        want = min(steps * a / (2 * sigma ** 2) + math.log(1 / delta) / (a - 1) for a in privacy.ORDERS)
        got = privacy.epsilon(sigma, 1.0, steps, delta)
        assert abs(got - want) <= 1e-12 * want
    assert privacy.ORDERS == tuple(range(2, 257))


def _renyi_quadrature(q, sigma, alpha, n):
    """D_alpha((1-q) N(0, s^2) + q N(1, s^2) || N(0, s^2)) by the trapezoidal rule on n + 1 points: the integrand
    p0(x) * ((1-q) + q exp((2x - 1) / (2 s^2)))^alpha is a sum of Gaussians centred at 0..alpha, so
    [-12 s, alpha + 12 s] leaves tails below exp(-72); evaluated in log space."""
    x = np.linspace(-12.0 * sigma, alpha + 12.0 * sigma, n + 1)
    log_p0 = -x * x / (2 * sigma ** 2) - 0.5 * math.log(2 * math.pi * sigma ** 2)
    log_ratio = np.logaddexp(math.log1p(-q), math.log(q) + (2 * x - 1) / (2 * sigma ** 2))
    f = np.exp(log_p0 + alpha * log_ratio)
    h = x[1] - x[0]
    integral = h * (f.sum() - 0.5 * (f[0] + f[-1]))
    return math.log(integral) / (alpha - 1)


@pytest.mark.parametrize("q", [0.01, 0.1])
@pytest.mark.parametrize("sigma", [0.8, 1.5])
@pytest.mark.parametrize("alpha", [2, 3, 8])
def test_step_rdp_matches_quadrature(q, sigma, alpha):
    n = 1 << 12
    prev, cur = _renyi_quadrature(q, sigma, alpha, n), _renyi_quadrature(q, sigma, alpha, 2 * n)
    while abs(cur - prev) > 1e-8 * abs(cur):  # tighten the grid until the quadrature itself is stable
        n *= 2
        assert n <= 1 << 22
        prev, cur = cur, _renyi_quadrature(q, sigma, alpha, 2 * n)
    got = privacy.rdp_step(sigma, q, alpha)
    assert abs(got - cur) <= 1e-6 * cur, (got, cur)


def test_epsilon_is_monotone():
    delta = 1e-5
    by_steps = [privacy.epsilon(1.1, 0.02, t, delta) for t in (1, 10, 100, 1000, 10000)]
    by_q = [privacy.epsilon(1.1, q, 500, delta) for q in (0.001, 0.01, 0.05, 0.2, 1.0)]
    by_inv_sigma = [privacy.epsilon(s, 0.02, 500, delta) for s in (4.0, 2.0, 1.0, 0.7, 0.5)]
    for seq in (by_steps, by_q, by_inv_sigma):
        assert all(math.isfinite(v) and v > 0 for v in seq)
        assert all(a < b for a, b in zip(seq, seq[1:])), seq


def test_no_noise_is_infinite_and_bad_arguments_raise():
    assert privacy.epsilon(0.0, 0.01, 10, 1e-5) == math.inf
    assert privacy.epsilon(1.0, 0.01, 0, 1e-5) == 0.0
    for bad in (dict(delta=0.0), dict(delta=1.0), dict(steps=-1), dict(sample_rate=1.5)):
        kw = dict(noise_multiplier=1.0, sample_rate=0.01, steps=10, delta=1e-5)
        kw.update(bad)
        with pytest.raises(ValueError):
            privacy.epsilon(**kw)
