"""Counter-based Gaussian noise of DP-SGD, shared by the torch backend and the tests of the HIP kernels.

Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), written from the
paper and checked against the Random123 known-answer vectors (tests/test_philox_cpu.py).  Conventions, the same as
``dp_normal`` in csrc/kernels/tiny_ecg_step.hip and ``cohort_dp_normal`` in csrc/kernels/tiny_ecg_close.hip (the rounds
themselves: ``philox4x32_10`` in csrc/include/tiny_ecg.h):

* counter ``(i, t & 0xffffffff, t >> 32, stream)``, key ``(seed & 0xffffffff, seed >> 32)``: ``i`` the flat parameter
  index, ``t`` the 64-bit DP step counter, ``seed`` the 64-bit DP seed; ``stream`` is 0 for DP-SGD (``dp_normal``) and
  1 for the client-level DP close of a cohort round (``cohort_dp_normal``, ``t`` the round counter), so the two
  noise streams never share a counter;
* ``u1 = ((w0 >> 8) + 1) * 2^-24`` in (0, 1], ``u2 = (w1 >> 8) * 2^-24`` in [0, 1) from output words 0 and 1 (both
  exact in fp32);
* ``z = sqrt(-2 ln u1) * cos(2 pi u2)`` (Box-Muller, one normal per counter; ``|z| <= sqrt(48 ln 2) < 5.77``).

Everything is vectorised over ``i`` with numpy; ``normal`` evaluates Box-Muller in float64 (the device uses fp32
``logf`` / ``sqrtf`` / ``cosf`` on the same uniforms and agrees to a few 1e-6).
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


def philox4x32_10(counter, key) -> np.ndarray:
    """Philox4x32 with 10 rounds.  ``counter``: uint32 [..., 4]; ``key``: two 32-bit words.  Returns uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(MASK32)
    c0, c1, c2, c3 = (c[..., j].copy() for j in range(4))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    lo32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> s32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> s32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & lo32, n2, p0 & lo32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed: int, t: int, n: int, stream: int = 0) -> np.ndarray:
    """Output words uint32 [n, 4] of parameter indices 0..n-1 at step ``t`` of noise stream ``stream``."""
    seed, t = int(seed) & MASK64, int(t) & MASK64
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(n, dtype=np.uint64)
    ctr[:, 1] = t & MASK32
    ctr[:, 2] = t >> 32
    ctr[:, 3] = int(stream) & MASK32
    return philox4x32_10(ctr, (seed & MASK32, seed >> 32))


def uniforms(seed: int, t: int, n: int, stream: int = 0):
    """(u1 in (0, 1], u2 in [0, 1)) as float64 arrays [n]; every value is a multiple of 2^-24."""
    w = words(seed, t, n, stream)
    u1 = ((w[:, 0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (w[:, 1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normal(seed: int, t: int, n: int, stream: int = 0) -> np.ndarray:
    """Standard normals float64 [n] of parameter indices 0..n-1 at step ``t`` of noise stream ``stream``."""
    u1, u2 = uniforms(seed, t, n, stream)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def mix64(x: int) -> int:
    """A fixed 64-bit mix (the splitmix64 finaliser): spreads nearby integers (seed + 7919 * rank) over the key space."""
    x = (int(x) + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)
