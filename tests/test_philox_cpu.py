"""``utils/philox.py``: Philox4x32-10 against the Random123 known-answer vectors, the uniform ranges of the
Box-Muller inputs, and distinct words for distinct (seed, step, parameter index)."""
import numpy as np

import crossscale_ecg  # noqa: F401
from crossscale_ecg.utils import philox

F = 0xFFFFFFFF
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((F, F, F, F), (F, F), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        got = philox.philox4x32_10(np.array(ctr, dtype=np.uint32), key)
        assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want
    # vectorised over the leading axis: the three counters under the first key, one call
    ctrs = np.array([k[0] for k in KAT], dtype=np.uint32)
    batch = philox.philox4x32_10(ctrs, KAT[0][1])
    assert tuple(int(v) for v in batch[0]) == KAT[0][2]
    for j in (1, 2):
        assert np.array_equal(batch[j], philox.philox4x32_10(ctrs[j], KAT[0][1]))


def test_counter_and_key_conventions():
    """words(seed, t, n)[i] is Philox of counter (i, t lo, t hi, 0) under key (seed lo, seed hi)."""
    seed, t = 0x299F31D0A4093822, 0x1319_8A2E_85A3_08D3
    w = philox.words(seed, t, 40)
    for i in (0, 7, 39):
        want = philox.philox4x32_10(np.array([i, t & F, t >> 32, 0], dtype=np.uint32), (seed & F, seed >> 32))
        assert np.array_equal(w[i], want)
    # the all-zero known-answer vector, reached through the public entry point
    assert np.array_equal(philox.words(0, 0, 1)[0], np.array(KAT[0][2], dtype=np.uint32))


def test_uniform_ranges_and_fp32_exactness():
    u1, u2 = philox.uniforms(seed=12345, t=3, n=200000)
    assert u1.min() > 0.0 and u1.max() <= 1.0
    assert u2.min() >= 0.0 and u2.max() < 1.0
    assert np.array_equal(u1.astype(np.float32).astype(np.float64), u1)
    assert np.array_equal(u2.astype(np.float32).astype(np.float64), u2)
    # the extreme words map to the ends of the ranges
    assert ((0xFFFFFFFF >> 8) + 1) * 2.0 ** -24 == 1.0 and ((0 >> 8) + 1) * 2.0 ** -24 == 2.0 ** -24
    assert (0xFFFFFFFF >> 8) * 2.0 ** -24 == 1.0 - 2.0 ** -24
    z = philox.normal(12345, 3, 200000)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(48 * np.log(2.0)) < 5.77
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1.0) < 0.01  # 200,000 draws: 4 sigma of the mean is 0.009


def test_distinct_inputs_give_distinct_words():
    base = philox.words(1, 0, 4096)
    assert len({tuple(r) for r in base.tolist()}) == 4096  # over i
    for other in (philox.words(2, 0, 4096), philox.words(1, 1, 4096), philox.words(1, 1 << 32, 4096),
                  philox.words(1 + (1 << 32), 0, 4096)):
        assert not (other == base).all(axis=1).any()
    # t and t + 2^32 differ (the high counter word is used), and so do seed and seed + 2^32 (the high key word)
    assert not np.array_equal(philox.normal(1, 5, 64), philox.normal(1, 5 + (1 << 32), 64))
    assert philox.mix64(1234) != philox.mix64(1234 + 7919) and 0 <= philox.mix64(2 ** 64 - 1) < 2 ** 64
