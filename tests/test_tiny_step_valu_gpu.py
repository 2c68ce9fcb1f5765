"""The MODE 4 step kernel (packed dataset read in place) after its vector-instruction cut computes, bit for bit, what it
computed before: weights, momentum and summed loss after each of two 3-step ``prepack="direct"`` rounds, and the
gradient rows of ``ecg_tiny_step_grads``, against fixtures under ``tests/golden/tiny_step_r19/``.

The fixtures were recorded on one MI355X by ``scripts/record_tiny_step_r19.py`` with the build of commit 702e5cb
("Cohort close: one Delta body, one dispatcher, a file of its own"), the parent of that change, from the same seeded
weights, windows and batches; the cases, and why each is there, are that script's ``CASES``.  No tolerance: the words
are compared with ``numpy.array_equal``."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_tiny_step_r19",
                                               os.path.join(ROOT, "scripts", "record_tiny_step_r19.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


def test_cases_cover_what_the_fixtures_claim():
    assert {(L, nc, w) for L, nc, w, kind in rec.CASES if kind == "randn"} == {
        (L, nc, w) for L in (8, 33, 100) for nc in (2, 5) for w in (8, 16)}
    assert any(kind == "zeros" for *_, kind in rec.CASES)
    x, _, _ = rec.case_inputs(100, 2, "zeros")
    assert (x[:, 15:58] == 0).all() and (x[:, 62:] <= 0).all() and (x[:, :15] > 0).any()


@pytest.mark.parametrize("case", rec.CASES, ids=[rec.case_name(*c) for c in rec.CASES])
def test_bitwise_equal_to_the_parent_build(case):
    L, nc, waves, kind = case
    want = np.load(os.path.join(rec.GOLDEN, rec.case_name(*case) + ".npy"))
    got = rec.compute_case(*case)
    assert got.dtype == want.dtype == np.uint32 and got.shape == want.shape
    from crossscale_ecg.models.tiny_ecg import num_params
    P = num_params(nc)
    names, off = [], 0
    for r in range(rec.ROUNDS):
        names += [(f"weights after round {r + 1}", P), (f"momentum after round {r + 1}", P),
                  (f"summed loss after round {r + 1}", 1)]
    names.append(("gradient rows", rec.B * (P + 1)))
    assert sum(n for _, n in names) == want.size
    for what, n in names:
        a, b = got[off:off + n], want[off:off + n]
        assert np.array_equal(a, b), (
            f"{rec.case_name(*case)}: {what}: {int((a != b).sum())} of {n} words differ, first at "
            f"{int(np.flatnonzero(a != b)[0])}: {a.view(np.float32)[np.flatnonzero(a != b)[0]]!r} != "
            f"{b.view(np.float32)[np.flatnonzero(a != b)[0]]!r}")
        off += n
    f = want.view(np.float32)
    assert np.isfinite(f).all() and (f[:P] != 0).any()
