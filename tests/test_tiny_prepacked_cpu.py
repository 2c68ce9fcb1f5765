"""``check_round`` and the packed dataset (``EcgTinyRound::xpk`` / ``prepack``): inconsistent pointer combinations are
rejected before anything is launched, so this needs the library but no GPU.  Pointers are made-up, 16-byte aligned
addresses that are never dereferenced: every round here is one that the check refuses."""
import ctypes as C

import pytest

import crossscale_ecg  # noqa: F401
from crossscale_ecg.ops import _lib

pytestmark = pytest.mark.skipif(not _lib.kernels_available(), reason="native kernel library not built")

BAD_ARG = 1
L, NC, B = 32, 2, 8


def _round(**kw):
    p = iter(range(0x10000, 0x100000, 0x1000))
    base = dict(X=next(p), ldx=L, idx=next(p), Y=next(p), params=next(p), mom=next(p), slab=next(p),
                loss_acc=next(p), wprep=next(p), xg=None, yg=next(p), L=L, nc=NC, slab_stride=1536, B=B, steps=3,
                lr=1e-2, momentum=0.9, wd=0.0, nesterov=0, prec=0, dp_clip=0.0, dp_sigma=0.0, dp_seed=0,
                dp_scale=None, dp_step=None, xbg=next(p), xpk=next(p), prepack=_lib.PREPACK["gather"])
    base.update(kw)
    return _lib.TinyRound(**base)


def _status(r):
    return _lib.kernels().ecg_tiny_round_enqueue(C.byref(r), None)


GATHER, DIRECT, NONE = (_lib.PREPACK[k] for k in ("gather", "direct", "none"))
REJECTED = {
    "xpk without a variant": dict(prepack=NONE, xg=0x200000),
    "variant without xpk": dict(xpk=None),
    "unknown variant": dict(prepack=3),
    "gather without xbg": dict(xbg=None),
    "gather without yg": dict(yg=None),
    "gather without wprep": dict(wprep=None),
    "gather without idx": dict(idx=None),
    "gather with xg": dict(xg=0x200000),
    "gather, fp32": dict(prec=1),
    "misaligned xpk": dict(xpk=0x300008),
    "direct with xbg": dict(prepack=DIRECT, yg=None),
    "direct with yg": dict(prepack=DIRECT, xbg=None),
    "direct with xg": dict(prepack=DIRECT, yg=None, xbg=None, xg=0x200000),
    "direct without wprep": dict(prepack=DIRECT, yg=None, xbg=None, wprep=None),
    "direct without idx": dict(prepack=DIRECT, yg=None, xbg=None, idx=None),
    # the rules that held before still hold without a packed dataset
    "xbg without xg": dict(prepack=NONE, xpk=None),
    "xg without yg": dict(prepack=NONE, xpk=None, xg=0x200000, yg=None),
}


@pytest.mark.parametrize("what", sorted(REJECTED))
def test_check_round_rejects(what):
    assert _status(_round(**REJECTED[what])) == BAD_ARG, what


def test_struct_and_sizes():
    lib = _lib.kernels()
    assert lib.ecg_tiny_round_sizeof() == C.sizeof(_lib.TinyRound)
    for length in (5, 8, 31, 32, 33, 100, 500):
        ldb = (length + 31) // 32 * 32 + 8
        assert lib.ecg_tiny_pack_halfs(length, 1) == ldb
        assert lib.ecg_tiny_pack_halfs(length, 3_000_000_000) == 3_000_000_000 * ldb  # 64-bit row counts
        assert lib.ecg_tiny_gather_halfs(length, B) == 2 * B * ldb
    # the pack entry point checks its arguments before it launches
    assert lib.ecg_tiny_pack_dataset(None, L, 5, L, 0x10000, None) == BAD_ARG
    assert lib.ecg_tiny_pack_dataset(0x10000, L - 1, 5, L, 0x20000, None) == BAD_ARG
    assert lib.ecg_tiny_pack_dataset(0x10000, L, 0, L, 0x20000, None) == BAD_ARG
    assert lib.ecg_tiny_pack_dataset(0x10000, L, 5, L, 0x20008, None) == BAD_ARG
