"""Dataset packed once (``FusedTinyTrainer(prepack=...)``, ``ecg_tiny_pack_dataset``): the packed shard is, byte for
byte, what the gather blocks write per step, and a round that copies packed rows (``"gather"``) or reads them in place
(``"direct"``) leaves the bits of the round that converts on every step.  No tolerance anywhere in this file."""
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG

pytestmark = pytest.mark.gpu

LEAD = 4  # kPackLead of csrc/kernels/tiny_ecg_step.hip
LENGTHS = [5, 8, 31, 32, 33, 100]  # scalar and 4-float forms, L < 8, both sides of a multiple of 32
VARIANTS = ["gather", "direct"]
B, N, STEPS = 8, 24, 3

SPECIALS = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8),  # exact bf16 rounding ties (to even: down, up)
            0.0, -0.0, 1e-40, -1e-40,                                    # signed zeros, fp32 subnormals
            1e30, -1e30, 3.4e38, -3.4e38]                                # large; rounds past the largest finite bf16


def _ldb(L):
    return (L + 31) // 32 * 32 + 8


@pytest.mark.parametrize("L", LENGTHS)
def test_packed_shard_bytes(L):
    """N = 5 rows; the specials sit on every other element from the first one on and at both ends of every row.  Row
    pitches L (contiguous), L + 4 (keeps the 4-float form where 4 | L) and L + 3 (forces the scalar form); the output
    starts as -7 everywhere, so a pad that is not written shows."""
    from crossscale_ecg.ops.fused_tiny import pack_dataset
    dev = torch.device("cuda:0")
    n = 5
    g = torch.Generator(device="cpu").manual_seed(L)
    x = torch.randn(n, L, generator=g)
    flat = x.view(-1)
    for k, v in enumerate(SPECIALS):
        flat[2 * k] = v
    for r in range(n):
        x[r, 0] = SPECIALS[(r + 3) % len(SPECIALS)]
        x[r, L - 1] = SPECIALS[(2 * r + 5) % len(SPECIALS)]
    assert torch.isfinite(x).all()
    ldb = _ldb(L)
    want = torch.zeros(n, ldb, dtype=torch.bfloat16)
    want[:, LEAD:LEAD + L] = x.to(torch.bfloat16)
    assert want[:, LEAD:LEAD + L].isinf().any()  # the overflow case is in
    for extra in (0, 4, 3):
        buf = torch.full((n, L + extra), 7.0)
        buf[:, :L] = x
        xd = buf.to(dev)[:, :L]
        assert xd.stride(0) == L + extra
        out = torch.full((n, ldb), -7.0, dtype=torch.bfloat16, device=dev)
        got = pack_dataset(xd, out)
        torch.cuda.synchronize()
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16)), f"L={L} pitch {L + extra}"


def _dataset(L, nc, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, L, generator=g)
    y = torch.randint(0, nc, (N,), generator=g)
    idx = torch.stack([torch.randperm(N, generator=g)[:B] for _ in range(STEPS)]).to(torch.int32)
    idx[:, 1] = idx[:, 0]   # the same window twice in a batch, in every step
    idx[1, 5] = idx[1, 2]
    return x, y, idx


def _round(x, y, idx, nc, use_graph, **kw):
    """Weights, momentum and mean loss after one STEPS-step round on the batches ``idx``; the trainer is closed."""
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    model = TinyECG(num_classes=nc).to(dev)
    tr = FusedTinyTrainer(model, x.to(dev), y.to(dev), B, STEPS, seed=11, use_graph=use_graph, **kw)
    tr.prepare_round(STEPS)
    tr.idx_stage[:STEPS].copy_(idx.to(dev))  # the staged table is what the round reads
    tr.launch_round(STEPS)
    torch.cuda.synchronize()
    out = (tr.params.clone(), tr.mom.clone(), tr.avg_loss())
    info = (tr.prepack, tr.prepack_fallback, tr.xpk is not None, tr.xg is not None, tr.yg is not None,
            tr.xbg is not None)
    tr.close()
    assert torch.isfinite(out[0]).all() and out[2] == out[2]
    return out, info


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: weights differ by {(a[0] - b[0]).abs().max().item()}"
    assert torch.equal(a[1], b[1]), f"{what}: momentum differs"
    assert a[2] == b[2], f"{what}: avg_loss {a[2]} != {b[2]}"


@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("nc", [2, 5])
@pytest.mark.parametrize("L", [L for L in LENGTHS if L >= 8])  # (the step kernel takes no window under 8 samples)
def test_prepacked_round_bitwise_equal(L, nc, waves):
    from crossscale_ecg.ops import _lib
    lib = _lib.kernels()
    x, y, idx = _dataset(L, nc, seed=100 * L + nc)
    prev = lib.ecg_tiny_force_waves(waves)
    try:
        ref, info = _round(x, y, idx, nc, True, prepack=False)
        assert info == ("none", None, False, True, True, True)
        for graph in (True, False):
            for variant in VARIANTS:
                out, info = _round(x, y, idx, nc, graph, prepack=variant)
                bufs = variant == "gather"
                assert info == (variant, None, True, False, bufs, bufs)
                _same(out, ref, f"{variant} graph={graph}")
    finally:
        lib.ecg_tiny_force_waves(prev)


def test_short_window_is_rejected_either_way():
    """L = 5 packs (test_packed_shard_bytes) but no round takes it, with or without the packed shard."""
    from crossscale_ecg.ops import _lib
    x, y, idx = _dataset(5, 2, seed=1)
    for prepack in (False, "gather", "direct"):
        with pytest.raises(_lib.NativeError):
            _round(x, y, idx, 2, True, prepack=prepack)


@pytest.mark.parametrize("variant", VARIANTS)
def test_repack_after_in_place_change(variant):
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer, pack_dataset
    dev = torch.device("cuda:0")
    L, nc = 100, 2
    x, y, idx = _dataset(L, nc, seed=77)
    xd = x.to(dev)
    torch.manual_seed(5)
    tr = FusedTinyTrainer(TinyECG(num_classes=nc).to(dev), xd, y.to(dev), B, STEPS, seed=11, prepack=variant)
    assert tr.x.data_ptr() == xd.data_ptr()
    xd.mul_(-0.75).add_(0.125)
    stale = tr.xpk.clone()
    tr.repack()
    assert not torch.equal(stale, tr.xpk) and torch.equal(tr.xpk, pack_dataset(xd))
    tr.prepare_round(STEPS)
    tr.idx_stage[:STEPS].copy_(idx.to(dev))
    tr.launch_round(STEPS)
    torch.cuda.synchronize()
    out = (tr.params.clone(), tr.mom.clone(), tr.avg_loss())
    tr.close()
    fresh, _ = _round(xd.cpu(), y, idx, nc, True, prepack=variant)
    _same(out, fresh, "repacked vs fresh trainer")
    plain, _ = _round(xd.cpu(), y, idx, nc, True, prepack=False)
    _same(out, plain, "repacked vs unpacked round")


@pytest.mark.parametrize("variant", VARIANTS)
def test_refused_shard_falls_back(variant):
    """A share of 0 refuses every shard: the trainer runs the unpacked round and says so."""
    x, y, idx = _dataset(33, 2, seed=3)
    out, info = _round(x, y, idx, 2, True, prepack=variant, prepack_share=0.0)
    assert info[0] == "none" and info[1] and "exceeds" in info[1]
    assert info[2:] == (False, True, True, True)
    ref, _ = _round(x, y, idx, 2, True, prepack=False)
    _same(out, ref, "fallback vs prepack=False")


def test_prepack_needs_pack():
    x, y, idx = _dataset(32, 2, seed=4)
    _, info = _round(x, y, idx, 2, True, prepack="gather", pack=False)
    assert info[0] == "none" and info[1] is None and not info[2]
