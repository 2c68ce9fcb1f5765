"""Packed gather (``FusedTinyTrainer(pack=True)``): the reduce launches also write every gathered window as a packed
bf16 row (``xbg``) and the gathered steps run the step-kernel variant that loads its conv1 operand from those rows.
The operand is bitwise the unpacked kernel's, so every result must ``torch.equal`` the ``pack=False`` round and the
ungathered round: no tolerance anywhere in this file."""
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG

pytestmark = pytest.mark.gpu

B, N = 32, 128
PLAN = [3, 1, 2, 4]  # both ping-pong buffers, a 1-step round (no gather), odd and even lengths
LEAD = 4             # kPackLead of csrc/kernels/tiny_ecg_step.hip


def _ldb(L):
    return (L + 31) // 32 * 32 + 8


def _dataset(L, nc, seed=0, n=N):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, L, generator=g)
    y = torch.randint(0, nc, (n,), generator=g)
    return x, y


def _run(x, y, nc, plan=PLAN, **kw):
    """Parameters, momentum and mean loss after ``plan``; the trainer is returned open (caller closes it)."""
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    model = TinyECG(num_classes=nc).to(dev)
    tr = FusedTinyTrainer(model, x.to(dev), y.to(dev), B, max(plan), seed=17, **kw)
    for n in plan:
        tr.run_round(n, reset_loss=False)
    torch.cuda.synchronize()
    return tr, (tr.params.clone(), tr.mom.clone(), tr.avg_loss())


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), f"{what}: params differ by {(a[0] - b[0]).abs().max().item()}"
    assert torch.equal(a[1], b[1]), f"{what}: momentum differs"
    assert a[2] == b[2], f"{what}: avg_loss {a[2]} != {b[2]}"


def _compare_paths(x, y, nc, plan=PLAN, **kw):
    """pack=True == pack=False == gather=False, replayed as a graph and enqueued launch by launch."""
    outs = {}
    for graph in (True, False):
        for name, cfg in (("pack", dict(pack=True)), ("nopack", dict(pack=False)), ("nogather", dict(gather=False))):
            tr, out = _run(x, y, nc, plan, use_graph=graph, **cfg, **kw)
            assert tr.pack == (name == "pack") and (tr.xbg is not None) == tr.pack
            assert tr.gather == (name != "nogather")
            tr.close()
            assert torch.isfinite(out[0]).all() and out[2] == out[2]
            outs[(name, graph)] = out
    ref = outs[("nopack", True)]
    for key, out in outs.items():
        _same(out, ref, f"{key} vs ('nopack', True)")


@pytest.mark.parametrize("nc", [2, 5])
@pytest.mark.parametrize("L", [8, 29, 32, 33, 63, 100, 250, 500])
def test_packed_rounds_bitwise_equal_unpacked(L, nc):
    x, y = _dataset(L, nc, seed=L + nc)
    _compare_paths(x, y, nc)


@pytest.mark.parametrize("waves,L", [(8, 100), (8, 1000), (16, 1000)])
def test_packed_rounds_wave_counts_and_further_pairs(waves, L):
    """8 waves: every wave owns several tile pairs (4 at L = 1000), so conv1's further-pairs loop issues packed loads
    of its own; 16 waves at L = 1000: two pairs per wave."""
    from crossscale_ecg.ops import _lib
    x, y = _dataset(L, 2, seed=waves + L)
    lib = _lib.kernels()
    prev = lib.ecg_tiny_force_waves(waves)
    try:
        _compare_paths(x, y, 2)
    finally:
        lib.ecg_tiny_force_waves(prev)


SPECIALS = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8),  # exact bf16 rounding ties (to even: down, up)
            0.0, -0.0, 1e-40, -1e-40,                                    # signed zeros, fp32 subnormals
            1e30, -1e30, 3.4e38, -3.4e38]                                # large; rounds past the largest finite bf16


@pytest.mark.parametrize("L", [500, 250, 29])  # 4-float gather rows / scalar rows (L % 4 != 0) / shorter than a tile pair
def test_packed_buffer_contents(L):
    """After the last round (4 steps: step 3 read buffer 1) buffer 1 of ``xbg`` holds that step's windows as bf16 - the
    bits of torch's round-to-nearest-even conversion - between zero pads, every pad element of both buffers is zero,
    and ``xg`` / ``yg`` hold what they always did.  N == B: every batch is a permutation of the whole dataset, so the
    special values, placed at both row ends and inside, are in the last batch.  (Weights and loss are not compared
    here: these inputs overflow them.)"""
    x, y = _dataset(L, 2, seed=L, n=B)
    for r in range(B):
        for k, v in enumerate(SPECIALS):
            x[r, (r + 3 * k) % L] = v
        x[r, 0] = SPECIALS[r % len(SPECIALS)]
        x[r, L - 1] = SPECIALS[(r + 5) % len(SPECIALS)]
    assert torch.isfinite(x).all()
    tr, _ = _run(x, y, 2, use_graph=True, pack=True)
    ldb, ldg = _ldb(L), (L + 3) // 4 * 4
    assert tr.xbg.dtype == torch.bfloat16 and tr.xbg.numel() == 2 * B * ldb and ldb % 8 == 0 and LEAD >= 3
    rows = tr.idx_table[3].long()
    xb = tr.xbg.view(2, B, ldb).cpu()
    want = x[rows.cpu()].to(torch.bfloat16)
    assert torch.equal(xb[1, :, LEAD:LEAD + L].view(torch.int16), want.view(torch.int16))  # bit for bit (-0, inf)
    lead, tail = xb[:, :, :LEAD].view(torch.int16), xb[:, :, LEAD + L:].view(torch.int16)
    assert tail.shape[2] >= 4 and not lead.any() and not tail.any()  # +0 bits in every pad element of both buffers
    assert torch.equal(tr.yg[B:], tr.y32[rows])
    assert torch.equal(tr.xg.view(2, B, ldg)[1, :, :L].cpu().view(torch.int32), x[rows.cpu()].view(torch.int32))
    tr.close()


def test_packed_dp_round_bitwise_equal_unpacked():
    """The DP-SGD reduce has its own gather branch: clipped, noised rounds with packed rows == without."""
    x, y = _dataset(250, 5, seed=9)
    outs = []
    for pack in (True, False):
        tr, out = _run(x, y, 5, use_graph=True, pack=pack, dp_clip=0.5, dp_noise=0.8, dp_seed=1234)
        assert tr.dp and tr.pack == pack
        tr.close()
        assert torch.isfinite(out[0]).all()
        outs.append(out)
    _same(outs[0], outs[1], "DP pack vs no pack")
