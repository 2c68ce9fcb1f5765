"""DP-SGD on the CPU: ``TorchLocalTrainer``'s per-sample clip + Philox noise against a hand-written float64 loop, the
FedAvg driver's --dp-clip / --dp-noise path (world 1, gloo world 2, resume) and the rejected configurations."""
import math
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from crossscale_ecg.parallel import env as penv
from crossscale_ecg.utils import philox
from crossscale_ecg.utils.csvio import read_csv


def _per_sample_grads64(model64, x, y):
    out = []
    for b in range(x.shape[0]):
        model64.zero_grad(set_to_none=True)
        F.cross_entropy(model64(x[b:b + 1].double().unsqueeze(1)), y[b:b + 1]).backward()
        out.append(torch.cat([p.grad.reshape(-1) for p in model64.parameters()]))
    return torch.stack(out)


def test_torch_dp_steps_match_float64_loop():
    """Two DP steps at B = 8, L = 64 (momentum and the step counter both advance) == clip each sample's autograd
    gradient in float64, sum, add sigma * C * z from utils/philox.py, divide by B, SGD + momentum by hand."""
    from crossscale_ecg.train.local import TorchLocalTrainer
    B, L, N, sigma, lr, mu, dp_seed = 8, 64, 40, 1.3, 1e-2, 0.9, 0xC0FFEE1234567
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, L, generator=g)
    y = torch.randint(0, 2, (N,), generator=g)
    torch.manual_seed(0)
    model = TinyECG()
    ref = TinyECG().double()
    ref.load_state_dict(model.state_dict())
    # clip norm: between the 4th and 5th per-sample norm of the first 8 windows at the initial weights, so that
    # samples on both sides of the clip exist in a typical batch
    n0 = _per_sample_grads64(ref, x[:B], y[:B]).norm(dim=1).sort().values
    C = float((n0[3] * n0[4]).sqrt())
    tr = TorchLocalTrainer(model, x, y, B, lr=lr, momentum=mu, amp_dtype=None, seed=5, dp_clip=C, dp_noise=sigma,
                           dp_seed=dp_seed)
    P = num_params(2)
    w = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
    buf = torch.zeros_like(w)
    clipped = kept = 0
    for t in range(2):
        tr.step()
        sel = tr._idx[0].long()
        gs = _per_sample_grads64(ref, x[sel], y[sel])
        norms = gs.norm(dim=1)
        c = torch.clamp(C / norms, max=1.0)
        clipped += int((c < 1).sum())
        kept += int((c == 1).sum())
        z = torch.from_numpy(philox.normal(dp_seed, t, P))
        grad = ((gs * c[:, None]).sum(0) + sigma * C * z) / B
        buf = mu * buf + grad
        w = w - lr * buf
        off = 0
        with torch.no_grad():
            for p in ref.parameters():
                p.copy_(w[off:off + p.numel()].view_as(p))
                off += p.numel()
        got = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).double()
        # fp32 forward / backward / clip against float64: relative 1e-5 of the update is ~100 ulp of headroom
        assert (got - w).abs().max() <= 1e-5 * (lr * buf).abs().max() + 1e-7 * w.abs().max(), (t, (got - w).abs().max())
    assert clipped > 0 and kept > 0 and tr.dp_steps == 2 and tr.steps_done == 2


def test_torch_dp_huge_clip_no_noise_equals_plain_sgd():
    from crossscale_ecg.train.local import TorchLocalTrainer
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(64, 64, generator=g), torch.randint(0, 2, (64,), generator=g)
    outs = []
    for kw in (dict(), dict(dp_clip=1e30)):
        torch.manual_seed(0)
        m = TinyECG()
        tr = TorchLocalTrainer(m, x, y, 16, amp_dtype=None, seed=2, **kw)
        tr.run_steps(3)
        outs.append((torch.cat([p.detach().reshape(-1) for p in m.parameters()]), tr.avg_loss()))
    assert torch.allclose(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-7)
    assert abs(outs[0][1] - outs[1][1]) < 1e-5


# ------------------------------------------------------------------------------------------------ driver
def _cfg(tmp, **kw):
    base = dict(batch_size=32, rounds=3, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, dp_clip=1.0, dp_noise=1.0,
                results_csv=os.path.join(tmp, "rounds.csv"), eval_csv=os.path.join(tmp, "eval.csv"),
                privacy_csv=os.path.join(tmp, "privacy.csv"), ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


def _check_privacy_rows(path, world, rounds, local_steps, q):
    from crossscale_ecg.utils.csvio import PRIVACY_COLUMNS
    from crossscale_ecg.utils.privacy import epsilon
    with open(path) as f:
        assert f.readline().strip().split(",") == PRIVACY_COLUMNS
    rows = read_csv(path)
    assert [int(r["round_idx"]) for r in rows] == list(range(rounds))
    eps = [float(r["epsilon"]) for r in rows]
    assert all(math.isfinite(e) and e > 0 for e in eps) and all(a < b for a, b in zip(eps, eps[1:]))
    for i, r in enumerate(rows):
        assert int(r["world_size"]) == world and int(r["steps"]) == (i + 1) * local_steps
        assert abs(float(r["sample_rate"]) - q) < 1e-12 and float(r["delta"]) == 1e-5
        assert float(r["noise_multiplier"]) == 1.0 and float(r["clip_norm"]) == 1.0
        assert abs(eps[i] - epsilon(1.0, q, (i + 1) * local_steps, 1e-5)) <= 1e-9 * eps[i]


def test_cli_flags_and_defaults():
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args([]))
    assert (cfg.dp_clip, cfg.dp_noise, cfg.dp_delta, cfg.privacy_csv) == (0.0, 0.0, 1e-5, "results/fedavg_privacy.csv")
    ns = entry.build_parser().parse_args(["--dp-clip", "1.5", "--dp-noise", "0.8", "--dp-delta", "1e-6"])
    cfg = from_args(FedAvgConfig, ns)
    assert (cfg.dp_clip, cfg.dp_noise, cfg.dp_delta) == (1.5, 0.8, 1e-6)


def test_driver_world1_writes_privacy_csv_and_default_run_does_not(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.utils.csvio import ROUND_COLUMNS
    cfg = _cfg(str(tmp_path))
    drv.run_fedavg(cfg, _ctx1())
    _check_privacy_rows(cfg.privacy_csv, 1, 3, 2, 32 / 256)
    with open(cfg.results_csv) as f:
        assert f.readline().strip().split(",") == ROUND_COLUMNS  # the round rows keep their columns
    off = _cfg(str(tmp_path / "off"), dp_clip=0.0, dp_noise=0.0)
    drv.run_fedavg(off, _ctx1())
    assert not os.path.exists(off.privacy_csv)


def test_resume_continues_the_noise_stream(tmp_path):
    """A run interrupted after round 1 and resumed ends on the weights of the uninterrupted run: the rank file
    carries the DP step counter, so rounds 2-3 draw steps 4..7 of the noise stream, not 0..3 again."""
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.utils.ckpt import ckpt_path, load_checkpoint, rank_state_path
    full = _cfg(str(tmp_path / "full"), rounds=4, ckpt_every=2)
    drv.run_fedavg(full, _ctx1())
    part = _cfg(str(tmp_path / "part"), rounds=2, ckpt_every=2)
    drv.run_fedavg(part, _ctx1())
    assert load_checkpoint(rank_state_path(part.ckpt_dir, 1, "G0", 0))["dp_steps"] == 4
    drv.run_fedavg(_cfg(str(tmp_path / "part"), rounds=4, ckpt_every=2, resume=True), _ctx1())
    a = load_checkpoint(ckpt_path(full.ckpt_dir, 3, "G0"))["model"]
    b = load_checkpoint(ckpt_path(part.ckpt_dir, 3, "G0"))["model"]
    assert all(torch.equal(a[k], b[k]) for k in a)
    mid = load_checkpoint(ckpt_path(part.ckpt_dir, 1, "G0"))["model"]
    assert not all(torch.equal(a[k], mid[k]) for k in a)
    rows = read_csv(part.privacy_csv)  # rounds 0, 1 of the first run, 2, 3 of the resumed one: steps keep counting
    assert [int(r["steps"]) for r in rows] == [2, 4, 6, 8]


def test_rejected_configurations_raise(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    with pytest.raises(ValueError, match="ResNet1D engine"):
        drv.check_dp_config(_cfg(str(tmp_path), model="resnet1d", kernel_backend="hip"), "G1", "hip")
    with pytest.raises(ValueError, match="fp16 AMP"):
        drv.check_dp_config(_cfg(str(tmp_path), amp_dtype="fp16", kernel_backend="auto"), "G1", "torch")
    with pytest.raises(ValueError, match="--sync ddp"):
        drv.check_dp_config(_cfg(str(tmp_path), sync="ddp", kernel_backend="fused"), "G1", "fused")
    with pytest.raises(ValueError, match="--dp-clip"):
        drv.check_dp_config(_cfg(str(tmp_path), dp_clip=0.0, dp_noise=1.0), "G0", "torch")
    # the same configurations are fine without DP, and fp16 only concerns the AMP configuration
    drv.check_dp_config(_cfg(str(tmp_path), sync="ddp", kernel_backend="fused", dp_clip=0.0, dp_noise=0.0), "G1", "fused")
    drv.check_dp_config(_cfg(str(tmp_path), amp_dtype="fp16"), "G0", "torch")
    # through the driver: nothing trains, nothing is written
    with pytest.raises(ValueError, match="fp16 AMP"):
        drv.run_fedavg(_cfg(str(tmp_path), amp_dtype="fp16", config="both"), _ctx1())
    assert not os.path.exists(os.path.join(str(tmp_path), "rounds.csv"))
    from crossscale_ecg.train.local import TorchLocalTrainer
    x, y = torch.randn(32, 64), torch.zeros(32, dtype=torch.long)
    with pytest.raises(ValueError, match="fp16"):
        TorchLocalTrainer(TinyECG(), x, y, 8, amp_dtype=torch.float16, dp_clip=1.0)
    with pytest.raises(ValueError, match="dp_clip"):
        TorchLocalTrainer(TinyECG(), x, y, 8, dp_noise=1.0)


# ------------------------------------------------------------------------------------------- gloo, world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    penv._CTX = None
    torch.set_num_threads(1)
    try:
        from crossscale_ecg.train import fedavg as drv
        ctx = penv.init_distributed(backend="gloo", prefer_gpu=False)
        seeds = []
        real = drv.make_trainer

        def spy(*a):
            tr = real(*a)
            seeds.append(tr.dp_seed)
            return tr

        drv.make_trainer = spy
        drv.run_fedavg(_cfg(tmp), ctx)
        q.put((rank, "ok", seeds[0]))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


def test_gloo_world2_privacy_rows_and_per_rank_seeds(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in ps:
        p.start()
    out = {}
    for _ in range(world):
        rank, status, res = q.get(timeout=240)
        assert status == "ok", res
        out[rank] = res
    for p in ps:
        p.join(timeout=60)
    _check_privacy_rows(os.path.join(str(tmp_path), "privacy.csv"), 2, 3, 2, 32 / 256)
    assert out[0] == philox.mix64(1234) and out[1] == philox.mix64(1234 + 7919) and out[0] != out[1]
