"""Client-level DP on cohort rounds, on the CPU: the Philox stream word, ``TorchCohortTrainer``'s DP close against the
definition in float64 numpy, the server step size, the driver's flags and its per-round client-privacy CSV (world 1 and
gloo world 2).

The definition (train/cohort.py): d_c = p_c - g, n_c = |d_c|_2, s_c = min(1, C / n_c) (n_c == 0 -> 1),
g_new = g + eta * ((sum_c s_c d_c) * fp32(1 / M) + nu * z), nu = sigma * C / (M * sqrt(W)),
z = philox.normal(seed, round, P, stream=1)."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv
from crossscale_ecg.utils import philox, privacy
from crossscale_ecg.utils.csvio import read_csv

P = 1458  # TinyECG, 2 classes
EPS32 = 2.0 ** -23


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


# ------------------------------------------------------------------------------------------------ 1: the stream word
def test_philox_stream_word():
    seed, t = 0x1234567890ABCDEF, (7 << 32) | 5
    assert np.array_equal(philox.normal(seed, t, 300), philox.normal(seed, t, 300, stream=0))
    assert np.array_equal(philox.words(seed, t, 300), philox.words(seed, t, 300, stream=0))
    # ... which are the values of the counter (i, t lo, t hi, 0), built by hand
    ctr = np.zeros((300, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(300), 5, 7
    assert np.array_equal(philox.words(seed, t, 300), philox.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)))
    ctr[:, 3] = 1
    assert np.array_equal(philox.words(seed, t, 300, stream=1),
                          philox.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)))
    z0, z1 = philox.normal(seed, t, 300), philox.normal(seed, t, 300, stream=1)
    assert not np.any(z0 == z1)
    u1, u2 = philox.uniforms(seed, t, 300, stream=1)
    assert np.array_equal(z1, np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    # 64 rounds x 1,458 values of the new stream: mean and variance within 5 standard errors of 0 and 1
    z = np.concatenate([philox.normal(99, r, P, stream=1) for r in range(64)])
    n = z.size
    assert n == 64 * 1458
    assert abs(z.mean()) < 5.0 / math.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) < 5.0 * math.sqrt(2.0 / n), z.var()


# ------------------------------------------------------------------------------------------------ reference trainer
B, S, K, M, L, N = 5, 3, 4, 3, 64, 48


def _data():
    g = torch.Generator().manual_seed(3)
    return torch.randn(N, L, generator=g), torch.randint(0, 2, (N,), generator=g)


def _trainer(**kw):
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = _data()
    torch.manual_seed(0)
    return TorchCohortTrainer(TinyECG(), x, y, B, S, clients=K, cohort=M, lr=1e-2, momentum=0.9, amp_dtype=None, seed=5,
                              **kw)


def test_huge_clip_no_noise_is_the_plain_round():
    """g + mean(d) against mean(p): the same quantity, summed in another order."""
    plain, dp = _trainer(), _trainer(client_dp_clip=1e9)
    assert not plain.client_dp and dp.client_dp
    for _ in range(2):
        plain.run_round(S)
        dp.run_round(S)
    a, b = _flat(plain.model), _flat(dp.model)
    assert not torch.equal(a, _flat(_trainer().model))
    assert torch.allclose(b, a, rtol=1e-5, atol=0.0), ((a - b).abs() / a.abs()).max()
    norms, clipped = dp.last_clip_stats()
    assert len(norms) == M and all(n > 0 for n in norms) and clipped == 0.0
    assert dp.round_clients == plain.round_clients and abs(dp.avg_loss() - plain.avg_loss()) < 1e-6


def _hand_made(tr, C):
    """Make ``tr``'s clients end on g + d_c with |d_c| in {0, C / 2, 4 C}; returns (g, d [M, P]) in float64."""
    g = _flat(tr.model).double().numpy()
    rng = np.random.default_rng(11)
    d = rng.standard_normal((M, P))
    d *= (np.array([0.0, C / 2, 4 * C]) / np.linalg.norm(d, axis=1))[:, None]
    shapes = [p.shape for p in tr.model.parameters()]

    def fake(j, n, table):
        w = torch.from_numpy(g + d[j]).float()
        out, off = [], 0
        for s in shapes:
            out.append(w[off:off + s.numel()].view(s).clone())
            off += s.numel()
        return out

    tr._client_round = fake
    # (the deltas the trainer sees are fp32(g + d) - g: what the definition is evaluated on below)
    d32 = np.stack([torch.from_numpy(g + d[j]).float().double().numpy() - g for j in range(M)])
    return g, d32


@pytest.mark.parametrize("eta", [1.0, 0.5])
@pytest.mark.parametrize("sigma, world", [(0.0, 1), (1.5, 1), (1.5, 2)])
def test_hand_made_deltas_against_the_definition_in_float64(sigma, world, eta):
    C = 0.3
    tr = _trainer(client_dp_clip=C, client_dp_noise=sigma, client_dp_seed=77, server_lr=eta, world_size=world)
    g, d = _hand_made(tr, C)
    tr.set_cohort_round(4)
    tr.run_round(S)
    n = np.linalg.norm(d, axis=1)
    s = np.array([1.0 if v == 0 else min(1.0, C / v) for v in n])
    assert s[0] == 1.0 and s[1] == 1.0 and abs(s[2] - 0.25) < 1e-6
    nu = sigma * C / (M * math.sqrt(world))
    z = philox.normal(77, 4, P, stream=1)  # the noise of round 4, the round the trainer was set to
    want = g + eta * ((s[:, None] * d).sum(0) / M + nu * z)
    got = _flat(tr.model).double().numpy()
    # fp32 evaluation of the formula: M products and sums, the 1 / M and noise terms, the step: (M + 8) roundings
    bound = (M + 8) * EPS32 * (np.abs(g) + eta * (np.abs(d).mean(0) + nu * np.abs(z)))
    assert np.all(np.abs(got - want) <= bound), float((np.abs(got - want) / bound).max())
    assert not np.allclose(got, g)
    norms, clipped = tr.last_clip_stats()
    assert np.allclose(norms, n, rtol=1e-5, atol=1e-7) and clipped == pytest.approx(1 / 3)
    if sigma > 0:  # another round draws other noise; stream 0 is not what was added
        assert np.abs(got - (g + eta * ((s[:, None] * d).sum(0) / M + nu * philox.normal(77, 4, P)))).max() > 1e-3
        assert np.abs(got - (g + eta * ((s[:, None] * d).sum(0) / M + nu * philox.normal(77, 5, P, stream=1)))).max() > 1e-3


def test_server_lr_half_halves_the_update():
    full, half = _trainer(client_dp_clip=0.05, client_dp_noise=1.0), _trainer(server_lr=0.5, client_dp_clip=0.05,
                                                                                client_dp_noise=1.0)
    g0 = _flat(full.model).clone()
    full.run_round(S)
    half.run_round(S)
    uf, uh = _flat(full.model) - g0, _flat(half.model) - g0
    assert uf.abs().max() > 1e-4
    assert (uh - 0.5 * uf).abs().max() <= 4 * EPS32 * (g0.abs().max() + uf.abs().max())
    # the step size alone (no clip) takes the same path: eta = 0.5 halves the plain round's update
    plain, eta = _trainer(), _trainer(server_lr=0.5)
    assert eta.client_dp
    plain.run_round(S)
    eta.run_round(S)
    up, ue = _flat(plain.model) - g0, _flat(eta.model) - g0
    assert (ue - 0.5 * up).abs().max() <= 4 * EPS32 * (g0.abs().max() + up.abs().max())


def test_trainer_argument_checks():
    with pytest.raises(ValueError, match="client_dp_noise needs"):
        _trainer(client_dp_noise=1.0)
    with pytest.raises(ValueError, match=">= 0"):
        _trainer(client_dp_clip=-1.0)
    with pytest.raises(ValueError, match="server_lr"):
        _trainer(server_lr=0.0)
    with pytest.raises(ValueError, match="DP-SGD"):  # record-level DP-SGD in a cohort stays rejected
        _trainer(dp_clip=1.0, client_dp_clip=1.0)


# ------------------------------------------------------------------------------------------------ 5: flags
def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=3, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=4, cohort=2, client_dp_clip=0.002,
                client_dp_noise=1.0, client_dp_delta=1e-5,
                results_csv=os.path.join(tmp, "rounds.csv"), eval_csv=os.path.join(tmp, "eval.csv"),
                privacy_csv=os.path.join(tmp, "privacy.csv"), cohort_csv=os.path.join(tmp, "cohort.csv"),
                client_privacy_csv=os.path.join(tmp, "client_privacy.csv"), ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


def test_flags_parse_and_are_checked(tmp_path):
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train import fedavg as drv
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args([]))
    assert (cfg.client_dp_clip, cfg.client_dp_noise, cfg.client_dp_delta, cfg.server_lr, cfg.client_privacy_csv) == \
        (0.0, 0.0, 1e-5, 1.0, "results/fedavg_client_privacy.csv")
    drv.check_client_dp_config(cfg)  # everything off: nothing to check
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(
        ["--clients-per-gpu", "64", "--cohort", "8", "--client-dp-clip", "0.5", "--client-dp-noise", "1.1",
         "--client-dp-delta", "1e-6", "--server-lr", "0.7", "--client-privacy-csv", "x.csv"]))
    assert (cfg.client_dp_clip, cfg.client_dp_noise, cfg.client_dp_delta, cfg.server_lr, cfg.client_privacy_csv) == \
        (0.5, 1.1, 1e-6, 0.7, "x.csv")
    drv.check_client_dp_config(cfg)  # accepted with client sampling
    drv.check_cohort_config(cfg, "fused")
    t = str(tmp_path)
    for kw in (dict(client_dp_clip=1.0), dict(client_dp_clip=1.0, client_dp_noise=1.0), dict(server_lr=0.5)):
        with pytest.raises(ValueError, match="--clients-per-gpu"):  # rejected without it
            drv.check_client_dp_config(_cfg(t, **{**dict(clients_per_gpu=1, cohort=0, client_dp_clip=0.0,
                                                         client_dp_noise=0.0), **kw}))
    with pytest.raises(ValueError, match="--client-dp-noise needs"):
        drv.check_client_dp_config(_cfg(t, client_dp_clip=0.0))
    with pytest.raises(ValueError, match=">= 0"):
        drv.check_client_dp_config(_cfg(t, client_dp_clip=-1.0))
    with pytest.raises(ValueError, match="--client-dp-delta"):
        drv.check_client_dp_config(_cfg(t, client_dp_delta=0.0))
    with pytest.raises(ValueError, match="--server-lr"):
        drv.check_client_dp_config(_cfg(t, server_lr=0.0))
    # every combination client sampling rejects stays rejected with client-level DP on, through the driver
    for kw, match in ((dict(dp_clip=1.0), "--dp-clip"), (dict(sync="ddp"), "--sync ddp"),
                      (dict(drop_prob=0.1), "--drop-prob"), (dict(overlap="delayed"), "--overlap delayed"),
                      (dict(model="resnet1d"), "ResNet1D")):
        with pytest.raises(ValueError, match=match):
            drv.run_fedavg(_cfg(t, **kw), _ctx1())
    with pytest.raises(ValueError, match="--clients-per-gpu"):
        drv.run_fedavg(_cfg(t, clients_per_gpu=1, cohort=0), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv")) and not os.path.exists(os.path.join(t, "client_privacy.csv"))


def test_noise_share_follows_the_all_reduce(tmp_path):
    """sigma / sqrt(W) per rank is right only where the driver averages the W ranks' weights (--sync fedavg on more
    than one rank); an independent client (--sync none) adds the whole noise itself."""
    from crossscale_ecg.train import fedavg as drv

    class Ctx2(penv.DistContext):  # rank 0 of 2 initialised ranks, without a process group
        distributed = True

    ctx2 = Ctx2(0, 2, 0, "gloo", torch.device("cpu"))
    t = str(tmp_path)
    assert drv.client_dp_world(_cfg(t), ctx2) == 2 and drv.client_dp_world(_cfg(t, sync="none"), ctx2) == 1
    assert drv.client_dp_world(_cfg(t), _ctx1()) == 1
    x, y = torch.randn(256, 64), torch.zeros(256, dtype=torch.long)
    nu = {}
    for sync in ("fedavg", "none"):
        cfg = _cfg(t, sync=sync)
        drv.check_cohort_config(cfg, "torch")  # client sampling accepts both
        nu[sync] = drv.make_trainer(cfg, "G0", TinyECG(), x, y, ctx2, "torch").cdp_nu
    assert nu["fedavg"] == float(np.float32(1.0 / math.sqrt(2.0) * 0.002 / 2))
    assert nu["none"] == float(np.float32(1.0 * 0.002 / 2))  # the whole noise: nothing averages it down


# ------------------------------------------------------------------------------------------------ 6: the driver
def _check_privacy_rows(path, world, rounds=3, sigma=1.0, clip=0.002, delta=1e-5):
    from crossscale_ecg.utils.csvio import CLIENT_PRIVACY_COLUMNS
    with open(path) as f:
        assert f.readline().strip().split(",") == CLIENT_PRIVACY_COLUMNS
    rows = read_csv(path)
    assert [int(r["round_idx"]) for r in rows] == list(range(rounds))
    eps = [float(r["epsilon"]) for r in rows]
    assert all(b >= a for a, b in zip(eps, eps[1:])) and eps[0] > 0 and math.isfinite(eps[-1])
    for i, r in enumerate(rows):
        assert (r["config"], int(r["world_size"]), float(r["sample_rate"]), float(r["noise_multiplier"]),
                float(r["clip_norm"]), float(r["delta"])) == ("G0", world, 0.5, sigma, clip, delta)
        assert float(r["epsilon"]) == pytest.approx(privacy.epsilon(sigma, 0.5, i + 1, delta), rel=1e-12)
        assert float(r["median_client_norm"]) > 0 and 0.0 <= float(r["clipped_share_rank0"]) <= 1.0
    return rows


def test_driver_world1_writes_the_client_privacy_csv(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    cfg = _cfg(str(tmp_path))
    kept = []
    real = drv.make_trainer
    drv.make_trainer = lambda *a: kept.append(real(*a)) or kept[-1]
    try:
        drv.run_fedavg(cfg, _ctx1())
    finally:
        drv.make_trainer = real
    rows = _check_privacy_rows(cfg.client_privacy_csv, 1)
    tr = kept[0]
    assert tr.cdp_nu == float(np.float32(1.0 * 0.002 / 2)) and tr.cdp_seed == philox.mix64(1234) and tr.cohort_round == 3
    # clip 0.002 is below what two SGD steps at lr 1e-2 move the weights (about 0.004 to 0.01): clients were clipped
    assert any(float(r["clipped_share_rank0"]) > 0 for r in rows)
    assert len(read_csv(cfg.cohort_csv)) == 3 and not os.path.exists(cfg.privacy_csv)
    # without the flags no client-privacy file appears, and the weights differ from the DP run's
    plain = _cfg(str(tmp_path / "plain"), client_dp_clip=0.0, client_dp_noise=0.0)
    drv.make_trainer = lambda *a: kept.append(real(*a)) or kept[-1]
    try:
        drv.run_fedavg(plain, _ctx1())
    finally:
        drv.make_trainer = real
    assert not os.path.exists(plain.client_privacy_csv)
    assert not kept[1].client_dp and not torch.equal(_flat(kept[0].model), _flat(kept[1].model))


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
        kept = []
        real = drv.make_trainer

        def spy(*a):
            kept.append(real(*a))
            return kept[-1]

        drv.make_trainer = spy
        drv.run_fedavg(_cfg(tmp), ctx)
        tr = kept[0]
        q.put((rank, "ok", (_flat(tr.model).tolist(), tr.cdp_nu, tr.cdp_seed)))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


def test_gloo_world2_noise_share_identical_weights_and_privacy_rows(tmp_path):
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
    assert out[0][0] == out[1][0] and len(out[0][0]) == P  # FedAvg leaves the same global weights on both ranks
    nu = float(np.float32(1.0 / math.sqrt(2.0) * 0.002 / 2))  # each rank adds sigma / sqrt(2) of the noise
    assert out[0][1] == nu and out[1][1] == nu
    assert (out[0][2], out[1][2]) == (philox.mix64(1234), philox.mix64(1234 + 7919))  # independent noise per rank
    _check_privacy_rows(os.path.join(str(tmp_path), "client_privacy.csv"), 2)
