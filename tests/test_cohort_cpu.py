"""Client sampling on the CPU: ``CohortSampler``'s partitions, cohorts and permutation passes, ``TorchCohortTrainer``
against a hand-written float64 loop, and the FedAvg driver's --clients-per-gpu / --cohort path (world 1, gloo world 2,
resume, rejected combinations, K = 1 == flag omitted)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.data.dataset import CohortSampler
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv
from crossscale_ecg.utils.csvio import read_csv
from crossscale_ecg.utils.philox import mix64


# ------------------------------------------------------------------------------------------------ sampler
def _table(s: CohortSampler, r: int):
    t = torch.zeros((s.S, s.M * s.B), dtype=torch.int32)
    return s.fill(r, t), t


def test_partitions_tile_the_windows_and_indices_stay_in_their_partition():
    N, B, S, K, M = 67, 5, 2, 6, 3  # n = 11, 1 window left over at the end
    s = CohortSampler(N, B, S, K, M, "cpu", seed=9)
    assert s.n == 11 and [k * s.n for k in range(K + 1)] == list(range(0, K * s.n + 1, s.n)) and K * s.n <= N
    seen = set()
    for r in range(40):
        ids, t = _table(s, r)
        assert len(ids) == M and len(set(ids)) == M and all(0 <= c < K for c in ids)
        for j, c in enumerate(ids):
            cols = t[:, j * B:(j + 1) * B]
            assert int(cols.min()) >= c * s.n and int(cols.max()) < (c + 1) * s.n
        seen.update(ids)
    assert seen == set(range(K))  # every client is drawn sooner or later
    assert int(t.max()) < K * s.n  # the remainder is never used


def test_cohort_is_a_function_of_seed_and_round_only():
    a = CohortSampler(64, 4, 3, 8, 3, "cpu", seed=5)
    b = CohortSampler(64, 4, 3, 8, 3, "cpu", seed=5)
    ids7, t7 = _table(a, 7)
    for r in (0, 3, 11):  # other rounds in between leave no trace
        _table(a, r)
    ids7b, t7b = _table(b, 7)
    assert ids7 == ids7b == a.clients_of(7) and torch.equal(t7, t7b) and torch.equal(_table(a, 7)[1], t7)
    g = torch.Generator().manual_seed(mix64(5) ^ 7)
    assert ids7 == torch.randperm(8, generator=g)[:3].tolist()  # the documented host generator
    other = CohortSampler(64, 4, 3, 8, 3, "cpu", seed=6)
    assert any(a.clients_of(r) != other.clients_of(r) for r in range(8))
    assert any(a.clients_of(r) != a.clients_of(r + 1) for r in range(8))


def test_no_repeats_within_a_pass_and_wrap_into_a_fresh_permutation():
    N, B, S, K, M = 40, 4, 7, 4, 2  # n = 10 < S * B = 28: two full passes and 8 rows of a third
    s = CohortSampler(N, B, S, K, M, "cpu", seed=1)
    assert s.passes == 3
    ids, t = _table(s, 0)
    for j, c in enumerate(ids):
        seq = t[:, j * B:(j + 1) * B].reshape(-1).tolist()  # the client's rows in the order it consumes them
        part = set(range(c * s.n, (c + 1) * s.n))
        assert set(seq[:10]) == part and set(seq[10:20]) == part  # each full pass is a permutation of the partition
        assert len(set(seq[20:])) == 8 and set(seq[20:]) <= part  # the last, partial pass repeats nothing
        assert seq[:10] != seq[10:20]  # fresh permutations
    big = CohortSampler(64, 4, 3, 4, 4, "cpu", seed=1)  # S * B = 12 <= n = 16: one pass, no row twice in a round
    ids, t = _table(big, 2)
    assert sorted(ids) == [0, 1, 2, 3]
    for j in range(4):
        assert len(set(t[:, j * 4:(j + 1) * 4].reshape(-1).tolist())) == 12


def test_sampler_rejects_bad_shapes():
    with pytest.raises(RuntimeError, match="per client"):
        CohortSampler(64, 8, 2, 10, 2, "cpu")  # n = 6 < B = 8
    with pytest.raises(ValueError, match="cohort"):
        CohortSampler(64, 4, 2, 4, 5, "cpu")
    with pytest.raises(ValueError, match="index table"):
        CohortSampler(64, 4, 2, 4, 2, "cpu").fill(0, torch.zeros((2, 7), dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ reference trainer
def test_torch_cohort_round_matches_float64_loop():
    """One cohort round (M = 3 of K = 4, B = 5, S = 3, momentum 0.9) == per client: float64 SGD from the global
    weights with zero momentum on its table columns; then the mean in ascending cohort order."""
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    B, S, K, M, L, N, lr, mu = 5, 3, 4, 3, 64, 48, 1e-2, 0.9
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, L, generator=g)
    y = torch.randint(0, 2, (N,), generator=g)
    torch.manual_seed(0)
    model = TinyECG()
    ref = TinyECG().double()
    ref.load_state_dict(model.state_dict())
    w0 = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
    tr = TorchCohortTrainer(model, x, y, B, S, clients=K, cohort=M, lr=lr, momentum=mu, amp_dtype=None, seed=5)
    tr.run_round(S)
    assert tr.cohort_round == 1 and tr.steps_done == S and tr.round_clients == tr.sampler.clients_of(0)
    finals, upd, losses = [], 0.0, []
    for j in range(M):
        w, buf = w0.clone(), torch.zeros_like(w0)
        for s in range(S):
            off = 0
            with torch.no_grad():
                for p in ref.parameters():
                    p.copy_(w[off:off + p.numel()].view_as(p))
                    off += p.numel()
            sel = tr.table[s, j * B:(j + 1) * B].long()
            ref.zero_grad(set_to_none=True)
            loss = F.cross_entropy(ref(x[sel].double().unsqueeze(1)), y[sel])
            loss.backward()
            losses.append(float(loss.detach()))
            grad = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
            buf = mu * buf + grad
            w = w - lr * buf
            upd = max(upd, float((lr * buf).abs().max()))
        finals.append(w)
    want = ((finals[0] + finals[1]) + finals[2]) / M
    got = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).double()
    # the bound of tests/test_dp_cpu.py's torch-vs-float64 comparison: 1e-5 of the update + 1e-7 of the weights
    assert (got - want).abs().max() <= 1e-5 * upd + 1e-7 * want.abs().max(), (got - want).abs().max()
    assert not torch.equal(got, w0)
    assert abs(tr.avg_loss() - sum(losses) / len(losses)) < 1e-5


# ------------------------------------------------------------------------------------------------ driver
def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=3, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=6, cohort=3,
                results_csv=os.path.join(tmp, "rounds.csv"), eval_csv=os.path.join(tmp, "eval.csv"),
                privacy_csv=os.path.join(tmp, "privacy.csv"), cohort_csv=os.path.join(tmp, "cohort.csv"),
                ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


def _check_cohort_rows(path, world, rounds, seed=1234):
    from crossscale_ecg.utils.csvio import COHORT_COLUMNS
    with open(path) as f:
        assert f.readline().strip().split(",") == COHORT_COLUMNS
    rows = read_csv(path)
    assert [int(r["round_idx"]) for r in rows] == list(range(rounds))
    s = CohortSampler(256, 8, 2, 6, 3, "cpu", seed=seed)  # rank 0's sampler: seed + 7919 * 0
    for r in rows:
        assert (r["config"], int(r["world_size"]), int(r["clients_per_gpu"]), int(r["cohort"]), int(r["batch_size"]),
                int(r["windows_per_round_per_gpu"])) == ("G0", world, 6, 3, 8, 3 * 8 * 2)
        assert [int(c) for c in r["clients_rank0"].split()] == s.clients_of(int(r["round_idx"]))


def test_cli_flags_and_defaults():
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train.fedavg import cohort_size
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args([]))
    assert (cfg.clients_per_gpu, cfg.cohort, cfg.cohort_csv) == (1, 0, "results/fedavg_cohort.csv")
    assert cohort_size(cfg) == 1
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(["--clients-per-gpu", "64"]))
    assert cohort_size(cfg) == 64  # --cohort defaults to K
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(["--clients-per-gpu", "64", "--cohort", "8"]))
    assert (cfg.clients_per_gpu, cohort_size(cfg)) == (64, 8)


def test_driver_world1_cohort_csv_round_columns_and_sample_count(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.utils.csvio import ROUND_COLUMNS
    cfg = _cfg(str(tmp_path), eval_every=1, eval_windows=64)
    rows = drv.run_fedavg(cfg, _ctx1())
    s = CohortSampler(256 - 64, 8, 2, 6, 3, "cpu", seed=1234)  # the hold-out comes off before partitioning
    crow = read_csv(cfg.cohort_csv)
    assert [[int(c) for c in r["clients_rank0"].split()] for r in crow] == [s.clients_of(r) for r in range(3)]
    with open(cfg.results_csv) as f:
        assert f.readline().strip().split(",") == ROUND_COLUMNS  # the round rows keep their columns
    for r in rows:  # batch_size stays the per-client B; samples/s counts all M * B * S windows
        assert r["batch_size"] == 8 and r["local_steps"] == 2
        assert abs(r["samples_per_s"] * r["local_train_ms"] / 1e3 - 3 * 8 * 2) < 1e-6
    assert len(read_csv(cfg.eval_csv)) == 3
    plain = _cfg(str(tmp_path / "plain"))
    drv.run_fedavg(plain, _ctx1())
    _check_cohort_rows(plain.cohort_csv, 1, 3)


def test_clients_per_gpu_1_is_the_run_without_the_flag(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.utils.ckpt import ckpt_path, load_checkpoint
    a = _cfg(str(tmp_path / "a"), clients_per_gpu=1, cohort=0, ckpt_every=3)
    base = {k: v for k, v in vars(a).items() if k not in ("clients_per_gpu", "cohort", "cohort_csv")}
    base.update({k: v.replace(os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b"))
                 for k, v in base.items() if isinstance(v, str) and str(tmp_path) in v})
    b = FedAvgConfig(**base)
    drv.run_fedavg(a, _ctx1())
    drv.run_fedavg(b, _ctx1())
    ma = load_checkpoint(ckpt_path(a.ckpt_dir, 2, "G0"))["model"]
    mb = load_checkpoint(ckpt_path(b.ckpt_dir, 2, "G0"))["model"]
    assert all(torch.equal(ma[k], mb[k]) for k in ma)
    assert not os.path.exists(a.cohort_csv)  # no client sampling, no cohort rows


def test_resume_after_round_1_of_3_ends_on_the_uninterrupted_weights(tmp_path):
    """The sampler is a function of (seed, round) and the rank file carries the round counter: rounds 2 (and 3) of the
    resumed run draw what the uninterrupted run drew."""
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.utils.ckpt import ckpt_path, load_checkpoint, rank_state_path
    full = _cfg(str(tmp_path / "full"), rounds=3, ckpt_every=1)
    drv.run_fedavg(full, _ctx1())
    part = _cfg(str(tmp_path / "part"), rounds=1, ckpt_every=1)
    drv.run_fedavg(part, _ctx1())
    assert load_checkpoint(rank_state_path(part.ckpt_dir, 0, "G0", 0))["cohort_round"] == 1
    drv.run_fedavg(_cfg(str(tmp_path / "part"), rounds=3, ckpt_every=1, resume=True), _ctx1())
    a = load_checkpoint(ckpt_path(full.ckpt_dir, 2, "G0"))["model"]
    b = load_checkpoint(ckpt_path(part.ckpt_dir, 2, "G0"))["model"]
    assert all(torch.equal(a[k], b[k]) for k in a)
    first = load_checkpoint(ckpt_path(part.ckpt_dir, 0, "G0"))["model"]
    assert not all(torch.equal(a[k], first[k]) for k in a)
    assert [int(r["round_idx"]) for r in read_csv(part.cohort_csv)] == [0, 1, 2]


def test_rejected_combinations_raise(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    t = str(tmp_path)
    with pytest.raises(ValueError, match="--dp-clip"):
        drv.check_cohort_config(_cfg(t, dp_clip=1.0), "torch")
    with pytest.raises(ValueError, match="--sync ddp"):
        drv.check_cohort_config(_cfg(t, sync="ddp"), "fused")
    with pytest.raises(ValueError, match="--drop-prob"):
        drv.check_cohort_config(_cfg(t, drop_prob=0.1), "torch")
    with pytest.raises(ValueError, match="--overlap delayed"):
        drv.check_cohort_config(_cfg(t, overlap="delayed"), "fused")
    with pytest.raises(ValueError, match="ResNet1D"):
        drv.check_cohort_config(_cfg(t, model="resnet1d"), "hip")
    with pytest.raises(ValueError, match="ResNet1D"):
        drv.check_cohort_config(_cfg(t, model="resnet1d"), "torch")
    with pytest.raises(ValueError, match="exceeds"):
        drv.check_cohort_config(_cfg(t, clients_per_gpu=4, cohort=5), "torch")
    for ov in ("none", "tail"):  # the supported overlaps, and every combination above without client sampling
        drv.check_cohort_config(_cfg(t, overlap=ov), "fused")
    drv.check_cohort_config(_cfg(t, clients_per_gpu=1, cohort=0, dp_clip=1.0, sync="ddp", drop_prob=0.1,
                                 overlap="delayed", model="resnet1d"), "hip")
    # through the driver: nothing trains, nothing is written
    with pytest.raises(ValueError, match="--drop-prob"):
        drv.run_fedavg(_cfg(t, drop_prob=0.5), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv")) and not os.path.exists(os.path.join(t, "cohort.csv"))
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = torch.randn(64, 64), torch.zeros(64, dtype=torch.long)
    with pytest.raises(ValueError, match="DP-SGD"):
        TorchCohortTrainer(TinyECG(), x, y, 8, 2, clients=4, dp_clip=1.0)


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
        kept = []
        real = drv.make_trainer

        def spy(*a):
            kept.append(real(*a))
            return kept[-1]

        drv.make_trainer = spy
        drv.run_fedavg(_cfg(tmp), ctx)
        tr = kept[0]
        w = torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()])
        # (plain floats: a tensor would travel as a shared-memory handle that dies with this process)
        q.put((rank, "ok", (w.tolist(), tr.sampler.seed, tr.round_clients)))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


def test_gloo_world2_identical_weights_and_cohort_rows(tmp_path):
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
    assert out[0][0] == out[1][0] and len(out[0][0]) == 1458  # FedAvg leaves the same global weights on both ranks
    assert (out[0][1], out[1][1]) == (1234, 1234 + 7919)  # every rank's seed stays seed + 7919 * rank
    _check_cohort_rows(os.path.join(str(tmp_path), "cohort.csv"), 2, 3)
