"""Robust aggregation in cohort rounds (``--aggregate trimmed | median``, ``--trim-frac``, ``--flip-clients``), on the
CPU: the definition ``robust_delta`` against ``robust_delta_f64`` and ``numpy.median``, NaN / infinite clients and
ties, ``trim_count``, ``flip_client_labels``, ``TorchCohortTrainer``, the driver's checks, one run of the entry point, and
two gloo ranks against the mean of the per-rank estimates."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MK = [(3, 1), (4, 1), (5, 2), (8, 1), (8, 3), (9, 4), (33, 5), (64, 1), (64, 31)]
U = 2.0 ** -24


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _inputs(M, P=600, seed=0):
    gen = torch.Generator().manual_seed(100 * M + seed)
    g = torch.randn(P, generator=gen)
    d = torch.randn(M, P, generator=gen) * 0.05
    d[1::2, ::3] = d[0:2 * (M // 2):2, ::3]  # exact ties across clients
    return g + d, g


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1: the definition
@pytest.mark.parametrize("M,k", MK)
def test_robust_delta_within_the_float64_bound(M, k):
    """(n + 1) 2^-24 sum over the kept |x_c| per element: one rounding per subtraction, n - 1 adds, one product."""
    from crossscale_ecg.train.cohort import robust_delta, robust_delta_f64
    stack, g = _inputs(M)
    got, want = robust_delta(stack, g, k), robust_delta_f64(stack, g, k)
    assert got.dtype == torch.float32 and want.dtype == torch.float64
    x = torch.sort(stack.double() - g.double(), dim=0).values[k:M - k]
    bound = (M - 2 * k + 1) * U * x.abs().sum(0)
    frac = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
    print(f"robust_delta M {M} k {k}: worst error / bound {frac:.3f}")
    assert frac <= 1.0
    assert float((got.double() - (stack.double() - g.double()).mean(0)).abs().max()) > 1e-4  # the trim acts


@pytest.mark.parametrize("M", [3, 4, 9, 64])
def test_median_is_numpy_median(M):
    """Odd M: the middle value itself, bit for bit.  Even M: (a + b) * 0.5 in fp32 against numpy's float64 median of
    the fp32 deltas: one rounding of the sum (the halving is exact)."""
    from crossscale_ecg.train.cohort import robust_delta, trim_count
    stack, g = _inputs(M, seed=1)
    k = trim_count("median", M)
    assert k == (M - 1) // 2
    got = robust_delta(stack, g, k)
    x = stack - g
    want = np.median(x.double().numpy(), axis=0)
    if M % 2:
        assert np.array_equal(got.double().numpy(), want)
    else:
        assert (np.abs(got.double().numpy() - want) <= U * np.abs(want)).all()


def test_bad_clients_ties_and_zeros():
    from crossscale_ecg.train.cohort import robust_delta, robust_delta_f64
    M, k = 8, 1
    stack, g = _inputs(M, seed=2)
    clean = robust_delta(stack, g, k)
    P = g.numel()
    # one client all NaN; one at +inf and one at -inf: trimmed away, the result finite and within the bound of float64
    for poison in ({3: float("nan")}, {1: float("inf"), 6: float("-inf")}):
        s = stack.clone()
        for c, val in poison.items():
            s[c] = val
        got, want = robust_delta(s, g, k), robust_delta_f64(s, g, k)
        assert torch.isfinite(got).all() and torch.isfinite(want).all()
        kept = torch.sort(s.double() - g.double(), dim=0).values[k:M - k]  # (NaN and +-inf sort to the ends)
        assert ((got.double() - want).abs() <= (M - 2 * k + 1) * U * kept.abs().sum(0)).all()
        assert not torch.equal(got, clean)
    # two NaN clients at every other parameter: NaN exactly there
    s = stack.clone()
    s[3] = float("nan")
    s[5, 0:P:2] = float("nan")
    got, want = robust_delta(s, g, k), robust_delta_f64(s, g, k)
    where = torch.zeros(P, dtype=torch.bool)
    where[0:P:2] = True
    assert torch.equal(torch.isnan(got), where) and torch.equal(torch.isnan(want), where)
    # a negative NaN sorts last too
    s = stack.clone()
    s[0] = torch.tensor([0xFFC00000 - (1 << 32)], dtype=torch.int32).view(torch.float32)
    assert torch.isfinite(robust_delta(s, g, k)).all()
    # ties break by client index, so equal values are kept as often as the ranks say: all equal -> that value
    eq = torch.full((5, 4), 0.25) + torch.zeros(4)
    assert torch.equal(robust_delta(eq, torch.zeros(4), 2), torch.full((4,), 0.25))
    # -0 < +0, and a kept -0 stays -0: deltas (-0, +0, -0) -> ranks (0, 2, 1), the median is client 2's -0
    z = torch.tensor([[-0.0], [0.0], [-0.0]])
    out = robust_delta(z, torch.zeros(1), 1)
    assert int(_bits(out)[0]) == -(1 << 31)
    z = torch.tensor([[0.0], [0.0], [-0.0]])  # ranks (1, 2, 0): client 0's +0
    assert int(_bits(robust_delta(z, torch.zeros(1), 1))[0]) == 0
    for bad_k in (0, 4, -1):
        with pytest.raises(ValueError, match="1 <= k"):
            robust_delta(stack, g, bad_k)


def test_trim_count_table_and_errors():
    from crossscale_ecg.train.cohort import AGGREGATES, ROBUST_AGGREGATES, trim_count
    assert AGGREGATES == ("mean", "weighted", "nova") and ROBUST_AGGREGATES == ("trimmed", "median")
    assert [trim_count("median", M) for M in (1, 2, 3, 4, 5, 8, 9, 64)] == [0, 0, 1, 1, 2, 3, 4, 31]
    assert [trim_count("trimmed", M, 0.25) for M in (4, 7, 8, 64)] == [1, 1, 2, 16]
    assert trim_count("trimmed", 10, 0.49) == 4 and trim_count("trimmed", 3, 0.34) == 1
    assert [trim_count(a, 100) for a in ("none", "mean", "weighted", "nova")] == [0, 0, 0, 0]
    for args, match in ((("trimmed", 8), "needs trim_frac"), (("trimmed", 8, 0.0), r"in \(0, 0.5\)"),
                        (("trimmed", 8, 0.5), r"in \(0, 0.5\)"), (("trimmed", 8, -0.1), r"in \(0, 0.5\)"),
                        (("trimmed", 3, 0.25), "drops floor"), (("median", 8, 0.25), "takes none"),
                        (("mean", 8, 0.25), "takes none"), (("median", 65), "at most 64 clients"),
                        (("trimmed", 65, 0.25), "at most 64 clients"), (("krum", 8), "aggregate must be one of"),
                        (("median", 0), "at least one client")):
        with pytest.raises(ValueError, match=match):
            trim_count(*args)


# ------------------------------------------------------------------------------------------------ 2: poisoned clients
def test_flip_client_labels():
    from crossscale_ecg.data.dataset import dirichlet_partition, flip_client_labels, flipped_labels
    gen = torch.Generator().manual_seed(0)
    nc, K = 5, 6
    y = torch.randint(0, nc, (100,), generator=gen)
    held = y.clone()
    order = torch.arange(96).view(K, 16)  # contiguous; rows 96..99 belong to nobody
    out = flip_client_labels(y, order, None, 2, nc)
    assert torch.equal(y, held) and out is not y  # the input is untouched
    assert torch.equal(out[:32], nc - 1 - y[:32]) and torch.equal(out[32:], y[32:])
    assert torch.equal(flip_client_labels(out, order, None, 2, nc), y)  # twice restores
    assert torch.equal(flip_client_labels(y, order, None, 0, nc), y)
    assert torch.equal(flipped_labels(y, None, None, K, 2, nc), out) and flipped_labels(y, None, None, K, 0, nc) is y
    # unequal clients: only the first sizes[k] entries of a row are the client's
    order, sizes = dirichlet_partition(y, K, 0.5, 4, 3)
    out = flip_client_labels(y, order, sizes, 3, nc)
    own = torch.zeros(100, dtype=torch.bool)
    for k in range(3):
        own[order[k, : int(sizes[k])]] = True
    assert torch.equal(out[own], nc - 1 - y[own]) and torch.equal(out[~own], y[~own]) and 0 < int(own.sum()) < 100
    assert torch.equal(flip_client_labels(out, order, sizes, 3, nc), y) and torch.equal(y, held)
    for F in (-1, K + 1):
        with pytest.raises(ValueError, match="flip_clients must be in"):
            flipped_labels(y, None, None, K, F, nc)


# ------------------------------------------------------------------------------------------------ 3: the trainer
B, S, K, N, L = 4, 3, 6, 64, 64


def _data():
    gen = torch.Generator().manual_seed(3)
    return torch.randn(N, L, generator=gen), torch.randint(0, 2, (N,), generator=gen)


def _trainer(**kw):
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = _data()
    torch.manual_seed(0)
    model = TinyECG()
    args = dict(clients=K, cohort=4, lr=1e-2, momentum=0.9, amp_dtype=None, seed=5)
    args.update(kw)
    return model, TorchCohortTrainer(model, x, y, B, S, **args)


@pytest.mark.parametrize("kw", [dict(robust="trimmed", trim_frac=0.25), dict(robust="median", cohort=5),
                                dict(robust="median", server_opt="adam", server_lr=0.05),
                                dict(robust="trimmed", trim_frac=0.25, server_opt="sgdm", server_lr=0.7),
                                dict(robust="median", server_lr=0.5),
                                dict(robust="trimmed", trim_frac=0.25, server_scope="global", server_opt="yogi",
                                     server_lr=0.05)])
def test_torch_trainer_takes_robust_delta_into_its_server_step(kw):
    """The round is: the clients of a mean round from the same start (same sampler, same local steps), their
    ``robust_delta``, the trainer's own server step."""
    from crossscale_ecg.train.cohort import robust_delta, trim_count
    from crossscale_ecg.train.server_opt import server_opt_init, server_opt_step
    model, tr = _trainer(**kw)
    plain_kw = {k: v for k, v in kw.items() if k == "cohort"}
    pmodel, plain = _trainer(**plain_kw)
    M = tr.M
    k = trim_count(kw["robust"], M, kw.get("trim_frac"))
    assert tr.trim == k >= 1 and not tr.hetero and plain.trim == 0
    opt, eta = kw.get("server_opt", "none"), kw.get("server_lr", 1.0)
    m, v = server_opt_init(opt, _flat(model).numel(), tr.server_tau, torch.device("cpu"))
    for rnd in range(2):
        g = _flat(model).clone()
        with torch.no_grad():
            torch.nn.utils.vector_to_parameters(g.clone(), pmodel.parameters())
        plain.set_cohort_round(rnd)
        ids = plain.sampler.fill(rnd, plain.table)
        clients = torch.stack([torch.cat([p.reshape(-1) for p in plain._client_round(j, S, plain.table)])
                               for j in range(M)])
        tr.run_round(S)
        assert tr.round_clients == ids
        delta = robust_delta(clients, g, k)
        if opt == "none":
            want = g + torch.tensor(eta, dtype=torch.float32) * delta
        else:
            want, m, v = server_opt_step(opt, g, delta, m, v, eta, tr.server_beta1, tr.server_beta2, tr.server_tau)
        assert torch.equal(_flat(model), want), rnd
        norms, clipped = tr.last_clip_stats()
        assert len(norms) == M and clipped == 0.0
        assert np.allclose(norms, (clients - g).norm(dim=1).tolist(), rtol=1e-5)
    if kw.get("server_scope") == "global":
        assert torch.equal(tr.server_delta, delta)


def test_torch_trainer_median_of_two_is_the_mean_and_flip_and_rejections():
    model, tr = _trainer(robust="median", cohort=2)
    model2, tr2 = _trainer(cohort=2)
    assert tr.trim == 0 and not tr.client_dp
    tr.run_round(S)
    tr2.run_round(S)
    assert torch.equal(_flat(model), _flat(model2))
    # flip_clients: the trainer's labels, not the caller's
    x, y = _data()
    _, tf = _trainer(robust="median", flip_clients=2)
    n = N // K
    assert torch.equal(tf.y[: 2 * n], 1 - y[: 2 * n]) and torch.equal(tf.y[2 * n:], y[2 * n:])
    _, t0 = _trainer(robust="median")
    assert torch.equal(t0.y, y)
    for kw, match in ((dict(aggregate="krum"), "aggregate must be one of"),
                      (dict(aggregate="median"), "aggregate must be one of"),  # the estimate is ``robust``'s to name
                      (dict(robust="krum"), "robust must be one of"),
                      (dict(robust="median", aggregate="weighted"), "takes no client weights"),
                      (dict(robust="trimmed"), "needs trim_frac"),
                      (dict(robust="trimmed", trim_frac=0.5), r"in \(0, 0.5\)"),
                      (dict(robust="trimmed", trim_frac=0.1), "drops floor"),
                      (dict(robust="median", trim_frac=0.25), "takes none"),
                      (dict(aggregate="weighted", trim_frac=0.25), "takes none"),
                      (dict(trim_frac=0.25), "takes none"),
                      (dict(robust="median", client_dp_clip=1.0), "sensitivity of a trimmed mean is not C / M"),
                      (dict(robust="trimmed", trim_frac=0.25, client_dp_clip=1.0),
                       "sensitivity of a trimmed mean is not C / M"),
                      (dict(robust="median", flip_clients=K + 1), "flip_clients must be in"),
                      (dict(robust="median", flip_clients=-1), "flip_clients must be in")):
        with pytest.raises(ValueError, match=match):
            _trainer(**kw)
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    gen = torch.Generator().manual_seed(1)
    xb, yb = torch.randn(65 * B, L, generator=gen), torch.randint(0, 2, (65 * B,), generator=gen)
    with pytest.raises(ValueError, match="at most 64 clients"):
        TorchCohortTrainer(TinyECG(), xb, yb, B, S, clients=65, robust="median", amp_dtype=None)
    # nova's restrictions do not apply; the robust aggregates compose with FedProx, nesterov and unequal local work
    _trainer(robust="median", prox_mu=0.1, nesterov=True, local_epochs=1)[1].run_round(S)


# ------------------------------------------------------------------------------------------------ 4: the driver
def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=2, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=8, cohort=4, aggregate="median",
                results_csv=os.path.join(tmp, "rounds.csv"), eval_csv=os.path.join(tmp, "eval.csv"),
                privacy_csv=os.path.join(tmp, "privacy.csv"), cohort_csv=os.path.join(tmp, "cohort.csv"),
                client_privacy_csv=os.path.join(tmp, "client_privacy.csv"), ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


def test_driver_checks_one_per_reason(tmp_path):
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train import fedavg as drv
    d = from_args(FedAvgConfig, entry.build_parser().parse_args([]))
    assert (d.aggregate, d.trim_frac, d.flip_clients) == ("mean", 0.0, 0)
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(
        ["--clients-per-gpu", "64", "--cohort", "8", "--aggregate", "trimmed", "--trim-frac", "0.25", "--flip-clients",
         "16"]))
    assert (cfg.aggregate, cfg.trim_frac, cfg.flip_clients) == ("trimmed", 0.25, 16)
    assert drv.check_robust_config(cfg) == 2
    t = str(tmp_path)
    for kw, match in (
            (dict(aggregate="krum"), "--aggregate must be one of"),
            (dict(clients_per_gpu=1, cohort=0), "need client sampling"),
            (dict(aggregate="mean", flip_clients=1, clients_per_gpu=1, cohort=0), "need client sampling"),
            (dict(aggregate="mean", trim_frac=0.25, clients_per_gpu=1, cohort=0), "need client sampling"),
            (dict(trim_frac=0.25), "--trim-frac is the share --aggregate trimmed drops"),
            (dict(aggregate="weighted", trim_frac=0.25), "--trim-frac is the share --aggregate trimmed drops"),
            (dict(aggregate="trimmed"), "--aggregate trimmed needs --trim-frac"),
            (dict(aggregate="trimmed", trim_frac=0.5), r"--trim-frac must be in \(0, 0.5\)"),
            (dict(aggregate="trimmed", trim_frac=-0.25), r"--trim-frac must be in \(0, 0.5\)"),
            (dict(aggregate="trimmed", trim_frac=0.1), "drops floor"),
            (dict(flip_clients=-1), "--flip-clients must be in"),
            (dict(flip_clients=9), "--flip-clients must be in"),
            (dict(clients_per_gpu=128, cohort=65), "at most 64 clients"),
            (dict(clients_per_gpu=65, cohort=0), "at most 64 clients"),
            (dict(client_dp_clip=1.0), "--aggregate median does not support --client-dp-clip: the sensitivity of a "
                                       "trimmed mean is not C / M"),
            (dict(aggregate="trimmed", trim_frac=0.25, client_dp_clip=1.0),
             "--aggregate trimmed does not support --client-dp-clip")):
        with pytest.raises(ValueError, match=match):
            drv.check_robust_config(_cfg(t, **kw))
    # accepted, with k
    for kw, k in ((dict(), 1), (dict(cohort=0), 3), (dict(aggregate="trimmed", trim_frac=0.25), 1),
                  (dict(aggregate="mean"), 0), (dict(aggregate="mean", flip_clients=8), 0),
                  (dict(clients_per_gpu=128, cohort=64), 31), (dict(server_opt="adam", server_scope="global"), 1),
                  (dict(prox_mu=0.1, client_partition="shards"), 1), (dict(aggregate="mean", client_dp_clip=1.0), 0),
                  (dict(aggregate="mean", clients_per_gpu=1, cohort=0), 0)):
        assert drv.check_robust_config(_cfg(t, **kw)) == k, kw
        wcfg, robust = drv.split_aggregate(_cfg(t, **kw))  # the checks of the weights see a robust estimate as "mean"
        assert wcfg.aggregate in ("mean", "weighted", "nova") and (robust != "none") == (k > 0)
        drv.check_hetero_config(wcfg)
    # a robust aggregate alone is not "unequal clients": no STEPS reduce, no cohort_shape events
    assert not drv.hetero_on(drv.split_aggregate(_cfg(t))[0])
    assert drv.hetero_on(drv.split_aggregate(_cfg(t, local_epochs=1))[0])
    # the driver stops before any configuration trains
    for kw, match in ((dict(client_dp_clip=1.0), "--client-dp-clip"), (dict(trim_frac=0.25), "--trim-frac"),
                      (dict(flip_clients=9), "--flip-clients")):
        with pytest.raises(ValueError, match=match):
            drv.run_fedavg(_cfg(t, **kw), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv"))


def _run_world1(tmp, **kw):
    from crossscale_ecg.train import fedavg as drv
    kept = []
    real = drv.make_trainer
    drv.make_trainer = lambda *a: kept.append(real(*a)) or kept[-1]
    try:
        rows = drv.run_fedavg(_cfg(tmp, **kw), _ctx1())
    finally:
        drv.make_trainer = real
    return kept[0], rows


def test_driver_world1_event_resume_and_the_flags_act(tmp_path):
    from crossscale_ecg.utils.csvio import ROUND_COLUMNS
    a = str(tmp_path / "a")
    whole, rows = _run_world1(a, rounds=3, flip_clients=2, server_opt="adam", server_lr=0.05,
                              jsonl=str(tmp_path / "a.jsonl"))
    assert (whole.aggregate, whole.robust, whole.trim, whole.flip_clients) == ("mean", "median", 1, 2)
    assert len(rows) == 3
    ev = [e for e in map(json.loads, open(tmp_path / "a.jsonl"))]
    rob = [e for e in ev if e["event"] == "robust"]
    assert len(rob) == 1
    assert {k: rob[0][k] for k in ("aggregate", "trim_frac", "k", "flip_clients")} == \
        dict(aggregate="median", trim_frac=0.0, k=1, flip_clients=2)
    assert not [e for e in ev if e["event"] == "cohort_shape"]
    with open(os.path.join(a, "rounds.csv")) as f:
        assert f.readline().strip().split(",") == ROUND_COLUMNS  # no CSV schema change
    # --resume continues bitwise: no new state
    b = str(tmp_path / "b")
    kw = dict(flip_clients=2, server_opt="adam", server_lr=0.05, ckpt_every=1)
    first, _ = _run_world1(b, rounds=1, **kw)
    part, _ = _run_world1(b, rounds=3, resume=True, **kw)
    assert first.cohort_round == 1 and part.cohort_round == 3
    assert torch.equal(_flat(part.model), _flat(whole.model))
    assert torch.equal(part.server_m, whole.server_m) and torch.equal(part.server_v, whole.server_v)
    # the flags act, each on its own
    ends = {"median+flip": _flat(_run_world1(str(tmp_path / "c"), flip_clients=2)[0].model)}
    for name, kw in (("median", dict()), ("mean", dict(aggregate="mean")), ("mean+flip", dict(aggregate="mean", flip_clients=2)),
                     ("trimmed", dict(aggregate="trimmed", trim_frac=0.25, cohort=8)), ("median8", dict(cohort=8))):
        ends[name] = _flat(_run_world1(str(tmp_path / name), **kw)[0].model)
    names = list(ends)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert not torch.equal(ends[p], ends[q]), (p, q)
    # no event without the flags
    _run_world1(str(tmp_path / "off"), aggregate="mean", jsonl=str(tmp_path / "off.jsonl"))
    assert not [e for e in map(json.loads, open(tmp_path / "off.jsonl")) if e["event"] == "robust"]


def test_entry_point_on_the_torch_backend(tmp_path):
    args = [sys.executable, os.path.join(ROOT, "part3_fedavg_overlap_mpi_gpu.py"), "--synthetic-windows", "256",
            "--labels", "parity", "--win-len", "64", "--batch-size", "8", "--local-steps", "2", "--rounds", "2",
            "--config", "G0", "--kernel-backend", "torch", "--aggregate", "median", "--flip-clients", "2",
            "--clients-per-gpu", "8", "--cohort", "4", "--results-csv", str(tmp_path / "r.csv"),
            "--cohort-csv", str(tmp_path / "c.csv"), "--jsonl", str(tmp_path / "log.jsonl"), "--quiet"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run(args, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout
    ev = [e for e in map(json.loads, open(tmp_path / "log.jsonl"))]
    rob = [e for e in ev if e["event"] == "robust"]
    assert len(rob) == 1 and (rob[0]["aggregate"], rob[0]["k"], rob[0]["flip_clients"]) == ("median", 1, 2)
    assert [e["round_idx"] for e in ev if e["event"] == "round"] == [0, 1]
    bad = subprocess.run(args + ["--trim-frac", "0.25"], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    assert bad.returncode != 0 and "--trim-frac is the share --aggregate trimmed drops" in bad.stdout


# ------------------------------------------------------------------------------------------------ 5: gloo world 2
RUNS = {"rank": dict(), "global": dict(server_scope="global", server_opt="adam", server_lr=0.05)}


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    penv._CTX = None
    try:
        from crossscale_ecg.train import fedavg as drv
        drv.usable_cpus = lambda: 1
        torch.set_num_threads(1)
        ctx = penv.init_distributed(backend="gloo", prefer_gpu=False)
        kept = []
        real = drv.make_trainer
        drv.make_trainer = lambda *a: kept.append(real(*a)) or kept[-1]
        out = {}
        for name, kw in RUNS.items():
            del kept[:]
            drv.run_fedavg(_cfg(os.path.join(tmp, name), flip_clients=1, **kw), ctx)
            out[name] = _flat(kept[0].model).tolist()
        q.put((rank, "ok", out))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


class Ctx2(penv.DistContext):  # a rank of 2 initialised ranks, without a process group
    distributed = True


def _emulate(tmp, rounds, **kw):
    """The definition for W = 2 ranks in one process: every rank trims within its own cohort, and the ranks' results -
    their weights under scope "rank", their deltas under scope "global" - are averaged as (a + b) / 2 in fp32."""
    from crossscale_ecg.models import build_model
    from crossscale_ecg.train import fedavg as drv
    cfg = _cfg(tmp, flip_clients=1, **kw)
    trainers = []
    for k in range(2):
        ctx = Ctx2(k, 2, k, "gloo", torch.device("cpu"))
        x, y = drv.load_client_data(cfg, ctx)
        x, y, _, _ = drv.split_holdout(cfg, x, y, k)
        torch.manual_seed(cfg.seed)
        trainers.append(drv.make_trainer(cfg, "G0", build_model(cfg.model, cfg.num_classes), x, y, ctx, "torch"))
    for _ in range(rounds):
        for tr in trainers:
            assert tr.trim == 1
            tr.prepare_round(cfg.local_steps)
            tr.launch_round(cfg.local_steps)
        if cfg.server_scope == "global":
            avg = (trainers[0].server_delta + trainers[1].server_delta) / 2
            for tr in trainers:
                tr.server_delta.copy_(avg)
                tr.apply_server_step()
        else:
            avg = (_flat(trainers[0].model) + _flat(trainers[1].model)) / 2
            for tr in trainers:
                with torch.no_grad():
                    torch.nn.utils.vector_to_parameters(avg.clone(), tr.model.parameters())
    return _flat(trainers[0].model)


def test_gloo_world2_is_the_mean_of_the_per_rank_estimates(tmp_path):
    """Each rank trims within its own cohort; all_reduce(AVG) averages the ranks' weights (scope "rank") or deltas
    (scope "global").  Against the one-process emulation: relative l2 at most 2^-23 - the average of two fp32 values
    is one rounding however the collective orders it, and everything else is the same fp32 program."""
    from test_cohort_global_server_cpu import _free_port
    tmp = str(tmp_path)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, tmp, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = {}
    for _ in range(2):
        rank, status, res = q.get(timeout=300)
        assert status == "ok", res
        got[rank] = res
    for p in ps:
        p.join(timeout=60)
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for name, kw in RUNS.items():
            assert got[0][name] == got[1][name], name
            want = _emulate(os.path.join(tmp, "emu_" + name), 2, **kw)
            have = torch.tensor(got[0][name], dtype=torch.float32)
            rel = float((have - want).norm() / want.norm())
            print(f"gloo world 2, median, scope {name}: relative l2 against the emulation {rel:.3e}")
            assert rel <= 2.0 ** -23, name
    finally:
        torch.set_num_threads(prev)
