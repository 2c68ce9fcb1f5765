"""Unequal virtual clients on the CPU: ``dirichlet_partition``, ``CohortSampler(sizes=...)`` and ``steps_of``,
``weights_of`` (mean, weighted, FedNova), ``TorchCohortTrainer`` with per-client local steps and a weighted aggregate
against a float64 loop of the definitions, and the driver's ``--client-partition dirichlet --client-alpha`` /
``--local-epochs`` / ``--aggregate`` flags on the torch backend: rejected combinations, the ``cohort_shape`` event,
``samples_per_s`` and ``--resume``."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv

LR, MOM, WD = 0.1, 0.9, 1e-2
B, S, L, N = 4, 5, 64, 200
# fp32 trainer against the float64 loop, relative l2 of the global weights after one round of at most S = 5 steps:
# every weight is rounded once per step (2^-24 each) and the fp32 gradients carry a few 1e-6 of |d|, scaled by
# lr * sum of the momentum factors (< 0.1 * 10) relative to |p|: 5 * 6e-8 + 1 * 5e-6 < 1e-5, the siblings' bound
TOL = 1e-5


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _data(seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, L, generator=g)
    return x, (x.mean(1) > 0).long()


# ------------------------------------------------------------------------------------------------ 1: the partition
@pytest.mark.parametrize("n_rows,K,alpha,nc", [(200, 6, 0.5, 2), (333, 10, 0.1, 5), (64, 16, 0.05, 3), (48, 12, 100.0, 2)])
def test_dirichlet_partition(n_rows, K, alpha, nc):
    from crossscale_ecg.data.dataset import client_partition, dirichlet_partition
    y = torch.randint(0, nc, (n_rows,), generator=torch.Generator().manual_seed(n_rows))
    order, sizes = dirichlet_partition(y, K, alpha, B, seed=11)
    assert order.dtype == sizes.dtype == torch.int64 and tuple(sizes.shape) == (K,)
    assert tuple(order.shape) == (K, int(sizes.max()))
    assert int(sizes.min()) >= B and int(sizes.sum()) <= n_rows  # every client holds a batch; no row is invented
    rows = [order[k, : int(sizes[k])].tolist() for k in range(K)]
    flat = [r for rs in rows for r in rs]
    assert len(set(flat)) == len(flat) and min(flat) >= 0 and max(flat) < n_rows  # disjoint clients, valid rows
    assert int(order.min()) >= 0 and int(order.max()) < n_rows  # the padding holds valid rows too
    # a pure function of its arguments; seed and alpha act
    again = dirichlet_partition(y.clone(), K, alpha, B, seed=11)
    assert torch.equal(again[0], order) and torch.equal(again[1], sizes)
    other = dirichlet_partition(y, K, alpha, B, seed=12)
    assert not (torch.equal(other[1], sizes) and torch.equal(other[0], order))
    via = client_partition("dirichlet", y, K, 2, 11, "cpu", alpha=alpha, min_rows=B)
    assert torch.equal(via[0], order) and torch.equal(via[1], sizes)


def test_dirichlet_partition_skews_sizes_and_labels_and_rejects_bad_arguments():
    from crossscale_ecg.data.dataset import PARTITIONS, client_partition, dirichlet_partition
    assert PARTITIONS == ("contiguous", "shards", "dirichlet")
    y = torch.randint(0, 2, (4000,), generator=torch.Generator().manual_seed(0))
    _, skew = dirichlet_partition(y, 8, 0.1, B, seed=1)
    order, even = dirichlet_partition(y, 8, 1000.0, B, seed=1)
    assert int(skew.max()) > 4 * int(skew.min()) and int(even.max()) < 1.3 * int(even.min())
    assert int(even.sum()) == 4000  # nothing is dropped when no client needs topping up
    share = torch.stack([y[order[k, : int(even[k])]].float().mean() for k in range(8)])
    assert float((share - 0.5).abs().max()) < 0.1  # alpha -> inf: every client sees the global label mix
    with pytest.raises(ValueError, match="alpha > 0"):
        dirichlet_partition(y, 8, 0.0, B, seed=1)
    with pytest.raises(RuntimeError, match="fewer than"):
        dirichlet_partition(y[:30], 8, 0.5, B, seed=1)
    with pytest.raises(ValueError, match="partition must be one of"):
        client_partition("dirichlet", y, 8, 2, 1, "cpu")  # no concentration


# ------------------------------------------------------------------------------------------------ 2: the sampler
def _table_of_today(n_windows, batch, steps, clients, cohort, seed, r):
    """The table ``CohortSampler.fill`` writes for equal clients (its lines, kept here as the reference)."""
    from crossscale_ecg.utils.philox import mix64
    n = n_windows // clients
    passes = (steps * batch + n - 1) // n
    round_seed = mix64(seed) ^ int(r)
    g = torch.Generator()
    g.manual_seed(round_seed)
    ids = torch.randperm(clients, generator=g)[:cohort].tolist()
    g = torch.Generator(device="cpu")
    g.manual_seed(mix64(round_seed))
    keys = torch.randint(0, 1 << 62, (cohort, passes, n), generator=g, dtype=torch.int64)
    rows = keys.argsort(dim=2).reshape(cohort, passes * n)[:, : steps * batch]
    rows = rows + (torch.tensor(ids, dtype=torch.int64) * n)[:, None]
    return ids, rows.view(cohort, steps, batch).permute(1, 0, 2).reshape(steps, cohort * batch).to(torch.int32)


def test_ragged_sampler():
    from crossscale_ecg.data.dataset import CohortSampler, dirichlet_partition
    K, M = 6, 4
    y = torch.randint(0, 2, (N,), generator=torch.Generator().manual_seed(1))
    order, sizes = dirichlet_partition(y, K, 0.3, B, seed=7)
    s = CohortSampler(N, B, S, K, M, "cpu", seed=7, order=order, sizes=sizes)
    n_min = int(sizes.min())
    assert n_min < S * B, "the case must wrap the smallest client"
    assert s.passes == -(-S * B // n_min) and s.sizes == sizes.tolist()
    for r in range(6):
        table = torch.zeros((S, M * B), dtype=torch.int32)
        ids = s.fill(r, table)
        assert ids == s.clients_of(r) == CohortSampler(N, B, S, K, M, "cpu", seed=7).clients_of(r)
        assert s.sizes_of(ids) == [int(sizes[k]) for k in ids]
        for j, k in enumerate(ids):
            n_k = int(sizes[k])
            seq = table[:, j * B:(j + 1) * B].reshape(-1).long()  # the client's rows in the order it consumes them
            own = order[k, :n_k]
            assert bool(torch.isin(seq, own).all()), (r, k)  # every entry - cut-off steps included - is its own row
            for p in range(0, S * B, n_k):  # no row twice within one pass; a full pass takes every row once
                chunk = seq[p:p + n_k]
                assert chunk.unique().numel() == chunk.numel()
                assert chunk.numel() < n_k or set(chunk.tolist()) == set(own.tolist())
        again = torch.zeros_like(table)
        assert s.fill(r, again) == ids and torch.equal(again, table)  # stateless
    # sizes=None: today's tables, bit for bit
    for sampler in (CohortSampler(N, B, S, K, M, "cpu", seed=7), CohortSampler(N, B, S, K, M, "cpu", seed=7, sizes=None)):
        for r in (0, 1, 5):
            table = torch.zeros((S, M * B), dtype=torch.int32)
            ids = sampler.fill(r, table)
            want_ids, want = _table_of_today(N, B, S, K, M, 7, r)
            assert ids == want_ids and torch.equal(table, want)
    with pytest.raises(ValueError, match="sizes need order"):
        CohortSampler(N, B, S, K, M, "cpu", seed=7, sizes=sizes)
    with pytest.raises(ValueError, match="sizes must be"):
        CohortSampler(N, B, S, K, M, "cpu", seed=7, order=order, sizes=sizes[:3])
    with pytest.raises(RuntimeError, match="per client < batch"):
        CohortSampler(N, B, S, K, M, "cpu", seed=7, order=order, sizes=torch.full((K,), B - 1))


def test_steps_of():
    from crossscale_ecg.data.dataset import CohortSampler
    K = 4
    order = torch.arange(K * 30, dtype=torch.int64).view(K, 30)
    s = CohortSampler(N, B, S, K, K, "cpu", seed=1, order=order, sizes=torch.tensor([4, 7, 9, 30]))
    ids = [0, 1, 2, 3]
    assert s.steps_of(ids, 0) == [S] * 4  # E = 0: S for everyone
    assert s.steps_of(ids, 1) == [1, 1, 2, 5]  # min(S, max(1, E * (n_k // B)))
    assert s.steps_of(ids, 2) == [2, 2, 4, 5]
    assert s.steps_of([3, 0], 1) == [5, 1]
    equal = CohortSampler(N, B, S, K, K, "cpu", seed=1)  # n = 50
    assert equal.sizes_of(ids) == [50] * 4 and equal.steps_of(ids, 1) == [5] * 4
    with pytest.raises(ValueError, match="local_epochs"):
        s.steps_of(ids, -1)


# ------------------------------------------------------------------------------------------------ 3: the weights
def test_weights_of():
    from crossscale_ecg.train.cohort import nova_norm, weights_of
    sizes, steps = [10, 30, 60, 7], [1, 3, 5, 2]
    for mode in ("mean", "weighted"):
        w = weights_of(sizes, steps, mode, 0.9)
        assert abs(sum(np.float64(v) for v in w) - 1.0) < 4 * 2.0 ** -24  # each weight rounded once to fp32
        assert all(float(np.float32(v)) == v for v in w)  # fp32 values
    assert weights_of(sizes, steps, "mean") == [0.25] * 4
    assert weights_of(sizes, steps, "weighted") == [float(np.float32(n / 107.0)) for n in sizes]
    # the normaliser is the displacement of tau momentum steps under a unit gradient and unit learning rate
    for rho in (0.0, 0.5, 0.9, 0.99):
        for tau in (1, 2, 5, 50):
            m = x = 0.0
            for _ in range(tau):
                m = rho * m + 1.0
                x += m
            assert abs(nova_norm(tau, rho) - x) <= 1e-12 * x, (rho, tau)
        assert nova_norm(7, 0.0) == 7.0
    for rho in (0.0, 0.9):
        # equal steps: tau_eff / a_c is 1, nova is weighted
        assert weights_of(sizes, [3] * 4, "nova", rho) == weights_of(sizes, [3] * 4, "weighted", rho)
        w = weights_of(sizes, steps, "nova", rho)
        p = [n / 107.0 for n in sizes]
        a = [nova_norm(t, rho) for t in steps]
        tau_eff = sum(pc * ac for pc, ac in zip(p, a))
        assert w == [float(np.float32(pc * tau_eff / ac)) for pc, ac in zip(p, a)]
        assert w[0] > p[0] and w[2] < p[2]  # short clients are scaled up, long ones down
    with pytest.raises(ValueError, match="aggregate must be one of"):
        weights_of(sizes, steps, "median")
    with pytest.raises(ValueError, match="per client"):
        weights_of(sizes, steps[:3], "mean")


# ------------------------------------------------------------------------------------------------ 4: the trainer
def _sgd64(model, x, y, batches, mom=MOM):
    """``len(batches)`` SGD steps from zero momentum on a float64 copy of ``model``; returns the flat weights."""
    m64 = copy.deepcopy(model).double()
    if getattr(m64, "_flat", None) is not None:
        m64._flat = None
    ps = list(m64.parameters())
    bufs = [torch.zeros_like(p) for p in ps]
    m64.train()
    for sel in batches:
        loss = F.cross_entropy(m64(x[sel].double().unsqueeze(1)), y[sel])
        grads = torch.autograd.grad(loss, ps)
        with torch.no_grad():
            for p, g, buf in zip(ps, grads, bufs):
                buf.mul_(mom).add_(g + WD * p)
                p.sub_(LR * buf)
    return _flat(m64)


def _trainer(**kw):
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = _data()
    torch.manual_seed(0)
    model = TinyECG()
    args = dict(clients=6, cohort=3, lr=LR, momentum=MOM, weight_decay=WD, amp_dtype=None, seed=5)
    args.update(kw)
    return model, TorchCohortTrainer(model, x, y, B, S, **args)


@pytest.mark.parametrize("aggregate", ["mean", "weighted", "nova"])
def test_torch_cohort_trainer_against_the_float64_definition(aggregate):
    from crossscale_ecg.train.cohort import weights_of
    x, y = _data()
    model, tr = _trainer(partition="dirichlet", dirichlet_alpha=0.3, local_epochs=1, aggregate=aggregate)
    assert tr.hetero and tr.sampler.sizes is not None
    varied = False
    for rnd in range(3):
        start = copy.deepcopy(model)
        tr.run_round(S)
        sizes, steps, weights = tr.last_round_shape()
        ids = tr.round_clients
        assert sizes == tr.sampler.sizes_of(ids) and steps == tr.sampler.steps_of(ids, 1)
        assert weights == weights_of(sizes, steps, aggregate, MOM)
        varied = varied or len(set(steps)) > 1
        g = _flat(start).double()
        want = g.clone()
        for j in range(3):  # client j runs its first S_j table rows
            batches = [tr.table[s, j * B:(j + 1) * B].long() for s in range(steps[j])]
            want += weights[j] * (_sgd64(start, x, y, batches) - g)
        rel = float((_flat(model).double() - want).norm() / want.norm())
        print(f"TorchCohortTrainer {aggregate} round {rnd}: steps {steps} sizes {sizes} rel l2 {rel:.3e}")
        assert rel < TOL
    assert varied, "no round with unequal steps: the case checks nothing"
    assert tr.avg_loss() > 0


def test_defaults_reproduce_the_equal_clients_trainer_bitwise():
    """Equal sizes, E = 0 and ``mean`` - given or left out - are the trainer of before: the table, the clients' S
    steps and ``sum / M``, written out here."""
    x, y = _data()
    model, tr = _trainer(local_epochs=0, aggregate="mean", dirichlet_alpha=0.0)
    model2, tr2 = _trainer()
    assert not tr.hetero and tr.sampler.sizes is None
    for rnd in range(2):
        start = copy.deepcopy(model)
        tr.run_round(S)
        tr2.run_round(S)
        assert torch.equal(_flat(model), _flat(model2)) and tr.avg_loss() == tr2.avg_loss()
        total, losses = None, 0.0
        for j in range(3):
            work = copy.deepcopy(start)
            opt = torch.optim.SGD(work.parameters(), lr=LR, momentum=MOM, weight_decay=WD)
            work.train()
            for s in range(S):
                sel = tr.table[s, j * B:(j + 1) * B].long()
                opt.zero_grad(set_to_none=True)
                loss = F.cross_entropy(work(x[sel].unsqueeze(1)), y[sel])
                loss.backward()
                opt.step()
                losses = losses + loss.detach().float()
            ps = [p.detach().clone() for p in work.parameters()]
            total = ps if total is None else [t + p for t, p in zip(total, ps)]
        want = torch.cat([(t * torch.tensor(1.0 / 3, dtype=torch.float32)).reshape(-1) for t in total])
        assert torch.equal(_flat(model), want)
        assert tr.avg_loss() == float(losses) / (3 * S)
        assert tr.last_round_shape() == ([N // 6] * 3, [S] * 3, [float(np.float32(1 / 3))] * 3)


def test_trainers_reject_what_the_aggregates_do_not_support():
    for kw, match in ((dict(aggregate="median"), "aggregate must be one of"),
                      (dict(local_epochs=-1), "local_epochs must be >= 0"),
                      (dict(aggregate="weighted", client_dp_clip=1.0), "not combined with client-level DP"),
                      (dict(aggregate="nova", client_dp_clip=1.0), "not combined with client-level DP"),
                      (dict(aggregate="nova", nesterov=True), "nesterov momentum or FedProx"),
                      (dict(aggregate="nova", prox_mu=0.1), "nesterov momentum or FedProx"),
                      (dict(partition="dirichlet"), "partition must be one of")):
        with pytest.raises(ValueError, match=match):
            _trainer(**kw)
    _trainer(aggregate="weighted", prox_mu=0.1, server_opt="adam", server_scope="global")  # compose


# ------------------------------------------------------------------------------------------------ 5: the driver
def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=3, local_steps=4, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=6, cohort=3, client_partition="dirichlet",
                client_alpha=0.3, local_epochs=1, aggregate="weighted", results_csv=os.path.join(tmp, "rounds.csv"),
                eval_csv=os.path.join(tmp, "eval.csv"), privacy_csv=os.path.join(tmp, "privacy.csv"),
                cohort_csv=os.path.join(tmp, "cohort.csv"), client_privacy_csv=os.path.join(tmp, "client_privacy.csv"),
                ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


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


def test_flags_parse_and_every_rejected_combination_raises_with_its_reason(tmp_path):
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train import fedavg as drv
    d = from_args(FedAvgConfig, entry.build_parser().parse_args([]))
    assert (d.client_alpha, d.local_epochs, d.aggregate) == (0.0, 0, "mean")
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(
        ["--clients-per-gpu", "64", "--cohort", "8", "--client-partition", "dirichlet", "--client-alpha", "0.5",
         "--local-epochs", "2", "--aggregate", "nova"]))
    assert (cfg.client_partition, cfg.client_alpha, cfg.local_epochs, cfg.aggregate) == ("dirichlet", 0.5, 2, "nova")
    t = str(tmp_path)
    plain = dict(client_partition="contiguous", client_alpha=0.0, local_epochs=0, aggregate="mean")
    for kw, match in (
            (dict(aggregate="median"), "--aggregate must be one of"),
            (dict(local_epochs=-1), "--local-epochs must be >= 0"),
            (dict(client_alpha=-1.0), "--client-alpha must be > 0"),
            (dict(client_partition="shards"), "--client-alpha is the concentration"),
            (dict(clients_per_gpu=1, cohort=0), "need client sampling"),
            (dict(plain, clients_per_gpu=1, cohort=0, local_epochs=1), "need client sampling"),
            (dict(plain, clients_per_gpu=1, cohort=0, aggregate="weighted"), "need client sampling"),
            (dict(client_dp_clip=1.0), "--aggregate weighted does not support --client-dp-clip"),
            (dict(aggregate="nova", client_dp_clip=1.0), "--aggregate nova does not support --client-dp-clip"),
            (dict(aggregate="mean", client_dp_clip=1.0), "--local-epochs does not support --client-dp-clip"),
            (dict(aggregate="mean", local_epochs=0, client_dp_clip=1.0),
             "--client-partition dirichlet does not support --client-dp-clip"),
            (dict(aggregate="nova", prox_mu=0.1), "--aggregate nova does not support --prox-mu")):
        with pytest.raises(ValueError, match=match):
            drv.check_hetero_config(_cfg(t, **kw))
    with pytest.raises(ValueError, match="--client-partition must be one of"):
        drv.check_prox_config(_cfg(t, client_alpha=0.0), "G0", "torch")  # dirichlet without its concentration
    # accepted: with FedProx (not nova), the server optimizers and the split close; everything off
    for kw in (dict(prox_mu=0.1), dict(server_opt="adam", server_scope="global"), dict(aggregate="nova", server_opt="sgdm"),
               dict(plain), dict(plain, clients_per_gpu=1, cohort=0), dict(plain, client_dp_clip=1.0)):
        drv.check_hetero_config(_cfg(t, **kw))
        drv.check_prox_config(_cfg(t, **kw), "G0", "torch")
    # the driver stops before any configuration trains
    for kw, match in ((dict(client_dp_clip=1.0), "--client-dp-clip"), (dict(aggregate="nova", prox_mu=0.1), "--prox-mu"),
                      (dict(plain, clients_per_gpu=1, cohort=0, local_epochs=1), "--clients-per-gpu")):
        with pytest.raises(ValueError, match=match):
            drv.run_fedavg(_cfg(t, **kw), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv"))


def test_driver_world1_shape_event_samples_and_resume(tmp_path):
    from crossscale_ecg.train.cohort import weights_of
    from crossscale_ecg.utils.csvio import COHORT_COLUMNS, ROUND_COLUMNS
    a = str(tmp_path / "a")
    whole, rows = _run_world1(a, jsonl=str(tmp_path / "a.jsonl"))
    assert (whole.partition, whole.local_epochs, whole.aggregate) == ("dirichlet", 1, "weighted")
    ev = [e for e in map(json.loads, open(tmp_path / "a.jsonl")) if e["event"] == "cohort_shape"]
    assert [e["round_idx"] for e in ev] == [0, 1, 2]  # one per round
    for e, row in zip(ev, rows):
        ids = whole.sampler.clients_of(e["round_idx"])
        sizes, steps = whole.sampler.sizes_of(ids), whole.sampler.steps_of(ids, 1)
        assert (e["sizes_rank0"], e["steps_rank0"]) == (sizes, steps)
        assert e["weights_rank0"] == weights_of(sizes, steps, "weighted", 0.9)
        assert (e["aggregate"], e["local_epochs"], e["client_alpha"]) == ("weighted", 1, 0.3)
        # samples_per_s counts B * sum_c S_c
        assert row["samples_per_s"] == pytest.approx(8 * sum(steps) / (row["local_train_ms"] / 1e3), rel=1e-9)
    assert any(len(set(e["steps_rank0"])) > 1 for e in ev), "no round with unequal steps: the case checks nothing"
    with open(os.path.join(a, "rounds.csv")) as f:
        assert f.readline().strip().split(",") == ROUND_COLUMNS  # no CSV schema change
    with open(os.path.join(a, "cohort.csv")) as f:
        assert f.readline().strip().split(",") == COHORT_COLUMNS
    # a run resumed at round r draws round r's sizes, steps and weights, and ends on the whole run's weights
    b = str(tmp_path / "b")
    first, _ = _run_world1(b, rounds=1, ckpt_every=1)
    assert first.cohort_round == 1
    part, _ = _run_world1(b, rounds=3, ckpt_every=1, resume=True, jsonl=str(tmp_path / "b.jsonl"))
    assert part.cohort_round == 3 and torch.equal(_flat(part.model), _flat(whole.model))
    assert part.last_round_shape() == whole.last_round_shape()
    evb = [e for e in map(json.loads, open(tmp_path / "b.jsonl")) if e["event"] == "cohort_shape"]
    assert [(e["round_idx"], e["sizes_rank0"], e["steps_rank0"], e["weights_rank0"]) for e in evb] == \
        [(e["round_idx"], e["sizes_rank0"], e["steps_rank0"], e["weights_rank0"]) for e in ev[1:]]
    # the flags act, each on its own
    ends = {"whole": _flat(whole.model)}
    for name, kw in (("mean", dict(aggregate="mean")), ("nova", dict(aggregate="nova")), ("E0", dict(local_epochs=0)),
                     ("alpha", dict(client_alpha=5.0))):
        ends[name] = _flat(_run_world1(str(tmp_path / name), **kw)[0].model)
    names = list(ends)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert not torch.equal(ends[p], ends[q]), (p, q)
    # no event without the flags
    _run_world1(str(tmp_path / "off"), client_partition="contiguous", client_alpha=0.0, local_epochs=0,
                aggregate="mean", jsonl=str(tmp_path / "off.jsonl"))
    assert not [e for e in map(json.loads, open(tmp_path / "off.jsonl")) if e["event"] == "cohort_shape"]
