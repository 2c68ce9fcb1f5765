"""Record-level DP-SGD inside cohort rounds, on the CPU: ``TorchCohortTrainer``'s definition (no clip and no noise is
the trainer without DP; one client's noised step; resume of the step counter) and the driver (the flags with client
sampling, the combinations that stay rejected, the per-round rows of the privacy CSV, their resume).

The definition (train/cohort.py): local step s of cohort slot j clips its B per-sample gradients to l2 norm C, sums
them, adds sigma * C * z and divides by B, with z = philox.normal(dp_seed, t0 + s, P, stream=2 + j) and t0 the trainer's
``dp_steps`` at the round's start, which every round advances by its step count."""
import os

import numpy as np
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.data.dataset import CohortSampler
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv
from crossscale_ecg.utils import philox, privacy
from crossscale_ecg.utils.csvio import PRIVACY_COLUMNS, read_csv

P = 1458  # TinyECG, 2 classes
B, S, K, M, L, N = 5, 3, 4, 3, 64, 48
LR = 1e-2


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _data():
    g = torch.Generator().manual_seed(3)
    return torch.randn(N, L, generator=g), torch.randint(0, 2, (N,), generator=g)


def _trainer(model=None, **kw):
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = _data()
    torch.manual_seed(0)
    model = TinyECG() if model is None else model
    return TorchCohortTrainer(model, x, y, B, S, clients=K, cohort=M, lr=LR, momentum=0.9, amp_dtype=None, seed=5, **kw)


# ------------------------------------------------------------------------------------------------ the trainer
def test_huge_clip_and_no_noise_is_the_trainer_without_dp():
    plain, dp = _trainer(), _trainer(dp_clip=1e9, dp_seed=77)
    assert dp.dp and not plain.dp
    for _ in range(2):
        plain.run_round(S)
        dp.run_round(S)
    a, b = _flat(plain.model), _flat(dp.model)
    rel = ((a - b).norm() / a.norm()).item()
    print(f"dp_clip = 1e9, no noise vs no DP: relative l2 difference {rel:.3e}")
    assert rel <= 1e-6  # per-sample gradients summed in another order than the batch's backward pass
    assert abs(plain.avg_loss() - dp.avg_loss()) < 1e-5
    assert dp.dp_steps == 2 * S and plain.dp_steps == 0 and dp.round_clients == plain.round_clients


@pytest.mark.parametrize("j", [0, 2])
def test_one_clients_noised_step_adds_lr_sigma_C_over_B_z_of_its_stream(j):
    """One step from the global weights with zero initial momentum moves by lr * gradient, so the noised and the
    noiseless step differ by lr * sigma * C / B * z(stream = 2 + j) - and not by another client's or step's draw."""
    sigma, clip, t0 = 1.3, 0.7, (1 << 32) + 11
    quiet, noisy = _trainer(dp_clip=clip, dp_seed=77), _trainer(dp_clip=clip, dp_noise=sigma, dp_seed=77)
    outs = []
    for tr in (quiet, noisy):
        tr.set_dp_steps(t0)
        tr.sampler.fill(0, tr.table)
        outs.append(torch.cat([p.reshape(-1) for p in tr._client_round(j, 1, tr.table)]).double())
    diff = outs[0] - outs[1]  # w - lr (g + nu z) against w - lr g
    nu = sigma * clip / B
    want = LR * nu * torch.from_numpy(philox.normal(77, t0, P, stream=2 + j))
    tol = 4 * 2.0 ** -24 * (outs[0].abs().max().item() + LR * nu * 5.77)  # fp32 roundings of the update
    assert (diff - want).abs().max().item() <= tol
    for other in (philox.normal(77, t0, P, stream=2 + (j + 1) % M), philox.normal(77, t0 + 1, P, stream=2 + j),
                  philox.normal(77, t0, P, stream=0)):
        assert (diff - LR * nu * torch.from_numpy(other)).abs().max().item() > 0.1 * LR * nu


def test_resumed_trainer_continues_bit_for_bit_only_with_its_step_counter():
    kw = dict(dp_clip=0.7, dp_noise=1.1, dp_seed=77)
    full = _trainer(**kw)
    for _ in range(3):
        full.run_round(S)
    first = _trainer(**kw)
    for _ in range(2):
        first.run_round(S)
    assert first.dp_steps == 2 * S and first.cohort_round == 2
    ends = []
    for restore in (True, False):
        model = TinyECG()
        model.load_state_dict(first.model.state_dict())
        tr = _trainer(model, **kw)
        tr.set_cohort_round(first.cohort_round)
        if restore:
            tr.set_dp_steps(first.dp_steps)
        tr.run_round(S)
        ends.append(_flat(tr.model))
        assert tr.round_clients == full.round_clients
    assert torch.equal(ends[0], _flat(full.model)) and not torch.equal(ends[1], _flat(full.model))


def test_trainer_argument_checks():
    for kw, match in ((dict(dp_clip=-1.0), ">= 0"), (dict(dp_noise=1.0), "needs a clip norm"),
                      (dict(dp_clip=1.0, dp_seed=77, prox_mu=0.1), "FedProx"),
                      (dict(dp_clip=1.0, dp_noise=1.0), "needs dp_seed")):  # the noise key has no default
        with pytest.raises(ValueError, match=match):
            _trainer(**kw)
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = _data()
    with pytest.raises(ValueError, match="fp16"):
        TorchCohortTrainer(TinyECG(), x, y, B, S, clients=K, cohort=M, amp_dtype=torch.float16, dp_clip=1.0, dp_seed=77)
    # the checkpoint's per-rank state carries the counter of any trainer that has it
    from crossscale_ecg.utils.ckpt import load_trainer_local_state, trainer_local_state
    tr = _trainer(dp_clip=0.7, dp_noise=1.1, dp_seed=77)
    tr.run_round(S)
    st = trainer_local_state(tr)
    assert st["dp_steps"] == S and st["cohort_round"] == 1
    twin = _trainer(dp_clip=0.7, dp_noise=1.1, dp_seed=77)
    load_trainer_local_state(twin, st)
    assert twin.dp_steps == S and twin.cohort_round == 1


# ------------------------------------------------------------------------------------------------ the driver
def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=4, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=4, cohort=2, dp_clip=0.5, dp_noise=1.1,
                dp_delta=1e-5,
                results_csv=os.path.join(tmp, "rounds.csv"), eval_csv=os.path.join(tmp, "eval.csv"),
                privacy_csv=os.path.join(tmp, "privacy.csv"), cohort_csv=os.path.join(tmp, "cohort.csv"),
                client_privacy_csv=os.path.join(tmp, "client_privacy.csv"), ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


def test_flags_are_accepted_with_client_sampling_and_the_named_combinations_stay_rejected(tmp_path):
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train import fedavg as drv
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(
        ["--clients-per-gpu", "64", "--cohort", "8", "--dp-clip", "0.5", "--dp-noise", "1.1", "--dp-delta", "1e-6"]))
    assert (cfg.clients_per_gpu, cfg.cohort, cfg.dp_clip, cfg.dp_noise, cfg.dp_delta) == (64, 8, 0.5, 1.1, 1e-6)
    for backend in ("fused", "torch"):
        drv.check_dp_config(cfg, "G1", backend)
        drv.check_cohort_config(cfg, backend)
        drv.check_prox_config(cfg, "G1", backend)
    t = str(tmp_path)
    x, y = torch.randn(256, 64), torch.zeros(256, dtype=torch.long)
    tr = drv.make_trainer(_cfg(t), "G0", TinyECG(), x, y, _ctx1(), "torch")
    assert tr.dp and (tr.dp_clip, tr.dp_noise) == (0.5, 1.1) and tr.dp_seed == philox.mix64(1234)
    # with the client-level close as well: the two privacy units side by side
    tr = drv.make_trainer(_cfg(t, client_dp_clip=0.05, client_dp_noise=1.0), "G0", TinyECG(), x, y, _ctx1(), "torch")
    assert tr.dp and tr.cdp_clip == 0.05
    for kw, cname, match in ((dict(prox_mu=0.1), "G0", r"--prox-mu\) does not support DP-SGD"),
                             (dict(amp_dtype="fp16"), "G1", "does not support fp16 AMP"),
                             (dict(sync="ddp"), "G0", "--sync ddp"),
                             (dict(model="resnet1d"), "G0", "ResNet1D"),
                             (dict(dp_noise=-1.0), "G0", ">= 0"),
                             (dict(dp_noise=0.0), "G0", "only together with --dp-noise > 0"),
                             (dict(dp_delta=0.0), "G0", "--dp-delta")):
        with pytest.raises(ValueError, match=match):
            drv.run_fedavg(_cfg(t, config=cname, **kw), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv")) and not os.path.exists(os.path.join(t, "privacy.csv"))


def _counts(cfg, rounds):
    """Per round, the largest number of local steps any of the K clients has run so far: recounted from a sampler of
    one's own (the cohort of round r is a function of (seed, r))."""
    s = CohortSampler(cfg.synthetic_windows, cfg.batch_size, cfg.local_steps, cfg.clients_per_gpu, cfg.cohort, "cpu",
                      seed=cfg.seed)
    steps, out = [0] * cfg.clients_per_gpu, []
    for r in range(rounds):
        for k in s.clients_of(r):
            steps[k] += cfg.local_steps
        out.append(max(steps))
    return out


def test_driver_privacy_rows_follow_the_most_trained_client_and_survive_resume(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    full = _cfg(str(tmp_path / "full"))
    drv.run_fedavg(full, _ctx1())
    rows = read_csv(full.privacy_csv)
    with open(full.privacy_csv) as f:
        assert f.readline().strip().split(",") == PRIVACY_COLUMNS  # no schema change
    assert [int(r["round_idx"]) for r in rows] == [0, 1, 2, 3]  # one row per round
    want = _counts(full, 4)
    assert [int(r["steps"]) for r in rows] == want and want[0] == 2 and want[-1] < 4 * 2 * 4
    q = 8 / (256 // 4)  # B / n_k: a record is sampled from its own client's rows
    eps = [float(r["epsilon"]) for r in rows]
    for r, st, e in zip(rows, want, eps):
        assert abs(float(r["sample_rate"]) - q) < 1e-12 and float(r["noise_multiplier"]) == 1.1
        assert abs(e - privacy.epsilon(1.1, q, st, 1e-5)) <= 1e-9 * e
    assert all(b >= a for a, b in zip(eps, eps[1:])) and eps[0] > 0 and np.isfinite(eps).all()
    # the cohorts the recount assumed are the ones the run drew
    s = CohortSampler(256, 8, 2, 4, 2, "cpu", seed=1234)
    assert [[int(c) for c in r["clients_rank0"].split()] for r in read_csv(full.cohort_csv)] == \
        [s.clients_of(r) for r in range(4)]
    # two rounds, a checkpoint, --resume for the other two: the same rows
    part = str(tmp_path / "part")
    drv.run_fedavg(_cfg(part, rounds=2, ckpt_every=1), _ctx1())
    drv.run_fedavg(_cfg(part, ckpt_every=1, resume=True), _ctx1())
    prow = read_csv(_cfg(part).privacy_csv)
    assert [int(r["round_idx"]) for r in prow] == [0, 1, 2, 3]
    assert [int(r["steps"]) for r in prow] == want
    assert [float(r["epsilon"]) for r in prow] == eps
    from crossscale_ecg.utils.ckpt import ckpt_path, load_checkpoint
    drv.run_fedavg(_cfg(str(tmp_path / "full2"), ckpt_every=4), _ctx1())
    a = load_checkpoint(ckpt_path(_cfg(str(tmp_path / "full2")).ckpt_dir, 3, "G0"))["model"]
    b = load_checkpoint(ckpt_path(_cfg(part).ckpt_dir, 3, "G0"))["model"]
    assert all(torch.equal(a[k], b[k]) for k in a)  # the resumed run continued its noise streams
