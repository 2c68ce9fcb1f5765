"""Evaluation on the CPU: ``evaluate_torch``, the FedAvg driver's --eval-every / --eval-windows path with the torch
backend (world 1 and gloo world 2), and the symbols the HIP evaluation path is bound through."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv
from crossscale_ecg.utils.csvio import read_csv


def _cfg(tmp, **kw):
    base = dict(batch_size=32, rounds=2, local_steps=3, config="G0", kernel_backend="torch", synthetic_windows=512,
                labels="parity", win_len=96, eval_every=1, eval_windows=64, quiet=True,
                results_csv=os.path.join(tmp, "rounds.csv"), eval_csv=os.path.join(tmp, "eval.csv"),
                ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _conf(field):
    return [[int(v) for v in row.split()] for row in field.split(";")]


def test_symbols_exist():
    from crossscale_ecg.ops import fused_tiny, tiny_eval
    from crossscale_ecg.utils.csvio import EVAL_COLUMNS
    assert EVAL_COLUMNS == ["config", "world_size", "round_idx", "windows", "loss", "accuracy", "confusion", "eval_ms",
                            "backend", "precision"]
    cfg = FedAvgConfig()
    assert (cfg.eval_every, cfg.eval_windows, cfg.eval_csv) == (0, 0, "results/fedavg_eval.csv")
    assert callable(tiny_eval.tiny_evaluate) and callable(tiny_eval.evaluate_torch)
    assert callable(fused_tiny.FusedTinyTrainer.evaluate) and fused_tiny.tiny_evaluate is tiny_eval.tiny_evaluate
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "kernels",
                            "tiny_ecg_eval.hip")).read()
    for name in ("ecg_tiny_eval(", "ecg_tiny_eval_scratch_bytes(", "ecg_tiny_eval_out_bytes("):
        assert "ECG_API int " + name in src or "ECG_API int " + name.replace("(", " (") in src, name


def test_cli_flags():
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    ns = entry.build_parser().parse_args(["--eval-every", "2", "--eval-windows", "100", "--eval-csv", "e.csv"])
    cfg = from_args(FedAvgConfig, ns)
    assert (cfg.eval_every, cfg.eval_windows, cfg.eval_csv) == (2, 100, "e.csv")


def test_evaluate_torch_matches_direct_and_restores_mode():
    from crossscale_ecg.ops.tiny_eval import evaluate_torch
    torch.manual_seed(0)
    nc, n = 3, 1000
    model = TinyECG(nc)
    with torch.no_grad():
        model.head.weight.mul_(8)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, 64, generator=g) * (0.25 + 2.75 * torch.rand(n, 1, generator=g))
    y = torch.randint(0, nc, (n,), generator=g)
    with torch.no_grad():
        logits = model(x.unsqueeze(1))
    pred = logits.argmax(1)
    assert pred.unique().numel() >= 2
    for mode in (True, False):
        model.train(mode)
        res = evaluate_torch(model, x, y, chunk=256)  # 1000 = 3 * 256 + 232: the last chunk is ragged
        assert model.training is mode
        assert res.count == n and res.correct == int((pred == y).sum())
        assert torch.equal(res.confusion, torch.bincount(y * nc + pred, minlength=nc * nc).reshape(nc, nc))
        ref = F.cross_entropy(logits.double(), y, reduction="sum").item()
        assert abs(res.loss_sum - ref) <= 1e-9 * abs(ref)
        assert abs(res.loss - ref / n) <= 1e-9 and abs(res.accuracy - res.correct / n) < 1e-12
    one = evaluate_torch(model, x, y, chunk=4096)
    assert torch.equal(one.counts_t, res.counts_t)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


def test_driver_eval_rows(tmp_path, monkeypatch):
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.utils.csvio import EVAL_COLUMNS, ROUND_COLUMNS
    built = []
    real = drv.make_trainer

    def spy(cfg, cname, model, x, y, ctx, backend):
        built.append(x.shape[0])
        return real(cfg, cname, model, x, y, ctx, backend)

    monkeypatch.setattr(drv, "make_trainer", spy)
    cfg = _cfg(str(tmp_path))
    drv.run_fedavg(cfg, _ctx1())
    assert built == [448]
    with open(cfg.eval_csv) as f:
        assert f.readline().strip().split(",") == EVAL_COLUMNS
    rows = read_csv(cfg.eval_csv)
    assert [int(r["round_idx"]) for r in rows] == [0, 1]
    for r in rows:
        assert int(r["windows"]) == 64 and r["backend"] == "torch" and r["config"] == "G0"
        conf = _conf(r["confusion"])
        assert len(conf) == 2 and sum(map(sum, conf)) == 64
        assert abs(float(r["accuracy"]) - (conf[0][0] + conf[1][1]) / 64) < 1e-9
        assert float(r["loss"]) > 0 and float(r["eval_ms"]) > 0
    with open(cfg.results_csv) as f:
        assert f.readline().strip().split(",") == ROUND_COLUMNS
    # every 2nd round of 2: one row; eval_windows = 0 evaluates the training windows
    d2 = tmp_path / "every2"
    cfg2 = _cfg(str(d2), eval_every=2, eval_windows=0)
    drv.run_fedavg(cfg2, _ctx1())
    rows = read_csv(cfg2.eval_csv)
    assert [int(r["round_idx"]) for r in rows] == [1] and int(rows[0]["windows"]) == 512
    assert built == [448, 512]


def test_default_config_writes_no_eval_file(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.utils.csvio import ROUND_COLUMNS
    cfg = _cfg(str(tmp_path), eval_every=0, eval_windows=0)
    drv.run_fedavg(cfg, _ctx1())
    assert not os.path.exists(cfg.eval_csv)
    with open(cfg.results_csv) as f:
        assert f.readline().strip().split(",") == ROUND_COLUMNS
    assert len(read_csv(cfg.results_csv)) == 2


def test_eval_windows_too_large_raises(tmp_path):
    from crossscale_ecg.train import fedavg as drv
    with pytest.raises(RuntimeError, match="eval-windows"):
        drv.run_fedavg(_cfg(str(tmp_path), eval_windows=512 - 31), _ctx1())
    assert not os.path.exists(os.path.join(str(tmp_path), "eval.csv"))


# ------------------------------------------------------------------------------------------- gloo, world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, tmp, overlap, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    penv._CTX = None
    torch.set_num_threads(1)
    try:
        from crossscale_ecg.ops.tiny_eval import evaluate_torch
        from crossscale_ecg.train import fedavg as drv
        from crossscale_ecg.utils.ckpt import ckpt_path, load_checkpoint
        ctx = penv.init_distributed(backend="gloo", prefer_gpu=False)
        cfg = _cfg(tmp, overlap=overlap, ckpt_every=1, bcast_every_round=False)
        drv.run_fedavg(cfg, ctx)
        # this client's own record of the LAST round's checkpoint (the averaged model) on its own holdout
        x, y = drv.load_client_data(cfg, ctx)
        _, _, xe, ye = drv.split_holdout(cfg, x, y, rank)
        model = TinyECG(cfg.num_classes)
        model.load_state_dict(load_checkpoint(ckpt_path(cfg.ckpt_dir, cfg.rounds - 1, "G0"))["model"])
        own = evaluate_torch(model, xe, ye)
        q.put((rank, "ok", (own.confusion.tolist(), own.loss_sum, own.count)))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


@pytest.mark.parametrize("overlap", ["none", "delayed"])
def test_gloo_world2_sums_client_records(tmp_path, overlap):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path), overlap, q)) for r in range(world)]
    for p in ps:
        p.start()
    out = {}
    for _ in range(world):
        rank, status, res = q.get(timeout=240)
        assert status == "ok", res
        out[rank] = res
    for p in ps:
        p.join(timeout=60)
    rows = read_csv(os.path.join(str(tmp_path), "eval.csv"))
    assert [int(r["round_idx"]) for r in rows] == [0, 1] and all(int(r["world_size"]) == 2 for r in rows)
    last = rows[-1]
    assert int(last["windows"]) == 128 == out[0][2] + out[1][2]
    want = [[a + b for a, b in zip(r0, r1)] for r0, r1 in zip(out[0][0], out[1][0])]
    assert _conf(last["confusion"]) == want
    assert abs(float(last["loss"]) - (out[0][1] + out[1][1]) / 128) < 1e-6
