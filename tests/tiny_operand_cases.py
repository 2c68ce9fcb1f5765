"""What tests/test_tiny_ref_cpu.py and tests/test_tiny_operand_exact_gpu.py share: the cases of the GPU file (weights,
windows and labels as CPU tensors, seeded), their float64 operand-exact references (models/tiny_ecg_ref.py), the
reference's own noise floor on exactly those cases, and the bounds set from it.  A plain module (pytest puts this
directory on ``sys.path``); it touches no GPU.

Bounds.  ``REF_BOUND = 10 x`` the noise floor: the worst, over every bf16 case below, of the reference evaluated in
float32 against the reference in float64 (per sample row and per tensor ``|a - b|_2 / |b|_2``, the loss column, and
``max |a - b| / max |b|`` for logits) - PyTorch on the CPU and the reference only, no kernel.  The factor 10 is for the
kernel's own summation orders (MFMA blocks of 32 steps, per-wave partials), each of which can put an isolated h1 or
dh1 element on the other side of a bf16 rounding boundary.  ``REF_BOUND`` must stay <= 1e-3, a third of the smallest
seam defect measured at L = 500 (one conv2 dgrad tap dropped at the last step: 2.9e-3), so a case's seed is acceptable
only if its own floor is <= ``SEED_FLOOR_MAX`` = 1e-4; ``inputs`` of every kind walks the seeds in order and takes the
first acceptable one (a seed at which a float32-vs-float64 flip of a ReLU sign or of a rounding moves a short row by
more is replaced by the next).  ``REF_BOUND_F32`` is set the same way for the fp32 kernels: float32 autograd of
``TinyECG`` against float64 autograd, per sample, over the fp32 cases.  tests/test_tiny_ref_cpu.py measures both floors
and asserts ``10 x floor <= bound``; the bounds below are those products rounded up to two digits.
"""
import functools
import importlib.util
import os

import torch
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from crossscale_ecg.models.tiny_ecg_ref import logit_error, row_errors, tiny_ecg_reference

B = 4
SEED_FLOOR_MAX = 1e-4
REF_FLOOR = 5.67e-7       # measured: tests/test_tiny_ref_cpu.py::test_noise_floor_sets_the_bound
REF_BOUND = 5.7e-6
REF_FLOOR_F32 = 2.23e-7   # measured: tests/test_tiny_ref_cpu.py::test_fp32_noise_floor_sets_the_bound
REF_BOUND_F32 = 2.3e-6

GRAD_L = (8, 29, 32, 33, 63, 100, 300, 500)
GRAD_CASES = [(L, nc, "randn") for L in GRAD_L for nc in (2, 5)] + [(100, 2, "zeros")]
TRAINER_CASES = [(L, nc) for L in (8, 33, 100, 500) for nc in (2, 5)]  # inputs: the "randn" gradient case of (L, nc)
COHORT_CASE = dict(L=99, nc=5, M=3, N=64)
LOGIT_CASES = [(L, nc) for L in (64, 96, 333, 500) for nc in (2, 5, 16)]
LOGIT_N = (1, 63, 257)
F32_CASES = [(L, nc) for L in (8, 33, 130, 333) for nc in (2, 5)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("record_tiny_step_r19",
                                                  os.path.join(ROOT, "scripts", "record_tiny_step_r19.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


def flat_of(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).float()


def worst(errs):
    """(tensor name, error) of the largest entry of a ``row_errors`` dict."""
    return max(errs.items(), key=lambda kv: kv[1])


def ref_floor(flat, x, y, nc, scale):
    """The reference in float32 against the reference in float64 on one set of inputs: the worst row / loss / logit
    error, and the float64 result."""
    r64 = tiny_ecg_reference(flat, x, y, scale, nc)
    r32 = tiny_ecg_reference(flat, x, y, scale, nc, dtype=torch.float32)
    e = max(worst(row_errors(r32.rows, r64.rows, nc))[1], logit_error(r32.logits, r64.logits))
    return e, r64


def _first_seed(draw, nc, scale, what):
    for seed in range(64):
        flat, x, y = draw(seed)
        floor, r64 = ref_floor(flat, x, y, nc, scale)
        if floor <= SEED_FLOOR_MAX:
            return dict(flat=flat, x=x, y=y, ref=r64, floor=floor, seed=seed)
        print(f"{what}: seed {seed} replaced: reference float32 vs float64 {floor:.3g}")
    raise AssertionError(f"{what}: no seed below 64 with a reference floor <= {SEED_FLOOR_MAX}")


def zeros_weights(nc):
    """The weights of the recorder's "zeros" case: zero conv1 bias, conv2 bias zero on every other channel."""
    torch.manual_seed(19)
    model = TinyECG(num_classes=nc)
    with torch.no_grad():
        model.net[0].bias.zero_()
        model.net[2].bias[::2] = 0.0
    return model


@functools.lru_cache(maxsize=None)
def grad_case(L, nc, kind="randn"):
    """dict(flat [P], x [B, L], y [B], ref (float64, loss scale 1 / B), floor, seed) of a gradient case."""
    if kind == "zeros":  # fixed inputs: scripts/record_tiny_step_r19.py::case_inputs, rows 0 .. B - 1
        x, y, _ = _recorder().case_inputs(L, nc, "zeros")
        flat, x, y = flat_of(zeros_weights(nc)), x[:B].clone(), y[:B].clone()
        floor, r64 = ref_floor(flat, x, y, nc, 1.0 / B)
        return dict(flat=flat, x=x, y=y, ref=r64, floor=floor, seed=None)

    def draw(seed):
        g = torch.Generator(device="cpu").manual_seed(1000 * seed + L)
        torch.manual_seed(seed)
        flat = flat_of(TinyECG(num_classes=nc))
        return flat, torch.randn(B, L, generator=g), torch.randint(0, nc, (B,), generator=g)

    return _first_seed(draw, nc, 1.0 / B, f"gradient case L={L} nc={nc}")


@functools.lru_cache(maxsize=None)
def cohort_case():
    """dict(x [N, L], y [N], table [1, M * B], w [M, P], refs [M] (float64, client c at its own weights), floor)."""
    L, nc, M, N = (COHORT_CASE[k] for k in ("L", "nc", "M", "N"))

    def draw(seed):
        g = torch.Generator(device="cpu").manual_seed(7000 + seed)
        torch.manual_seed(seed)
        flat = flat_of(TinyECG(num_classes=nc))
        x, y = torch.randn(N, L, generator=g), torch.randint(0, nc, (N,), generator=g)
        table = torch.randperm(N, generator=g)[:M * B].reshape(1, M * B).to(torch.int32)
        w = flat[None, :] + 0.05 * torch.randn(M, flat.numel(), generator=g)
        return x, y, table, w

    for seed in range(64):
        x, y, table, w = draw(seed)
        floors, refs = [], []
        for c in range(M):
            rows = table[0, c * B:(c + 1) * B].long()
            f, r = ref_floor(w[c], x[rows], y[rows], nc, 1.0 / B)
            floors.append(f)
            refs.append(r)
        if max(floors) <= SEED_FLOOR_MAX:
            return dict(x=x, y=y, table=table, w=w, refs=refs, floor=max(floors), seed=seed)
        print(f"cohort case: seed {seed} replaced: reference float32 vs float64 {max(floors):.3g}")
    raise AssertionError("cohort case: no acceptable seed below 64")


@functools.lru_cache(maxsize=None)
def logit_case(L, nc):
    """dict(flat, x [257, L], y [257], ref (float64), floor): windows with an amplitude and an offset per window and
    a head scaled by 8 (the inputs of tests/test_tiny_eval_gpu.py: distinct logits per window)."""
    n = max(LOGIT_N)

    def draw(seed):
        g = torch.Generator(device="cpu").manual_seed(3000 * seed + 10 * L + nc)
        amp = 0.25 + 2.75 * torch.rand(n, generator=g)
        off = 2 * torch.rand(n, generator=g) - 1
        x = torch.randn(n, L, generator=g) * amp[:, None] + off[:, None]
        y = torch.randint(0, nc, (n,), generator=g)
        torch.manual_seed(seed)
        model = TinyECG(nc)
        with torch.no_grad():
            model.head.weight.mul_(8)
        return flat_of(model), x, y

    for seed in range(64):
        flat, x, y = draw(seed)
        r64 = tiny_ecg_reference(flat, x, y, 1.0, nc)
        r32 = tiny_ecg_reference(flat, x, y, 1.0, nc, dtype=torch.float32)
        floor = max(max(logit_error(r32.logits[:k], r64.logits[:k]) for k in LOGIT_N),
                    max(abs(r32.loss[:k].double().sum().item() - r64.loss[:k].sum().item()) / r64.loss[:k].sum().item()
                        for k in LOGIT_N))
        if floor <= SEED_FLOOR_MAX:
            return dict(flat=flat, x=x, y=y, ref=r64, floor=floor, seed=seed)
        print(f"logit case L={L} nc={nc}: seed {seed} replaced: reference float32 vs float64 {floor:.3g}")
    raise AssertionError(f"logit case L={L} nc={nc}: no acceptable seed below 64")


def autograd_rows(model, x, y, scale, dtype):
    """Per-sample rows [B, P + 1] (gradient times ``scale``, loss in column P) and logits of ``TinyECG`` by autograd."""
    nc = model.num_classes
    twin = TinyECG(num_classes=nc)
    twin.load_state_dict(model.state_dict())
    twin = twin.to(dtype)
    rows, logits = [], []
    for s in range(x.shape[0]):
        twin.zero_grad(set_to_none=True)
        out = twin(x[s:s + 1, None].to(dtype))
        loss = F.cross_entropy(out, y[s:s + 1].long())
        loss.backward()
        rows.append(torch.cat([p.grad.reshape(-1) * scale for p in twin.parameters()] + [loss.detach().reshape(1)]))
        logits.append(out.detach()[0])
    return torch.stack(rows), torch.stack(logits)


@functools.lru_cache(maxsize=None)
def f32_case(L, nc):
    """dict(flat, x [B, L], y [B], ref (float64, rounding=None), floor): the floor is float32 autograd against float64
    autograd of the same inputs."""
    for seed in range(64):
        g = torch.Generator(device="cpu").manual_seed(5000 * seed + L)
        torch.manual_seed(seed)
        model = TinyECG(num_classes=nc)
        x, y = torch.randn(B, L, generator=g), torch.randint(0, nc, (B,), generator=g)
        r32, l32 = autograd_rows(model, x, y, 1.0 / B, torch.float32)
        r64, l64 = autograd_rows(model, x, y, 1.0 / B, torch.float64)
        floor = max(worst(row_errors(r32, r64, nc))[1], logit_error(l32, l64))
        if floor <= SEED_FLOOR_MAX:
            flat = flat_of(model)
            ref = tiny_ecg_reference(flat, x, y, 1.0 / B, nc, rounding=None)
            return dict(flat=flat, x=x, y=y, ref=ref, floor=floor, seed=seed, autograd64=(r64, l64))
        print(f"fp32 case L={L} nc={nc}: seed {seed} replaced: float32 vs float64 autograd {floor:.3g}")
    raise AssertionError(f"fp32 case L={L} nc={nc}: no acceptable seed below 64")


def bf16_floor():
    """The worst reference floor over every bf16 case of the GPU file, and the case it comes from."""
    floors = {("grad",) + c: grad_case(*c)["floor"] for c in GRAD_CASES}
    floors[("cohort",)] = cohort_case()["floor"]
    floors.update({("logits",) + c: logit_case(*c)["floor"] for c in LOGIT_CASES})
    return floors


def f32_floor():
    return {c: f32_case(*c)["floor"] for c in F32_CASES}
