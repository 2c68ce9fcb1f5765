"""What the GPU tests of the cohort rounds share: the dataset, index tables, starting weights, client weights at
chosen delta norms, and ``Cohort``, the buffers of one native cohort round with its ``TinyCohortRound``.  A plain
module (pytest puts this directory on ``sys.path``), imported by test_tiny_cohort_gpu.py, test_tiny_cohort_client_dp_gpu.py,
test_tiny_cohort_server_opt_gpu.py, test_tiny_cohort_global_server_gpu.py and test_tiny_prox_gpu.py."""
import ctypes as C

import torch

from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

N = 64  # windows of the dataset
LR, MU, WD = 1e-2, 0.9, 1e-3
DELTA_CANARY = -777.25  # behind a ``server_delta`` buffer


def _lib():
    from crossscale_ecg.ops import _lib
    return _lib


def _data(L, nc, seed=0):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, L, generator=g).to(dev)
    y32 = torch.randint(0, nc, (N,), generator=g).to(torch.int32).to(dev)
    return dev, x, y32


def _table(S, rows, seed=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, N, (S, rows), generator=g).to(torch.int32).cuda()


def _global(nc, seed=1):
    torch.manual_seed(seed)
    return torch.cat([p.detach().reshape(-1) for p in TinyECG(num_classes=nc).parameters()]).cuda()


def _clients(nc, M, clip, seed=2):
    """(g [P], params [M, pstride]): client c ends on g + d_c with |d_c| = 4 C, C / 2, 0 for c % 3 = 0, 1, 2; the
    pstride - P padding floats are NaN (a kernel that read them into a result would return NaN)."""
    P, ps = num_params(nc), _lib().kernels().ecg_tiny_cohort_param_stride(nc)
    g = _global(nc)
    gen = torch.Generator().manual_seed(seed)
    d = torch.randn(M, P, generator=gen, dtype=torch.float64)
    target = torch.tensor([[4 * clip, clip / 2, 0.0][c % 3] for c in range(M)], dtype=torch.float64)
    d = d * (target / d.norm(dim=1))[:, None]
    params = torch.full((M, ps), float("nan"), dtype=torch.float32, device="cuda")
    params[:, :P] = (g.double().cpu()[None, :] + d).float().cuda()
    return g, params


class Cohort:
    """The buffers of one native cohort round and its ``TinyCohortRound``.  ``glob`` [P] the global weights (None:
    zeros); ``w`` / ``m`` [M, P] per-client weights and momenta for rounds with ``fanout`` = 0; ``pad`` fills the
    clients' buffers, their pstride - P padding floats included.  The optional field groups - what is None or False is
    not named when the struct is built:
      ``dp``       dict of cdp_clip, cdp_sigma, server_lr, cdp_seed, round: the client-DP fields with scale / norm
                   buffers of -1.0 and the round word;
      ``so``       dict of server_opt, server_beta1, server_beta2, server_tau: the server optimizer's fields with
                   m = 0 and (not sgdm) v = tau^2;
      ``split``    a ``server_delta`` buffer of P floats with 8 floats of DELTA_CANARY behind it;
      ``prox_mu``  the FedProx coefficient;
      ``fields``   any further struct fields by name; tensors among them are kept alive and are part of ``state()``."""

    def __init__(self, x, y32, nc, M, B, S, precision, table, glob=None, dp=None, so=None, split=False, *, fanout=1,
                 w=None, m=None, momentum=MU, pad=0.0, prox_mu=None, **fields):
        from crossscale_ecg.ops.fused_tiny import prec_id, slab_stride
        L_ = _lib()
        lib = L_.kernels()
        dev, L = x.device, x.shape[1]
        self.P, self.M, self.B, self.S = num_params(nc), M, B, S
        self.ps, self.ws = lib.ecg_tiny_cohort_param_stride(nc), lib.ecg_tiny_cohort_wprep_stride()
        self.wp_bytes = lib.ecg_tiny_wprep_bytes()
        f32 = dict(dtype=torch.float32, device=dev)
        self.cparams, self.cmom = torch.full((M, self.ps), pad, **f32), torch.full((M, self.ps), pad, **f32)
        if w is not None:
            self.cparams[:, : self.P] = w
            self.cmom[:, : self.P] = m
        self.glob = torch.zeros(self.P, **f32) if glob is None else glob.clone()
        self.slab = torch.zeros((M * B, slab_stride(nc)), **f32)
        self.loss = torch.zeros(M, **f32)
        self.table = table
        self.wprep = self.xg = self.yg = self.xbg = None
        if precision == "bf16":
            self.wprep = torch.zeros(M * self.ws, dtype=torch.uint8, device=dev)
            self.xg = torch.zeros(lib.ecg_tiny_gather_floats(L, M * B), **f32)
            self.yg = torch.zeros(2 * M * B, dtype=torch.int32, device=dev)
            self.xbg = torch.zeros(lib.ecg_tiny_gather_halfs(L, M * B), dtype=torch.bfloat16, device=dev)
        p = L_.ptr
        kw = dict(X=x.data_ptr(), ldx=x.stride(0), idx=table.data_ptr(), Y=y32.data_ptr(), params=self.cparams.data_ptr(),
                  mom=self.cmom.data_ptr(), slab=self.slab.data_ptr(), loss_acc=self.loss.data_ptr(), wprep=p(self.wprep),
                  xg=p(self.xg), yg=p(self.yg), xbg=p(self.xbg), global_params=self.glob.data_ptr(), L=L, nc=nc,
                  slab_stride=self.slab.shape[1], B=B, steps=S, M=M, fanout=fanout, lr=LR, momentum=momentum, wd=WD,
                  nesterov=0, prec=prec_id(precision))
        self.scale = self.norm = self.word = self.m = self.v = self.delta = None
        if dp is not None:
            self.scale, self.norm = torch.full((M,), -1.0, **f32), torch.full((M,), -1.0, **f32)
            self.word = torch.tensor([dp["round"]], dtype=torch.int64, device=dev)
            kw.update(cdp_clip=dp["cdp_clip"], cdp_sigma=dp["cdp_sigma"], server_lr=dp["server_lr"],
                      cdp_seed=dp["cdp_seed"], cdp_scale=self.scale.data_ptr(), cdp_norm=self.norm.data_ptr(),
                      cdp_round=self.word.data_ptr())
        if so is not None:
            self.m = torch.zeros(self.P, **f32)
            if so["server_opt"] != 1:
                self.v = torch.full((self.P,), so["server_tau"], **f32) ** 2
            kw.update(so, server_m=self.m.data_ptr(), server_v=p(self.v))
        if split:
            self.delta = torch.full((self.P + 8,), DELTA_CANARY, **f32)
            kw.update(server_delta=self.delta.data_ptr())
        if prox_mu is not None:
            kw["prox_mu"] = prox_mu
        self.keep = []
        for k, v in fields.items():
            if isinstance(v, torch.Tensor):
                self.keep.append(v)
                v = v.data_ptr()
            kw[k] = v
        self.round = L_.TinyCohortRound(**kw)

    def enqueue(self):
        L_ = _lib()
        return L_.kernels().ecg_tiny_cohort_round_enqueue(C.byref(self.round), L_.stream_ptr(self.glob.device))

    def run(self):
        _lib().check(self.enqueue(), "ecg_tiny_cohort_round_enqueue")
        torch.cuda.synchronize()
        return self

    def image(self, c):
        return self.wprep[c * self.ws: c * self.ws + self.wp_bytes]

    def state(self):
        """Clones of everything a round writes, ``server_delta`` apart."""
        out = [self.glob, self.cparams, self.cmom, self.loss] + self.keep
        out += [t for t in (self.wprep, self.scale, self.norm, self.word, self.m, self.v) if t is not None]
        return [t.clone() for t in out]
