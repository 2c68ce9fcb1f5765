"""Datasets, host DataLoader and GPU-resident batch sources.

Reference parity (Module_3/shard_dataset.py):
  * ``ShardDataset``        <- :50-77  (concatenate shards, truncate to max_windows, dummy zero labels)
  * ``make_dataloader``     <- :82-98
  * ``load_shards_to_gpu``  <- :103-115
  * ``make_gpu_batch_iter`` <- :118-136  (per-epoch device randperm, drop-last, infinite)

MI355X-first additions:
  * ``load_shards_to_gpu`` streams shards through page-locked staging buffers with async H2D on a
    dedicated copy stream (double-buffered, event-fenced) instead of one pageable ``.to()``; with the
    native IO library present it uses ``hipHostMalloc`` + ``hipMemcpyAsync`` from C++ (csrc/io).
  * ``DeviceIndexSampler`` produces the same epoch/drop-last batch order as ``make_gpu_batch_iter`` but as
    a static int32 index table ``[steps, B]`` on the device, which the fused HIP train step gathers from
    directly (no per-step gather kernel, graph-capturable).
  * ``CohortSampler`` partitions the windows among virtual clients and draws, per FedAvg round, a cohort of clients
    and their batches as one ``[steps, cohort * B]`` table - a pure function of ``(seed, round)``.
  * ``labels="parity"`` gives a learnable synthetic label (sign of the window mean) for convergence tests.
"""
from __future__ import annotations

import warnings
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from .shards import load_shard, shard_header


def make_labels(x: np.ndarray, mode: str = "zeros") -> np.ndarray:
    if mode == "zeros":
        return np.zeros(x.shape[0], dtype=np.int64)
    if mode == "parity":
        return (x.mean(axis=1) > 0).astype(np.int64)
    raise ValueError(f"unknown label mode {mode!r}")


class ShardDataset(Dataset):
    """Concatenates shards into one in-memory [N, L] dataset with dummy labels."""

    def __init__(self, shard_paths: Sequence[str], max_windows: Optional[int] = None, labels: str = "zeros"):
        xs = [load_shard(p) for p in shard_paths]
        if not xs:
            raise RuntimeError("No shards assigned to this rank.")
        arr = np.concatenate(xs, axis=0).astype(np.float32, copy=False)
        if max_windows is not None:
            arr = arr[:max_windows]
        arr = np.ascontiguousarray(arr)
        self.x = torch.from_numpy(arr)
        self.y = torch.from_numpy(make_labels(arr, labels))

    def __len__(self) -> int:
        return self.x.shape[0]

    def __getitem__(self, idx):
        return self.x[idx].unsqueeze(0), self.y[idx]


def make_dataloader(shard_paths: Sequence[str], batch_size: int, max_windows: Optional[int] = None,
                    num_workers: int = 2, pin_memory: bool = True, shuffle: bool = True,
                    labels: str = "zeros") -> Tuple[DataLoader, int]:
    ds = ShardDataset(shard_paths, max_windows=max_windows, labels=labels)
    dl = DataLoader(ds, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                    pin_memory=pin_memory and torch.cuda.is_available(), drop_last=True,
                    persistent_workers=num_workers > 0)
    return dl, len(ds)


def _count_windows(shard_paths: Sequence[str], max_windows: Optional[int]) -> Tuple[int, int]:
    total, L = 0, None
    for p in shard_paths:
        n, l = shard_header(p)
        if L is None:
            L = l
        elif l != L:
            raise RuntimeError(f"shard {p} has L={l}, expected {L}")
        total += n
    if L is None:
        raise RuntimeError("No shards assigned to this rank.")
    if max_windows is not None:
        total = min(total, max_windows)
    return total, L


def load_shards_to_gpu(shard_paths: Sequence[str], device, max_windows: Optional[int] = None,
                       labels: str = "zeros", chunk_windows: int = 16384,
                       use_native: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Upload this rank's shards once: returns (x [N, L] float32, y [N] int64) on ``device``.

    On a GPU the upload is chunked through pinned staging buffers on a side copy stream; the
    returned tensors are valid on the current stream (it waits on the copy stream).
    """
    device = torch.device(device)
    n_total, L = _count_windows(shard_paths, max_windows)
    if device.type != "cuda":
        ds = ShardDataset(shard_paths, max_windows=max_windows, labels=labels)
        return ds.x.to(device), ds.y.to(device)

    if use_native is None or use_native:
        from ..ops import native_io
        if native_io.available():
            try:
                x = native_io.upload_shards(shard_paths, device, n_total, L)
                y = _labels_on_device(x, labels)
                return x, y
            except Exception as e:  # the native uploader exists but failed: say so, then take the torch path
                if use_native:
                    raise
                warnings.warn(f"load_shards_to_gpu: native upload failed ({e!r}); using the torch pinned path",
                              RuntimeWarning, stacklevel=2)
        elif use_native:
            raise RuntimeError("load_shards_to_gpu(use_native=True): libecg_io.so is not available")
        else:
            warnings.warn("load_shards_to_gpu: libecg_io.so not available; using the torch pinned path",
                          RuntimeWarning, stacklevel=2)

    x = torch.empty((n_total, L), dtype=torch.float32, device=device)
    copy_stream = torch.cuda.Stream(device=device)
    staging = [torch.empty((chunk_windows, L), dtype=torch.float32).pin_memory() for _ in range(2)]
    done = [None, None]
    row = 0
    slot = 0
    for p in shard_paths:
        if row >= n_total:
            break
        mm = load_shard(p, mmap=True)
        i = 0
        while i < mm.shape[0] and row < n_total:
            take = min(chunk_windows, mm.shape[0] - i, n_total - row)
            if done[slot] is not None:
                done[slot].synchronize()  # staging slot free again
            staging[slot][:take].numpy()[:] = mm[i:i + take]
            with torch.cuda.stream(copy_stream):
                x[row:row + take].copy_(staging[slot][:take], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            done[slot] = ev
            slot ^= 1
            row += take
            i += take
    torch.cuda.current_stream(device).wait_stream(copy_stream)
    x.record_stream(torch.cuda.current_stream(device))
    for ev in done:
        if ev is not None:
            ev.synchronize()
    y = _labels_on_device(x, labels)
    return x, y


def _labels_on_device(x: torch.Tensor, labels: str) -> torch.Tensor:
    if labels == "zeros":
        return torch.zeros(x.shape[0], dtype=torch.long, device=x.device)
    if labels == "parity":
        return (x.mean(dim=1) > 0).long()
    raise ValueError(f"unknown label mode {labels!r}")


def make_gpu_batch_iter(x_gpu: torch.Tensor, y_gpu: torch.Tensor, batch_size: int,
                        generator: Optional[torch.Generator] = None) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
    """Infinite iterator of random mini-batches gathered on the device: ``([B,1,L], [B])``."""
    N = x_gpu.size(0)
    if N < batch_size:
        raise RuntimeError(f"Not enough windows ({N}) for a batch of {batch_size}")
    device = x_gpu.device
    while True:
        perm = torch.randperm(N, device=device, generator=generator)
        for start in range(0, N - batch_size + 1, batch_size):
            sel = perm[start:start + batch_size]
            yield x_gpu[sel].unsqueeze(1), y_gpu[sel]


class DeviceIndexSampler:
    """Epoch-permutation batch indices as a static device table for the fused step.

    Same semantics as ``make_gpu_batch_iter``: a fresh ``randperm(N)`` per epoch, consecutive
    ``batch_size`` slices, trailing partial batch dropped.  ``fill(table)`` writes the next
    ``table.shape[0]`` batches into ``table`` (int32 [S, B]) in place, so a captured graph that
    reads ``table`` sees new batches every replay.

    Permutations are generated ``epochs_per_block`` epochs at a time as one batched ``argsort`` of
    independent 62-bit random keys (a uniform random permutation per row): one sort of [E, N] costs about
    as many launches as one ``randperm(N)``, so for small shards (N=20,000: ~8 sort/scan kernels per
    epoch, ~40 us per 50-step round, ~6 % of a 0.64 ms fused round) the per-round cost drops to the one
    or two table copies.
    """

    def __init__(self, n_windows: int, batch_size: int, device, seed: Optional[int] = None,
                 epochs_per_block: Optional[int] = None):
        if n_windows < batch_size:
            raise RuntimeError(f"Not enough windows ({n_windows}) for a batch of {batch_size}")
        self.N = n_windows
        self.B = batch_size
        self.device = torch.device(device)
        self.steps_per_epoch = n_windows // batch_size
        self.gen = None
        if seed is not None:
            self.gen = torch.Generator(device=self.device)
            self.gen.manual_seed(seed)
        if epochs_per_block is None:  # ~2M keys per block: small shards batch many epochs, big ones one
            epochs_per_block = max(1, min(32, (1 << 21) // max(1, n_windows)))
        self.E = int(epochs_per_block)
        self._perm: Optional[torch.Tensor] = None
        self._rows = 0
        self._cursor = 0  # force a new block on first use

    def _new_epoch(self):
        spe, B = self.steps_per_epoch, self.B
        if self.E == 1:
            p = torch.randperm(self.N, device=self.device, generator=self.gen).view(1, self.N)
        else:
            keys = torch.randint(0, 1 << 62, (self.E, self.N), device=self.device, generator=self.gen,
                                 dtype=torch.int64)
            p = keys.argsort(dim=1)
        # [E, spe*B] -> rows of consecutive epochs, each epoch's batches in order (drop-last per epoch)
        self._perm = p[:, : spe * B].to(torch.int32).reshape(self.E * spe, B)
        self._rows = self.E * spe
        self._cursor = 0

    def prime(self) -> None:
        """Draw the first block of epoch permutations now (the same block ``fill`` would draw on first use, so the
        batch sequence is unchanged): keeps the one-time sort-kernel load out of a timed first round."""
        if self._cursor >= self._rows:
            self._new_epoch()

    def fill(self, table: torch.Tensor) -> torch.Tensor:
        S = table.shape[0]
        if table.dtype != torch.int32 or table.shape[1] != self.B:
            raise ValueError(f"index table must be int32 [S, {self.B}], got {table.dtype} {tuple(table.shape)}")
        s = 0
        while s < S:
            if self._cursor >= self._rows:
                self._new_epoch()
            take = min(S - s, self._rows - self._cursor)
            table[s:s + take].copy_(self._perm[self._cursor:self._cursor + take], non_blocking=True)
            s += take
            self._cursor += take
        return table

    def state_dict(self) -> dict:
        """Everything needed to continue the exact batch order (generator state, current block, cursor)."""
        return {"gen": None if self.gen is None else self.gen.get_state(),
                "perm": None if self._perm is None else self._perm.detach().cpu(),
                "rows": self._rows, "cursor": self._cursor, "N": self.N, "B": self.B, "E": self.E}

    def load_state_dict(self, st: dict) -> None:
        if (int(st["N"]), int(st["B"])) != (self.N, self.B):
            raise ValueError(f"sampler state is for N={st['N']}, B={st['B']}; this sampler has N={self.N}, B={self.B}")
        if st.get("gen") is not None:
            if self.gen is None:
                self.gen = torch.Generator(device=self.device)
            self.gen.set_state(st["gen"])
        self.E = int(st["E"])
        self._perm = None if st.get("perm") is None else st["perm"].to(self.device)
        self._rows, self._cursor = int(st["rows"]), int(st["cursor"])

    def next_batch(self) -> torch.Tensor:
        t = torch.empty((1, self.B), dtype=torch.int32, device=self.device)
        return self.fill(t)[0]


PARTITIONS = ("contiguous", "shards", "dirichlet")


def shard_partition(y: torch.Tensor, clients: int, shards_per_client: int, seed: Optional[int]) -> torch.Tensor:
    """Label-skewed clients, the sort-and-deal partition of McMahan et al. ("Communication-Efficient Learning of Deep
    Networks from Decentralized Data"): int64 ``[K, n]`` on ``y``'s device, row k the dataset rows of client k.

    The stable argsort of the labels ``y`` [N] is cut into ``K * s`` shards of ``n / s`` consecutive entries, with
    ``n = s * (N // (K * s))`` (a remainder at the end of the sorted order is unused), and the shards are dealt by a host
    permutation seeded from ``mix64(seed)``: client k owns shards ``perm[k * s : (k + 1) * s]``, so its rows come from at
    most s runs of the sorted order - with two classes and s = 2 most clients see one or two labels.  A pure function
    of its arguments: a resumed run rebuilds the partition it had."""
    from ..utils.philox import mix64
    K, s = int(clients), int(shards_per_client)
    if K < 1 or s < 1:
        raise ValueError(f"need clients >= 1 and shards_per_client >= 1, got {K} and {s}")
    if y.dim() != 1:
        raise ValueError("labels must be a vector [N]")
    rows = y.shape[0] // (K * s)  # rows of one shard
    if rows < 1:
        raise RuntimeError(f"{y.shape[0]} windows are fewer than {K} clients x {s} shards")
    order = torch.argsort(y, stable=True)[: K * s * rows].view(K * s, rows)
    g = torch.Generator()
    g.manual_seed(mix64(0 if seed is None else int(seed)) & ((1 << 63) - 1))
    perm = torch.randperm(K * s, generator=g).to(order.device)
    return order[perm].reshape(K, s * rows).to(torch.int64).contiguous()


def dirichlet_partition(y: torch.Tensor, clients: int, alpha: float, min_rows: int,
                        seed: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """Clients of unequal sizes and label mixes, the label-Dirichlet split of Hsu et al. ("Measuring the Effects of
    Non-Identical Data Distribution for Federated Visual Classification"): ``(order, sizes)`` on ``y``'s device, int64
    ``[K, n_max]`` and ``[K]``; row k of ``order`` holds client k's dataset rows in its first ``sizes[k]`` entries (the
    rest repeats its first row: valid rows that no sampler reads).

    For every class in ascending order, the class's rows - in a host permutation - are dealt to the K clients in
    proportions ``q ~ Dir(alpha)``: client k takes entries ``[floor(c_{k-1} n), floor(c_k n))`` of the n permuted rows,
    c the running sum of q (c_K = 1).  Small alpha: most of a class goes to few clients.  Then, in ascending client
    order, a client below ``min_rows`` (a batch) is topped up from the tail of the currently largest client (the
    lowest id among equals), which never drops below ``min_rows`` itself.  Every row belongs to at most one client.
    Permutations and proportions come from one host generator seeded from ``mix64(seed)``: a pure function of its
    arguments, so a resumed run rebuilds the partition it had."""
    from ..utils.philox import mix64
    K, m = int(clients), int(min_rows)
    if K < 1 or m < 1 or not alpha > 0:
        raise ValueError(f"need clients >= 1, min_rows >= 1 and alpha > 0, got {K}, {m} and {alpha}")
    if y.dim() != 1:
        raise ValueError("labels must be a vector [N]")
    if y.shape[0] < K * m:
        raise RuntimeError(f"{y.shape[0]} windows are fewer than {K} clients x {m} rows")
    g = torch.Generator()
    g.manual_seed(mix64(0 if seed is None else int(seed)) & ((1 << 63) - 1))
    yc = y.detach().cpu()
    parts: List[List[torch.Tensor]] = [[] for _ in range(K)]
    for c in torch.unique(yc).tolist():  # (sorted)
        rows = torch.nonzero(yc == c).reshape(-1)
        rows = rows[torch.randperm(rows.numel(), generator=g)]
        q = torch._standard_gamma(torch.full((K,), float(alpha), dtype=torch.float64), generator=g)
        if not float(q.sum()) > 0.0:  # every draw underflowed (alpha << 1): the whole class to one client
            q = torch.zeros(K, dtype=torch.float64)
            q[int(torch.randint(K, (1,), generator=g))] = 1.0
        cuts = torch.floor(torch.cumsum(q / q.sum(), 0) * rows.numel()).to(torch.int64).clamp_(0, rows.numel())
        cuts[-1] = rows.numel()
        lo = 0
        for k in range(K):
            hi = max(lo, int(cuts[k]))
            parts[k].append(rows[lo:hi])
            lo = hi
    own = [torch.cat(p) if p else torch.zeros(0, dtype=torch.int64) for p in parts]
    for k in range(K):
        while own[k].numel() < m:
            d = max(range(K), key=lambda j: (own[j].numel(), -j))
            t = min(m - own[k].numel(), own[d].numel() - m)
            if d == k or t < 1:
                raise RuntimeError(f"cannot give every one of {K} clients {m} rows")  # (unreachable: N >= K * m)
            own[k] = torch.cat([own[k], own[d][-t:]])
            own[d] = own[d][:-t]
    sizes = torch.tensor([o.numel() for o in own], dtype=torch.int64)
    order = torch.stack([torch.cat([o, o[:1].expand(int(sizes.max()) - o.numel())]) for o in own])
    return order.contiguous().to(y.device), sizes.to(y.device)


def client_partition(partition: str, y: torch.Tensor, clients: int, shards_per_client: int, seed: Optional[int],
                     device, alpha: float = 0.0, min_rows: int = 1):
    """The ``order`` argument of ``CohortSampler`` for a trainer's ``partition``: None for "contiguous" (client k owns
    rows ``[k * n, (k + 1) * n)``), ``shard_partition`` of the labels on ``device`` for "shards".  "dirichlet":
    ``dirichlet_partition(y, clients, alpha, min_rows, seed)`` on ``device`` - the pair ``(order, sizes)``, ``CohortSampler``'s
    ``order`` and ``sizes``."""
    if partition not in PARTITIONS or (partition == "dirichlet" and not alpha > 0):
        raise ValueError(f"partition must be one of {list(PARTITIONS)}, dirichlet together with its concentration "
                         f"alpha > 0 (there is no default); got {partition!r} with alpha {alpha:g}")
    if partition == "contiguous":
        return None
    if partition == "dirichlet":
        order, sizes = dirichlet_partition(y, clients, alpha, min_rows, seed)
        return order.to(device), sizes.to(device)
    return shard_partition(y, clients, shards_per_client, seed).to(device)


def flip_client_labels(y: torch.Tensor, order: torch.Tensor, sizes: Optional[torch.Tensor], clients: int,
                       nc: int) -> torch.Tensor:
    """Poisoned clients by label flipping: a copy of the labels ``y`` [N] in which the training rows owned by clients
    ``0 .. clients - 1`` - the first ``sizes[k]`` entries of row k of ``order`` (int64 ``[K, n]``; ``sizes`` None: all n)
    - hold ``nc - 1 - y``.  Rows of other clients and rows no client owns (a partition's remainder, an evaluation
    hold-out kept elsewhere) are as in ``y``.  A pure function: ``y`` is not modified, and applying it twice restores
    the labels."""
    F = int(clients)
    if order.dim() != 2 or not 0 <= F <= order.shape[0]:
        raise ValueError(f"need order [K, n] and 0 <= clients <= K, got {tuple(order.shape)} and {F}")
    out = y.clone()
    for k in range(F):
        rows = order[k] if sizes is None else order[k, : int(sizes[k])]
        rows = rows.to(y.device)
        out[rows] = (int(nc) - 1) - y[rows]
    return out


def flipped_labels(y: torch.Tensor, order: Optional[torch.Tensor], sizes: Optional[torch.Tensor], clients: int,
                   flip_clients: int, nc: int) -> torch.Tensor:
    """The labels a cohort trainer of ``clients`` K virtual clients trains on: ``y`` itself for ``flip_clients`` F == 0,
    else ``flip_client_labels`` for clients 0..F-1 of the partition ``order`` / ``sizes`` as ``CohortSampler`` takes them
    (``order`` None: the contiguous partitions of ``N // K`` rows)."""
    K, F = int(clients), int(flip_clients)
    if not 0 <= F <= K:
        raise ValueError(f"flip_clients must be in [0, clients = {K}], got {F}")
    if F == 0:
        return y
    if order is None:
        n = y.shape[0] // K
        order = torch.arange(K * n, dtype=torch.int64, device=y.device).view(K, n)
    return flip_client_labels(y, order, sizes, F, nc)


class CohortSampler:
    """Client sampling for cohorts of virtual clients: which clients train in round ``r``, and on which rows.

    The ``n_windows`` training windows are split into ``clients`` contiguous partitions of ``n = n_windows // clients``
    rows (client k owns rows ``[k * n, (k + 1) * n)``; a remainder at the end is unused).  Round ``r`` draws ``cohort``
    distinct clients with a host generator seeded from ``mix64(seed) ^ r`` and, for each of them, ``steps * B`` rows of
    its partition: consecutive slices of fresh random permutations of the partition (no row twice within one pass
    over the partition; a new permutation starts where one runs out, also in the middle of a batch), produced on the
    device by one batched ``argsort`` of random keys like ``DeviceIndexSampler``'s, from a device generator seeded from
    the same pair.  ``fill`` writes them as the table ``[steps][cohort * B]``, client j of the cohort in columns
    ``[j * B, (j + 1) * B)``.

    ``order`` (int64 ``[clients, n]``, e.g. ``shard_partition``): client k's local row j is dataset row ``order[k, j]``
    instead of ``k * n + j``, and ``n`` is its row length; None: the contiguous partitions, the tables of before.

    ``sizes`` (int64 ``[clients]``, with ``order``; e.g. ``dirichlet_partition``): clients of unequal sizes - client k
    owns the first ``n_k = sizes[k]`` entries of its ``order`` row.  Its local row for position t of a round (t in
    ``[0, steps * B)``, step ``t // B``) is entry ``t % n_k`` of its permutation number ``t // n_k``: consecutive slices of
    fresh permutations of ITS partition, as above, with ``passes = ceil(steps * B / min(sizes))`` permutations drawn
    per client.  Every table entry is a row of its client's own partition, the steps that ``steps_of`` cuts off
    included (the round still reads them).  None: equal sizes, the tables of before, bit for bit.

    The sampler holds no state between rounds: a run resumed at round r draws what the uninterrupted run drew.
    """

    def __init__(self, n_windows: int, batch_size: int, steps: int, clients: int, cohort: int, device,
                 seed: Optional[int] = None, order: Optional[torch.Tensor] = None,
                 sizes: Optional[torch.Tensor] = None):
        if clients < 1 or not 1 <= cohort <= clients:
            raise ValueError(f"need 1 <= cohort <= clients, got cohort {cohort} of {clients} clients")
        self.N, self.B, self.S, self.K, self.M = int(n_windows), int(batch_size), int(steps), int(clients), int(cohort)
        self.n = self.N // self.K
        self.device = torch.device(device)
        self.order = None
        if order is not None:
            if order.dim() != 2 or order.shape[0] != self.K or order.dtype != torch.int64:
                raise ValueError(f"order must be int64 [{self.K}, n], got {order.dtype} {tuple(order.shape)}")
            if order.numel() and (int(order.min()) < 0 or int(order.max()) >= self.N):
                raise ValueError(f"order holds rows outside [0, {self.N})")
            self.order = order.to(self.device)
            self.n = int(order.shape[1])
        self.sizes: Optional[List[int]] = None
        if sizes is not None:
            if self.order is None:
                raise ValueError("sizes need order: the rows of clients of unequal sizes")
            self.sizes = [int(v) for v in sizes.tolist()]
            if len(self.sizes) != self.K or min(self.sizes) < 1 or max(self.sizes) > self.n:
                raise ValueError(f"sizes must be {self.K} values in [1, {self.n}]")
        n_min = self.n if self.sizes is None else min(self.sizes)
        if n_min < self.B:
            raise RuntimeError(f"{self.N} windows over {self.K} clients leave {n_min} per client < batch {self.B}")
        self.seed = 0 if seed is None else int(seed)
        self.passes = (self.S * self.B + n_min - 1) // n_min  # permutations of a partition per client and round

    def _round_seed(self, r: int) -> int:
        from ..utils.philox import mix64
        return mix64(self.seed) ^ int(r)

    def clients_of(self, r: int) -> List[int]:
        """The cohort of round ``r``: ``cohort`` distinct client ids, in the order of their table columns."""
        g = torch.Generator()
        g.manual_seed(self._round_seed(r))
        return torch.randperm(self.K, generator=g)[: self.M].tolist()

    def fill(self, r: int, table: torch.Tensor) -> List[int]:
        """Write round ``r``'s batches into ``table`` (int32 ``[steps, cohort * B]``) in place; returns the cohort."""
        if table.dtype != torch.int32 or tuple(table.shape) != (self.S, self.M * self.B):
            raise ValueError(f"index table must be int32 [{self.S}, {self.M * self.B}], got {table.dtype} "
                             f"{tuple(table.shape)}")
        from ..utils.philox import mix64
        ids = self.clients_of(r)
        g = torch.Generator(device=self.device)
        g.manual_seed(mix64(self._round_seed(r)))
        keys = torch.randint(0, 1 << 62, (self.M, self.passes, self.n), device=self.device, generator=g,
                             dtype=torch.int64)
        if self.sizes is not None:
            # entries past a client's n_k get a key above every drawn one: the argsort's first n_k are a uniform
            # permutation of its partition
            nk = torch.tensor([self.sizes[i] for i in ids], dtype=torch.int64).to(self.device)
            pos = torch.arange(self.n, device=self.device)
            keys = torch.where(pos[None, None, :] < nk[:, None, None], keys, torch.full_like(keys, 1 << 62))
            t = torch.arange(self.S * self.B, device=self.device)[None, :]
            perm = keys.argsort(dim=2).reshape(self.M, self.passes * self.n)
            rows = perm.gather(1, (t // nk[:, None]) * self.n + t % nk[:, None])
        else:
            rows = keys.argsort(dim=2).reshape(self.M, self.passes * self.n)[:, : self.S * self.B]
        if self.order is None:
            rows = rows + (torch.tensor(ids, dtype=torch.int64) * self.n).to(self.device)[:, None]
        else:
            rows = self.order[torch.tensor(ids, dtype=torch.int64).to(self.device)].gather(1, rows)
        # [M, S, B] -> [S, M, B]: a step's row holds the clients' batches back to back
        table.copy_(rows.view(self.M, self.S, self.B).permute(1, 0, 2).reshape(self.S, self.M * self.B))
        return ids

    def sizes_of(self, ids: List[int]) -> List[int]:
        """The partition sizes n_k of the clients ``ids``."""
        return [self.n if self.sizes is None else self.sizes[i] for i in ids]

    def steps_of(self, ids: List[int], local_epochs: int) -> List[int]:
        """Local steps of the clients ``ids`` for ``local_epochs`` E passes over their own rows in batches of B:
        ``S_k = min(S, max(1, E * (n_k // B)))``; E == 0: S for everyone."""
        E = int(local_epochs)
        if E < 0:
            raise ValueError("local_epochs must be >= 0")
        if E == 0:
            return [self.S] * len(ids)
        return [min(self.S, max(1, E * (n // self.B))) for n in self.sizes_of(ids)]
