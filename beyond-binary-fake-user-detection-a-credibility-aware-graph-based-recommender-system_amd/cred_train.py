"""SLAS subgraph sampling and the credibility-GNN training loop on the device.

Restates ``train_and_export_credibility`` (main.py:609-1025) from the loaded
graph tensors on: the similarity profiles (:727-737), the two reference-order
CSRs (:739-753), ``build_slas_subgraph`` (:809-883), the losses (:650-658,
:897-907), the training loop (:885-963), the export pass and the min-max
normalisation (:965-1025). The output, ``credibility_scores_minmax.npy``, is
what the drop-in ``build_message_passing_mats`` loads.

The reference builds a subgraph three times per step with a Python loop per
seed user, per sampled item and per edge of every subgraph user. Here one call
is a fixed sequence of launches:

* ``bbgr_slas_sample`` (user rows, temporal view)  -> items per seed
* mark + ``bbgr_mask_to_list``                      -> ``items_global`` (np.unique)
* ``bbgr_slas_sample`` (item rows, labels upweighted, no view) -> users per item
* mark, clear the seeds, ``bbgr_mask_to_list``       -> ``extra_only``
* ``bbgr_list_positions``, ``bbgr_slas_induce``      -> the induced edge list

and three scalar device->host reads (item, user and edge counts) that size the
outputs. The feature, label and attribute gathers are ``index_select``.

The device sampler draws by exponential clocks from Philox (bbgr.h); it has
the distribution of the reference's ``rng.choice(.., replace=False, p=w)`` but
not numpy's stream: subgraphs agree with the reference in law and, given the
same picks, exactly. The host-side draws (labeled split, epoch shuffles) are
numpy's, in the reference's call order.
"""
from __future__ import annotations

import csv
import ctypes
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from ._lib import call, ptr, stream_handle
from .cred_gnn import EDGE_ATTR_KEYS, CredModel
from .scatter import index_add_rows

# main.py:629-643
SLAS_KAPPA = 3.0
SLAS_UPWEIGHT_LABELED = 1.0
K_USER_NEIGH = 15
K_ITEM_NEIGH = 15
LAMBDA_SMOOTH = 0.1
LAMBDA_CONT = 0.1
TAU_TEMP = 0.2
TEMP_SPLIT = 0.5
SMOOTH_MIN_W = 0.0


def _host_array(x):
    if isinstance(x, torch.Tensor):
        return x
    return np.asarray(x)


def _to_device(x, device, dtype) -> torch.Tensor:
    """numpy arrays, memory maps or tensors -> a contiguous device tensor."""
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=dtype).contiguous()
    a = np.ascontiguousarray(np.asarray(x))
    return torch.from_numpy(a).to(device=device, dtype=dtype).contiguous()


class _RefCsr:
    """build_csr_from_src (main.py:739-749) on the device: rows in ascending
    input edge id. bbgr_csr_build with the edge id as the column sorts by
    (row, edge id), so its indices are the edge ids of the slots."""

    def __init__(self, rows32: torch.Tensor, nbr32: torch.Tensor, n_rows: int):
        dev = rows32.device
        E = rows32.numel()
        self.n_rows = int(n_rows)
        self.indptr = torch.empty(self.n_rows + 1, dtype=torch.int32, device=dev)
        self.eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        cols = torch.arange(E, dtype=torch.int32, device=dev)
        _lib.call_with_workspace("bbgr_csr_build", E, ptr(rows32), ptr(cols), self.n_rows,
                                 max(E, 1), ptr(self.indptr), ptr(self.eid), None, device=dev)
        self.nbr = (nbr32[self.eid[:E].long()].contiguous() if E
                    else torch.zeros(1, dtype=torch.int32, device=dev))


class SlasGraph:
    """The loaded credibility graph on the device: edges, edge attributes,
    features and labels, the two reference-order CSRs and the SLAS profiles.

    ``e_u2i``: [2, E] (numpy, memory map or tensor) or a ``(src, dst)`` pair
    as ``ingest.load_u2i_memmap(with_attr=True)`` returns them.
    """

    def __init__(self, e_u2i, edge_attr, user_x, user_y, item_x, device,
                 edge_attr_keys=EDGE_ATTR_KEYS):
        _lib.require_gpu()
        device = torch.device(device)
        self.device = device
        if isinstance(e_u2i, (tuple, list)):
            src, dst = e_u2i
        else:
            e = _host_array(e_u2i)
            if e.shape[0] != 2:
                raise ValueError("e_u2i must have shape [2, E]")
            src, dst = e[0], e[1]
        self.user_x = _to_device(user_x, device, torch.float32)
        self.user_y = _to_device(user_y, device, torch.int64).view(-1)
        self.item_x = _to_device(item_x, device, torch.float32)
        self.edge_attr = _to_device(edge_attr, device, torch.float32)
        self.U, self.I = int(self.user_x.shape[0]), int(self.item_x.shape[0])
        self.F = int(self.item_x.shape[1])
        if not 1 <= self.F <= 16:
            raise ValueError(f"item feature width {self.F} not in [1, 16]")
        if self.user_y.numel() != self.U:
            raise ValueError("user_y must hold one label per user")
        src32 = _to_device(src, device, torch.int32)
        dst32 = _to_device(dst, device, torch.int32)
        self.E = int(src32.numel())
        if dst32.numel() != self.E or self.edge_attr.shape[0] != self.E:
            raise ValueError("source, destination and edge_attr differ in length")
        if self.E >= 2**31 - 1:
            raise ValueError("E must be < 2^31")
        if self.E and (int(src32.min()) < 0 or int(src32.max()) >= self.U
                       or int(dst32.min()) < 0 or int(dst32.max()) >= self.I):
            raise ValueError("edge index out of range")
        self.edge_attr_keys = list(edge_attr_keys)
        self.ts_idx = self.edge_attr_keys.index("timestamp_norm")
        self.A = int(self.edge_attr.shape[1])
        if self.ts_idx >= self.A:
            raise ValueError("edge_attr has no timestamp_norm column")
        # one float per edge id, read in place from the attribute table
        self._ts_src = self.edge_attr if self.E else torch.zeros(1, self.A, device=device)
        self._ts_ptr = self._ts_src.data_ptr() + 4 * self.ts_idx
        self.u_csr = _RefCsr(src32, dst32, self.U)   # user rows: items, edge ids
        self.i_csr = _RefCsr(dst32, src32, self.I)   # item rows: users, edge ids
        f32 = dict(dtype=torch.float32, device=device)
        self.item_norm = torch.empty(max(self.I, 1), self.F, **f32)
        self.user_mu = torch.empty(max(self.U, 1), self.F, **f32)
        call("bbgr_slas_profiles", self.U, self.I, self.F, ptr(self.item_x),
             self.item_x.stride(0) if self.I else self.F, ptr(self.u_csr.indptr),
             ptr(self.u_csr.nbr), ptr(self.item_norm), ptr(self.user_mu), stream_handle())
        # persistent set tables: all zero / all -1 between calls
        self._mask_u = _lib.byte_mask(self.U, device)
        self._mask_i = _lib.byte_mask(self.I, device)
        self._item_local = torch.full((max(self.I, 1),), -1, dtype=torch.int32, device=device)
        self._counts = torch.zeros(3, dtype=torch.int64, device=device)   # items, users, edges
        self._list_ws: dict = {}
        self.last_picks = None

    # -- pieces ------------------------------------------------------------------
    def sample(self, rows: torch.Tensor, side: str, k: int, *, kappa: float = SLAS_KAPPA,
               temporal_view=None, split: float = TEMP_SPLIT, upweight: float | None = None,
               seed: int = 42, counter: int = 0, stage: int = 0):
        """bbgr_slas_sample over the user rows (side="user": neighbours are
        items) or the item rows (side="item": neighbours are users, the labeled
        ones upweighted when `upweight` is given). Returns (nbr, eid, count):
        int32 [n, k], [n, k] (-1 padded) and [n]."""
        if side == "user":
            csr, rp, npf = self.u_csr, self.user_mu, self.item_norm
        elif side == "item":
            csr, rp, npf = self.i_csr, self.item_norm, self.user_mu
        else:
            raise ValueError("side must be 'user' or 'item'")
        if temporal_view not in _lib.SLAS_VIEW:
            raise ValueError(f"temporal_view must be None, 'early' or 'late', not {temporal_view!r}")
        rows = rows.to(device=self.device, dtype=torch.int64).contiguous()
        n = rows.numel()
        i32 = dict(dtype=torch.int32, device=self.device)
        out_nbr = torch.empty(max(n, 1), k, **i32)
        out_eid = torch.empty(max(n, 1), k, **i32)
        out_cnt = torch.empty(max(n, 1), **i32)
        a = _lib.SlasSampleArgs()
        a.n, a.rows, a.n_rows = n, ptr(rows), csr.n_rows
        a.indptr, a.nbr, a.eid = ptr(csr.indptr), ptr(csr.nbr), ptr(csr.eid)
        a.row_profile, a.nbr_profile = ptr(rp), ptr(npf)
        a.F, a.kappa, a.k = self.F, float(kappa), int(k)
        a.ts, a.ts_stride = self._ts_ptr, self.A
        a.view, a.split = _lib.SLAS_VIEW[temporal_view], float(split)
        if upweight is not None:
            a.label, a.upweight = ptr(self.user_y), float(upweight)
        a.seed, a.counter, a.stage = int(seed), int(counter), int(stage)
        a.out_nbr, a.out_eid, a.out_count = ptr(out_nbr), ptr(out_eid), ptr(out_cnt)
        call("bbgr_slas_sample", ctypes.byref(a), stream_handle())
        return out_nbr[:n], out_eid[:n], out_cnt[:n]

    def _unique(self, ids32: torch.Tensor, mask: torch.Tensor, n_rows: int, slot: int,
                exclude: torch.Tensor | None = None) -> torch.Tensor:
        """Ascending distinct ids >= 0 of a -1-padded int32 list (np.unique),
        less the ids of `exclude`; the mask is all zero again on return. One
        host read (the count)."""
        n = ids32.numel()
        if n == 0 or n_rows == 0:
            return torch.empty(0, dtype=torch.int64, device=self.device)
        st = stream_handle()
        call("bbgr_mark_ids32", n, ptr(ids32), 1, ptr(mask), n_rows, st)
        if exclude is not None and exclude.numel():
            call("bbgr_mark_rows", exclude.numel(), ptr(exclude), 0, ptr(mask), n_rows, st)
        out = torch.empty(max(min(n, n_rows), 1), dtype=torch.int64, device=self.device)
        count = self._counts[slot:slot + 1]
        # hipcub's temp size depends on n_rows only: one buffer per n_rows, sized once
        keep = self._list_ws.setdefault(n_rows, _lib.Workspace(grow=False))
        _lib.call_with_workspace("bbgr_mask_to_list", n_rows, ptr(mask), ptr(out), ptr(count),
                                 after=(st,), device=self.device, keep=keep)
        call("bbgr_mark_ids32", n, ptr(ids32), 0, ptr(mask), n_rows, st)
        return out[: int(count.item())]

    def _induce(self, users_global: torch.Tensor, temporal_view, split: float):
        """(e_u2i [2, E] int64 local ids, eid [E] int64) of main.py:835-856, with
        self._item_local holding the sampled items' local ids. One host read."""
        a = _lib.SlasInduceArgs()
        csr = self.u_csr
        a.n_users_listed, a.users, a.n_users = users_global.numel(), ptr(users_global), self.U
        a.item_local = ptr(self._item_local)
        a.indptr, a.nbr, a.eid = ptr(csr.indptr), ptr(csr.nbr), ptr(csr.eid)
        a.ts, a.ts_stride = self._ts_ptr, self.A
        a.view, a.split = _lib.SLAS_VIEW[temporal_view], float(split)
        count = self._counts[2:3]
        a.count = ptr(count)
        st = stream_handle()
        keep = _lib.Workspace(grow=False)   # the count and the fill share one buffer
        _lib.call_with_workspace("bbgr_slas_induce", ctypes.byref(a), after=(st,),
                                 device=self.device, keep=keep)
        n_e = int(count.item())
        edges = torch.empty(2, n_e, dtype=torch.int64, device=self.device)
        eid = torch.empty(n_e, dtype=torch.int64, device=self.device)
        if n_e:
            a.out_edges, a.out_eid, a.capacity = ptr(edges), ptr(eid), n_e
            _lib.call_with_workspace("bbgr_slas_induce", ctypes.byref(a), after=(st,), keep=keep)
        return edges, eid

    # -- build_slas_subgraph -------------------------------------------------------
    def build_subgraph(self, seed_users, temporal_view=None, *, k_item: int = K_ITEM_NEIGH,
                       k_user: int = K_USER_NEIGH, kappa: float = SLAS_KAPPA,
                       upweight_labeled: float = SLAS_UPWEIGHT_LABELED,
                       split: float = TEMP_SPLIT, counter: int, seed: int = 42) -> dict:
        """main.py:809-883 with the reference's keys; tensors on the device, ids
        and edge lists int64. `seed_users` must be distinct (the reference's
        dictionary silently collapses repeats). `counter` selects the random
        stream of this call: equal (seed, counter) give equal subgraphs."""
        if isinstance(seed_users, torch.Tensor):
            seeds = seed_users.to(device=self.device, dtype=torch.int64).contiguous().view(-1)
        else:
            seeds = torch.from_numpy(np.ascontiguousarray(np.asarray(seed_users, np.int64))) \
                .to(self.device).view(-1)
        bs = int(seeds.numel())
        kw = dict(kappa=kappa, seed=seed, counter=counter)
        it_nbr, it_eid, it_cnt = self.sample(seeds, "user", k_item, temporal_view=temporal_view,
                                             split=split, stage=0, **kw)
        items_global = self._unique(it_nbr, self._mask_i, self.I, 0)
        # the item -> user stage applies no temporal filter (main.py:788-807)
        us_nbr, us_eid, us_cnt = self.sample(items_global, "item", k_user,
                                             upweight=upweight_labeled, stage=1, **kw)
        extra_only = self._unique(us_nbr, self._mask_u, self.U, 1, exclude=seeds)
        users_global = torch.cat([seeds, extra_only])
        self.last_picks = dict(items=(it_nbr, it_eid, it_cnt), items_global=items_global,
                               users=(us_nbr, us_eid, us_cnt))
        ni = int(items_global.numel())
        if ni and users_global.numel():
            st = stream_handle()
            call("bbgr_list_positions", ni, ptr(items_global), ptr(self._counts[0:1]),
                 ptr(self._item_local), st)
            e_u2i, eid = self._induce(users_global, temporal_view, split)
            self._item_local.index_fill_(0, items_global, -1)   # back to all -1
        else:
            e_u2i = torch.zeros(2, 0, dtype=torch.int64, device=self.device)
            eid = torch.zeros(0, dtype=torch.int64, device=self.device)
        ea_u2i = self.edge_attr.index_select(0, eid)
        return {
            "bs": bs,
            "users_global": users_global,
            "items_global": items_global,
            "x_u": self.user_x.index_select(0, users_global),
            "y_u": self.user_y.index_select(0, users_global),
            "x_i": self.item_x.index_select(0, items_global),
            "e_u2i": e_u2i,
            "ea_u2i": ea_u2i,
            "e_i2u": torch.stack([e_u2i[1], e_u2i[0]], dim=0),
            "ea_i2u": ea_u2i,
        }


# -- losses (main.py:650-658, 897-907) ---------------------------------------------
def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    return x / (x.norm(dim=-1, keepdim=True) + eps)


class _GatherRows(torch.autograd.Function):
    """x[idx]; the backward is the deterministic row scatter (autograd's own is
    a float-atomic index_add: the run would not repeat bit for bit)."""

    @staticmethod
    def forward(ctx, x, idx):
        ctx.save_for_backward(idx)
        ctx.n = x.shape[0]
        return x.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        g = g.contiguous()
        out = torch.zeros(ctx.n, g.shape[1], dtype=g.dtype, device=g.device)
        if idx.numel():
            index_add_rows(out, idx, g)
        return out, None


def _gather_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    if x.is_cuda and x.dtype == torch.float32 and x.shape[1] in (8, 16, 32, 64, 128, 256):
        return _GatherRows.apply(x, idx)
    return x.index_select(0, idx)


def smoothness_loss(h_u2: torch.Tensor, h_i1: torch.Tensor, e_u2i: torch.Tensor,
                    w_u2i_norm: torch.Tensor, min_w: float = SMOOTH_MIN_W) -> torch.Tensor:
    """mean over the edges with w > min_w of w * |h_u2[src] - h_i1[dst]|^2, 0
    when there is none (main.py:897-907), without the host's `mask.any()`."""
    if e_u2i.size(1) == 0:
        return torch.zeros((), device=h_u2.device)
    w = w_u2i_norm
    mask = (w > min_w).to(w.dtype)
    diff = _gather_rows(h_u2, e_u2i[0]) - _gather_rows(h_i1, e_u2i[1])
    num = (w * mask * diff.pow(2).sum(dim=-1)).sum()
    return num / mask.sum().clamp(min=1.0)


def info_nce(z1: torch.Tensor, z2: torch.Tensor, tau: float) -> torch.Tensor:
    """main.py:653-658; the B x B logits product is one library GEMM."""
    z1 = l2_normalize(z1)
    z2 = l2_normalize(z2)
    logits = (z1 @ z2.t()) / tau
    labels = torch.arange(z1.size(0), device=z1.device)
    return F.cross_entropy(logits, labels)


def supervised_loss(pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """BCE over the labeled (y >= 0) entries, 0 when there is none
    (main.py:945-951), without a boolean-index host read."""
    keep = (y >= 0).to(pred.dtype)
    s = F.binary_cross_entropy(pred, y.clamp(min=0).to(pred.dtype), weight=keep, reduction="sum")
    return s / keep.sum().clamp(min=1.0)


def step_loss(model, g1: dict, g2: dict, *, lambda_smooth: float = LAMBDA_SMOOTH,
              lambda_cont: float = LAMBDA_CONT, tau: float = TAU_TEMP) -> torch.Tensor:
    """The objective of one training step over the early (g1) and late (g2)
    subgraphs of the same seeds (main.py:936-956)."""
    o1 = model.forward_subgraph(g1["x_u"], g1["x_i"], g1["e_u2i"], g1["ea_u2i"], g1["e_i2u"],
                                g1["ea_i2u"])
    o2 = model.forward_subgraph(g2["x_u"], g2["x_i"], g2["e_u2i"], g2["ea_u2i"], g2["e_i2u"],
                                g2["ea_i2u"])
    pred1, h_u2_1, h_i1_1, w1t_1 = o1
    h_u2_2 = o2[1]
    bs = g1["bs"]
    loss_sup = supervised_loss(pred1[:bs], g1["y_u"][:bs])
    loss_smooth = smoothness_loss(h_u2_1, h_i1_1, g1["e_u2i"], w1t_1)
    loss_cont = info_nce(h_u2_1[:bs], h_u2_2[:bs], tau=tau)
    return loss_sup + lambda_smooth * loss_smooth + lambda_cont * loss_cont


# -- host planning (main.py:885-892, 909-919) --------------------------------------
class HostPlan:
    """The reference's host draws, in its call order: default_rng(seed), one
    shuffle of the labeled users, the 80 % split, then one shuffle of the train
    users per epoch. (The reference's rng also feeds its samplers between the
    epochs, so only the split and the first epoch's order equal its run.)"""

    def __init__(self, user_y, seed: int = 42):
        y = user_y.detach().cpu().numpy() if isinstance(user_y, torch.Tensor) else np.asarray(user_y)
        labeled = np.nonzero(y.reshape(-1) >= 0)[0].astype(np.int64)
        if labeled.size == 0:
            raise RuntimeError("No labeled users found (y>=0).")
        self.rng = np.random.default_rng(seed)
        self.rng.shuffle(labeled)
        self.labeled_users = labeled
        self.train_users = labeled[: int(0.8 * labeled.size)]

    def epoch_batches(self, batch_size: int) -> list:
        self.rng.shuffle(self.train_users)
        t = self.train_users
        return [np.asarray(t[j:j + batch_size], dtype=np.int64).copy()
                for j in range(0, len(t), batch_size)]


def minmax_normalize(cred: np.ndarray) -> np.ndarray:
    """main.py:986-993: (x - min) / (max - min) in fp32, all zeros when constant."""
    cred = np.asarray(cred, dtype=np.float32)
    cmin, cmax = float(cred.min()), float(cred.max())
    if (cmax - cmin) < 1e-12:
        return np.zeros_like(cred, dtype=np.float32)
    return ((cred - cmin) / (cmax - cmin)).astype(np.float32)


def write_credibility_csv(path, scores, idx2user=None) -> None:
    """main.py:1014-1019: header user_id,user_idx,credibility; %.6f scores; the
    user id left empty where idx2user has none."""
    n_ids = len(idx2user) if idx2user is not None else 0
    with open(path, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f)
        w.writerow(["user_id", "user_idx", "credibility"])
        for idx, score in enumerate(np.asarray(scores).reshape(-1)):
            uid = idx2user[idx] if idx < n_ids else None
            w.writerow([uid, idx, f"{float(score):.6f}"])


def export_credibility(graph: SlasGraph, model, batch_size: int = 2048, *, counter: int = 0,
                       seed: int = 42) -> torch.Tensor:
    """The export pass (main.py:965-984): every user's score from its own
    temporal_view=None subgraph, in batches; fp32 [U] on the device."""
    model.eval()
    cred_all = torch.empty(graph.U, dtype=torch.float32, device=graph.device)
    with torch.no_grad():
        for j in range(0, graph.U, batch_size):
            users = torch.arange(j, min(j + batch_size, graph.U), dtype=torch.int64,
                                 device=graph.device)
            g = graph.build_subgraph(users, None, counter=counter, seed=seed)
            counter += 1
            pred = model.forward_subgraph(g["x_u"], g["x_i"], g["e_u2i"], g["ea_u2i"],
                                          g["e_i2u"], g["ea_i2u"])[0]
            cred_all[j:j + g["bs"]] = pred[: g["bs"]]
    return cred_all


def train_and_export_credibility(graph: SlasGraph, *, hidden_dim: int = 64, epochs: int = 100,
                                 batch_size: int = 2048, lr: float = 1e-3,
                                 lambda_smooth: float = LAMBDA_SMOOTH,
                                 lambda_cont: float = LAMBDA_CONT, tau: float = TAU_TEMP,
                                 seed: int = 42, out_dir=None, idx2user=None, model=None) -> dict:
    """main.py:885-1025. Returns {"cred_raw", "cred" (min-max, numpy fp32 [U]),
    "model", "losses" (per-epoch mean)}; with out_dir also writes
    credibility_scores_minmax.npy, credibility_scores_minmax_with_user_id.csv
    and cred_model.pt. The model's initial weights are drawn under
    torch.manual_seed(seed) in a forked generator unless `model` is given."""
    plan = HostPlan(graph.user_y, seed)
    if model is None:
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            model = CredModel(graph.user_x.shape[1], graph.item_x.shape[1], hidden_dim,
                              graph.edge_attr_keys)
    model = model.to(graph.device)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    counter = 0   # one random stream per build_subgraph call
    losses = []
    for _ in range(epochs):
        model.train()
        total = torch.zeros((), device=graph.device)
        nsteps = 0
        for batch in plan.epoch_batches(batch_size):
            g1 = graph.build_subgraph(batch, "early", counter=counter, seed=seed)
            g2 = graph.build_subgraph(batch, "late", counter=counter + 1, seed=seed)
            counter += 2
            opt.zero_grad()
            loss = step_loss(model, g1, g2, lambda_smooth=lambda_smooth, lambda_cont=lambda_cont,
                             tau=tau)
            loss.backward()
            opt.step()
            total += loss.detach()
            nsteps += 1
        losses.append(float(total) / max(nsteps, 1))
    cred_raw = export_credibility(graph, model, batch_size, counter=counter, seed=seed).cpu().numpy()
    cred = minmax_normalize(cred_raw)
    if out_dir is not None:
        out = Path(out_dir)
        out.mkdir(parents=True, exist_ok=True)
        np.save(out / "credibility_scores_minmax.npy", cred)
        write_credibility_csv(out / "credibility_scores_minmax_with_user_id.csv", cred, idx2user)
        torch.save(model.state_dict(), out / "cred_model.pt")
    return {"cred_raw": cred_raw, "cred": cred, "model": model, "losses": losses}
