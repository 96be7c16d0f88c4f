"""Recommendation lists: the top-k items of a set of users, on the device.

recommend() ranks the whole catalogue for every listed user with the scoring
chain of the full-ranking evaluation (bbgr_recommend: fp32 MFMA, one fma chain
per score over the components 0, d/2, 1, d/2+1, ...; order (score desc, item id
asc)) and returns the lists themselves. Unlike evaluate_full it

  - takes any users, in any order, duplicates included (no test CSR);
  - DROPS excluded items (a CSR of items per user, typically the train
    interactions) instead of scoring them -1e9, so a list never holds one;
  - can restrict the catalogue with an item mask (e.g. long-tail items only);
  - serves every embedding width 8 ... 256 and any k up to 128, exactly
    (k above the kernel's register list depth runs continuation passes).

A user with fewer than k eligible items gets -1 / -inf in the tail of the row.

precision="bf16" ranks by the scores of the bf16-rounded tables on the bf16
MFMA (bbgr_recommend_bf16): cheapest, approximate near ties. precision=
"bf16_exact" uses that pass for candidates only: bbgr_recommend_rescore scores
them with the fp32 chain and certifies, per user, that no other item can enter
the list (|s^ - s| <= bf16_error_bound(d) ||u|| ||i||); the users it cannot
certify go through the fp32 kernel. Its result is the fp32 result, bit for bit.
evaluate_ranking() is the full-ranking protocol computed from these lists
(bbgr_eval_lists reduces caller-supplied lists to the metric sums).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from . import evaluation as E
from ._lib import ld, ptr
from .graph import Csr

MAX_K = 128
WIDTHS = (8, 16, 32, 64, 128, 256)
PRECISIONS = ("fp32", "bf16", "bf16_exact")


def bf16_error_bound(d: int) -> float:
    """eps(d) with |s^ - s| <= eps(d) ||u|| ||i||: s^ the fp32-accumulated score
    of the bf16-rounded rows, s the fp32 fma chain. 1.02 * 2^-7 covers the
    rounding of both operands (2^-8 each: bf16 has 8 significant bits),
    d * 2^-21 both accumulations (csrc/recommend_bf16.hip has the derivation)."""
    return 1.02 * 2.0 ** -7 + d * 2.0 ** -21


def default_prefilter_k(k: int) -> int:
    """Candidates per user of the bf16 pass of precision="bf16_exact"."""
    return min(MAX_K, max(32, 2 * k))


def _exclusion(exclude, n_user_rows: int, n_items: int, dev) -> Csr | None:
    if exclude is None:
        return None
    if not isinstance(exclude, Csr):
        exclude = E.csr_from_host(exclude, n_items, dev)
    if exclude.n_rows != n_user_rows or exclude.n_cols != n_items:
        raise ValueError(f"exclude: a [{n_user_rows} x {n_items}] CSR expected, got "
                         f"[{exclude.n_rows} x {exclude.n_cols}]")
    if not exclude.cols_sorted:
        raise ValueError("exclude: the rows' columns must be sorted ascending")
    if exclude.indptr.device != dev:
        raise ValueError("exclude: the CSR is on another device")
    return exclude


def _bf16_table(t: torch.Tensor) -> torch.Tensor:
    """An fp32 table [n, d] (d a multiple of 8 here: 64, 128, 256) rounded to
    bf16 by bbgr_to_bf16."""
    out = torch.empty(t.shape[0], (t.shape[1] + 7) // 8 * 8, dtype=torch.bfloat16,
                      device=t.device)
    _lib.call("bbgr_to_bf16", t.shape[0], t.shape[1], ptr(t), ld(t), ptr(out), ld(out),
              _lib.stream_handle())
    return out


def _fill(a, n, users, n_user_rows, uf, itf, n_items, k, ex, mask, topk, scores):
    a.n_users, a.users, a.n_user_rows = n, ptr(users), n_user_rows
    a.uf, a.lduf, a.itf, a.ldif = ptr(uf), ld(uf), ptr(itf), ld(itf)
    a.d, a.n_items, a.k = uf.shape[1], n_items, k
    if ex is not None:
        a.ex_indptr, a.ex_indices = ptr(ex.indptr), ptr(ex.indices)
    a.item_mask = ptr(mask)
    a.topk, a.topk_score = ptr(topk), ptr(scores)
    return a


def recommend(user_emb: torch.Tensor, item_emb: torch.Tensor, users, k: int, exclude=None,
              item_mask=None, return_scores: bool = False, precision: str = "fp32",
              prefilter_k: int | None = None, return_info: bool = False):
    """topk int32 [n, k] (and scores float32 [n, k]) on the device: for each
    of `users` (ids into user_emb, any order, duplicates allowed) the k
    eligible items of highest score <user_emb[u], item_emb[i]>, ties to the
    lower item id; -1 (-inf) where fewer than k items are eligible.

    exclude: a graph.Csr [n_user_rows x n_items] or a host (indptr, indices)
    pair, rows sorted ascending (duplicates allowed): items left out per user.
    item_mask: [n_items], nonzero / True = eligible.
    Widths 8, 16 and 32 are zero-padded to 64 columns so that the scores are
    the true width's chain (evaluation._pad_narrow). 1 <= k <= 128.

    precision: "fp32" (default); "bf16": lists and scores of the bf16-rounded
    tables; "bf16_exact": the fp32 lists and scores, bit for bit, from a bf16
    pass for prefilter_k candidates per user (default default_prefilter_k(k);
    k <= prefilter_k <= 128), an fp32 rescoring with a per-user certificate,
    and the fp32 kernel for the users it does not certify (one device-to-host
    read of their count).
    return_info=True appends a dict: certified (bool [n], on the device),
    n_fallback, k_pre (under "fp32" / "bf16": all False, 0, None)."""
    _lib.require_gpu(user_emb)
    dev = user_emb.device
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    k_pre = None
    if precision == "bf16_exact":
        k_pre = default_prefilter_k(k) if prefilter_k is None else int(prefilter_k)
        if not k <= k_pre <= MAX_K:
            raise ValueError(f"prefilter_k must be in [k, {MAX_K}] = [{k}, {MAX_K}], got {k_pre}")
    elif prefilter_k is not None:
        raise ValueError('prefilter_k belongs to precision="bf16_exact"')
    if user_emb.dim() != 2 or item_emb.dim() != 2 or user_emb.shape[1] != item_emb.shape[1]:
        raise ValueError("user_emb and item_emb must be 2-D tables of one width")
    if user_emb.shape[1] not in WIDTHS:
        raise ValueError(f"embedding width {user_emb.shape[1]} unsupported {WIDTHS}")
    n_user_rows, n_items = user_emb.shape[0], item_emb.shape[0]
    users = torch.as_tensor(users).to(dev, torch.int64).contiguous().view(-1)
    n = users.numel()
    topk = torch.empty(n, k, dtype=torch.int32, device=dev)
    scores = torch.empty(n, k, dtype=torch.float32, device=dev) if return_scores else None
    info = dict(certified=torch.zeros(n, dtype=torch.bool, device=dev), n_fallback=0, k_pre=k_pre)

    def result():
        out = (topk, scores) if return_scores else (topk,)
        out = out + (info,) if return_info else out
        return out if len(out) > 1 else out[0]

    if n == 0:
        return result()
    lo, hi = (int(x) for x in torch.aminmax(users))
    if lo < 0 or hi >= n_user_rows:
        raise ValueError(f"user ids must be in [0, {n_user_rows}); got [{lo}, {hi}]")
    ex = _exclusion(exclude, n_user_rows, n_items, dev)
    mask = None
    if item_mask is not None:
        mask = (torch.as_tensor(item_mask).to(dev) != 0).to(torch.uint8).contiguous().view(-1)
        if mask.numel() != n_items:
            raise ValueError(f"item_mask: {n_items} entries expected, got {mask.numel()}")
    uf = user_emb.detach().to(torch.float32).contiguous()
    itf = item_emb.detach().to(dev, torch.float32).contiguous()
    if uf.shape[1] in E.NARROW_WIDTHS:
        uf, itf = E._pad_narrow(uf), E._pad_narrow(itf)
    if precision == "fp32":
        a = _fill(_lib.RecommendArgs(), n, users, n_user_rows, uf, itf, n_items, k, ex, mask,
                  topk, scores)
        E._run("bbgr_recommend", a, dev)
        return result()
    ufh, ith = _bf16_table(uf), _bf16_table(itf)
    if precision == "bf16":
        a = _fill(_lib.RecommendBf16Args(), n, users, n_user_rows, ufh, ith, n_items, k, ex, mask,
                  topk, scores)
        E._run("bbgr_recommend_bf16", a, dev)
        return result()
    # bf16_exact: candidates, their fp32 scores and the certificate, the rest in fp32
    n_max = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.call("bbgr_row_norm_max", n_items, itf.shape[1], ptr(itf), ld(itf), ptr(n_max),
              _lib.stream_handle())
    cand = torch.empty(n, k_pre, dtype=torch.int32, device=dev)
    cand_score = torch.empty(n, k_pre, dtype=torch.float32, device=dev)
    a = _fill(_lib.RecommendBf16Args(), n, users, n_user_rows, ufh, ith, n_items, k_pre, ex, mask,
              cand, cand_score)
    E._run("bbgr_recommend_bf16", a, dev)
    if scores is None:
        scores = torch.empty(n, k, dtype=torch.float32, device=dev)
    cert = torch.empty(n, dtype=torch.uint8, device=dev)
    r = _lib.RecommendRescoreArgs()
    r.n_users, r.users, r.n_user_rows = n, ptr(users), n_user_rows
    r.uf, r.lduf, r.itf, r.ldif = ptr(uf), ld(uf), ptr(itf), ld(itf)
    r.d, r.n_items, r.k, r.k_pre = uf.shape[1], n_items, k, k_pre
    r.cand, r.cand_score, r.n_max = ptr(cand), ptr(cand_score), ptr(n_max)
    r.topk, r.topk_score, r.certified = ptr(topk), ptr(scores), ptr(cert)
    _lib.call("bbgr_recommend_rescore", ctypes.byref(r), _lib.stream_handle())
    n_fb = n - int(cert.sum())      # the one device-to-host read
    if n_fb:
        # the uncertified positions in order, without a second read of the device
        rows = torch.argsort(cert, stable=True)[:n_fb]
        fb = recommend(uf, itf, users[rows], k, exclude=ex, item_mask=mask, return_scores=True)
        topk[rows], scores[rows] = fb
    info.update(certified=cert.bool(), n_fallback=n_fb)
    if not return_scores:
        scores = None
    return result()


def recommend_model(model, users, k: int, **kw):
    """recommend() on a drop-in module's final tables (final_embeddings() or
    get_user_item_emb(), as the reference's evaluate_* read them)."""
    ue, ie = E._model_tables(model, next(model.parameters()).device)
    return recommend(ue, ie, users, k, **kw)


def evaluate_ranking(user_emb: torch.Tensor, item_emb: torch.Tensor, train_csr: Csr,
                     test_csr: Csr, num_items: int, item_pop, total_train_interactions: int,
                     cred, Ks=(10, 20), cred_group_pct: float = 0.20, return_raw: bool = False,
                     users=None, groups=None, cred_utility=None, precision: str = "fp32"):
    """The full-ranking protocol with evaluate_full's signature and result
    dictionary ("mode": "full"; `_raw` under return_raw=True), computed as
    recommend(exclude = train rows) followed by bbgr_eval_lists. Every
    embedding width 8 ... 256 and max(Ks) <= 128.

    Where it differs from evaluate_full: train items never enter a list here,
    while evaluate_full (as the reference) ranks them at -1e9. The two agree
    bit for bit unless a user has fewer than max(Ks) items outside the train
    row; for such a user evaluate_full fills the tail with train items (which
    count in coverage and novelty) and this function leaves it at -1, skipped
    by every metric.

    precision: recommend()'s; "bf16_exact" gives the "fp32" dictionary exactly."""
    _lib.require_gpu(user_emb)
    dev = user_emb.device
    users = E._eval_users(test_csr) if users is None else users.to(dev, torch.int64)
    n = users.numel()
    Ks = tuple(int(k) for k in Ks)
    k_max = max(Ks)
    topk, topk_score = recommend(user_emb, item_emb[:num_items], users, k_max,
                                 exclude=train_csr, return_scores=True, precision=precision)
    uf, itf, pop, cred_t = E._tables(user_emb, item_emb, item_pop, cred, dev)
    groups = (E.cred_groups(users, cred_t, cred_group_pct) if groups is None
              else torch.as_tensor(groups).to(dev, torch.uint8))
    sums = torch.empty(len(Ks) * E.NOUT, dtype=torch.float64, device=dev)
    a = E._args(users, train_csr, test_csr, uf, itf, num_items, Ks, pop,
                total_train_interactions, groups, sums)
    a.topk = ptr(topk)
    E._run("bbgr_eval_lists", a, dev)
    cu = float(cred_t[users].double().mean()) if cred_utility is None else cred_utility
    results = E._results(sums, Ks, num_items, cu, "full", {})
    if return_raw:
        results["_raw"] = dict(users=users, topk=topk.view(n, k_max),
                               topk_score=topk_score.view(n, k_max), groups=groups)
    return results
