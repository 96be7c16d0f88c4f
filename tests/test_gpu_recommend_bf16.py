"""GPU: recommend(precision="bf16" / "bf16_exact") and the three entry points
behind them (bbgr_recommend_bf16, bbgr_row_norm_max, bbgr_recommend_rescore).

Shapes, users and exclusion rows are tests/test_gpu_recommend.py's (U = 300,
I = 1500, 257 listed users with one duplicate, user 7 keeping 5 items).

 - Integer tables (entries in {-2..2}): every product and partial sum is a
   small integer, exact in bf16 and in fp32 in any summation order, so the
   "bf16" lists and scores are the fp32 oracle's, bit for bit, with many ties.
 - Uniform tables under "bf16": against float64 on the bf16-rounded tables,
   within d_k * 2^-21 * sum |u^_c||i^_c| (one fp32 ulp per addition with a
   factor two to spare; d_k = the kernel's width, 64 for the narrow tables,
   whose zero padding adds exactly).
 - "bf16_exact": bit for bit the "fp32" result and the oracle's, on tables
   that certify every user, none, and (near ties the bf16 pass cannot see)
   tables whose true lists lie outside the candidates.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bbgr import _lib  # noqa: E402
from oracle import native as N  # noqa: E402
from test_gpu_recommend import (DEV, I, KS_64, KS_OTHER, U, WIDTHS, _check, _eval_inputs,  # noqa: E402
                                _ex_csr, _exclusion, _frozen, _oracle, _rows_to_csr, _t, _tables,
                                _users)

WIDE = (64, 128, 256)


def _bf16(a):
    return torch.tensor(np.asarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def _want(ptr, idx, uf, itf, k):
    """The oracle's lists with the -1e9 entries (excluded items) dropped."""
    items, scores = N.full_topk(_users(), ptr, idx, uf, itf, k)
    real = scores > -1e8
    assert (real[:, :-1] >= real[:, 1:]).all()
    return np.where(real, items, -1), np.where(real, scores, -np.inf).astype(np.float32)


def _rec(uf, itf, k, n_items=I, **kw):
    from bbgr.recommend import recommend
    kw.setdefault("exclude", _ex_csr(n_items))
    return recommend(_t(uf), _t(itf), _t(_users(), torch.long), k, return_scores=True, **kw)


# ---------------------------------------------------------------------------
# integer tables
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _int_tables(d, n_items=I):
    rng = np.random.default_rng(2000 + d + n_items)
    uf = rng.integers(-2, 3, (U, d)).astype(np.float32)
    itf = rng.integers(-2, 3, (n_items, d)).astype(np.float32)
    return _frozen(uf, itf)


@functools.lru_cache(maxsize=None)
def _int_oracle(d, n_items=I, k=128):
    ptr, idx, _ = _exclusion(n_items)
    return _frozen(*_want(ptr, idx, *_int_tables(d, n_items), k))


INT_CASES = [(64, k) for k in KS_64] + [(d, k) for d in WIDTHS if d != 64 for k in KS_OTHER]


@pytest.mark.parametrize("d,k", INT_CASES)
def test_bf16_integer_tables_bitexact(d, k):
    uf, itf = _int_tables(d)
    want = _int_oracle(d)
    # many ties: on average a score value is shared by several of a row's 128 entries
    assert np.mean([np.unique(r[r > -np.inf]).size for r in want[1]]) < 64
    got = _rec(uf, itf, k, precision="bf16")
    _check(got, want, k)
    b7 = int(np.flatnonzero(_users() == 7)[0])
    row = got[0][b7].cpu().numpy()
    assert (row[:min(k, 5)] >= 0).all() and (row[5:] == -1).all()


@pytest.mark.parametrize("d", WIDTHS)
def test_bf16_integer_tables_item_mask(d):
    """Items j % 3 != 0 only, with the exclusion rows: the oracle's lists with
    each row united with the ineligible items."""
    uf, itf = _int_tables(d)
    mask = np.arange(I) % 3 != 0
    off = np.flatnonzero(~mask).astype(np.int32)
    _, _, rows = _exclusion()
    want = _want(*_rows_to_csr([np.union1d(r, off).astype(np.int32) for r in rows]), uf, itf, 128)
    for k in KS_OTHER:
        got = _rec(uf, itf, k, precision="bf16", item_mask=_t(mask, torch.bool))
        _check(got, want, k)
        assert (got[0].cpu().numpy() % 3 != 0).all()


@pytest.mark.parametrize("n_items", [5, 31, 33, 129])
def test_bf16_small_catalogues(n_items):
    """Less than a sub-tile, one short of it, one over, one over a tile."""
    for d, k in ((64, 33), (256, 10)):
        uf, itf = _int_tables(d, n_items)
        got = _rec(uf, itf, k, n_items, precision="bf16")
        _check(got, _int_oracle(d, n_items, k), k)
        _, _, rows = _exclusion(n_items)
        n_ok = np.array([n_items - np.unique(rows[u]).size for u in _users()])
        assert np.array_equal((got[0].cpu().numpy() >= 0).sum(1), np.minimum(n_ok, k))


def test_bf16_two_runs_identical():
    for d, k in ((64, 100), (256, 33)):
        uf, itf = _tables(d)
        a, b = _rec(uf, itf, k, precision="bf16"), _rec(uf, itf, k, precision="bf16")
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32),
                                                       b[1].view(torch.int32))


# ---------------------------------------------------------------------------
# uniform tables, "bf16"
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
def test_bf16_uniform_tables_against_float64(d):
    k = 33
    uf, itf = _tables(d)
    uh, ih = _bf16(uf).astype(np.float64), _bf16(itf).astype(np.float64)
    users = _users()
    ref = uh[users] @ ih.T
    tol = max(d, 64) * 2.0 ** -21 * (np.abs(uh[users]) @ np.abs(ih).T)
    mask = np.arange(I) % 5 != 0
    _, _, rows = _exclusion()
    ok = np.tile(mask, (users.size, 1))
    for b, u in enumerate(users):
        ok[b, rows[u]] = False
    topk, score = (x.cpu().numpy() for x in _rec(uf, itf, k, precision="bf16", item_mask=mask))
    worst = 0.0
    for b in range(users.size):
        row, sc = topk[b], score[b].astype(np.float64)
        n = int((row >= 0).sum())
        assert (row[n:] == -1).all() and np.isneginf(sc[n:]).all()
        assert n == min(k, int(ok[b].sum()))
        items = row[:n]
        assert ok[b, items].all() and np.unique(items).size == n
        err = np.abs(sc[:n] - ref[b, items])
        worst = max(worst, float((err / tol[b, items]).max()))
        assert (err <= tol[b, items]).all()
        # sorted by (score desc, item asc) on the kernel's own scores
        assert ((sc[:n - 1] > sc[1:n]) | ((sc[:n - 1] == sc[1:n]) & (items[:-1] < items[1:]))).all()
        # nothing eligible left out that beats the row's last score by more than its tolerance
        if n == k:
            out = ok[b].copy()
            out[items] = False
            assert not (ref[b, out] > sc[n - 1] + tol[b, out]).any()
    print(f"d={d}: worst |score - float64| / tolerance = {worst:.3f}")


# ---------------------------------------------------------------------------
# "bf16_exact"
# ---------------------------------------------------------------------------
def _exact(uf, itf, k, k_pre, want):
    """bf16_exact == fp32 == the oracle, bit for bit; returns the info dict."""
    topk, score, info = _rec(uf, itf, k, precision="bf16_exact", prefilter_k=k_pre,
                             return_info=True)
    fp32 = _rec(uf, itf, k)
    assert torch.equal(topk, fp32[0])
    assert torch.equal(score.view(torch.int32), fp32[1].view(torch.int32))
    _check((topk, score), want, k)
    cert = info["certified"]
    assert cert.dtype == torch.bool and cert.is_cuda and cert.shape == (_users().size,)
    assert info["k_pre"] == k_pre and info["n_fallback"] == int((~cert).sum())
    return info


K_PAIRS = [(1, 32), (10, 32), (16, 32), (33, 66), (64, 128), (128, 128)]
# (the narrow widths run the d = 64 kernels on padded tables: two pairs each)
EXACT_CASES = ([(d, k, kp) for d in WIDE for k, kp in K_PAIRS]
               + [(d, k, kp) for d in WIDTHS if d < 64 for k, kp in ((10, 32), (128, 128))])


@pytest.mark.parametrize("d,k,k_pre", EXACT_CASES)
def test_bf16_exact_plain_tables(d, k, k_pre):
    info = _exact(*_tables(d), k, k_pre, _oracle(d))
    b7 = int(np.flatnonzero(_users() == 7)[0])
    assert bool(info["certified"][b7])     # 5 eligible items: the candidates are all of them
    print(f"d={d} k={k} k_pre={k_pre}: fallback {info['n_fallback']} of {_users().size}")
    if d >= 64 and (k, k_pre) == (10, 32):
        assert bool(info["certified"].all())        # computed on the host beforehand
    if k == k_pre:
        assert info["n_fallback"] > 200             # t^ is the k-th score itself


@pytest.mark.parametrize("d", WIDE)
def test_bf16_exact_default_prefilter(d):
    """prefilter_k=None: min(128, max(32, 2 k)); ids only."""
    from bbgr.recommend import recommend
    uf, itf = _tables(d)
    users = _t(_users(), torch.long)
    topk, info = recommend(_t(uf), _t(itf), users, 17, exclude=_ex_csr(), precision="bf16_exact",
                           return_info=True)
    assert info["k_pre"] == 34
    assert torch.equal(topk, recommend(_t(uf), _t(itf), users, 17, exclude=_ex_csr()))


@pytest.mark.parametrize("d", WIDE)
def test_bf16_exact_tied_tables_fall_back(d):
    """50 exact copies per score: the k-th and the k_pre-th score tie, nothing
    is certified but the user with 5 items, and the fp32 kernel decides."""
    uf, itf = _tables(d, "tied")
    info = _exact(uf, itf, 10, 32, _oracle(d, "tied"))
    assert info["n_fallback"] > 0
    assert info["n_fallback"] == int((_users() != 7).sum())
    info = _exact(uf, itf, 128, 128, _oracle(d, "tied"))
    assert info["n_fallback"] > 0


@functools.lru_cache(maxsize=None)
def _near_tie_tables(d):
    """Items 0..47 are base * (1 + j 2^-15), base ten times the other rows'
    scale and bf16-valued: equal after bf16 rounding (48 * 2^-15 stays under the
    half ulp, 2^-9 relative at least; a step of 2^-12 would leave it from j = 8),
    distinct in fp32. For a user with <u, base> > 0 they lead the list, the bf16
    pass keeps items 0..31 of them, and the fp32 order prefers the HIGHEST j."""
    uf, itf = (a.copy() for a in _tables(d))
    rng = np.random.default_rng(31 + d)
    base = _bf16(rng.uniform(-3.0, 3.0, d).astype(np.float32))
    j = np.arange(48, dtype=np.float64)[:, None]
    itf[:48] = (base.astype(np.float64) * (1.0 + j * 2.0 ** -15)).astype(np.float32)
    assert (_bf16(itf[:48]) == base).all() and np.unique(itf[:48], axis=0).shape[0] == 48
    return _frozen(uf, itf)


@pytest.mark.parametrize("d", WIDE)
def test_bf16_exact_near_ties_outside_the_candidates(d):
    uf, itf = _near_tie_tables(d)
    ptr, idx, _ = _exclusion()
    k, k_pre = 10, 32
    want = _want(ptr, idx, uf, itf, k)
    lead = (want[0] < 48).all(1) & (want[0] >= 0).all(1)
    beyond = lead & (want[0] >= 32).any(1)
    print(f"d={d}: {int(lead.sum())} users led by the near-tie group, "
          f"{int(beyond.sum())} with list entries the bf16 pass does not return")
    assert beyond.sum() >= 50
    bf = _rec(uf, itf, k_pre, precision="bf16")[0].cpu().numpy()
    for b in np.flatnonzero(beyond):                    # the candidates miss them
        assert not np.isin(want[0][b], bf[b]).all()
    info = _exact(uf, itf, k, k_pre, want)
    assert info["n_fallback"] > 0
    assert not info["certified"].cpu().numpy()[beyond].any()


# ---------------------------------------------------------------------------
# the flag and the norm bound
# ---------------------------------------------------------------------------
def _norm_max(t, d=None, ld=None):
    d = t.shape[1] if d is None else d
    out = torch.full((1,), -1.0, device=DEV)
    _lib.call("bbgr_row_norm_max", t.shape[0], d, t.data_ptr(), t.stride(0) if ld is None else ld,
              out.data_ptr(), _lib.stream_handle())
    return float(out)


def test_row_norm_max_is_a_tight_upper_bound():
    rng = np.random.default_rng(3)
    spread = (rng.uniform(1, 2, (777, 128)) * 2.0 ** rng.integers(-20, 21, (777, 1))
              ).astype(np.float32)
    cases = [_tables(64)[1], _tables(256)[1], _tables(8)[1], spread, _int_tables(128)[1],
             np.full((3, 256), 0.1, np.float32)]
    for a in cases:
        true = np.linalg.norm(a.astype(np.float64), axis=1).max()
        got = _norm_max(_t(a))
        assert true <= got <= true * (1 + 1e-5), (a.shape, true, got)
    # a row stride above d, rows past d not read as part of the row
    wide = _t(np.concatenate([cases[0], np.full((I, 4), 1e6, np.float32)], axis=1))
    true = np.linalg.norm(cases[0].astype(np.float64), axis=1).max()
    assert true <= _norm_max(wide, 64, 68) <= true * (1 + 1e-5)
    # twice the same bits; no rows: 0; a NaN stays
    assert _norm_max(_t(spread)) == _norm_max(_t(spread))
    assert _norm_max(torch.empty(0, 64, device=DEV)) == 0.0
    bad = cases[0].copy()
    bad[17, 3] = np.nan
    assert np.isnan(_norm_max(_t(bad)))


@pytest.mark.parametrize("d,k,k_pre", [(64, 10, 32), (64, 24, 32), (128, 30, 32), (256, 16, 32),
                                       (256, 100, 128), (64, 128, 128)])
def test_certified_flag_against_the_host_inequality(d, k, k_pre):
    """certified == (row not full) or s_k > t^ + E_u in float64, E_u = eps(d)
    ||u|| N_max with +-0.1 % slack (the device's norms are inflated by 2^-20
    and its underflow terms are below 2^-100)."""
    from bbgr.recommend import bf16_error_bound
    uf, itf = _tables(d)
    users = _users()
    cand, cand_score = (x.cpu().numpy() for x in _rec(uf, itf, k_pre, precision="bf16"))
    *_, info = _rec(uf, itf, k, precision="bf16_exact", prefilter_k=k_pre, return_info=True)
    cert = info["certified"].cpu().numpy()
    u64, i64 = uf.astype(np.float64), itf.astype(np.float64)
    e_u = bf16_error_bound(d) * np.linalg.norm(u64[users], axis=1) * np.linalg.norm(i64, axis=1).max()
    full = cand[:, -1] >= 0
    s = np.where(cand >= 0, np.einsum("bd,bjd->bj", u64[users], i64[np.maximum(cand, 0)]), -np.inf)
    s_k = -np.sort(-s, axis=1)[:, k - 1]
    t_hat = cand_score[:, -1].astype(np.float64)
    must = ~full | (s_k > t_hat + 1.001 * e_u)
    must_not = full & (s_k < t_hat + 0.999 * e_u)
    print(f"d={d} k={k} k_pre={k_pre}: certified {int(cert.sum())}, must {int(must.sum())}, "
          f"must not {int(must_not.sum())} of {users.size}")
    assert cert[must].all() and not cert[must_not].any()
    assert must.sum() + must_not.sum() >= users.size - 2
    assert must.any() and (k < 24 or must_not.any())


# ---------------------------------------------------------------------------
# pass-through and errors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 256])
def test_evaluate_ranking_bf16_exact_equals_fp32(d):
    from bbgr.recommend import evaluate_ranking
    *_, args = _eval_inputs(d)
    a = evaluate_ranking(*args, Ks=(10, 20), return_raw=True)
    b = evaluate_ranking(*args, Ks=(10, 20), return_raw=True, precision="bf16_exact")
    ar, br = a.pop("_raw"), b.pop("_raw")
    assert a == b
    assert torch.equal(ar["topk"], br["topk"])
    assert torch.equal(ar["topk_score"].view(torch.int32), br["topk_score"].view(torch.int32))
    c = evaluate_ranking(*args, Ks=(10, 20), precision="bf16")
    assert set(c) == set(a) and c[10]["users_eval"] == a[10]["users_eval"]


def test_trainer_recommend_bf16_exact():
    from bbgr.graph import BipartiteGraph
    from bbgr.synthetic import synthetic_credibility, synthetic_edges
    from bbgr.trainer import FusedTrainer
    e = synthetic_edges(U, 350, 4000, 17, items="zipf", duplicates=20)
    g = BipartiteGraph(e, U, 350, DEV, vertex_order="degree")
    tr = FusedTrainer(g, "v2_pop", cred=synthetic_credibility(U, 5), emb_dim=64, num_layers=2,
                      batch_size=64)
    tr.step()
    users = _t(_users(), torch.long)
    want = tr.recommend(users, 20, return_scores=True)
    topk, score, info = tr.recommend(users, 20, return_scores=True, precision="bf16_exact",
                                     return_info=True)
    assert torch.equal(topk, want[0])
    assert torch.equal(score.view(torch.int32), want[1].view(torch.int32))
    assert info["k_pre"] == 40
    print(f"trainer tables: fallback {info['n_fallback']} of {users.numel()}")
    approx = tr.recommend(users, 20, precision="bf16")
    assert approx.shape == topk.shape and approx.dtype == torch.int32


def test_bad_precision_and_prefilter_raise_and_the_device_stays_healthy():
    from bbgr.recommend import recommend
    uf, itf = _tables(64)
    users = _t(_users(), torch.long)
    with pytest.raises(ValueError, match="precision"):
        recommend(_t(uf), _t(itf), users, 10, precision="fp16")
    for bad in (9, 129, 0):
        with pytest.raises(ValueError, match="prefilter_k"):
            recommend(_t(uf), _t(itf), users, 10, precision="bf16_exact", prefilter_k=bad)
    with pytest.raises(ValueError, match="prefilter_k"):
        recommend(_t(uf), _t(itf), users, 10, precision="bf16", prefilter_k=32)
    with pytest.raises(ValueError, match="k must be"):
        recommend(_t(uf), _t(itf), users, 129, precision="bf16_exact")
    empty = recommend(_t(uf), _t(itf), [], 10, precision="bf16_exact", return_info=True)
    assert empty[0].shape == (0, 10) and empty[1]["n_fallback"] == 0
    got = _rec(uf, itf, 10, precision="bf16_exact")
    torch.cuda.synchronize()
    _check(got, _oracle(64), 10)
