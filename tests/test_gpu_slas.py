"""GPU: the SLAS subgraph sampler and the credibility training loop
(bbgr.cred_train, csrc/slas.hip) against the host restatement tests/slas_ref.py
(main.py:727-883), exact successive-sampling probabilities, and
oracle.ref_torch.CredModelRef."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slas_ref as SR  # noqa: E402

DEV = "cuda"
A = 5          # edge attribute columns (EDGE_ATTR_KEYS), timestamp_norm = column 3
TS = 3
SPLIT = 0.5


def _graph(e, ea, user_x, user_y, item_x):
    from bbgr.cred_train import SlasGraph
    return SlasGraph(e, ea, user_x, user_y, item_x, DEV)


def _attrs(rng, E):
    ea = rng.uniform(-0.5, 1.5, (E, A)).astype(np.float32)
    ea[:, TS] = rng.uniform(0, 1, E).astype(np.float32)
    ea[rng.integers(0, max(E, 1), E // 10), TS] = SPLIT     # exactly at the split: late
    return ea


def _close(got, want, what, tol):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want, np.float64)
    err = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    amax = np.abs(got - want).max() if want.size else 0.0
    print(f"{what}: normwise {err:.3e} max-abs {amax:.3e}")
    assert err <= tol and amax <= tol * max(np.abs(want).max(), 1e-30), (what, err, amax)


# -- profiles ------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 5])
def test_profiles_vs_float64(F):
    from bbgr._lib import call, ptr, stream_handle
    U, I, E = 700, 300, 9000
    rng = np.random.default_rng(10 + F)
    src = rng.integers(0, U - 1, E - 3000 - 20 - 1)         # user U-1 stays isolated
    dst = rng.integers(0, I, src.size)
    src[src == 11] = 12
    src = np.concatenate([src, np.full(3000, 5), src[:20]])  # a 3000-edge hub, duplicate edges
    dst = np.concatenate([dst, rng.integers(0, I, 3000), dst[:20]])
    item_x = rng.normal(size=(I, F)).astype(np.float32)
    item_x[7] = 0.0                                          # a zero feature row
    src = np.concatenate([src, [11]])                        # a user whose only item is that row
    dst = np.concatenate([dst, [7]])
    if F == 1:
        # item_norm is +-1 here, and a user whose signs cancel has a mean of exactly 0 in
        # fp32 but of ~1e-12 in float64, which l2n then blows up to order 1: such a row has
        # no reference. One edge of each such user is turned to the zero item instead.
        sign = np.sign(item_x[:, 0]).astype(np.int64)
        for u in np.flatnonzero((np.bincount(src, sign[dst], U) == 0)
                                & (np.bincount(src, np.abs(sign[dst]), U) > 0)):
            j = np.flatnonzero((src == u) & (dst != 7))[-1]
            dst[j] = 7
        assert not ((np.bincount(src, sign[dst], U) == 0)
                    & (np.bincount(src, np.abs(sign[dst]), U) > 0)).any()
    e = np.stack([src, dst])
    assert e.shape[1] == E
    g = _graph(e, _attrs(rng, e.shape[1]), rng.normal(size=(U, 4)), rng.integers(-1, 2, U), item_x)
    want_in, want_mu = SR.profiles64(e, item_x, U)
    _close(g.item_norm[:I], want_in, "item_norm", 1e-5)
    _close(g.user_mu[:U], want_mu, "user_mu", 1e-5)
    assert g.item_norm[7].abs().sum().item() == 0 and g.user_mu[U - 1].abs().sum().item() == 0
    assert g.user_mu[11].abs().sum().item() == 0
    a, b = torch.empty_like(g.item_norm), torch.empty_like(g.user_mu)
    call("bbgr_slas_profiles", U, I, F, ptr(g.item_x), F, ptr(g.u_csr.indptr), ptr(g.u_csr.nbr),
         ptr(a), ptr(b), stream_handle())
    assert torch.equal(a, g.item_norm) and torch.equal(b, g.user_mu)      # fixed order


# -- row invariants --------------------------------------------------------------------
def _lengths(k):
    """(1024 | 1025: the last one-wave row and the first workgroup row.)"""
    return sorted({0, 1, k - 1, k, k + 1, 63, 64, 65, 129, 300, 1024, 1025, 5000})


def _invariant_graph(k):
    """Group A: user j has L[j] early edges (rows emptied by the late view).
    Group B: user has L[j] late edges, a tenth of them exactly at the split,
    and 3 early ones. Items repeat within a row (duplicate edges)."""
    rng = np.random.default_rng(k)
    L = _lengths(k)
    I = 400
    src, ts = [], []
    for j, n in enumerate(L):
        src += [j] * n
        ts += list(rng.uniform(0.0, 0.49, n))
        late = rng.uniform(0.5, 1.0, n)
        late[: (n + 9) // 10] = SPLIT
        src += [len(L) + j] * (n + 3)
        ts += list(late) + [0.1, 0.2, 0.3]
    src = np.array(src, np.int64)
    order = rng.permutation(src.size)                       # row order = edge id order, mixed
    src, ts = src[order], np.array(ts, np.float32)[order]
    dst = rng.integers(0, I, src.size)
    ea = rng.uniform(0, 1, (src.size, A)).astype(np.float32)
    ea[:, TS] = ts
    U = 2 * len(L)
    e = np.stack([src, dst])
    g = _graph(e, ea, rng.normal(size=(U, 3)), rng.integers(-1, 2, U),
               rng.normal(size=(I, 2)).astype(np.float32))
    return g, e, ts, U


@pytest.mark.parametrize("k", [1, 15, 32, 64])
def test_sample_row_invariants(k):
    g, e, ts, U = _invariant_graph(k)
    ptr_, nbr, eid = SR.csr_from_src(e[0], e[1], U)
    rows = torch.arange(U, device=DEV)
    for view in (None, "early", "late"):
        o_nbr, o_eid, o_cnt = (t.cpu().numpy() for t in g.sample(
            rows, "user", k, temporal_view=view, split=SPLIT, seed=1, counter=5, stage=0))
        seen = set()
        for u in range(U):
            sl = slice(ptr_[u], ptr_[u + 1])
            ok = (np.ones(sl.stop - sl.start, bool) if view is None else
                  ts[eid[sl]] < SPLIT if view == "early" else ts[eid[sl]] >= SPLIT)
            el_nbr, el_eid = nbr[sl][ok], eid[sl][ok]
            m = el_eid.size
            seen.add(m)
            c = o_cnt[u]
            assert c == min(m, k), (view, u, m, c)
            assert (o_nbr[u, c:] == -1).all() and (o_eid[u, c:] == -1).all()
            if m <= k:
                np.testing.assert_array_equal(o_eid[u, :c], el_eid)
                np.testing.assert_array_equal(o_nbr[u, :c], el_nbr)
            else:
                assert len(set(o_eid[u].tolist())) == k                     # no edge twice
                assert set(o_eid[u].tolist()) <= set(el_eid.tolist())       # eligible, this row
                np.testing.assert_array_equal(o_nbr[u], e[1][o_eid[u]])     # its neighbour
        assert set(_lengths(k)) <= seen, (view, sorted(seen))
        if view == "late":
            assert 0 in seen                                                # emptied by the view
    # a row's picks: a pure function of (seed, counter, stage, row)
    full = g.sample(rows, "user", k, temporal_view="late", seed=1, counter=5, stage=0)
    some = torch.tensor([U - 1, 3, U - 2, 0, len(_lengths(k)) + 2], device=DEV)
    part = g.sample(some, "user", k, temporal_view="late", seed=1, counter=5, stage=0)
    for a, b in zip(full, part):
        assert torch.equal(a[some], b)
    other = g.sample(rows, "user", k, temporal_view="late", seed=1, counter=6, stage=0)
    assert not torch.equal(other[1][U - 1], full[1][U - 1])                 # the 5000-edge row
    stage1 = g.sample(rows, "user", k, temporal_view="late", seed=1, counter=5, stage=1)
    assert not torch.equal(stage1[1][U - 1], full[1][U - 1])


@pytest.mark.parametrize("k", [1, 15, 64])
def test_workgroup_rows_pick_what_one_wave_picks(k):
    """A row above 1024 slots is dealt out to 16 waves. Its keys depend on
    (seed, counter, stage, row, slot position) and the weight alone, so with
    equal item features the 5000-slot row under a view that keeps its first
    1024 slots must pick exactly what the same row cut to those 1024 slots
    (one wave) picks."""
    rng = np.random.default_rng(k)
    n, cut, I = 5000, 1024, 50
    e = np.stack([np.zeros(n, np.int64), rng.integers(0, I, n)])
    ea = np.zeros((n, A), np.float32)
    ea[:cut, TS], ea[cut:, TS] = 0.1, 0.9
    item_x = np.tile(np.array([[1.0, 0.0]], np.float32), (I, 1))   # both profiles exact
    rest = (np.zeros((1, 2)), np.array([1]), item_x)
    long_g, short_g = _graph(e, ea, *rest), _graph(e[:, :cut], ea[:cut], *rest)
    row = torch.zeros(1, dtype=torch.int64, device=DEV)
    kw = dict(seed=9, counter=4, stage=0)
    a = long_g.sample(row, "user", k, temporal_view="early", split=SPLIT, **kw)
    b = short_g.sample(row, "user", k, **kw)
    assert int(a[2]) == k
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# -- distribution ------------------------------------------------------------------------
N_ROWS = 16384


def _chi2_bound(df):
    from scipy.stats import chi2
    return chi2.ppf(1 - 1e-6, df)


def _pair_chi2(picks, w):
    """Pearson chi^2 of the ordered (first, second) pick counts of 6 neighbours
    against successive sampling p_a p_b / (1 - p_a)."""
    p = w / w.sum()
    n = picks.shape[0]
    stat, cells = 0.0, 0
    for a in range(6):
        for b in range(6):
            if a == b:
                continue
            exp = n * p[a] * p[b] / (1 - p[a])
            assert exp >= 20, (a, b, exp)
            obs = np.count_nonzero((picks[:, 0] == a) & (picks[:, 1] == b))
            stat += (obs - exp) ** 2 / exp
            cells += 1
    assert cells == 30
    return stat


def _angles(deg):
    t = np.deg2rad(np.asarray(deg, np.float64))
    return np.stack([np.cos(t), np.sin(t)], 1).astype(np.float32)


def test_distribution_items_for_user():
    """(a) 16384 users wired to the same 6 items; weights span a ratio of ~7."""
    item_x = _angles([-70, -40, -10, 10, 40, 70])
    e = np.stack([np.repeat(np.arange(N_ROWS), 6), np.tile(np.arange(6), N_ROWS)])
    rng = np.random.default_rng(0)
    g = _graph(e, _attrs(rng, e.shape[1]), np.zeros((N_ROWS, 2)), np.full(N_ROWS, -1), item_x)
    nbr, _, cnt = g.sample(torch.arange(N_ROWS, device=DEV), "user", 2, seed=42, counter=0)
    assert (cnt == 2).all()
    inorm, mu = SR.profiles64(e, item_x, N_ROWS)
    w = np.exp(3.0 * inorm @ mu[0])
    assert 6 < w.max() / w.min() < 8
    stat = _pair_chi2(nbr.cpu().numpy(), w)
    print("chi2 (items for user, df 29):", stat)
    assert stat < _chi2_bound(29)


def test_distribution_users_for_item_with_labels():
    """(b) 16384 items wired to the same 6 users, three of them labeled (x2);
    each user's profile is turned by an anchor item of its own."""
    n = N_ROWS
    anchors = [100, -60, 20, -100, 60, -20]
    item_x = np.concatenate([np.tile(_angles([0]), (n, 1)), _angles(anchors)])
    src = np.concatenate([np.tile(np.arange(6), n), np.repeat(np.arange(6), n)])
    dst = np.concatenate([np.repeat(np.arange(n), 6), n + np.repeat(np.arange(6), n)])
    e = np.stack([src, dst])
    y = np.array([1, -1, 0, -1, 1, -1])
    rng = np.random.default_rng(1)
    g = _graph(e, _attrs(rng, e.shape[1]), np.zeros((6, 2)), y, item_x)
    nbr, _, cnt = g.sample(torch.arange(n, device=DEV), "item", 2, upweight=1.0, seed=42,
                           counter=1, stage=1)
    assert (cnt == 2).all()
    inorm, mu = SR.profiles64(e, item_x, 6)
    w = np.exp(3.0 * mu @ inorm[0]) * np.where(y >= 0, 2.0, 1.0)
    stat = _pair_chi2(nbr.cpu().numpy(), w)
    print("chi2 (users for item, df 29):", stat)
    assert stat < _chi2_bound(29)
    # the check has power: without the label factor the same counts miss the same bound
    assert _pair_chi2(nbr.cpu().numpy(), np.exp(3.0 * mu @ inorm[0])) > _chi2_bound(29)


def test_distribution_across_chunks():
    """(c) 70 eligible neighbours (more than one 64-slot chunk), k = 15."""
    from scipy.stats import norm
    m, k, n = 70, 15, N_ROWS
    item_x = _angles(np.linspace(-70, 70, m))
    e = np.stack([np.repeat(np.arange(n), m), np.tile(np.arange(m), n)])
    ea = np.zeros((e.shape[1], A), np.float32)
    g = _graph(e, ea, np.zeros((n, 2)), np.full(n, -1), item_x)
    rows = torch.arange(n, device=DEV)
    nbr, _, cnt = g.sample(rows, "user", k, seed=42, counter=2)
    assert (cnt == k).all()
    inorm, mu = SR.profiles64(e, item_x, n)
    w = np.exp(3.0 * inorm @ mu[0])
    exp = n * w / w.sum()
    assert exp.min() >= 20
    obs = np.bincount(nbr[:, 0].cpu().numpy(), minlength=m)
    stat = float(((obs - exp) ** 2 / exp).sum())
    print("chi2 (position 0, df 69):", stat)
    assert stat < _chi2_bound(69)
    # equal weights (kappa = 0): every neighbour is included k/m of the time
    nbr0, _, _ = g.sample(rows, "user", k, kappa=0.0, seed=42, counter=3)
    c = np.bincount(nbr0.cpu().numpy().ravel(), minlength=m)
    z = norm.ppf(1 - (1e-6 / m) / 2)
    dev = np.abs(c - n * k / m) / np.sqrt(n * (k / m) * (1 - k / m))
    print("inclusion |z| max:", dev.max(), "bound", z)
    assert (dev <= z).all(), dev


# -- structure ---------------------------------------------------------------------------
def _random_graph(seed, U=600, I=200, E=5000):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, U - 1, E - 200)                    # user U-1 has no edges
    src = np.concatenate([src, rng.integers(0, 4, 200)])     # four users with ~50 more edges
    dst = np.minimum(rng.zipf(1.3, src.size) - 1, I - 1)
    src = np.concatenate([src, src[:30]])                    # duplicate edges
    dst = np.concatenate([dst, dst[:30]])
    e = np.stack([src, dst]).astype(np.int64)
    ea = _attrs(rng, e.shape[1])
    user_x = rng.normal(size=(U, 6)).astype(np.float32)
    user_y = np.where(rng.uniform(size=U) < 0.6, rng.integers(0, 2, U), -1)
    item_x = rng.normal(size=(I, 2)).astype(np.float32)
    return e, ea, user_x, user_y, item_x


@pytest.fixture(scope="module")
def random_graph():
    data = _random_graph(21)
    return data, _graph(*data)


def _same_dict(got, want):
    assert set(got) == set(want)
    assert got["bs"] == want["bs"]
    for key in ("users_global", "items_global"):
        assert got[key].dtype == torch.int64
        np.testing.assert_array_equal(got[key].cpu().numpy(), want[key])
    for key in ("x_u", "y_u", "x_i", "e_u2i", "ea_u2i", "e_i2u", "ea_i2u"):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert torch.equal(got[key].cpu(), want[key]), key      # bit for bit


@pytest.mark.parametrize("view", [None, "early", "late"])
@pytest.mark.parametrize("bs", [1, 7, 256])
def test_structure_given_the_picks(random_graph, view, bs):
    data, g = random_graph
    U = data[2].shape[0]
    rng = np.random.default_rng(bs)
    seeds = rng.permutation(U - 1)[:bs].astype(np.int64)
    if bs > 1:
        seeds[1] = U - 1                                      # a seed with no edges
    got = g.build_subgraph(seeds, view, counter=bs)
    picks = g.last_picks
    host = SR.HostSlas(*data, ts_idx=TS, pick=SR.picks_from_device(picks, seeds))
    want = host.build_subgraph(seeds, view)
    _same_dict(got, want)
    if bs == 256:
        # some seeds were also drawn as neighbours of the sampled items
        drawn = set(picks["users"][0].cpu().numpy().ravel().tolist())
        assert drawn & set(seeds.tolist())
        assert got["users_global"].numel() > bs and got["e_u2i"].shape[1] > 0
    # the set tables are clean again, and a second call is unaffected
    assert not g._mask_u.any() and not g._mask_i.any() and (g._item_local == -1).all()
    again = g.build_subgraph(seeds, view, counter=bs)
    for key in got:
        assert got[key] == again[key] if key == "bs" else torch.equal(got[key], again[key]), key


def test_no_edge_survives(random_graph):
    data, g = random_graph
    U = data[2].shape[0]
    got = g.build_subgraph(np.array([U - 1]), "early", counter=0)
    want = SR.HostSlas(*data, ts_idx=TS).build_subgraph(np.array([U - 1]), "early")
    _same_dict(got, want)
    assert got["e_u2i"].shape == (2, 0) and got["ea_u2i"].shape == (0, A)
    assert got["e_i2u"].shape == (2, 0) and got["items_global"].numel() == 0
    with pytest.raises(ValueError, match="temporal_view"):
        g.build_subgraph(np.array([0]), "middle", counter=0)


def _capped_graph(seed, U=600, I=200, cap=15):
    """Every user and every item has at most `cap` edges: E = I * cap = 3000,
    the most this shape admits."""
    rng = np.random.default_rng(seed)
    dst = np.repeat(np.arange(I), cap)
    src = np.concatenate([rng.permutation(U)[:cap] for _ in range(I)])
    keep = np.ones(src.size, bool)
    deg = np.zeros(U, int)
    for j, u in enumerate(src):
        deg[u] += 1
        keep[j] = deg[u] <= cap
    order = rng.permutation(int(keep.sum()))
    e = np.stack([src[keep], dst[keep]])[:, order].astype(np.int64)
    ea = _attrs(rng, e.shape[1])
    user_x = rng.normal(size=(U, 6)).astype(np.float32)
    user_y = np.where(rng.uniform(size=U) < 0.6, rng.integers(0, 2, U), -1)
    item_x = rng.normal(size=(I, 2)).astype(np.float32)
    return e, ea, user_x, user_y, item_x


@pytest.fixture(scope="module")
def capped_graph():
    data = _capped_graph(33)
    e = data[0]
    assert np.bincount(e[0]).max() <= 15 and np.bincount(e[1]).max() <= 15
    return data, _graph(*data)


@pytest.mark.parametrize("view", [None, "early", "late"])
def test_deterministic_graph_end_to_end(capped_graph, view):
    """Maximum degree <= k: no draw is made, the dictionary equals the
    unmodified host loop."""
    data, g = capped_graph
    seeds = np.random.default_rng(4).permutation(600)[:128].astype(np.int64)
    _same_dict(g.build_subgraph(seeds, view, counter=9), SR.HostSlas(*data, ts_idx=TS)
               .build_subgraph(seeds, view))


# -- training ----------------------------------------------------------------------------
def test_first_step_vs_torch_reference(capped_graph):
    """U = 600, I = 200, hidden 64, batch 128, ~60 % labeled, maximum degree
    <= 15 (so E = 3000: I * 15 is the most such a graph holds). Loss and
    gradients of the first step against CredModelRef on the CPU over the
    host-built subgraphs, same weights: forward 2e-5, gradients 1e-4."""
    import torch.nn.functional as F
    from bbgr.cred_gnn import CredModel
    from bbgr.cred_train import HostPlan, step_loss
    from oracle.ref_torch import CredModelRef
    data, g = capped_graph
    torch.manual_seed(0)
    ref = CredModelRef(6, 2, 64)
    dev = CredModel(6, 2, 64).to(DEV)
    dev.load_state_dict({k: v.to(DEV) for k, v in ref.state_dict().items()})
    batch = HostPlan(data[3], 42).epoch_batches(128)[0]
    assert batch.size == 128
    loss_d = step_loss(dev, g.build_subgraph(batch, "early", counter=0),
                       g.build_subgraph(batch, "late", counter=1))
    loss_d.backward()

    host = SR.HostSlas(*data, ts_idx=TS)
    g1, g2 = host.build_subgraph(batch, "early"), host.build_subgraph(batch, "late")
    p1, hu1, hi1, w1 = ref.forward_subgraph(g1["x_u"], g1["x_i"], g1["e_u2i"], g1["ea_u2i"],
                                            g1["e_i2u"], g1["ea_i2u"])
    _, hu2, _, _ = ref.forward_subgraph(g2["x_u"], g2["x_i"], g2["e_u2i"], g2["ea_u2i"],
                                        g2["e_i2u"], g2["ea_i2u"])
    bs = 128
    y = g1["y_u"][:bs]
    keep = y >= 0
    assert keep.all()                                          # train users are labeled
    sup = F.binary_cross_entropy(p1[:bs][keep], y[keep].float())
    mask = w1 > 0.0
    diff = hu1[g1["e_u2i"][0][mask]] - hi1[g1["e_u2i"][1][mask]]
    smooth = (w1[mask] * diff.pow(2).sum(-1)).mean()
    z1 = hu1[:bs] / (hu1[:bs].norm(dim=-1, keepdim=True) + 1e-12)
    z2 = hu2[:bs] / (hu2[:bs].norm(dim=-1, keepdim=True) + 1e-12)
    cont = F.cross_entropy((z1 @ z2.t()) / 0.2, torch.arange(bs))
    loss_r = sup + 0.1 * smooth + 0.1 * cont
    loss_r.backward()
    _close(loss_d.reshape(1), loss_r.detach().numpy().reshape(1), "loss", 2e-5)
    for (n, p_r), (_, p_d) in zip(ref.named_parameters(), dev.named_parameters()):
        _close(p_d.grad, p_r.grad.numpy(), f"grad {n}", 1e-4)


def test_train_and_export(capped_graph, tmp_path):
    from bbgr import ingest
    from bbgr.cred_train import train_and_export_credibility
    from bbgr.lightgcn_cu_pop import build_message_passing_mats
    data, g = capped_graph
    U, I = 600, 200
    out = train_and_export_credibility(g, hidden_dim=64, epochs=2, batch_size=128, out_dir=tmp_path)
    assert len(out["losses"]) == 2 and np.isfinite(out["losses"]).all()
    cred = out["cred"]
    assert cred.shape == (U,) and cred.dtype == np.float32 and np.isfinite(out["cred_raw"]).all()
    assert cred.min() == 0.0 and cred.max() == 1.0
    assert set(out["model"].state_dict()) == {f"{m}.{p}" for m in (
        "user_proj", "item_proj", "item_upd", "user_upd", "out") for p in ("weight", "bias")}
    again = train_and_export_credibility(g, hidden_dim=64, epochs=2, batch_size=128)
    assert np.array_equal(out["cred_raw"], again["cred_raw"])              # bit for bit
    assert out["losses"] == again["losses"]
    c_npy = ingest.load_credibility_npy(tmp_path / "credibility_scores_minmax.npy", U)
    np.testing.assert_array_equal(c_npy, cred)
    c_csv = ingest.load_credibility_csv(tmp_path / "credibility_scores_minmax_with_user_id.csv", U)
    assert np.abs(c_csv - cred).max() <= 5.1e-7                            # the %.6f of the file
    assert set(torch.load(tmp_path / "cred_model.pt")) == set(out["model"].state_dict())
    M_ui, M_iu = build_message_passing_mats(data[0], U, I, torch.from_numpy(c_npy), DEV)
    assert M_ui is not None and M_iu is not None
