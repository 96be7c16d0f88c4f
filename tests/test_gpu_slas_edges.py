"""GPU: the SLAS sampler's picks against the keys restated on the host
(tests/slas_ref.py: Philox4x32-10, -log(U) / w in float64), bbgr_slas_induce
called directly at the tile boundaries of its scan, and bbgr_slas_profiles at
its feature-width dispatch edges with a padded leading dimension.

bbgr.h promises, for a row with more than k eligible slots: the k smallest keys
win, in ascending key order, equal keys the lower slot first; U_j the first
Philox word at counter {counter, stage, row id, slot position in the full
row}, key = seed. test_gpu_slas.py checks that in law and in structure; here
every pick is checked against the host's keys."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import slas_ref as SR  # noqa: E402

DEV = "cuda"
A, TS, SPLIT = 5, 3, 0.5
VIEWS = (None, "early", "late")
KS = (1, 15, 64)
# k + 1 for every k, the 64-slot chunk and its neighbours, the 1024 | 1025 kernel
# boundary, 1089 = 17 chunks + 1 (a second chunk for wave 0 of a workgroup row
# only), 2049 (two full rounds of the 16 waves + 1), 5000 and 20000 (5 and 20
# chunks per wave).
LENGTHS = sorted({k + 1 for k in KS} | {65, 127, 128, 129, 300, 1023, 1024, 1025, 1089, 2049,
                                       5000, 20000})
U24_09 = int(np.ceil(0.9 * 2 ** 24))
# (seed, counter) of the exact-order test: the result of a host search over the
# counters 0 .. 5999 at seed 42 with slas_ref.slas_u24 for qualifying rows with an
# exact u24 tie inside their first k picks on both sides and one whose tie
# straddles the picks k and k + 1 (35 counters had both).
# test_exact_order_meets_exact_ties asserts it of these inputs.
EXACT_SEED, EXACT_COUNTER = 42, 4079
EXACT_TIES_AT_K = [("user", 15, "late", 12)]                 # the 5000-slot user row


def edge_graph(F=2, lengths=LENGTHS, fill=600, seed=0):
    """User j < len(lengths) has lengths[j] edges to `fill` filler items (so
    items repeat within the row), item j has lengths[j] edges from `fill` filler
    users; the input order is shuffled, ~40 % of every row is early, a tenth of
    the late edges sit exactly at the split, about half the users are labelled.
    Pure numpy (the host search for EXACT_COUNTER builds the same graph)."""
    rng = np.random.default_rng(seed)
    n = len(lengths)
    src, dst = [], []
    for j, m in enumerate(lengths):
        src.append(np.full(m, j))
        dst.append(rng.integers(n, n + fill, m))
        src.append(rng.integers(n, n + fill, m))
        dst.append(np.full(m, j))
    src, dst = np.concatenate(src), np.concatenate(dst)
    order = rng.permutation(src.size)                       # row order != input order
    e = np.stack([src[order], dst[order]]).astype(np.int64)
    E = e.shape[1]
    early = rng.uniform(size=E) < 0.4
    ts = np.where(early, rng.uniform(0.0, 0.49, E), rng.uniform(0.5, 1.0, E)).astype(np.float32)
    ts[~early & (rng.uniform(size=E) < 0.1)] = SPLIT        # exactly at the split: late
    ea = rng.uniform(0, 1, (E, A)).astype(np.float32)
    ea[:, TS] = ts
    U = I = n + fill
    user_y = np.where(rng.uniform(size=U) < 0.5, rng.integers(0, 2, U), -1)
    item_x = rng.normal(size=(I, F)).astype(np.float32)
    return e, ea, rng.normal(size=(U, 3)).astype(np.float32), user_y, item_x


class HostSide:
    """One direction of the graph as the sampler sees it: the reference-order
    CSR, (row, position) per slot, and the float64 dot products of the
    device's own fp32 profiles."""

    def __init__(self, side, e, ea, user_y, item_norm, user_mu):
        src, dst = (e[0], e[1]) if side == "user" else (e[1], e[0])
        rp, npf = (user_mu, item_norm) if side == "user" else (item_norm, user_mu)
        self.side, self.n_rows = side, rp.shape[0]
        self.ptr, self.nbr, self.eid = SR.csr_from_src(src, dst, self.n_rows)
        self.row, self.pos = SR.slot_rows(self.ptr)
        self.slot_of_eid = np.empty(e.shape[1], np.int64)
        self.slot_of_eid[self.eid] = np.arange(e.shape[1])
        self.ts = ea[self.eid, TS]
        rp, npf = np.asarray(rp, np.float64), np.asarray(npf, np.float64)
        self.dot = (npf[self.nbr] * rp[self.row]).sum(-1)
        self.labels = user_y[self.nbr] if side == "item" else None
        self.stage = 0 if side == "user" else 1

    def eligible(self, view):
        if view is None:
            return np.ones(self.ts.size, bool)
        return self.ts < SPLIT if view == "early" else self.ts >= SPLIT

    def u24(self, seed, counter, stage=None, pos=None):
        return SR.slas_u24(seed, counter, self.stage if stage is None else stage, self.row,
                           self.pos if pos is None else pos)

    def rank_positions(self, view):
        """The mutant of the power check: a slot's rank among the eligible slots
        of its row in place of its position in the full row."""
        ok = self.eligible(view)
        c = np.cumsum(ok) - ok
        return c - c[self.ptr[self.row]]

    def rows(self):
        return range(self.n_rows)

    def sl(self, r):
        return slice(self.ptr[r], self.ptr[r + 1])


def _close(got, want, what, tol):
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, np.float64)
    err = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    amax = np.abs(got - want).max()
    print(f"{what}: normwise {err:.3e} max-abs {amax:.3e}")
    assert err <= tol and amax <= tol * max(np.abs(want).max(), 1e-30), (what, err, amax)


def _graph(data):
    from bbgr.cred_train import SlasGraph
    return SlasGraph(*data, DEV)


def _sides(data, g):
    e, ea, _, user_y, _ = data
    inorm, mu = g.item_norm.cpu().numpy(), g.user_mu.cpu().numpy()
    return {s: HostSide(s, e, ea, user_y, inorm, mu) for s in ("user", "item")}


@pytest.fixture(scope="module")
def graph():
    data = edge_graph()
    g = _graph(data)
    return g, _sides(data, g)


def _sample(g, h, k, rows=None, **kw):
    rows = torch.arange(h.n_rows, device=DEV) if rows is None else rows
    kw.setdefault("stage", h.stage)
    return tuple(t.cpu().numpy() for t in g.sample(rows, h.side, k, split=SPLIT, **kw))


def check_side(h, k, view, out, keys, u24, w, delta):
    """Every row of one sample call over all rows: the count, the -1 padding, the
    neighbour of every pick; rows of at most k eligible slots in row order,
    the others through check_picks. Returns (rows drawn, largest inversion)."""
    o_nbr, o_eid, o_cnt = out
    ok = h.eligible(view)
    drawn, worst = 0, 0.0
    for j, r in enumerate(h.rows()):
        sl = h.sl(r)
        el = np.flatnonzero(ok[sl])
        c = o_cnt[j]
        assert c == min(el.size, k), (h.side, view, r, el.size, c)
        assert (o_nbr[j, c:] == -1).all() and (o_eid[j, c:] == -1).all()
        if c == 0:
            continue
        slots = h.slot_of_eid[o_eid[j, :c]]
        assert ((slots >= sl.start) & (slots < sl.stop)).all(), (h.side, view, r)   # this row's
        np.testing.assert_array_equal(o_nbr[j, :c], h.nbr[slots])
        if el.size <= k:
            np.testing.assert_array_equal(slots - sl.start, el)
            continue
        try:
            inv = SR.check_picks(keys[sl], ok[sl], slots - sl.start, delta, u24[sl], w[sl])
        except AssertionError as err:
            raise AssertionError((h.side, view, "row", r, "slots", sl.stop - sl.start, "k", k,
                                  *err.args)) from None
        drawn, worst = drawn + 1, max(worst, inv)
    return drawn, worst


# -- a. integer-exact order at kappa = 0 -----------------------------------------------
def exact_rows(h, k, view, u24):
    """{row: the expected positions} for the rows whose (k+1)-th largest
    eligible U is at least 0.9: there neighbouring distinct U differ by at least
    8 ulp of the key -logf(U) < 0.125, so logf (3 ulp) can neither reorder nor
    merge them and the picks are the host's sort by (u24 descending, position
    ascending) with no tolerance. Also the rows with an exact u24 tie inside
    the first k picks, and those whose tie straddles the picks k and k + 1."""
    ok = h.eligible(view)
    want, tie_in, tie_at = {}, [], []
    for r in h.rows():
        sl = h.sl(r)
        el = np.flatnonzero(ok[sl])
        if el.size <= k:
            continue
        u = u24[sl][el]
        order = np.lexsort((el, -u))
        top = u[order[:k + 1]]
        if top[k] < U24_09:
            continue
        want[r] = el[order[:k]]
        if (top[1:k] == top[:k - 1]).any():
            tie_in.append(r)
        if top[k] == top[k - 1]:
            tie_at.append(r)
    return want, tie_in, tie_at


def exact_need(k, view):
    """The row lengths the exact-order claim must cover (whatever else
    qualifies by chance). Under a view ~40 % (early) / ~60 % (late) of a row is
    eligible, and k + 1 of those must lie above 0.9."""
    at_least = {(1, False): 127, (15, False): 1023, (64, False): 1024,
                (1, True): 300, (15, True): 1023, (64, True): 5000}[k, view is not None]
    need = {m for m in LENGTHS if m >= at_least}
    return need | {300} if (k, view) == (15, None) else need


def exact_cases(sides, seed, counter, ks=KS):
    out = {}
    for side, h in sides.items():
        u24 = h.u24(seed, counter)
        for k in ks:
            for view in VIEWS:
                out[side, k, view] = exact_rows(h, k, view, u24)
    return out


@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("k", KS)
def test_exact_order(graph, side, k):
    """kappa = 0: every weight is exactly 1, the device key is -logf(U)."""
    g, sides = graph
    h = sides[side]
    u24 = h.u24(EXACT_SEED, EXACT_COUNTER)
    length = np.diff(h.ptr)
    for view in VIEWS:
        want, tie_in, tie_at = exact_rows(h, k, view, u24)
        have = {int(length[r]) for r in want}
        need = exact_need(k, view)
        assert need <= have, (side, k, view, sorted(need - have))
        o_nbr, o_eid, o_cnt = _sample(g, h, k, kappa=0.0, temporal_view=view, seed=EXACT_SEED,
                                      counter=EXACT_COUNTER)
        for r, pos in want.items():
            assert o_cnt[r] == k
            got = h.slot_of_eid[o_eid[r]] - h.ptr[r]          # position in the FULL row
            np.testing.assert_array_equal(got, pos, err_msg=f"{side} row {r} ({length[r]} slots) "
                                          f"k={k} view={view}")
            np.testing.assert_array_equal(o_nbr[r], h.nbr[h.ptr[r] + pos])
        print(f"exact order {side} k={k} view={view}: {len(want)} rows, lengths {sorted(have)}, "
              f"ties inside {tie_in}, at k|k+1 {tie_at}")


def test_exact_order_meets_exact_ties(graph):
    """The (seed, counter) of test_exact_order was chosen so that qualifying
    rows hold an exact u24 tie inside their first k picks, and one whose tie
    straddles the picks k and k + 1 (the tie rule decides which slot is in)."""
    _, sides = graph
    cases = exact_cases(sides, EXACT_SEED, EXACT_COUNTER)
    inside = sorted((s, k, str(v), r) for (s, k, v), (_, ti, _) in cases.items() for r in ti)
    at_k = sorted((s, k, str(v), r) for (s, k, v), (_, _, ta) in cases.items() for r in ta)
    print("ties inside the first k picks:", inside)
    print("ties at picks k | k + 1:", at_k)
    assert {(s, k) for s, k, _, _ in inside} >= {("user", 64), ("item", 15), ("item", 64)}
    assert at_k == EXACT_TIES_AT_K


# -- b. weighted picks at kappa = 3 --------------------------------------------------
def _weighted(h, view, seed, counter, kappa, upweight, stage=None, pos=None, labels=True):
    u24 = h.u24(seed, counter, stage, pos)
    lab = h.labels if (labels and upweight is not None) else None
    w = SR.slas_weights64(h.dot, kappa, lab, upweight or 0.0)
    return SR.slas_keys64(u24, w, h.eligible(view)), u24, w


def _rejected_somewhere(h, k, view, out, keys, u24, w, delta):
    try:
        check_side(h, k, view, out, keys, u24, w, delta)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("k", KS)
def test_weighted_picks(graph, k):
    """Every row of the graph against the float64 keys at the derived delta:
    user rows under the three views, item rows with the label factor (one-wave
    rows, 16-wave rows, rows where a wave scans several chunks)."""
    g, sides = graph
    delta = SR.pick_delta(2, 3.0)
    worst = 0.0
    h = sides["user"]
    for view in VIEWS:
        out = _sample(g, h, k, kappa=3.0, temporal_view=view, seed=42, counter=7)
        keys, u24, w = _weighted(h, view, 42, 7, 3.0, None)
        drawn, inv = check_side(h, k, view, out, keys, u24, w, delta)
        assert drawn >= 8
        worst = max(worst, inv)
        if view is not None:
            # power: the slot position is the one in the full row, not the rank among
            # the eligible slots
            bad = _weighted(h, view, 42, 7, 3.0, None, pos=h.rank_positions(view))
            assert _rejected_somewhere(h, k, view, out, *bad, delta)
    h = sides["item"]
    out = _sample(g, h, k, kappa=3.0, upweight=1.0, seed=42, counter=7)
    keys, u24, w = _weighted(h, None, 42, 7, 3.0, 1.0)
    drawn, inv = check_side(h, k, None, out, keys, u24, w, delta)
    assert drawn >= 8
    worst = max(worst, inv)
    # power: the same picks against keys without the label factor
    bad = _weighted(h, None, 42, 7, 3.0, 1.0, labels=False)
    assert _rejected_somewhere(h, k, None, out, *bad, delta)
    # ... and with the factor on the unlabelled side instead
    flipped = SR.slas_weights64(h.dot, 3.0, -1 - h.labels, 1.0)
    assert _rejected_somewhere(h, k, None, out, SR.slas_keys64(u24, flipped), u24, flipped, delta)
    print(f"weighted picks k={k}: largest relative inversion {worst:.3e} "
          f"(budget {SR.key_error_budget(2, 3.0):.3e}, delta {delta:.3e})")
    assert worst <= SR.key_error_budget(2, 3.0)      # above the un-multiplied budget: a finding


def test_weighted_picks_f16():
    """F = 16, the dot loop's bound, on a smaller graph."""
    data = edge_graph(F=16, lengths=[16, 65, 129, 1025, 2049], fill=100, seed=3)
    g = _graph(data)
    sides = _sides(data, g)
    delta, k, worst = SR.pick_delta(16, 3.0), 15, 0.0
    for side, view, up in (("user", "late", None), ("user", None, None), ("item", None, 1.0)):
        h = sides[side]
        out = _sample(g, h, k, kappa=3.0, temporal_view=view, upweight=up, seed=42, counter=8)
        keys, u24, w = _weighted(h, view, 42, 8, 3.0, up)
        drawn, inv = check_side(h, k, view, out, keys, u24, w, delta)
        assert drawn >= 4
        worst = max(worst, inv)
    print(f"weighted picks F=16: largest relative inversion {worst:.3e} "
          f"(budget {SR.key_error_budget(16, 3.0):.3e})")
    assert worst <= SR.key_error_budget(16, 3.0)


# -- c. stream words -------------------------------------------------------------------
SEED_HI = (0x9E3779B9 << 32) | 0x7F4A7C15
WORDS = [dict(seed=SEED_HI, counter=3, stage=0), dict(seed=42, counter=2 ** 31 + 12345, stage=0),
         dict(seed=42, counter=3, stage=255),
         dict(seed=SEED_HI, counter=2 ** 32 - 1, stage=255)]


@pytest.mark.parametrize("words", WORDS, ids=["seed-high", "counter-high", "stage-255", "all"])
def test_stream_words(graph, words):
    g, sides = graph
    delta, k = SR.pick_delta(2, 3.0), 15
    for side, view, up in (("user", "late", None), ("item", None, 1.0)):
        h = sides[side]
        out = _sample(g, h, k, kappa=3.0, temporal_view=view, upweight=up, **words)
        keys, u24, w = _weighted(h, view, words["seed"], words["counter"], 3.0, up,
                                 stage=words["stage"])
        drawn, _ = check_side(h, k, view, out, keys, u24, w, delta)
        assert drawn >= 8
        # power: each word dropped or truncated on the host is noticed
        for lost in (dict(words, seed=words["seed"] & 0xFFFFFFFF),
                     dict(words, counter=words["counter"] & 0x7FFFFFFF),
                     dict(words, stage=words["stage"] & 0x7F)):
            if lost == words:
                continue
            bad = _weighted(h, view, lost["seed"], lost["counter"], 3.0, up, stage=lost["stage"])
            assert _rejected_somewhere(h, k, view, out, *bad, delta), lost


def test_row_lists(graph):
    """A row's picks do not depend on the list: a row listed twice, the list
    in reverse, and ids outside [0, n_rows)."""
    g, sides = graph
    k = 15
    kw = dict(kappa=3.0, seed=42, counter=7)
    for side, view in (("user", "early"), ("item", None)):
        h = sides[side]
        full = _sample(g, h, k, temporal_view=view, **kw)
        n = h.n_rows
        rev = torch.arange(n - 1, -1, -1, device=DEV)
        for a, b in zip(full, _sample(g, h, k, rows=rev, temporal_view=view, **kw)):
            np.testing.assert_array_equal(a[::-1], b)
        hub = len(LENGTHS) - 1                                  # the 20000-slot row
        ids = [hub, 3, -1, hub, n, 2 ** 31 + 5, 0, hub, n - 1, -2 ** 31, 2 ** 40]
        o_nbr, o_eid, o_cnt = _sample(g, h, k, rows=torch.tensor(ids, device=DEV),
                                      temporal_view=view, **kw)
        for j, r in enumerate(ids):
            if 0 <= r < n:
                for a, b in zip(full, (o_nbr, o_eid, o_cnt)):
                    np.testing.assert_array_equal(a[r], b[j])
            else:
                assert o_cnt[j] == 0 and (o_nbr[j] == -1).all() and (o_eid[j] == -1).all(), r


# -- d. the weight clamp ---------------------------------------------------------------
def test_weight_clamp():
    """kappa = 200: exp(+-200) leaves fp32 on both sides, the weights are
    FLT_MAX (10 slots) and FLT_MIN (190 slots). The heavy slots' keys are
    denormal (their mutual order depends on flushing and is not asserted); the
    light slots' weight is exactly FLT_MIN, so only logf and the division
    separate the device's key from the host's."""
    m, heavy, k = 200, 10, 15
    rng = np.random.default_rng(5)
    e = np.stack([np.zeros(m, np.int64), rng.permutation(m)])
    ea = np.zeros((m, A), np.float32)
    item_x = np.tile(np.array([[1.0, 0.0]], np.float32), (m, 1))
    g = _graph((e, ea, np.zeros((1, 3), np.float32), np.array([-1]), item_x))
    assert g.user_mu[0].tolist() == [1.0, 0.0]
    is_heavy = np.zeros(m, bool)
    is_heavy[rng.permutation(m)[:heavy]] = True               # by slot position
    items = e[1]                                              # slot j holds edge j: item e[1][j]
    g.item_norm[torch.from_numpy(items[~is_heavy]).to(DEV)] = torch.tensor([-1.0, 0.0], device=DEV)
    row = torch.zeros(1, dtype=torch.int64, device=DEV)
    nbr, eid, cnt = (t.cpu().numpy() for t in g.sample(row, "user", k, kappa=200.0, seed=42,
                                                       counter=9))
    assert cnt[0] == k
    np.testing.assert_array_equal(nbr[0], items[eid[0]])
    assert sorted(eid[0, :heavy].tolist()) == np.flatnonzero(is_heavy).tolist()
    u24 = SR.slas_u24(42, 9, 0, 0, np.arange(m))
    w = SR.slas_weights64(np.where(is_heavy, 1.0, -1.0), 200.0)
    assert set(w.tolist()) == {SR.FLT_MIN, SR.FLT_MAX}
    SR.check_picks(SR.slas_keys64(u24, w, ~is_heavy), ~is_heavy, eid[0, heavy:],
                   SR.pick_delta(2, 0.0), u24, w)
    # non-finite profiles: still k distinct eligible edges
    for j, bad in enumerate(([np.nan, 0.0], [np.inf, 0.0], [-np.inf, 1.0], [np.nan, np.inf])):
        g.item_norm[int(items[3 + 7 * j])] = torch.tensor(bad, device=DEV)
    nbr, eid, cnt = (t.cpu().numpy() for t in g.sample(row, "user", k, kappa=200.0, seed=42,
                                                       counter=10))
    assert cnt[0] == k and len(set(eid[0].tolist())) == k
    assert ((eid[0] >= 0) & (eid[0] < m)).all()
    np.testing.assert_array_equal(nbr[0], items[eid[0]])


# -- bbgr_slas_induce at the scan's tile boundaries ----------------------------------------
IND_U, IND_I = 304, 64
SENTINEL = -0x0123456789ABCDEF
GUARD = 64


@pytest.fixture(scope="module")
def induce_csr():
    """304 user rows over 64 items, degrees cycling through the chunk edges;
    item_local is -1 for half the items; ts per edge id, some at the split."""
    rng = np.random.default_rng(11)
    deg = np.resize(np.array([0, 1, 63, 64, 65, 128, 129, 200]), IND_U)
    rng.shuffle(deg)
    ptr = np.zeros(IND_U + 1, np.int64)
    ptr[1:] = np.cumsum(deg)
    E = int(ptr[-1])
    nbr = rng.integers(0, IND_I, E)
    eid = rng.permutation(E)                                  # any one-to-one edge numbering
    ts = rng.uniform(0, 1, E).astype(np.float32)
    ts[rng.integers(0, E, E // 10)] = SPLIT
    item_local = np.full(IND_I, -1, np.int64)
    keep = rng.permutation(IND_I)[: IND_I // 2]
    item_local[keep] = rng.permutation(IND_I // 2)
    host = dict(ptr=ptr, nbr=nbr, eid=eid, ts=ts, item_local=item_local, deg=deg)
    i32 = dict(dtype=torch.int32, device=DEV)
    dev = dict(ptr=torch.tensor(ptr, **i32), nbr=torch.tensor(nbr, **i32),
               eid=torch.tensor(eid, **i32), ts=torch.tensor(ts, device=DEV),
               item_local=torch.tensor(item_local, **i32))
    return host, dev


def induce_ref(host, users, view):
    """(local user, local item, eid) in list order, then row order."""
    ptr, U = host["ptr"], host["ptr"].size - 1
    inside = (users >= 0) & (users < U)
    u = np.where(inside, users, 0)
    n = np.where(inside, ptr[u + 1] - ptr[u], 0)
    j = np.repeat(np.arange(users.size), n)
    off = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    slot = ptr[u][j] + off
    eid = host["eid"][slot]
    it = host["item_local"][host["nbr"][slot]]
    ts = host["ts"][eid]
    ok = it >= 0
    if view is not None:
        ok &= ts < SPLIT if view == "early" else ts >= SPLIT
    return j[ok], it[ok], eid[ok]


def _induce_args(dev, users, view, count):
    from bbgr import _lib
    from bbgr._lib import ptr
    a = _lib.SlasInduceArgs()
    a.n_users_listed, a.users, a.n_users = users.numel(), ptr(users), IND_U
    a.item_local = ptr(dev["item_local"])
    a.indptr, a.nbr, a.eid = ptr(dev["ptr"]), ptr(dev["nbr"]), ptr(dev["eid"])
    a.ts, a.ts_stride = ptr(dev["ts"]), 1
    a.view, a.split = _lib.SLAS_VIEW[view], SPLIT
    a.count = ptr(count)
    return a


def _induce(dev, users, view, capacity_short=0):
    """count + fill (twice) from one workspace into sentinel-filled buffers of
    the full size plus a guard. Returns (count, edges buffer, eid buffer,
    capacity, second fill's buffers)."""
    from bbgr._lib import call, ptr, stream_handle
    count = torch.full((1,), -77, dtype=torch.int64, device=DEV)
    a = _induce_args(dev, users, view, count)
    st = stream_handle()
    nb = ctypes.c_size_t(0)
    call("bbgr_slas_induce", ctypes.byref(a), None, ctypes.byref(nb), st)
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=DEV)
    call("bbgr_slas_induce", ctypes.byref(a), ptr(ws), ctypes.byref(nb), st)
    total = int(count.item())
    cap = max(total - capacity_short, 0)
    fills = []
    for _ in range(2):
        edges = torch.full((2 * total + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
        eids = torch.full((total + GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
        a.out_edges, a.out_eid, a.capacity = ptr(edges), ptr(eids), cap
        call("bbgr_slas_induce", ctypes.byref(a), ptr(ws), ctypes.byref(nb), st)
        fills.append((edges.cpu().numpy(), eids.cpu().numpy()))
    return total, cap, fills


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("n", [1, 4, 5, 8191, 8192, 8193, 16384, 16385, 24580])
def test_induce_at_scan_tiles(induce_csr, n, view):
    """slas_scan_kernel walks the per-user counts in tiles of 8192 with a
    carry: list lengths below, at and above one, two and three tiles."""
    host, dev = induce_csr
    rng = np.random.default_rng(n)
    users = rng.integers(-2, IND_U + 2, n)
    if n <= 5:
        users[0] = int(np.flatnonzero(host["deg"] == 200)[0])   # not an empty list
    want = induce_ref(host, users, view)
    users_d = torch.tensor(users, dtype=torch.int64, device=DEV)
    for short in (0, 7):
        total, cap, fills = _induce(dev, users_d, view, short)
        assert total == want[0].size and total > 7
        (edges, eids), again = fills
        for got, ref in ((edges[:cap], want[0]), (edges[cap:2 * cap], want[1]),
                         (eids[:cap], want[2])):
            np.testing.assert_array_equal(got, ref[:cap])
        # behind each array's own extent, guard included: untouched
        assert (edges[2 * cap:] == SENTINEL).all() and (eids[cap:] == SENTINEL).all()
        assert edges[2 * cap:].size >= GUARD and eids[cap:].size >= GUARD
        assert np.array_equal(edges, again[0]) and np.array_equal(eids, again[1])


@pytest.mark.parametrize("n", [3, 8193])
def test_induce_all_counts_zero(induce_csr, n):
    """Ids outside [0, U) and users without a row or without a sampled item."""
    host, dev = induce_csr
    empty = np.flatnonzero(host["deg"] == 0)
    one = np.flatnonzero(host["deg"] == 1)                    # ... whose only item is unsampled
    one = one[host["item_local"][host["nbr"][host["ptr"][one]]] < 0]
    assert empty.size and one.size
    users = np.resize(np.concatenate([[-1, IND_U, -2 ** 40, 2 ** 31 + 5], empty, one]), n)
    assert induce_ref(host, users, "late")[0].size == 0
    total, cap, fills = _induce(dev, torch.tensor(users, dtype=torch.int64, device=DEV), "late")
    assert total == 0 and cap == 0
    assert (fills[0][0] == SENTINEL).all() and (fills[0][1] == SENTINEL).all()


# -- bbgr_slas_profiles at the dispatch edges ---------------------------------------------
@pytest.mark.parametrize("F", [3, 4, 8, 16])
def test_profiles_padded_rows(F):
    """F <= 2 | <= 4 | else 16 select the kernel; item_x is a column slice of a
    wider tensor (ldx = F + 3) whose pad columns hold large values."""
    from bbgr._lib import call, ptr, stream_handle
    U, I, E = 700, 300, 9000
    rng = np.random.default_rng(40 + F)
    src = rng.integers(0, U - 1, E - 3000 - 1)               # user U-1 stays isolated
    src[src == 11] = 12
    dst = rng.integers(0, I, src.size)
    dst[dst == 7] = 8
    src = np.concatenate([src, np.full(3000, 5), [11]])       # a 3000-edge hub
    dst = np.concatenate([dst, rng.integers(0, I, 3000), [7]])
    dst[(src == 5) & (dst == 7)] = 8
    # no cancelling rows: every feature has mean 0.5, so a user's mean stays away from 0
    x = (rng.normal(size=(I, F)) + 0.5).astype(np.float32)
    x[7] = 0.0                                       # a zero feature row: user 11's only item
    e = np.stack([src, dst])
    ea = np.zeros((E, A), np.float32)
    g = _graph((e, ea, np.zeros((U, 3), np.float32), np.full(U, -1), x))
    wide = torch.full((I, F + 3), 1e4, device=DEV)
    wide[:, 1:1 + F] = torch.from_numpy(x).to(DEV)
    item_x = wide[:, 1:1 + F]
    assert item_x.stride(0) == F + 3 and not item_x.is_contiguous()
    outs = []
    for _ in range(2):
        a = torch.full((I, F), 7.0, device=DEV)
        b = torch.full((U, F), 7.0, device=DEV)
        call("bbgr_slas_profiles", U, I, F, ptr(item_x), F + 3, ptr(g.u_csr.indptr),
             ptr(g.u_csr.nbr), ptr(a), ptr(b), stream_handle())
        outs.append((a, b))
    (a, b), (a2, b2) = outs
    want_in, want_mu = SR.profiles64(e, x, U)
    _close(a, want_in, f"item_norm F={F} ldx={F + 3}", 1e-5)
    _close(b, want_mu, f"user_mu F={F} ldx={F + 3}", 1e-5)
    assert a[7].abs().sum().item() == 0 and b[11].abs().sum().item() == 0
    assert b[U - 1].abs().sum().item() == 0
    assert torch.equal(a, a2) and torch.equal(b, b2)          # fixed order
    assert torch.equal(a, g.item_norm[:I]) and torch.equal(b, g.user_mu[:U])   # = the packed call
    assert (wide[:, 0] == 1e4).all() and (wide[:, 1 + F:] == 1e4).all()
