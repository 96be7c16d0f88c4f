"""Host restatement of the SLAS subgraph builder (main.py:727-883), the loop
the GPU tests compare against: same order, np.unique and dictionaries, fp32
profiles through torch as the reference forms them. Every sampling call can be
replaced by supplied picks (``pick(kind, row, nbrs, eids, k)`` returns the
chosen positions in the eligible arrays, in output order); without it the
draws are ``rng.choice(n, k, replace=False, p=w)`` on ``default_rng(42)``.
Below it, the sampler's own keys restated (Philox4x32-10, u24, float64 keys)
and ``check_picks``, the tolerant form of "the k smallest keys, ascending".
A helper, not a test module."""
import numpy as np
import torch


def l2n(x, eps=1e-12):
    return x / (x.norm(dim=-1, keepdim=True) + eps)


def profiles64(e_u2i, item_x, num_users):
    """item_norm, user_mu of main.py:727-737 in float64 (the profiles' parity
    reference)."""
    x = np.asarray(item_x, np.float64)
    inorm = x / (np.sqrt((x * x).sum(-1, keepdims=True)) + 1e-12)
    e = np.asarray(e_u2i).astype(np.int64)
    s = np.zeros((num_users, x.shape[1]))
    np.add.at(s, e[0], inorm[e[1]])
    deg = np.bincount(e[0], minlength=num_users).astype(np.float64)
    mu = s / np.maximum(deg, 1.0)[:, None]
    return inorm, mu / (np.sqrt((mu * mu).sum(-1, keepdims=True)) + 1e-12)


def csr_from_src(src, dst, num_src):
    order = np.argsort(src, kind="mergesort")
    counts = np.bincount(src[order], minlength=num_src)
    ptr = np.zeros(num_src + 1, np.int64)
    ptr[1:] = np.cumsum(counts, dtype=np.int64)
    return ptr, dst[order].astype(np.int64), order.astype(np.int64)


class HostSlas:
    def __init__(self, e_u2i, edge_attr, user_x, user_y, item_x, ts_idx=3, kappa=3.0,
                 upweight=1.0, k_item=15, k_user=15, split=0.5, seed=42, pick=None):
        self.e = np.asarray(e_u2i).astype(np.int64)
        self.ea = torch.as_tensor(np.asarray(edge_attr), dtype=torch.float32)
        self.user_x = torch.as_tensor(np.asarray(user_x), dtype=torch.float32)
        self.user_y = torch.as_tensor(np.asarray(user_y), dtype=torch.int64)
        self.item_x = torch.as_tensor(np.asarray(item_x), dtype=torch.float32)
        self.U, self.I, self.E = self.user_x.size(0), self.item_x.size(0), self.e.shape[1]
        self.ts_idx, self.kappa, self.upweight = ts_idx, kappa, upweight
        self.k_item, self.k_user, self.split = k_item, k_user, split
        self.pick = pick
        self.rng = np.random.default_rng(seed)
        # profiles
        self.item_norm = l2n(self.item_x.clone())
        src_u, dst_i = torch.from_numpy(self.e[0]), torch.from_numpy(self.e[1])
        s = torch.zeros((self.U, self.item_norm.size(1)), dtype=torch.float32)
        s.index_add_(0, src_u, self.item_norm[dst_i])
        deg = torch.zeros((self.U,), dtype=torch.float32)
        deg.index_add_(0, src_u, torch.ones((self.E,), dtype=torch.float32))
        self.user_mu = l2n(s / deg.unsqueeze(-1).clamp(min=1.0))
        # adjacency in input-edge order
        self.u_ptr, self.u_nbr, self.u_eid = csr_from_src(self.e[0], self.e[1], self.U)
        self.i_ptr, self.i_nbr, self.i_eid = csr_from_src(self.e[1], self.e[0], self.I)

    def _view_mask(self, eids, view):
        ts = self.ea[torch.from_numpy(eids), self.ts_idx].numpy()
        return ts < self.split if view == "early" else ts >= self.split

    def _choose(self, kind, row, nbrs, eids, k, w):
        if self.pick is not None:
            return np.asarray(self.pick(kind, row, nbrs, eids, k), dtype=np.int64)
        return self.rng.choice(nbrs.size, size=k, replace=False, p=w)

    def items_for_user(self, u, view):
        a, b = self.u_ptr[u], self.u_ptr[u + 1]
        if b <= a:
            return np.empty((0,), np.int64)
        items, eids = self.u_nbr[a:b], self.u_eid[a:b]
        if view is not None:
            m = self._view_mask(eids, view)
            items, eids = items[m], eids[m]
            if items.size == 0:
                return np.empty((0,), np.int64)
        if items.size <= self.k_item:
            return items.copy()
        sim = (self.item_norm[torch.from_numpy(items)] @ self.user_mu[u]).numpy()
        w = np.exp(self.kappa * sim)
        w = w / (w.sum() + 1e-12)
        return items[self._choose("items", u, items, eids, self.k_item, w)]

    def users_for_item(self, i):
        a, b = self.i_ptr[i], self.i_ptr[i + 1]
        if b <= a:
            return np.empty((0,), np.int64)
        users, eids = self.i_nbr[a:b], self.i_eid[a:b]
        if users.size <= self.k_user:
            return users.copy()
        sim = (self.user_mu[torch.from_numpy(users)] @ self.item_norm[i]).numpy()
        w = np.exp(self.kappa * sim)
        y = self.user_y[torch.from_numpy(users)].numpy()
        w[y >= 0] *= (1.0 + self.upweight)
        w = w / (w.sum() + 1e-12)
        return users[self._choose("users", i, users, eids, self.k_user, w)]

    def build_subgraph(self, seed_users, view):
        seed_users = np.asarray(seed_users, np.int64)
        got = [self.items_for_user(int(u), view) for u in seed_users]
        sampled_items = np.unique(np.concatenate(got) if got else np.empty((0,), np.int64))
        got = [self.users_for_item(int(i)) for i in sampled_items]
        extra = np.unique(np.concatenate(got) if got else np.empty((0,), np.int64))
        seed_set = set(seed_users.tolist())
        extra_only = np.array([u for u in extra.tolist() if u not in seed_set], dtype=np.int64)
        users_global = np.concatenate([seed_users, extra_only], axis=0)
        u_lid = {int(g): j for j, g in enumerate(users_global.tolist())}
        i_lid = {int(g): j for j, g in enumerate(sampled_items.tolist())}
        src_l, dst_l, eid_l = [], [], []
        for ug in users_global.tolist():
            a, b = self.u_ptr[ug], self.u_ptr[ug + 1]
            if b <= a:
                continue
            items, eids = self.u_nbr[a:b], self.u_eid[a:b]
            if view is not None:
                m = self._view_mask(eids, view)
                items, eids = items[m], eids[m]
            for it, eid in zip(items.tolist(), eids.tolist()):
                if it in i_lid:
                    src_l.append(u_lid[ug])
                    dst_l.append(i_lid[it])
                    eid_l.append(eid)
        if not eid_l:
            e_u2i = torch.zeros((2, 0), dtype=torch.long)
            ea = torch.zeros((0, self.ea.size(1)), dtype=torch.float32)
        else:
            e_u2i = torch.tensor([src_l, dst_l], dtype=torch.long)
            ea = self.ea[torch.tensor(eid_l, dtype=torch.long)].clone()
        return {
            "bs": seed_users.size,
            "users_global": users_global,
            "items_global": sampled_items,
            "x_u": self.user_x[torch.from_numpy(users_global)].clone(),
            "y_u": self.user_y[torch.from_numpy(users_global)].clone(),
            "x_i": self.item_x[torch.from_numpy(sampled_items)].clone(),
            "e_u2i": e_u2i,
            "ea_u2i": ea,
            "e_i2u": torch.stack([e_u2i[1], e_u2i[0]], dim=0),
            "ea_i2u": ea,
        }


def picks_from_device(last_picks, seed_users):
    """A `pick` callback that replays a device call's picks: the chosen edge
    ids of each row, mapped to positions in the host's eligible arrays."""
    it_nbr, it_eid, it_cnt = (t.cpu().numpy() for t in last_picks["items"])
    us_nbr, us_eid, us_cnt = (t.cpu().numpy() for t in last_picks["users"])
    row_of = {("items", int(u)): j for j, u in enumerate(np.asarray(seed_users).tolist())}
    row_of.update({("users", int(i)): j
                   for j, i in enumerate(last_picks["items_global"].cpu().numpy().tolist())})

    def pick(kind, row, nbrs, eids, k):
        j = row_of[(kind, int(row))]
        e, c = (it_eid, it_cnt) if kind == "items" else (us_eid, us_cnt)
        assert c[j] == k
        where = {int(x): p for p, x in enumerate(eids.tolist())}
        return [where[int(x)] for x in e[j, :k]]
    return pick


# -- the sampler's keys, restated on the host -------------------------------------
# bbgr.h: slot j of a row with more than k eligible slots gets the key
# -log(U_j) / w_j, U_j from the first Philox4x32-10 word at counter
# {counter, stage, row id, slot position in the full row}, key = seed.
_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
FLT_MIN, FLT_MAX = 1.17549435e-38, 3.40282347e38


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 as csrc/common.h states it, vectorised: uint64 arithmetic
    masked to 32 bits. Returns the four output words (uint64 arrays < 2^32)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) & _M32
                                           for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = _PHILOX_M0 * c0                      # 32 x 32 bits: no overflow in 64
        p1 = _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32)
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def slas_u24(seed, counter, stage, row, positions):
    """The integer (x0 >> 8) + 1 in [1, 2^24] behind U = u24 * 2^-24.
    `positions` are slot positions in the full row (e - indptr[row]), not ranks
    among the eligible slots; `row` may be an array of the same shape."""
    seed = int(seed)
    x0 = philox4x32_10(counter, stage, row, positions, seed & 0xFFFFFFFF, seed >> 32)[0]
    return (x0 >> np.uint64(8)).astype(np.int64) + 1


def slas_weights64(dot64, kappa, labels=None, upweight=0.0):
    """clip(exp(kappa * dot) * (1 + upweight where label >= 0), FLT_MIN, FLT_MAX)
    in float64; a NaN weight becomes FLT_MIN as fminf(fmaxf(.)) makes it."""
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(float(kappa) * np.asarray(dot64, np.float64))
        if labels is not None:
            w = w * np.where(np.asarray(labels) >= 0, 1.0 + float(upweight), 1.0)
    return np.clip(np.where(np.isnan(w), FLT_MIN, w), FLT_MIN, FLT_MAX)


def slas_keys64(u24, w, eligible=None):
    """float64 keys -log(u24 * 2^-24) / w, +inf at the ineligible slots."""
    keys = -np.log(np.asarray(u24, np.float64) * 2.0 ** -24) / np.asarray(w, np.float64)
    keys = np.abs(keys)                              # -log(1) / w is -0.0
    return keys if eligible is None else np.where(eligible, keys, np.inf)


def slot_rows(ptr):
    """(row id, position in the row) of every slot of a CSR."""
    ptr = np.asarray(ptr, np.int64)
    row = np.repeat(np.arange(ptr.size - 1, dtype=np.int64), np.diff(ptr))
    return row, np.arange(ptr[-1], dtype=np.int64) - ptr[row]


# The relative error of a device key against slas_keys64, and check_picks' delta.
#   exponent: the fmaf chain of the dot product rounds F times and kappa * dot
#     once, each by at most 2^-24 of a value of magnitude <= 1 (unit profiles,
#     Cauchy-Schwarz for the partial sums) resp. <= |kappa|: an absolute error
#     of at most (F + 1) * 2^-24 * |kappa| in the exponent, the same relative
#     error in w (first order);
#   expf and logf: 3 ulp each; the division: 2.5 ulp; the label multiply: 0.5 ulp
#     (correctly rounded). One ulp is at most 2^-23 relative. These are the
#     OpenCL 3.0 full-profile bounds (table "ULP values for single precision
#     built-in math functions": exp <= 3, log <= 3, x / y <= 2.5), which the
#     ROCm device library's expf / logf / division are specified against. HIP's
#     math API page lists measured maxima per function, none above these, so
#     the OpenCL figures are the looser, safe choice.
# Two keys are compared and a factor two covers slack: delta = 4 * budget.
_KEY_ULPS = 3.0 + 3.0 + 2.5 + 0.5


def key_error_budget(F, kappa):
    return (F + 1) * 2.0 ** -24 * abs(float(kappa)) + _KEY_ULPS * 2.0 ** -23


def pick_delta(F, kappa):
    return 4.0 * key_error_budget(F, kappa)


def check_picks(keys64, eligible, picked, delta, u24=None, w=None):
    """The tolerant form of "the k smallest keys, ascending, equal keys the
    lower slot first" for one row: `picked` are slot positions in output order.
    Where every gap between neighbouring keys exceeds delta this is equality
    with argsort. Returns the largest relative inversion met (0 if none):
    1 - later / earlier over consecutive picks and over (last pick, best
    unpicked slot)."""
    keys64 = np.asarray(keys64, np.float64)
    eligible = np.asarray(eligible, bool)
    p = np.asarray(picked, np.int64)
    assert p.size >= 1
    assert ((p >= 0) & (p < keys64.size)).all(), ("position out of the row", p)
    assert np.unique(p).size == p.size, ("a slot picked twice", p)
    assert eligible[p].all(), ("an ineligible slot picked", p[~eligible[p]])
    kp = keys64[p]
    assert np.isfinite(kp).all(), ("a pick without a finite key", p)
    lo = kp[:-1] * (1.0 - delta)
    assert (kp[1:] >= lo).all(), ("picks not in ascending key order",
                                  p[:-1][kp[1:] < lo], kp[:-1][kp[1:] < lo], kp[1:][kp[1:] < lo])
    rest = eligible.copy()
    rest[p] = False
    best_rest = keys64[rest].min() if rest.any() else np.inf
    assert best_rest >= kp[-1] * (1.0 - delta), ("an unpicked slot beats the last pick",
                                                 int(np.flatnonzero(rest)[keys64[rest].argmin()]),
                                                 best_rest, kp[-1])
    if u24 is not None:
        u24, w = np.asarray(u24), np.asarray(w)
        tie = (u24[p[1:]] == u24[p[:-1]]) & (w[p[1:]] == w[p[:-1]])
        assert (p[1:][tie] > p[:-1][tie]).all(), ("equal keys, higher slot first", p[:-1][tie])
    later = np.append(kp[1:], best_rest)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(kp > 0, 1.0 - later / kp, 0.0)
    return float(max(inv.max(), 0.0))
