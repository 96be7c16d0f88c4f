"""GPU: credibility edge weights (csrc/cred.hip, bbgr_ewa_normalize) and the
aggregation at the row-plan boundaries, in every input mode and workspace
layout, with non-default columns and coefficients and with non-finite
attributes, against the float64 oracle (oracle/ref_numpy) and torch's CPU
expressions (oracle/ref_torch.CredModelRef).

Every tolerance here is bitwise, one of the two derived bounds below, or
test_gpu_cred.py's for the whole-model comparison.

u = 2^-24 (fp32 unit roundoff), gamma_n = n u / (1 - n u).

Normalised weights, w~ = w / (den + eps), all w >= 0. A sum of non-negative
terms in which no term passes through more than k fp32 additions has a
relative error of at most gamma_k, whatever the order. `den + eps` and the
division round once each (csrc/Makefile sets no fast-math flag, so the division
is correctly rounded), hence |w~ - exact| <= gamma_{k+2} |exact| per element.
k from seg_sum_kernel / seg_fixup_kernel, for a row of deg >= 1 edges:
  * short row (deg <= long_threshold): each of the 16 lanes starts from 0 (the
    first `s += x` is exact) and adds its ceil(deg/16) terms at the most:
    ceil(deg/16) - 1 additions; group16_sum_c then adds across the lanes in 4
    shuffle steps: k = ceil(deg/16) - 1 + 4;
  * a chunk of L edges: each of the 256 threads adds ceil(L/256) terms at the
    most from 0: ceil(L/256) - 1 additions, then the LDS tree of 8 levels
    (w = 128 .. 1): k = ceil(L/256) - 1 + 8;
  * a row split into c chunks: the plan's chunks hold floor or ceil(deg/c)
    edges, so L <= ceil(deg/c); seg_fixup_kernel adds the c partials in order
    from 0: c - 1 more additions.
(The float64 oracle's own error, about deg * 2^-53, is not added to the bound.)

Aggregation, out[r] = sum_e w_e x[src_e] over the deg edges of row r: each
product rounds at most once and passes through at most deg - 1 additions (an
FMA only removes roundings), so in any order
|got - exact| <= gamma_{deg+1} * sum_e |w_e| |x_e| per output element.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ref_numpy as R  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
LONG_THRESHOLD, CHUNK_EDGES = 64, 2048      # what EdgeSet plans with below 8M edges
DEGREES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097,
           6145]
ZERO_DEGREES = [70, 2100]                   # rows whose raw weights are all zero
N_SRC_USED, N_SRC = 50, 53                  # sources 50..52 have no edge
EPS = float(np.float32(1e-12))              # the float the ABI receives
SENTINEL, PAD, TAIL = -7.0, 64, 1024
MODES = ("w_in", "attr", "own_raw")


def _gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def _n_chunks(deg):
    """include/bbgr.h: deg > long_threshold -> ceil(deg / chunk_edges) chunks."""
    return -(-deg // CHUNK_EDGES) if deg > LONG_THRESHOLD else 0


def _k_sum(deg):
    """Additions on the longest path of a row's sum (module docstring)."""
    if deg == 0:
        return 0
    c = _n_chunks(deg)
    if c == 0:
        return math.ceil(deg / 16) - 1 + 4
    L = math.ceil(deg / c)
    return math.ceil(L / 256) - 1 + 8 + (c - 1)


def boundary_edges(seed=0):
    """A bipartite edge list with prescribed destination degrees: every plan
    boundary, two all-zero rows, a few degree-3 rows so that n_dst % 16 != 0;
    destination ids shuffled with row 0 empty and the last row non-empty;
    sources from 50 ids (duplicate pairs); edge order shuffled.
    Returns (edge_index [2, E] int64, degrees by destination id, n_src, n_dst)."""
    rng = np.random.default_rng(seed)
    want = DEGREES + ZERO_DEGREES + [3, 3, 3, 3]
    n_dst = len(want)
    assert n_dst % 16 != 0 and want[0] == 0 and all(d > 0 for d in want[1:])
    ids = np.concatenate([[0], 1 + rng.permutation(n_dst - 1)])   # the empty row keeps id 0
    deg = np.zeros(n_dst, np.int64)
    deg[ids] = want
    assert deg[0] == 0 and deg[-1] > 0
    dst = np.repeat(np.arange(n_dst), deg)
    src = rng.integers(0, N_SRC_USED, dst.size)
    order = rng.permutation(dst.size)
    ei = np.stack([src[order], dst[order]])
    pairs = ei[0] * n_dst + ei[1]
    assert np.unique(pairs).size < pairs.size                     # duplicate (src, dst) pairs
    return ei, deg, N_SRC, n_dst


def _expected_plan(deg):
    ch = [_n_chunks(int(d)) for d in deg]
    return sum(ch), sum(c > 1 for c in ch)


class Graph:
    def __init__(self):
        from bbgr.cred_gnn import EdgeSet
        self.ei, self.deg, self.n_src, self.n_dst = boundary_edges()
        self.E = self.ei.shape[1]
        self.es = EdgeSet(torch.tensor(self.ei, device=DEV), self.n_src, self.n_dst)
        self.perm = self.es.by_dst.perm[: self.E].cpu().numpy().astype(np.int64)
        # the same hubs on the source side
        self.ei_f = np.ascontiguousarray(self.ei[::-1])
        self.es_f = EdgeSet(torch.tensor(self.ei_f, device=DEV), self.n_dst, self.n_src)
        self.zero_rows = np.flatnonzero(np.isin(self.deg, ZERO_DEGREES))
        self.k_edge = np.asarray([_k_sum(int(d)) for d in self.deg])[self.ei[1]]


@pytest.fixture(scope="module")
def G():
    return Graph()


def normalize_raw(es, mode, with_dst, *, raw=None, attr=None, cv=0, ca=1, beta=1.0, gamma=1.0,
                  eps=EPS):
    """bbgr_ewa_normalize through ctypes in one input mode: raw weights given
    (`w_in`), attributes with a w_raw output (`attr`), attributes with w_raw NULL
    (`own_raw`: the raw weights live at the front of the workspace). Outputs and
    workspace carry sentinel-filled tails, which must come back untouched."""
    from bbgr._lib import call, ptr, stream_handle
    E = es.E
    w_raw, w_edge, w_csr = (torch.full((E + PAD,), SENTINEL, device=DEV) for _ in range(3))
    w_in = torch.tensor(raw, device=DEV) if mode == "w_in" else None
    a = None if mode == "w_in" else torch.tensor(attr, device=DEV).contiguous()
    cs = es.by_dst.struct()
    args = (ctypes.byref(cs), ptr(es.by_dst.perm), ptr(es.dst if with_dst else None), ptr(w_in),
            ptr(a), 0 if a is None else a.shape[1], cv, ca, float(beta), float(gamma), float(eps),
            ptr(w_raw if mode == "attr" else None), ptr(w_edge), ptr(w_csr))
    n = ctypes.c_size_t(0)
    call("bbgr_ewa_normalize", *args, None, ctypes.byref(n), stream_handle())
    ws = torch.full((n.value + TAIL,), 0xA5, dtype=torch.uint8, device=DEV)
    have = ctypes.c_size_t(n.value)
    call("bbgr_ewa_normalize", *args, ptr(ws), ctypes.byref(have), stream_handle())
    torch.cuda.synchronize()
    assert bool((ws[n.value:] == 0xA5).all()), (mode, with_dst, "workspace tail written")
    for name, t in (("w_raw", w_raw), ("w_edge", w_edge), ("w_csr", w_csr)):
        assert bool((t[E:] == SENTINEL).all()), (mode, with_dst, name, "written past E")
    if mode != "attr":
        assert bool((w_raw == SENTINEL).all()), (mode, "w_raw written though not given")
    return dict(ws_bytes=n.value, w_raw=w_raw[:E].cpu().numpy(), w_edge=w_edge[:E].cpu().numpy(),
                w_csr=w_csr[:E].cpu().numpy())


def all_modes(es, attr, **kw):
    """{(mode, with_dst): result} with w_in = the oracle's raw weights of attr."""
    raw = R.ewa_raw(attr, kw.get("cv", 0), kw.get("ca", 1), kw.get("beta", 1.0),
                    kw.get("gamma", 1.0))
    return raw, {(m, wd): normalize_raw(es, m, wd, raw=raw, attr=attr, **kw)
                 for m in MODES for wd in (True, False)}


def _general_attr(G, seed=1):
    """verified in {-0.5, 0} (both clamp to 0) and rating_align uniform in
    (0, 1], so with beta = gamma = 1 the raw weight is rating_align itself;
    some exact zeros (align -1), and the two zero rows entirely."""
    rng = np.random.default_rng(seed)
    attr = rng.uniform(-1, 1, (G.E, 5)).astype(np.float32)
    attr[:, 0] = rng.choice(np.asarray([-0.5, 0.0], np.float32), G.E)
    attr[:, 1] = (1.0 - rng.random(G.E)).astype(np.float32)       # (0, 1]
    attr[rng.random(G.E) < 0.05, 1] = -1.0
    attr[np.isin(G.ei[1], G.zero_rows), 1] = -1.0
    return attr


@pytest.fixture(scope="module")
def general(G):
    attr = _general_attr(G)
    raw, res = all_modes(G.es, attr)
    assert raw.max() <= 1.0 and raw.min() == 0.0 and (raw > 0).mean() > 0.8
    return attr, raw, res


def _assert_rel_bound(got, ref, k_edge, what):
    ref = np.asarray(ref, np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    bound = _gamma(k_edge + 2) * np.abs(ref)
    units = np.divide(err, np.abs(ref) * U, out=np.zeros_like(err), where=ref != 0)
    worst = int(np.argmax(units))
    msg = (f"{what}: largest error {units.max():.3f} u (edge {worst}, k + 2 = "
           f"{int(np.broadcast_to(k_edge, err.shape)[worst]) + 2})")
    print(msg)
    assert np.all(err <= bound), msg + f"; {int((err > bound).sum())} elements over the bound"
    assert np.all(got[ref == 0] == 0), what + ": a zero weight is not exactly zero"


# -- the plan -----------------------------------------------------------------------

def test_boundary_graph_is_on_every_plan_path(G):
    """The plan EdgeSet builds is the header's rule at long_threshold 64 and
    chunk_edges 2048: a change of defaults moves the cases off these paths and
    fails here. Chunk table: equal-size chunks, slot -1 for a sole chunk."""
    assert 25_000 < G.E < 33_000 and G.n_dst % 16 != 0
    want_deg = sorted(DEGREES + ZERO_DEGREES + [3, 3, 3, 3])
    assert sorted(np.bincount(G.ei[1], minlength=G.n_dst).tolist()) == want_deg
    n_chunks, n_split = _expected_plan(G.deg)
    assert (n_chunks, n_split) == (22, 6)
    for csr in (G.es.by_dst, G.es_f.by_src):
        assert (csr.long_threshold, csr.chunk_edges) == (LONG_THRESHOLD, CHUNK_EDGES)
        assert (csr.n_chunks, csr.n_split) == (n_chunks, n_split)
        indptr = csr.indptr.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.diff(indptr), G.deg)
        want_ch, want_sp = [], []
        for r, d in enumerate(G.deg):
            c = _n_chunks(int(d))
            if c > 1:
                want_sp.append([r, len(want_ch), c, 0])
            for j in range(c):
                want_ch.append([r, indptr[r] + d * j // c, indptr[r] + d * (j + 1) // c,
                                len(want_ch) if c > 1 else -1])
        assert np.array_equal(csr.chunks[: 4 * n_chunks].view(-1, 4).cpu().numpy(), want_ch)
        assert np.array_equal(csr.split[: 4 * n_split].view(-1, 4).cpu().numpy(), want_sp)
    # the flipped graph's destination side: rows of one chunk each
    assert G.es_f.by_dst.n_chunks == N_SRC_USED and G.es_f.by_dst.n_split == 0


# -- normalisation --------------------------------------------------------------------

@pytest.mark.parametrize("with_dst", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_exact_weights_are_bitwise(G, mode, with_dst):
    """Small non-negative integer raw weights (verified in {0, 1}, integer
    rating_align, beta = 2, gamma = 3): every row sum is an integer below 2^24,
    exact in fp32 in any order, and the division is correctly rounded."""
    rng = np.random.default_rng(2)
    attr = np.zeros((G.E, 5), np.float32)
    attr[:, 0] = rng.integers(0, 2, G.E)
    attr[:, 1] = rng.integers(-2, 6, G.E)
    attr[np.isin(G.ei[1], G.zero_rows), :2] = (0.0, -1.0)
    attr[:, 2:] = rng.uniform(-9, 9, (G.E, 3))
    raw = R.ewa_raw(attr, beta=2.0, gamma=3.0)
    assert np.array_equal(raw, np.round(raw)) and raw.max() == 17 and raw.min() == 0
    den = np.bincount(G.ei[1], weights=raw.astype(np.float64), minlength=G.n_dst)
    assert den.max() < 2 ** 24 and np.all(den[G.zero_rows] == 0)
    got = normalize_raw(G.es, mode, with_dst, raw=raw, attr=attr, beta=2.0, gamma=3.0)
    want = raw / (den.astype(np.float32) + np.float32(EPS))[G.ei[1]]
    assert want.dtype == np.float32
    if mode == "attr":
        np.testing.assert_array_equal(got["w_raw"], raw)
    np.testing.assert_array_equal(got["w_edge"], want)
    np.testing.assert_array_equal(got["w_csr"], want[G.perm])
    assert np.all(got["w_edge"][np.isin(G.ei[1], G.zero_rows)] == 0)


@pytest.mark.parametrize("with_dst", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_general_weights_within_the_derived_bound(G, general, mode, with_dst):
    """Uniform raw weights in (0, 1] with exact zeros, against the float64
    oracle of the same fp32 raw weights: gamma_{k+2} per element, k by row
    (module docstring). Rows of all-zero weights give exactly 0 / (0 + eps)."""
    attr, raw, res = general
    got = res[(mode, with_dst)]
    if mode == "attr":
        np.testing.assert_array_equal(got["w_raw"], raw)
    ref = R.normalize_per_dst(raw, G.ei[1], G.n_dst, eps=EPS)
    _assert_rel_bound(got["w_edge"], ref, G.k_edge, f"w_edge {mode} dst={with_dst}")
    np.testing.assert_array_equal(got["w_csr"], got["w_edge"][G.perm])
    zero = np.isin(G.ei[1], G.zero_rows)
    assert zero.sum() == sum(ZERO_DEGREES) and np.all(got["w_edge"][zero] == 0)


def test_all_modes_and_both_dst_variants_are_bitwise_equal(general):
    _, _, res = general
    first = res[("w_in", True)]
    for key, got in res.items():
        assert np.array_equal(got["w_edge"], first["w_edge"]), key
        assert np.array_equal(got["w_csr"], first["w_csr"]), key


def test_workspace_sizes(G, general):
    """own_raw adds exactly align_up(4 E) for its input-order raw weights; the
    tails behind the queried sizes were checked untouched in every run."""
    _, _, res = general

    def align(x):
        return (x + 255) // 256 * 256
    base = align(4 * G.E) + align(4 * G.n_dst) + align(4 * G.es.by_dst.n_chunks)
    for (mode, _), got in res.items():
        assert got["ws_bytes"] == base + (align(4 * G.E) if mode == "own_raw" else 0), mode


@pytest.mark.parametrize("with_dst", [True, False])
def test_non_default_eps(G, general, with_dst):
    """eps = 1e-3 (the float the ABI receives) against the oracle's eps."""
    attr, raw, res = general
    eps = float(np.float32(1e-3))
    got = normalize_raw(G.es, "own_raw", with_dst, attr=attr, eps=eps)
    ref = R.normalize_per_dst(raw, G.ei[1], G.n_dst, eps=eps)
    _assert_rel_bound(got["w_edge"], ref, G.k_edge, f"w_edge eps=1e-3 dst={with_dst}")
    np.testing.assert_array_equal(got["w_csr"], got["w_edge"][G.perm])
    assert not np.array_equal(got["w_edge"], res[("own_raw", with_dst)]["w_edge"])


def test_edge_set_normalize_is_the_same_call(G, general):
    """EdgeSet.normalize (what CredModel drives) gives the raw call's bits."""
    attr, raw, res = general
    w_raw, w_edge, w_csr = G.es.normalize(edge_attr=torch.tensor(attr, device=DEV))
    np.testing.assert_array_equal(w_raw.cpu().numpy(), raw)
    np.testing.assert_array_equal(w_edge.cpu().numpy(), res[("attr", True)]["w_edge"])
    np.testing.assert_array_equal(w_csr.cpu().numpy(), res[("attr", True)]["w_csr"])
    _, w_edge2, _ = G.es.normalize(w=torch.tensor(raw, device=DEV))
    np.testing.assert_array_equal(w_edge2.cpu().numpy(), res[("w_in", True)]["w_edge"])


# -- EWA parameters and special values ------------------------------------------------

COEFFS = [(0.75, 1.3), (1.3, 0.75), (2.0, -0.6)]
COLUMNS = [(3, 1, 5), (4, 0, 5), (1, 1, 2), (0, 7, 8)]


def _identity_edges(E):
    from bbgr.cred_gnn import EdgeSet
    idx = torch.arange(E, dtype=torch.int64, device=DEV)
    return EdgeSet(torch.stack([idx, idx]), E, E)


@pytest.mark.parametrize("E", [1, 255, 256, 257])
def test_ewa_raw_parameter_sweep_is_exact(E):
    """Coefficients whose products are inexact, every column layout: bitwise the
    oracle's two fp32 products and their fp32 sum (no contraction into an FMA,
    no swapped coefficient, no column or lda mix-up)."""
    es = _identity_edges(E)
    rng = np.random.default_rng(100 + E)
    for cv, ca, lda in COLUMNS:
        attr = rng.uniform(-0.5, 1.5, (E, lda)).astype(np.float32)
        for beta, gamma in COEFFS:
            want = R.ewa_raw(attr, cv, ca, beta, gamma)
            for mode in ("attr", "own_raw"):
                got = normalize_raw(es, mode, True, attr=attr, cv=cv, ca=ca, beta=beta,
                                    gamma=gamma)
                if mode == "attr":
                    np.testing.assert_array_equal(got["w_raw"], want, str((cv, ca, lda, beta, gamma)))
                # one edge per row: w~ = w / (w + eps), correctly rounded
                np.testing.assert_array_equal(got["w_edge"], want / (want + np.float32(EPS)),
                                              str((mode, cv, ca, lda, beta, gamma)))
    # the sweep can tell the faults apart: an FMA or swapped coefficients change bits
    a = rng.uniform(-0.5, 1.5, (257, 5)).astype(np.float32)
    v = np.clip(a[:, 3], 0, 1).astype(np.float64)
    fused = np.maximum((0.75 * v + np.float64(np.float32(1.3)) * a[:, 1]), 0).astype(np.float32)
    assert not np.array_equal(fused, R.ewa_raw(a, 3, 1, 0.75, 1.3))
    assert not np.array_equal(R.ewa_raw(a, 3, 1, 1.3, 0.75), R.ewa_raw(a, 3, 1, 0.75, 1.3))


def _close(got, want, what, tol=1e-5):
    """test_gpu_cred.py's comparison (norm-wise and max-wise)."""
    got = got.detach().double().cpu().numpy()
    want = np.asarray(want, np.float64)
    err = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
    assert err <= tol and np.abs(got - want).max() <= tol * max(np.abs(want).max(), 1e-30), \
        (what, err)


def _small_graph(nu, ni, E, seed):
    rng = np.random.default_rng(seed)
    src = np.concatenate([rng.integers(0, nu, E), rng.integers(0, nu, 300)])
    dst = np.concatenate([rng.integers(0, ni - 1, E), np.zeros(300, np.int64)])   # a hub
    src = np.concatenate([src, src[:20]])
    dst = np.concatenate([dst, dst[:20]])
    ea = rng.uniform(-0.5, 1.5, (src.size, 5)).astype(np.float32)
    return np.stack([src, dst]), ea


def test_cred_model_with_reordered_keys_and_coefficients():
    """edge_attr_keys in another order (verified in column 3, rating_align in 1)
    with beta = 0.75, gamma = 1.3: forward and parameter gradients of the BCE +
    smoothness loss against CredModelRef with those columns and coefficients,
    at test_gpu_cred.py's tolerances."""
    from bbgr.cred_gnn import CredModel
    from oracle.ref_torch import CredModelRef
    torch.manual_seed(0)
    nu, ni, hidden = 300, 120, 64
    ei, ea = _small_graph(nu, ni, 3000, 11)
    keys = ["rating", "rating_align", "helpful_vote", "verified", "timestamp_norm"]
    ref = CredModelRef(9, 7, hidden, col_verified=3, col_align=1, beta=0.75, gamma=1.3)
    dev = CredModel(9, 7, hidden, edge_attr_keys=keys, beta=0.75, gamma=1.3).to(DEV)
    assert (dev.EDGE_VERIFIED, dev.EDGE_ALIGN) == (3, 1)
    dev.load_state_dict({k: v.to(DEV) for k, v in ref.state_dict().items()})
    x_u, x_i = torch.randn(nu, 9), torch.randn(ni, 7)
    e_u2i = torch.tensor(ei)
    e_i2u = torch.stack([e_u2i[1], e_u2i[0]])
    eat = torch.tensor(ea)
    np.testing.assert_array_equal(dev.ewa_raw(eat.to(DEV)).cpu().numpy(),
                                  ref.ewa_raw(eat).numpy())
    assert not np.array_equal(ref.ewa_raw(eat).numpy(), R.ewa_raw(ea))   # the defaults differ
    outs_r = ref.forward_subgraph(x_u, x_i, e_u2i, eat, e_i2u, eat)
    outs_d = dev.forward_subgraph(x_u.to(DEV), x_i.to(DEV), e_u2i.to(DEV), eat.to(DEV),
                                  e_i2u.to(DEV), eat.to(DEV))
    for a, b, what in zip(outs_d, outs_r, ("cred", "h_u2", "h_i1", "w1t")):
        _close(a, b.detach().numpy(), what, 2e-5)
    y = (torch.rand(nu) > 0.5).float()
    bce = torch.nn.functional.binary_cross_entropy

    def loss_of(outs, yy):
        cred, h_u2, h_i1, w1t = outs
        return bce(cred, yy) + 0.1 * (w1t * (h_u2[e_u2i[0].to(cred.device)] -
                                             h_i1[e_u2i[1].to(cred.device)]).pow(2).sum(-1)).mean()

    loss_of(outs_r, y).backward()
    loss_of(outs_d, y.to(DEV)).backward()
    for (n, p_r), (_, p_d) in zip(ref.named_parameters(), dev.named_parameters()):
        _close(p_d.grad, p_r.grad.numpy(), f"grad {n}", 1e-4)


SPECIAL = np.asarray([np.nan, np.inf, -np.inf, -0.0, 1e-40, 0.0, 1.0, 1.0 + 2.0 ** -23],
                     np.float32)


def _torch_cpu_ewa(attr, cv, ca, beta, gamma):
    """The reference's expressions (main.py:675-678) in torch on the CPU."""
    ea = torch.tensor(attr)
    w = beta * ea[:, cv].clamp(0, 1) + gamma * ea[:, ca]
    return w.clamp(min=0.0).numpy()


@pytest.mark.parametrize("beta,gamma", [(1.0, 1.0)] + COEFFS)
def test_special_values_follow_torch(beta, gamma):
    """NaN, +-inf, -0.0, a denormal, 0, 1 and 1 + 2^-23 in both columns (all 64
    pairs): NaN where torch gives NaN, equal values elsewhere (the sign of a
    zero is not compared)."""
    assert SPECIAL[4] != 0 and SPECIAL[4] < np.finfo(np.float32).tiny   # a denormal
    attr = np.stack([np.repeat(SPECIAL, 8), np.tile(SPECIAL, 8)], 1)
    want = _torch_cpu_ewa(attr, 0, 1, beta, gamma)
    assert np.isnan(want).sum() >= 15 and np.isinf(want).any()
    oracle = R.ewa_raw(attr, 0, 1, beta, gamma)                  # the oracle agrees with torch
    assert np.array_equal(np.isnan(oracle), np.isnan(want))
    assert np.array_equal(oracle[~np.isnan(want)], want[~np.isnan(want)])
    got = normalize_raw(_identity_edges(64), "attr", True, attr=attr, beta=beta,
                        gamma=gamma)["w_raw"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]), (got, want)


@pytest.mark.parametrize("with_dst", [True, False])
@pytest.mark.parametrize("deg", [17, 257, 6145])
@pytest.mark.parametrize("column", [0, 1])
def test_one_nan_edge_poisons_its_destination_only(G, general, deg, column, with_dst):
    """One NaN attribute on one edge of a short row, a one-chunk row or a split
    row: every weight of that destination is NaN, as torch's scatter_add and
    division give; every other destination keeps its bits."""
    attr, raw, res = general
    row = int(np.flatnonzero(G.deg == deg)[0])
    edges = np.flatnonzero(G.ei[1] == row)
    attr = attr.copy()
    attr[edges[len(edges) // 2], column] = np.nan
    got = normalize_raw(G.es, "attr", with_dst, attr=attr)
    base = res[("attr", with_dst)]
    hit = G.ei[1] == row
    assert np.isnan(got["w_raw"]).sum() == 1
    assert np.all(np.isnan(got["w_edge"][hit])) and hit.sum() == deg
    assert np.array_equal(got["w_edge"][~hit], base["w_edge"][~hit])
    hit_csr = hit[G.perm]
    assert np.all(np.isnan(got["w_csr"][hit_csr]))
    assert np.array_equal(got["w_csr"][~hit_csr], base["w_csr"][~hit_csr])


# -- aggregation ----------------------------------------------------------------------

def _assert_agg_bound(got, x, ei, w, n_out, what):
    """|got - ref| <= gamma_{deg+1} * sum_e |w_e| |x_e| per output element."""
    got = got.detach().cpu().numpy().astype(np.float64)
    ref = R.aggregate(x, ei, w, n_out)
    mag = R.aggregate(np.abs(x), ei, np.abs(w), n_out)
    deg = np.bincount(ei[1], minlength=n_out)
    err = np.abs(got - ref)
    bound = _gamma(deg + 1)[:, None] * mag
    units = np.divide(err, mag * U, out=np.zeros_like(err), where=mag != 0)
    msg = f"{what}: largest error {units.max():.3f} u of sum |w||x| (row degree " \
          f"{int(deg[np.unravel_index(np.argmax(units), units.shape)[0]])})"
    print(msg)
    assert np.all(err <= bound), msg + f"; {int((err > bound).sum())} elements over the bound"
    assert np.all(got[deg == 0] == 0), what + ": an isolated row is not exactly zero"


@pytest.mark.parametrize("d", [64, 128, 256])
def test_aggregate_forward_elementwise(G, general, d):
    from bbgr.cred_gnn import aggregate
    _, _, res = general
    w = res[("attr", True)]
    w_t, w_c = torch.tensor(w["w_edge"], device=DEV), torch.tensor(w["w_csr"], device=DEV)
    torch.manual_seed(d)
    x = torch.randn(G.n_src, d, device=DEV)
    out = aggregate(x, G.es, w_t, w_c)
    assert out.shape == (G.n_dst, d) and G.deg[0] == 0
    _assert_agg_bound(out, x.cpu().numpy(), G.ei, w["w_edge"], G.n_dst, f"aggregate d={d}")
    # weights in input order only: the permutation path gives the same bits; so does a rerun
    assert torch.equal(aggregate(x, G.es, w_t), out)
    assert torch.equal(aggregate(x, G.es, w_t, w_c), out)


@pytest.mark.parametrize("d", [64, 128, 256])
def test_aggregate_backward_elementwise_on_source_hubs(G, d):
    """The hubs on the source side: by_src has the split rows, and d out / d x is
    the transposed product over it."""
    from bbgr.cred_gnn import aggregate
    rng = np.random.default_rng(5)
    raw = (1.0 - rng.random(G.E)).astype(np.float32)
    raw[rng.random(G.E) < 0.05] = 0.0
    _, w_t, w_c = G.es_f.normalize(w=torch.tensor(raw, device=DEV))
    torch.manual_seed(1000 + d)
    x = torch.randn(G.n_dst, d, device=DEV, requires_grad=True)
    out = aggregate(x, G.es_f, w_t, w_c)
    w = w_t.cpu().numpy()
    _assert_agg_bound(out, x.detach().cpu().numpy(), G.ei_f, w, G.n_src, f"flipped forward d={d}")
    g = torch.randn(G.n_src, d, device=DEV)
    (out * g).sum().backward()
    assert x.grad.shape == (G.n_dst, d)
    _assert_agg_bound(x.grad, g.cpu().numpy(), G.ei, w, G.n_dst, f"d aggregate / d x d={d}")
    x2 = x.detach().clone().requires_grad_(True)
    (aggregate(x2, G.es_f, w_t) * g).sum().backward()          # w_csr=None path, and a rerun
    assert torch.equal(x2.grad, x.grad)


def test_no_edges():
    """E == 0 with rows on both sides: three empty weight tensors, zeros out,
    zeros back."""
    from bbgr.cred_gnn import EdgeSet, aggregate
    es = EdgeSet(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 5, 7)
    for kw in (dict(edge_attr=torch.zeros(0, 5, device=DEV)), dict(w=torch.zeros(0, device=DEV))):
        outs = es.normalize(**kw)
        assert len(outs) == 3 and all(t.shape == (0,) and t.dtype == torch.float32 for t in outs)
    w = outs[1]
    for w_csr in (None, outs[2]):
        x = torch.randn(5, 64, device=DEV, requires_grad=True)
        out = aggregate(x, es, w, w_csr)
        assert out.shape == (7, 64) and not out.any()
        (out * torch.randn(7, 64, device=DEV)).sum().backward()
        assert x.grad.shape == (5, 64) and not x.grad.any()


def test_one_edge():
    from bbgr.cred_gnn import EdgeSet, aggregate
    es = EdgeSet(torch.tensor([[2], [1]], device=DEV), 4, 3)
    attr = np.asarray([[0.7, 0.25, 0, 0, 0]], np.float32)
    w_raw, w_t, w_c = es.normalize(edge_attr=torch.tensor(attr, device=DEV))
    raw = R.ewa_raw(attr)
    np.testing.assert_array_equal(w_raw.cpu().numpy(), raw)
    np.testing.assert_array_equal(w_t.cpu().numpy(), raw / (raw + np.float32(EPS)))
    assert torch.equal(w_t, w_c)
    x = torch.randn(4, 64, device=DEV, requires_grad=True)
    out = aggregate(x, es, w_t, w_c)
    want = torch.zeros(3, 64, device=DEV)
    want[1] = w_t[0] * x.detach()[2]
    assert torch.equal(out, want)
    g = torch.randn(3, 64, device=DEV)
    (out * g).sum().backward()
    want_g = torch.zeros(4, 64, device=DEV)
    want_g[2] = w_t[0] * g[1]
    assert torch.equal(x.grad, want_g)


def test_one_destination_with_5000_edges():
    """A single row of three chunks (n_rows = 1: one short-row block, all of
    whose other 15 row slots are past the end)."""
    from bbgr.cred_gnn import EdgeSet, aggregate
    rng = np.random.default_rng(9)
    E, n_src = 5000, 40
    ei = np.stack([rng.integers(0, n_src, E), np.zeros(E, np.int64)])
    es = EdgeSet(torch.tensor(ei, device=DEV), n_src, 1)
    assert (es.by_dst.n_chunks, es.by_dst.n_split) == (3, 1)
    raw = (1.0 - rng.random(E)).astype(np.float32)
    k = np.full(E, _k_sum(E))
    assert _k_sum(E) == math.ceil(1667 / 256) - 1 + 8 + 2
    ref = R.normalize_per_dst(raw, ei[1], 1, eps=EPS)
    outs = []
    for with_dst in (True, False):
        got = normalize_raw(es, "w_in", with_dst, raw=raw)
        _assert_rel_bound(got["w_edge"], ref, k, f"one destination dst={with_dst}")
        outs.append(got)
    assert np.array_equal(outs[0]["w_edge"], outs[1]["w_edge"])
    assert np.array_equal(outs[0]["w_csr"], outs[1]["w_csr"])
    x = torch.randn(n_src, 128, device=DEV)
    w_t = torch.tensor(outs[0]["w_edge"], device=DEV)
    out = aggregate(x, es, w_t, torch.tensor(outs[0]["w_csr"], device=DEV))
    _assert_agg_bound(out, x.cpu().numpy(), ei, outs[0]["w_edge"], 1, "one destination")


def test_forward_subgraph_without_edges_equals_the_cpu_reference():
    from bbgr.cred_gnn import CredModel
    from oracle.ref_torch import CredModelRef
    torch.manual_seed(3)
    nu, ni = 6, 4
    ref = CredModelRef(9, 7, 64)
    dev = CredModel(9, 7, 64).to(DEV)
    dev.load_state_dict({k: v.to(DEV) for k, v in ref.state_dict().items()})
    x_u, x_i = torch.randn(nu, 9), torch.randn(ni, 7)
    e = torch.zeros(2, 0, dtype=torch.int64)
    ea = torch.zeros(0, 5)
    outs_r = ref.forward_subgraph(x_u, x_i, e, ea, e, ea)
    outs_d = dev.forward_subgraph(x_u.to(DEV), x_i.to(DEV), e.to(DEV), ea.to(DEV), e.to(DEV),
                                  ea.to(DEV))
    for a, b, what in zip(outs_d[:3], outs_r[:3], ("cred", "h_u2", "h_i1")):
        assert a.shape == b.shape
        _close(a, b.detach().numpy(), what, 2e-5)
    assert outs_d[3].shape == outs_r[3].shape == (0,)


def test_aggregate_refuses_other_widths_and_types(G, general):
    from bbgr.cred_gnn import aggregate
    _, _, res = general
    w = torch.tensor(res[("attr", True)]["w_edge"], device=DEV)
    with pytest.raises(ValueError, match="width 64, 128 or 256"):
        aggregate(torch.randn(G.n_src, 48, device=DEV), G.es, w)
    with pytest.raises(ValueError, match="fp32"):
        aggregate(torch.randn(G.n_src, 64, device=DEV, dtype=torch.float64), G.es, w)
