"""GPU: the drop-in step and the evaluation at every embedding width.

The kernels dispatch on the embedding width d in {8, 16, 32, 64, 128, 256}
(csrc/common.h supported_width). The raw SpMM, scatter and BPR entry points are
tested at all six in test_gpu_parity.py; this file runs what is built on top
of them at all six: the four drop-in modules' training step against the
float64 oracle (oracle/ref_numpy), torch.optim.Adam and bbgr.optim.FusedAdam
(also with the step inside the backward), the deferred final tables against
the dense ones, both evaluation protocols, and the errors raised for a width
outside an entry point's set (the table "Embedding widths" in INTEGRATION.md).

Inputs of the step tests: one graph, synthetic_edges(600, 350, 8000, 17,
zipf, 20 duplicate pairs) with synthetic_credibility(600, 5); the user side
averages 13 edges per row (the two-row CSR path at d >= 64), the Zipf head
gives long item rows. Weights default_rng(d).uniform(-0.3, 0.3) as float32 and
a batch of B = 200 from the same generator with users[::7] = users[0]
(repeated rows); a second batch holds one invalid triple (neg[3] = -1).

Tolerances are the suite's own: tables and gradients normwise AND max-abs at
1e-5 (BASELINE "Parity", test_gpu_parity.assert_parity), the loss 1e-5
relative, the first Adam update w1 - w0 normwise at 1e-4
(test_fused_trainer_shapes_vs_oracle), exp_avg after step 1 (= 0.1 g) at 1e-5.
What the fp32 reference restatement (oracle/ref_torch, CPU) itself differs
from the float64 chain by on these inputs, over all six widths, K = 3, both
batches: gradients <= 1.3e-7 normwise and <= 3.2e-7 max-abs for GS, Method A
and Jacobi (lambda_fair = 0.01), 1.2e-7 normwise / 3.0e-7 max-abs for the
symmetric family (margin >= 30x); the first Adam update <= 5.9e-6 normwise
(symmetric: 5.2e-6; margin 17x); the loss <= 1.6e-7 relative.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bbgr import lightgcn as SYM  # noqa: E402
from bbgr import lightgcn_cu as CU  # noqa: E402
from bbgr import lightgcn_cu_pop as V2  # noqa: E402
from bbgr import lightgcn_cu_pop_long_tail_exposure as MA  # noqa: E402
from bbgr._lib import BbgrError  # noqa: E402
from bbgr.graph import BipartiteGraph, Csr  # noqa: E402
from bbgr.synthetic import synthetic_credibility, synthetic_edges  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402

DEV = "cuda"
TOL = 1e-5
U, I, E, B = 600, 350, 8000, 200
REG, LR, LAMBDA_FAIR = 1e-4, 1e-3, 0.01
WIDTHS = (8, 16, 32, 64, 128, 256)
FAMILIES = ("v2_pop", "method_a", "cu_fair", "plain")
UNSUPPORTED = "(?i)unsupported"


def _errors(got, ref):
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else got
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nrm = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    mx = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    return nrm, mx


def assert_parity(got, ref, what, tol=TOL):
    """test_gpu_parity.assert_parity: normwise relative error <= tol AND
    max-abs error <= tol * max|ref|; prints both figures first."""
    nrm, mx = _errors(got, ref)
    print(f"PARITY {what}: normwise {nrm:.3e} max-abs {mx:.3e} (bound {tol:.0e})")
    assert nrm <= tol, f"{what}: normwise rel err {nrm:.3e}"
    assert mx <= tol, f"{what}: max-abs err {mx:.3e}"


def assert_normwise(got, ref, what, tol):
    nrm, _ = _errors(got, ref)
    print(f"PARITY {what}: normwise {nrm:.3e} (bound {tol:.0e})")
    assert nrm <= tol, f"{what}: normwise rel err {nrm:.3e}"


def assert_loss(loss, want, what):
    got = float(loss.detach())
    err = abs(got - want) / abs(want)
    print(f"PARITY {what}: loss rel err {err:.3e} (bound {TOL:.0e})")
    assert err <= TOL, (what, got, want)


# ---------------------------------------------------------------------------
# Inputs and the float64 oracle: computed once, shared, read-only
# ---------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _graph():
    e = synthetic_edges(U, I, E, 17, items="zipf", duplicates=20)
    cred = synthetic_credibility(U, 5)
    return _frozen(e, cred)


@functools.lru_cache(maxsize=None)
def _inputs(d):
    """(u0, i0, the valid batch, the batch with one invalid triple)."""
    rng = np.random.default_rng(d)
    u0 = rng.uniform(-0.3, 0.3, (U, d)).astype(np.float32)
    i0 = rng.uniform(-0.3, 0.3, (I, d)).astype(np.float32)
    users, pos, neg = (rng.integers(0, n, B) for n in (U, I, I))
    users[::7] = users[0]
    bad = neg.copy()
    bad[3] = -1
    _frozen(u0, i0, users, pos, neg, bad)
    return u0, i0, (users, pos, neg), (users, pos, bad)


@functools.lru_cache(maxsize=None)
def _operators(family):
    e, cred = _graph()
    if family in ("v2_pop", "method_a"):
        return R.gs_mats(e, U, I, cred, method_a=family == "method_a")
    if family == "cu_fair":
        return R.j_mats(e, U, I, cred)
    return (R.sym_values(e, U, I),)


def _fair_pop(deg_i):
    """lightgcn_cu.py:583-584 as tests/test_gpu_training_loop.py:_cu writes it."""
    return (deg_i / max(float(deg_i.max()), 1.0)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle(family, d, K, which):
    """The float64 chain of one step on batch `which` (0 valid, 1 with the
    invalid triple): loss, the weight gradients by table name, the finals.

    The invalid triple (neg = -1): bpr_kernel (csrc/train.hip) leaves a triple
    with any id out of range out of the loss and of every gradient but keeps
    G = dloss / batch (P.inv_b = 1 / a->batch, bbgr_bpr_reduce divides by the
    batch too), so the mean divides by B where the oracle, given the B - 1
    valid triples, divides by B - 1: the oracle's loss and gradients are
    rescaled by (B - 1) / B. The Jacobi family's loss is the reference's own
    torch expressions (lightgcn_cu.py:632-648), where index -1 is torch's
    last row: its oracle takes neg = I - 1 there and is not rescaled."""
    u0, i0, *batches = _inputs(d)
    users, pos, neg = batches[which]
    scale = 1.0
    if which == 1 and family == "cu_fair":
        neg = np.where(neg < 0, I - 1, neg)
    elif which == 1:
        keep = neg >= 0
        users, pos, neg = users[keep], pos[keep], neg[keep]
        scale = keep.sum() / B
        assert keep.sum() == B - 1
    ops = _operators(family)
    if family in ("v2_pop", "method_a"):
        A, Bm = ops
        uf, itf, _, _ = R.propagate_gs(A, Bm, u0, i0, K)
        loss, gr = R.bpr_loss(uf, itf, u0, i0, users, pos, neg, REG)
        gu, gi = R.backward_gs(A, Bm, gr["g_uf"], gr["g_if"], K)
        grads = {"user_emb": gu + gr["g_ue"], "item_emb": gi + gr["g_ie"]}
    elif family == "cu_fair":
        A, Bm, deg_i = ops
        uf, itf, _, _ = R.propagate_j(A, Bm, u0, i0, K)
        loss, gr = R.bpr_loss(uf, itf, u0, i0, users, pos, neg, REG, _fair_pop(deg_i),
                              LAMBDA_FAIR)
        gu, gi = R.backward_j(A, Bm, gr["g_uf"], gr["g_if"], K)
        grads = {"user_emb": gu + gr["g_ue"], "item_emb": gi + gr["g_ie"]}
    else:
        (A,) = ops
        xf, _ = R.propagate_sym(A, np.vstack([u0, i0]), K)
        uf, itf = xf[:U], xf[U:]
        loss, gr = R.bpr_loss(uf, itf, u0, i0, users, pos, neg, REG)
        g = R.backward_sym(A, np.vstack([gr["g_uf"], gr["g_if"]]), K)
        grads = {"emb": g + np.vstack([gr["g_ue"], gr["g_ie"]])}
    grads = {k: v * scale for k, v in grads.items()}
    _frozen(uf, itf, *grads.values())
    return loss * scale, grads, (uf, itf)


def _weights(d):
    u0, i0, _, _ = _inputs(d)
    return {"user_emb": u0, "item_emb": i0, "emb": np.vstack([u0, i0])}


def _dev(a, dtype=torch.long):
    return torch.tensor(np.asarray(a), device=DEV, dtype=dtype)


def _dropin(family, d, K=3):
    """(model with the inputs' weights, {table name: parameter}, the step as the
    family's script writes it, the finals as that script reads them)."""
    e, cred = _graph()
    e, cred = e.copy(), cred.copy()
    if family in ("v2_pop", "method_a"):
        mod = V2 if family == "v2_pop" else MA
        M_ui, M_iu = mod.build_message_passing_mats(e, U, I, torch.as_tensor(cred), DEV)
        m = mod.LightGCN(U, I, d, K, M_ui, M_iu).to(DEV)
        tables = {"user_emb": m.user_emb.weight, "item_emb": m.item_emb.weight}
    elif family == "cu_fair":
        M_ui, M_iu, deg_i = CU.build_cred_weighted_mats(e, U, I, cred, DEV)
        pop_t = torch.tensor(_fair_pop(deg_i), device=DEV)
        m = CU.CredLightGCN(U, I, d, K, M_ui, M_iu).to(DEV)
        tables = {"user_emb": m.user_emb.weight, "item_emb": m.item_emb.weight}
    else:
        m = SYM.LightGCN(U, I, d, K, SYM.build_norm_adj(e, U, I, DEV)).to(DEV)
        tables = {"emb": m.emb.weight}
    w = _weights(d)
    with torch.no_grad():
        for name, p in tables.items():
            p.copy_(_dev(w[name], torch.float32))

    if family == "cu_fair":
        def step(users_t, pos_t, neg_t, reg):   # lightgcn_cu.py:632-648, as written there
            e_u, e_i = m.final_embeddings()
            pos_scores = m.score(users_t, pos_t, e_u, e_i)
            neg_scores = m.score(users_t, neg_t, e_u, e_i)
            loss_bpr = -torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-12).mean()
            loss_fair = (pop_t[pos_t] * pos_scores).mean()
            loss_reg = m.l2_reg(users_t, pos_t, neg_t)
            return loss_bpr + LAMBDA_FAIR * loss_fair + reg * loss_reg
        finals = m.final_embeddings
    else:
        def step(users_t, pos_t, neg_t, reg):   # Version-2/lighgcn_cu_pop.py:858-859
            user_emb, item_emb = m.get_user_item_emb()
            return m.bpr_loss(users_t, pos_t, neg_t, user_emb, item_emb, reg)
        finals = m.get_user_item_emb
    return m, tables, step, finals


# ---------------------------------------------------------------------------
# (a) the eager drop-in step vs the float64 chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("family", FAMILIES)
def test_dropin_first_step_vs_float64(family, d):
    """The reference's loop body, unchanged and eager with default settings
    (deferred finals, the sparse-ego BPR backward and the rows backward for the
    GS families), at every width: the loss (1e-5 relative) and every weight
    gradient (normwise and max-abs 1e-5) against the float64 chain, on the
    valid batch and on the batch with one invalid triple (_oracle's docstring
    pins how each family treats it); then the finals read as whole tables."""
    m, tables, step, finals = _dropin(family, d)
    _, _, *batches = _inputs(d)
    for which, batch in enumerate(batches):
        want, grads, _ = _oracle(family, d, 3, which)
        m.zero_grad(set_to_none=True)
        loss = step(*(_dev(x) for x in batch), REG)
        loss.backward()
        what = f"{family} d={d} batch {which}"
        assert_loss(loss, want, what)
        for name, p in tables.items():
            assert p.grad is not None and not p.grad.is_sparse, name
            assert_parity(p.grad, grads[name], f"{what} grad {name}")
    uf, itf = finals()
    _, _, (ruf, ritf) = _oracle(family, d, 3, 0)
    assert_parity(uf + 0, ruf, f"{family} d={d} u_final")
    assert_parity(itf + 0, ritf, f"{family} d={d} i_final")


# ---------------------------------------------------------------------------
# (b) deferred finals vs the dense step, bit for bit
# ---------------------------------------------------------------------------
def _three_batches(d):
    _, _, b0, b1 = _inputs(d)
    rng = np.random.default_rng(100 + d)
    b2 = (rng.permutation(U)[:B], rng.integers(0, I, B), rng.integers(0, I, B))   # distinct users
    return [tuple(_dev(x) for x in b) for b in (b0, b1, b2)]


def _steps(m, batches):
    """The reference's loop body (Version-2:858-863) over the batches."""
    opt = torch.optim.Adam(m.parameters(), lr=LR)
    out = []
    for users, pos, neg in batches:
        user_emb, item_emb = m.get_user_item_emb()
        loss = m.bpr_loss(users, pos, neg, user_emb, item_emb, REG)
        opt.zero_grad()
        loss.backward()
        grads = [p.grad.clone() for p in m.parameters()]
        opt.step()
        out.append((float(loss), grads))
    return out


@pytest.mark.parametrize("d", [8, 32, 128, 256])
def test_deferred_step_is_bitwise_the_dense_step_at_width(d):
    """Three reference steps with lazy_finals on (batch rows only) vs off
    (whole tables) at the widths test_gpu_lazy.py (d = 64) leaves out: losses,
    gradients and weights equal bit for bit, for Version-2 at K = 3 and K = 1
    and for Method A at K = 3; repeated users, distinct users and an invalid
    triple among the batches."""
    batches = _three_batches(d)
    for family, K in (("v2_pop", 3), ("v2_pop", 1), ("method_a", 3)):
        a, b = _dropin(family, d, K)[0], _dropin(family, d, K)[0]
        a.lazy_finals, b.lazy_finals = True, False
        for k, ((la, ga), (lb, gb)) in enumerate(zip(_steps(a, batches), _steps(b, batches))):
            assert la == lb, (family, K, k)
            for x, y in zip(ga, gb):
                assert torch.equal(x, y), (family, K, k)
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert torch.equal(pa, pb), (family, K)


# ---------------------------------------------------------------------------
# (c) the optimizers' first step vs the float64 chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("opt,K", [("torch", 3), ("fused", 3), ("fused_backward", 2),
                                   ("fused_backward", 3)])
def test_dropin_optimizers_vs_float64(opt, K, d):
    """One Version-2 step with torch.optim.Adam, bbgr.optim.FusedAdam and
    FusedAdam(fuse_backward=True) (the step inside loss.backward(): GS order,
    K >= 2) at every width against the float64 oracle: the loss, the update
    w1 - w0 normwise at 1e-4, and exp_avg (= 0.1 g after step 1) at the
    gradient's 1e-5, so that a miss of the update bound alone points at
    near-zero components and not at the gradient. The in-backward leg leaves
    no .grad on the stepped tables."""
    from bbgr.optim import FusedAdam
    m, tables, step, _ = _dropin("v2_pop", d, K)
    if opt == "torch":
        o = torch.optim.Adam(m.parameters(), lr=LR)
    else:
        o = FusedAdam(m.parameters(), lr=LR, fuse_backward=opt == "fused_backward")
    _, _, batch, _ = _inputs(d)
    want, grads, _ = _oracle("v2_pop", d, K, 0)
    loss = step(*(_dev(x) for x in batch), REG)
    o.zero_grad()
    loss.backward()
    if opt == "fused_backward":
        assert all(p.grad is None for p in tables.values())
    o.step()
    what = f"{opt} K={K} d={d}"
    assert_loss(loss, want, what)
    w = _weights(d)
    for name, p in tables.items():
        z = np.zeros_like(grads[name])
        w1, m1, _ = R.adam_step(w[name], grads[name], z, z, 1, lr=LR)
        exp_avg = o.state[p]["exp_avg"] if opt == "torch" else o.moments(p)[0]
        assert_parity(exp_avg, m1, f"{what} exp_avg {name}")
        got = p.detach().double().cpu().numpy() - w[name].astype(np.float64)
        assert_normwise(got, w1 - w[name], f"{what} update {name}", 1e-4)
        assert int(o.state[p]["step"]) == 1


# ---------------------------------------------------------------------------
# FusedTrainer below d = 64 for the other two variants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["cu_fair", "method_a"])
def test_fused_trainer_step_vs_oracle_at_d32(variant):
    """test_gpu_parity.test_fused_trainer_step_vs_oracle's check at d = 32 on
    this file's graph: loss, the weight gradients fed to Adam (1e-5), the Adam
    update normwise (1e-4), the sparse gradient tables zero again."""
    from bbgr.trainer import FusedTrainer
    d, K = 32, 3
    e, cred = _graph()
    u0, i0, _, _ = _inputs(d)
    lam = 0.05 if variant == "cu_fair" else 0.0
    tr = FusedTrainer(BipartiteGraph(e.copy(), U, I, DEV), variant, cred=cred.copy(), emb_dim=d,
                      num_layers=K, batch_size=B, lambda_fair=lam, u0=u0.copy(), i0=i0.copy(),
                      fuse_adam=False, frontier=True)
    users = tr.next_users()
    loss = tr.step(users)
    n = users.numel()
    uu, pos, neg = users.cpu().numpy(), tr.pos[:n].cpu().numpy(), tr.neg[:n].cpu().numpy()
    assert (neg >= 0).all()
    if variant == "cu_fair":
        A, Bm, deg_i = _operators("cu_fair")
        uf, itf, _, _ = R.propagate_j(A, Bm, u0, i0, K)
        pop = deg_i / max(deg_i.max(), 1.0)
        want, gr = R.bpr_loss(uf, itf, u0, i0, uu, pos, neg, REG, pop, lam)
        gu0, gi0 = R.backward_j(A, Bm, gr["g_uf"], gr["g_if"], K)
    else:
        A, Bm = _operators("method_a")
        uf, itf, _, _ = R.propagate_gs(A, Bm, u0, i0, K)
        want, gr = R.bpr_loss(uf, itf, u0, i0, uu, pos, neg, REG)
        gu0, gi0 = R.backward_gs(A, Bm, gr["g_uf"], gr["g_if"], K)
    gu0, gi0 = gu0 + gr["g_ue"], gi0 + gr["g_ie"]
    assert_loss(loss, want, f"trainer {variant} d=32")
    assert_parity(tr.g_u0, gu0, f"trainer {variant} d=32 grad u0")
    assert_parity(tr.g_i0, gi0, f"trainer {variant} d=32 grad i0")
    z = np.zeros_like
    pu, _, _ = R.adam_step(u0, gu0, z(gu0), z(gu0), 1)
    pi, _, _ = R.adam_step(i0, gi0, z(gi0), z(gi0), 1)
    for got, ref, name in ((tr.user_w - _dev(u0, torch.float32), pu - u0, "user update"),
                           (tr.item_w - _dev(i0, torch.float32), pi - i0, "item update")):
        assert_normwise(got, ref, f"trainer {variant} d=32 {name}", 1e-4)
    assert tr.g_uf.abs().sum().item() == 0 and tr.g_if.abs().sum().item() == 0


# ---------------------------------------------------------------------------
# (d), (e) evaluation
# ---------------------------------------------------------------------------
def _split(n_users, n_items, n_edges, seed):
    e = synthetic_edges(n_users, n_items, n_edges, seed, items="zipf")
    test = np.random.default_rng(seed).random(e.shape[1]) < 0.2
    return e[:, ~test], e[:, test]


@functools.lru_cache(maxsize=None)
def _eval_graph():
    tr, te = _split(300, 900, 6000, 5)
    return _frozen(tr, te)


def _eval_inputs():
    """(train edges, test edges, item popularity, credibility) of the 300 x 900
    evaluation graph; the last two fresh (the package wraps them as tensors)."""
    tr, te = _eval_graph()
    return tr, te, np.bincount(tr[1], minlength=900), synthetic_credibility(300, 5)


@pytest.mark.parametrize("n_neg", [1, 5, 127, 128, 255])
@pytest.mark.parametrize("d", WIDTHS)
def test_eval_sampled_exact_at_width_and_capacity(d, n_neg):
    """test_eval_sampled_ranks_and_lists_exact_with_ties' method at every width
    evaluate_sampled accepts (d < 64 zero-padded to 64 columns, which adds
    exact zeros) and at candidate counts below the gather batch (1 and 5
    negatives), on both sides of the kernel's LDS capacity switch (1 + 127 =
    128 candidates, 1 + 128) and at the ABI maximum (1 + 255 = 256): integer
    embeddings in [-2, 2] make every score an exact fp32 integer (|s| <= 4 d
    <= 1024), so the positive's rank and the top-k lists must be exactly the
    stable descending order (score desc, candidate slot asc); list entries
    past the candidate count stay -1."""
    from bbgr.evaluation import evaluate_sampled
    nu, ni, Ks = 300, 900, (1, 10)
    tr, te, pop, cred = _eval_inputs()
    rng = np.random.default_rng(1000 * d + n_neg)
    uf = rng.integers(-2, 3, size=(nu, d)).astype(np.float32)
    itf = rng.integers(-2, 3, size=(ni, d)).astype(np.float32)
    res = evaluate_sampled(_dev(uf, torch.float32), _dev(itf, torch.float32),
                           Csr(tr[0], tr[1], nu, ni, DEV), Csr(te[0], te[1], nu, ni, DEV), ni,
                           pop, int(tr.shape[1]), cred, Ks=Ks, sampled_negatives=n_neg,
                           return_raw=True)
    raw = res.pop("_raw")
    assert raw["fails"] == 0
    users = raw["users"].cpu().numpy()
    nc, km = 1 + n_neg, max(Ks)
    cand = raw["cand"].cpu().numpy()
    assert cand.shape == (users.size, nc) and users.size > 200
    assert (cand >= 0).all() and (cand < ni).all()
    pos_rank = raw["pos_rank"].cpu().numpy()
    topk = raw["topk"].cpu().numpy()
    s = np.einsum("ncd,nd->nc", itf[cand].astype(np.int64), uf[users].astype(np.int64))
    order = np.lexsort((np.broadcast_to(np.arange(nc), s.shape), -s), axis=1)   # score desc, slot asc
    np.testing.assert_array_equal(pos_rank, np.argmax(order == 0, axis=1))
    want = np.full((users.size, km), -1, np.int64)
    want[:, : min(km, nc)] = np.take_along_axis(cand, order[:, :km], axis=1)
    np.testing.assert_array_equal(topk, want)
    if nc >= 100:
        assert (nc - np.array([np.unique(r).size for r in s])).sum() > users.size * 10   # tie-heavy
    for K in Ks:   # gt = {pos}: recall@K is the share of users ranking it below K
        assert res[K]["recall"] == pytest.approx(float((pos_rank < K).mean()), abs=1e-12)
        assert res[K]["users_eval"] == users.size and res[K]["negatives"] == n_neg


def _full_case(n_users, n_items, n_edges, d, seed):
    """test_gpu_eval._full_case with its heavy user: user 0 has trained all but
    5 items, so its top-16 ends in -1e9 entries."""
    tr, te = _split(n_users, n_items, n_edges, seed)
    keep = tr[0] != 0
    tr = np.concatenate([tr[:, keep], np.stack([np.zeros(n_items - 5, np.int32),
                                                np.arange(5, n_items, dtype=np.int32)])], axis=1)
    te = np.concatenate([te[:, te[0] != 0], np.array([[0], [1]], np.int32)], axis=1)
    rng = np.random.default_rng(seed + 1)
    uf = rng.normal(size=(n_users, d)).astype(np.float32)
    itf = rng.normal(size=(n_items, d)).astype(np.float32)
    return tr, te, uf, itf


@pytest.mark.parametrize("d", [8, 16, 32, 64, 128])
def test_eval_full_bitexact_vs_c_oracle_at_width(d):
    """test_eval_full_bitexact_vs_c_oracle's method at every width
    evaluate_full accepts: top-K ids and scores bit-identical to the C oracle's
    fma chain (oracle/csrc/eval_full.c) run at the TRUE width. Below d = 64 the
    tables are evaluated zero-padded to 64 columns with the two halves of the
    d columns at columns 0 and 32 (evaluation._pad_narrow), so the kernel's
    chain (components 0, 32, 1, 33, ...) meets them in the true width's order
    (0, d/2, 1, d/2 + 1, ...) and then only zeros: each extra fma(0, 0, acc)
    returns acc, so no score changes, except a score of exactly -0.0 (which
    would become +0.0), and normal-distributed inputs do not produce one."""
    from bbgr.evaluation import evaluate_full
    from oracle import native as N
    nu, ni, Ks = 300, 777, (16,)
    tr, te, uf, itf = _full_case(nu, ni, 20 * nu, d, 11)
    pop = np.bincount(tr[1], minlength=ni)
    cred = synthetic_credibility(nu, 4)
    res = evaluate_full(_dev(uf, torch.float32), _dev(itf, torch.float32),
                        Csr(tr[0], tr[1], nu, ni, DEV), Csr(te[0], te[1], nu, ni, DEV), ni, pop,
                        int(tr.shape[1]), cred, Ks=Ks, return_raw=True)
    raw = res.pop("_raw")
    users = raw["users"].cpu().numpy()
    topk = raw["topk"].cpu().numpy()
    score = raw["topk_score"].cpu().numpy()
    tr_ptr, tr_idx = R.edges_to_user_csr(tr, nu)
    te_ptr, te_idx = R.edges_to_user_csr(te, nu)
    o_items, o_scores = N.full_topk(users, tr_ptr, tr_idx, uf, itf, max(Ks))
    o_items = np.where(np.isneginf(o_scores), -1, o_items)
    np.testing.assert_array_equal(topk, o_items)
    np.testing.assert_array_equal(score.view(np.uint32), o_scores.view(np.uint32))
    flags = raw["groups"].cpu().numpy()
    ref = R.evaluate_given_topk(users, o_items, te_ptr, te_idx, pop, int(tr.shape[1]), ni, cred,
                                users[flags & 1 > 0], users[flags & 2 > 0], Ks=Ks)
    for K in Ks:
        for k in ref[K]:
            assert res[K][k] == pytest.approx(ref[K][k], rel=1e-9, abs=1e-12), (K, k)
        assert res[K]["mode"] == "full" and res[K]["users_eval"] == users.size


@pytest.mark.parametrize("family", FAMILIES)
def test_narrow_model_evaluates_with_its_modules_functions(family):
    """A drop-in model at d = 16 calls its own module's evaluate_sampled /
    evaluate_full_ranking (the reference's signatures): the results are
    bbgr.evaluation's on the model's final tables, which the float64 oracle
    reproduces on the same candidates (hit metrics within 2 users: fp32 vs
    float64 near-ties)."""
    from bbgr import evaluation as EV
    from bbgr import host_sampler as HS
    d = 16
    m, _, _, finals = _dropin(family, d)
    mod = {"v2_pop": V2, "method_a": MA, "cu_fair": CU, "plain": SYM}[family]
    e, cred = _graph()
    test = np.random.default_rng(3).random(e.shape[1]) < 0.2
    tr, te = e[:, ~test], e[:, test]
    tr_csr, te_csr = HS.edges_to_user_csr(tr, U), HS.edges_to_user_csr(te, U)
    pop = np.bincount(tr[1].astype(np.int64), minlength=I).astype(np.float32)
    extra = (pop, int(tr.shape[1]), cred.copy()) if family == "v2_pop" else ()
    got = EV.evaluate_sampled_reference(m, tr_csr, te_csr, I, DEV, *extra, return_raw=True)
    raw = got.pop("_raw")
    exp = mod.evaluate_sampled(m, tr_csr, te_csr, I, DEV, *extra)
    with torch.no_grad():
        uf, itf = (torch.as_tensor(x + 0).cpu().numpy() for x in finals())
    users, cand = raw["users"].cpu().numpy(), raw["cand"].cpu().numpy()
    flags = raw["groups"].cpu().numpy()
    r_cred = cred if family == "v2_pop" else np.ones(U, np.float32)
    ref = R.evaluate_sampled_given(users, cand, uf, itf, pop, int(tr.shape[1]), I, r_cred,
                                   users[flags & 1 > 0], users[flags & 2 > 0], Ks=(10, 20))
    n = users.size
    for K in (10, 20):
        assert exp[K] == got[K]
        for k in ("precision", "recall", "ndcg"):
            assert abs(got[K][k] - ref[K][k]) <= 2.0 / n + 1e-6, (family, K, k)
        assert got[K]["users_eval"] == n
    if hasattr(mod, "evaluate_full_ranking"):
        full = mod.evaluate_full_ranking(m, tr_csr, te_csr, I, DEV, *extra)
        assert sorted(full) == [10, 20] and full[10]["mode"] == "full"
        assert full[10]["users_eval"] == n and 0.0 <= full[20]["recall"] <= 1.0


# ---------------------------------------------------------------------------
# (f) the width contract (INTEGRATION.md "Embedding widths")
# ---------------------------------------------------------------------------
def _eval_call(fn, d):
    nu, ni = 300, 900
    tr, te, pop, cred = _eval_inputs()
    g = torch.Generator().manual_seed(d)
    uf, itf = torch.randn(nu, d, generator=g).to(DEV), torch.randn(ni, d, generator=g).to(DEV)
    return fn(uf, itf, Csr(tr[0], tr[1], nu, ni, DEV), Csr(te[0], te[1], nu, ni, DEV), ni, pop,
              int(tr.shape[1]), cred)


@pytest.mark.parametrize("d", [48, 4, 512])
def test_width_contract_evaluation(d):
    """evaluate_sampled: d in {8, 16, 32, 64, 128, 256}; evaluate_full: d in
    {8, 16, 32, 64, 128}. Any other width raises BbgrError naming
    BBGR_ERR_UNSUPPORTED from the entry point, before any launch."""
    from bbgr.evaluation import evaluate_full, evaluate_sampled
    for fn in (evaluate_sampled, evaluate_full):
        with pytest.raises(BbgrError, match=UNSUPPORTED) as ei:
            _eval_call(fn, d)
        assert ei.value.rc == -2
    torch.cuda.synchronize()


def test_width_contract_eval_full_at_256():
    """bbgr_eval_full has no d = 256 form (FullShape<256> is separate kernel
    work): evaluate_full, and a d = 256 model's evaluate_full_ranking, raise
    the clean UNSUPPORTED error; its evaluate_sampled works."""
    from bbgr import host_sampler as HS
    from bbgr.evaluation import evaluate_full
    with pytest.raises(BbgrError, match=UNSUPPORTED) as ei:
        _eval_call(evaluate_full, 256)
    assert ei.value.rc == -2
    m = _dropin("v2_pop", 256)[0]
    e, cred = _graph()
    test = np.random.default_rng(3).random(e.shape[1]) < 0.2
    tr, te = e[:, ~test], e[:, test]
    tr_csr, te_csr = HS.edges_to_user_csr(tr, U), HS.edges_to_user_csr(te, U)
    extra = (np.bincount(tr[1].astype(np.int64), minlength=I).astype(np.float32),
             int(tr.shape[1]), cred.copy())
    with pytest.raises(BbgrError, match=UNSUPPORTED):
        V2.evaluate_full_ranking(m, tr_csr, te_csr, I, DEV, *extra)
    res = V2.evaluate_sampled(m, tr_csr, te_csr, I, DEV, *extra)
    assert res[10]["users_eval"] > 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", FAMILIES)
def test_width_contract_modules_at_48(family):
    """propagate / bpr_loss / the modules' evaluation at d = 48 (outside
    {8, 16, 32, 64, 128, 256}): the finals read as whole tables, the
    reference's step, and the module's evaluate_* each raise the op layer's
    RuntimeError (or BbgrError, a RuntimeError) naming the unsupported width;
    the weights are untouched and the device is healthy afterwards."""
    from bbgr import host_sampler as HS
    d = 48
    e, cred = _graph()
    e, cred = e.copy(), cred.copy()
    torch.manual_seed(0)
    if family in ("v2_pop", "method_a"):
        mod = V2 if family == "v2_pop" else MA
        m = mod.LightGCN(U, I, d, 3, *mod.build_message_passing_mats(
            e, U, I, torch.as_tensor(cred), DEV)).to(DEV)
        finals = m.get_user_item_emb
    elif family == "cu_fair":
        mod = CU
        M_ui, M_iu, _ = CU.build_cred_weighted_mats(e, U, I, cred, DEV)
        m = CU.CredLightGCN(U, I, d, 3, M_ui, M_iu).to(DEV)
        finals = m.final_embeddings
    else:
        mod = SYM
        m = SYM.LightGCN(U, I, d, 3, SYM.build_norm_adj(e, U, I, DEV)).to(DEV)
        finals = m.get_user_item_emb
    w0 = [p.detach().clone() for p in m.parameters()]
    _, _, batch, _ = _inputs(8)
    users, pos, neg = (_dev(x) for x in batch)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        uf, itf = finals()
        uf + 0
    if family != "cu_fair":   # (its step is torch expressions over final_embeddings())
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            uf, itf = m.get_user_item_emb()
            m.bpr_loss(users, pos, neg, uf, itf, REG).backward()
    tr_csr = HS.edges_to_user_csr(e, U)
    extra = (np.bincount(e[1].astype(np.int64), minlength=I).astype(np.float32),
             int(e.shape[1]), cred) if family == "v2_pop" else ()
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        mod.evaluate_sampled(m, tr_csr, tr_csr, I, DEV, *extra)
    if hasattr(mod, "evaluate_full_ranking"):
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            mod.evaluate_full_ranking(m, tr_csr, tr_csr, I, DEV, *extra)
    torch.cuda.synchronize()
    for p, w in zip(m.parameters(), w0):
        assert torch.equal(p.detach(), w) and p.grad is None


def test_width_contract_bpr_loss_at_48():
    """bbgr.bpr.bpr_loss on plain d = 48 tables (bbgr::bpr_loss): UNSUPPORTED."""
    from bbgr import bpr
    d = 48
    g = torch.Generator().manual_seed(d)
    uf, ue = (torch.randn(U, d, generator=g).to(DEV).requires_grad_() for _ in range(2))
    itf, ie = (torch.randn(I, d, generator=g).to(DEV).requires_grad_() for _ in range(2))
    _, _, batch, _ = _inputs(8)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        bpr.bpr_loss(*(_dev(x) for x in batch), uf, itf, ue, ie, REG)
    torch.cuda.synchronize()


def test_width_contract_fused_trainer_and_fused_backward_at_48():
    """FusedTrainer and FusedAdam(fuse_backward=True) at d = 48: the first step
    raises UNSUPPORTED (BbgrError from the C ABI, RuntimeError from the op
    layer) and no weight has moved."""
    from bbgr.optim import FusedAdam
    from bbgr.trainer import FusedTrainer
    d = 48
    e, cred = _graph()
    e, cred = e.copy(), cred.copy()
    rng = np.random.default_rng(d)
    u0 = rng.uniform(-0.3, 0.3, (U, d)).astype(np.float32)
    i0 = rng.uniform(-0.3, 0.3, (I, d)).astype(np.float32)
    with pytest.raises(BbgrError, match=UNSUPPORTED) as ei:
        tr = FusedTrainer(BipartiteGraph(e, U, I, DEV), "v2_pop", cred=cred, emb_dim=d,
                          num_layers=3, batch_size=B, u0=u0, i0=i0)
        tr.step()
    assert ei.value.rc == -2
    torch.manual_seed(0)
    m = V2.LightGCN(U, I, d, 3, *V2.build_message_passing_mats(
        e, U, I, torch.as_tensor(cred), DEV)).to(DEV)
    w0 = [p.detach().clone() for p in m.parameters()]
    o = FusedAdam(m.parameters(), lr=LR, fuse_backward=True)
    _, _, batch, _ = _inputs(8)
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        uf, itf = m.get_user_item_emb()
        loss = m.bpr_loss(*(_dev(x) for x in batch), uf, itf, REG)
        o.zero_grad()
        loss.backward()
        o.step()
    torch.cuda.synchronize()
    for p, w in zip(m.parameters(), w0):
        assert torch.equal(p.detach(), w)
