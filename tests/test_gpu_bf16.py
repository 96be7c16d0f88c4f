"""GPU: the opt-in bf16 forward (bbgr_to_bf16, bbgr_spmm_bf16,
forward(table_dtype=torch.bfloat16), FusedTrainer(forward_dtype="bf16")).

The contract is the summation order: a bf16-source product is, element for
element, the fp32 kernel's product on the source widened to fp32, so its fp32
outputs are compared BITWISE with the existing kernels on `x.bfloat16().float()`
and its bf16 output with their fp32 output rounded once. Independent of the
project's kernels, the same outputs are held to scipy float64 products of the
rounded source at the fp32 tolerance (no rounding decision lies between the
two), the chain to a float64 chain with the roundings restated in numpy, and
the training step's gradients to the float64 adjoint at the step's own final
tables."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bbgr import _lib  # noqa: E402
from bbgr import propagate as P  # noqa: E402
from bbgr._lib import OP_GS, OP_J  # noqa: E402
from bbgr.graph import BipartiteGraph, Csr  # noqa: E402
from bbgr.synthetic import synthetic_credibility, synthetic_edges  # noqa: E402
from bbgr.trainer import FusedTrainer, GraphedStep  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402
from test_bf16_abi import rne_bits, rne_values  # noqa: E402
from test_gpu_parity import TOL, assert_parity  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(DEV, dtype)


def bits(x: torch.Tensor) -> torch.Tensor:
    return x.contiguous().view(torch.int16)


def widen(b: np.ndarray) -> np.ndarray:
    """fp32 values of bf16 bit patterns."""
    return (b.astype(np.uint32) << 16).view(np.float32)


def rb(x: np.ndarray) -> np.ndarray:
    """float64 -> the bf16 value the device stores (through fp32, nearest even)."""
    return widen(rne_bits(np.ascontiguousarray(x, np.float32))).astype(np.float64)


# ---------------------------------------------------------------------------
# 1. conversion
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 256])
def test_to_bf16_bits_are_torchs_and_padding_is_untouched(d):
    n = 37
    v = rne_values()
    vals = np.concatenate([v[-16:], v[:n * d - 16]]).reshape(n, d)   # the edge cases first
    src = torch.full((n, d + 4), float("nan"), device=DEV)
    src[:, :d] = t(vals)
    dst = torch.full((n, d + 8), -7.0, dtype=BF, device=DEV)
    _lib.call("bbgr_to_bf16", n, d, src.data_ptr(), d + 4, dst.data_ptr(), d + 8,
              _lib.stream_handle())
    torch.cuda.synchronize()
    want = torch.from_numpy(vals).to(BF)                       # torch's CPU conversion
    assert torch.equal(bits(dst[:, :d].cpu()), bits(want))
    assert np.array_equal(bits(dst[:, :d].cpu()).numpy().view(np.uint16), rne_bits(vals))
    assert torch.equal(bits(dst[:, :d]), bits(src[:, :d].to(BF)))   # and the device conversion
    assert (dst[:, d:].float() == -7.0).all()
    # NaN stays NaN
    src[:, :d] = float("nan")
    P.to_bf16(src[:, :d], dst[:, :d])
    assert torch.isnan(dst[:, :d].float()).all() and (dst[:, d:].float() == -7.0).all()


# ---------------------------------------------------------------------------
# 2. product against the fp32 kernel and against scipy float64
# ---------------------------------------------------------------------------
def _product_case(rows, cols, n_rows, n_cols, d, mode, seed, **csr_kw):
    rng = np.random.default_rng(seed)
    vals = rng.uniform(0.1, 1.0, rows.size).astype(np.float32)
    c = Csr(rows, cols, n_rows, n_cols, DEV, edge_values=t(vals) if mode == 1 else None, **csr_kw)
    prod = P.Product(c, c.values if mode == 1 else None, None, None, {})
    x = rng.uniform(-1, 1, (n_cols, d)).astype(np.float32)
    w = vals if mode == 1 else np.ones(rows.size, np.float32)
    ep = dict(ys=rng.uniform(0.5, 1.5, n_rows).astype(np.float32),
              acc_in=rng.normal(size=(n_rows, d)).astype(np.float32),
              accs=rng.uniform(0.5, 1.5, n_rows).astype(np.float32))
    return c, prod, x, w, ep


def _both(prod, xb, ep, n_rows, d, **kw):
    """(y bf16, acc) of the bf16 entry and (y fp32, acc) of the fp32 entry on
    the widened source, same epilogue arguments; outputs prefilled with sentinels."""
    out = []
    for x, ydt in ((xb, BF), (xb.float(), torch.float32)):
        y = torch.full((n_rows, d), 3.0, dtype=ydt, device=DEV)
        acc = torch.full((n_rows, d), -5.0, device=DEV)
        P.spmm(prod, x, True, y=y, y_scale=t(ep["ys"]), y_scale_s=0.75, acc_in=t(ep["acc_in"]),
               acc_out=acc, acc_scale=t(ep["accs"]), acc_scale_s=1.25, gamma=0.25, **kw)
        out += [y, acc]
    torch.cuda.synchronize()
    return out


def _check_product(prod, rows, cols, w, x, ep, n_rows, n_cols, d):
    xb = t(x).to(BF)
    yb, accb, y32, acc32 = _both(prod, xb, ep, n_rows, d)
    assert torch.equal(accb, acc32), "acc_out is not bitwise the fp32 kernel's on the widened x"
    assert torch.equal(bits(yb), bits(y32.to(BF))), "y is not the fp32 y rounded once"
    # independent yardstick: float64 product of the rounded source
    Tm = R.csr64(rows, cols, w, (n_rows, n_cols)) @ xb.float().double().cpu().numpy()
    want = 0.25 * (ep["acc_in"] + 1.25 * ep["accs"][:, None] * Tm)
    assert_parity(accb, want, "acc vs float64", TOL)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("thr", [256, 8])
def test_spmm_bf16_item_rows_bitwise_fp32_kernel(d, mode, thr):
    R_, C_ = 400, 350
    e = synthetic_edges(C_ - 3, R_ - 3, 9000, 7, items="zipf", duplicates=20)
    rows, cols = e[1], e[0]                     # item rows (skewed)
    c, prod, x, w, ep = _product_case(rows, cols, R_, C_, d, mode, d + mode + thr,
                                      long_threshold=thr, chunk_edges=32)
    if thr == 8:
        assert c.n_split > 0 and c.n_chunks > c.n_split
    _check_product(prod, rows, cols, w, x, ep, R_, C_, d)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("mode", [0, 1])
def test_spmm_bf16_two_row_user_csr_bitwise_fp32_kernel(d, mode, monkeypatch):
    monkeypatch.delenv("BBGR_SPMM_PAIR", raising=False)
    R_, C_ = 900, 400
    e = synthetic_edges(R_ - 3, C_ - 3, 12000, 11, items="zipf", duplicates=20)
    rows, cols = e[0], e[1]                     # user rows, average degree ~13
    c, prod, x, w, ep = _product_case(rows, cols, R_, C_, d, mode, 3 * d + mode)
    assert c.nnz <= 24 * c.n_rows               # the two-row form
    _check_product(prod, rows, cols, w, x, ep, R_, C_, d)


# ---------------------------------------------------------------------------
# 3. masks and lists
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("side", ["item", "user"])
def test_spmm_bf16_masks_and_lists(d, side, monkeypatch):
    monkeypatch.delenv("BBGR_SPMM_PAIR", raising=False)
    if side == "item":   # chunked plan with split rows
        R_, C_ = 400, 350
        e = synthetic_edges(C_ - 3, R_ - 3, 9000, 7, items="zipf", duplicates=20)
        rows, cols, kw = e[1], e[0], dict(long_threshold=8, chunk_edges=32)
    else:                # two-row form
        R_, C_ = 900, 400
        e = synthetic_edges(R_ - 3, C_ - 3, 12000, 11, items="zipf", duplicates=20)
        rows, cols, kw = e[0], e[1], {}
    c, prod, x, w, ep = _product_case(rows, cols, R_, C_, d, 0, d + 1, **kw)
    if side == "item":
        assert c.n_split > 0
    rng = np.random.default_rng(d)
    flag = rng.random(R_) < 0.3
    mask = t(flag.astype(np.uint8), torch.uint8)
    lst = t(np.flatnonzero(flag), torch.int64)
    n = lst.numel()
    padded = torch.cat([lst, torch.zeros(50, dtype=torch.int64, device=DEV)])   # capacity > length
    count = torch.tensor([n], dtype=torch.int64, device=DEV)
    xb = t(x).to(BF)
    full_y, full_acc, _, _ = _both(prod, xb, ep, R_, d)
    sel = t(flag, torch.bool)
    for what, kw2 in (("row_mask", dict(row_mask=mask, acc_mask=mask)),
                      ("row_list by length", dict(row_mask=mask, acc_mask=mask, row_list=lst)),
                      ("row_list by device count", dict(row_mask=mask, acc_mask=mask,
                                                        row_list=padded, row_count=count))):
        yb, accb, y32, acc32 = _both(prod, xb, ep, R_, d, **kw2)
        assert torch.equal(bits(yb[sel]), bits(full_y[sel])), what
        assert torch.equal(accb[sel], full_acc[sel]), what
        assert (yb[~sel].float() == 3.0).all() and (accb[~sel] == -5.0).all(), what
        assert torch.equal(accb, acc32) and torch.equal(bits(yb), bits(y32.to(BF))), what


def test_spmm_python_refusals_raise_value_error():
    e = synthetic_edges(300, 200, 3000, 3, items="zipf")
    c = Csr(e[1], e[0], 200, 300, DEV)
    prod = P.Product(c, None, None, None, {})
    xb = torch.zeros(300, 64, dtype=BF, device=DEV)
    y32 = torch.empty(200, 64, device=DEV)
    m = torch.ones(300, dtype=torch.uint8, device=DEV)
    im = torch.arange(200, dtype=torch.int32, device=DEV)
    for kw in (dict(y=y32), dict(add=y32), dict(src_mask=m), dict(y_map=im), dict(acc_map=im),
               dict(rng=(0, 200, 0, 0, 0, 0)), dict(tag_out=im, tag_mask=m)):
        with pytest.raises(ValueError):
            P.spmm(prod, xb, False, **kw)
    with pytest.raises(ValueError):
        P.spmm(prod, torch.zeros(300, 32, dtype=BF, device=DEV), False)
    with pytest.raises(ValueError):      # a column slice: rows no longer 16-byte aligned
        P.spmm(prod, torch.zeros(300, 72, dtype=BF, device=DEV)[:, 4:68], False)
    with pytest.raises(ValueError):
        P.spmm(prod, torch.zeros(300, 64, device=DEV), False,
               y=torch.empty(200, 64, dtype=BF, device=DEV))


# ---------------------------------------------------------------------------
# 4. chain
# ---------------------------------------------------------------------------
U, I, E, B = 600, 350, 8000, 200     # the graph of tests/test_gpu_widths.py


def _graph():
    return synthetic_edges(U, I, E, 17, items="zipf", duplicates=20), synthetic_credibility(U, 5)


def _weights(d):
    rng = np.random.default_rng(d)
    return (rng.uniform(-0.3, 0.3, (U, d)).astype(np.float32),
            rng.uniform(-0.3, 0.3, (I, d)).astype(np.float32))


def _pair(kind):
    e, cred = _graph()
    g = BipartiteGraph(e, U, I, DEV)
    sc = g.scales(kind, t(cred))
    return e, g, sc, P.OperatorPair.factored(g, sc)


def _round(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF).float()


def _fp32_chain(pair, u0, i0, K, order):
    """forward_steps restated with the existing fp32 spmm: every gathered
    table and every fed-forward y rounded to bf16 and widened again."""
    FI, FU = pair.fwd_item, pair.fwd_user
    acc_u, acc_i = torch.empty_like(u0), torch.empty_like(i0)
    yU, yI = torch.empty_like(u0), torch.empty_like(i0)
    gl = 1.0 / (K + 1)
    xu, xi = _round(u0), _round(i0)
    for k in range(1, K + 1):
        g = gl if k == K else 1.0
        ai = dict(acc_in=i0 if k == 1 else acc_i, acc_out=acc_i, acc_scale=FI.out_scale, gamma=g)
        au = dict(acc_in=u0 if k == 1 else acc_u, acc_out=acc_u, acc_scale=FU.out_scale, gamma=g)
        if order == P.ORDER_GS:
            P.spmm(FI, xu, k == 1, y=yI, y_scale=pair.feed_fwd_iu, **ai)
            P.spmm(FU, _round(yI), False, y=yU, y_scale=pair.feed_fwd_ui, **au)
            xu = _round(yU)
        else:
            P.spmm(FI, xu, k == 1, y=yI, y_scale=pair.feed_fwd_iu, **ai)
            P.spmm(FU, xi, k == 1, y=yU, y_scale=pair.feed_fwd_ui, **au)
            xu, xi = _round(yU), _round(yI)
    return acc_u, acc_i


def _f64_chain(e, sc, u0, i0, K, order):
    """The factored chain in float64 (scipy), the bf16 roundings restated."""
    ones = np.ones(e.shape[1])
    Ai = R.csr64(e[1], e[0], ones, (I, U))
    Au = R.csr64(e[0], e[1], ones, (U, I))
    p, q, s, tt, pt, qs = (getattr(sc, n).double().cpu().numpy()[:, None]
                           for n in ("p", "q", "s", "t", "pt", "qs"))
    acc_u, acc_i = u0.astype(np.float64), i0.astype(np.float64)
    xu, xi = rb(u0), rb(i0)
    for k in range(1, K + 1):
        Ti = Ai @ (q * xu if k == 1 else xu)
        if order == P.ORDER_GS:
            zi = rb(pt * Ti)
            Tu = Au @ zi
        else:
            Tu = Au @ (tt * xi if k == 1 else xi)
            xi = rb(pt * Ti)
        acc_i = acc_i + p * Ti
        acc_u = acc_u + s * Tu
        xu = rb(qs * Tu)
    return acc_u / (K + 1), acc_i / (K + 1)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("kind,order", [(OP_GS, P.ORDER_GS), (OP_J, P.ORDER_J)])
def test_bf16_chain_is_bitwise_the_rounded_fp32_chain(kind, order, K):
    d = 64
    e, g, sc, pair = _pair(kind)
    u0n, i0n = _weights(d)
    u0, i0 = t(u0n), t(i0n)
    ws = {}
    uf, itf = P.forward(pair, u0, i0, K, order, ws=ws, table_dtype=BF)
    want_u, want_i = _fp32_chain(pair, u0, i0, K, order)
    assert torch.equal(uf, want_u) and torch.equal(itf, want_i)
    assert uf.dtype == torch.float32 and itf.dtype == torch.float32
    # the tables the products gathered are bf16; the shadow is the rounded master
    assert all(v.dtype == BF for k, v in ws.items() if len(k) == 4)
    assert torch.equal(bits(ws[("u0h", U, d, BF)]), bits(u0.to(BF)))
    assert (("i0h", I, d, BF) in ws) == (order == P.ORDER_J)
    # without a workspace, and the default dtype, which is the fp32 chain
    uf2, itf2 = P.forward(pair, u0, i0, K, order, table_dtype=BF)
    assert torch.equal(uf2, uf) and torch.equal(itf2, itf)
    f32 = P.forward(pair, u0, i0, K, order)
    f32kw = P.forward(pair, u0, i0, K, order, table_dtype=torch.float32)
    assert torch.equal(f32[0], f32kw[0]) and torch.equal(f32[1], f32kw[1])
    assert not torch.equal(f32[0], uf)
    # sanity against float64 with the same roundings: one bf16 ulp, normwise
    ru, ri = _f64_chain(e, sc, u0n, i0n, K, order)
    for got, ref, name in ((uf, ru, "u_final"), (itf, ri, "i_final")):
        err = np.linalg.norm(got.double().cpu().numpy() - ref) / np.linalg.norm(ref)
        print(f"{name} K={K} {order}: normwise error vs float64 {err:.3e}")
        assert err <= 2.0 ** -8, (name, err)


def test_forward_bf16_refusals():
    e, g, sc, pair = _pair(OP_GS)
    u0n, i0n = _weights(64)
    with pytest.raises(ValueError):
        P.forward(pair, t(u0n), t(i0n), 2, reduce=lambda x: x, table_dtype=BF)
    with pytest.raises(ValueError):
        P.forward(pair, t(u0n), t(i0n), 2, table_dtype=BF,
                  tag=(torch.empty(E + 20, dtype=torch.int32, device=DEV),
                       torch.ones(I, dtype=torch.uint8, device=DEV)))
    with pytest.raises(ValueError):
        P.forward(pair, t(u0n), t(i0n), 2, table_dtype=torch.float16)
    u32, i32 = _weights(32)
    with pytest.raises(ValueError):
        P.forward(pair, t(u32), t(i32), 2, table_dtype=BF)
    gd = BipartiteGraph(e, U, I, DEV, vertex_order="degree")
    pio = P.OperatorPair.factored(gd, gd.scales(OP_GS, None))
    pio.set_input_order(gd.user_order, gd.item_order)
    with pytest.raises(ValueError):
        P.forward(pio, t(u0n), t(i0n), 2, table_dtype=BF)


def test_propagate_bf16_forward_with_the_fp32_backward():
    e, g, sc, pair = _pair(OP_GS)
    u0n, i0n = _weights(64)
    u0, i0 = t(u0n).requires_grad_(), t(i0n).requires_grad_()
    uf, itf = P.propagate(pair, u0, i0, 2, P.ORDER_GS, table_dtype=BF)
    want = P.forward(pair, u0.detach(), i0.detach(), 2, P.ORDER_GS, table_dtype=BF)
    assert torch.equal(uf, want[0]) and torch.equal(itf, want[1])
    gU, gI = torch.randn_like(uf), torch.randn_like(itf)
    torch.autograd.backward([uf, itf], [gU, gI])
    gu, gi = P.backward(pair, gU, gI, 2, P.ORDER_GS)
    assert torch.equal(u0.grad, gu) and torch.equal(i0.grad, gi)


# ---------------------------------------------------------------------------
# 5. step
# ---------------------------------------------------------------------------
REG = 1e-4


def _trainer(variant="v2_pop", d=64, K=3, **kw):
    e, cred = _graph()
    u0, i0 = _weights(d)
    return FusedTrainer(BipartiteGraph(e.copy(), U, I, DEV), variant,
                        cred=None if variant == "plain" else cred.copy(), emb_dim=d,
                        num_layers=K, batch_size=B, u0=u0.copy(), i0=i0.copy(), seed=11, **kw)


@pytest.mark.parametrize("variant", ["v2_pop", "cu_fair"])
def test_bf16_step_gradients_are_the_float64_adjoint_at_its_own_tables(variant):
    """Modelled on test_gpu_parity.test_fused_trainer_step_vs_oracle. The bf16
    forward changes the final tables, not the map from them to the loss and
    the gradients: the oracle's BPR at the trainer's own uf / itf, pushed
    through the transposed float64 chain, is what the fp32 backward computes."""
    K, d = 3, 64
    e, cred = _graph()
    u0, i0 = _weights(d)
    lam = 0.05 if variant == "cu_fair" else 0.0
    tr = _trainer(variant, d, K, forward_dtype="bf16", fuse_adam=False, frontier=False,
                  lambda_fair=lam)
    users = tr.next_users()
    loss = tr.step(users)
    n = users.numel()
    uu, pos, neg = users.cpu().numpy(), tr.pos[:n].cpu().numpy(), tr.neg[:n].cpu().numpy()
    assert (neg >= 0).all()
    uf, itf = tr.uf.double().cpu().numpy(), tr.itf.double().cpu().numpy()
    if variant == "cu_fair":
        A, Bm, deg_i = R.j_mats(e, U, I, cred)
        pop = deg_i / max(deg_i.max(), 1.0)
        want, gr = R.bpr_loss(uf, itf, u0, i0, uu, pos, neg, REG, pop, lam)
        gu0, gi0 = R.backward_j(A, Bm, gr["g_uf"], gr["g_if"], K)
    else:
        A, Bm = R.gs_mats(e, U, I, cred)
        want, gr = R.bpr_loss(uf, itf, u0, i0, uu, pos, neg, REG)
        gu0, gi0 = R.backward_gs(A, Bm, gr["g_uf"], gr["g_if"], K)
    gu0, gi0 = gu0 + gr["g_ue"], gi0 + gr["g_ie"]
    print(f"{variant}: loss {float(loss):.8f} oracle {want:.8f}")
    assert abs(float(loss) - want) <= 1e-5 * want
    assert_parity(tr.g_u0, gu0, f"bf16 step {variant} grad u0")
    assert_parity(tr.g_i0, gi0, f"bf16 step {variant} grad i0")
    assert tr.g_uf.abs().sum().item() == 0 and tr.g_if.abs().sum().item() == 0


def _state(tr):
    return [tr.user_w, tr.item_w, tr.m_u, tr.v_u, tr.m_i, tr.v_i]


def _run(tr, steps=3, stepper=None):
    losses = [float((stepper or tr).step()) for _ in range(steps)]
    torch.cuda.synchronize()
    return losses


def _assert_same(a, b):
    for x, y in zip(_state(a), _state(b)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("variant", ["v2_pop", "cu_fair"])
def test_bf16_step_frontier_determinism_and_graph_replay(variant):
    kw = dict(forward_dtype="bf16")
    a = _trainer(variant, frontier=True, **kw)
    la = _run(a)
    b = _trainer(variant, frontier=False, **kw)
    assert _run(b) == la                      # frontier on / off: bitwise
    _assert_same(a, b)
    c = _trainer(variant, frontier=True, **kw)
    assert _run(c) == la                      # two identical trainers: bitwise
    _assert_same(a, c)
    g = _trainer(variant, frontier=True, **kw)
    gs = GraphedStep(g)                       # its first step runs eagerly
    lg = [float(gs.first_loss)] + _run(g, 2, gs)
    assert lg == la
    _assert_same(a, g)
    assert int(a.mask_u.sum()) == 0 and int(a.mask_i.sum()) == 0
    f32 = _trainer(variant, frontier=True)
    assert _run(f32) != la                    # and it is not the fp32 step


def test_bf16_shadow_is_refreshed_every_step():
    """Every step rounds the shadow from the masters it starts from: after
    step 2 it holds the weights step 1 left (the masters as step 2 began; its
    own Adam update comes after the forward), and a forward() afterwards holds
    the current weights."""
    tr = _trainer("cu_fair", forward_dtype="bf16")
    assert tr.forward_shadow() == (None, None)
    tr.step()
    w1u, w1i = tr.user_w.clone(), tr.item_w.clone()
    tr.step()
    su, si = tr.forward_shadow()
    assert torch.equal(bits(su), bits(w1u.to(BF))) and torch.equal(bits(si), bits(w1i.to(BF)))
    assert not torch.equal(bits(su), bits(tr.user_w.to(BF)))
    tr.forward()
    su, si = tr.forward_shadow()
    assert torch.equal(bits(su), bits(tr.user_w.to(BF)))
    assert torch.equal(bits(si), bits(tr.item_w.to(BF)))
    gs_tr = _trainer("v2_pop", forward_dtype="bf16")
    gs_tr.step()
    su, si = gs_tr.forward_shadow()
    assert su is not None and si is None      # GS gathers u0 only


@pytest.mark.parametrize("variant", ["v2_pop", "cu_message", "method_a", "cu_fair", "plain"])
def test_bf16_trainer_forward_and_recommend_use_its_mode(variant):
    tr = _trainer(variant, K=2, forward_dtype="bf16")
    uf, itf = tr.forward()
    want = P.forward(tr.pair, tr.user_w, tr.item_w, 2, tr.order, table_dtype=BF)
    assert torch.equal(uf, want[0]) and torch.equal(itf, want[1])
    users = torch.arange(0, 40, device=DEV)
    from bbgr.recommend import recommend
    got = tr.recommend(users, 10)
    assert torch.equal(got, recommend(uf, itf, users, 10, exclude=tr._train_rows()))
    assert np.isfinite(float(tr.step()))


# ---------------------------------------------------------------------------
# 6. the default is unchanged
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["v2_pop", "cu_fair"])
def test_default_trainer_is_the_fp32_trainer(variant):
    a, b = _trainer(variant), _trainer(variant, forward_dtype="fp32")
    assert a.forward_dtype == "fp32" and a.table_dtype == torch.float32
    assert _run(a) == _run(b)
    _assert_same(a, b)
    assert not any(len(k) == 4 for k in a.ws)     # no bf16 table was ever allocated


def test_forward_dtype_refusals():
    e, cred = _graph()
    g = BipartiteGraph(e, U, I, DEV)
    with pytest.raises(ValueError, match="emb_dim >= 64"):
        FusedTrainer(g, "v2_pop", emb_dim=32, forward_dtype="bf16")
    with pytest.raises(ValueError, match="forward_dtype"):
        FusedTrainer(g, "v2_pop", emb_dim=64, forward_dtype="fp16")
    from bbgr.columns import ColumnShardedTrainer
    from bbgr.distributed import ShardedTrainer
    with pytest.raises(ValueError, match="forward_dtype"):
        ColumnShardedTrainer(g, U, I, "v2_pop", emb_dim=64, column_parts=1, column_index=0,
                             forward_dtype="bf16")
    with pytest.raises(ValueError, match="forward_dtype"):
        ShardedTrainer(e, U, I, "v2_pop", emb_dim=64, forward_dtype="bf16")
