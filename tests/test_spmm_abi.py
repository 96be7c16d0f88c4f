"""CPU: every refusal of the SpMM-side C ABI, by return code and exact message.

bbgr_spmm, bbgr_epilogue, bbgr_scatter_apply, bbgr_bpr, bbgr_ego_rows and the
four bbgr_rows_* entries validate on the host before any launch, so the tables
below run through ctypes with fake aligned addresses (tests/test_bf16_abi.py's
style). Each row mutates one valid call; the rows that break two rules at once
pin which check speaks first. The strings are the library's own: a change of
wording, of return code or of check order fails here."""
import ctypes

import pytest

from bbgr import _lib

FAKE = 4096   # a non-null, 16-byte aligned address that is never dereferenced
OK, INVALID, UNSUPPORTED = 0, -1, -2
WIDTHS = "(8, 16, 32, 64, 128, 256)"


def _call(name, *args):
    L = _lib.lib()
    rc = getattr(L, name)(*args)
    return rc, L.bbgr_last_error().decode() if rc else ""


# --------------------------------------------------------------------------
# bbgr_spmm
# --------------------------------------------------------------------------
PLAN = dict(long_threshold=8, chunk_edges=32, n_chunks=4, n_split=1, chunks=FAKE, split=FAKE)
ADAM = dict(adam_param=FAKE, adam_exp_avg=FAKE, adam_exp_avg_sq=FAKE, adam_ld=64,
            adam_bias_correction1=1.0, adam_bias_correction2_sqrt=1.0)


def _csr(**kw):
    c = _lib.CsrStruct()
    c.n_rows, c.n_cols, c.nnz = 100, 80, 1000   # average degree 10: two rows per group
    c.indptr = c.indices = FAKE
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _args(**kw):
    a = _lib.SpmmArgs()
    a.d = 64
    a.x, a.ldx, a.y, a.ldy = FAKE, 64, FAKE, 64
    a.col_scale_s = a.y_scale_s = a.add_scale_s = a.acc_scale_s = a.gamma = 1.0
    for k, v in kw.items():
        if k == "range":
            a.use_range = 1
            a.range[:] = v
        else:
            setattr(a, k, v)
    return a


def _spmm(csr_kw, args_kw):
    c, a = _csr(**csr_kw), _args(**args_kw)
    return _call("bbgr_spmm", ctypes.byref(c), ctypes.byref(a), None)


S = "bbgr_spmm: "
TABLES = S + "tables must be 16-byte aligned with ld >= d, ld % 4 == 0"
ADAM_NEEDS = (S + "fused Adam needs param/exp_avg/exp_avg_sq (16-byte aligned, adam_ld >= d) "
              "and bias corrections > 0")
ADAM_ROWS = S + "fused Adam needs every row (no masks, row list or range)"
RANGE = S + "range out of bounds"
TAG_OUT = (S + "tag_out needs tag_mask and a full launch (no masks, list, range or fused Adam)")
SRC_TAGGED = S + "src_tagged replaces src_mask (no src_mask / src_bits / fused Adam)"
TAG_PAIR = S + "tagged indices need a two-row CSR (average degree <= 24) and d >= 64"
LIST_MASK = S + "row_list needs row_mask when the plan has long-row chunks"
W32 = dict(d=32, ldx=32, ldy=32)

SPMM_ROWS = [
    # the CSR
    (dict(n_rows=-1), {}, INVALID, S + "negative csr size"),
    (dict(n_cols=-1), {}, INVALID, S + "negative csr size"),
    (dict(nnz=-1), {}, INVALID, S + "negative csr size"),
    (dict(indptr=None), {}, INVALID, S + "null csr arrays"),
    (dict(indices=None), {}, INVALID, S + "null csr arrays"),
    # width, x and the tables
    ({}, dict(d=48), UNSUPPORTED, S + "embedding dim 48 unsupported " + WIDTHS),
    ({}, dict(d=0), UNSUPPORTED, S + "embedding dim 0 unsupported " + WIDTHS),
    ({}, dict(x=None), INVALID, S + "null x"),
    ({}, dict(x=FAKE + 4), INVALID, TABLES),
    ({}, dict(ldx=60), INVALID, TABLES),
    ({}, dict(ldx=66), INVALID, TABLES),
    ({}, dict(y=FAKE + 8), INVALID, TABLES),
    ({}, dict(ldy=32), INVALID, TABLES),
    ({}, dict(add=FAKE, ldadd=0), INVALID, TABLES),
    ({}, dict(acc_in=FAKE + 2, ldacc_in=64), INVALID, TABLES),
    ({}, dict(acc_out=FAKE, ldacc_out=65), INVALID, TABLES),
    # fused Adam
    ({}, dict(ADAM, adam_exp_avg=None), INVALID, ADAM_NEEDS),
    ({}, dict(ADAM, adam_exp_avg_sq=None), INVALID, ADAM_NEEDS),
    ({}, dict(ADAM, adam_ld=32), INVALID, ADAM_NEEDS),
    ({}, dict(ADAM, adam_param=FAKE + 4), INVALID, ADAM_NEEDS),
    ({}, dict(ADAM, adam_bias_correction1=0.0), INVALID, ADAM_NEEDS),
    ({}, dict(ADAM, adam_bias_correction2_sqrt=0.0), INVALID, ADAM_NEEDS),
    ({}, dict(ADAM, adam_state=FAKE), INVALID, ADAM_NEEDS),            # no bias-correction table
    ({}, dict(ADAM, adam_grad=FAKE, adam_grad_ld=60), INVALID, ADAM_NEEDS),
    ({}, dict(adam_mirror=FAKE), INVALID, ADAM_NEEDS),                 # mirror without a step
    ({}, dict(ADAM, adam_mirror=FAKE), INVALID, ADAM_NEEDS),           # mirror needs unmapped moments
    ({}, dict(ADAM, src_mask=FAKE), INVALID, ADAM_ROWS),
    ({}, dict(ADAM, row_mask=FAKE), INVALID, ADAM_ROWS),
    ({}, dict(ADAM, row_list=FAKE, n_row_list=4), INVALID, ADAM_ROWS),
    ({}, dict(ADAM, range=[0, 100, 0, 0, 0, 0]), INVALID, ADAM_ROWS),
    # source masks and weights
    ({}, dict(src_mask_bits=FAKE), INVALID, S + "src_mask_bits packs src_mask (pass both)"),
    ({}, dict(src_bits=FAKE), INVALID,
     S + "src_bits needs src_mask (narrow and two-row kernels read the mask)"),
    ({}, dict(weight_mode=1), INVALID, S + "weight_mode 1 needs edge_val"),
    ({}, dict(weight_mode=2), INVALID, S + "weight_mode 2 needs col_scale"),
    ({}, dict(weight_mode=3), INVALID, S + "weight_mode 3 not in {0,1,2}"),
    ({}, dict(weight_mode=-1), INVALID, S + "weight_mode -1 not in {0,1,2}"),
    # the load-balance plan
    (dict(PLAN, chunks=None), dict(partial=FAKE), INVALID, S + "plan chunks missing"),
    (dict(PLAN, split=None), dict(partial=FAKE), INVALID,
     S + "split rows need plan + partial workspace"),
    (PLAN, {}, INVALID, S + "split rows need plan + partial workspace"),
    (dict(PLAN, long_threshold=0), dict(partial=FAKE), INVALID,
     S + "plan without long_threshold"),
    # the row list and the range
    ({}, dict(row_count=FAKE), INVALID, S + "row_count needs row_list"),
    ({}, dict(row_list=FAKE, n_row_list=-1), INVALID, S + "negative n_row_list"),
    (PLAN, dict(partial=FAKE, row_list=FAKE, n_row_list=4), INVALID, LIST_MASK),
    (PLAN, dict(partial=FAKE, range=[-1, 100, 0, 4, 0, 1]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[60, 50, 0, 4, 0, 1]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 101, 0, 4, 0, 1]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 100, -1, 4, 0, 1]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 100, 3, 2, 0, 1]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 100, 0, 5, 0, 1]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 100, 0, 4, -1, 1]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 100, 0, 4, 1, 0]), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 100, 0, 4, 0, 2]), INVALID, RANGE),
    ({}, dict(range=[0, 100, 0, 0, 0, 1]), INVALID, RANGE),             # a CSR without a plan
    ({}, dict(range=[0, 100, 0, 0, 0, 0], row_list=FAKE, n_row_list=4), INVALID,
     S + "range with row_list needs row_mask (chunk rows)"),
    # tagged indices
    ({}, dict(tag_out=FAKE), INVALID, TAG_OUT),
    ({}, dict(tag_out=FAKE, tag_mask=FAKE, src_tagged=FAKE), INVALID, TAG_OUT),
    ({}, dict(tag_out=FAKE, tag_mask=FAKE, src_mask=FAKE), INVALID, TAG_OUT),
    ({}, dict(tag_out=FAKE, tag_mask=FAKE, row_mask=FAKE), INVALID, TAG_OUT),
    ({}, dict(tag_out=FAKE, tag_mask=FAKE, row_list=FAKE, n_row_list=4), INVALID, TAG_OUT),
    ({}, dict(tag_out=FAKE, tag_mask=FAKE, range=[0, 100, 0, 0, 0, 0]), INVALID, TAG_OUT),
    ({}, dict(ADAM, tag_out=FAKE, tag_mask=FAKE), INVALID, TAG_OUT),
    ({}, dict(src_tagged=FAKE, src_mask=FAKE), INVALID, SRC_TAGGED),
    ({}, dict(src_tagged=FAKE, src_mask=FAKE, src_bits=FAKE), INVALID, SRC_TAGGED),
    ({}, dict(ADAM, src_tagged=FAKE), INVALID, SRC_TAGGED),
    ({}, dict(W32, tag_out=FAKE, tag_mask=FAKE), UNSUPPORTED, TAG_PAIR),
    ({}, dict(W32, src_tagged=FAKE), UNSUPPORTED, TAG_PAIR),
    (dict(nnz=2401), dict(tag_out=FAKE, tag_mask=FAKE), UNSUPPORTED, TAG_PAIR),
    (dict(nnz=2401), dict(src_tagged=FAKE), UNSUPPORTED, TAG_PAIR),
    (dict(nnz=2401), dict(src_tagged=FAKE, row_mask=FAKE), UNSUPPORTED, TAG_PAIR),
    # two rules broken at once: the earlier check speaks
    (dict(n_rows=-1, indptr=None), {}, INVALID, S + "negative csr size"),
    (dict(indptr=None), dict(d=48), INVALID, S + "null csr arrays"),
    ({}, dict(d=48, x=None), UNSUPPORTED, S + "embedding dim 48 unsupported " + WIDTHS),
    ({}, dict(x=None, ldy=32), INVALID, S + "null x"),
    ({}, dict(ADAM, ldx=60, adam_ld=32), INVALID, TABLES),
    ({}, dict(ADAM, adam_ld=32, src_mask=FAKE), INVALID, ADAM_NEEDS),
    ({}, dict(ADAM, row_mask=FAKE, src_mask_bits=FAKE), INVALID, ADAM_ROWS),
    ({}, dict(src_mask_bits=FAKE, src_bits=FAKE), INVALID,
     S + "src_mask_bits packs src_mask (pass both)"),
    ({}, dict(src_bits=FAKE, weight_mode=1), INVALID,
     S + "src_bits needs src_mask (narrow and two-row kernels read the mask)"),
    (dict(PLAN, chunks=None), dict(weight_mode=2), INVALID, S + "weight_mode 2 needs col_scale"),
    (dict(PLAN, chunks=None, long_threshold=0), {}, INVALID, S + "plan chunks missing"),
    (dict(PLAN, long_threshold=0), {}, INVALID, S + "split rows need plan + partial workspace"),
    (dict(PLAN, long_threshold=0), dict(partial=FAKE, row_count=FAKE), INVALID,
     S + "plan without long_threshold"),
    ({}, dict(row_count=FAKE, range=[0, 101, 0, 0, 0, 0]), INVALID, S + "row_count needs row_list"),
    ({}, dict(range=[0, 101, 0, 0, 0, 0], row_list=FAKE, n_row_list=-1), INVALID, RANGE),
    (PLAN, dict(partial=FAKE, range=[0, 100, 0, 4, 0, 1], row_list=FAKE, n_row_list=-1), INVALID,
     S + "range with row_list needs row_mask (chunk rows)"),
    (PLAN, dict(partial=FAKE, row_list=FAKE, n_row_list=-1), INVALID, S + "negative n_row_list"),
    (PLAN, dict(partial=FAKE, row_list=FAKE, n_row_list=4, tag_out=FAKE), INVALID, LIST_MASK),
    ({}, dict(tag_out=FAKE, src_tagged=FAKE, src_mask=FAKE), INVALID, TAG_OUT),
    ({}, dict(src_tagged=FAKE, src_mask=FAKE, weight_mode=3), INVALID, SRC_TAGGED),
    ({}, dict(W32, src_tagged=FAKE, weight_mode=3), INVALID, S + "weight_mode 3 not in {0,1,2}"),
    # nothing to compute: accepted without a launch
    (dict(n_rows=0, nnz=0), dict(x=None), OK, ""),
    (dict(n_rows=0, nnz=0), dict(W32, x=None, weight_mode=2, col_scale=FAKE), OK, ""),
    ({}, dict(row_list=FAKE, n_row_list=0), OK, ""),
    ({}, dict(row_list=FAKE, n_row_list=0, row_count=FAKE, src_mask=FAKE, src_bits=FAKE), OK, ""),
    ({}, dict(range=[7, 7, 0, 0, 0, 0]), OK, ""),
    (PLAN, dict(partial=FAKE, range=[100, 100, 4, 4, 1, 1]), OK, ""),
    (PLAN, dict(partial=FAKE, range=[0, 100, 2, 2, 0, 1], row_list=FAKE, n_row_list=0,
                row_mask=FAKE), OK, ""),
]


@pytest.fixture(autouse=True)
def _default_pairing(monkeypatch):
    monkeypatch.delenv("BBGR_SPMM_PAIR", raising=False)   # the A/B override of the two-row rule


def test_spmm_null_structs():
    c, a = _csr(), _args()
    want = (INVALID, S + "null csr/args")
    assert _call("bbgr_spmm", None, None, None) == want
    assert _call("bbgr_spmm", ctypes.byref(c), None, None) == want
    assert _call("bbgr_spmm", None, ctypes.byref(a), None) == want


@pytest.mark.parametrize("csr_kw,args_kw,rc,msg", SPMM_ROWS)
def test_spmm_refusals(csr_kw, args_kw, rc, msg):
    assert _spmm(csr_kw, args_kw) == (rc, msg)


def test_spmm_f32_form_refuses_split_plans():
    want = (INVALID, "bbgr_spmm_f32: the plan has split rows; use bbgr_spmm with a partial workspace")
    c = _csr(**PLAN)
    assert _call("bbgr_spmm_f32", ctypes.byref(c), FAKE, 64, FAKE, 64, 64, None, None, None, 1.0,
                 None) == want
    assert _call("bbgr_spmm_f32", None, FAKE, 64, FAKE, 64, 64, None, None, None, 1.0,
                 None) == (INVALID, "bbgr_spmm_f32: null csr")
    # the thin form reaches bbgr_spmm's own checks
    c = _csr()
    assert _call("bbgr_spmm_f32", ctypes.byref(c), FAKE, 60, FAKE, 64, 64, None, None, None, 1.0,
                 None) == (INVALID, TABLES)


# --------------------------------------------------------------------------
# bbgr_epilogue(n_rows, t, ldt, args, stream)
# --------------------------------------------------------------------------
E = "bbgr_epilogue: "
E_TABLES = E + "tables must be 16-byte aligned with ld >= d, ld % 4 == 0"

EPILOGUE_ROWS = [
    ((-1, FAKE, 64), {}, INVALID, E + "bad args"),
    ((100, FAKE, 64), dict(d=48), UNSUPPORTED, E + "embedding dim 48 unsupported " + WIDTHS),
    ((100, None, 64), {}, INVALID, E_TABLES),
    ((100, FAKE + 4, 64), {}, INVALID, E_TABLES),
    ((100, FAKE, 60), {}, INVALID, E_TABLES),
    ((100, FAKE, 66), {}, INVALID, E_TABLES),
    ((100, FAKE, 64), dict(y=FAKE + 8), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(ldy=32), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(add=FAKE, ldadd=62), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(acc_in=FAKE, ldacc_in=0), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(acc_out=FAKE + 1, ldacc_out=64), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(ADAM, adam_exp_avg=None), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(ADAM, adam_bias_correction1=0.0), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(adam_mirror=FAKE), INVALID, E_TABLES),
    ((100, FAKE, 64), dict(row_list=FAKE, n_row_list=-1), INVALID, E + "negative n_row_list"),
    # two at once
    ((-1, FAKE, 64), dict(d=48), INVALID, E + "bad args"),
    ((100, None, 64), dict(d=48), UNSUPPORTED, E + "embedding dim 48 unsupported " + WIDTHS),
    ((100, FAKE, 60), dict(row_list=FAKE, n_row_list=-1), INVALID, E_TABLES),
    # nothing to do: accepted without a launch (the width is still checked first)
    ((0, None, 0), {}, OK, ""),
    ((0, None, 0), dict(d=48), UNSUPPORTED, E + "embedding dim 48 unsupported " + WIDTHS),
    ((100, FAKE, 64), dict(row_list=FAKE, n_row_list=0), OK, ""),
]


@pytest.mark.parametrize("call,args_kw,rc,msg", EPILOGUE_ROWS)
def test_epilogue_refusals(call, args_kw, rc, msg):
    a = _args(**args_kw)
    assert _call("bbgr_epilogue", *call, ctypes.byref(a), None) == (rc, msg)
    assert _call("bbgr_epilogue", 100, FAKE, 64, None, None) == (INVALID, E + "bad args")


# --------------------------------------------------------------------------
# bbgr_scatter_apply(n, n_dst, plan, src, ldsrc, src2, ldsrc2, dst, lddst, d, stream)
# --------------------------------------------------------------------------
A = "bbgr_scatter_apply: "
A_TABLES = A + "tables must be 16-byte aligned, ld >= d, ld % 4 == 0"
A_OK = dict(n=10, n_dst=50, plan=FAKE, src=FAKE, ldsrc=64, src2=None, ldsrc2=0, dst=FAKE,
            lddst=64, d=64)

SCATTER_ROWS = [
    (dict(n=-1), INVALID, A + "bad sizes"),
    (dict(n=1 << 31), INVALID, A + "bad sizes"),
    (dict(n_dst=-1), INVALID, A + "bad sizes"),
    (dict(n_dst=0xFFFFFFFF), INVALID, A + "bad sizes"),
    (dict(d=48), UNSUPPORTED, A + "d = 48 unsupported " + WIDTHS),
    (dict(plan=None), INVALID, A + "null arrays"),
    (dict(src=None), INVALID, A + "null arrays"),
    (dict(dst=None), INVALID, A + "null arrays"),
    (dict(src=FAKE + 4), INVALID, A_TABLES),
    (dict(dst=FAKE + 8), INVALID, A_TABLES),
    (dict(ldsrc=60), INVALID, A_TABLES),
    (dict(ldsrc=66), INVALID, A_TABLES),
    (dict(lddst=32), INVALID, A_TABLES),
    (dict(lddst=65), INVALID, A_TABLES),
    (dict(src2=FAKE + 4, ldsrc2=64), INVALID, A_TABLES),
    (dict(src2=FAKE, ldsrc2=0), INVALID, A_TABLES),
    (dict(src2=FAKE, ldsrc2=70), INVALID, A_TABLES),
    (dict(n=-1, d=48), INVALID, A + "bad sizes"),
    (dict(d=48, plan=None), UNSUPPORTED, A + "d = 48 unsupported " + WIDTHS),
    (dict(src=None, lddst=32), INVALID, A + "null arrays"),
    (dict(n=0, plan=None, src=None, dst=None), OK, ""),
    (dict(n=0, d=48), UNSUPPORTED, A + "d = 48 unsupported " + WIDTHS),
]


@pytest.mark.parametrize("kw,rc,msg", SCATTER_ROWS)
def test_scatter_apply_refusals(kw, rc, msg):
    v = dict(A_OK, **kw)
    assert _call("bbgr_scatter_apply", *v.values(), None) == (rc, msg)


# --------------------------------------------------------------------------
# bbgr_bpr
# --------------------------------------------------------------------------
B = "bbgr_bpr: "
B_TABLES = B + "tables must be 16-byte aligned with ld >= d, ld % 4 == 0"
B_OK = dict(batch=32, d=64, n_users=100, n_items=80, users=FAKE, pos=FAKE, neg=FAKE,
            uf=FAKE, lduf=64, itf=FAKE, ldif=64)
B_EGO = dict(ue=FAKE, ldue=64, ie=FAKE, ldie=64)

BPR_ROWS = [
    (dict(batch=-1), INVALID, B + "negative batch"),
    (dict(d=48), UNSUPPORTED, B + "embedding dim 48 unsupported " + WIDTHS),
    (dict(users=None), INVALID, B + "null index/table"),
    (dict(pos=None), INVALID, B + "null index/table"),
    (dict(neg=None), INVALID, B + "null index/table"),
    (dict(uf=None), INVALID, B + "null index/table"),
    (dict(itf=None), INVALID, B + "null index/table"),
    (dict(n_users=0), INVALID, B + "n_users/n_items must be set"),
    (dict(n_items=0), INVALID, B + "n_users/n_items must be set"),
    (dict(parts=FAKE), INVALID, B + "ego tables required"),
    (dict(g_ue=FAKE, ldgue=64), INVALID, B + "ego tables required"),
    (dict(g_ie=FAKE, ldgie=64, ue=FAKE, ldue=64), INVALID, B + "ego tables required"),
    (dict(scores_out=FAKE), INVALID, B + "ego tables required"),
    (dict(B_EGO, scores_out=FAKE, scores=FAKE), INVALID,
     B + "scores_out and scores exclude each other"),
    (dict(uf=FAKE + 4), INVALID, B_TABLES),
    (dict(lduf=60), INVALID, B_TABLES),
    (dict(ldif=66), INVALID, B_TABLES),
    (dict(ue=FAKE, ldue=0), INVALID, B_TABLES),
    (dict(ie=FAKE + 8, ldie=64), INVALID, B_TABLES),
    (dict(g_uf=FAKE, ldguf=32), INVALID, B_TABLES),
    (dict(g_if=FAKE + 2, ldgif=64), INVALID, B_TABLES),
    (dict(B_EGO, g_ue=FAKE, ldgue=65), INVALID, B_TABLES),
    (dict(B_EGO, g_ie=FAKE, ldgie=63), INVALID, B_TABLES),
    (dict(contrib=FAKE, ldcontrib=48), INVALID, B_TABLES),
    (dict(batch=-1, d=48), INVALID, B + "negative batch"),
    (dict(d=48, users=None), UNSUPPORTED, B + "embedding dim 48 unsupported " + WIDTHS),
    (dict(users=None, n_users=0), INVALID, B + "null index/table"),
    (dict(parts=FAKE, lduf=60), INVALID, B + "ego tables required"),
    (dict(batch=0, d=48, users=None), OK, ""),   # an empty batch returns before the width check
]


@pytest.mark.parametrize("kw,rc,msg", BPR_ROWS)
def test_bpr_refusals(kw, rc, msg):
    a = _lib.BprArgs()
    for k, v in dict(B_OK, **kw).items():
        setattr(a, k, v)
    assert _call("bbgr_bpr", ctypes.byref(a), None) == (rc, msg)
    assert _call("bbgr_bpr", None, None) == (INVALID, B + "null args")
    assert _call("bbgr_bpr_fwd_bwd", ctypes.byref(a), None) == (rc, msg)   # the blueprint name


# --------------------------------------------------------------------------
# bbgr_ego_rows(B, d, cu, sp, sn, iu, ii, ue, ldue, ie, ldie, dloss, reg, counts,
#               g_u, ldgu, g_i, ldgi, scale, counts_u_out, stream)
# --------------------------------------------------------------------------
G = "bbgr_ego_rows: "
G_TABLES = G + "tables must be 16-byte aligned, ld % 4 == 0"
G_OK = dict(B=32, d=64, cu=FAKE, sp=FAKE, sn=FAKE, iu=FAKE, ii=FAKE, ue=FAKE, ldue=64, ie=FAKE,
            ldie=64, dloss=None, reg=1e-4, counts=FAKE, g_u=FAKE, ldgu=64, g_i=FAKE, ldgi=64,
            scale=1.0, counts_u_out=None)

EGO_ROWS = [
    (dict(B=-1), INVALID, G + "bad batch"),
    (dict(B=(1 << 31) // 3 + 1), INVALID, G + "bad batch"),
    (dict(d=48), UNSUPPORTED, G + "embedding dim 48 unsupported " + WIDTHS),
    *[(({k: None}), INVALID, G + "null arrays")
      for k in ("cu", "sp", "sn", "iu", "ii", "ue", "ie", "counts", "g_u", "g_i")],
    (dict(ue=FAKE + 4), INVALID, G_TABLES),
    (dict(ie=FAKE + 8), INVALID, G_TABLES),
    (dict(g_u=FAKE + 2), INVALID, G_TABLES),
    (dict(g_i=FAKE + 1), INVALID, G_TABLES),
    (dict(ldue=66), INVALID, G_TABLES),
    (dict(ldie=65), INVALID, G_TABLES),
    (dict(ldgu=67), INVALID, G_TABLES),
    (dict(ldgi=62), INVALID, G_TABLES),
    (dict(B=-1, d=48), INVALID, G + "bad batch"),
    (dict(d=48, cu=None), UNSUPPORTED, G + "embedding dim 48 unsupported " + WIDTHS),
    (dict(cu=None, ldue=66), INVALID, G + "null arrays"),
    (dict(B=0, cu=None, ue=None), OK, ""),
    (dict(B=0, d=48), UNSUPPORTED, G + "embedding dim 48 unsupported " + WIDTHS),
]


@pytest.mark.parametrize("kw,rc,msg", EGO_ROWS)
def test_ego_rows_refusals(kw, rc, msg):
    v = dict(G_OK, **kw)
    assert _call("bbgr_ego_rows", *v.values(), None) == (rc, msg)


# --------------------------------------------------------------------------
# bbgr_rows_copy / _gather (n, idx, src, ldsrc, dst, lddst, d, stream),
# bbgr_rows_add_unique (.., d, n_dst, stream),
# bbgr_rows_add_slots (n, slot, counts, rows, src, ldsrc, dst, lddst, d, n_dst, stream)
# --------------------------------------------------------------------------
R_OK = dict(n=10, slot=FAKE, counts=FAKE, rows=FAKE, src=FAKE, ldsrc=64, dst=FAKE, lddst=64,
            d=64, n_dst=50)
ROWS_ENTRIES = {   # entry -> its arguments, in order, by R_OK's names (slot doubles as idx)
    "bbgr_rows_copy": ("n", "slot", "src", "ldsrc", "dst", "lddst", "d"),
    "bbgr_rows_gather": ("n", "slot", "src", "ldsrc", "dst", "lddst", "d"),
    "bbgr_rows_add_unique": ("n", "slot", "src", "ldsrc", "dst", "lddst", "d", "n_dst"),
    "bbgr_rows_add_slots": ("n", "slot", "counts", "rows", "src", "ldsrc", "dst", "lddst", "d",
                            "n_dst"),
}
SIZES = "bad sizes (d, ld multiples of 4, ld >= d)"
ARRAYS = "null or unaligned arrays"

ROWS_ROWS = [
    (dict(n=-1), INVALID, SIZES),
    (dict(n_dst=-1), INVALID, SIZES),
    (dict(d=0), INVALID, SIZES),
    (dict(d=-4), INVALID, SIZES),
    (dict(d=6, ldsrc=8, lddst=8), INVALID, SIZES),
    (dict(ldsrc=60), INVALID, SIZES),
    (dict(lddst=32), INVALID, SIZES),
    (dict(ldsrc=66), INVALID, SIZES),
    (dict(lddst=65), INVALID, SIZES),
    (dict(slot=None), INVALID, ARRAYS),
    (dict(counts=None), INVALID, ARRAYS),
    (dict(rows=None), INVALID, ARRAYS),
    (dict(src=None), INVALID, ARRAYS),
    (dict(dst=None), INVALID, ARRAYS),
    (dict(src=FAKE + 4), INVALID, ARRAYS),
    (dict(dst=FAKE + 8), INVALID, ARRAYS),
    (dict(ldsrc=60, src=None), INVALID, SIZES),
    (dict(n=-1, slot=None), INVALID, SIZES),
    (dict(n=0, slot=None, src=None, dst=None), OK, ""),
    (dict(n=0, d=6), INVALID, SIZES),
]


# each mutation against every entry that takes the mutated arguments
ROWS_CASES = [(entry, kw, rc, msg) for entry, names in sorted(ROWS_ENTRIES.items())
              for kw, rc, msg in ROWS_ROWS if set(kw) <= set(names)]


@pytest.mark.parametrize("entry,kw,rc,msg", ROWS_CASES)
def test_rows_entries_refusals(entry, kw, rc, msg):
    v = dict(R_OK, **kw)
    want = (rc, f"{entry}: {msg}" if rc else "")
    assert _call(entry, *(v[k] for k in ROWS_ENTRIES[entry]), None) == want
