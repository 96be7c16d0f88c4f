"""CPU: bbgr_ewa_normalize through ctypes: the workspace query and its documented
sum, BBGR_ERR_WORKSPACE, every argument check with its message, and the order
they run in (the query before any validation of the arrays, the nothing-to-do
return before the null checks). Every call here returns before a launch."""
import ctypes

import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
NAME = "bbgr_ewa_normalize"


def _err():
    return _lib.lib().bbgr_last_error().decode()


def _align(x, a=256):
    return (x + a - 1) // a * a


def _csr(**kw):
    """A planned CSR of 1000 edges over 40 rows: 3 chunks, one split row."""
    c = _lib.CsrStruct()
    c.n_rows, c.n_cols, c.nnz = 40, 50, 1000
    c.indptr = c.indices = c.chunks = c.split = FAKE
    c.long_threshold, c.chunk_edges, c.n_chunks, c.n_split = 64, 2048, 3, 1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _call(csr=None, *, null_csr=False, perm=FAKE, dst=FAKE, w_in=None, attr=FAKE, lda=5, cv=0,
          ca=1, w_raw=FAKE, ws=FAKE, nbytes=1 << 30, null_nbytes=False):
    """(status, workspace_bytes afterwards)."""
    n = ctypes.c_size_t(nbytes)
    c = None if null_csr else ctypes.byref(csr if csr is not None else _csr())
    rc = _lib.lib().bbgr_ewa_normalize(c, perm, dst, w_in, attr, lda, cv, ca, 1.0, 1.0, 1e-12,
                                       w_raw, FAKE, FAKE, ws,
                                       None if null_nbytes else ctypes.byref(n), None)
    return rc, n.value


def test_symbol_resolves_and_abi_is_still_12():
    L = _lib.lib()
    assert hasattr(L, NAME) and NAME in _lib._SIGNATURES and NAME in _lib.header_symbols()
    assert L.bbgr_abi_version() == 12


@pytest.mark.parametrize("nnz,n_rows,n_chunks", [
    (1000, 40, 3), (1000, 40, 0), (0, 40, 0), (1000, 0, 0), (0, 0, 0), (1, 1, 0), (64, 1, 1),
    (65, 1, 1), (32771, 77, 13), (1 << 20, 12345, 600),
])
def test_workspace_query_is_the_documented_sum(nnz, n_rows, n_chunks):
    """Raw weights in CSR order, per-row sums and chunk partials, each rounded up
    to 256 bytes and never empty; the input-order raw weights come on top only
    when neither w_in nor w_raw is given (own_raw)."""
    c = _csr(nnz=nnz, n_rows=n_rows, n_chunks=n_chunks, n_split=0)
    a_e = _align(4 * max(nnz, 1))
    base = a_e + _align(4 * max(n_rows, 1)) + _align(4 * max(n_chunks, 1))
    for kw, want in [(dict(), base),                                   # edge_attr, w_raw given
                     (dict(w_in=FAKE, attr=None, lda=0), base),        # w_in, w_raw given
                     (dict(w_in=FAKE, attr=None, lda=0, w_raw=None), base),
                     (dict(w_raw=None), base + a_e)]:                  # own_raw
        rc, n = _call(c, ws=None, nbytes=7, **kw)
        assert rc == 0 and n == want, (kw, n, want, _err())


def test_query_comes_before_validation_of_the_arrays():
    """A size query needs the CSR's sizes only: no array, no columns."""
    c = _csr(indptr=None, indices=None, chunks=None, split=None)
    rc, n = _call(c, perm=None, dst=None, attr=None, lda=0, cv=-1, ca=9, w_raw=None, ws=None,
                  nbytes=0)
    assert rc == 0, _err()
    assert n == 2 * _align(4000) + _align(160) + _align(12)


def test_small_workspace_names_both_sizes():
    _, need = _call(ws=None)
    rc, _ = _call(nbytes=need - 1)
    assert rc == -4 and _lib.STATUS[rc] == "BBGR_ERR_WORKSPACE", _err()
    assert _err().startswith(NAME + ":") and "workspace" in _err(), _err()
    assert str(need - 1) in _err() and str(need) in _err(), _err()
    rc, _ = _call(nbytes=0)
    assert rc == -4 and " 0 " in _err() and str(need) in _err(), _err()
    # own_raw needs more than the other modes: their size is too small for it
    rc, _ = _call(w_raw=None, nbytes=need)
    assert rc == -4 and str(need + _align(4000)) in _err(), _err()
    # the size comes before the argument checks below it
    rc, _ = _call(_csr(indptr=None), perm=None, nbytes=need - 1)
    assert rc == -4, _err()


@pytest.mark.parametrize("kw,text", [
    (dict(null_csr=True), "bad csr / workspace_bytes"),
    (dict(null_nbytes=True), "bad csr / workspace_bytes"),
    (dict(null_nbytes=True, ws=None), "bad csr / workspace_bytes"),
    (dict(csr=dict(n_rows=-1)), "bad csr / workspace_bytes"),
    (dict(csr=dict(nnz=-1)), "bad csr / workspace_bytes"),
    (dict(csr=dict(indptr=None)), "null indptr / perm"),
    (dict(perm=None), "null indptr / perm"),
    (dict(csr=dict(chunks=None)), "csr needs its load-balance plan"),
    (dict(csr=dict(long_threshold=0)), "csr needs its load-balance plan"),
    (dict(csr=dict(split=None)), "plan split rows missing"),
    (dict(attr=None), "need w_in or edge_attr with valid columns"),
    (dict(cv=-1), "need w_in or edge_attr with valid columns"),
    (dict(ca=-1), "need w_in or edge_attr with valid columns"),
    (dict(cv=5), "need w_in or edge_attr with valid columns"),
    (dict(ca=5), "need w_in or edge_attr with valid columns"),
    (dict(cv=1, ca=2, lda=2), "need w_in or edge_attr with valid columns"),
    (dict(lda=0), "need w_in or edge_attr with valid columns"),
])
def test_refusals_and_their_messages(kw, text):
    kw = dict(kw)
    if isinstance(kw.get("csr"), dict):
        kw["csr"] = _csr(**kw["csr"])
    rc, _ = _call(**kw)
    assert rc == -1, (rc, _err())
    assert _err() == NAME + ": " + text, _err()


def test_plan_arrays_are_needed_only_where_the_plan_has_entries():
    """n_chunks == 0 / n_split == 0 need no chunks / split array: with both NULL
    the call gets as far as the next check (the columns)."""
    c = _csr(n_chunks=0, n_split=0, chunks=None, split=None, long_threshold=0)
    rc, _ = _call(c, cv=7)
    assert rc == -1 and "valid columns" in _err(), _err()
    c = _csr(n_split=0, split=None)
    rc, _ = _call(c, cv=7)
    assert rc == -1 and "valid columns" in _err(), _err()


@pytest.mark.parametrize("sizes", [dict(nnz=0), dict(n_rows=0), dict(nnz=0, n_rows=0)])
def test_nothing_to_do_is_ok_without_touching_a_pointer(sizes):
    """E == 0 or n_rows == 0 returns before the null checks and before any launch
    (no GPU here): every array may be NULL, the columns need not be valid."""
    c = _csr(indptr=None, indices=None, chunks=None, split=None, **sizes)
    n = ctypes.c_size_t(1 << 20)
    rc = _lib.lib().bbgr_ewa_normalize(ctypes.byref(c), None, None, None, None, 0, -1, -1, 1.0,
                                       1.0, 1e-12, None, None, None, FAKE, ctypes.byref(n), None)
    assert rc == 0, _err()
    assert n.value == 1 << 20                      # a given size is left as it is
    # ... but after the workspace check
    rc, _ = _call(c, nbytes=1)
    assert rc == -4, _err()
