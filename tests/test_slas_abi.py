"""CPU: argument validation and workspace queries of the SLAS entry points
through ctypes (host code only: every check runs before any launch), the host
planner of train_and_export_credibility, and the CSV writer / reader."""
import ctypes
import subprocess

import numpy as np
import pytest

from bbgr import _lib

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced


def _err():
    return _lib.lib().bbgr_last_error().decode()


def test_abi_version_is_still_12():
    assert _lib.lib().bbgr_abi_version() == 12


@pytest.mark.parametrize("cname,pyty", [("bbgr_slas_sample_args", _lib.SlasSampleArgs),
                                        ("bbgr_slas_induce_args", _lib.SlasInduceArgs)])
def test_struct_layout_matches_header(cname, pyty, tmp_path):
    src = f'#include "bbgr.h"\n#include <stdio.h>\nint main(){{printf("%zu", sizeof({cname}));}}'
    exe = str(tmp_path / ("sizeof_" + cname))
    subprocess.run(["gcc", "-x", "c", "-", "-I", str(_lib.HEADER_PATH.parent), "-o", exe],
                   input=src, text=True, check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert int(out) == ctypes.sizeof(pyty)


# -- bbgr_slas_sample ------------------------------------------------------------
def _sample_args(**kw):
    a = _lib.SlasSampleArgs()
    a.n, a.n_rows, a.F, a.k, a.kappa = 100, 1000, 2, 15, 3.0
    a.rows = a.indptr = a.nbr = a.eid = a.row_profile = a.nbr_profile = FAKE
    a.out_nbr = a.out_eid = a.out_count = FAKE
    a.ts_stride = 5
    for key, v in kw.items():
        setattr(a, key, v)
    return a


@pytest.mark.parametrize("kw,field", [
    (dict(rows=None), "rows"), (dict(indptr=None), "indptr"), (dict(nbr=None), "nbr"),
    (dict(eid=None), "eid"), (dict(row_profile=None), "row_profile"),
    (dict(nbr_profile=None), "nbr_profile"), (dict(out_nbr=None), "out_nbr"),
    (dict(out_eid=None), "out_eid"), (dict(out_count=None), "out_count"),
    (dict(k=0), "k"), (dict(k=65), "k"), (dict(F=0), "F"), (dict(F=17), "F"),
    (dict(n=-1), "n"), (dict(n_rows=-1), "n_rows"),
    (dict(view=1), "ts"), (dict(view=2), "ts"), (dict(view=3), "view"),
    (dict(ts=FAKE, ts_stride=0, view=1), "ts_stride"), (dict(stage=256), "stage"),
])
def test_sample_invalid_arguments_name_the_field(kw, field):
    rc = _lib.lib().bbgr_slas_sample(ctypes.byref(_sample_args(**kw)), None)
    assert rc == -1, _err()
    assert _err().startswith("bbgr_slas_sample:") and field in _err(), _err()


def test_sample_null_args_and_empty_list():
    L = _lib.lib()
    assert L.bbgr_slas_sample(None, None) == -1 and "null args" in _err()
    a = _sample_args(n=0, rows=None, out_nbr=None, out_eid=None, out_count=None)
    assert L.bbgr_slas_sample(ctypes.byref(a), None) == 0   # no launch (there is no GPU here)
    # bad arguments are still refused for an empty list
    assert L.bbgr_slas_sample(ctypes.byref(_sample_args(n=0, k=65)), None) == -1


# -- bbgr_slas_profiles ----------------------------------------------------------
def _profiles(n_users=10, n_items=10, F=2, item_x=FAKE, ldx=2, indptr=FAKE, nbr=FAKE,
              item_norm=FAKE, user_mu=FAKE):
    return _lib.lib().bbgr_slas_profiles(n_users, n_items, F, item_x, ldx, indptr, nbr, item_norm,
                                         user_mu, None)


@pytest.mark.parametrize("kw,field", [
    (dict(F=0), "F"), (dict(F=17, ldx=17), "F"), (dict(n_users=-1), "n_users"),
    (dict(n_items=-2), "n_items"), (dict(ldx=1), "ldx"), (dict(item_x=None), "item_x"),
    (dict(indptr=None), "indptr_u"), (dict(nbr=None), "nbr_u"),
    (dict(item_norm=None), "item_norm"), (dict(user_mu=None), "user_mu"),
])
def test_profiles_invalid_arguments_name_the_field(kw, field):
    assert _profiles(**kw) == -1, _err()
    assert _err().startswith("bbgr_slas_profiles:") and field in _err(), _err()


def test_profiles_of_nothing_is_ok_without_a_launch():
    assert _profiles(n_users=0, n_items=0, item_x=None, indptr=None, nbr=None, item_norm=None,
                     user_mu=None) == 0


# -- bbgr_mark_ids32 -------------------------------------------------------------
def test_mark_ids32_validation():
    L = _lib.lib()
    assert L.bbgr_mark_ids32(-1, FAKE, 1, FAKE, 10, None) == -1 and "n < 0" in _err()
    assert L.bbgr_mark_ids32(5, FAKE, 1, FAKE, -1, None) == -1 and "n_rows" in _err()
    assert L.bbgr_mark_ids32(5, None, 1, FAKE, 10, None) == -1 and "ids" in _err()
    assert L.bbgr_mark_ids32(5, FAKE, 1, None, 10, None) == -1 and "mask" in _err()
    assert L.bbgr_mark_ids32(0, None, 1, None, 10, None) == 0


# -- bbgr_slas_induce ------------------------------------------------------------
def _induce_args(**kw):
    a = _lib.SlasInduceArgs()
    a.n_users_listed, a.n_users = 500, 1000
    a.users = a.item_local = a.indptr = a.nbr = a.eid = a.count = FAKE
    a.ts_stride = 5
    for key, v in kw.items():
        setattr(a, key, v)
    return a


def _induce(a, ws=None, nbytes=0):
    n = ctypes.c_size_t(nbytes)
    rc = _lib.lib().bbgr_slas_induce(ctypes.byref(a), ws, ctypes.byref(n), None)
    return rc, n.value


def test_induce_workspace_query_and_small_workspace():
    rc, need = _induce(_induce_args())
    assert rc == 0 and need >= 2 * 8 * 501      # counts and offsets, one past the list
    rc, _ = _induce(_induce_args(), ctypes.c_void_p(FAKE), need - 1)
    assert rc == -4 and "workspace" in _err()
    L = _lib.lib()
    assert L.bbgr_slas_induce(None, None, ctypes.byref(ctypes.c_size_t(0)), None) == -1
    assert "null args" in _err()
    assert L.bbgr_slas_induce(ctypes.byref(_induce_args()), None, None, None) == -1
    assert "workspace_bytes" in _err()


@pytest.mark.parametrize("kw,field", [
    (dict(users=None), "users"), (dict(item_local=None), "item_local"),
    (dict(indptr=None), "indptr"), (dict(nbr=None), "nbr"), (dict(eid=None), "eid"),
    (dict(count=None), "count"), (dict(n_users_listed=-1), "n_users_listed"),
    (dict(n_users=-1), "n_users"), (dict(view=1), "ts"), (dict(view=7), "view"),
    (dict(capacity=-1), "capacity"), (dict(out_edges=FAKE), "out_eid"),
    (dict(out_eid=FAKE), "out_edges"),
])
def test_induce_invalid_arguments_name_the_field(kw, field):
    a = _induce_args(**kw)
    _, need = _induce(_induce_args())
    rc, _ = _induce(a, ctypes.c_void_p(FAKE), need)
    assert rc == -1, _err()
    assert _err().startswith("bbgr_slas_induce:") and field in _err(), _err()


def test_induce_of_no_users_is_ok_without_a_launch():
    a = _induce_args(n_users_listed=0, users=None)
    rc, need = _induce(a)
    assert rc == 0
    rc, _ = _induce(a, ctypes.c_void_p(FAKE), need)
    assert rc == 0, _err()


# -- host planner and files --------------------------------------------------------
def test_host_plan_equals_the_literal_restatement():
    """Labeled split and first-epoch batch order: default_rng(42), one shuffle
    of the labeled users, the 80 % cut, one shuffle of the train users
    (main.py:885-919)."""
    import torch
    from bbgr.cred_train import HostPlan
    y = np.random.default_rng(3).integers(-1, 2, 1000)
    rng = np.random.default_rng(42)
    labeled = (torch.tensor(y).long() >= 0).nonzero(as_tuple=False).view(-1).numpy()
    rng.shuffle(labeled)
    split = int(0.8 * labeled.size)
    train = labeled[:split]
    want_split = train.copy()
    rng.shuffle(train)
    want_batches = [train[j:j + 128] for j in range(0, len(train), 128)]

    plan = HostPlan(torch.tensor(y), seed=42)
    np.testing.assert_array_equal(plan.train_users, want_split)
    assert plan.train_users.dtype == np.int64
    got = plan.epoch_batches(128)
    assert len(got) == len(want_batches)
    for a, b in zip(got, want_batches):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(RuntimeError, match="No labeled users"):
        HostPlan(np.full(10, -1))


def test_minmax_and_csv_round_trip(tmp_path):
    from bbgr import ingest
    from bbgr.cred_train import minmax_normalize, write_credibility_csv
    raw = np.random.default_rng(0).uniform(0.2, 0.9, 50).astype(np.float32)
    c = minmax_normalize(raw)
    assert c.dtype == np.float32 and c.min() == 0.0 and c.max() == 1.0
    assert not minmax_normalize(np.full(7, 0.25, np.float32)).any()    # constant scores: zeros
    idx2user = [f"user{j}" for j in range(48)]                           # two users without an id
    p = tmp_path / "credibility_scores_minmax_with_user_id.csv"
    write_credibility_csv(p, c, idx2user)
    lines = p.read_text().splitlines()
    assert lines[0] == "user_id,user_idx,credibility"
    assert lines[1] == f"user0,0,{float(c[0]):.6f}" and lines[50] == f",49,{float(c[49]):.6f}"
    want = np.array([float(f"{float(v):.6f}") for v in c], np.float32)
    np.testing.assert_array_equal(ingest.load_credibility_csv(p, 50), want)
    by_id = ingest.load_credibility_csv(p, 50, {u: j for j, u in enumerate(idx2user)})
    np.testing.assert_array_equal(by_id[:48], want[:48])
    np.save(tmp_path / "credibility_scores_minmax.npy", c)
    np.testing.assert_array_equal(
        ingest.load_credibility_npy(tmp_path / "credibility_scores_minmax.npy", 50), c)
