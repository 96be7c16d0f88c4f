#!/usr/bin/env python3
"""The workspace size every `(void *workspace, size_t *workspace_bytes)` entry
point of libbbgr.so reports, at two fixed shapes each (one tiny, one large;
both paths where the size depends on one): one JSON object
{entry: {shape label: bytes, or the negative bbgr_status of a refused query}}.

    python tools/workspace_sizes.py                    # the built library
    BBGR_LIB=/other/libbbgr.so python tools/workspace_sizes.py

Two builds that print the same object size their workspaces alike. ctypes
and fake non-null pointers only: a size query reads no array and launches
nothing. hipcub asks the runtime for a device while it sizes a scan, a
DeviceSelect::If or a larger radix sort, so without a GPU the entries of
DEVICE_QUERIES (and the larger sorts of the graph build) answer BBGR_ERR_HIP
or leave hipcub's share out; the numbers also depend on the installed
rocprim. Compare builds on one machine.

CASES is also the entry list of tests/test_workspace_abi.py.
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bbgr import _lib  # noqa: E402

FAKE = 16   # a non-null, 16-byte aligned address that is never dereferenced
# entries whose size is hipcub's alone, or whose query reports hipcub's error:
# without a device they answer BBGR_ERR_HIP (the first five) or 0 bytes
DEVICE_QUERIES = ("bbgr_csr_plan_build", "bbgr_csr_plan_count", "bbgr_mask_to_list",
                  "bbgr_nonempty_rows", "bbgr_pop_cdf", "bbgr_ids_table", "bbgr_jsonl_offsets")


def _struct(cls, **kw):
    s = cls()
    for k, v in kw.items():
        setattr(s, k, v)
    return ctypes.byref(s)


def _csr(n_rows, nnz, n_chunks=0):
    return _struct(_lib.CsrStruct, n_rows=n_rows, n_cols=n_rows, nnz=nnz, indptr=FAKE,
                   indices=FAKE, n_chunks=n_chunks)


def _eval(n_users, n_items):
    return _struct(_lib.EvalArgs, n_users=n_users, users=FAKE, te_indptr=FAKE, te_indices=FAKE,
                   tr_indptr=FAKE, tr_indices=FAKE, uf=FAKE, lduf=64, itf=FAKE, ldif=64, d=64,
                   n_items=n_items, n_neg=99, k_max=20, n_k=2, ks=(ctypes.c_int32 * 8)(10, 20),
                   item_pop=FAKE, pos_rank=FAKE, topk=FAKE, sums=FAKE)


def _rec(cls, n_users, n_items, k):
    return _struct(cls, n_users=n_users, users=FAKE, n_user_rows=n_users, uf=FAKE, lduf=64,
                   itf=FAKE, ldif=64, d=64, n_items=n_items, k=k, topk=FAKE)


def _feat(n, n_users, n_items):
    return _struct(_lib.FeatColumns, n=n, n_users=n_users, n_items=n_items, user=FAKE, item=FAKE,
                   rating=FAKE, helpful_vote=FAKE, verified=FAKE, timestamp=FAKE, ts_valid=FAKE,
                   n_tokens=FAKE, n_unique_tokens=FAKE)


def _text(n, n_bytes):
    return _struct(_lib.TextArgs, n=n, data=FAKE, offsets=FAKE, first=0, last=n_bytes,
                   n_tokens=FAKE, n_unique_tokens=FAKE, recheck=FAKE, totals=FAKE)


def _gather(n_list, n, n_bytes):
    return _struct(_lib.TextGatherArgs, n_list=n_list, records=FAKE, n=n, data=FAKE, offsets=FAKE,
                   first=0, last=n_bytes, out_offsets=FAKE, out_data=FAKE, capacity=n_bytes,
                   total=FAKE)


def _jsonl(n_bytes, n_lines):
    return _struct(_lib.JsonlArgs, n_bytes=n_bytes, data=FAKE, n_lines=n_lines, line_end=FAKE,
                   status=FAKE, rating=FAKE, helpful_vote=FAKE, verified=FAKE, timestamp=FAKE,
                   ts_valid=FAKE, sizes=FAKE, spos=FAKE, totals=FAKE, offs=FAKE)


def _split(n):
    return _struct(_lib.SplitArgs, n=n, n_users=50, n_items=40, user=FAKE, item=FAKE, rating=FAKE,
                   hash32=FAKE, pos_threshold=4.0, thr_train=3435973836, thr_val=3865470566,
                   user_map=FAKE, item_map=FAKE, user_src=FAKE, item_src=FAKE, edges=FAKE,
                   ld_edges=n, counts=FAKE)


# entry -> [(shape label, arguments before `workspace`)]; the stream (null) follows
# `workspace_bytes` in every entry
CASES = {
    "bbgr_csr_build": [
        ("nnz=1000,50x60", (1000, FAKE, FAKE, 50, 60, FAKE, FAKE, None)),
        ("nnz=5000000,200000x100000", (5_000_000, FAKE, FAKE, 200_000, 100_000, FAKE, FAKE, FAKE))],
    "bbgr_csr_plan_count": [
        ("rows=77", (_csr(77, 1000), None, None)),
        ("rows=1000000", (_csr(1_000_000, 5_000_000), None, None))],
    "bbgr_csr_plan_build": [
        ("rows=77", (_csr(77, 1000), FAKE, FAKE)),
        ("rows=1000000", (_csr(1_000_000, 5_000_000), FAKE, FAKE))],
    "bbgr_degree_count_ws": [
        ("ids=1000,n=77 (atomics)", (1000, FAKE, 77, FAKE)),
        ("ids=4194304,n=100000 (sort)", (1 << 22, FAKE, 100_000, FAKE))],
    "bbgr_degree_order": [("n=1000", (1000, FAKE, FAKE, FAKE)),
                          ("n=3000000", (3_000_000, FAKE, FAKE, FAKE))],
    "bbgr_ewa_normalize": [
        ("rows=77,nnz=1000,own raw", (_csr(77, 1000), FAKE, None, None, FAKE, 4, 0, 1, 0.5, 0.5,
                                      1e-8, None, FAKE, FAKE)),
        ("rows=1000000,nnz=5000000,chunks=300,w_in",
         (_csr(1_000_000, 5_000_000, 300), FAKE, None, FAKE, None, 0, 0, 0, 0.5, 0.5, 1e-8, None,
          FAKE, FAKE))],
    "bbgr_scatter_add_rows": [
        ("n=1000,n_dst=500", (1000, FAKE, FAKE, 64, FAKE, 64, 64, 500)),
        ("n=2000000,n_dst=1000000", (2_000_000, FAKE, FAKE, 64, FAKE, 64, 64, 1_000_000))],
    "bbgr_scatter_plan": [("n=1000,n_dst=500", (1000, FAKE, 500)),
                          ("n=2000000,n_dst=1000000", (2_000_000, FAKE, 1_000_000))],
    "bbgr_pop_cdf": [("items=1000", (1000, FAKE, 0.75, FAKE)),
                     ("items=2000000", (2_000_000, FAKE, 0.75, FAKE))],
    "bbgr_shuffle": [("n=1000", (1000, FAKE, FAKE, 7, 0)),
                     ("n=5000000", (5_000_000, FAKE, FAKE, 7, 0))],
    "bbgr_eval_sampled": [("users=100,items=300", (_eval(100, 300),)),
                          ("users=20000,items=100000", (_eval(20_000, 100_000),))],
    "bbgr_eval_full": [("users=100,items=300", (_eval(100, 300),)),
                       ("users=20000,items=100000", (_eval(20_000, 100_000),))],
    "bbgr_eval_lists": [("users=100,items=300", (_eval(100, 300),)),
                        ("users=20000,items=100000", (_eval(20_000, 100_000),))],
    "bbgr_recommend": [
        ("users=100,items=300,k=10", (_rec(_lib.RecommendArgs, 100, 300, 10),)),
        ("users=20000,items=100000,k=100", (_rec(_lib.RecommendArgs, 20_000, 100_000, 100),))],
    "bbgr_recommend_bf16": [
        ("users=100,items=300,k=10", (_rec(_lib.RecommendBf16Args, 100, 300, 10),)),
        ("users=20000,items=100000,k=100", (_rec(_lib.RecommendBf16Args, 20_000, 100_000, 100),))],
    "bbgr_nonempty_rows": [("rows=1000", (1000, FAKE, FAKE, FAKE)),
                           ("rows=3000000", (3_000_000, FAKE, FAKE, FAKE))],
    "bbgr_mask_to_list": [("n=1000", (1000, FAKE, FAKE, FAKE)),
                          ("n=3000000", (3_000_000, FAKE, FAKE, FAKE))],
    "bbgr_slas_induce": [
        ("users=100", (_struct(_lib.SlasInduceArgs, n_users_listed=100, n_users=100),)),
        ("users=1000000", (_struct(_lib.SlasInduceArgs, n_users_listed=1_000_000,
                                   n_users=1_000_000),))],
    "bbgr_feat_items": [("n=1000", (_feat(1000, 50, 40), FAKE, FAKE, FAKE, FAKE)),
                        ("n=5000000", (_feat(5_000_000, 400_000, 90_000), FAKE, FAKE, FAKE, FAKE))],
    "bbgr_feat_users": [
        ("n=1000", (_feat(1000, 50, 40), _struct(_lib.FeatUserArgs))),
        ("n=5000000", (_feat(5_000_000, 400_000, 90_000), _struct(_lib.FeatUserArgs)))],
    "bbgr_feat_lenlog": [("n=1000", (_feat(1000, 50, 40), FAKE)),
                         ("n=5000000", (_feat(5_000_000, 400_000, 90_000), FAKE))],
    "bbgr_feat_item_means": [
        ("n=1000", (_feat(1000, 50, 40), FAKE, FAKE, FAKE)),
        ("n=5000000", (_feat(5_000_000, 400_000, 90_000), FAKE, FAKE, FAKE))],
    "bbgr_feat_gaps": [("n=1000", (_feat(1000, 50, 40), FAKE, FAKE, FAKE)),
                       ("n=5000000", (_feat(5_000_000, 400_000, 90_000), FAKE, FAKE, FAKE))],
    "bbgr_feat_users_v2": [
        ("n=1000", (_feat(1000, 50, 40), _struct(_lib.FeatUserV2Args))),
        ("n=5000000", (_feat(5_000_000, 400_000, 90_000), _struct(_lib.FeatUserV2Args)))],
    "bbgr_split_edges": [("n=1000", (_split(1000),)), ("n=5000000", (_split(5_000_000),))],
    "bbgr_text_unique": [
        ("n=1000,tokens=20000", (_text(1000, 100_000), 20_000)),
        ("n=1000000,tokens=60000000", (_text(1_000_000, 400_000_000), 60_000_000))],
    "bbgr_text_unique_stages": [
        ("n=1000,tokens=20000,sort", (_text(1000, 100_000), 20_000, 2)),
        ("n=1000000,tokens=60000000,all", (_text(1_000_000, 400_000_000), 60_000_000, 7))],
    "bbgr_text_unique_pooled": [
        ("n=1000,tokens=20000,groups=50",
         (_text(1000, 100_000), 20_000, FAKE, 50, FAKE, FAKE, FAKE)),
        ("n=1000000,tokens=60000000,groups=400000",
         (_text(1_000_000, 400_000_000), 60_000_000, FAKE, 400_000, FAKE, FAKE, FAKE))],
    "bbgr_text_unique_pooled_stages": [
        ("n=1000,tokens=20000,groups=50,sort",
         (_text(1000, 100_000), 20_000, FAKE, 50, FAKE, FAKE, FAKE, 2)),
        ("n=1000000,tokens=60000000,groups=400000,all",
         (_text(1_000_000, 400_000_000), 60_000_000, FAKE, 400_000, FAKE, FAKE, FAKE, 7))],
    "bbgr_text_gather": [("list=1000,n=1000", (_gather(1000, 1000, 100_000),)),
                         ("list=5000000,n=5000000", (_gather(5_000_000, 5_000_000, 1 << 31),))],
    "bbgr_text_gather_fetch": [
        ("list=1000,n=1000,unaligned", (_gather(1000, 1000, 100_000), 0)),
        ("list=5000000,n=5000000,aligned pair", (_gather(5_000_000, 5_000_000, 1 << 31), 1))],
    "bbgr_jsonl_lines": [("bytes=100000,lines=300", (_jsonl(100_000, 300),)),
                         ("bytes=2000000000,lines=3000000", (_jsonl(2_000_000_000, 3_000_000),))],
    "bbgr_jsonl_offsets": [("bytes=100000,lines=300", (_jsonl(100_000, 300),)),
                           ("bytes=2000000000,lines=3000000", (_jsonl(2_000_000_000, 3_000_000),))],
    "bbgr_ids_number": [("n=1000", (1000, FAKE, FAKE, 20_000, 0, FAKE, FAKE, FAKE)),
                        ("n=5000000", (5_000_000, FAKE, FAKE, 100_000_000, 0, FAKE, FAKE, FAKE))],
    "bbgr_ids_table": [
        ("ids=300,n=1000", (300, FAKE, 1000, FAKE, FAKE, 20_000, FAKE, None, 0)),
        ("ids=400000,n=5000000", (400_000, FAKE, 5_000_000, FAKE, FAKE, 100_000_000, FAKE, None,
                                  0))],
}


def run(entry, before, workspace, n_bytes):
    """One call of `entry`: `n_bytes` is a ctypes.c_size_t, or None for a null pointer."""
    return getattr(_lib.lib(), entry)(*before, workspace,
                                      None if n_bytes is None else ctypes.byref(n_bytes), None)


def query(entry, before):
    """The bytes `entry` asks for, or its negative status."""
    n = ctypes.c_size_t(0)
    rc = run(entry, before, None, n)
    return n.value if rc == 0 else rc


def table():
    return {entry: {label: query(entry, before) for label, before in cases}
            for entry, cases in CASES.items()}


if __name__ == "__main__":
    print(json.dumps(table(), indent=1, sort_keys=True))
