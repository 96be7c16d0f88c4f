"""Benchmark: review columns -> train / val / test edges on MI355X.

    python tools/split_bench.py [--config C2] [--reps 10] [--host]
                                [--out profiles/split/split_c2.json]

Workload: the records of a config's interaction graph (C2: 100k users x 50k
items, 1M records; C4: 5M x 1M, 50M records; Zipf items, so hub ids exist) in
shuffled (file) order with half-star ratings 1..5 (a third positive at the
default threshold), and synthetic printable ids of 28 bytes per user and 10 per
item, the dataset's shapes.

Each launch group of bbgr.split.split_interactions is timed alone with device
events (median of --reps after --warmup) and set against the bytes it has to
move (inputs read once plus outputs written, gathers at their payload) and the
8 TB/s of HBM:

  md5     bbgr_md5_pair_hash over the positive records (keep mask): one launch
  split   bbgr_split_edges: two memsets and five launches (first record per id,
          codes + tile counts, tile scan, ids, edges)

`call_ms` is one whole split_interactions from device-resident columns and id
tables already encoded (host clock; the id tables' upload and the one device
read inside); `upload_ms` the host -> device copy of the three columns. With
--host the host restatement (tests/split_ref.py: the reference's hashlib and
dictionaries over the same columns and id strings, json parsing not included)
is timed once and compared: the only baseline there is. Prints ONE JSON line;
writes --out.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bbgr  # noqa: E402,F401
from bbgr import split as SP  # noqa: E402
from bbgr.synthetic import CONFIGS, config_edges  # noqa: E402

HBM_PEAK = 8.0e12
USER_ID_BYTES, ITEM_ID_BYTES = 28, 10


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def synthetic_ids(n: int, width: int, rng) -> SP.IdTable:
    """n printable ASCII ids of `width` bytes each."""
    data = rng.integers(48, 123, (n, width), dtype=np.uint8)
    return SP.IdTable(data.reshape(-1), np.arange(n + 1, dtype=np.int64) * width)


def id_strings(t: SP.IdTable, width: int) -> list:
    return [b.decode("ascii") for b in np.asarray(t.data).view(f"S{width}").tolist()]


def timed_events(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def bytes_moved(n: int, P: int, U: int, I: int, first_u: int, first_i: int) -> dict:
    """Inputs read once + outputs written, per launch group (P positives)."""
    return {
        # keep per record; per positive: user, item, two offset pairs, the id bytes, the hash
        "md5": n + P * (4 + 4 + 16 + 16 + USER_ID_BYTES + ITEM_ID_BYTES + 4),
        # memsets; first: user, item, rating; codes: user, item, rating, code, and per positive
        # hash and two map reads; ids: code, per first record id + list + map; edges: code, per
        # positive user, item, two map reads, two stores
        "split": (U + I) * 4 + n * 12 + n * 13 + P * 12 + n + (first_u + first_i) * 12
                 + n + P * 24,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host", action="store_true", help="also time the host restatement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("split_bench needs a GPU: no timing is taken without one")
    out_path = args.out or os.path.join(ROOT, "profiles", "split",
                                        f"split_{args.config.lower()}.json")
    cfg = CONFIGS[args.config]
    U, I = cfg["num_users"], cfg["num_items"]
    t0 = time.perf_counter()
    e = np.asarray(config_edges(args.config))
    n = e.shape[1]
    rng = np.random.default_rng(0)
    order = rng.permutation(n)
    user, item = e[0][order].astype(np.int32), e[1][order].astype(np.int32)
    rating = (rng.integers(2, 11, n) * 0.5).astype(np.float32)
    ut, it = synthetic_ids(U, USER_ID_BYTES, rng), synthetic_ids(I, ITEM_ID_BYTES, rng)
    log(f"columns and ids drawn in {time.perf_counter() - t0:.1f} s: n = {n}")
    rec = {"config": args.config, "users": U, "items": I, "records": n,
           "user_id_bytes": USER_ID_BYTES, "item_id_bytes": ITEM_ID_BYTES,
           "max_user_degree": int(np.bincount(user, minlength=U).max()),
           "max_item_degree": int(np.bincount(item, minlength=I).max()),
           "device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12}
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d_user, d_item, d_rating = (torch.from_numpy(x).to(dev) for x in (user, item, rating))
    torch.cuda.synchronize()
    rec["upload_ms"] = (time.perf_counter() - t0) * 1e3

    # the launch groups, on the buffers split_interactions would make
    i32 = dict(dtype=torch.int32, device=dev)
    utab = (SP._bytes_dev(np.asarray(ut.data), dev), torch.from_numpy(ut.offsets).to(dev))
    itab = (SP._bytes_dev(np.asarray(it.data), dev), torch.from_numpy(it.offsets).to(dev))
    keep = (d_rating >= 4.0).view(torch.uint8)
    h = torch.zeros(n, **i32)
    edges, counts = torch.empty(2, n, **i32), torch.zeros(5, dtype=torch.int64, device=dev)
    umap, imap = torch.empty(U, **i32), torch.empty(I, **i32)
    usrc, isrc = torch.empty(U, **i32), torch.empty(I, **i32)
    thr = SP.split_thresholds()
    groups = {
        "md5": lambda: SP._launch_hash(d_user, d_item, utab, itab, keep, h),
        "split": lambda: SP._run_split(d_user, d_item, None, d_rating, 4.0, h, thr, U, I, umap,
                                       imap, usrc, isrc, edges, counts),
    }
    kernels = {}
    for name, fn in groups.items():
        kernels[name] = timed_events(fn, args.warmup, args.reps)
    e_tr, e_va, e_te, n_u, n_i = (int(v) for v in counts.tolist())
    P = e_tr + e_va + e_te
    rec.update(positives=P, train=e_tr, val=e_va, test=e_te, new_users=n_u, new_items=n_i)
    moved = bytes_moved(n, P, U, I, n_u, n_i)
    for name, r in kernels.items():
        r["bytes"] = moved[name]
        r["TBps"] = moved[name] / (r["median_ms"] * 1e-3) / 1e12
        r["of_hbm_peak"] = r["TBps"] * 1e12 / HBM_PEAK
        r["ns_per_record"] = r["median_ms"] * 1e6 / n
        log(name, r)
    kernels["md5"]["ns_per_hashed_record"] = kernels["md5"]["median_ms"] * 1e6 / max(P, 1)
    rec["kernels"] = kernels
    rec["kernels_sum_ms"] = sum(r["median_ms"] for r in kernels.values())

    ts = []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = SP.split_interactions(d_user, d_item, d_rating, ut, it, device=dev)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    rec["call_ms"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                      "reps": args.reps}
    log("call_ms", rec["call_ms"])
    # the host's share of a call: the id tables' checks and their upload
    t0 = time.perf_counter()
    tabs = [SP._host_table(t, "ids") for t in (ut, it)]
    rec["call_table_checks_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    held = [(SP._bytes_dev(d, dev), torch.from_numpy(o).to(dev)) for d, o in tabs]
    torch.cuda.synchronize()
    rec["call_table_upload_ms"] = (time.perf_counter() - t0) * 1e3
    del held
    t0 = time.perf_counter()
    SP._check_columns(d_user, d_item, U, I, rating=d_rating)
    rec["call_id_range_ms"] = (time.perf_counter() - t0) * 1e3
    if args.host:
        import split_ref as SR
        uids, iids = id_strings(ut, USER_ID_BYTES), id_strings(it, ITEM_ID_BYTES)
        t0 = time.perf_counter()
        ref = SR.split(user, item, rating, uids, iids)
        rec["host_restatement_s"] = time.perf_counter() - t0
        log("host_restatement_s", rec["host_restatement_s"])
        rec["vs_host"] = {k: bool(np.array_equal(getattr(out, k).cpu().numpy(), ref[k]))
                          for k in ("train", "val", "test", "user_src", "item_src")}
        log("vs_host", rec["vs_host"])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
