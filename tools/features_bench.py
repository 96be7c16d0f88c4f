"""Benchmark: review columns -> credibility graph tensors on MI355X.

    python tools/features_bench.py [--config C2] [--reps 10] [--host] [--feature-set main|v2]
                                   [--out profiles/features/features_c2.json]

Workload: synthetic review columns over the interaction graph of a config (C2:
100k users x 50k items, 1M records; C4: 5M x 1M, 50M records; Zipf items, so hub
rows exist), in shuffled (file) order: half-star ratings, 10 % of the records
without a timestamp, timestamps over ten years, token counts 0..200.

Each launch group of bbgr.features.build_credibility_graph is timed alone with
device events (median of --reps after --warmup) and set against the bytes it
has to move (the inputs it reads once plus the outputs it writes; gathers
counted at their payload, index arrays included) and the 8 TB/s of HBM:

  stats, buckets, edges          streaming passes over the records (csrc/features.hip)
  items, users                   one row per item / user, gathers by record id
  group_users / _items / _buckets  the three bbgr_csr_build (radix sort; time only)

--feature-set v2 times the launches of the v2 build (main_v2_.py's features:
the same groups plus lenlog and item means inside stats / items, and pooled,
gaps and the v2 users pass) on the same columns with the 1M-review corpus of
tools/text_bench.py as their text and its token counts as n_tokens; `pooled`
is the whole bbgr.text.pooled_token_counts (its upload of the text and its
host reads included). Default --out: profiles/features_v2/features_v2_c2.json.

`build_ms` is one whole call from device-resident columns (host clock, one
device read inside); `upload_ms` the host -> device copy of the columns.
With --host the host restatement (tests/features_ref.py: the reference's
dictionaries and loops over the same columns, json parsing not included) is
timed once: the only baseline there is. Prints ONE JSON line; writes --out.
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
from bbgr import features as FT  # noqa: E402
from bbgr.synthetic import CONFIGS, config_edges  # noqa: E402

HBM_PEAK = 8.0e12
TAU = FT.TAU_MS


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def synthetic_columns(config: str, seed: int = 0) -> FT.ReviewColumns:
    e = np.asarray(config_edges(config))
    E = e.shape[1]
    rng = np.random.default_rng(seed)
    order = rng.permutation(E)
    n_tokens = rng.integers(0, 200, E, dtype=np.int32)
    return FT.ReviewColumns(
        user=e[0][order].astype(np.int32), item=e[1][order].astype(np.int32),
        rating=(rng.integers(2, 11, E) * 0.5).astype(np.float32),
        helpful_vote=rng.geometric(0.25, E).astype(np.int32) - 1,
        verified=(rng.uniform(size=E) < 0.8).astype(np.uint8),
        timestamp=rng.integers(1_400_000_000_000, 1_400_000_000_000 + 3650 * TAU, E),
        n_tokens=n_tokens,
        n_unique_tokens=(n_tokens * rng.uniform(0.5, 1.0, E)).astype(np.int32),
        ts_valid=rng.uniform(size=E) >= 0.1)


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


def bytes_moved(E: int, U: int, I: int, n_ts: int) -> dict:
    """Inputs read once + outputs written, per launch group."""
    return {
        # n_tokens, timestamp, ts_valid
        "stats": E * (4 + 8 + 1),
        # user, timestamp, ts_valid -> row, column
        "buckets": E * (4 + 8 + 1) + E * 8,
        # record id, rating per record; indptr, item_x, item_rbar per item
        "items": E * (4 + 4) + I * (4 + 8 + 8),
        # the pack launch (item, n_tokens, n_unique, rating, helpful_vote -> 16 bytes), then
        # record id, packed record, item_rbar per record; a bucket per record with a timestamp;
        # two indptr, user_x, user_y, two counts per user
        "users": E * (20 + 16) + E * (4 + 16 + 8) + n_ts * 4 + U * (8 + 28 + 8 + 8),
        # rating, item, item mean, verified, timestamp, ts_valid, helpful_vote -> 5 floats
        "edges": E * (4 + 4 + 4 + 1 + 8 + 1 + 4) + E * 20,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host", action="store_true", help="also time the host restatement")
    ap.add_argument("--out", default=None)
    ap.add_argument("--feature-set", default="main", choices=FT.FEATURE_SETS)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("features_bench needs a GPU: no timing is taken without one")
    v2 = args.feature_set == "v2"
    out_path = args.out or os.path.join(
        ROOT, "profiles", "features_v2" if v2 else "features",
        f"features{'_v2' if v2 else ''}_{args.config.lower()}.json")
    cfg = CONFIGS[args.config]
    U, I = cfg["num_users"], cfg["num_items"]
    t0 = time.perf_counter()
    cols = synthetic_columns(args.config)
    E = len(cols)
    log(f"columns drawn in {time.perf_counter() - t0:.1f} s: E = {E}")
    if v2:
        if args.host:
            raise SystemExit("--host times the main restatement only")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from text_bench import synthetic_corpus
        from bbgr import text as TX
        cols.text = synthetic_corpus(E)
        n_tok, n_uniq, _ = TX.token_counts(cols.text, "cuda")
        cols.n_tokens, cols.n_unique_tokens = n_tok.cpu().numpy(), n_uniq.cpu().numpy()
    rec = {"config": args.config, "feature_set": args.feature_set, "users": U, "items": I, "records": E,
           "max_user_degree": int(np.bincount(cols.user, minlength=U).max()),
           "max_item_degree": int(np.bincount(cols.item, minlength=I).max()),
           "device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12}
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    on_dev = FT.ReviewColumns(**{k: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
                                 for k, v in cols.__dict__.items() if k != "text"})
    torch.cuda.synchronize()
    rec["upload_ms"] = (time.perf_counter() - t0) * 1e3
    if v2:
        on_dev.text = cols.text          # host bytes: the pooled call uploads them itself
        rec["text_bytes"] = int(cols.text.data.shape[0])

    p = (FT._PipelineV2 if v2 else FT._Pipeline)(on_dev, U, I, E, dev)
    p.stats()
    p.read_stats()
    moved = bytes_moved(E, U, I, p.n_ts)
    kernels = {}
    for step in p.STEPS:
        if step == "read_stats":
            continue
        r = timed_events(getattr(p, step), args.warmup, args.reps)
        if step in moved and not (v2 and step in ("stats", "items", "users")):
            r["bytes"] = moved[step]
            r["TBps"] = moved[step] / (r["median_ms"] * 1e-3) / 1e12
            r["of_hbm_peak"] = r["TBps"] * 1e12 / HBM_PEAK
        kernels[step] = r
        log(step, r)
    rec["kernels"] = kernels
    rec["kernels_sum_ms"] = sum(r["median_ms"] for r in kernels.values())

    def build():
        return FT.build_credibility_graph(on_dev, U, I, dev, feature_set=args.feature_set)

    ts = []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = build()
        torch.cuda.synchronize()
        if k >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    rec["build_ms"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                       "reps": args.reps}
    log("build_ms", rec["build_ms"])
    rec["labels"] = {str(v): int((out.user_y == v).sum()) for v in (-1, 0, 1)}
    if args.host:
        import features_ref as FR
        t0 = time.perf_counter()
        ref = FR.features_ref(cols, U, I)
        rec["host_restatement_s"] = time.perf_counter() - t0
        log("host_restatement_s", rec["host_restatement_s"])
        ux, rx = out.user_x.cpu().numpy(), ref["user_x"]
        nan = np.isnan(rx)
        d = np.abs(ux.view(np.int32).astype(np.int64) - rx.view(np.int32).astype(np.int64))
        d[nan] = 0
        rec["vs_host"] = {
            "user_x_max_ulp": int(d.max()), "nan_rows_equal": bool((np.isnan(ux) == nan).all()),
            "user_y_equal": bool((out.user_y.cpu().numpy() == ref["user_y"]).all()),
            "item_x_equal": bool((out.item_x.cpu().numpy() == ref["item_x"]).all()),
            "edge_attr_equal": bool(np.array_equal(out.edge_attr.cpu().numpy(), ref["edge_attr"],
                                                   equal_nan=True))}
        log("vs_host", rec["vs_host"])
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
