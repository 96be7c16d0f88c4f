"""Benchmark: SLAS subgraph sampling and one credibility training step on MI355X.

    python tools/slas_bench.py [--config C2] [--batch 2048] [--k 15] [--reps 15]
                               [--out profiles/slas/slas_c2.json] [--time-limit 420]

Workload: the C2 synthetic interaction graph (100k users x 50k items, 1M edges,
Zipf items, so hub item rows exist) as the credibility graph, with F = 2 item
features, 5 edge attribute columns, 6 user features and 30 % labeled users.
Timed, each as the median of `reps` runs after `warmup` (host clock around
work that ends in a device synchronise):

  build_subgraph_{none,early,late}_ms  one SlasGraph.build_subgraph call
  sample_items_ms / sample_users_ms    its two bbgr_slas_sample launches alone
                                       (device events), the second also over
                                       the 64 longest item rows only
  train_step_ms                        two views + forward + backward + Adam
  export_pass_s                        every user, in batches (3 runs)
  host_loop_s                          tests/slas_ref.py's literal host loop,
                                       one batch, one view (the baseline)

Phases that would start after --time-limit seconds are left "not measured".
Writes the record to --out and prints it as ONE JSON line on stdout.
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
from bbgr.cred_gnn import CredModel  # noqa: E402
from bbgr.cred_train import SlasGraph, export_credibility, step_loss  # noqa: E402
from bbgr.synthetic import CONFIGS, config_edges  # noqa: E402


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn, warmup, reps):
    """Median and spread (ms) of fn() by the host clock; fn's work is
    synchronised before the clock is read."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "reps": reps}


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
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--time-limit", type=float, default=420.0)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slas", "slas_c2.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slas_bench needs a GPU: no timing is taken without one")
    t_start = time.perf_counter()
    left = lambda: args.time_limit - (time.perf_counter() - t_start)  # noqa: E731
    cfg = CONFIGS[args.config]
    U, I = cfg["num_users"], cfg["num_items"]
    e = np.asarray(config_edges(args.config)).astype(np.int64)
    E = e.shape[1]
    rng = np.random.default_rng(0)
    ea = rng.uniform(0, 1, (E, 5)).astype(np.float32)
    user_x = rng.normal(size=(U, 6)).astype(np.float32)
    user_y = np.where(rng.uniform(size=U) < 0.3, rng.integers(0, 2, U), -1).astype(np.int64)
    item_x = rng.normal(size=(I, 2)).astype(np.float32)
    deg_i = np.bincount(e[1], minlength=I)
    rec = {"config": args.config, "users": U, "items": I, "edges": E, "batch": args.batch,
           "k": args.k, "hidden": args.hidden, "F": 2, "attr_cols": 5,
           "max_item_degree": int(deg_i.max()), "max_user_degree": int(np.bincount(e[0]).max()),
           "device": torch.cuda.get_device_name(0)}
    t0 = time.perf_counter()
    g = SlasGraph(e, ea, user_x, user_y, item_x, "cuda")
    torch.cuda.synchronize()
    rec["graph_build_s"] = time.perf_counter() - t0
    seeds = torch.from_numpy(rng.permutation(U)[: args.batch].astype(np.int64)).cuda()
    kw = dict(k_item=args.k, k_user=args.k)
    for view in (None, "early", "late"):
        name = f"build_subgraph_{view or 'none'}_ms"
        rec[name] = timed(lambda: g.build_subgraph(seeds, view, counter=1, **kw), args.warmup,
                          args.reps)
        sub = g.build_subgraph(seeds, view, counter=1, **kw)
        rec[name].update(users=int(sub["users_global"].numel()),
                         items=int(sub["items_global"].numel()), edges=int(sub["e_u2i"].shape[1]))
        log(name, rec[name])
    # the two sampling launches alone
    sub = g.build_subgraph(seeds, None, counter=1, **kw)
    items = sub["items_global"]
    rec["sample_items_ms"] = timed_events(
        lambda: g.sample(seeds, "user", args.k, counter=1, stage=0), args.warmup, args.reps)
    rec["sample_users_ms"] = timed_events(
        lambda: g.sample(items, "item", args.k, upweight=1.0, counter=1, stage=1), args.warmup,
        args.reps)
    hubs = torch.from_numpy(np.argsort(-deg_i)[:64].astype(np.int64)).cuda()
    rec["sample_users_64_longest_rows_ms"] = timed_events(
        lambda: g.sample(hubs, "item", args.k, upweight=1.0, counter=1, stage=1), args.warmup,
        args.reps)
    rec["sample_users_64_longest_rows_ms"]["slots"] = int(np.sort(deg_i)[-64:].sum())
    rec["sample_users_ms"]["slots"] = int(deg_i[items.cpu().numpy()].sum())
    log("samples", rec["sample_items_ms"], rec["sample_users_ms"],
        rec["sample_users_64_longest_rows_ms"])
    # one training step
    torch.manual_seed(0)
    model = CredModel(6, 2, args.hidden).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    state = {"c": 0}

    def step():
        g1 = g.build_subgraph(seeds, "early", counter=state["c"], **kw)
        g2 = g.build_subgraph(seeds, "late", counter=state["c"] + 1, **kw)
        state["c"] += 2
        opt.zero_grad()
        loss = step_loss(model, g1, g2)
        loss.backward()
        opt.step()
        return loss

    if left() > 60:
        rec["train_step_ms"] = timed(step, args.warmup, args.reps)
        log("train_step_ms", rec["train_step_ms"])
    else:
        rec["train_step_ms"] = "not measured"
    if left() > 120:
        ts = []
        for r in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            export_credibility(g, model, args.batch, counter=1000 * (r + 1))
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        rec["export_pass_s"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts),
                                "reps": 3, "batches": (U + args.batch - 1) // args.batch}
        log("export_pass_s", rec["export_pass_s"])
    else:
        rec["export_pass_s"] = "not measured"
    if not args.no_host_loop and left() > 150:
        import slas_ref as SR
        host = SR.HostSlas(e, ea, user_x, user_y, item_x, ts_idx=3, k_item=args.k, k_user=args.k)
        t0 = time.perf_counter()
        hs = host.build_subgraph(seeds.cpu().numpy(), None)
        rec["host_loop_s"] = {"one_batch_view_none": time.perf_counter() - t0,
                              "users": int(hs["users_global"].size),
                              "items": int(hs["items_global"].size),
                              "edges": int(hs["e_u2i"].shape[1])}
        log("host_loop_s", rec["host_loop_s"])
    else:
        rec["host_loop_s"] = "not measured"
    rec["wall_s"] = time.perf_counter() - t_start
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
