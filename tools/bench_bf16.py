"""Benchmark: the opt-in bf16 forward beside the fp32 step, in one process.

    python tools/bench_bf16.py [--config C4] [--steps 20] [--legs 3] [--out FILE]
    python tools/bench_bf16.py --quality [--config C2] [--epochs 60] [--seeds 1 2 3] [--out FILE]

Step time (default): one graph, two FusedTrainers that differ only in
forward_dtype. After a warm-up the two run alternately, `--legs` legs of
`--steps` timed steps each (wall clock around a device sync), so drift of the
box shows in both. Then each runs `--steps` more steps under a SpmmTimer for
the per-product times (forward launches: the full-CSR products and the masked
last layer; the backward is the same code in both modes and is listed for
comparison), and the conversion pass (bbgr_to_bf16 of the user table into its
shadow) is timed alone. The byte model printed beside the times is the one
DESIGN uses for the gathers: every edge reads one source row (d * 4 or d * 2
bytes) plus its 4-byte index; every row writes its layer table row once.

Quality (--quality): a 90/10 edge split of the config's graph, both modes
trained for the same epochs at each seed (the seed sets the initial tables and
the sampler stream; the split is fixed), evaluate_sampled with device-drawn
(Philox) candidates: Recall@20 / NDCG@20 per mode and seed, and whether the
bf16 mean lies below the fp32 mean by more than the fp32 runs' own spread.

Prints ONE JSON line on stdout (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bbgr  # noqa: E402,F401
from bbgr import propagate as P  # noqa: E402
from bbgr.evaluation import evaluate_sampled  # noqa: E402
from bbgr.graph import BipartiteGraph, Csr  # noqa: E402
from bbgr.synthetic import CONFIGS, CONFIG_SEED, config_edges, synthetic_credibility  # noqa: E402
from bbgr.trainer import FusedTrainer  # noqa: E402

MODES = ("fp32", "bf16")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def timed_steps(tr, n: int) -> float:
    """ms per step over n steps (wall clock, device idle before and after)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        tr.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def product_times(tr, n: int, n_items: int) -> list:
    """Average ms per launch of every SpMM launch group over n steps."""
    timer = P.SpmmTimer()
    P.set_spmm_timer(timer)
    try:
        for _ in range(n):
            tr.step()
        torch.cuda.synchronize()
    finally:
        P.set_spmm_timer(None)
    out = []
    for (kind, sig, rows, cols, d), (launches, ms, _, nnz) in sorted(timer.groups().items()):
        out.append({"kind": kind, "masks": sig, "d": d,
                    "side": "item<-user" if rows == n_items else "user<-item",
                    "launches_per_step": launches / n, "avg_ms": ms / launches})
    return out


def conversion_ms(tr, reps: int = 20) -> float:
    """bbgr_to_bf16 of the user weight table into a shadow of its own, alone."""
    dst = torch.empty(tr.U, tr.d, dtype=torch.bfloat16, device=tr.device)
    P.to_bf16(tr.user_w, dst)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        P.to_bf16(tr.user_w, dst)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def byte_model(U: int, I: int, E: int, d: int) -> dict:
    """Bytes per launch of the forward products under the gather model."""
    m = {}
    for name, eb in (("fp32", 4), ("bf16", 2)):
        m[name] = {
            "item<-user gather": E * (d * eb + 4),
            "user<-item gather": E * (d * eb + 4),
            "user layer table write": U * d * eb,
            "item layer table write": I * d * eb,
        }
    m["conversion pass (read fp32 + write bf16 user table)"] = U * d * 6
    return m


def step_bench(args) -> dict:
    cfg = CONFIGS[args.config]
    U, I, d, K, B = (cfg["num_users"], cfg["num_items"], cfg["emb_dim"], cfg["num_layers"],
                     cfg["batch"])
    edges = config_edges(args.config)
    cred = synthetic_credibility(U, CONFIG_SEED[args.config])
    t0 = time.perf_counter()
    graph = BipartiteGraph(edges, U, I, "cuda", vertex_order="degree")
    tr = {m: FusedTrainer(graph, "v2_pop", cred=cred, emb_dim=d, num_layers=K, batch_size=B,
                          forward_dtype=m) for m in MODES}
    torch.cuda.synchronize()
    log(f"[bf16] {args.config}: graph + two trainers in {time.perf_counter() - t0:.1f}s")
    for m in MODES:
        timed_steps(tr[m], args.warmup)
    legs = {m: [] for m in MODES}
    for leg in range(args.legs):
        for m in MODES:
            legs[m].append(timed_steps(tr[m], args.steps))
        log(f"[bf16] leg {leg}: " + ", ".join(f"{m} {legs[m][-1]:.3f} ms" for m in MODES))
    prods = {m: product_times(tr[m], args.steps, I) for m in MODES}
    conv = conversion_ms(tr["bf16"])
    log(f"[bf16] conversion pass {conv:.3f} ms")
    med = {m: float(np.median(legs[m])) for m in MODES}
    return {
        "metric": "bf16_forward_step_ms", "config": args.config, "d": d, "num_layers": K,
        "batch": B, "num_users": U, "num_items": I, "num_edges": int(edges.shape[1]),
        "steps_per_leg": args.steps, "warmup": args.warmup,
        "ms_per_step": {m: {"legs": legs[m], "median": med[m]} for m in MODES},
        "bf16_over_fp32": med["bf16"] / med["fp32"],
        "products": prods, "conversion_ms": conv,
        "byte_model": byte_model(U, I, int(edges.shape[1]), d),
        "losses": {m: float(tr[m].loss) for m in MODES},
    }


def quality(args) -> dict:
    cfg = CONFIGS[args.config]
    U, I, d, K, B = (cfg["num_users"], cfg["num_items"], cfg["emb_dim"], cfg["num_layers"],
                     cfg["batch"])
    edges = config_edges(args.config)
    E = edges.shape[1]
    rng = np.random.default_rng(CONFIG_SEED[args.config] + 90)
    held = np.zeros(E, bool)
    held[rng.choice(E, E // 10, replace=False)] = True
    train, test = edges[:, ~held], edges[:, held]
    cred = synthetic_credibility(U, CONFIG_SEED[args.config])
    graph = BipartiteGraph(train, U, I, "cuda", vertex_order="degree")
    test_csr = Csr(test[0], test[1], U, I, "cuda")
    pop = np.bincount(train[1], minlength=I).astype(np.float32)
    steps = args.epochs * ((U + B - 1) // B)
    runs = {m: [] for m in MODES}
    for seed in args.seeds:
        for m in MODES:
            tr = FusedTrainer(graph, "v2_pop", cred=cred, emb_dim=d, num_layers=K, batch_size=B,
                              lr=args.lr, seed=seed, forward_dtype=m)
            for _ in range(steps):
                tr.step()
            uf, itf = tr.forward()
            res = evaluate_sampled(uf, itf, tr._train_rows(), test_csr, I, pop, train.shape[1],
                                   cred, Ks=(20,))[20]
            runs[m].append({"seed": seed, "recall@20": res["recall"], "ndcg@20": res["ndcg"],
                            "loss": float(tr.loss), "users_eval": res["users_eval"]})
            log(f"[bf16] quality seed {seed} {m}: recall@20 {res['recall']:.4f} "
                f"ndcg@20 {res['ndcg']:.4f} loss {float(tr.loss):.4f}")
    out = {"metric": "bf16_forward_quality", "config": args.config, "epochs": args.epochs,
           "steps": steps, "lr": args.lr, "split": "90/10 edges, fixed", "runs": runs,
           "protocol": "evaluate_sampled, 1 positive + 99 negatives, device-drawn candidates"}
    for key in ("recall@20", "ndcg@20"):
        v = {m: np.array([r[key] for r in runs[m]]) for m in MODES}
        spread = float(v["fp32"].max() - v["fp32"].min())
        out[key] = {"fp32_mean": float(v["fp32"].mean()), "bf16_mean": float(v["bf16"].mean()),
                    "fp32_seed_spread": spread,
                    "bf16_below_fp32_by_more_than_spread":
                        bool(v["fp32"].mean() - v["bf16"].mean() > spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.config is None:
        args.config = "C2" if args.quality else "C4"
    line = quality(args) if args.quality else step_bench(args)
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
