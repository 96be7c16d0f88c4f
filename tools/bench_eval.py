"""Benchmark: sampled evaluation on MI355X.

    python tools/bench_eval.py [--config C4] [--reps 5] [--cpu-users 40000] [--full]

Workload: the C4 synthetic graph (5M users x 1M items, 50M interactions);
20% of the interactions (seeded) are held out as the test split, the rest is
the train split. Embeddings are random (metric values are irrelevant to the
timing; the protocol is: every user with a test item gets 1 pos + 99 negatives
rejected against its test and train rows, K = 10, 20).

value = evaluated users / wall time of one bbgr.evaluation.evaluate_sampled
        call (inputs resident in HBM; includes the host read-back of the sums).
roofline = eval_sampled_kernel: algorithmic bytes per user = (1 + n_neg + 1)
        rows of d fp32 (the user row and every candidate's item row) / launch
        time, timed with HIP events on the launching stream.
--stream numpy: the candidates of the reference's own numpy stream
        (np.random.default_rng(seed + 999), drawn on the host by
        bbgr_eval_draw_candidates, bit for bit the reference loop's), uploaded
        and scored by the same kernel; the host draw is timed apart
        (host_draw_s) and included in the wall time.
--full: the full-ranking protocol; roofline = fp32 MFMA (2*d flops per
        (user, item) score) over the whole evaluate_full device time.
cpu_baseline = the reference's per-user loop restated in oracle/ref_numpy.py
        (evaluate_sampled_reference_style, numpy RNG + searchsorted rejection +
        per-user scoring and metrics) on a bounded sample of users.
--recommend: recommendation lists (bbgr_recommend) beside the full-ranking
        scorer, raw C-ABI calls alternating in one process, HIP events around
        each: `eval_full` (scorer + merge + metrics), `eval_lists` (the same
        metrics kernels alone; eval_full - eval_lists = its scorer + merge),
        `recommend` at k = --k (one pass) and at k = --k-long (continuation
        passes). With --max-users N the graph is drawn over N users with the
        config's degree law and item set (the tables keep the config's item
        count and --dim or the config's width); the listed users are those
        with test items. d = 256 has no eval_full arm (unsupported there).
        In the same rounds: `recommend_bf16` (bbgr_recommend_bf16 on tables
        converted once; the conversion is timed apart, `to_bf16_ms`) and
        `recommend_bf16_exact`, the stages of precision="bf16_exact" with an
        event between them: item-norm bound, bf16 pass at k_pre, rescoring,
        and the fp32 fallback on the uncertified users (their share is
        reported; its lists are checked against the fp32 arm's).
        --trained-steps N takes the tables from a FusedTrainer run for N steps
        on the train split instead of random ones.
Prints ONE JSON line on stdout.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import ctypes

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bbgr  # noqa: E402,F401
from bbgr.evaluation import evaluate_full, evaluate_sampled  # noqa: E402
from bbgr.graph import Csr  # noqa: E402
from bbgr.synthetic import (CONFIGS, CONFIG_SEED, config_edges, synthetic_credibility,  # noqa: E402
                            synthetic_edges)

HBM_PEAK_GBS = 8000.0
FP32_MFMA_PEAK_TF = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def split(edges, frac, seed):
    rng = np.random.default_rng([seed, 0x7E57])
    test = rng.random(edges.shape[1]) < frac
    return np.ascontiguousarray(edges[:, ~test]), np.ascontiguousarray(edges[:, test])


def bench_recommend(args):
    """The --recommend arms (see the module docstring)."""
    from bbgr import _lib
    from bbgr import evaluation as EV
    from bbgr.recommend import recommend
    cfg = CONFIGS[args.config]
    U, I, d = cfg["num_users"], cfg["num_items"], args.dim or cfg["emb_dim"]
    dev = "cuda"
    if args.max_users and args.max_users < U:
        E = int(cfg["num_edges"] * (args.max_users / U))
        U = args.max_users
        edges = synthetic_edges(U, I, E, CONFIG_SEED[args.config], items=cfg["items"])
    else:
        edges = config_edges(args.config)
    tr, te = split(edges, 0.2, 5)
    del edges
    trc, tec = Csr(tr[0], tr[1], U, I, dev), Csr(te[0], te[1], U, I, dev)
    if args.trained_steps:
        from bbgr.graph import BipartiteGraph
        from bbgr.trainer import FusedTrainer
        trainer = FusedTrainer(BipartiteGraph(tr, U, I, dev), "v2_pop",
                               cred=synthetic_credibility(U, 3), emb_dim=d,
                               num_layers=cfg["num_layers"], batch_size=cfg["batch"])
        for _ in range(args.trained_steps):
            trainer.step()
        uf, itf = (t.detach().clone() for t in trainer.forward())
        del trainer
    else:
        g = torch.Generator(device=dev).manual_seed(7)
        uf = (torch.rand(U, d, device=dev, generator=g) - 0.5)
        itf = (torch.rand(I, d, device=dev, generator=g) - 0.5)
    pop_t = torch.tensor(np.bincount(tr[1], minlength=I).astype(np.float32), device=dev)
    users = EV._eval_users(tec)
    n = users.numel()
    log(f"[recommend] {args.config}: {n} listed users x {I} items, d {d}, "
        f"{'trained ' + str(args.trained_steps) + ' steps' if args.trained_steps else 'random'} "
        f"tables")
    k, kl = args.k, args.k_long
    with_full = d in (64, 128) and k <= 32
    i32 = dict(dtype=torch.int32, device=dev)
    groups = torch.zeros(n, dtype=torch.uint8, device=dev)
    sums = torch.empty(EV.NOUT, dtype=torch.float64, device=dev)
    topk_full = torch.empty(n * k, **i32)
    ea = EV._args(users, trc, tec, uf, itf, I, (k,), pop_t, int(tr.shape[1]), groups, sums)
    ea.topk = topk_full.data_ptr()

    def rec_args(kk, cls=_lib.RecommendArgs, tu=uf, ti=itf, scores=False):
        out = torch.empty(n * kk, **i32)
        a = cls()
        a.n_users, a.users, a.n_user_rows = n, users.data_ptr(), U
        a.uf, a.lduf, a.itf, a.ldif = tu.data_ptr(), d, ti.data_ptr(), d
        a.d, a.n_items, a.k = d, I, kk
        a.ex_indptr, a.ex_indices = trc.indptr.data_ptr(), trc.indices.data_ptr()
        a.topk = out.data_ptr()
        if scores:
            sc = torch.empty(n * kk, dtype=torch.float32, device=dev)
            a.topk_score = sc.data_ptr()
            return a, out, sc
        return a, out

    from bbgr.recommend import _bf16_table, default_prefilter_k
    ufh, ith = _bf16_table(uf), _bf16_table(itf)
    k_pre = args.prefilter_k or default_prefilter_k(args.k)

    arms = {}
    if with_full:
        arms["eval_full"] = ("bbgr_eval_full", ea)
        arms["eval_lists"] = ("bbgr_eval_lists", ea)
    ra, topk_rec = rec_args(k)
    arms["recommend"] = ("bbgr_recommend", ra)
    rl, _long = rec_args(kl)
    arms["recommend_long"] = ("bbgr_recommend", rl)
    rb, topk_bf16 = rec_args(k, _lib.RecommendBf16Args, ufh, ith)
    arms["recommend_bf16"] = ("bbgr_recommend_bf16", rb)
    rp, cand, cand_score = rec_args(k_pre, _lib.RecommendBf16Args, ufh, ith, scores=True)
    arms["bf16_pass_k_pre"] = ("bbgr_recommend_bf16", rp)
    ws = {}
    for name, (fn, a) in arms.items():
        ws[name] = EV._run(fn, a, dev)   # sizes the workspace; first (warm-up) call
    st = _lib.stream_handle()
    s = torch.cuda.current_stream()

    def once(name):
        fn, a = arms[name]
        nb = ctypes.c_size_t(ws[name].numel())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        _lib.call(fn, ctypes.byref(a), ws[name].data_ptr(), ctypes.byref(nb), st)
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # the other stages of precision="bf16_exact" (its bf16 pass is the arm above)
    n_max = torch.empty(1, device=dev)
    topk_ex = torch.empty(n * k, **i32)
    score_ex = torch.empty(n * k, dtype=torch.float32, device=dev)
    cert = torch.empty(n, dtype=torch.uint8, device=dev)
    ra_ = _lib.RecommendRescoreArgs()
    ra_.n_users, ra_.users, ra_.n_user_rows = n, users.data_ptr(), U
    ra_.uf, ra_.lduf, ra_.itf, ra_.ldif = uf.data_ptr(), d, itf.data_ptr(), d
    ra_.d, ra_.n_items, ra_.k, ra_.k_pre = d, I, k, k_pre
    ra_.cand, ra_.cand_score, ra_.n_max = cand.data_ptr(), cand_score.data_ptr(), n_max.data_ptr()
    ra_.topk, ra_.topk_score, ra_.certified = (topk_ex.data_ptr(), score_ex.data_ptr(),
                                              cert.data_ptr())

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        f()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    fb_users = [0]

    def exact_rest():
        """(to_bf16, norm, rescore, fallback) ms; the lists land in topk_ex."""
        t_conv = timed(lambda: (_bf16_table(uf), _bf16_table(itf)))
        t_norm = timed(lambda: _lib.call("bbgr_row_norm_max", I, d, itf.data_ptr(), d,
                                         n_max.data_ptr(), st))
        t_res = timed(lambda: _lib.call("bbgr_recommend_rescore", ctypes.byref(ra_), st))
        n_fb = n - int(cert.sum())
        fb_users[0] = n_fb
        t_fb = 0.0
        if n_fb:
            def fallback():
                rows = torch.argsort(cert, stable=True)[:n_fb]
                topk_ex.view(n, k)[rows] = recommend(uf, itf, users[rows], k, exclude=trc)
            t_fb = timed(fallback)
        return t_conv, t_norm, t_res, t_fb

    for _ in range(args.warmup):
        for name in arms:
            once(name)
        exact_rest()
    ms = {name: [] for name in arms}
    rest = []
    for _ in range(args.reps):   # the arms alternate inside every round
        for name in arms:
            ms[name].append(once(name))
        rest.append(exact_rest())
    stat = {name: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)),
                   "max_ms": float(np.max(v))} for name, v in ms.items()}
    flops = 2.0 * n * I * d
    tf = lambda t_ms: flops / (t_ms * 1e-3) / 1e12   # noqa: E731
    km = 16 if (k + 15) // 16 <= (k + 23) // 24 else 24
    kml = 16 if (kl + 15) // 16 <= (kl + 23) // 24 else 24
    passes, passes_long = -(-k // km), -(-kl // kml)
    rec = stat["recommend"]["median_ms"]
    line = {
        "metric": "recommend_users_per_s", "value": n / (rec * 1e-3), "unit": "users/s",
        "n_gpus": 1, "steps": args.reps, "warmup": args.warmup + 1, "ms_per_step": rec,
        "higher_is_better": True, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{args.config} recommend (all items, train rows excluded)",
                   "users": n, "num_items": I, "emb_dim": d, "k": k, "k_long": kl,
                   "train_edges": int(tr.shape[1])},
        "arms_ms": stat,
        "recommend": {"k": k, "passes": passes, "list_depth": km, "tflops": tf(rec),
                      "frac_fp32_mfma_peak": tf(rec) / FP32_MFMA_PEAK_TF},
        "recommend_long": {"k": kl, "passes": passes_long, "list_depth": kml,
                           "ms": stat["recommend_long"]["median_ms"],
                           "x_single_pass": stat["recommend_long"]["median_ms"] / rec},
        "note": "HIP events around each raw C-ABI call; frac = 2*users*items*d flops of ONE "
                "scoring pass over the call's time, against the fp32 MFMA dense peak",
    }
    if with_full:
        sm = stat["eval_full"]["median_ms"] - stat["eval_lists"]["median_ms"]
        line["eval_full_scorer_merge_ms"] = sm
        line["eval_full_scorer_merge_frac_peak"] = tf(sm) / FP32_MFMA_PEAK_TF
        line["recommend_over_eval_full_scorer_merge"] = rec / sm
        # same lists wherever no train item reaches eval_full's top-k (always, at these sizes)
        line["lists_equal_eval_full"] = bool(torch.equal(topk_full, topk_rec))
    bf = stat["recommend_bf16"]["median_ms"]
    conv, norm, res, fb = (float(np.median(v)) for v in zip(*rest))
    pre = stat["bf16_pass_k_pre"]["median_ms"]
    same = (topk_bf16.view(n, k) == topk_rec.view(n, k)).all(1).float().mean()
    line["recommend_bf16"] = {"k": k, "ms": bf, "to_bf16_ms": conv, "x_faster_than_fp32": rec / bf,
                              "x_faster_with_conversion": rec / (bf + conv),
                              "rows_equal_fp32": float(same)}
    line["recommend_bf16_exact"] = {
        "k": k, "k_pre": k_pre, "ms": conv + norm + pre + res + fb,
        "x_faster_than_fp32": rec / (conv + norm + pre + res + fb),
        "split_ms": {"to_bf16": conv, "item_norm_max": norm, "bf16_pass": pre, "rescore": res,
                     "fallback_fp32": fb},
        "certified_share": 1.0 - fb_users[0] / n, "fallback_users": fb_users[0],
        "lists_equal_fp32": bool(torch.equal(topk_ex, topk_rec))}
    line["tables"] = f"trained {args.trained_steps} steps" if args.trained_steps else "random"
    chk = recommend(uf, itf, users[:4096], kl, exclude=trc)
    line["long_prefix_equals_short"] = bool(torch.equal(chk[:, :k],
                                                        topk_rec.view(n, k)[:4096]))
    log(json.dumps(line, indent=1))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--negatives", type=int, default=99)
    ap.add_argument("--cpu-users", type=int, default=40000)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--ks", type=int, nargs="+", default=[10, 20],
                    help="--full: the cutoffs (the top-K list is max(ks) deep)")
    ap.add_argument("--full", action="store_true",
                    help="full-ranking protocol (evaluate_full_ranking) instead of sampled")
    ap.add_argument("--stream", default="philox", choices=["philox", "numpy"],
                    help="sampled: device Philox candidates, or the reference's numpy stream")
    ap.add_argument("--max-users", type=int, default=0,
                    help="evaluate only the first N users with test items (0 = all)")
    ap.add_argument("--recommend", action="store_true",
                    help="recommendation lists beside the full-ranking scorer (see above)")
    ap.add_argument("--dim", type=int, default=0, help="--recommend: table width (0 = config's)")
    ap.add_argument("--k", type=int, default=10, help="--recommend: the single-pass list length")
    ap.add_argument("--k-long", type=int, default=100,
                    help="--recommend: a list length that needs continuation passes")
    ap.add_argument("--prefilter-k", type=int, default=0,
                    help="--recommend: candidates of the bf16_exact arm (0 = the default rule)")
    ap.add_argument("--trained-steps", type=int, default=0,
                    help="--recommend: tables from a FusedTrainer run for N steps on the train "
                         "split instead of random ones")
    args = ap.parse_args()
    if args.recommend:
        return bench_recommend(args)
    cfg = CONFIGS[args.config]
    U, I, d = cfg["num_users"], cfg["num_items"], cfg["emb_dim"]
    dev = "cuda"
    t0 = time.perf_counter()
    edges = config_edges(args.config)
    tr, te = split(edges, 0.2, 5)
    del edges
    log(f"[eval] {args.config}: train {tr.shape[1]} test {te.shape[1]} ({time.perf_counter()-t0:.1f}s)")
    trc = Csr(tr[0], tr[1], U, I, dev)
    tec = Csr(te[0], te[1], U, I, dev)
    g = torch.Generator(device=dev).manual_seed(7)
    uf = (torch.rand(U, d, device=dev, generator=g) - 0.5)
    itf = (torch.rand(I, d, device=dev, generator=g) - 0.5)
    pop = np.bincount(tr[1], minlength=I).astype(np.float32)
    pop_t = torch.tensor(pop, device=dev)
    cred = synthetic_credibility(U, 3)
    cred_t = torch.tensor(cred, device=dev, dtype=torch.float32)
    T = int(tr.shape[1])
    if args.max_users:   # restrict the test split to the first N users that have test items
        keep_u = np.unique(te[0])[: args.max_users]
        te = te[:, np.isin(te[0], keep_u)]
        tec = Csr(te[0], te[1], U, I, dev)
    if args.full:
        run = lambda c: evaluate_full(uf, itf, trc, tec, I, pop_t, T, cred_t,  # noqa: E731
                                      Ks=tuple(args.ks))
    elif args.stream == "numpy":
        from bbgr import evaluation as EV
        from bbgr.host_sampler import edges_to_user_csr
        tr_csr, te_csr = edges_to_user_csr(tr, U), edges_to_user_csr(te, U)
        host_users = np.where(np.diff(te_csr[0]) > 0)[0].astype(np.int64)
        users_t = torch.from_numpy(host_users).to(dev)
        groups_t = torch.from_numpy(EV.cred_group_flags(host_users, cred, 0.2)).to(dev)
        draw_s = []

        def run(c):
            t = time.perf_counter()
            cand = EV.draw_candidates(np.random.default_rng(42 + 999), host_users, tr_csr,
                                      te_csr, I, args.negatives)
            draw_s.append(time.perf_counter() - t)
            return evaluate_sampled(uf, itf, trc, tec, I, pop_t, T, cred_t,
                                    sampled_negatives=args.negatives,
                                    cand=torch.from_numpy(cand).pin_memory(), users=users_t,
                                    groups=groups_t)
    else:
        run = lambda c: evaluate_sampled(uf, itf, trc, tec, I, pop_t, T, cred_t,  # noqa: E731
                                         sampled_negatives=args.negatives, counter=c)
    for w in range(args.warmup):
        run(w)
    torch.cuda.synchronize()
    # kernel time: HIP events on the launching stream around the whole call
    s = torch.cuda.current_stream()
    evs = []
    walls = []
    res = None
    for r in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        a.record(s)
        res = run(100 + r)
        b.record(s)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t1)
        evs.append(a.elapsed_time(b) / 1e3)
    k0 = args.ks[0] if args.full else 10
    n_eval = int(res[k0]["users_eval"])
    wall = float(np.median(walls))
    dev_s = float(np.median(evs))
    nc = 1 + args.negatives
    if args.full:   # MFMA-bound: 2*d flops per (user, item) score
        alg = 2.0 * n_eval * I * d
        roof = {"bound": "mfma", "achieved": alg / dev_s / 1e12, "peak": FP32_MFMA_PEAK_TF,
                "unit": "TFLOP/s", "frac": alg / dev_s / 1e12 / FP32_MFMA_PEAK_TF,
                "traffic": None, "note": "whole evaluate_full device time (score+top-K, merge, "
                                         "metrics); fp32 MFMA dense peak"}
    else:
        alg = n_eval * (nc + 1) * d * 4
        roof = {"bound": "hbm", "achieved": alg / dev_s / 1e9, "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": alg / dev_s / 1e9 / HBM_PEAK_GBS, "traffic": None,
                "note": "whole evaluate_sampled device time (sample+score+rank, metrics)"}
    log(f"[eval] users {n_eval}  wall {wall*1e3:.2f} ms  device {dev_s*1e3:.2f} ms  "
        f"ndcg@{k0} {res[k0]['ndcg']:.4f}")
    cpu = None
    if not args.no_cpu_baseline:
        from oracle import ref_numpy as R
        trp, tri = R.edges_to_user_csr(tr, U)
        tep, tei = R.edges_to_user_csr(te, U)
        n_cpu = max(1, args.cpu_users // 400) if args.full else args.cpu_users
        users = np.where(np.diff(tep) > 0)[0][:n_cpu]
        ufn, itn = uf.cpu().numpy(), itf.cpu().numpy()
        t1 = time.perf_counter()
        if args.full:
            ranked = R.full_ranking_reference_style(users, trp, tri, ufn, itn, 20)
            hi, lo = R.make_cred_groups(users, cred, 0.2)
            R.evaluate_given_topk(users, ranked, tep, tei, pop, T, I, cred, hi, lo)
        else:
            R.evaluate_sampled_reference_style(trp, tri, tep, tei, ufn, itn, I, pop, T, cred,
                                               n_neg=args.negatives, users=users)
        el = time.perf_counter() - t1
        cpu = {"value": users.size / el, "unit": "users/s", "cores": 1, "kind": "port",
               "sample": f"reference per-user loop (oracle restatement) on the first "
                         f"{users.size} evaluated users of the same split: {el:.1f} s"}
        log(f"[eval] cpu {users.size} users {el:.1f}s -> {users.size/el:.0f} users/s")
    kstr = ",".join(str(k) for k in args.ks)
    proto = f"full ranking (all items, K={kstr})" if args.full else \
        f"sampled eval (1 pos + {args.negatives} neg, K=10,20; {args.stream} candidates)"
    line = {
        "metric": "eval_users_per_s", "value": n_eval / wall, "unit": "users/s",
        "n_gpus": 1, "steps": args.reps, "warmup": args.warmup, "ms_per_step": wall * 1e3,
        "higher_is_better": True, "scaling": "none", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"{args.config} {proto}",
                   "users_eval": n_eval, "num_items": I, "emb_dim": d,
                   "train_edges": T, "test_edges": int(te.shape[1])},
        "device_ms": dev_s * 1e3,
        "host_draw_s": (float(np.median(draw_s)) if not args.full and args.stream == "numpy"
                        else None),
        "candidate_stream": None if args.full else args.stream,
        "roofline": roof,
        "cpu_baseline": cpu,
    }
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
