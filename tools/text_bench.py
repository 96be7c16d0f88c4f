"""Benchmark: review text -> token and distinct-token counts on MI355X.

    python tools/text_bench.py [--records 1000000] [--reps 10] [--host-records N]
                               [--jsonl-lines 200000] [--out profiles/text/text_c2.json]
    python tools/text_bench.py --pooled [--chunk-bytes N [N ..]]

Workload: a seeded synthetic corpus of --records reviews (C2's record count by
default): Zipf (1 / rank) draws from a vocabulary of 50,000 lower-case words
of 2..11 letters, a Poisson number of tokens a record (mean 60), mixed case
(lower, Capitalised, UPPER), separators of spaces, punctuation and apostrophes,
about 2 % of them non-ASCII (accented letters, U+2019, U+0130, an emoji), and
U+212A in about one record of 10,000 (the records the host counts again).

Each launch group is timed alone with device events (median of --reps after
--warmup) on device-resident text:

  count   bbgr_text_count: the coalesced walk, n_tokens and the token total
  emit    the scan of n_tokens, the tokens' starts and records, their hashes
  sort    hipcub's segmented radix sort by hash inside each record
  verify  distinct counts, the byte comparison of equal hashes, the recheck total

`count` is set against the text bytes it has to read and the 8 TB/s of HBM.
`call_ms` is one whole bbgr.text.token_counts from host memory (host clock: the
host -> device copy, both host reads, the host recount of flagged records);
`upload_ms` the copy alone (median of three after the first, `upload_first_ms`). The baseline is the parent's path: the
bbgr.features.tokenize loop (findall, list, set) over the first --host-records
records' strings on this machine's CPU (all of them by default); the device
counts are compared with it record by record (`vs_host`). `jsonl` times
bbgr.features.review_columns_from_jsonl in both modes on a dump of the first
--jsonl-lines records. Prints ONE JSON line; writes --out.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bbgr  # noqa: E402,F401
from bbgr import _lib  # noqa: E402
from bbgr import features as FT  # noqa: E402
from bbgr import text as TX  # noqa: E402

HBM_PEAK = 8.0e12
VOCAB, MEAN_TOKENS, BLOCK = 50_000, 60, 50_000
# separator, weight: mostly spaces, some punctuation and apostrophes, a few non-ASCII
SEPS = [(" ", 70), (", ", 6), (". ", 6), ("! ", 1), ("? ", 1), (" - ", 1), ("\n", 1), (" (", 1),
        (") ", 1), ("'", 2), ("'s ", 2), ("' ", 1), (" '", 1), ("\u2019s ", 1.5), (" \u00e9 ", 1.5),
        ("\u00fc", 1), (" \u0130", 1), (" \U0001F600 ", 1)]
KELVIN_SEP = " \u212a "


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def _table(words: list) -> tuple:
    """(bytes [n, width] zero padded, lengths [n]) of a list of byte strings."""
    width = max(len(w) for w in words)
    tab = np.zeros((len(words), width), np.uint8)
    for k, w in enumerate(words):
        tab[k, :len(w)] = np.frombuffer(w, np.uint8)
    return tab, np.array([len(w) for w in words], np.int64)


def synthetic_corpus(n_records: int, seed: int = 0) -> TX.ReviewText:
    rng = np.random.default_rng(seed)
    lengths = rng.integers(2, 12, VOCAB)
    letters = rng.integers(97, 123, (VOCAB, 11), dtype=np.uint8)
    vocab = np.where(np.arange(11)[None, :] < lengths[:, None], letters, 0).astype(np.uint8)
    p = 1.0 / np.arange(1, VOCAB + 1)
    cdf = np.cumsum(p / p.sum())
    seps, sep_len = _table([s.encode("utf-8") for s, _ in SEPS] + [KELVIN_SEP.encode("utf-8")])
    sep_p = np.array([w for _, w in SEPS], float)
    sep_p /= sep_p.sum()
    parts, offsets = [], [np.zeros(1, np.int64)]
    end = 0
    for r0 in range(0, n_records, BLOCK):
        nr = min(BLOCK, n_records - r0)
        per = rng.poisson(MEAN_TOKENS, nr)
        T = int(per.sum())
        w = np.minimum(np.searchsorted(cdf, rng.random(T)), VOCAB - 1)
        case = rng.choice(3, T, p=[0.8, 0.15, 0.05])          # lower, Capitalised, UPPER
        sep = rng.choice(len(SEPS), T, p=sep_p)
        sep[rng.random(T) < 1.0 / (10_000 * MEAN_TOKENS)] = len(SEPS)
        wl, sl = lengths[w], sep_len[sep]
        tl = wl + sl
        starts = np.cumsum(tl) - tl
        total = int(tl.sum())
        tok = np.repeat(np.arange(T), tl)
        j = np.arange(total) - starts[tok]
        in_word = j < wl[tok]
        ch = np.where(in_word, vocab[w[tok], np.minimum(j, 10)],
                      seps[sep[tok], np.clip(j - wl[tok], 0, seps.shape[1] - 1)])
        upper = in_word & ((case[tok] == 2) | ((case[tok] == 1) & (j == 0)))
        parts.append(np.where(upper, ch - 32, ch).astype(np.uint8))
        rec_end = np.cumsum(per)                               # tokens before each record's end
        tok_end = np.concatenate([[0], np.cumsum(tl)])
        offsets.append(end + tok_end[rec_end])
        end += total
    return TX.ReviewText(np.concatenate(parts), np.concatenate(offsets).astype(np.int64))


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


def strings_of(text: TX.ReviewText, n: int) -> list:
    raw, off = text.data.tobytes(), text.offsets
    return [raw[off[r]:off[r + 1]].decode("utf-8", "surrogatepass") for r in range(n)]


def host_loop(strings: list) -> tuple:
    """The parent's per-review steps: findall, list, set."""
    n_tok, n_uniq = [], []
    for s in strings:
        toks = FT.tokenize(s)
        n_tok.append(len(toks))
        n_uniq.append(len(set(toks)))
    return np.asarray(n_tok, np.int32), np.asarray(n_uniq, np.int32)


def write_jsonl(path: str, strings: list, seed: int = 1) -> None:
    rng = np.random.default_rng(seed)
    n = len(strings)
    users, items = rng.integers(0, max(n // 10, 1), n), rng.integers(0, max(n // 20, 1), n)
    ratings, votes = rng.integers(1, 6, n), rng.integers(0, 5, n)
    ts = 1_500_000_000_000 + rng.integers(0, 10**11, n)
    with open(path, "w", encoding="utf-8") as f:
        for k, s in enumerate(strings):
            f.write(json.dumps({
                "rating": float(ratings[k]), "title": s[:40], "text": s[40:],
                "user_id": f"AE{int(users[k]):026d}", "parent_asin": f"B{int(items[k]):09d}",
                "timestamp": int(ts[k]), "helpful_vote": int(votes[k]),
                "verified_purchase": bool(k & 1)}) + "\n")


def pooled_main(args):
    """--pooled: the launch groups of bbgr_text_unique_pooled on the same
    corpus, its records assigned to the users of tools/features_bench.py's C2
    columns (the same seeded draw); the whole pooled_token_counts from host
    memory; and the host loop it replaces, a set per user over
    features.tokenize (on --host-records records, scaled to all)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from features_bench import synthetic_columns
    from bbgr.synthetic import CONFIGS
    out_path = args.out or os.path.join(ROOT, "profiles", "features_v2", "text_pooled_c2.json")
    U = CONFIGS["C2"]["num_users"]
    user = np.ascontiguousarray(synthetic_columns("C2").user[:args.records])
    text = synthetic_corpus(len(user))
    n, nbytes = len(text), int(text.data.shape[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    rec = {"records": n, "users": U, "text_bytes": nbytes,
           "max_user_records": int(np.bincount(user, minlength=U).max()),
           "device": torch.cuda.get_device_name(0)}
    data, off = torch.from_numpy(text.data).to(dev), torch.from_numpy(text.offsets).to(dev)
    grp = torch.from_numpy(user).to(dev)
    n_tok = torch.zeros(n, dtype=torch.int32, device=dev)
    n_uniq = torch.zeros(n, dtype=torch.int32, device=dev)
    recheck = torch.zeros(n, dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    g_tok = torch.zeros(U, dtype=torch.int64, device=dev)
    g_uniq = torch.zeros(U, dtype=torch.int32, device=dev)
    g_flag = torch.zeros(U, dtype=torch.uint8, device=dev)
    a = TX._text_args(data, off, 0, nbytes, 0, n_tok, n_uniq, recheck, totals)
    st = _lib.stream_handle()
    _lib.call("bbgr_text_count", ctypes.byref(a), st)
    tokens = int(totals[0])
    head = (ctypes.byref(a), tokens, _lib.ptr(grp), U, _lib.ptr(g_tok), _lib.ptr(g_uniq),
            _lib.ptr(g_flag))
    # one whole call sizes the workspace the launch groups below run on
    keep = _lib.Workspace(grow=False)
    _lib.call_with_workspace("bbgr_text_unique_pooled", *head, after=(st,), device=dev, keep=keep)
    rec.update(device_tokens=tokens, workspace_bytes=keep.buf.numel())

    def stage(bits):
        return lambda: _lib.call_with_workspace("bbgr_text_unique_pooled_stages", *head, bits,
                                                after=(st,), keep=keep)

    kernels = {name: timed_events(stage(bits), args.warmup, args.reps)
               for name, bits in (("emit", 1), ("sort", 2), ("verify", 4))}
    for name, r in kernels.items():
        r["ns_per_token"] = r["median_ms"] * 1e6 / max(tokens, 1)
        log(name, r)
    rec["kernels"] = kernels
    rec["kernels_sum_ms"] = sum(r["median_ms"] for r in kernels.values())
    rec["flagged_groups"] = int(totals[1])
    del keep
    ts = []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_tok, d_uniq, info = TX.pooled_token_counts(text, user, U, dev)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    rec["call_ms"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                      "reps": args.reps}
    rec["info"] = info
    log("call_ms", rec["call_ms"], info)
    m = n if args.host_records is None else min(args.host_records, n)
    strings = strings_of(text, m)
    t0 = time.perf_counter()
    sets, total = {}, np.zeros(U, np.int64)
    for u, s in zip(user[:m].tolist(), strings):
        toks = FT.tokenize(s)
        total[u] += len(toks)
        sets.setdefault(u, set()).update(toks)
    host_s = time.perf_counter() - t0
    rec["host_loop"] = {"records": m, "seconds": host_s, "us_per_record": host_s * 1e6 / max(m, 1)}
    if m == n:
        uniq = np.zeros(U, np.int32)
        for u, v in sets.items():
            uniq[u] = len(v)
        rec["vs_host"] = {"tokens": bool(np.array_equal(d_tok.cpu().numpy(), total)),
                          "unique": bool(np.array_equal(d_uniq.cpu().numpy(), uniq))}
    rec["call_vs_host_loop"] = host_s * (n / max(m, 1)) * 1e3 / rec["call_ms"]["median_ms"]
    log("host_loop", rec["host_loop"], rec.get("vs_host"))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def _alternate(arms: dict, warmup: int, reps: int, clock: str) -> dict:
    """The arms in turn, round after round in one process (a drift of the
    clocks hits all alike): per arm the median, min and max of `reps` rounds
    after `warmup`. clock "events": device events around the call; "host": the
    host clock between two synchronisations (calls that read back)."""
    ts = {name: [] for name in arms}
    for k in range(warmup + reps):
        for name, fn in arms.items():
            if clock == "events":
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                t = a.elapsed_time(b)
            else:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e3
            if k >= warmup:
                ts[name].append(t)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                   "reps": reps} for name, v in ts.items()}


def chunked_main(args):
    """--pooled --chunk-bytes N [N ..]: what the regrouped pooled count costs,
    on the --pooled corpus resident on the device. (1) bbgr_text_gather alone
    over all records in user order beside a device copy_ of as many bytes
    (which reads and writes every byte once), alternating, with lists that
    take the search or the misalignment of the source words away (below; the
    events of a gather arm span the host's ctypes call too, `host_call_us`).
    (2) The whole
    pooled_token_counts: the one-chunk call beside chunk_bytes = each N,
    alternating; an N of at least the text is one range, so its excess over
    the one-chunk call is the regrouping itself (the CSR build, the gather,
    the local ids), and the smaller N add the per-range host reads."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from features_bench import synthetic_columns
    from bbgr.synthetic import CONFIGS
    out_path = args.out or os.path.join(ROOT, "profiles", "features_v2",
                                        "text_pooled_chunked_c2.json")
    U = CONFIGS["C2"]["num_users"]
    user = np.ascontiguousarray(synthetic_columns("C2").user[:args.records])
    host_text = synthetic_corpus(len(user))
    n, nbytes = len(host_text), int(host_text.data.shape[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    text = TX.resident(host_text, dev)
    grp = torch.from_numpy(user).to(dev)
    off = torch.from_numpy(host_text.offsets).to(dev)
    rec = {"records": n, "users": U, "text_bytes": nbytes, 
           "source_fetch": "unaligned 16-byte load; arms *_aligned_pair: two aligned loads + shift",
           "device": torch.cuda.get_device_name(0), "hbm_peak_TBps": HBM_PEAK / 1e12}

    # (1) the gather alone, all records in user order
    indptr, eid = FT._group(grp, torch.zeros(n, dtype=torch.int32, device=dev), U)
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    other = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    p_total = torch.empty(1, dtype=torch.int64, device=dev)
    ga = _lib.TextGatherArgs()
    ga.n_list, ga.records, ga.n = n, _lib.ptr(eid), n
    ga.data, ga.offsets, ga.first, ga.last = _lib.ptr(text.data), _lib.ptr(off), 0, nbytes
    ga.out_offsets, ga.out_data, ga.capacity = _lib.ptr(p_off), _lib.ptr(packed), nbytes
    ga.total = _lib.ptr(p_total)
    keep = _lib.Workspace(grow=False)
    st = _lib.stream_handle()
    ga_null = _lib.TextGatherArgs.from_buffer_copy(ga)
    ga_null.out_data = None
    # Lists that take parts of the work away. The records in file order: the source is read
    # front to back. Records of 496 bytes each over the same bytes, in order (REC bytes, the
    # corpus's mean, a multiple of 16): the search stays, and every source word is 16-byte
    # aligned when the text starts at 0, off by one byte everywhere when it starts at 1. The
    # whole text as ONE record: no search (one pair of offsets for all lanes), again aligned
    # from 0 and off by one from 1. The four make search x alignment.
    REC = 496
    file_order = torch.arange(n, dtype=torch.int32, device=dev)
    ga_file = _lib.TextGatherArgs.from_buffer_copy(ga)
    ga_file.records = _lib.ptr(file_order)
    n_fix = (nbytes - 1) // REC
    fix_order = torch.arange(n_fix, dtype=torch.int32, device=dev)
    assert text.data.data_ptr() % 16 == 0 and packed.data_ptr() % 16 == 0
    variants, held = {}, []
    for name, start, m in (("one_record", 0, 1), ("one_record_off_by_1", 1, 1),
                           ("fixed_496", 0, n_fix), ("fixed_496_off_by_1", 1, n_fix)):
        o = (start + REC * torch.arange(m + 1, dtype=torch.int64, device=dev) if m > 1 else
             torch.tensor([start, nbytes], dtype=torch.int64, device=dev))
        v = _lib.TextGatherArgs.from_buffer_copy(ga)
        v.n_list, v.n, v.offsets, v.records = m, m, _lib.ptr(o), _lib.ptr(fix_order)
        v.first, v.last = start, int(o[-1])
        held.append(o)
        variants[name] = (v, _lib.Workspace(grow=False), int(o[-1]) - start)

    def gather_arm(a, ws, fetch=None):
        if fetch is None:
            return lambda: _lib.call_with_workspace("bbgr_text_gather", ctypes.byref(a),
                                                    after=(st,), device=dev, keep=ws)
        return lambda: _lib.call_with_workspace("bbgr_text_gather_fetch", ctypes.byref(a),
                                                _lib.TEXT_FETCH[fetch], after=(st,), device=dev,
                                                keep=ws)

    arms = {"copy": lambda: other.copy_(text.data),
            "gather_offsets_only": gather_arm(ga_null, keep),
            "gather_file_order": gather_arm(ga_file, keep)}
    for name, (v, ws, _) in variants.items():
        arms["gather_" + name] = gather_arm(v, ws)
        arms["gather_" + name + "_aligned_pair"] = gather_arm(v, ws, "aligned_pair")
    # the other source fetch (two aligned loads and a byte shift) on the real lists
    arms["gather_file_order_aligned_pair"] = gather_arm(ga_file, keep, "aligned_pair")
    arms["gather_aligned_pair"] = gather_arm(ga, keep, "aligned_pair")
    arms["gather"] = gather_arm(ga, keep)   # last in a round: the buffers checked below are its
    g = _alternate(arms, args.warmup, args.reps, "events")
    assert int(p_total) == nbytes
    order = eid[:n].long()
    starts = off[:-1][order]
    k = int(torch.randint(0, n, (1,)))                      # one record checked byte for byte
    a0, b0 = int(p_off[k]), int(p_off[k + 1])
    assert torch.equal(packed[a0:b0], text.data[int(starts[k]):int(starts[k]) + b0 - a0])
    # the variants copy what they should: the text from its start on
    for name, (v, ws, moved) in variants.items():
        gather_arm(v, ws)()
        assert int(p_total) == moved
        assert torch.equal(packed[:moved], text.data[v.first:v.first + moved])
    moved = {}
    for name, (v, ws, m) in variants.items():
        moved["gather_" + name] = moved["gather_" + name + "_aligned_pair"] = m
        gather_arm(v, ws, "aligned_pair")()
        assert torch.equal(packed[:m], text.data[v.first:v.first + m])
    g_pair = torch.empty_like(packed)
    gather_arm(ga, keep)()
    g_pair.copy_(packed)
    gather_arm(ga, keep, "aligned_pair")()
    assert torch.equal(g_pair, packed)                       # both fetches: the same bytes
    del g_pair
    for name, r in g.items():
        if name != "gather_offsets_only":                   # that arm moves no text
            r["bytes"] = moved.get(name, nbytes)
            r["TBps_read_plus_write"] = 2 * r["bytes"] / (r["median_ms"] * 1e-3) / 1e12
        log(name, r)
    # Between the two events of a gather arm lies the host's ctypes call as well (no size
    # query: the workspace is kept); the copy arm has none. Its length, from a call that
    # returns before any launch (n_list = 0), by the host clock:
    ga_none = _lib.TextGatherArgs.from_buffer_copy(ga)
    ga_none.n_list = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        gather_arm(ga_none, keep)()
    g["host_call_us"] = (time.perf_counter() - t0) * 1e6 / 200
    g["gather"]["kernel_ms"] = g["gather"]["median_ms"] - g["gather_offsets_only"]["median_ms"]
    g["gather_over_copy"] = g["gather"]["median_ms"] / g["copy"]["median_ms"]
    g["aligned_pair_over_copy"] = g["gather_aligned_pair"]["median_ms"] / g["copy"]["median_ms"]
    rec["gather"] = g
    del packed, other, keep

    # (2) the whole call, one chunk beside the regrouped ones
    calls, infos = {}, {}

    def arm(name, **kw):
        def run():
            infos[name] = TX.pooled_token_counts(text, grp, U, dev, **kw)
        return run

    calls["one_chunk"] = arm("one_chunk")
    for c in args.chunk_bytes:
        calls[f"chunk_bytes={c}"] = arm(f"chunk_bytes={c}", chunk_bytes=c)
    rec["calls"] = _alternate(calls, args.warmup, args.reps, "host")
    base = infos["one_chunk"]
    for name, r in rec["calls"].items():
        tok, uniq, info = infos[name]
        r["info"] = info
        r["equals_one_chunk"] = bool(torch.equal(tok, base[0]) and torch.equal(uniq, base[1]))
        r["over_one_chunk"] = r["median_ms"] / rec["calls"]["one_chunk"]["median_ms"]
        log(name, r)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-records", type=int, default=None,
                    help="records of the host baseline (default: all)")
    ap.add_argument("--jsonl-lines", type=int, default=200_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pooled", action="store_true",
                    help="time bbgr.text.pooled_token_counts (distinct tokens per user) instead")
    ap.add_argument("--chunk-bytes", type=int, nargs="+", default=None,
                    help="with --pooled: time the regrouped count at these chunk sizes and "
                         "bbgr_text_gather alone (profiles/features_v2/text_pooled_chunked_c2.json)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("text_bench needs a GPU: no timing is taken without one")
    if args.chunk_bytes and not args.pooled:
        raise SystemExit("--chunk-bytes goes with --pooled")
    if args.pooled:
        return chunked_main(args) if args.chunk_bytes else pooled_main(args)
    out_path = args.out or os.path.join(ROOT, "profiles", "text", "text_c2.json")
    t0 = time.perf_counter()
    text = synthetic_corpus(args.records)
    n, nbytes = len(text), int(text.data.shape[0])
    log(f"corpus drawn in {time.perf_counter() - t0:.1f} s: {n} records, {nbytes} bytes")
    dev = torch.device("cuda", torch.cuda.current_device())
    rec = {"records": n, "text_bytes": nbytes, "vocabulary": VOCAB,
           "non_ascii_bytes": int((text.data >= 0x80).sum()),
           "text_step": TX.TEXT_STEP, "device": torch.cuda.get_device_name(0),
           "hbm_peak_TBps": HBM_PEAK / 1e12}

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data = torch.from_numpy(text.data).to(dev)
    off = torch.from_numpy(text.offsets).to(dev)
    torch.cuda.synchronize()
    rec["upload_first_ms"] = (time.perf_counter() - t0) * 1e3
    ts = []
    for _ in range(3):                       # the pages are touched now, as in call_ms below
        t0 = time.perf_counter()
        again = torch.from_numpy(text.data).to(dev)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    del again
    rec["upload_ms"] = statistics.median(ts)

    # the launch groups, on the buffers token_counts would make
    n_tok = torch.zeros(n, dtype=torch.int32, device=dev)
    n_uniq = torch.zeros(n, dtype=torch.int32, device=dev)
    recheck = torch.zeros(n, dtype=torch.uint8, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    a = TX._text_args(data, off, 0, nbytes, 0, n_tok, n_uniq, recheck, totals)
    st = _lib.stream_handle()
    _lib.call("bbgr_text_count", ctypes.byref(a), st)
    tokens = int(totals[0])
    # one whole call sizes the workspace the launch groups below run on
    keep = _lib.Workspace(grow=False)
    _lib.call_with_workspace("bbgr_text_unique", ctypes.byref(a), tokens, after=(st,), device=dev,
                             keep=keep)
    rec.update(device_tokens=tokens, tokens_per_record=tokens / max(n, 1),
               workspace_bytes=keep.buf.numel())

    def stage(bits):
        return lambda: _lib.call_with_workspace("bbgr_text_unique_stages", ctypes.byref(a), tokens,
                                                bits, after=(st,), keep=keep)

    groups = {"count": lambda: _lib.call("bbgr_text_count", ctypes.byref(a), st),
              "emit": stage(1), "sort": stage(2), "verify": stage(4)}
    kernels = {name: timed_events(fn, args.warmup, args.reps) for name, fn in groups.items()}
    for name, r in kernels.items():
        r["ns_per_token"] = r["median_ms"] * 1e6 / max(tokens, 1)
        log(name, r)
    c = kernels["count"]
    c["text_TBps"] = nbytes / (c["median_ms"] * 1e-3) / 1e12
    c["of_hbm_peak"] = c["text_TBps"] * 1e12 / HBM_PEAK
    rec["kernels"] = kernels
    rec["kernels_sum_ms"] = sum(r["median_ms"] for r in kernels.values())
    rec["sort_share"] = kernels["sort"]["median_ms"] / rec["kernels_sum_ms"]
    del keep

    ts = []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d_tok, d_uniq, info = TX.token_counts(text, dev)
        torch.cuda.synchronize()
        if k >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    rec["call_ms"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                      "reps": args.reps}
    rec["info"] = info
    log("call_ms", rec["call_ms"], info)

    m = n if args.host_records is None else min(args.host_records, n)
    strings = strings_of(text, m)
    t0 = time.perf_counter()
    h_tok, h_uniq = host_loop(strings)
    host_s = time.perf_counter() - t0
    rec["host_loop"] = {"records": m, "subset": "all" if m == n else f"the first {m}",
                        "seconds": host_s, "us_per_record": host_s * 1e6 / max(m, 1),
                        "tokens": int(h_tok.sum(dtype=np.int64))}
    rec["vs_host"] = {
        "records_compared": m,
        "n_tokens": bool(np.array_equal(d_tok[:m].cpu().numpy(), h_tok)),
        "n_unique_tokens": bool(np.array_equal(d_uniq[:m].cpu().numpy(), h_uniq)),
        "rechecked": info["rechecked"]}
    rec["call_vs_host_loop"] = host_s * (n / max(m, 1)) * 1e3 / rec["call_ms"]["median_ms"]
    log("host_loop", rec["host_loop"], rec["vs_host"])

    lines = min(args.jsonl_lines, m)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "reviews.jsonl")
        write_jsonl(path, strings[:lines])
        del strings
        jl = {"lines": lines, "file_bytes": os.path.getsize(path)}
        cols = {}
        for mode in ("host", "device", "host", "device"):      # the second pair is reported
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cols[mode] = FT.review_columns_from_jsonl(path, tokens=mode, device=dev)[0]
            torch.cuda.synchronize()
            jl[f"{mode}_s"] = time.perf_counter() - t0
        jl["host_over_device"] = jl["host_s"] / jl["device_s"]
        jl["columns_equal"] = bool(
            np.array_equal(cols["host"].n_tokens, cols["device"].n_tokens.cpu().numpy())
            and np.array_equal(cols["host"].n_unique_tokens,
                               cols["device"].n_unique_tokens.cpu().numpy()))
    rec["jsonl"] = jl
    log("jsonl", jl)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
