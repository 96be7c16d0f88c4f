"""Benchmark: a review dump -> columns, text and id tables on MI355X.

    python tools/jsonl_bench.py [--lines 1000000] [--reps 5] [--out profiles/jsonl/jsonl_c2.json]

Workload: --lines synthetic reviews (tools/text_bench.py's seeded corpus and
its dump: json.dumps with ensure_ascii, so every non-ASCII character is a
\\uXXXX escape), written to a file.

Each launch group of bbgr.jsonl is timed alone with device events (median of
--reps after --warmup) on the file's bytes resident on the device, buffers
from torch's caching allocator included:

  count    bbgr_jsonl_count: the terminators of the chunk
  lines    bbgr_jsonl_lines: tile counts, their scan, the line ends
  scan     bbgr_jsonl_scan: structure, keys, values and sizes per line
  offsets  bbgr_jsonl_offsets: four exclusive scans
  write    bbgr_jsonl_write: the compact columns, unescaped ids and text
  number   bbgr_ids_number + bbgr_ids_table, users and items
  tokens   bbgr.text.token_counts on the resident text

`call_ms` is one whole bbgr.jsonl.read_reviews from the file (host clock: the
memory map, the host -> device copy, every host read, numbering and token
counts); `upload_ms` the copy alone. The baseline is the parent's reader on
the same file and machine: bbgr.features.review_columns_from_jsonl with
tokens="device" (`host_reader_ms`). The two results are compared column by
column (`equal`). Prints ONE JSON line; writes --out.
"""
from __future__ import annotations

import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bbgr  # noqa: E402,F401
import text_bench as TB  # noqa: E402
from bbgr import features as FT  # noqa: E402
from bbgr import jsonl as JL  # noqa: E402
from bbgr import text as TX  # noqa: E402


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def equal(parsed, host) -> bool:
    cols, user2idx, item2idx = host
    same = all(_np(getattr(parsed.cols, k)).tobytes() == _np(getattr(cols, k)).tobytes()
               for k in ("user", "item", "rating", "helpful_vote", "verified", "timestamp",
                         "ts_valid", "n_tokens", "n_unique_tokens"))
    same &= _np(parsed.cols.text.data).tobytes() == _np(cols.text.data).tobytes()
    same &= _np(parsed.cols.text.offsets).tolist() == _np(cols.text.offsets).tolist()
    for got, want in ((parsed.user_ids, user2idx), (parsed.item_ids, item2idx)):
        same &= _np(got.data).tobytes() == b"".join(s.encode("utf-8", "surrogatepass") for s in want)
    return bool(same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    t0 = time.perf_counter()
    corpus = TB.synthetic_corpus(args.lines)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "reviews.jsonl")
    TB.write_jsonl(path, TB.strings_of(corpus, args.lines))
    file_bytes = os.path.getsize(path)
    TB.log(f"[jsonl_bench] {args.lines} lines, {file_bytes / 1e6:.0f} MB, made in "
           f"{time.perf_counter() - t0:.1f} s")
    dev = torch.device("cuda", torch.cuda.current_device())

    # the whole call from the file (the first call also loads the library: run one before)
    JL.read_reviews(b'{"user_id":"u","parent_asin":"p","rating":1}\n')
    calls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t = time.perf_counter()
        parsed = JL.read_reviews(path)
        torch.cuda.synchronize()
        calls.append((time.perf_counter() - t) * 1e3)
    TB.log(f"[jsonl_bench] read_reviews {calls} ms, info {parsed.info}")

    host_arr = np.array(np.memmap(path, np.uint8, "r"))
    ups = []
    for _ in range(4):
        torch.cuda.synchronize()
        t = time.perf_counter()
        d = torch.from_numpy(host_arr).to(dev)
        torch.cuda.synchronize()
        ups.append((time.perf_counter() - t) * 1e3)

    # the launch groups, each alone, on the resident bytes
    key = torch.from_numpy(np.frombuffer(b"parent_asin", np.uint8).copy()).to(dev)
    rd = JL._Reader(d, key, "parent_asin", lambda b, e: host_arr[b:e].tobytes())
    rd.run()
    stages = {}
    for step in ("count", "lines", "scan", "offsets", "write"):
        stages[step] = TB.timed_events(getattr(rd, step), args.warmup, args.reps)
        if step == "scan":       # the scan's totals, as run() reads them
            rd.read_scan()
    n = int(rd.a.n_records)
    users = JL._joined([(rd.strs[0][0][:rd.a.user_bytes], rd.strs[0][1][:n])], dev)
    items = JL._joined([(rd.strs[1][0][:rd.a.item_bytes], rd.strs[1][1][:n])], dev)
    text = TX.ReviewText(*JL._joined([(rd.strs[2][0][:rd.a.text_bytes], rd.strs[2][1][:n])], dev))
    stages["number"] = TB.timed_events(lambda: (JL.number_ids(*users), JL.number_ids(*items)),
                                       args.warmup, args.reps)
    stages["tokens"] = TB.timed_events(lambda: TX.token_counts(text, dev), args.warmup, args.reps)
    kernels_ms = sum(s["median_ms"] for s in stages.values())

    t = time.perf_counter()
    host = FT.review_columns_from_jsonl(path, "parent_asin", tokens="device")
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t) * 1e3
    rec = {
        "bench": "jsonl", "lines": args.lines, "file_bytes": file_bytes, "info": parsed.info,
        "users": len(parsed.user_ids), "items": len(parsed.item_ids),
        "stages": stages, "stages_sum_ms": kernels_ms,
        "scan_gbps": file_bytes / stages["scan"]["median_ms"] / 1e6,
        "call_ms": statistics.median(calls), "call_first_ms": calls[0], "calls_ms": calls,
        "upload_ms": statistics.median(ups[1:]), "upload_first_ms": ups[0],
        "host_reader_ms": host_ms, "speedup": host_ms / statistics.median(calls),
        "equal": equal(parsed, host),
        "device": torch.cuda.get_device_name(dev),
    }
    os.remove(path)
    os.rmdir(tmp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
