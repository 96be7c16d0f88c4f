"""GPU: bench.py's plain run and --dump-outputs.

* collect_outputs holds what the last step left its caller: the loss, the
  batch and the updated tables' rows (by input id), unchanged by later steps,
  and identical for two trainers built from the same arguments;
* a plain run (no --full) times exactly --steps steps, prints the headline
  keys without the figures of --full, and writes the dump as float32 /
  float64 .npy files within the size limit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bbgr.graph import BipartiteGraph  # noqa: E402
from bbgr.synthetic import synthetic_credibility, synthetic_edges  # noqa: E402
from bbgr.trainer import FusedTrainer, GraphedStep  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        sys.path.insert(0, ROOT)
        import bench as b
    finally:
        sys.argv = argv
    return b


def _trainer(order):
    U, I, E = 3000, 1200, 60000
    e = synthetic_edges(U, I, E, seed=5, items="zipf")
    g = BipartiteGraph(e, U, I, "cuda", vertex_order=order)
    return FusedTrainer(g, "v2_pop", cred=synthetic_credibility(U, 5), emb_dim=64,
                        num_layers=3, batch_size=256, frontier=True)


@pytest.mark.parametrize("order,graphed", [("degree", False), ("input", False),
                                           ("degree", True)])
def test_collect_outputs_is_the_last_steps_state(bench, order, graphed):
    a, b = _trainer(order), _trainer(order)
    step_a = a.step
    if graphed:
        step_a = GraphedStep(a).step   # (runs the trainer's first step itself, eagerly)
        b.step()
    for _ in range(3):
        loss = step_a()
        b.step()
    out = bench.collect_outputs(a, loss, False)
    want_loss = float(loss)
    sd = {k: v.cpu().numpy() for k, v in a.state_dict().items()}
    users, pos, neg = (x.cpu().numpy() for x in a.batch())
    a.step()   # a later step must not reach what was collected
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert out["loss"].shape == (1,) and float(out["loss"][0]) == want_loss
    np.testing.assert_array_equal(out["batch_users"], users)
    np.testing.assert_array_equal(out["batch_pos"], pos)
    np.testing.assert_array_equal(out["batch_neg"], neg)
    np.testing.assert_array_equal(out["user_emb_batch"], sd["user_emb.weight"][users])
    np.testing.assert_array_equal(out["item_emb_pos"], sd["item_emb.weight"][pos])
    np.testing.assert_array_equal(out["item_emb_neg"], sd["item_emb.weight"][neg])
    for side, n in (("user", 3000), ("item", 1200)):
        rows = out[f"{side}_sample_rows"].astype(np.int64)
        assert rows.size == n and np.array_equal(rows, np.arange(n))   # small table: every row
        np.testing.assert_array_equal(out[f"{side}_emb_sample"], sd[f"{side}_emb.weight"][rows])
    # same arguments, same inputs and results: the other trainer's dump is equal
    other = bench.collect_outputs(b, b.loss, False)
    assert set(other) == set(out)
    for k in out:
        np.testing.assert_array_equal(other[k], out[k], err_msg=k)


def test_sample_rows_are_fixed_and_bounded(bench):
    """A table larger than the per-table budget is sampled: the same distinct
    rows on every call, within the budget."""
    class _T:   # collect_outputs reads only these
        U, I, d = 1 << 20, 1 << 19, 64
        user_w = torch.zeros(U, d, device="cuda")
        item_w = torch.zeros(I, d, device="cuda")

        class graph:
            user_order = item_order = None

        @staticmethod
        def batch():
            z = torch.zeros(4, dtype=torch.int64, device="cuda")
            return z, z, z
    o1 = bench.collect_outputs(_T, torch.zeros((), device="cuda"), False)
    o2 = bench.collect_outputs(_T, torch.zeros((), device="cuda"), False)
    n = bench.DUMP_TABLE_BYTES // (4 * 64)
    for side, size in (("user", _T.U), ("item", _T.I)):
        rows = o1[f"{side}_sample_rows"]
        assert rows.size == n and np.unique(rows).size == n and rows.max() < size
        np.testing.assert_array_equal(rows, o2[f"{side}_sample_rows"])
        assert o1[f"{side}_emb_sample"].shape == (n, 64)
    assert sum(a.nbytes for a in o1.values()) <= 64 << 20


def test_plain_run_times_the_steps_and_dumps(tmp_path):
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C2",
           "--steps", "4", "--warmup", "1", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["steps"] == 4 and j["warmup"] == 1 and j["full"] is False
    assert j["unit"] == "edges/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0 and j["metric"]
    assert j["value"] == pytest.approx(j["edges_gathered_per_step"] * 1000.0 / j["ms_per_step"])
    for k in ("roofline", "cpu_baseline", "torch_gpu_reference", "dense_ms_per_step",
              "dropin_module_step"):
        assert k not in j, k
    assert "cpu baseline" not in r.stderr and "reference step" not in r.stderr
    files = sorted(p.name for p in dump.iterdir())
    assert files == sorted(n + ".npy" for n in (
        "loss", "batch_users", "batch_pos", "batch_neg", "user_emb_batch", "item_emb_pos",
        "item_emb_neg", "user_sample_rows", "user_emb_sample", "item_sample_rows",
        "item_emb_sample"))
    arrays = {p.stem: np.load(p) for p in dump.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert float(arrays["loss"][0]) == j["final_loss"]
    assert arrays["user_emb_batch"].shape == (4096, 64)
    assert np.isfinite(arrays["user_emb_sample"]).all() and arrays["user_emb_sample"].any()
