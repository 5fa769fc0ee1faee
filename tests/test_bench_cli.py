"""bench.py's options: a plain run is the headline leg only, `--full` runs every leg, `--dump-outputs DIR` writes the last
timed step's top-k (CPU: argument handling and the file format; GPU: a small run, twice, against its planted rows)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("no_cpu_baseline", "no_two_stage", "no_graph_eval", "no_encode", "no_extra_legs")


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_is_the_headline_leg_only(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert all(getattr(a, name) for name in LEGS)
    full = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--full")
    assert full.full and not any(getattr(full, name) for name in LEGS)
    assert _args(monkeypatch, "--full", "--no-encode").no_encode  # the per-leg switches still apply under --full
    with pytest.raises(SystemExit):
        _args(monkeypatch, "--graph-kernels", "--dump-outputs", "x")


def test_dump_outputs_format_and_sample(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(0)
    scores = torch.rand(6, 5, generator=g).sort(dim=1, descending=True).values
    ids = torch.randint(0, 1 << 40, (6, 5), generator=g)
    bench.dump_outputs(str(tmp_path / "whole"), scores, ids, seed=1)
    s, i = np.load(tmp_path / "whole" / "scores.npy"), np.load(tmp_path / "whole" / "ids.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and s.shape == i.shape == (6, 5)
    assert np.array_equal(s, scores.numpy()) and np.array_equal(i.astype(np.int64), ids.numpy())
    assert not (tmp_path / "whole" / "query_rows.npy").exists()
    # above the size limit: a fixed seeded sample of the query rows, the same one every time
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3 * (5 * 12 + 8))
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), scores, ids, seed=1)
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    assert rows.dtype == np.float64 and rows.shape == (3,) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "query_rows.npy"))
    r = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy"), scores.numpy()[r])
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy").astype(np.int64), ids.numpy()[r])


def test_inputs_depend_only_on_key_and_element_index():
    m32 = 0xFFFFFFFF

    def mix_ref(x):  # the same finaliser in plain wrap-around 32-bit arithmetic
        x ^= x >> 16
        x = (x * 0x7FEB352D) & m32
        x ^= x >> 15
        x = (x * 0x846CA68B) & m32
        return x ^ (x >> 16)

    xs = np.random.default_rng(0).integers(0, 1 << 32, 4096, dtype=np.int64)
    assert bench._mix32(torch.from_numpy(xs)).tolist() == [mix_ref(int(x)) for x in xs]
    # a value does not depend on how many are drawn with it; other keys give other values
    assert torch.equal(bench.counter_normal((7, 0), 4000, "cpu")[:1000], bench.counter_normal((7, 0), 1000, "cpu"))
    assert not torch.equal(bench.counter_normal((7, 0), 1000, "cpu"), bench.counter_normal((7, 1), 1000, "cpu"))
    z = bench.counter_normal((1, 0), 1 << 20, "cpu").double()
    assert abs(float(z.mean())) < 5e-3 and abs(float(z.std()) - 1.0) < 5e-3
    # a destination drawn twice takes the later draw
    u, last = bench.last_draw_per_destination(torch.tensor([5, 3, 5, 9, 3]))
    assert u.tolist() == [3, 5, 9] and last.tolist() == [4, 2, 3]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_bench_dump_outputs_are_the_last_timed_step(dev, tmp_path):
    # the input words on the GPU are the host's, bit for bit: nothing depends on the device or its launch geometry
    assert torch.equal(bench.counter_bits((5, 1), 1 << 20, dev).cpu(), bench.counter_bits((5, 1), 1 << 20, "cpu"))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    rows, steps, warmup, k = 200000, 3, 1, 50
    dumps = []
    for name in ("a", "b"):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--rows", str(rows), "--dim", "128", "--k", str(k), "--dump-outputs", str(out)],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")]
        assert len(lines) == 1, lines
        line = json.loads(lines[0])
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["hits_at_k"]["hits@50"] == 1.0
        assert not {"cpu_baseline", "sustained", "two_stage", "graph_eval", "encode", "end_to_end"} & set(line)  # a plain run
        dumps.append((np.load(out / "scores.npy"), np.load(out / "ids.npy")))
    (s, i), (s2, i2) = dumps
    assert s.dtype == np.float32 and i.dtype == np.float64 and s.shape == i.shape == (32, k)
    assert np.array_equal(s, s2) and np.array_equal(i, i2)  # same arguments, same inputs, same outputs
    assert np.all(s[:, 1:] <= s[:, :-1])
    # the last timed batch's planted rows are in its top-k
    gold = [bench.gold_row(warmup + steps - 1, q, rows) for q in range(32)]
    assert all(gold[q] in set(i[q].astype(np.int64).tolist()) for q in range(32))
