"""bench.py --dump-outputs: what the last timed step computed, as DIR/<name>.npy in float64 with the samples they hold in
DIR/sample_index.npy -- every sample, or, above 64 MB in all, a fixed, seeded sample of them (the same rows from every
output) -- and every NaN / inf recorded in DIR/nonfinite.npy; the shares of several ranks merge into the same dump; and,
on the GPU, the very outputs the oracle computes for the benchmark's seeded inputs, and what a plain line holds against one
with --full."""

import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


def _outputs(n, n_hla, n_cell=None, seed=0):
    rng = np.random.default_rng(seed)
    o = {"h1": rng.integers(0, n_hla, n).astype(np.int32), "h2": rng.integers(0, n_hla, n).astype(np.int32),
         "prob": rng.random(n), "matching": rng.random(n), "dosage": rng.random((n, n_hla))}
    if n_cell:
        o["postprob"] = rng.random((n, n_cell))
    return o


def _underflow(o, rows):
    """What the reference gives a sample whose posterior sums underflow: a call with prob inf, or no call; NaN dosage."""
    a, b = rows
    o["prob"][a] = np.inf
    o["dosage"][a] = np.nan
    o["h1"][b] = o["h2"][b] = -2**31
    o["prob"][b] = 0.0
    o["dosage"][b] = np.nan
    if "postprob" in o:
        o["postprob"][a, ::2] = np.inf
        o["postprob"][a, 1::2] = np.nan
        o["postprob"][b, 3] = -np.inf
    return o


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_dump_holds_every_sample_while_it_fits(tmp_path):
    o = _outputs(10_000, 50)                                  # the benchmark's default: 4.3 MB
    bench.dump_outputs(str(tmp_path), o)
    got = _files(str(tmp_path))
    assert sorted(got) == sorted(list(o) + ["nonfinite", "sample_index"])
    assert got["nonfinite"].shape == (0, 4)
    assert np.array_equal(got["sample_index"], np.arange(10_000))
    for k, v in o.items():
        assert got[k].dtype == np.float64 and np.array_equal(got[k], v.astype(np.float64)), k


def test_nan_and_inf_are_kept_with_every_sample(tmp_path):
    o = _underflow(_outputs(1000, 50, 60), (7, 500))
    bench.dump_outputs(str(tmp_path), o)
    raw = _files(str(tmp_path))
    assert all(np.isfinite(v).all() for v in raw.values())    # every file holds numbers ...
    assert len(raw["nonfinite"]) == 1 + 50 + 60 + 50 + 1
    got = bench.read_dump(str(tmp_path))                      # ... and the dump restores every value as computed
    assert np.array_equal(got.pop("sample_index"), np.arange(1000))
    assert _same(got, {k: v.astype(np.float64) for k, v in o.items()})
    assert got["h1"][500] == -2**31 and np.isinf(got["prob"][7]) and np.isneginf(got["postprob"][500, 3])


def test_dump_of_large_outputs_is_a_fixed_sample_under_64_mb(tmp_path):
    o = _underflow(_outputs(10_000, 50, 1275), (3, 9000))     # --prob: 106 MB of outputs
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, o)
    bench.dump_outputs(b, o)
    assert _size(a) <= 64_000_000
    got = bench.read_dump(a)
    rows = got.pop("sample_index").astype(np.int64)
    assert len(rows) > 1000 and np.all(np.diff(rows) > 0) and rows[-1] < 10_000
    assert _same(got, {k: v[rows].astype(np.float64) for k, v in o.items()})
    assert _same(_files(a), _files(b))


@pytest.mark.parametrize("n_cell", [None, 1275])
@pytest.mark.parametrize("world", [2, 3])
def test_rank_shares_merge_into_the_single_process_dump(tmp_path, world, n_cell):
    """bench.py's multi-process route: every rank takes its rows of the step's seeded sample from its own contiguous slice
    (dump_part at its offset), rank 0 writes the gathered shares in rank order -- the same files as one process holding
    every sample."""
    from hibag_amd.dist import shard_bounds
    n = 10_000
    o = _underflow(_outputs(n, 50, n_cell), (4999, 5001))     # (underflow rows on both sides of a slice boundary)
    bench.dump_outputs(str(tmp_path / "one"), o)
    parts = []
    for rank in range(world):
        lo, hi = shard_bounds(n, world, rank)
        mine = {k: v[lo:hi] for k, v in o.items()}
        parts.append(bench.dump_part(mine, bench.dump_rows(n, mine), lo))
    bench.write_dump(str(tmp_path / "ranks"), parts)
    assert _same(_files(str(tmp_path / "one")), _files(str(tmp_path / "ranks")))


@pytest.mark.gpu
def test_bench_dump_equals_the_oracle(tmp_path, oracle):
    from hibag_amd import synth
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-extras",
                        "--no-cpu-baseline", "--dump-outputs", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, p.stderr[-2000:]
    model, founders, af = synth.make_model(bench.SHAPE)
    geno, _ = synth.make_samples(founders, af, bench.SAMPLES_PER_GPU, seed=synth.DEFAULT_SEED + 1)
    want = oracle.predict(oracle.flatten(model), geno, vote_method=1, avx2=True, n_threads=8)
    assert all(np.isfinite(v).all() for v in _files(out).values())
    got = bench.read_dump(out)
    assert sorted(got) == ["dosage", "h1", "h2", "matching", "prob", "sample_index"]
    assert np.array_equal(got.pop("sample_index"), np.arange(len(geno)))
    for k, v in got.items():                                  # every sample, the underflowing ones included
        assert np.array_equal(v, np.asarray(want[k], np.float64), equal_nan=True), k


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--full", "--no-extras", "--no-cpu-baseline"]])
def test_bench_line_plain_and_full(extra):
    """A plain run's line is the headline figure and its configuration; --full adds the roofline of the same timed steps
    and the calls' accuracy (--no-extras / --no-cpu-baseline keep the other legs out)."""
    import json
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "hlaPredict() samples/sec, 10k samples x 100-classifier HLA-B"
    assert (d["unit"], d["higher_is_better"], d["dtype"], d["steps"], d["warmup"]) == ("samples/s", True, "f64", 3, 1)
    assert d["value"] > 0 and d["value"] * d["ms_per_step"] * 1e-3 == pytest.approx(bench.SAMPLES_PER_GPU, rel=1e-9)
    assert all(v == 0 for v in d["handover_faults"].values())
    moved = {"roofline", "call_accuracy_vs_truth", "protocol", "host_inclusive", "api_inclusive", "host_inclusive_100k",
             "other_configs", "cpu_baseline", "classifier_shard_check", "classifier_sharded"}
    if not extra:
        assert not moved & set(d)
        assert "k_total_ms" not in d["ranks"][0]
    else:
        assert moved & set(d) == {"roofline", "call_accuracy_vs_truth"}
        assert d["call_accuracy_vs_truth"] > 0.99
        assert d["roofline"]["bound"] == "simd-issue" and set(d["roofline"]["kernels_ms_per_step"]) >= {"total", "accum"}
