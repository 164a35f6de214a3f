"""bench.py --dump-outputs on the GPU: the arrays written are what the timed
path handed its caller in the last step.

* C2 (the plain run's workload): `results.npy` holds all 1M u16 checksums as
  float32, equal to the oracle's on a sample of images (first, last, random),
  and a second workload built the same way dumps identical arrays.
* FILL on C2's layout: `fields.npy` are the two bytes stored at offset 28 of
  every image and spell `results.npy`; `images.npy` is the arena's seeded
  sample, the same positions in every run, equal to the arena's bytes there.

* The plain command line once as a process: K steps timed, the contract's
  fields, no --full key in the line, `results.npy` written.

The other workloads are stepped in-process (bench.Workload /
bench.dump_outputs, the code main() runs); no timing there.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bench  # noqa: E402  (the repository root is on sys.path, tests/conftest.py)


@pytest.fixture(scope="module")
def ctx(built_lib):
    import tcpck
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    c = tcpck.Context(0)
    yield c
    c.close()


def _dump(name, ctx, out_dir, steps=3, arenas=2):
    """`steps` steps of config `name` over `arenas` batches taken in turn, then its dump."""
    w = bench.Workload(name, ctx, torch.cuda.current_stream(), 0, 1, arenas)
    for _ in range(steps):
        w.step()
    bench.dump_outputs(w, str(out_dir), 0)
    return w, {p.stem: np.load(p) for p in out_dir.iterdir()}


def test_c2_results_dump(ctx, oracle_c, tmp_path):
    _, count, L = bench.CONFIGS["c2"][1:]
    w, got = _dump("c2", ctx, tmp_path / "a")
    assert set(got) == {"results"}
    res = got["results"]
    assert res.dtype == np.float32 and res.shape == (count,)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    rng = np.random.default_rng(5)
    idx = np.unique(np.concatenate([np.arange(64), np.arange(count - 64, count), rng.integers(0, count, 4096)]))
    sample = w.arena.view(count, L)[torch.from_numpy(idx).cuda()].cpu().numpy().reshape(-1)
    exp = oracle_c.batch(sample, stride=L, length=L, count=idx.size)
    np.testing.assert_array_equal(res[idx], exp.astype(np.float32))
    del w
    torch.cuda.empty_cache()
    # the same arguments again: identical inputs, so identical arrays (another step count ends on the other arena)
    w2, again = _dump("c2", ctx, tmp_path / "b", steps=2)
    np.testing.assert_array_equal(again["results"], res)
    del w2
    torch.cuda.empty_cache()


def test_plain_run_line_and_dump(tmp_path):
    """The command every change is measured with, once as a process: K timed
    steps, the contract's fields, none of the --full keys, and the dump."""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, f"{ROOT}/bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (3, 1, 1)
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["dtype"] == "u16"
    assert line["higher_is_better"] is True and line["value"] > 0
    # ms_per_step is the time of one of the K steps: value's bytes over it give value back
    count, L = bench.CONFIGS["c2"][2:]
    assert line["value"] == pytest.approx(count * L / (line["ms_per_step"] * 1e-3) / bench.GIB, rel=1e-3)
    full_only = {"one_arena", "e2e", "cpu_baseline", "c1"} | {key for _, key in bench.EXTRAS}
    assert not full_only & set(line)
    res = np.load(tmp_path / "out" / "results.npy")
    assert res.dtype == np.float32 and res.shape == (count,)


def test_fill_dump_fields_and_sampled_images(ctx, tmp_path):
    _, count, L = bench.EXTRA["fill"][1:]
    w, got = _dump("fill", ctx, tmp_path, steps=2)
    assert set(got) == {"results", "fields", "images"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    fields = got["fields"].reshape(count, 2)
    np.testing.assert_array_equal(fields[:, 0] + 256.0 * fields[:, 1], got["results"])  # stored as the u16 lies in memory
    # the arena (1.5 GB) is cut to DUMP_MAX_ELEMS bytes at positions that depend on DUMP_SEED and its size alone
    at = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, count * L, bench.DUMP_MAX_ELEMS))
    assert got["images"].shape == (bench.DUMP_MAX_ELEMS,)
    last = w.bufs[(w.turn - 1) % w.n_arenas]
    np.testing.assert_array_equal(got["images"], last[torch.from_numpy(at).cuda()].cpu().numpy().astype(np.float32))
    del w
    torch.cuda.empty_cache()
