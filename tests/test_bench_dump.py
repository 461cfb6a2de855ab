"""bench.py --dump-outputs: the arrays are written exactly (float32 /
float64), whole when small and as the same seeded sample from run to run
when large; on the GPU a plain run's dump equals the oracle's pack of the
generator's words, and its JSON line carries the headline figure only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_exact_and_reproducible(tmp_path):
    import bench
    cap = bench.DUMP_CAP_DEFAULT
    big = torch.arange(3 * cap, dtype=torch.int64) * 7 + (1 << 40)
    arrays = {
        "packed": torch.tensor([0, 1, 254, 255], dtype=torch.uint8),
        "words": torch.tensor([-1, 1 << 40, 5], dtype=torch.int64),
        "status": torch.tensor([0, -3, 2], dtype=torch.int32),
        "sync_index": torch.tensor([-1, 0x01000002], dtype=torch.int32),
        "consumed": big,
    }
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, torch, arrays)
    bench.dump_outputs(b, torch, arrays)
    got = {k: np.load(os.path.join(a, k + ".npy")) for k in arrays}
    for k in arrays:
        assert np.array_equal(got[k], np.load(os.path.join(b, k + ".npy")))
    assert got["packed"].dtype == np.float32 and got["packed"].tolist() == [0, 1, 254, 255]
    assert got["words"].dtype == np.float64
    assert got["words"].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0, 256, 5, 0]
    assert got["status"].tolist() == [0, -3, 2]
    assert got["sync_index"].tolist() == [0xFFFFFFFF, 0x01000002]
    s = got["consumed"]
    assert s.dtype == np.float64 and s.shape == (cap,)
    idx = (s.astype(np.int64) - (1 << 40)) // 7   # the sample is exact and in order
    assert np.array_equal(idx * 7 + (1 << 40), s) and (np.diff(idx) >= 0).all()
    assert idx[0] < cap // 4 and idx[-1] > 3 * cap - cap // 4   # spread over the whole array


def test_steps_must_be_positive():
    import bench
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    assert bench.parse([]).full is False


@pytest.mark.gpu
def test_plain_run_dumps_what_it_computed(tmp_path):
    import bench
    n, cw = 4096, 128
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "1", "--chunks", str(n),
                        "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "GiB/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["value"] == pytest.approx(n * cw * 8 / 2 ** 30 / (d["ms_per_step"] * 1e-3), rel=2e-2)
    assert "kernels" not in d and "cpu_baseline" not in d and "roofline" not in d
    offs = np.arange(0, (n + 1) * cw, cw, dtype=np.uint64)
    words = O.gen_fill(offs, kind0=0, pz=bench.PZ["config2"])
    st, ref, ref_offs = O.pack_batch(words, offs)
    assert st == 0

    def load(name):
        return np.load(tmp_path / (name + ".npy"))
    assert np.array_equal(load("packed"), ref.astype(np.float32))
    assert np.array_equal(load("packed_byte_off"), ref_offs.astype(np.float64))
    assert np.array_equal(load("words"), words.view(np.uint32).astype(np.float64))
    assert not load("status").any()
    assert np.array_equal(load("consumed"), np.diff(ref_offs).astype(np.float64))
    ref_sync = O.sync_index(ref, ref_offs, offs)
    got = load("sync_index")
    given = got != 0xFFFFFFFF
    assert given.any() and np.array_equal(got[given], ref_sync[given].astype(np.float64))
