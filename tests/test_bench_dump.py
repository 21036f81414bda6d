"""bench.py --dump-outputs: what the last timed step computed, written as .npy files that two builds can compare output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _store():
    from oracle import violet_ref as R
    from pytorch_empirical_mvm_amd.store import ParamStore
    cfg = R.make_cfg("tiny", T=2, img=96, arch=dict(embed_dim=32, depths=(1, 1, 1, 1), num_heads=(1, 2, 4, 8), window=(8, 7, 7)), bert_layers=1)
    S = ParamStore(R.param_shapes(cfg), "cpu")
    g = torch.Generator().manual_seed(0)
    S.flat.copy_(torch.randn(S.flat.shape, generator=g))
    S.m.copy_(torch.randn(S.m.shape, generator=g))
    return S


def test_dump_outputs_writes_a_fixed_sample_in_float(tmp_path):
    import bench
    S = _store()
    losses = {"mtm": torch.tensor([2.5]), "vtm": torch.tensor([0.75])}
    bench.dump_outputs(str(tmp_path / "a"), S, losses, with_moments=True)
    bench.dump_outputs(str(tmp_path / "b"), S, losses, with_moments=True)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["adam_m.npy", "loss_mtm.npy", "loss_vtm.npy", "params.npy"]
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y), n       # same positions from run to run
        total += x.nbytes
    assert total <= bench.DUMP_LIMIT
    assert float(np.load(tmp_path / "a" / "loss_mtm.npy")) == 2.5 and float(np.load(tmp_path / "a" / "loss_vtm.npy")) == 0.75
    # a tensor no larger than the per-tensor sample is written whole, in name order, from the arena's own values
    p = np.load(tmp_path / "a" / "params.npy")
    first = sorted(S.index)[0]
    o, c, _ = S.index[first]
    assert c <= bench.DUMP_PER_PARAM and np.array_equal(p[:c], S.flat[o:o + c].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "adam_m.npy")[:c], S.m[o:o + c].numpy())
    bench.dump_outputs(str(tmp_path / "c"), S, losses, with_moments=False)
    assert "adam_m.npy" not in os.listdir(tmp_path / "c")


def test_steps_below_one_is_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES=""))
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bench_dumps_the_last_timed_step(tmp_path):
    """one GPU, a small batch: the loss files hold the losses the JSON line reports for the last timed step, the parameter sample is
    finite and the Adam moments are non-zero (the step's gradients reached them)"""
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--no-cpu-baseline",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    o = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert o["steps"] == 3
    for k, v in o["losses_last_step"].items():
        assert float(np.load(out / f"loss_{k}.npy")) == v, k
    prm, m = np.load(out / "params.npy"), np.load(out / "adam_m.npy")
    assert prm.dtype == np.float32 and prm.shape == m.shape and np.isfinite(prm).all() and np.isfinite(m).all() and np.abs(m).max() > 0
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64 << 20
