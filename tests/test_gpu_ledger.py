"""GPU: the stored-format byte ledger behind bench.py's `vcycle_stored` (sss_hip_cycle_bytes).

The ledger walks one outer iteration into a discarded stream capture: it must not change the
iterates or the engine's pending-pass state, and its per-level bytes must be consistent with the
level's stored formats (every smoothed level moves at least its matrix once and at most a few
times per smoother sweep)."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

pytestmark = pytest.mark.gpu


def _cycles(D, n, k, ledger_every=False):
    D.upload(0, "b", np.ones(n))
    D.upload(0, "x", np.ones(n))
    out = []
    for _ in range(k):
        if ledger_every:
            D.cycle_bytes()
        D.cycle()
        out.append(D.residual_norm())
    return D.download(0, "x"), out


@pytest.mark.parametrize("kind,n,mode", [(7, 32, "throughput"), (27, 20, "throughput"), (7, 24, "parity")])
def test_cycle_bytes_no_side_effects_and_bounds(kind, n, mode):
    import amg_amd as A
    from conftest import build_hierarchy, quiet_ctx

    H = build_hierarchy(A.generate(kind, n), quiet_ctx)
    N = H.level(0).A.num_rows
    kw = dict(smoother="hybrid", coarse="direct", sum_order=1) if mode == "throughput" else \
        dict(smoother="exact", coarse="krylov", sum_order=0)
    D = A.DeviceHierarchy(H, device=0, **kw)
    x0, r0 = _cycles(D, N, 3)
    x1, r1 = _cycles(D, N, 3, ledger_every=True)   # the same cycles with the ledger walked before each
    assert np.array_equal(x0.view(np.uint64), x1.view(np.uint64))
    assert r0 == r1
    cb = D.cycle_bytes()
    nl = H.num_levels
    assert len(cb["levels"]) == nl
    assert cb["total"] == pytest.approx(sum(cb["levels"]) + cb["outer"] + cb["coarse"])
    tail = A.lib().sss_hip_tail_from(D.h)   # levels below a single-workgroup tail book into its first
    for l in range(nl - 1):
        if 0 < tail < l:
            assert cb["levels"][l] == 0.0
            continue
        info = D.level_info(l)
        stored = info.a_stream_bytes
        rows = H.level(l).A.num_rows
        # at least one pass over the matrix plus one vector; at most (sweeps + residual + 4) passes
        # over it with 20 row vectors each, plus R and P
        hi = 10 * stored + 200 * rows + 4 * 16 * H.level(l).P.num_nnzs
        if 0 < tail == l:
            hi = float("inf")
        assert 8 * rows < cb["levels"][l] <= hi, (l, cb["levels"][l], stored, rows)
    A0 = H.level(0).A
    # outer residual + norm: at least b, r and the gathered x; at most its CSR bytes + vectors
    assert 24 * N <= cb["outer"] <= 12 * A0.num_nnzs + 4 * (N + 1) + 48 * N
    if mode == "throughput" and tail <= 0:   # explicit inverse: n_c^2 doubles (else inside the tail)
        nc = H.level(nl - 1).A.num_rows
        assert cb["coarse"] >= 8 * nc * nc
    D.close()


def test_bench_plain_run_line_and_dump(tmp_path):
    """A plain `bench.py` run (no --full) end to end at 32^3: the headline fields, the secondary
    measurements null and not run, an option of theirs named on stderr, and --dump-outputs = the
    level-0 iterate and the residual norm of the last timed step.  The two dumped files must belong
    together: ||b - A0 x|| recomputed on the host from x.npy equals residual_norm.npy to float64
    rounding.  Bound: each residual entry carries at most ~8 * 2^-53 * sum|a_ij x_j| <= 1e-15 * 12 max|x|,
    over 32768 entries that is below 3e-12 * max|x| in the norm, and the sum of squares adds a relative
    n * 2^-53 = 4e-12 (1e-9 asked)."""
    import json
    import subprocess

    import amg_amd as A

    n = 32
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--n", str(n), "--steps", "2",
                        "--warmup", "1", "--converge-max", "50", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["full"] is False and rec["steps"] == 2 and rec["warmup"] == 1 and rec["dtype"] == "f64"
    assert rec["unit"] == "V-cycle iter/s" and rec["higher_is_better"] is True
    assert rec["value"] > 0 and abs(rec["ms_per_step"] * rec["value"] - 1e3) < 1e-6 * 1e3
    for k in ("roofline", "parity_mode", "cpu_baseline", "cpu_baseline_same_mode"):
        assert rec[k] is None, k
    cfg = rec["config"]
    assert cfg["rows"] == n ** 3 and cfg["iterations_to_tol"] is None and cfg["amg_pcg"] is None
    assert cfg["reference_convergence"] is None and cfg["relres_history"] is None
    assert rec["vcycle_stored"]["bytes_per_step"] > 0
    assert "converge iteration" not in r.stderr and "CPU baseline" not in r.stderr
    assert "--converge-max: no effect without --full" in r.stderr
    x = np.load(tmp_path / "d" / "x.npy")
    nrm = np.load(tmp_path / "d" / "residual_norm.npy")
    assert x.dtype == np.float64 and x.shape == (n ** 3,) and nrm.dtype == np.float64 and nrm.shape == (1,)
    assert rec["outputs"]["dir"] == str(tmp_path / "d") and "all 32768" in rec["outputs"]["x"]
    rp, ci, v = A.csr_arrays(A.generate(7, n))
    res = np.ones(n ** 3) - np.add.reduceat(v * x[ci], rp[:-1])
    assert np.isfinite(x).all() and nrm[0] > 0
    assert abs(float(np.sqrt(np.dot(res, res))) - nrm[0]) <= 1e-9 * nrm[0] + 3e-12 * np.abs(x).max()
