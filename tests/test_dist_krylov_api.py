"""CPU: the distributed Krylov solvers' public surface -- the C symbols are exported by
libsss_amg.so and declared in the header, and DistHierarchy has the two methods."""
from __future__ import annotations

import inspect
import re
import subprocess
from pathlib import Path

import pytest

import amg_amd as A
from amg_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ["sss_hip_dist_pcg", "sss_hip_dist_fgmres", "sss_hip_host_pcg_update", "sss_hip_host_dot2"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_declared_and_bound(name):
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert name in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert re.search(r"\b%s\s*\(" % name, (ROOT / "include" / "sss_hip.h").read_text())
    assert name in N.ABI_SYMBOLS
    assert getattr(A.lib(), name).argtypes   # the ctypes prototype is declared


def test_dist_hierarchy_has_the_solvers():
    for meth, pars in (("pcg", ["self", "tol", "maxit"]), ("fgmres", ["self", "tol", "restart", "maxit"])):
        f = getattr(A.DistHierarchy, meth)
        assert list(inspect.signature(f).parameters) == pars
    sig = inspect.signature(A.DistHierarchy.fgmres).parameters
    assert sig["restart"].default == 20 and sig["maxit"].default == 100
    assert inspect.signature(A.DistHierarchy.pcg).parameters["maxit"].default == 100


def test_lab_timer_is_not_public():
    """The fused-against-chain timer is a lab entry point: exported, but not in the public header."""
    assert hasattr(A.lib(), "sss_lab_time_pcg_fused")
    assert "sss_lab_time_pcg_fused" not in (ROOT / "include" / "sss_hip.h").read_text()
