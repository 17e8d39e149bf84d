"""MI355X-native AMG solve-phase engine (drop-in for the SSS_SOLVE path of txthpc/amg).

The product is the C-ABI library ``amg_amd/lib/libsss_amg.so`` (host C + gfx950 HIP kernels)
and the ``amg_amd/bin/amg`` CLI; this package is the Python binding used by tests and bench.py.
"""
from ._native import (  # noqa: F401
    ABI_SYMBOLS, COARSE, COARSE_LAST_FIELDS, COARSE_PMIS, COARSE_PMIS_AGG, COARSE_RS, INTERP_MPASS, SMOOTH, SPMV, Comm, DeviceHierarchy, DistHierarchy, Hierarchy, NumpyCSR, PartPlan,
    SSS_AMG, SSS_AMG_COMP,
    SSS_AMG_PARS, SSS_HIP_OPTS, SSS_MAT, SSS_RTN, SSS_SMTR, SSS_VEC, coarse_last, csr_arrays, default_pars, device_count,
    hbm_used_bytes, level_step, spmv_enc,
    agg_graph, generate, interp_exti, interp_mpass, interp_std, interp_trunc, lib, part_save, pmis, pmis_agg, rap_values, read_mtx, setup_pmax, std_pattern,
)
from .workloads import convdiff_csr  # noqa: F401
