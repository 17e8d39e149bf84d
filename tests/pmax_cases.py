"""The cap on the entries per row of P (SSS_SETUP_PMAX): the rule restated in plain Python
from its specification, not from the C or HIP code, and the inputs the CPU and GPU tests share.

The rule, per row of P in coarse columns, with eps the truncation threshold:

1. pos_sum, neg_sum (sums of the positive and of the negative entries, in stored order), pos_max, neg_min;
   the thresholds are pos_max * eps and neg_min * eps; an entry survives when v >= the positive threshold
   or v <= the negative one.
2. At most pmax survivors (or pmax == 0): the uncapped row.  The survivors are kept; pos_kept and neg_kept
   are their sums in stored order (an entry at or above the positive threshold is of the positive class,
   any other of the negative); a class is scaled by sum / kept when its kept sum is beyond SMALLFLOAT.
3. More: the row is capped.  The pmax survivors of largest |v| are kept, ties going to the earlier stored
   position, in stored order.  The factors as in 2; but a class that had entries and kept nothing beyond
   SMALLFLOAT is lost, and when the other class kept something its factor is (pos_sum + neg_sum) / its
   kept sum: the row sum of P survives.
"""
from __future__ import annotations

import numpy as np

import amg_amd as A
import interp_std_cases as K
import mpass_cases as MP

SMALLFLOAT = 1e-20   # include/sss_amg.h
EPS = [K.TRUNC, 0.0]
PMAX = [1, 2, 4, 7]
STD, EXTI, MPASS = 2, 3, 4


def row_restated(cols, vals, eps, pmax):
    """(kept columns, new values, survivors, capped) of one row given as Python lists."""
    psum = nsum = pmx = nmn = 0.0
    for v in vals:
        if v > 0:
            psum, pmx = psum + v, max(pmx, v)
        elif v < 0:
            nsum, nmn = nsum + v, min(nmn, v)
    tp, tn = pmx * eps, nmn * eps
    keep = [k for k, v in enumerate(vals) if v >= tp or v <= tn]
    survivors = len(keep)
    capped = pmax > 0 and survivors > pmax
    if capped:
        keep = sorted(sorted(keep, key=lambda k: (-abs(vals[k]), k))[:pmax])
    pkept = nkept = 0.0
    for k in keep:
        if vals[k] >= tp:
            pkept = pkept + vals[k]
        else:
            nkept = nkept + vals[k]
    pos_has, neg_has = pkept > SMALLFLOAT, nkept < -SMALLFLOAT
    pfac = psum / pkept if pos_has else 1.0
    nfac = nsum / nkept if neg_has else 1.0
    if capped:
        if psum > 0 and not pos_has and neg_has:
            nfac = (psum + nsum) / nkept
        if nsum < 0 and not neg_has and pos_has:
            pfac = (psum + nsum) / pkept
    return [cols[k] for k in keep], [vals[k] * (pfac if vals[k] >= tp else nfac) for k in keep], survivors, capped


def restated(P, eps, pmax):
    """((row_ptr, col_idx, val, ncols), survivors per row, capped flags per row) of P = (row_ptr, col_idx, val, ncols)."""
    rp, ci, v = P[0].tolist(), P[1].tolist(), P[2].tolist()
    orp, oci, ov, surv, capped = [0], [], [], [], []
    for i in range(len(rp) - 1):
        c, x, s, cap = row_restated(ci[rp[i]:rp[i + 1]], v[rp[i]:rp[i + 1]], eps, pmax)
        oci += c
        ov += x
        orp.append(len(oci))
        surv.append(s)
        capped.append(cap)
    out = (np.array(orp, np.int32), np.array(oci, np.int32), np.array(ov, np.float64), P[3])
    return out, np.array(surv), np.array(capped, bool)


# ---------------------------------------------------------------- hand-built rows
#: rows of one P with 6 columns: six survivors; a tie of equal |v| with opposite signs; positives the cap
#: cuts entirely; a C row
HAND_ROWS = [
    [0.5, -0.1, 0.3, 0.05, -0.4, 0.2],
    [0.5, -0.25, 0.25, -0.5, 0.125],
    [0.1, -0.6, -0.5, 0.05, -0.4],
    [1.0],
]
HAND_PMAX = [3, 3, 2, 3]   # the cap each hand-built row is worked out for


def hand_p():
    rp = np.concatenate([[0], np.cumsum([len(r) for r in HAND_ROWS])]).astype(np.int32)
    ci = np.array([c for r in HAND_ROWS for c in range(len(r))], np.int32)
    return rp, ci, np.array([v for r in HAND_ROWS for v in r], np.float64), 6


# ---------------------------------------------------------------- the inputs
_inputs = {}


def input_names(quiet):
    """(interp_type, case name) of every input: the cases of interp_std_cases with the standard and the
    extended+i weights, the cases of mpass_cases with the multipass ones."""
    return [(t, n) for t in (STD, EXTI) for n in K.all_cases(quiet)] + [(MPASS, n) for n in MP.all_cases(quiet)]


def untruncated(itype, name, quiet):
    """(row_ptr, col_idx, val, ncols) of the host's P at truncation threshold 0.0 (which keeps every entry
    with its value), computed once.  SSS_SETUP_PMAX must not be set."""
    assert A.setup_pmax() == 0
    if (itype, name) not in _inputs:
        with quiet():
            if itype == MPASS:
                c = MP.all_cases(quiet)[name]
                P = A.interp_mpass(c.A, c.S, c.mark, 0.0)[:4]
            else:
                c = K.all_cases(quiet)[name]
                P = (A.interp_std if itype == STD else A.interp_exti)(c.A, c.S, c.mark, c.P, 0.0)
        _inputs[itype, name] = P
    return _inputs[itype, name]


def tiled(P, copies):
    """`copies` copies of P's rows one after the other (the same columns)."""
    rp, ci, v, nc = P
    nnz = len(ci)
    rps = np.concatenate([[0]] + [rp[1:].astype(np.int64) + k * nnz for k in range(copies)]).astype(np.int32)
    return rps, np.tile(ci, copies), np.tile(v, copies), nc


def serial_host_trunc(P, eps):
    """SSS_amg_interp_trunc on a copy of P (the in-place serial form below 2^20 entries, the row-parallel
    one from there), with the cap SSS_SETUP_PMAX names."""
    import ctypes as C
    lib = A.lib()
    rp, ci, v, nc = P
    M = lib.SSS_mat_struct_create(len(rp) - 1, nc, len(ci))
    C.memmove(M.row_ptr, rp.ctypes.data, rp.nbytes)
    if len(ci):
        C.memmove(M.col_idx, np.ascontiguousarray(ci, np.int32).ctypes.data, 4 * len(ci))
        C.memmove(M.val, np.ascontiguousarray(v, np.float64).ctypes.data, 8 * len(ci))
    pars = A.default_pars()
    pars.trunc_threshold = eps
    fn = lib.SSS_amg_interp_trunc
    fn.restype, fn.argtypes = None, [C.POINTER(A.SSS_MAT), C.POINTER(A.SSS_AMG_PARS)]
    fn(C.byref(M), C.byref(pars))
    try:
        return (*A.csr_arrays(M), M.num_cols)
    finally:
        lib.SSS_mat_destroy(C.byref(M))


# ---------------------------------------------------------------- whole setups
#: (cs_type, interp_type) of the hierarchies: PMIS with every interpolation, aggressive PMIS
HIER = [(3, 1), (3, 2), (3, 3), (3, 4), (4, 2)]
HIER_MATRIX = "p7_16"


def hier_key(cs, interp):
    return f"{HIER_MATRIX}_cs{cs}_interp{interp}"
