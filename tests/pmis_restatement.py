"""The PMIS C/F split (cs_type 3) restated in numpy from its specification (DESIGN.md "PMIS
coarsening"), not from the C or HIP code, plus the matrices the CPU and GPU tests share.

The rule, on a compacted strength matrix S (CSR, n rows):

  lambda_i = stored entries of S whose column is i (the length of row i of S^T)
  h(i), uint32 with wrapping multiplies:
      i ^= i >> 16; i *= 0x7feb352d; i ^= i >> 15; i *= 0x846ca68b; i ^= i >> 16
  key_i = lambda_i << 32 | h(i)         (h is a bijection: keys are pairwise distinct)

  start:  S row i empty -> ISPT (2); else lambda_i = 0 -> FGPT (0); else undecided (-1)
  round, on the marks as they stand at its start:
    (a) every undecided i whose key is larger than the key of every undecided j != i in
        S_i u S^T_i becomes CGPT (1)
    (b) then every still undecided i with a CGPT point in row i of S becomes FGPT
  until nobody is undecided.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import amg_amd as A
from amg_amd._native import SSS_IMAT, SSS_MAT
from amg_amd.workloads import circuit_csr

FGPT, CGPT, ISPT, UNPT = 0, 1, 2, -1
PMIS, STD = 3, 2


def h32(i):
    i = np.asarray(i, dtype=np.uint32).copy()
    i ^= i >> np.uint32(16)
    i *= np.uint32(0x7FEB352D)
    i ^= i >> np.uint32(15)
    i *= np.uint32(0x846CA68B)
    i ^= i >> np.uint32(16)
    return i


def pmis_restated(rp, ci):
    """(marks, C points, rounds) of the rule above."""
    rp = np.asarray(rp, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    lam = np.bincount(ci, minlength=n).astype(np.uint64)
    key = (lam << np.uint64(32)) | h32(np.arange(n)).astype(np.uint64)
    mark = np.full(n, UNPT, np.int32)
    mark[lam == 0] = FGPT
    mark[np.diff(rp) == 0] = ISPT
    # the neighbourhood S_i u S^T_i as directed pairs (i, j), i != j
    src = np.concatenate([rows, ci])
    dst = np.concatenate([ci, rows])
    keep = src != dst
    src, dst = src[keep], dst[keep]
    rounds = 0
    while (mark == UNPT).any():
        rounds += 1
        assert rounds <= n, "the largest undecided key becomes C every round"
        und = mark == UNPT
        e = und[src] & und[dst]
        nbmax = np.zeros(n, np.uint64)          # 0 < every undecided key (lambda >= 1)
        np.maximum.at(nbmax, src[e], key[dst[e]])
        mark[und & (key > nbmax)] = CGPT
        e = (mark[rows] == UNPT) & (mark[ci] == CGPT)
        mark[rows[e]] = FGPT
    return mark, int((mark == CGPT).sum()), rounds


def check_invariants(rp, ci, mark, ncoarse, symmetric=None):
    """symmetric: whether S is known to have a symmetric pattern (None: whatever it has)."""
    rp = np.asarray(rp, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    lam = np.bincount(ci, minlength=n)
    off = rows != ci
    # No two C points are S-neighbours.  The rule gives this for every pair that is coupled in both
    # directions, so for every pair when S has a symmetric pattern (the stencils).  Where only i
    # depends on j (j in row i, i not in row j: the circuit, the bus) the rule itself lets both become
    # C: i first, after which nothing in j's row makes j an F point.
    both_c = (mark[rows] == CGPT) & (mark[ci] == CGPT) & off
    mutual = np.isin(rows * n + ci, ci * n + rows)
    assert not (both_c & mutual).any()
    if symmetric is None:
        symmetric = bool(mutual.all())
    assert symmetric == bool(mutual.all())
    if symmetric:
        assert not both_c.any()
    # every F point that started undecided has a C point in its row
    has_c = np.zeros(n, bool)
    has_c[rows[mark[ci] == CGPT]] = True
    started_undecided = (np.diff(rp) > 0) & (lam > 0)
    assert has_c[(mark == FGPT) & started_undecided].all()
    assert np.array_equal(mark == ISPT, np.diff(rp) == 0)
    assert set(np.unique(mark)) <= {FGPT, CGPT, ISPT}
    assert ncoarse == int((mark == CGPT).sum())


# ------------------------------------------------------------------------------- the matrices
_keep = []   # numpy-owned matrices whose buffers must outlive their SSS_MAT views


def matrix(name):
    if name == "bus":
        from conftest import BUS_MTX
        return A.read_mtx(BUS_MTX)
    if name.startswith("p7_"):
        return A.generate(7, int(name[3:]))
    if name.startswith("a27_"):
        return A.generate(27, int(name[4:]))
    if name.startswith("circuit"):
        M = circuit_csr(int(name[7:]))
        _keep.append(M)
        return M.mat
    raise ValueError(name)


def pars(cs_type=PMIS, interp_type=STD):
    p = A.default_pars()
    p.cs_type, p.interp_type = cs_type, interp_type
    return p


def strength(M, quiet):
    """The compacted strength matrix of M as numpy (row_ptr, col_idx), or None when nothing is strong
    (the split then fails, as the RS split does), with the marks and status SSS_amg_coarsen gave for
    cs_type 3."""
    lib = A.lib()
    verts = lib.SSS_ivec_create(M.num_rows)
    P, S = SSS_MAT(), SSS_IMAT()
    p = pars()
    with quiet():
        rc = lib.SSS_amg_coarsen(C.byref(M), C.byref(verts), C.byref(P), C.byref(S), C.byref(p))
    if rc < 0:
        return None, None, rc
    n = S.num_rows
    rp = np.ctypeslib.as_array(S.row_ptr, shape=(n + 1,)).copy()
    ci = np.ctypeslib.as_array(S.col_idx, shape=(max(int(rp[n]), 1),)).copy()[: rp[n]]
    mark = np.ctypeslib.as_array(verts.d, shape=(n,)).copy()
    return (rp, ci), mark, rc


def random_s(n, seed, maxrow=5):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, maxrow + 1, n)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ci = np.empty(rp[-1], np.int32)
    for i in range(n):
        others = np.setdiff1d(np.arange(max(0, i - 40), min(n, i + 41)), [i])
        ci[rp[i]:rp[i + 1]] = rng.choice(others, size=lens[i], replace=False) if len(others) >= lens[i] else others[: lens[i]]
    return rp, ci


def from_rows(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ci = np.array([c for r in rows for c in r], dtype=np.int32)
    return rp, ci


def hand_built():
    """name -> (row_ptr, col_idx): the edges of the rule."""
    long_row = [list(range(1, 701))] + [[i + 1] for i in range(1, 700)] + [[0]]
    return {
        "n1": from_rows([[]]),
        # row 2 is empty (ISPT) though rows 1 and 3 depend on it
        "empty_row": from_rows([[1], [0, 2], [], [2, 1], [3]]),
        # point 1 (lambda 0, F from the start) has point 0 as its only strong neighbour; 0 depends
        # only on the isolated point 2, so 0 never has an undecided neighbour
        "lambda0_neighbour": from_rows([[2], [0], []]),
        # nobody depends on points 3 and 4 (lambda 0): F from the start
        "nobody_depends": from_rows([[1], [2], [0], [0, 1], [3, 2]]),
        "long_row_700": from_rows(long_row),
        "n257": random_s(257, 3),
        "n1025": random_s(1025, 4),
        "n4097_long": random_s(4097, 5, maxrow=30),
    }


def hierarchy_levels(name, quiet):
    """The operators A_l of every level of the PMIS + interp 2 hierarchy of a matrix; keeps H alive."""
    with quiet():
        H = A.Hierarchy(matrix(name), pars())
    _keep.append(H)
    return [H.level(l).A for l in range(H.num_levels)]


_cache = {}


def all_s(quiet):
    """name -> (row_ptr, col_idx) of every S the tests split, computed once."""
    if _cache:
        return _cache
    for name in ["p7_12", "p7_24", "a27_8", "circuit3000", "bus"]:
        s, _, rc = strength(matrix(name), quiet)
        assert rc == 0
        _cache[name] = s
    for name in ["p7_24", "circuit3000"]:
        for l, Al in enumerate(hierarchy_levels(name, quiet)):
            s, _, rc = strength(Al, quiet)
            if s is not None:   # the coarsest level may have nothing strong: no S to split
                _cache[f"{name}_level{l}"] = s
    _cache.update(hand_built())
    return _cache
