"""The cases the aggressive-coarsening and multipass tests share (CPU and GPU), and the rules restated in
plain Python from their specification, not from the C or HIP code.

The distance-two graph S2.  m1 are the marks of the PMIS split of a compacted S; c(i) numbers the points
with m1 == C in increasing i.  S2 has one row per such point.  Row c(i) is one walk of S_i in stored
order: for each k != i of S_i, k is a candidate when it is a C point, and then, whatever k's mark, every
C point l != i of S_k in stored order is one.  A candidate is kept at its first occurrence, in
discovery order, as column c(l).

The final marks.  m2 is the PMIS split of S2.  A stage-one C point stays C when m2 is C or ISPT (an empty
S2 row), else it becomes F; every other point keeps m1.

Multipass interpolation, on the final marks.  pass(i) = 0 for C points; an F point gets 1 + the least
pass(j) over the j != i of S_i that have a number; points never numbered (and ISPT points) have empty
rows.  Row i of pass p >= 1 with N_i = { j in S_i : j != i, pass(j) = p - 1 }: walk the stored entries
(i, k) of A; d is the last stored diagonal entry, tot the sum of the entries with k != i, sub the sum of
those with k in N_i; for k in N_i walk row k of P (untruncated, fine columns) in stored order: a column
joins the pattern at its first occurrence and hat w_c (from 0.0) receives a_ik p_kc.  Then
p_ic = -((tot / sub) hat w_c) / d, or 0.0 for the whole row when sub or d is 0.  C rows hold one 1.0.
Then the columns take their coarse numbers and the rows are truncated.

A case is (A, S, mark): A = (row_ptr, col_idx, val), S = (row_ptr, col_idx), mark the final marks.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

import amg_amd as A
import interp_std_cases as K
import pmis_restatement as R
from amg_amd._native import SSS_IMAT, SSS_MAT

FGPT, CGPT, ISPT = 0, 1, 2
PMIS, AGG, STD, MPASS = 3, 4, 2, 4
TRUNC = 0.2          # SSS_amg_pars_init's trunc_threshold
SMALLFLOAT = 1e-20   # include/sss_amg.h

Case = namedtuple("Case", "A S mark")
_keep = []


# ---------------------------------------------------------------- the rules, restated
def s2_restated(srp, sci, m1):
    srp, sci = np.asarray(srp), np.asarray(sci)
    cnum = np.cumsum(np.asarray(m1) == CGPT) - 1
    rp, ci = [0], []
    for i in range(len(srp) - 1):
        if m1[i] != CGPT:
            continue
        seen, row = set(), []
        for k in sci[srp[i]:srp[i + 1]]:
            if k == i:
                continue
            cand = ([k] if m1[k] == CGPT else []) + [l for l in sci[srp[k]:srp[k + 1]] if l != i and m1[l] == CGPT]
            for l in cand:
                if l not in seen:
                    seen.add(l)
                    row.append(int(cnum[l]))
        ci += row
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32)


def final_marks_restated(srp, sci):
    """(final marks, m1, (S2 row_ptr, S2 col_idx)) of a compacted S, with the restated PMIS split."""
    m1 = R.pmis_restated(srp, sci)[0]
    s2 = s2_restated(srp, sci, m1)
    mark = np.array(m1, np.int32)
    cpts = np.flatnonzero(m1 == CGPT)
    if len(cpts):
        m2 = R.pmis_restated(*s2)[0]
        for c, i in enumerate(cpts):
            if not (m2[c] == CGPT or m2[c] == ISPT):
                mark[i] = FGPT
    return mark, m1, s2


def pass_numbers(srp, sci, mark):
    n = len(mark)
    num = np.where(np.asarray(mark) == CGPT, 0, -1)
    while True:
        new = {}
        for i in range(n):
            if mark[i] != FGPT or num[i] >= 0:
                continue
            have = [num[j] for j in sci[srp[i]:srp[i + 1]] if j != i and num[j] >= 0]
            if have:
                new[i] = 1 + min(have)
        if not new:
            return num
        for i, p in new.items():
            num[i] = p


def rows_restated(c):
    """The untruncated rows of P in fine columns: a list of (columns, values) per row, and the pass numbers."""
    arp, aci, av = (np.asarray(x) for x in c.A)
    srp, sci = (np.asarray(x) for x in c.S)
    n = len(c.mark)
    num = pass_numbers(srp, sci, c.mark)
    rows = [([i], [1.0]) if c.mark[i] == CGPT else ([], []) for i in range(n)]
    for p in range(1, int(num.max()) + 1 if n else 0):
        for i in np.flatnonzero(num == p):
            N = {int(j) for j in sci[srp[i]:srp[i + 1]] if j != i and num[j] == p - 1}
            cols, w = [], {}
            d = tot = sub = 0.0
            for q in range(arp[i], arp[i + 1]):
                k, a = int(aci[q]), float(av[q])
                if k == i:
                    d = a
                    continue
                tot = tot + a
                if k not in N:
                    continue
                sub = sub + a
                for col, pkc in zip(*rows[k]):
                    if col not in w:
                        w[col] = 0.0
                        cols.append(col)
                    w[col] = w[col] + a * pkc
            if sub == 0.0 or d == 0.0:
                vals = [0.0] * len(cols)
            else:
                vals = [-((tot / sub) * w[col]) / d for col in cols]
            rows[i] = (cols, vals)
    return rows, num


def truncate_restated(rows, eps):
    out = []
    for cols, vals in rows:
        pmax = nmin = psum = nsum = pkept = nkept = 0.0
        for v in vals:
            if v > 0:
                psum, pmax = psum + v, max(pmax, v)
            elif v < 0:
                nsum, nmin = nsum + v, min(nmin, v)
        pmax, nmin = pmax * eps, nmin * eps
        keep = []
        for col, v in zip(cols, vals):
            if v >= pmax:
                keep.append((col, v, True))
                pkept = pkept + v
            elif v <= nmin:
                keep.append((col, v, False))
                nkept = nkept + v
        pfac = psum / pkept if pkept > SMALLFLOAT else 1.0
        nfac = nsum / nkept if nkept < -SMALLFLOAT else 1.0
        out.append(([col for col, _, _ in keep], [v * (pfac if pos else nfac) for _, v, pos in keep]))
    return out


_rows = {}


def restated(name, c, eps):
    """((row_ptr, col_idx, val, ncols), passes, unreached rows) of a case; the untruncated rows are computed once."""
    if name not in _rows:
        _rows[name] = rows_restated(c)
    rows, num = _rows[name]
    cmap = np.cumsum(np.asarray(c.mark) == CGPT) - 1
    rows = truncate_restated([([int(cmap[col]) for col in cols], vals) for cols, vals in rows], eps)
    rp = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int32)
    ci = np.array([col for r in rows for col in r[0]], np.int32)
    v = np.array([x for r in rows for x in r[1]], np.float64)
    unreached = [i for i in range(len(c.mark)) if c.mark[i] != CGPT and num[i] < 0]
    return (rp, ci, v, int((np.asarray(c.mark) == CGPT).sum())), int(num.max()), unreached


# ---------------------------------------------------------------- the cases
def coarsened(M, quiet, cs_type=AGG, interp_type=STD):
    """Case of one level: A, the compacted S and the marks SSS_amg_coarsen leaves; and P's (rows, cols)."""
    lib = A.lib()
    verts = lib.SSS_ivec_create(M.num_rows)
    P, S = SSS_MAT(), SSS_IMAT()
    p = R.pars(cs_type, interp_type)
    with quiet():
        rc = lib.SSS_amg_coarsen(C.byref(M), C.byref(verts), C.byref(P), C.byref(S), C.byref(p))
    if rc < 0:
        return None, None
    n = M.num_rows
    srp = np.ctypeslib.as_array(S.row_ptr, shape=(n + 1,)).copy()
    sci = np.ctypeslib.as_array(S.col_idx, shape=(max(int(srp[n]), 1),)).copy()[: srp[n]]
    mark = np.ctypeslib.as_array(verts.d, shape=(n,)).copy()
    return Case(A.csr_arrays(M), (srp, sci), mark), (P.num_rows, P.num_cols, bool(P.row_ptr))


def _case(a_rows, s_rows, mark):
    """a_rows: per row a list of (column, value) in stored order; s_rows: per row the columns of S."""
    A_ = K._csr_from_rows([[c for c, _ in r] for r in a_rows], [[v for _, v in r] for r in a_rows])
    return Case(A_, K._csr_from_rows(s_rows), np.array(mark, np.int32))


def _from_s(s_rows, mark, seed=5, extra=None):
    """Row i of A: the columns S_i u {i} (and extra[i]) sorted, off-diagonals -(0.5 + U[0, 1)), the
    diagonal the sum of their magnitudes + 1."""
    rng = np.random.default_rng(seed)
    a_rows = []
    for i, s in enumerate(s_rows):
        cols = sorted(set(s) | {i} | set((extra or {}).get(i, [])))
        off = {c: -(0.5 + rng.random()) for c in cols if c != i}
        a_rows.append([(c, off[c] if c != i else 1.0 - sum(off.values())) for c in cols])
    return _case(a_rows, s_rows, mark)


def mstar(K_):
    """n = 1 + K + K^2 + 3.  Point 0 and points 1..K are F, the rest C, the last three of them shared.
    S_0 names the F points 1..K only, so point 0 is of pass 2 and its candidates are the rows of P of
    all K neighbours: K (K + 3) of them, K^2 + 3 distinct; S_k names half of its own K C points, the
    shared ones, point 0, the other half."""
    n = 1 + K_ + K_ * K_ + 3
    shared = [n - 3, n - 2, n - 1]
    s_rows = [list(range(1, K_ + 1))]
    for k in range(1, K_ + 1):
        own = list(range(1 + K_ + (k - 1) * K_, 1 + K_ + k * K_))
        s_rows.append(own[: K_ // 2] + shared + [0] + own[K_ // 2:])
    s_rows += [[] for _ in range(n - 1 - K_)]
    extra = {i: [(i * 7 + 1) % n] for i in range(0, n, 3)}
    return _from_s(s_rows, [FGPT] * (K_ + 1) + [CGPT] * (n - 1 - K_), seed=K_, extra=extra)


def laplacian(n=60, seed=3):
    """A graph Laplacian (zero row sums) of a random connected graph; S = its adjacency, the marks the
    two-stage split's."""
    rng = np.random.default_rng(seed)
    adj = [set() for _ in range(n)]
    for i in range(1, n):
        for j in {int(rng.integers(0, i)), int(rng.integers(0, i))}:
            adj[i].add(j), adj[j].add(i)
    w = {}
    for i in range(n):
        for j in adj[i]:
            w[min(i, j), max(i, j)] = 0.5 + rng.random()
    a_rows, s_rows = [], []
    for i in range(n):
        cols = sorted(adj[i] | {i})
        off = {j: -w[min(i, j), max(i, j)] for j in adj[i]}
        dsum = 0.0
        for j in sorted(adj[i]):
            dsum = dsum - off[j]
        a_rows.append([(c, off[c] if c != i else dsum) for c in cols])
        s_rows.append(sorted(adj[i]))
    S = K._csr_from_rows(s_rows)
    return _case(a_rows, s_rows, final_marks_restated(*S)[0])


#: S of the hand-built split case: m1 = [C, F, C, F]; S2 row of point 0 is {c(2)} and nobody's S2 row
#: names it (lambda = 0 in S2: it becomes F); S2 row of point 2 is empty (ISPT in stage two: it stays C)
TWO_STAGE_S = [[1], [0, 2], [3], [2]]
TWO_STAGE_M1, TWO_STAGE_FINAL = [CGPT, FGPT, CGPT, FGPT], [FGPT, FGPT, CGPT, FGPT]


def hand_cases():
    F, Cc, I = FGPT, CGPT, ISPT
    chain = [[1]] + [[i - 1, i + 1] for i in range(1, 39)] + [[38]]
    return {
        "n1_c": _case([[(0, 2.0)]], [[]], [Cc]),
        "all_c": _from_s([[1, 2], [0], [0, 3], [2]], [Cc, Cc, Cc, Cc]),
        "ispt_row": Case(*K.small_cases()["ispt_row"][:3]),
        "two_stage": _from_s(TWO_STAGE_S, TWO_STAGE_FINAL),
        # the only C point at one end: point i is of pass i, |N_i| = 1
        "chain40": _from_s(chain, [Cc] + [F] * 39),
        # point 0 is of pass 2; rows 1 and 2 of P are {3, 4} and {4, 5}: column 4 comes twice
        "repeat_cols": _from_s([[1, 2], [3, 0, 4], [4, 0, 5], [], [], []], [F, F, F, Cc, Cc, Cc]),
        "mstar12": mstar(12),
        "star130": mstar(130),
        # row 0: a_01 + a_02 = 0 (sub = 0); row 3: a stored diagonal of 0.0 (d = 0)
        "sub_zero": _case([[(0, 3.0), (1, 1.5), (2, -1.5)], [(1, 1.0)], [(2, 1.0)]], [[1, 2], [], []], [F, Cc, Cc]),
        "d_zero": _case([[(0, 0.0), (1, -1.0), (2, -2.0)], [(1, 1.0)], [(2, 1.0)]], [[1, 2], [], []], [F, Cc, Cc]),
        # points 0 and 1 name each other only; point 2 names point 0: all three are never numbered
        "unreached": _from_s([[1], [0], [0], [4], []], [F, F, F, F, Cc]),
        # row 0 stores (0, 1) twice and two diagonal entries (the last one counts); row 2 names F point 0
        "dup_entries": _case([[(0, 9.0), (1, -1.0), (2, -0.5), (1, -0.25), (0, 4.0)], [(1, 2.0)],
                              [(0, -1.0), (2, 3.0), (1, -0.5)]], [[1, 2], [], [0]], [F, Cc, F]),
        # 0 is in S_1 but 1 is not in S_0; 1 is of pass 2 through 0
        "nonsym": _from_s([[2], [0], [], [1, 2]], [F, F, Cc, F], extra={0: [1]}),
        "laplacian": laplacian(),
    }


HAND = ["n1_c", "all_c", "ispt_row", "two_stage", "chain40", "repeat_cols", "mstar12", "star130", "sub_zero", "d_zero",
        "unreached", "dup_entries", "nonsym", "laplacian"]
SMALL = [h for h in HAND if h not in ("mstar12", "star130")]
NATURAL = ["p7_12", "a27_8", "bus", "circuit3000", "convdiff12"]
STENCILS = ["p7_12", "a27_8"]
_cache = {}


def all_cases(quiet):
    """name -> Case, computed once: the natural matrices with the two-stage marks, the levels of a 7-pt
    24^3 cs_type 4 hierarchy, the hand-built cases."""
    if _cache:
        return _cache
    for name in NATURAL:
        c, _ = coarsened(K.matrix(name), quiet)
        assert c is not None, name
        _cache[name] = c
    with quiet():
        H = A.Hierarchy(K.matrix("p7_24"), R.pars(AGG, STD))
    _keep.append(H)
    for l in range(H.num_levels):
        c, _ = coarsened(H.level(l).A, quiet)
        if c is not None:   # the coarsest level may have nothing strong
            _cache[f"p7_24_level{l}"] = c
    _cache.update(hand_cases())
    return _cache


def assert_same_graph(got, want, what=""):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), what
