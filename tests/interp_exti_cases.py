"""The extended+i interpolation (interp_type 3) restated in plain Python floats from its specification
(DESIGN.md 6.7), not from the C or HIP code, and the hand-built cases the CPU and GPU tests share on top
of those of tests/interp_std_cases.py.  The restatement is sequential, so it is the rule bit for bit.

The rule, on the pattern of the standard interpolation (pattern_restated): a C row is one stored 1.0;
a row that is neither F nor C, or an F row with an empty pattern, gets nothing.  An F row i with
pattern C_i: d = a_ii (the row's last diagonal entry), ahat[c] = 0.0 for c in C_i, then the stored
entries (i, k), k != i, in stored order:

  1. k in C_i ...................... ahat[k] += a_ik
  2. else k in S_i and k is F ...... over the stored entries (k, l) of row k with l != k, (l in C_i or
                                     l == i) and a_kl * a_kk < 0, in stored order: den = their sum from
                                     0.0; if den != 0.0: f = a_ik / den and t = f * a_kl goes to d
                                     (l == i) or to ahat[l]; if den == 0.0: d += a_ik
  3. else .......................... d += a_ik

  p_ic = -ahat[c] / d, c in pattern order.

Then the columns get their coarse numbers, and each row is truncated: with pmax the largest positive
and nmin the smallest negative value of the row, an entry stays when v >= eps * pmax or v <= eps * nmin;
the kept positive values are scaled by (sum of the positive) / (sum of the kept positive) when the
latter exceeds 1e-20 in magnitude, the negative ones likewise; every sum in stored order.
"""
from __future__ import annotations

import numpy as np

import interp_std_cases as K
from interp_std_cases import CGPT, FGPT, Case

SMALLFLOAT = 1e-20   # include/sss_amg.h
HAND_EXTI = ["den_zero", "same_sign_skipped", "weak_in_pattern", "plus_i", "nonsym_no_aki"]
HAND = HAND_EXTI + ["star20", "star130", "n1_c", "ispt_row", "f_only_neighbours", "f_in_nobodys_s"]
SMALL = HAND_EXTI + ["n1_c", "ispt_row", "f_only_neighbours", "f_in_nobodys_s"]
NATURAL = ["p7_12", "a27_8", "bus", "circuit3000", "convdiff12"]


def weights_restated(c):
    """(values on the pattern c.P in fine numbering, rows that qualify for the row-sum check): the
    qualifying rows are the F rows with a non-empty pattern, |sum_j a_ij| <= 1e-14 |a_ii| and no
    strong F neighbour with den == 0."""
    arp, aci, av = [x.tolist() for x in c.A]
    srp, sci = [x.tolist() for x in c.S]
    prp, pci = [x.tolist() for x in c.P]
    mark = c.mark.tolist()
    n = len(mark)
    diag = [0.0] * n
    for i in range(n):
        for j in range(arp[i], arp[i + 1]):
            if aci[j] == i:
                diag[i] = av[j]
    val = [0.0] * len(pci)
    qualifying = []
    for i in range(n):
        if mark[i] == CGPT:
            val[prp[i]] = 1.0
            continue
        if mark[i] != FGPT or prp[i + 1] == prp[i]:
            continue
        pattern = pci[prp[i]:prp[i + 1]]
        ahat = {col: 0.0 for col in pattern}
        strong = set(sci[srp[i]:srp[i + 1]])
        d = diag[i]
        rowsum, den_zero = 0.0, False
        for j in range(arp[i], arp[i + 1]):
            rowsum += av[j]
            k, aik = aci[j], av[j]
            if k == i:
                continue
            if k in ahat:
                ahat[k] += aik
            elif k in strong and mark[k] == FGPT:
                akk = diag[k]
                terms = [(aci[m], av[m]) for m in range(arp[k], arp[k + 1])
                         if aci[m] != k and (aci[m] in ahat or aci[m] == i) and av[m] * akk < 0]
                den = 0.0
                for _, akl in terms:
                    den += akl
                if den != 0.0:
                    f = aik / den
                    for l, akl in terms:
                        t = f * akl
                        if l == i:
                            d += t
                        else:
                            ahat[l] += t
                else:
                    den_zero = True
                    d += aik
            else:
                d += aik
        for o, col in enumerate(pattern):
            val[prp[i] + o] = -ahat[col] / d
        if abs(rowsum) <= 1e-14 * abs(diag[i]) and not den_zero:
            qualifying.append(i)
    return val, qualifying


def truncate_restated(c, val, eps):
    """(row_ptr, col_idx, val, ncols) after the coarse renumbering and the truncation at eps."""
    prp, pci = [x.tolist() for x in c.P]
    cmap = (np.cumsum(c.mark == CGPT) - 1).tolist()
    rp, ci, out = [0], [], []
    for i in range(len(prp) - 1):
        row = val[prp[i]:prp[i + 1]]
        pmax = nmin = psum = nsum = pkept = nkept = 0.0
        for v in row:
            if v > 0:
                psum += v
                pmax = max(pmax, v)
            elif v < 0:
                nsum += v
                nmin = min(nmin, v)
        pmax *= eps
        nmin *= eps
        kept = []
        for o, v in enumerate(row):
            if v >= pmax:
                kept.append((o, v, True))
                pkept += v
            elif v <= nmin:
                kept.append((o, v, False))
                nkept += v
        pfac = psum / pkept if pkept > SMALLFLOAT else 1.0
        nfac = nsum / nkept if nkept < -SMALLFLOAT else 1.0
        for o, v, positive in kept:
            ci.append(cmap[pci[prp[i] + o]])
            out.append(v * (pfac if positive else nfac))
        rp.append(len(ci))
    return np.array(rp, np.int32), np.array(ci, np.int32), np.array(out, np.float64), int((c.mark == CGPT).sum())


_restated = {}


def restated(name, c, eps):
    """The restated P of a case at truncation eps and its qualifying rows; the weights computed once."""
    if name not in _restated:
        _restated[name] = weights_restated(c)
    val, qualifying = _restated[name]
    return truncate_restated(c, val, eps), qualifying


def _case(a_rows, s_rows, mark):
    """a_rows: per row the stored (column, value) pairs in stored order."""
    A = K._csr_from_rows([[col for col, _ in r] for r in a_rows], [[v for _, v in r] for r in a_rows])
    S = K._csr_from_rows(s_rows)
    mark = np.array(mark, np.int32)
    return Case(A, S, mark, K.pattern_restated(*S, mark))


F, C_ = FGPT, CGPT


def hand_cases():
    """The smallest shapes where the extended+i weights can go wrong (row 0 is the row of interest)."""
    return {
        # Strong F neighbours without a qualifying entry: point 1 has no entry (1, 0) and no column in
        # C_0 = {3}; point 2's only entry in C_0 u {0} has the sign of a_22.  Both a_0k go to d:
        # d = 5 - 1 - 1.5, p_03 = 2 / 2.5.
        "den_zero": _case(
            [[(0, 5.0), (1, -1.0), (2, -1.5), (3, -2.0)], [(1, 3.0), (4, -1.0)], [(2, 4.0), (3, 0.5)], [(3, 1.0)],
             [(4, 1.0)]],
            [[1, 2, 3], [], [3], [], []], [F, F, F, C_, C_]),
        # (1, 3) = +0.5 has the sign of a_11: neither in den (= -1 - 1) nor in ahat[3]
        "same_sign_skipped": _case(
            [[(0, 4.0), (1, -1.25), (2, -1.5)], [(0, -1.0), (1, 4.0), (2, -1.0), (3, 0.5)], [(2, 1.0)], [(3, 1.0)]],
            [[1, 2], [0, 2, 3], [], []], [F, F, C_, C_]),
        # (0, 3) is not in S_0 but 3 is in C_0 through point 1: it goes to ahat[3]; (0, 4) is weak and
        # 4 is not in C_0: it goes to d.  Row 0 is stored out of column order.
        "weak_in_pattern": _case(
            [[(3, -0.125), (1, -2.0), (0, 4.0), (4, -0.0625)], [(1, 4.0), (0, -1.0), (2, -1.5), (3, -1.0)], [(2, 1.0)],
             [(3, 1.0)], [(4, 1.0)]],
            [[1], [2, 3], [], [], []], [F, F, C_, C_, C_]),
        # the strong F neighbour has an entry (1, 0): f * a_10 lands in d
        "plus_i": _case(
            [[(0, 3.0), (1, -1.0), (2, -1.0)], [(0, -0.75), (1, 3.0), (2, -1.5)], [(2, 1.0)]],
            [[1, 2], [0, 2], []], [F, F, C_]),
        # the same without the entry (1, 0): all of a_01 goes through (1, 2)
        "nonsym_no_aki": _case(
            [[(0, 3.0), (1, -1.0), (2, -1.0)], [(1, 3.0), (2, -1.5)], [(2, 1.0)]],
            [[1, 2], [2], []], [F, F, C_]),
    }


_cache = {}


def all_cases(quiet):
    """The cases of interp_std_cases.all_cases and the hand-built ones above, computed once."""
    if not _cache:
        _cache.update(K.all_cases(quiet))
        _cache.update(hand_cases())
    return _cache
