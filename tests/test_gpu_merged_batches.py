"""GPU tests of the merged-group kernels at the batch edges of the LDS form (merged_sums_lds).

A wave of ts_stage0 / ts_inner / spmv_merged takes its share of a group's entries in batches of up to
U chunks of 64 (U = 6 with two segments, 8 with one), each chunk count with its own straight-line
code, then reduces its accumulators by a tree read out of LDS.  The hierarchies of the other merged
tests hold whatever shares their stencils give; the matrix here is built so that the per-wave shares
take every value at which that code changes path:

    0 (a group shorter than W), 1, 63, 64, 65, 64 U - 1, 64 U, 64 U + 1, 64 (U + 1), 2 * 64 U - 1,
    2 * 64 U + 1

for the two-segment copies (U = 6: the [N | L] copies ts_stage0 reads) and for the one-segment
copies (U = 8: the L copies ts_inner reads and the level matrix spmv_merged reads), for every
G in {4, 8} and W in {1, 2, 4}.  The shares are recomputed here from the matrix and its C/F marks in
the way the engine forms its groups (G consecutive rows of the class-contiguous order, W consecutive
shares of ceil(len / W) entries), and every test first asserts that each value occurs; it fails,
never skips, if one does not.

The matrix (level 0 of a hierarchy): rows [0, n0) are a 1-D chain of strong couplings (-1 to
i - 1 and i + 1), which the coarsening splits into alternating F (even) and C (odd) rows; rows
[n0, n) have no strong coupling and become F rows.  Every other off-diagonal is positive, hence
never strong, and only pads the rows: towards same-class lower rows (the L segment) or the other
class (N).  The chain rows carry the one-segment targets in their L counts, the tail rows the
two-segment targets in their row lengths, in groups whose entries are all N, all L, and mixed.  The
F class, and so the level matrix, ends in a partial group.

Checks, each for stage 0 + the inner step (one smoother call per direction, inner = 1), stage 0's
plain C/F-Jacobi counterpart (inner = 0), whole cycles (the residual with its norm, restriction
and prolongation) and the four SpMV ops of spmv_merged on a matrix with the one-segment design's row
lengths (sss_hip_host_spmv_order): the LDS form and the register
form agree as uint64; both agree with the oracle's order within the bounds of the other free-order
tests (test_gpu_free_order.py: 1e-12 relative for a smoother call; whole cycles 1e-10 on the iterate
and 1e-8 on the residual norm); and the forms agree on subnormal products and signed zeros.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A
import oracle
from amg_amd._native import csr_arrays, dptr
from conftest import build_hierarchy

pytestmark = pytest.mark.gpu

GS = (4, 8)
WS = (1, 2, 4)
N0 = 3072            # chain rows: N0 / 2 per class, a multiple of 8
FILL = 1040          # class rows before the first designed block (room for 1025 lower columns)


def _targets(u):
    return (0, 1, 63, 64, 65, 64 * u - 1, 64 * u, 64 * u + 1, 64 * (u + 1), 2 * 64 * u - 1, 2 * 64 * u + 1)


def _group_totals(u):
    """group lengths W * s whose first share is the target s, for every W"""
    return sorted({w * s for w in WS for s in _targets(u) if s > 0})


def _spread(total, rows):
    return [total // rows + (1 if r < total % rows else 0) for r in range(rows)]


def _design():
    """(per chain class row: L count), (per tail row: (N count, L count))"""
    chain_l = [q % 3 for q in range(FILL)]
    for tot in _group_totals(8):   # one-segment targets: a group of 4, an empty group, a group of 8
        chain_l += _spread(tot, 4) + [0] * 4 + _spread(tot, 8)
    assert len(chain_l) <= N0 // 2, len(chain_l)
    chain_l += [q % 5 for q in range(N0 // 2 - len(chain_l))]
    tail = []
    for k, tot in enumerate(_group_totals(6)):   # two-segment targets: groups of 4 rows, all N / all L / mixed
        for r in _spread(tot, 4):
            tail.append((r, 0) if k % 3 == 0 else (0, r) if k % 3 == 1 else (r - r // 2, r // 2))
    tail += [(0, 0)] * 4          # an empty group
    tail += [(2, 1)] * 5          # the F class and the level matrix end in a partial group
    return chain_l, tail


@pytest.fixture(scope="module")
def edge_matrix():
    chain_l, tail = _design()
    n = N0 + len(tail)
    rp, ci, v = [0], [], []
    for i in range(n):
        row = {}
        if i < N0:
            q = i // 2
            if i > 0:
                row[i - 1] = -1.0
            if i + 1 < N0:
                row[i + 1] = -1.0
            lower = [i - 2 * t for t in range(1, chain_l[q] + 1)]              # same class, below
            other = [c for c in (i + 3, i - 3, i + 5) if 0 <= c < N0][: 1 + q % 3]
        else:
            nn, nl = tail[i - N0]
            lower = list(range(i - 1, N0 - 1, -1)) + list(range(N0 - 2, -1, -2))   # F rows below
            lower = lower[:nl]
            other = list(range(N0 - 1, 0, -2))[:nn]                                 # C rows
        assert all(c >= 0 for c in lower)
        for t, c in enumerate(lower + other):
            row[c] = 0.02 + 0.001 * ((5 * i + 11 * t) % 160)
        row[i] = 1.0 + sum(abs(x) for x in row.values())
        for c in sorted(row):
            ci.append(c)
            v.append(row[c])
        rp.append(len(ci))
    return A.NumpyCSR(rp, ci, v)


@pytest.fixture(scope="module")
def edge_h(edge_matrix, quiet):
    return build_hierarchy(edge_matrix.mat, quiet)


def _copies(H):
    """Row lengths of the merged copies of level 0 in the engine's row order (F rows first, then C,
    each in ascending order): the level matrix, and per class the [N | L] copy with its L counts and
    the L copy."""
    L = H.level(0)
    rp, ci, _ = csr_arrays(L.A)
    n = len(rp) - 1
    mark = np.ctypeslib.as_array(L.cfmark.d, shape=(n,)).copy()
    is_c = mark == 1
    assert not is_c[0:N0:2].any() and is_c[1:N0:2].all() and not is_c[N0:].any(), "the C/F split is not the designed one"
    perm = np.concatenate([np.flatnonzero(~is_c), np.flatnonzero(is_c)])
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    row = np.repeat(np.arange(n), np.diff(rp))
    off = ci != row
    same_lower = off & (is_c[ci] == is_c[row]) & (inv[ci] < inv[row])
    a_len = np.diff(rp)[perm]
    nl_len = np.bincount(row[off], minlength=n)[perm]
    l_len = np.bincount(row[same_lower], minlength=n)[perm]
    nf = int((~is_c).sum())
    return a_len, [(nl_len[:nf], l_len[:nf]), (nl_len[nf:], l_len[nf:])]


def _shares(lens, g, w):
    """the per-wave shares of the groups of g rows, as merged_block cuts them"""
    n = len(lens)
    cs = np.concatenate([[0], np.cumsum(lens)])
    glen = cs[np.minimum(np.arange(g, n + g, g), n)] - cs[np.arange(0, n, g)]
    per = (glen + w - 1) // w
    out = [np.minimum(glen, (p + 1) * per) - np.minimum(glen, p * per) for p in range(w)]
    return glen, np.concatenate(out)


def _assert_edges(H, g, w):
    a_len, classes = _copies(H)
    two, one = [], [_shares(a_len, g, w)[1]]
    kinds = set()
    for nl_len, l_len in classes:
        glen, sh = _shares(nl_len, 4, w)          # two segments: the engine caps G at 4
        two.append(sh)
        gl = _shares(l_len, 4, w)[0]
        kinds |= {"N"} if ((glen > 0) & (gl == 0)).any() else set()
        kinds |= {"L"} if ((glen > 0) & (gl == glen)).any() else set()
        kinds |= {"mixed"} if ((gl > 0) & (gl < glen)).any() else set()
        if l_len.sum() >= len(l_len):             # the L copy is on merged groups (free-order threshold 1)
            one.append(_shares(l_len, g, w)[1])
    assert kinds == {"N", "L", "mixed"}, kinds
    assert len(a_len) % g and len(classes[0][0]) % 4, "no partial last group"
    missing2 = set(_targets(6)) - set(np.concatenate(two).tolist())
    missing1 = set(_targets(8)) - set(np.concatenate(one).tolist())
    assert not missing2 and not missing1, (sorted(missing2), sorted(missing1))


@pytest.fixture(params=[(g, w) for g in GS for w in WS], ids=lambda p: f"G{p[0]}W{p[1]}")
def merged(request, monkeypatch):
    g, w = request.param
    monkeypatch.setenv("SSS_HIP_WAVE_MIN", "1")
    monkeypatch.setenv("SSS_HIP_FREE_MIN", "1")
    monkeypatch.setenv("SSS_HIP_MERGE_MIN_ROWS", "1")
    monkeypatch.setenv("SSS_HIP_MERGE_G", str(g))
    monkeypatch.setenv("SSS_HIP_MERGE_W", str(w))
    return g, w


def _both_forms(monkeypatch, run):
    out = []
    for acc in ("0", "1"):
        monkeypatch.setenv("SSS_HIP_MERGE_ACC", acc)
        out.append(run())
    return out


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                          np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _smooth0(H, inner, data):
    """(b, x0, x) of one pre and one post smoother call on level 0"""
    D = A.DeviceHierarchy(H, smoother="jacobi", coarse="direct", relabel=1, inner=inner, inner_from=0, sum_order=1)
    out = []
    try:
        assert D.level_info(0).a_format & 8   # merged copies
        n = H.level(0).A.num_rows
        for post in (False, True):
            b, x0 = data(n)
            D.upload(0, "b", b)
            D.upload(0, "x", x0)
            D.smooth(0, post)
            out.append((b, x0, D.download(0, "x")))
    finally:
        D.close()
    return out


@pytest.mark.parametrize("inner", [1, 0])
def test_smoother_forms_and_oracle(edge_h, monkeypatch, merged, inner):
    """ts_stage0 + ts_inner (inner = 1) and the C/F-Jacobi passes (inner = 0) on level 0."""
    H = edge_h
    _assert_edges(H, *merged)

    def run():
        rng = np.random.default_rng(41)
        return _smooth0(H, inner, lambda n: (rng.standard_normal(n), rng.standard_normal(n)))

    reg, lds = _both_forms(monkeypatch, run)
    ora = oracle.load()
    L = H.level(0)
    for k, ((b, x0, xr), (_, _, xl)) in enumerate(zip(reg, lds)):
        assert np.isfinite(xr).all() and np.any(xr != 0.0)
        assert _same_bits(xr, xl), "post" if k else "pre"
        xo = x0.copy()
        sweeps = H.pars.post_iter if k else H.pars.pre_iter
        if inner > 0:
            ora.ora_cf_twostage(dptr(xo), C.byref(L.A), dptr(b), sweeps, L.cfmark.d, inner)
        else:
            ora.ora_cf_jacobi(dptr(xo), C.byref(L.A), dptr(b), sweeps, L.cfmark.d)
        err = np.linalg.norm(xl - xo) / np.linalg.norm(xo)
        print(f"inner {inner} {'post' if k else 'pre'}: relative distance to the oracle {err:.3e}")
        assert err <= 1e-12, (k, err)


def test_cycle_forms_and_stored_order(edge_h, monkeypatch, merged):
    """Whole cycles: the residual (with and without its norm), restriction and prolongation
    products of spmv_merged on every level.  The two forms agree bitwise; against the stored
    summation order (the oracle's, bitwise, by the parity tests) they are held to the bounds of
    test_free_order_solve_matches_stored_order: the iterate within 1e-10 relative, the residual
    norm within 1e-8 relative.  (r = b - A x cancels to ~1e-4 of its terms after two cycles, so
    its norm does not carry the 1e-12 of a single smoother call.)"""
    H = edge_h
    _assert_edges(H, *merged)
    n = H.level(0).A.num_rows

    def run(sum_order=1):
        D = A.DeviceHierarchy(H, smoother="hybrid", coarse="direct", sum_order=sum_order)
        try:
            assert not sum_order or D.level_info(0).a_format & 8
            D.upload(0, "b", np.ones(n))
            D.upload(0, "x", np.ones(n))
            for _ in range(2):
                D.cycle()
            return D.download(0, "x"), D.residual_norm()
        finally:
            D.close()

    (x_reg, r_reg), (x_lds, r_lds) = _both_forms(monkeypatch, run)
    assert np.isfinite(r_reg) and r_reg > 0.0
    assert _same_bits(x_reg, x_lds)
    assert _same_bits([r_reg], [r_lds])
    x_s, r_s = run(0)
    print(f"residual norm {r_lds:.17g}, stored order {r_s:.17g}; "
          f"iterate distance {np.linalg.norm(x_lds - x_s) / np.linalg.norm(x_s):.3e}")
    assert np.linalg.norm(x_lds - x_s) <= 1e-10 * np.linalg.norm(x_s)
    assert np.isclose(r_lds, r_s, rtol=1e-8, atol=0)


@pytest.fixture(scope="module")
def share_matrix():
    """A square matrix without diagonal whose row q holds the one-segment design's count of entries
    (columns q - 1, q - 2, ...): its groups of G rows in stored order are the chain classes' L copies,
    plus an empty group and a partial last group."""
    lens = _design()[0] + [0] * 8 + [3] * 5
    n = len(lens)
    rp, ci, v = [0], [], []
    for q, m in enumerate(lens):
        for c in range(q - m, q):
            ci.append(c)
            v.append((-1.0) ** c * (0.25 + 0.001 * ((7 * q + 3 * c) % 500)))
        rp.append(len(ci))
    return A.NumpyCSR(rp, ci, v), np.array(lens)


def test_spmv_ops_forms_and_oracle(share_matrix, monkeypatch, merged):
    """The four SpMV ops of spmv_merged (sss_hip_host_spmv_order, free order): the two forms
    bitwise, and within 1e-12 relative of the oracle's product."""
    M, lens = share_matrix
    g, w = merged
    n = len(lens)
    assert n % g
    missing = set(_targets(8)) - set(_shares(lens, g, w)[1].tolist())
    assert not missing, sorted(missing)
    ora = oracle.load()
    lib = A.lib()
    rng = np.random.default_rng(44)
    for op in ("mxy", "amxpy", "resid", "acc"):
        x, b, y0 = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
        alpha = -1.0 if op in ("resid", "amxpy") else 1.0
        cap = 1000 if op == "acc" else 0

        def run():
            y = y0.copy()
            assert lib.sss_hip_host_spmv_order(A.SPMV[op], alpha, C.byref(M.mat), dptr(x), dptr(b), dptr(y), cap, 1) == 0
            return y

        y_reg, y_lds = _both_forms(monkeypatch, run)
        assert _same_bits(y_reg, y_lds), op
        y_ref = y0.copy()
        if op == "mxy":
            ora.ora_mv_mxy(C.byref(M.mat), dptr(x), dptr(y_ref))
        elif op == "amxpy":
            ora.ora_mv_amxpy(alpha, C.byref(M.mat), dptr(x), dptr(y_ref), 0)
        elif op == "resid":
            y_ref[:] = b
            ora.ora_mv_amxpy(-1.0, C.byref(M.mat), dptr(x), dptr(y_ref), 0)
        else:
            ora.ora_mv_acc(C.byref(M.mat), dptr(x), dptr(y_ref), cap)
        assert not _same_bits(y_lds, y0)
        err = np.linalg.norm(y_lds - y_ref) / np.linalg.norm(y_ref)
        print(f"{op}: relative distance to the oracle {err:.3e}")
        assert err <= 1e-12, (op, err)


def test_subnormal_and_signed_zero(edge_h, monkeypatch, merged):
    """b and x0 scaled by 2^-1040: every product and partial sum is subnormal; then x0 = 0 with
    -0.0 entries in b: every product is a signed zero."""
    H = edge_h
    _assert_edges(H, *merged)
    scale = 2.0 ** -1040

    def tiny():
        rng = np.random.default_rng(42)
        return _smooth0(H, 1, lambda n: (scale * rng.standard_normal(n), scale * rng.standard_normal(n)))

    def zeros():
        rng = np.random.default_rng(43)

        def data(n):
            b = rng.standard_normal(n)
            b[rng.random(n) < 0.5] = -0.0
            return b, np.zeros(n)
        return _smooth0(H, 1, data)

    reg, lds = _both_forms(monkeypatch, tiny)
    for (_, _, xr), (_, _, xl) in zip(reg, lds):
        assert np.any(xr != 0.0) and np.abs(xr).max() < 2.0 ** -1022   # subnormal results, not flushed
        assert _same_bits(xr, xl)
    reg, lds = _both_forms(monkeypatch, zeros)
    for (_, _, xr), (_, _, xl) in zip(reg, lds):
        assert _same_bits(xr, xl)
