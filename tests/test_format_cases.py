"""CPU: every case of format_cases.py sits where it claims to sit.

The cases are built around the limits of the storage formats; test_gpu_format_edges.py runs the
kernels on them.  Here each quantity a case declares in `edge` is recomputed in numpy from its CSR,
over the row blocks it declares, and must be exactly on the limit, or one past it: an edit to a
generator cannot move a case off its edge without a failure here.
"""
from __future__ import annotations

import numpy as np
import pytest

import format_cases as F
from amg_amd import _native as N


def _rows(c, r0, r1):
    """(row index, column, value bits) of the entries of rows [r0, r1)"""
    rp = c.rp
    k0, k1 = int(rp[r0]), int(rp[r1])
    row = np.repeat(np.arange(r0, r1), np.diff(rp[r0:r1 + 1]))
    return row, c.ci[k0:k1].astype(np.int64), F.bits(c.v[k0:k1])


def _offsets(c, r0, r1, based=False):
    row, col, _ = _rows(c, r0, r1)
    if based:   # against the row's first column
        first = np.array([c.ci[c.rp[r]] if c.rp[r] < c.rp[r + 1] else 0 for r in range(r0, r1)], dtype=np.int64)
        return np.unique(col - first[row - r0])
    return np.unique(col - row)


def _values(c, r0, r1):
    return np.unique(_rows(c, r0, r1)[2])


def test_constants_are_the_librarys():
    assert (F.ENC_SORTED, F.ENC_DICT, F.ENC_MERGED_ONLY, F.ENC_XELL, F.ENC_ELL, F.ENC_ELL_BASE) == \
        (N.ENC_SORTED_TILES, N.ENC_DICT, N.ENC_MERGED_ONLY, N.ENC_XELL, N.ENC_ELL, N.ENC_ELL_BASE)
    assert (F.FMT_SORTED, F.FMT_DICT, F.FMT_ELL, F.FMT_XELL) == (N.FMT_SORTED, N.FMT_DICT, N.FMT_ELL, N.FMT_XELL)


def test_the_table_is_complete():
    """one case per row of the table: every width, every pair shape, both sides of every limit"""
    want = {"ell8_full", "ell8_over_off", "ell8_over_val", "ell16_exact", "ell16_plus1", "ell32_exact", "ell32_plus1",
            "ell_based_R", "xell_w8", "xell_w16", "xell_w20", "xell_w24", "xell_w32", "xell_w40", "xell_sparse",
            "xell_halved", "xell_halved_w40_refused", "xell_shift24", "dtile_full", "dtile_over_off", "dtile_over_val",
            "vdict_full", "vdict_over", "sorted_span", "sorted_span_over", "xell_w32_plus1_refused"}
    want |= {f"ell8_pairs_{n}_{nF}" for n, nF in [(511, 255), (512, 255), (513, 1), (513, 512), (300, 150), (769, 257)]}
    want |= {f"xell_w{W}_plus1" for W in (8, 16, 20, 24)}
    assert set(F.NAMES) == want
    assert sorted(sum(F.GROUPS.values(), [])) == sorted(F.NAMES)


@pytest.mark.parametrize("name", F.NAMES)
def test_case_is_well_formed(name):
    c = F.case(name)
    n = c.n
    assert 300 <= n <= 1400
    assert c.rp[0] == 0 and np.all(np.diff(c.rp) >= 0) and c.rp[n] == len(c.ci) == len(c.v)
    assert c.ci.min() >= 0 and c.ci.max() < c.ncols
    assert np.isfinite(c.v).all()
    if c.square:
        assert 0 < c.nF < n
    else:
        assert c.nF == -1 and not c.kinds
        assert 8e6 <= 8 * c.ncols <= 70e6 or c.ncols < 4000   # the wide x vectors: 8 to 70 MB
    # the declared blocks tile the rows, cut at the class split, and are the first variant's
    assert c.blocks[0][0] == 0 and c.blocks[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(c.blocks, c.blocks[1:]))
    assert all(0 < r1 - r0 <= F.K_BLOCK for r0, r1 in c.blocks)
    if c.nF > 0:
        assert any(r0 == c.nF for r0, _ in c.blocks)
    want = c.variants[0][1]
    assert want["nblk"] == len(c.blocks) and want["split_blk"] == F.split_blk_of(c.blocks, c.nF)
    # the planted values: +0.0, -0.0 and the subnormal by bit pattern; 2^30, then later in the same
    # row -2^30 on the same column
    r = c.special_row
    _, col, vb = _rows(c, r, r + 1)
    for a in (F.PZERO, F.NZERO, F.SUBNORMAL):
        assert F.bits([a])[0] in vb, a
    kb, kn = np.flatnonzero(vb == F.bits([F.BIG])[0]), np.flatnonzero(vb == F.bits([F.NBIG])[0])
    assert len(kb) == 1 and len(kn) == 1 and kb[0] < kn[0] and col[kb[0]] == col[kn[0]]
    assert np.count_nonzero(F.bits(c.v) == 0) == 1 and np.count_nonzero(F.bits(c.v) == 1 << 63) == 1
    assert 0.0 < F.SUBNORMAL < np.finfo(np.float64).tiny
    # smoothing cases: at most one diagonal entry per row, 1e-30 on two or three of them (one where the
    # class that takes them is a single row)
    if c.kinds:
        row, col, _ = _rows(c, 0, n)
        assert np.bincount(row[col == row], minlength=n).max() == 1
        tiny = np.flatnonzero((c.v == F.TINY_DIAG))
        assert np.array_equal(np.sort(row[tiny]), np.array(c.tiny_rows)) and np.all(col[tiny] == row[tiny])
        assert len(c.tiny_rows) in (2, 3) or (len(c.tiny_rows) == 1 and n - c.nF == 1)
        assert set(c.split_copies) == {k for k in N.PLAN_INFO_FIELDS if k[:3] in ("nl_", "lo_")}


def _ell_width(longest):
    return 8 if longest <= 8 else 16 if longest <= 16 else 32 if longest <= 32 else 0


@pytest.mark.parametrize("name", F.NAMES)
def test_case_sits_on_its_edge(name):
    c = F.case(name)
    e = dict(c.edge)
    n, nnz = c.n, len(c.v)
    lens = np.diff(c.rp)
    longest = int(lens.max())
    first = c.variants[0][1]
    if "n" in e:
        assert (e.pop("n"), e.pop("nF")) == (n, c.nF)
    if "longest_row" in e:
        assert longest == e.pop("longest_row")
    if "W" in e:   # the width the first variant must report, from the longest row
        W = e.pop("W")
        if first["a_format"] & F.FMT_ELL:
            assert W == _ell_width(longest) == first["ell_w"]
        elif first["a_format"] & F.FMT_XELL:
            assert W == F.xell_width(longest) == first["xell_w"]
        else:
            assert W == 0 and first["ell_w"] == first["xell_w"] == 0
    blk = e.pop("block", None)
    if "offsets" in e:
        assert len(_offsets(c, *blk)) == e.pop("offsets")
    if "values" in e:
        assert len(_values(c, *blk)) == e.pop("values")
    if "offsets_gt" in e:
        assert len(_offsets(c, *blk)) > e.pop("offsets_gt")
    if "max_offsets_le" in e:   # every block of a dictionary ELL within its dictionaries
        lim = e.pop("max_offsets_le")
        assert max(len(_offsets(c, *b)) for b in c.blocks) <= lim
    if "max_values_le" in e:
        lim = e.pop("max_values_le")
        assert max(len(_values(c, *b)) for b in c.blocks) <= lim
    if e.pop("code_fe", False):   # the largest bit pattern on the largest offset: value 7, offset 30
        row, col, vb = _rows(c, *blk)
        assert np.any((vb == vb.max()) & (col - row == (col - row).max()))
    if e.pop("full_rows", False):
        assert np.count_nonzero(lens == 8) > 0 and longest == 8
    if "empty_row" in e:
        assert lens[e.pop("empty_row")] == 0
    if e.pop("independent", False):   # no entry couples two rows of a class
        row, col, _ = _rows(c, 0, n)
        off = col != row
        assert not np.any((row[off] < c.nF) == (col[off] < c.nF))
    if "based_offsets_le" in e:
        lim = e.pop("based_offsets_le")
        assert max(len(_offsets(c, *b, based=True)) for b in c.blocks) <= lim
        assert max(len(_offsets(c, *b)) for b in c.blocks) > e.pop("plain_offsets_gt")
    if "values_gt" in e:   # more values than a dictionary ELL holds, in some block of its blocking
        lim = e.pop("values_gt")
        assert max(len(_values(c, *b)) for b in F.tile_blocks(c.rp, c.nF)) > lim
    if "dense" in e:   # rows padded to 8 codes against 12 bytes per entry
        W8 = F.xell_width(longest)
        assert (nnz * 3 >= W8 * n) == e.pop("dense")
    if e.pop("all_distinct", False):   # but for the 1e-30 diagonals, which share one
        assert len(np.unique(F.bits(c.v))) == nnz - (len(c.tiny_rows) - 1)
        per16 = e.pop("rows16_values")
        assert len(_values(c, 0, 16)) == per16 and (per16 <= F.XELL_VALUES) == bool(first["a_format"] & F.FMT_XELL)
        assert len(_values(c, 0, 17)) > F.XELL_VALUES
    if "nblk" in e:
        assert first["nblk"] == e.pop("nblk")
        sizes = [r1 - r0 for r0, r1 in c.blocks]
        assert sizes[:16] == [16] * 16 and sorted(set(sizes[16:])) == [12, 13]
    if "shift" in e:
        S = e.pop("shift")
        assert (1 << (S - 1)) <= c.ncols < (1 << S) and first["xell_shift"] == S
        assert len(_values(c, *blk)) == 1 << (32 - S)
    if e.pop("top_code", False):   # the highest value index on the highest legal column
        row, col, vb = _rows(c, *blk)
        assert np.any((vb == vb.max()) & (col == c.ncols - 1)) and c.ncols - 1 < (1 << first["xell_shift"]) - 1
    if e.pop("rows_41_60", False):
        assert lens.min() == 41 and lens.max() == 60
    if "span" in e:   # the block's columns from `cut` on: one cluster, and the gap below it the widest
        span, cut = e.pop("span"), e.pop("cut")
        _, col, _ = _rows(c, *blk)
        cs = np.unique(col)
        hi, lo = cs[cs >= cut], cs[cs < cut]
        assert hi[-1] - hi[0] == span and span in (F.TILE_DIAG_MARK - 1, F.TILE_DIAG_MARK)
        assert hi[0] - lo[-1] > max(np.diff(hi).max(), np.diff(lo).max()) and lo[-1] - lo[0] < F.TILE_DIAG_MARK
        assert (span < F.TILE_DIAG_MARK) == bool(first["a_format"] & F.FMT_SORTED)
    if e.pop("c_eq_r", False):
        row, col, _ = _rows(c, 0, n)
        assert not c.square and np.count_nonzero(row == col) == n
    assert not e, e   # every declared quantity was looked at


@pytest.mark.parametrize("over,full", [("ell8_over_off", "ell8_full"), ("ell8_over_val", "ell8_full"),
                                       ("dtile_over_off", "dtile_full"), ("dtile_over_val", "dtile_full"),
                                       ("vdict_over", "vdict_full"), ("sorted_span_over", "sorted_span")])
def test_twins_differ_in_one_entry(over, full):
    """a case one past a limit is its twin on the limit with a single entry moved or revalued"""
    a, b = F.case(over), F.case(full)
    assert np.array_equal(a.rp, b.rp)
    assert np.count_nonzero((a.ci != b.ci) | (F.bits(a.v) != F.bits(b.v))) == 1


def test_expected_formats_follow_the_limits():
    """what the cases expect of an upload, against the limits stated in their names"""
    for name in F.NAMES:
        c = F.case(name)
        fmt = c.variants[0][1]["a_format"]
        assert bool(fmt & F.FMT_ELL) == (name.startswith("ell") and "over" not in name and name != "ell32_plus1"), name
        if name.startswith("xell"):
            assert bool(fmt & F.FMT_XELL) == ("refused" not in name and name != "xell_sparse"), name
    assert F.case("ell16_plus1").variants[0][1]["ell_w"] == 32
    assert [F.case(f"xell_w{W}_plus1").variants[0][1]["xell_w"] for W in (8, 16, 20, 24)] == [16, 20, 24, 32]
    assert F.case("xell_w40").variants[1][1]["a_format"] & F.FMT_XELL == 0       # without ENC_MERGED_ONLY
    assert F.case("ell_based_R").variants[1][1]["a_format"] & F.FMT_ELL == 0     # without ENC_ELL_BASE
    assert F.case("dtile_full").variants[0][1]["a_format"] == F.FMT_DICT
    assert F.case("vdict_full").variants[0][1]["a_format"] == F.FMT_DICT | F.FMT_SORTED
    assert F.case("vdict_over").variants[0][1]["a_format"] == F.FMT_SORTED
    assert F.case("sorted_span_over").variants[0][1]["a_format"] == 0
