"""Matrices that sit on the limits of the storage formats: pure numpy, no GPU.

Every level of the cycle is read through a storage format with hard limits: the dictionary ELL holds
31 column offsets and 8 values per row block in rows of 8, 16 or 32 one-byte codes (0xFF pads); the
column ELL 512 or 2^(32 - S) values per block (blocks halved until their values fit) in rows of 8 to
40 codes (0xFFFFFFFF pads); the dictionary tiles 256 offsets and 256 values per block; the sorted
tiles two column clusters per block, each spanning less than 2^20 - 256 columns, with the diagonal
mark just above.  The hierarchies of the other tests produce whatever fills their stencils happen to
give.  The cases here are built so that one declared block sits exactly on a limit, or one past it.

A case gives its CSR, the class split nF (square cases: rows [0, nF) are class F), the encodings to
upload it with and what each must choose (the fields of sss_hip_store_info), the row blocks of its
first encoding's format, and `edge`: the quantities it was designed around, which
test_format_cases.py recomputes from the CSR.  test_gpu_format_edges.py runs the kernels on them.

Values are chosen by bit pattern.  Every case plants, in one row, +0.0 and -0.0 (two dictionary values),
the largest subnormal, and 2^30 followed later in the row by -2^30 on the same column: the two products
cancel exactly, and what is summed between them loses its low bits, so a kernel that adds a row in
another order than the stored one gives other bits.  The smoothing cases store 1e-30 on the diagonal
of two or three rows, which every smoother leaves as they are (|d| <= 1e-20).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# SSS_HIP_ENC_* (include/sss_hip.h) and the a_format bits of sss_hip_store_info
ENC_SORTED, ENC_DICT, ENC_MERGED_ONLY, ENC_XELL, ENC_ELL, ENC_ELL_BASE = 1, 4, 8, 16, 32, 64
FMT_SORTED, FMT_DICT, FMT_ELL, FMT_XELL = 1, 2, 64, 128
#: what a level matrix is offered (level_encoding), a transfer operator, a restriction
ENC_LEVEL = ENC_SORTED | ENC_DICT | ENC_XELL
ENC_TRANSFER = ENC_SORTED | ENC_XELL
ENC_RESTRICT = ENC_TRANSFER | ENC_ELL_BASE

K_BLOCK = 256                       # rows of a row block at most
TILE_ENTRIES = 2048                 # entries of a CSR-adaptive row block at most (unless one long row)
TILE_DIAG_MARK = (1 << 20) - 256    # a sorted-tile cluster spans fewer columns than this
ELL_OFFSETS, ELL_VALUES = 31, 8
TILE_DICT = 256
XELL_VALUES = 512
XELL_WIDTHS = (8, 16, 20, 24, 32, 40)


def f64(bits: int) -> float:
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


PZERO, NZERO = f64(0), f64(1 << 63)
SUBNORMAL = f64(0x000FFFFFFFFFFFFF)
BIG, NBIG = f64(0x41D0000000000000), f64(0xC1D0000000000000)   # +-2^30
TINY_DIAG = 1e-30
SPECIALS = (PZERO, NZERO, SUBNORMAL, BIG, NBIG)


def regular(k: int) -> float:
    """The k-th regular off-diagonal value, -(1 + k / 1024): distinct bit patterns, all below -2^30's"""
    return -(1.0 + k / 1024.0)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- the blockings, restated
def tile_blocks(rp, split=-1):
    """CSR-adaptive row blocks: at most 256 rows and 2048 entries (a longer row alone), cut at split"""
    n = len(rp) - 1
    out, r = [], 0
    while r < n:
        lim = split if r < split < n else n
        e = r + 1
        if rp[e] - rp[r] <= TILE_ENTRIES:
            while e < lim and e - r < K_BLOCK and rp[e + 1] - rp[r] <= TILE_ENTRIES:
                e += 1
        out.append((r, e))
        r = e
    return out


def row_chunks(n, split=-1):
    """256-row chunks cut at split: the column ELL's blocks before any halving"""
    out, r = [], 0
    while r < n:
        lim = split if r < split < n else n
        out.append((r, min(lim, r + K_BLOCK)))
        r = out[-1][1]
    return out


def xell_shift(ncols: int) -> int:
    for s in range(23, 29):
        if ncols < (1 << s):
            return s
    return 0


def xell_width(longest: int) -> int:
    for w in XELL_WIDTHS:
        if longest <= w:
            return w
    return 0


def xell_blocks(rp, v, split, vcap):
    """The column ELL's blocks: each chunk halved until its distinct values fit vcap; None when a part
    of 16 rows or fewer still does not fit"""
    out = []

    def fit(r0, r1):
        if len(np.unique(bits(v[rp[r0]:rp[r1]]))) <= vcap:
            out.append((r0, r1))
            return True
        if r1 - r0 <= 16:
            return False
        mid = r0 + (r1 - r0) // 2
        return fit(r0, mid) and fit(mid, r1)

    for r0, r1 in row_chunks(len(rp) - 1, split):
        if not fit(r0, r1):
            return None
    return out


def split_blk_of(blocks, split):
    if split < 0:
        return len(blocks)
    return next((q for q, (r0, _) in enumerate(blocks) if r0 >= split), len(blocks))


def xell_choice(rp, v, ncols, split, enc):
    """(W, S, blocks) of the column ELL an upload with `enc` takes for these rows, or None"""
    n = len(rp) - 1
    S = xell_shift(ncols)
    nnz = int(rp[n])
    if not (enc & ENC_XELL) or nnz == 0 or S == 0:
        return None
    W = xell_width(int(np.max(np.diff(rp))))
    if W == 0 or nnz * 3 < W * n or (W == 40 and not enc & ENC_MERGED_ONLY):
        return None
    blocks = xell_blocks(rp, v, split, min(XELL_VALUES, 1 << (32 - S)))
    return None if blocks is None else (W, S, blocks)


def two_stage_rows(rp, ci, v, lo, hi):
    """The two-stage copies of the class pass over rows [lo, hi): (rp, v) of the [N | L] rows and of
    the L rows (L: same class, column < row; N: the other off-diagonals; both in stored order)"""
    nrp, nv, lrp, lv = [0], [], [0], []
    for i in range(lo, hi):
        c, a = ci[rp[i]:rp[i + 1]], v[rp[i]:rp[i + 1]]
        low = (c >= lo) & (c < i)
        nv += list(a[~low & (c != i)]) + list(a[low])
        lv += list(a[low])
        nrp.append(len(nv))
        lrp.append(len(lv))
    return (np.array(nrp), np.array(nv, dtype=np.float64)), (np.array(lrp), np.array(lv, dtype=np.float64))


def split_copy_format(rp, v, ncols, enc):
    """(a_format, xell_w) of a two-stage copy: uploaded without the dictionary formats and with
    ENC_MERGED_ONLY, so it is a column ELL where that qualifies, else sorted or plain tiles"""
    tenc = (enc & ~ENC_DICT) | ENC_MERGED_ONLY
    if int(rp[-1]) == 0:
        return 0, 0
    x = xell_choice(rp, v, ncols, -1, tenc)
    if x:
        return FMT_DICT | FMT_XELL, x[0]
    return (FMT_SORTED if tenc & ENC_SORTED else 0), 0   # (ncols far below a cluster's span here)


# ---------------------------------------------------------------- rows and what is planted in them
def to_csr(rows):
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([c for r in rows for c, _ in r], dtype=np.int32)
    v = np.array([a for r in rows for _, a in r], dtype=np.float64)
    return rp, ci, v


def plant_specials(rows, r, square=True, big_col=None):
    """Row r's off-diagonal slots in stored order: +0.0, -0.0 and the subnormal on the first three that
    are free, 2^30 on the slot of column big_col (default: the fourth), -2^30 on the last one, whose
    column becomes that of 2^30."""
    slots = [s for s, (c, _) in enumerate(rows[r]) if not (square and c == r)]
    assert len(slots) >= 6, (r, len(slots))
    sb = slots[3] if big_col is None else next(s for s in slots if rows[r][s][0] == big_col)
    rest = [s for s in slots if s != sb]
    last = rest[-1]
    assert last > sb, (r, sb, last)
    cb = rows[r][sb][0]
    for s, a in zip(rest[:3], (PZERO, NZERO, SUBNORMAL)):
        rows[r][s] = (rows[r][s][0], a)
    rows[r][sb] = (cb, BIG)
    rows[r][last] = (cb, NBIG)


def plant_tiny(rows, which):
    for r in which:
        s = next(s for s, (c, _) in enumerate(rows[r]) if c == r)
        rows[r][s] = (r, TINY_DIAG)


def rotate(row, k):
    k %= max(len(row), 1)
    return row[k:] + row[:k]


# ---------------------------------------------------------------- the case
@dataclass
class Case:
    name: str
    group: str                     # ell / xell / tile: one GPU test per group
    gen: str                       # bipartite / banded / distinct / rows
    rp: np.ndarray
    ci: np.ndarray
    v: np.ndarray
    ncols: int
    nF: int                        # class split row; -1: none (rectangular cases)
    variants: list                 # [(enc, expected store info)], the first is the case's own
    blocks: list                   # row blocks [(r0, r1)] of the first variant's format
    edge: dict                     # what the case was designed around (test_format_cases.py)
    kinds: tuple = ()              # smoother kinds of the level step: "exact", "jacobi"
    inners: tuple = (0, 1, 2)      # inner steps of the Jacobi level step
    tiny_rows: tuple = ()
    special_row: int = -1
    split_copies: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.rp) - 1

    @property
    def square(self):
        return self.n == self.ncols

    @property
    def enc(self):
        return self.variants[0][0]


def info(fmt, blocks, split, ell_w=0, xell_w=0, shift=0, based=0):
    return dict(a_format=fmt, ell_w=ell_w, xell_w=xell_w, xell_shift=shift, ell_based=based, nblk=len(blocks),
                split_blk=split_blk_of(blocks, split))


def ell_info(rp, split, W, based=0):
    return info(FMT_DICT | FMT_ELL, tile_blocks(rp, split), split, ell_w=W, based=based)


def xell_info(rp, v, ncols, split, enc):
    W, S, blocks = xell_choice(rp, v, ncols, split, enc)
    return info(FMT_DICT | FMT_XELL, blocks, split, xell_w=W, shift=S)


def tile_info(rp, split, fmt):
    return info(fmt, tile_blocks(rp, split), split)


def _split_copies(c: Case):
    """expected (a_format, xell_w) of the four two-stage copies of a square case, keyed as plan_info"""
    out = {}
    for cls, (lo, hi) in (("f", (0, c.nF)), ("c", (c.nF, c.n))):
        (nrp, nv), (lrp, lv) = two_stage_rows(c.rp, c.ci, c.v, lo, hi)
        for key, (rp, v) in (("nl", (nrp, nv)), ("lo", (lrp, lv))):
            fmt, w = split_copy_format(rp, v, c.ncols, c.enc) if hi > lo else (0, 0)
            out[f"{key}_{cls}_format"], out[f"{key}_{cls}_xell_w"] = fmt, w
    return out


def _finish(c: Case) -> Case:
    if c.kinds:
        c.split_copies = _split_copies(c)
    return c


# ---------------------------------------------------------------- generators
BIP_D = (0, 1, 2, 5, 9, 17, 40)   # a bipartite F row i holds columns nF + i + d, the C rows the mirror image


def bipartite_rows(n, nF):
    """F rows: the diagonal and the columns nF + i + d (d in BIP_D) that exist; C row j: the diagonal and
    the columns j - nF - d.  No entry couples two rows of a class.  Per block of 256 rows of a class one
    off-diagonal value and one diagonal value, other values in the next block; the stored order of a row
    is rotated by its index, so the diagonal takes every slot."""
    ds = BIP_D if n - nF > 1 else [-d for d in BIP_D]   # (a C class of one row: the F rows 0, 1, 2, 5, ... reach it)
    rows = []
    for i in range(n):
        q = (i if i < nF else i - nF) // K_BLOCK + (0 if i < nF else 2)
        if i < nF:
            cols = [nF + i + d for d in ds if nF <= nF + i + d < n]
        else:
            cols = [i - nF - d for d in ds if 0 <= i - nF - d < nF]
        row = [(i, 8.0 + q / 4.0)] + [(c, regular(q)) for c in cols]
        rows.append(rotate(row, i))
    return rows


def tri_offsets(noff):
    """noff offsets each way: 1, 3, 6, 10, ... (the banded matrix of test_gpu_parity.py)"""
    t = [k * (k + 1) // 2 for k in range(1, noff + 1)]
    return [-o for o in reversed(t)] + t


def banded_rows(n, offs, nvals=2, diag=64.0):
    """Row i: the diagonal and the columns i + o (o in offs) that exist, in ascending column order;
    off-diagonal values regular((i * 7 + k * 13) % nvals) for the k-th offset."""
    rows = []
    for i in range(n):
        row = [(i + o, regular((i * 7 + k * 13) % nvals)) for k, o in enumerate(offs) if 0 <= i + o < n]
        row.append((i, diag))
        rows.append(sorted(row))
    return rows


def extra_entries(rows, r, count):
    """`count` more entries on row r, each on the column of its first off-diagonal entry (a longer row
    with no new offset)"""
    c = next(c for c, _ in rows[r] if c != r)
    rows[r] += [(c, regular(0))] * count


def _tiny_c_rows(n, nF):
    """rows of class C for the 1e-30 diagonals (the F rows keep theirs, so the F pass still overwrites
    every F row and the pending-F form stays possible): three, or the only one"""
    nC = n - nF
    return tuple(sorted({nF + nC // 4, nF + nC // 2, n - 1}))


# ---------------------------------------------------------------- dictionary ELL cases
def case_ell8_pairs(n, nF):
    rows = bipartite_rows(n, nF)
    # the specials go to a row of the larger class with seven off-diagonal entries (to the one row that
    # has them where a class is a single row)
    big = range(nF) if nF >= n - nF else range(nF, n)
    full = [i for i in big if len(rows[i]) == 8] or [i for i in range(n) if len(rows[i]) == 8]
    sr = full[len(full) // 3]
    plant_specials(rows, sr)
    tiny = _tiny_c_rows(n, nF)
    plant_tiny(rows, tiny)
    rp, ci, v = to_csr(rows)
    blocks = tile_blocks(rp, nF)
    return _finish(Case(f"ell8_pairs_{n}_{nF}", "ell", "bipartite", rp, ci, v, n, nF,
                        [(ENC_LEVEL, ell_info(rp, nF, 8))], blocks,
                        dict(longest_row=8, W=8, max_offsets_le=ELL_OFFSETS, max_values_le=ELL_VALUES, n=n, nF=nF,
                             independent=True),
                        kinds=("exact", "jacobi"), tiny_rows=tiny, special_row=sr))


PAIR_SHAPES = [(511, 255), (512, 255), (513, 1), (513, 512), (300, 150), (769, 257)]

ELL8_POOL = [o for o in range(-15, 16) if o != 0]   # 30 non-zero offsets; with the diagonal: 31


def ell8_rows(n=600):
    """Rows of 8: the diagonal and 7 of the 30 offsets of ELL8_POOL, the window moving by 6 with the
    row index (five row types cover the pool), so every block of interior rows holds exactly 31 offsets.
    One off-diagonal value per row parity and one diagonal value."""
    rows = []
    for i in range(n):
        offs = [ELL8_POOL[(6 * (i % 5) + j) % 30] for j in range(7)]
        row = [(i + o, regular(i % 2)) for o in offs if 0 <= i + o < n] + [(i, 64.0)]
        rows.append(rotate(row, i))
    return rows


def case_ell8(kind, n=600, nF=300):
    """ell8_full: block [0, 256) has exactly 31 offsets and 8 values -- the two regular ones, the
    diagonal's and the five planted -- and -2^30, its largest bit pattern, sits on offset +15, its
    largest offset: code 0xFE.  Row 77 is empty.  over_off: one entry of that block moves to offset
    +16 (32 offsets); over_val: one takes a ninth value."""
    rows = ell8_rows(n)
    # the planted row holds offset +15, and not as its last off-diagonal entry
    sr = next(i for i in range(16, 200) if any(c == i + 15 for c, _ in rows[i]) and len(rows[i]) == 8 and
              [c for c, _ in rows[i] if c != i][-1] != i + 15)
    plant_specials(rows, sr, big_col=sr + 15)
    rows[77] = []
    tiny = (400, 500, 599)   # block [300, 556) and the last one: the first block keeps 8 values
    plant_tiny(rows, tiny)
    if kind == "over_off":
        s = next(s for s, (c, _) in enumerate(rows[40]) if c != 40)
        rows[40][s] = (40 + 16, rows[40][s][1])
    if kind == "over_val":
        s = next(s for s, (c, _) in enumerate(rows[40]) if c != 40)
        rows[40][s] = (rows[40][s][0], regular(2))
    rp, ci, v = to_csr(rows)
    blocks = tile_blocks(rp, nF)
    edge = dict(longest_row=8, block=(0, 256), n=n, nF=nF, empty_row=77)
    if kind == "full":
        variants = [(ENC_LEVEL, ell_info(rp, nF, 8))]
        edge.update(W=8, offsets=ELL_OFFSETS, values=ELL_VALUES, code_fe=True, full_rows=True)
    else:
        # not a dictionary ELL: offered the column ELL it takes that (8 codes per row, far fewer than
        # 512 values); offered the dictionary formats alone, the dictionary tiles
        variants = [(ENC_LEVEL, xell_info(rp, v, n, nF, ENC_LEVEL)),
                    (ENC_SORTED | ENC_DICT, tile_info(rp, nF, FMT_DICT))]
        blocks = xell_choice(rp, v, n, nF, ENC_LEVEL)[2]
        edge.update(offsets=ELL_OFFSETS + (kind == "over_off"), values=ELL_VALUES + (kind == "over_val"))
    return _finish(Case(f"ell8_{kind}", "ell", "rows", rp, ci, v, n, nF, variants, blocks, edge,
                        kinds=("jacobi",), tiny_rows=tiny, special_row=sr))


def case_ell_banded(name, longest, n=600, nF=300):
    """Banded rows of 15 / 30 offsets and the diagonal: 16 / 31 entries, two off-diagonal values.  The
    longest row is the planted one: one more entry on a column it already holds makes it the 32nd of
    ell32_exact (31 offsets are all a block's dictionary holds), and the neighbours' 17th and 33rd."""
    base = 16 if longest <= 17 else 31
    offs = tri_offsets(7) + [40] if base == 16 else [o for o in range(-15, 16) if o != 0]
    rows = banded_rows(n, offs)
    sr = 100
    plant_specials(rows, sr)
    extra_entries(rows, sr, longest - base)
    tiny = (450, 520, 599)
    plant_tiny(rows, tiny)
    rp, ci, v = to_csr(rows)
    edge = dict(longest_row=longest, n=n, nF=nF, max_offsets_le=ELL_OFFSETS, max_values_le=ELL_VALUES)
    if longest <= 32:
        W = 16 if longest <= 16 else 32
        variants = [(ENC_LEVEL, ell_info(rp, nF, W))]
        blocks = tile_blocks(rp, nF)
        edge.update(W=W)
    else:
        # 33 entries: no dictionary ELL; a column ELL of 40 where no range relaxation reads it, else
        # dictionary tiles
        variants = [(ENC_LEVEL, tile_info(rp, nF, FMT_DICT)),
                    (ENC_LEVEL | ENC_MERGED_ONLY, xell_info(rp, v, n, nF, ENC_LEVEL | ENC_MERGED_ONLY))]
        blocks = tile_blocks(rp, nF)
        edge.update(W=0)
    return _finish(Case(name, "ell", "banded", rp, ci, v, n, nF, variants, blocks, edge,
                        kinds=("jacobi",), tiny_rows=tiny, special_row=sr))


def case_ell_based(m=600):
    """A restriction-like 600 x 2,600 matrix: row r holds the columns first(r) + {0, 1, 2, 10, 11, 12,
    100, 101} with first(r) = 3 r + 11 (r mod 7), so col - row takes far more than 31 values in a
    block while col - (first col) takes 8.  Row 300 is empty (its base is 0).  With per-row bases a
    dictionary ELL of width 8; without them (ENC_ELL alone) it must not be one."""
    rel = (0, 1, 2, 10, 11, 12, 100, 101)
    rows = []
    for r in range(m):
        f = 3 * r + 11 * (r % 7)
        rows.append([(f + d, regular((r + k) % 2)) for k, d in enumerate(rel)])
    sr = 50
    plant_specials(rows, sr, square=False)
    rows[300] = []
    rp, ci, v = to_csr(rows)
    ncols = 2600
    assert ci.max() < ncols
    variants = [(ENC_RESTRICT, ell_info(rp, -1, 8, based=1)),
                (ENC_TRANSFER | ENC_ELL, xell_info(rp, v, ncols, -1, ENC_TRANSFER | ENC_ELL))]
    return Case("ell_based_R", "ell", "rows", rp, ci, v, ncols, -1, variants, tile_blocks(rp),
                dict(longest_row=8, W=8, based_offsets_le=ELL_OFFSETS, plain_offsets_gt=ELL_OFFSETS,
                     max_values_le=ELL_VALUES, empty_row=300), special_row=sr)


# ---------------------------------------------------------------- column ELL cases
def case_xell_w(W, extra=0, n=600, nF=300, merged_only=False):
    """Banded rows of W - 1 offsets and the diagonal, 97 off-diagonal values (no 8-value dictionary, so
    no dictionary ELL): a column ELL of exactly W codes per row.  extra = 1: the planted row holds one
    more entry and the matrix takes the next width."""
    half = (W - 1) // 2
    offs = [o for o in range(-half, W - 1 - half + 1) if o != 0]
    assert len(offs) == W - 1
    rows = banded_rows(n, offs, nvals=97)
    sr = 100
    plant_specials(rows, sr)
    extra_entries(rows, sr, extra)
    tiny = (450, 520, 599)
    plant_tiny(rows, tiny)
    rp, ci, v = to_csr(rows)
    enc = ENC_LEVEL | (ENC_MERGED_ONLY if merged_only else 0)
    nxt = xell_width(W + extra)
    edge = dict(longest_row=W + extra, W=nxt, n=n, nF=nF, values_gt=ELL_VALUES, dense=True)
    name = f"xell_w{W}" + ("_plus1" if extra else "")
    if nxt == 40 and not merged_only:
        name += "_refused"
        # rows of 33 to 40 entries without ENC_MERGED_ONLY: no column ELL; dictionary tiles
        variants = [(enc, tile_info(rp, nF, FMT_DICT))]
        blocks = tile_blocks(rp, nF)
        edge.update(W=0)
    else:
        variants = [(enc, xell_info(rp, v, n, nF, enc))]
        blocks = xell_choice(rp, v, n, nF, enc)[2]
        if nxt == 40:   # the same matrix without the flag
            variants.append((ENC_LEVEL, tile_info(rp, nF, FMT_DICT)))
    inners = (1, 2) if nxt == 40 else (0, 1, 2)   # 40 codes per row: no range relaxation reads them
    return _finish(Case(name, "xell", "banded", rp, ci, v, n, nF, variants, blocks, edge,
                        kinds=("jacobi",), inners=inners, tiny_rows=tiny, special_row=sr))


def case_xell_sparse(n=600, nF=300):
    """One row of 8 entries, every other row 2: 3 nnz < 8 n, so the rows padded to 8 codes would be
    larger than the CSR entries and the column ELL is refused.  97 values: no dictionary ELL either;
    dictionary tiles."""
    rows = [[(i, 64.0), ((i + 5) % n, regular(i % 97))] for i in range(n)]
    sr = 100
    rows[sr] = [(sr, 64.0)] + [(sr + o, regular(o)) for o in (1, 2, 3, 4, 6, 7, 8)]
    plant_specials(rows, sr)
    tiny = (450, 520, 599)
    plant_tiny(rows, tiny)
    rp, ci, v = to_csr(rows)
    return _finish(Case("xell_sparse", "xell", "rows", rp, ci, v, n, nF, [(ENC_LEVEL, tile_info(rp, nF, FMT_DICT))],
                        tile_blocks(rp, nF), dict(longest_row=8, W=0, n=n, nF=nF, dense=False, values_gt=ELL_VALUES),
                        kinds=("jacobi",), tiny_rows=tiny, special_row=sr))


def distinct_rows(n, per_row, seed):
    """Every row `per_row` entries -- the diagonal and the next per_row - 1 columns, wrapping -- and every
    value of the matrix a bit pattern of its own (regular values; the diagonal 64 + i / 1024)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n * per_row)
    rows, k = [], 0
    for i in range(n):
        row = [(i, 64.0 + i / 1024.0)]
        for j in range(1, per_row):
            row.append(((i + j) % n, regular(int(order[k]) + 3)))
            k += 1
        rows.append(rotate(row, i))
    return rows


def case_xell_halved(per_row=32, n=356, nF=256):
    """356 rows of 32 entries, all values distinct: a block of 16 rows holds exactly 512 values -- the
    most a code can index, so value index 511 appears -- and any larger one too many.  The chunk
    [0, 256) is halved down to sixteen blocks of 16 rows; the chunk [256, 356) to 50, 25 and then
    12 / 13 rows: eight blocks of odd sizes with fewer than 16 live threads.  The twin with 40 entries
    per row cannot fit 16 x 40 values and is refused (sorted tiles: its adaptive blocks hold more than
    256 values)."""
    rows = distinct_rows(n, per_row, 11)
    sr = 40
    plant_specials(rows, sr)
    tiny = (300, 330, 355)
    plant_tiny(rows, tiny)
    rp, ci, v = to_csr(rows)
    enc = ENC_LEVEL | ENC_MERGED_ONLY
    edge = dict(longest_row=per_row, n=n, nF=nF, all_distinct=True, rows16_values=16 * per_row)
    if per_row == 32:
        variants = [(enc, xell_info(rp, v, n, nF, enc))]
        blocks = xell_choice(rp, v, n, nF, enc)[2]
        edge.update(W=32, nblk=24, block=(0, 16))
        name = "xell_halved"
    else:
        variants = [(enc, tile_info(rp, nF, FMT_SORTED))]
        blocks = tile_blocks(rp, nF)
        edge.update(W=0)
        name = "xell_halved_w40_refused"
    return _finish(Case(name, "xell", "distinct", rp, ci, v, n, nF, variants, blocks, edge,
                        kinds=("jacobi",), tiny_rows=tiny, special_row=sr))


def case_xell_shift24(m=600):
    """600 x (2^23 + 1000): the columns need 24 bits, which leaves 8 for the value index, 256 values per
    block.  Block [0, 256) holds exactly 256; its largest bit pattern, -2^30, sits on the last column:
    the code 255 << 24 | (2^23 + 999)."""
    ncols = (1 << 23) + 1000
    rows = []
    for r in range(m):
        cols = [(r * 13999 + j * 1048583) % (ncols - 1) for j in range(8)]
        rows.append([(c, regular(3 + (r * 8 + j) % 251)) for j, c in enumerate(cols)])
    sr = 30
    rows[sr][3] = (ncols - 1, rows[sr][3][1])
    plant_specials(rows, sr, square=False, big_col=ncols - 1)
    rp, ci, v = to_csr(rows)
    variants = [(ENC_TRANSFER, xell_info(rp, v, ncols, -1, ENC_TRANSFER))]
    return Case("xell_shift24", "xell", "rows", rp, ci, v, ncols, -1, variants, xell_choice(rp, v, ncols, -1, ENC_TRANSFER)[2],
                dict(longest_row=8, W=8, shift=24, block=(0, 256), values=256, top_code=True, dense=True), special_row=sr)


# ---------------------------------------------------------------- tile cases
TILE_POOL = [o for o in range(-127, 129) if o != 0]   # 255 non-zero offsets; with the diagonal: 256


def dtile_rows(n, nvals, seed, pool=True):
    """Rows of 41 to 60 entries: the diagonal and, pool: offsets of TILE_POOL from a start that moves
    by 37 with the row (a block of ~40 rows covers the pool: 256 offsets with the diagonal's), else
    random columns (far more than 256 offsets in a block).  nvals regular values, cycled entry by entry."""
    rng = np.random.default_rng(seed)
    rows, k = [], 0
    for i in range(n):
        m = 40 + (i * 7) % 20
        if pool:
            s = (i * 37) % 255
            cols = [i + o for o in (TILE_POOL[s:] + TILE_POOL[:s]) if 0 <= i + o < n][:m]
        else:
            cols = [int(c) for c in rng.permutation(n) if c != i][:m]
        row = [(i, 64.0)]
        for c in cols:
            row.append((c, regular(3 + k % nvals)))
            k += 1
        rows.append(rotate(row, i))
    return rows


def case_tile(name, n=400, nF=200):
    """dtile_full: in block `block` exactly 256 offsets and 256 values (250 regular ones, the diagonal's
    and the five planted).  dtile_over_off: one entry of the block on offset +129, so 257 offsets
    and value-dictionary sorted tiles; dtile_over_val: one entry with a 257th value, so plain sorted
    tiles.  vdict_full / vdict_over: random columns (no offset dictionary) with 256 / 257 values."""
    pool = name.startswith("dtile")
    rows = dtile_rows(n, 250, 5, pool)
    blocks0 = tile_blocks(to_csr(rows)[0], nF)
    # a block of interior rows: every offset of the pool stays inside the matrix
    blk = next(b for b in blocks0 if b[0] >= 127 and b[1] + 128 <= n)
    sr = blk[0] + 3
    plant_specials(rows, sr)
    tiny = (nF + 150, nF + 170, n - 1)
    plant_tiny(rows, tiny)
    r1 = blk[0] + 5
    s = next(s for s, (c, _) in enumerate(rows[r1]) if c != r1)
    if name == "dtile_over_off":
        rows[r1][s] = (r1 + 129, rows[r1][s][1])
    if name in ("dtile_over_val", "vdict_over"):
        rows[r1][s] = (rows[r1][s][0], regular(2))
    rp, ci, v = to_csr(rows)
    blocks = tile_blocks(rp, nF)
    assert blocks == blocks0
    over_val = name in ("dtile_over_val", "vdict_over")
    fmt = FMT_DICT if name == "dtile_full" else FMT_SORTED if over_val else FMT_SORTED | FMT_DICT
    edge = dict(rows_41_60=True, block=blk, n=n, nF=nF, values=TILE_DICT + over_val)
    if pool:
        edge.update(offsets=TILE_DICT + (name == "dtile_over_off"))
    else:
        edge.update(offsets_gt=TILE_DICT)
    return _finish(Case(name, "tile", "rows", rp, ci, v, n, nF, [(ENC_LEVEL, tile_info(rp, nF, fmt))], blocks, edge,
                        kinds=("jacobi",), tiny_rows=tiny, special_row=sr))


def case_sorted_span(over, m=600):
    """600 x (2^20 + 4096): row r holds column r and seven columns from 4096 on; the 1,792 of block
    [0, 256) are spread so that their cluster spans exactly TILE_DIAG_MARK - 1 columns (accepted: the
    largest packed offset is the one below the diagonal mark) or, over, TILE_DIAG_MARK (refused: the
    matrix keeps stored-order staging).  The other blocks span half of that.  Column r of row r gets
    the diagonal mark although the matrix is rectangular."""
    ncols = (1 << 20) + 4096
    b1 = 4096
    rows = []
    for r in range(m):
        q, t = divmod(r, K_BLOCK)
        span = TILE_DIAG_MARK - 1 if q == 0 else TILE_DIAG_MARK // 2
        row = []
        for j in range(7):
            e = t + K_BLOCK * j                       # 0 .. 1791 within the block
            last = over and q == 0 and e == 7 * K_BLOCK - 1   # the twin: the block's last column one further
            row.append((b1 + (e * span) // (7 * K_BLOCK - 1) + last, regular((r + j) % 100 + 3)))
        row.insert(3, (r, 64.0))
        rows.append(row)
    sr = 300
    plant_specials(rows, sr, square=False, big_col=rows[sr][4][0])   # (not on column r)
    rp, ci, v = to_csr(rows)
    assert ci.max() < ncols
    blocks = tile_blocks(rp)
    edge = dict(block=(0, 256), cut=b1, span=TILE_DIAG_MARK - 1 + over, c_eq_r=True)
    if over:
        variants = [(ENC_SORTED, tile_info(rp, -1, 0)), (ENC_SORTED | ENC_DICT, tile_info(rp, -1, 0))]
    else:
        variants = [(ENC_SORTED, tile_info(rp, -1, FMT_SORTED)),
                    (ENC_SORTED | ENC_DICT, tile_info(rp, -1, FMT_SORTED | FMT_DICT))]
    return Case("sorted_span" + ("_over" if over else ""), "tile", "rows", rp, ci, v, ncols, -1, variants, blocks, edge,
                special_row=sr)


# ---------------------------------------------------------------- the table
_BUILDERS = {}


def _register():
    B = _BUILDERS
    B["ell8_full"] = lambda: case_ell8("full")
    B["ell8_over_off"] = lambda: case_ell8("over_off")
    B["ell8_over_val"] = lambda: case_ell8("over_val")
    B["ell16_exact"] = lambda: case_ell_banded("ell16_exact", 16)
    B["ell16_plus1"] = lambda: case_ell_banded("ell16_plus1", 17)
    B["ell32_exact"] = lambda: case_ell_banded("ell32_exact", 32)
    B["ell32_plus1"] = lambda: case_ell_banded("ell32_plus1", 33)
    for n, nF in PAIR_SHAPES:
        B[f"ell8_pairs_{n}_{nF}"] = lambda n=n, nF=nF: case_ell8_pairs(n, nF)
    B["ell_based_R"] = case_ell_based
    for W in (8, 16, 20, 24, 32):
        B[f"xell_w{W}"] = lambda W=W: case_xell_w(W)
        if W < 32:
            B[f"xell_w{W}_plus1"] = lambda W=W: case_xell_w(W, 1)
    B["xell_w32_plus1_refused"] = lambda: case_xell_w(32, 1)
    B["xell_w40"] = lambda: case_xell_w(40, merged_only=True)
    B["xell_sparse"] = case_xell_sparse
    B["xell_halved"] = case_xell_halved
    B["xell_halved_w40_refused"] = lambda: case_xell_halved(40)
    B["xell_shift24"] = case_xell_shift24
    for name in ("dtile_full", "dtile_over_off", "dtile_over_val", "vdict_full", "vdict_over"):
        B[name] = lambda name=name: case_tile(name)
    B["sorted_span"] = lambda: case_sorted_span(0)
    B["sorted_span_over"] = lambda: case_sorted_span(1)


_register()
NAMES = list(_BUILDERS)
GROUPS = {"ell": [k for k in NAMES if k.startswith("ell")], "xell": [k for k in NAMES if k.startswith("xell")],
          "tile": [k for k in NAMES if not k.startswith(("ell", "xell"))]}
_cache = {}


def case(name: str) -> Case:
    """The case of that name (built once; callers leave its arrays unchanged)"""
    if name not in _cache:
        c = _BUILDERS[name]()
        assert c.name == name, (c.name, name)
        for a in (c.rp, c.ci, c.v):
            a.setflags(write=False)
        _cache[name] = c
    return _cache[name]
