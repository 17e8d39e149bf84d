"""CPU: the narrowing of the merged-group keys (sss_hip_merged_narrow, include/sss_hip.h).

A merged copy holds, per group of G rows, the entries sorted by the 32-bit key
col << 4 | segment << 3 | row; W waves take consecutive shares of ceil(len / W) entries, in chunks of
64 counted from each share's start.  The narrow format stores per entry a 16-bit key
(col - base) << 3 | accumulator (accumulator: segment << 2 | row with two segments, else row) and per
chunk a descriptor {base_lo, base_hi, split, esc}: lanes below `split` add base_lo, the others
base_hi; a share with a chunk that fits neither one base (span < 2^13) nor two keeps its 32-bit keys
in the escape list, esc being the chunk's first key there.  Chunk c of share p of group g is
descriptor (first entry of the share >> 6) + g W + p + c.

Here the function runs on designed and on seeded random key lists for G in {4, 8}, one and two
segments (two: G = 4, as the engine caps it) and W in {1, 2, 4}; decoding keys, descriptors and escape
list must give back every (col, segment, row) at its position.  Designed chunks: span exactly
2^13 - 1 and exactly 2^13; the one wide gap at lane 1, 32 and 63; two wide gaps (escapes); a wide gap
exactly on a chunk boundary (no split); a share shorter than 64, an empty share, an empty group; a
last chunk of one entry; a column at ncols - 1 with ncols = 2^28 - 1.  Every descriptor kind must
occur: the tests fail, never skip, if one does not.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import amg_amd as A

B = 13
SPAN = 1 << B
NCOLS = (1 << 28) - 1
CASES = [(4, False), (8, False), (4, True)]
WS = (1, 2, 4)


def _keys(cols, g, two):
    """sorted unique 32-bit keys of the columns `cols` (strictly increasing), rows and segments cycling"""
    cols = np.asarray(cols, dtype=np.int64)
    assert (np.diff(cols) > 0).all() and (cols.size == 0 or (cols[0] >= 0 and cols[-1] < NCOLS))
    i = np.arange(cols.size)
    seg = (i // g) % 2 if two else np.zeros(cols.size, np.int64)
    return (cols << 4 | seg << 3 | i % g).astype(np.uint32)


def _narrow(keys, gp, two, w):
    lib = A.lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    gp = np.ascontiguousarray(gp, dtype=np.int32)
    nnz, ng = keys.size, gp.size - 1
    cap = (nnz >> 6) + ng * w + 1
    k16 = np.full(max(nnz, 1), 0xFFFF, np.uint16)
    desc = np.full((cap, 4), -7, np.int32)
    esc = np.zeros(max(nnz, 1), np.uint32)
    nd, ne = C.c_longlong(), C.c_longlong()
    cnt = (C.c_longlong * 5)()
    rc = lib.sss_hip_merged_narrow(keys.ctypes.data, nnz, gp.ctypes.data_as(C.POINTER(C.c_int)), ng, int(two), w,
                                   k16.ctypes.data, desc.ctypes.data, cap, C.byref(nd), esc.ctypes.data, esc.size,
                                   C.byref(ne), cnt)
    assert rc == 0 and nd.value == cap
    return k16[:nnz], desc, esc[: ne.value], list(cnt)


def _shares(gp, w):
    """(group, part, first entry, end, first descriptor) of every non-empty share"""
    for g in range(len(gp) - 1):
        k0, ln = int(gp[g]), int(gp[g + 1] - gp[g])
        per = (ln + w - 1) // w
        for p in range(w):
            a, e = k0 + min(ln, p * per), k0 + min(ln, (p + 1) * per)
            if a < e:
                yield g, p, a, e, (a >> 6) + g * w + p


def _decode(k16, desc, esc, gp, two, w):
    """the 32-bit keys back, the kind of every chunk {(group, part, chunk): (kind, descriptor)},
    and the descriptor slots in use"""
    out = np.zeros(k16.size, np.uint32)
    kinds, used = {}, set()
    for g, p, a, e, d0 in _shares(gp, w):
        for c, kb in enumerate(range(a, e, 64)):
            m = min(64, e - kb)
            lo, hi, split, off = (int(x) for x in desc[d0 + c])
            used.add(d0 + c)
            if off >= 0:
                out[kb:kb + m] = esc[off:off + m]
                kinds[g, p, c] = ("esc", (lo, hi, split, off))
                continue
            q = k16[kb:kb + m].astype(np.int64)
            lane = np.arange(m)
            col = np.where(lane < split, lo, hi) + (q >> 3)
            acc = q & 7
            seg, row = (acc >> 2, acc & 3) if two else (0 * acc, acc)
            out[kb:kb + m] = (col << 4 | seg << 3 | row).astype(np.uint32)
            assert split == 64 or 1 <= split < m
            kinds[g, p, c] = ("one" if split == 64 else "two", (lo, hi, split, off))
    return out, kinds, used


# the designed chunks of a share: name -> 64 column offsets from the chunk's base
def _chunks():
    r = np.arange
    return [
        ("span_max", np.concatenate([r(63), [SPAN - 1]])),                     # one base, the widest
        ("span_over", np.concatenate([r(63), [SPAN]])),                        # one too wide: two bases, split 63
        ("gap1", np.concatenate([[0], 100000 + r(63)])),
        ("gap32", np.concatenate([r(32), 100000 + r(32)])),
        ("gap63", np.concatenate([3 * r(63), [100000]])),
        ("tie", np.concatenate([r(10), 50000 + r(10), 100000 - 10 + r(44)])),   # two equal widest gaps (test_tie_...)
        ("plain", 5 * r(64)),
        ("halves_max", np.concatenate([r(31), [SPAN - 1], SPAN - 1 + 70000 + r(31), [2 * SPAN - 2 + 70000]])),
    ]


def _designed(g, two, w):
    """key list and group bounds: group 0 the designed narrow chunks in every share (the last share
    ends at column ncols - 1 in a chunk of one entry), group 1 a share with two wide gaps in one chunk
    among plain chunks, group 2 empty, group 3 of 5 entries (short and empty shares), group 4 of one
    entry, group 5 plain"""
    names = [n for n, _ in _chunks() if n != "tie"]
    groups = []
    cols = []
    for p in range(w):
        base = p << 25
        for j, (name, off) in enumerate(c for c in _chunks() if c[0] != "tie"):
            cols += list(base + (j << 20) + off)
        if p == w - 1:   # the last share: two bases reaching ncols - 2, then ncols - 1 alone
            cols += list(np.concatenate([(1 << 27) + 5 + np.arange(32), NCOLS - 1 - 32 + np.arange(32)]))
            cols.append(NCOLS - 1)
        else:
            cols += list(base + (20 << 20) + 7 * np.arange(64))
            cols.append(base + (21 << 20))
    groups.append(cols)
    two_gaps = np.concatenate([np.arange(21), 100000 + np.arange(21), 200000 + np.arange(22)])
    cols = []
    for p in range(w):
        base = p << 25
        cols += list(base + 3 * np.arange(64)) + list(base + (1 << 20) + two_gaps) + list(base + (2 << 20) + np.arange(40))
    groups.append(cols)
    groups.append([])
    groups.append([3, 9, 5000, 5001, 90000])
    groups.append([NCOLS - 1])
    groups.append(list(11 * np.arange(200)))
    keys = np.concatenate([_keys(c, g, two) for c in groups])
    gp = np.concatenate([[0], np.cumsum([len(c) for c in groups])])
    return keys, gp, names


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("g,two", CASES, ids=lambda v: str(v))
def test_designed_chunks(g, two, w):
    keys, gp, names = _designed(g, two, w)
    k16, desc, esc, cnt = _narrow(keys, gp, two, w)
    back, kinds, used = _decode(k16, desc, esc, gp, two, w)
    assert np.array_equal(back, keys)
    # every share of group 0 holds the designed chunks in order, then a two-base / plain chunk and one entry
    want = {"span_max": ("one", 64), "span_over": ("two", 63), "gap1": ("two", 1), "gap32": ("two", 32),
            "gap63": ("two", 63), "plain": ("one", 64), "halves_max": ("two", 32)}
    for p in range(w):
        for j, name in enumerate(names):
            kind, d = kinds[0, p, j]
            assert (kind, d[2]) == want[name], (p, name, kind, d)
        kind, d = kinds[0, p, len(names)]
        assert kind == ("two" if p == w - 1 else "one")
        kind, d = kinds[0, p, len(names) + 1]   # the last chunk: one entry
        assert kind == "one" and d[:3] == ((NCOLS - 1 if p == w - 1 else (p << 25) + (21 << 20)),) * 2 + (64,)
    # consecutive chunks lie 2^20 columns apart: the wide gap on a chunk boundary needs no split
    j = names.index("plain")
    assert kinds[0, 0, j][0] == "one" and kinds[0, 0, j][1][0] - (kinds[0, 0, j - 1][1][1] + SPAN) > SPAN
    # group 1: the chunk with two wide gaps escapes, and its whole share with it
    for p in range(w):
        assert [kinds[1, p, c][0] for c in range(3)] == ["esc"] * 3
        off = [kinds[1, p, c][1][3] for c in range(3)]
        assert off[1] == off[0] + 64 and off[2] == off[0] + 128
    assert esc.size == w * 168
    # group 3 (5 entries) and group 4 (1 entry): shares shorter than 64, empty shares without a descriptor
    assert sum(1 for k in kinds if k[0] == 3) == {1: 1, 2: 2, 4: 3}[w]
    assert [k for k in kinds if k[0] == 4] == [(4, 0, 0)] and not [k for k in kinds if k[0] == 2]
    # every kind occurs; the counts are the decoded kinds
    n_one = sum(1 for k, _ in kinds.values() if k == "one")
    n_two = sum(1 for k, _ in kinds.values() if k == "two")
    n_esc = sum(1 for k, _ in kinds.values() if k == "esc")
    assert n_one > 0 and n_two > 0 and n_esc > 0
    assert cnt[0] == len(kinds) and cnt[3] == w and cnt[4] == n_esc == 3 * w
    assert cnt[1] == n_one + 2 * w and cnt[2] == n_two   # (the escaped shares' plain chunks count as one base)
    # unused descriptor slots stay zero
    free = np.ones(len(desc), bool)
    free[list(used)] = False
    assert not desc[free].any()


def test_tie_takes_the_lowest_lane():
    """two equal widest gaps: the split is the first; the upper half then spans too far (wide)"""
    off = dict(_chunks())["tie"]
    keys, gp = _keys(off, 4, False), np.array([0, 64])
    k16, desc, esc, cnt = _narrow(keys, gp, False, 1)
    assert cnt == [1, 0, 0, 1, 1] and np.array_equal(esc, keys) and desc[0, 3] == 0
    # ... and a tie that fits: gaps 9000 | 9000 cannot both be skipped, so lower the second
    cols = np.concatenate([np.arange(10), 9009 + np.arange(10), 9019 + 8000 + np.arange(44)])
    keys = _keys(cols, 4, False)
    k16, desc, esc, cnt = _narrow(keys, gp, False, 1)
    assert cnt == [1, 0, 1, 0, 0] and tuple(desc[0]) == (0, 9009, 10, -1)
    back, _, _ = _decode(k16, desc, esc, gp, False, 1)
    assert np.array_equal(back, keys)


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("g,two", CASES, ids=lambda v: str(v))
def test_random_lists(g, two, w):
    rng = np.random.default_rng(1000 * g + 10 * w + int(two))
    groups = []
    for _ in range(150):
        n = int(rng.choice([0, 1, 3, 63, 64, 65, 130, 300, 700, 1500]))
        f0, c0 = int(rng.integers(0, 40000)), int(rng.integers(60000, 900000))
        pool = np.concatenate([f0 + rng.integers(0, 6000, n), c0 + rng.integers(0, 6000, n),
                               rng.integers(0, 1 << 20, max(n // 50, 1) if rng.random() < 0.3 else 0)])
        cols = np.unique(pool)
        groups.append(np.sort(rng.choice(cols, min(n, cols.size), replace=False)))
    keys = np.concatenate([_keys(c, g, two) for c in groups])
    gp = np.concatenate([[0], np.cumsum([len(c) for c in groups])])
    k16, desc, esc, cnt = _narrow(keys, gp, two, w)
    back, kinds, used = _decode(k16, desc, esc, gp, two, w)
    assert np.array_equal(back, keys)
    got = [sum(1 for k, _ in kinds.values() if k == name) for name in ("one", "two", "esc")]
    assert min(got) > 0, got
    assert cnt[0] == len(kinds) and cnt[4] == got[2] and cnt[3] > 0 and cnt[1] + cnt[2] + cnt[3] == cnt[0]
    # the rule itself, chunk by chunk, from the original keys
    col = (keys >> 4).astype(np.int64)
    wide_shares = set()
    for gi, p, a, e, d0 in _shares(gp, w):
        for c, kb in enumerate(range(a, e, 64)):
            cc = col[kb:min(kb + 64, e)]
            kind, d = kinds[gi, p, c]
            if cc[-1] - cc[0] < SPAN:
                fits = "one"
            else:
                s = int(np.argmax(np.diff(cc))) + 1
                fits = "two" if cc[s - 1] - cc[0] < SPAN and cc[-1] - cc[s] < SPAN else "wide"
            if fits == "wide":
                wide_shares.add((gi, p))
            elif kind != "esc":
                assert kind == fits
    assert wide_shares == {(k[0], k[1]) for k, v in kinds.items() if v[0] == "esc"}


def test_bad_arguments():
    lib = A.lib()
    keys, gp = _keys(np.arange(10), 4, False), np.array([0, 10], np.int32)
    k16, desc, esc = np.zeros(10, np.uint16), np.zeros((8, 4), np.int32), np.zeros(10, np.uint32)
    nd, ne, cnt = C.c_longlong(), C.c_longlong(), (C.c_longlong * 5)()

    def call(w, cap, gpv=gp):
        return lib.sss_hip_merged_narrow(keys.ctypes.data, 10, gpv.ctypes.data_as(C.POINTER(C.c_int)), 1, 0, w,
                                         k16.ctypes.data, desc.ctypes.data, cap, C.byref(nd), esc.ctypes.data, 10,
                                         C.byref(ne), cnt)

    assert call(4, 8) == 0 and nd.value == 5
    assert call(3, 8) != 0                                  # W is 1, 2 or 4
    assert call(4, 4) != 0 and nd.value == 5                # too few descriptor slots: the need is reported
    assert call(4, 8, np.array([0, 9], np.int32)) != 0      # the bounds do not cover the keys
