"""Chunk kinds of the narrow merged keys (SSS_HIP_MERGE_KEY16) of a saved hierarchy, host-side.

    python tools/merged_keys.py HIERARCHY.bin [--n 400] [--levels 5-10] [--w 4]

(HIERARCHY.bin: a file of bench.py --hier-cache; when it cannot be loaded the 7-pt n^3 hierarchy is
set up instead.)

Per level the merged copies are rebuilt as the engine forms them -- the level relabeled F-first,
G consecutive rows per group (G = 8 from 80,000 rows, else 4; the two-segment [N | L] copies always
4), W shares of ceil(len / W) entries, chunks of 64 from each share's start -- and narrowed by the
library's own host function (sss_hip_merged_narrow).  Prints per copy (the level matrix A, and per
class the [N | L] copy and the L copy) the chunks with one base, with two bases, the wide ones, and
the chunks stored with 32-bit keys because their share holds a wide one; and the bytes per entry of
the narrow format (values, keys, descriptors, escaped keys).  On a GPU the same counts of an
uploaded hierarchy come from sss_hip_merged_key_stats.
"""
from __future__ import annotations

import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402
from amg_amd._native import csr_arrays  # noqa: E402


def narrow_counts(rows, cols, seg, nrows, g, w, two):
    """rows / cols / seg of a copy's entries (rows numbered from 0 in the copy) -> (counts[5], entries,
    descriptor slots, escaped keys)"""
    key = np.sort((rows // g) << 40 | cols << 4 | seg << 3 | rows % g)
    keys = (key & 0xFFFFFFFF).astype(np.uint32)
    del key
    ng = (nrows + g - 1) // g
    cs = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=nrows))])
    gp = cs[np.minimum(np.arange(ng + 1) * g, nrows)].astype(np.int32)
    cap = (keys.size >> 6) + ng * w + 1
    k16, desc, esc = np.zeros(keys.size, np.uint16), np.zeros((cap, 4), np.int32), np.zeros(max(keys.size, 1), np.uint32)
    nd, ne, cnt = C.c_longlong(), C.c_longlong(), (C.c_longlong * 5)()
    rc = A.lib().sss_hip_merged_narrow(keys.ctypes.data, keys.size, gp.ctypes.data_as(C.POINTER(C.c_int)), ng, int(two),
                                       w, k16.ctypes.data, desc.ctypes.data, cap, C.byref(nd), esc.ctypes.data, esc.size,
                                       C.byref(ne), cnt)
    if rc != 0:
        raise RuntimeError(f"sss_hip_merged_narrow failed ({rc})")
    return list(cnt), keys.size, nd.value, ne.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("hier")
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--levels", default="5-10")
    ap.add_argument("--w", type=int, default=4)
    a = ap.parse_args()
    lo, hi = (int(t) for t in a.levels.split("-"))
    try:
        H = A.Hierarchy.load(a.hier)
    except OSError:
        H = A.Hierarchy(A.generate(7, a.n))
    print(f"W = {a.w}; chunks of 64 entries; one / two bases with 13-bit column deltas")
    print("level copy       G     chunks   one base  two bases       wide  32-bit keys   B/entry")
    for l in range(lo, min(hi, H.num_levels - 2) + 1):
        L = H.level(l)
        rp, ci, _ = csr_arrays(L.A, copy=False)
        rp, ci = np.asarray(rp, np.int64), np.asarray(ci, np.int64)
        n = len(rp) - 1
        is_c = np.ctypeslib.as_array(L.cfmark.d, shape=(n,)) == 1
        perm = np.concatenate([np.flatnonzero(~is_c), np.flatnonzero(is_c)])
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
        nr, nc = inv[np.repeat(np.arange(n), np.diff(rp))], inv[ci]
        nf = int((~is_c).sum())
        g = 8 if n >= 80000 else 4
        off = nr != nc
        same_lower = off & ((nc < nf) == (nr < nf)) & (nc < nr)
        copies = [("A", np.ones(len(nr), bool), None, 0, n, g, False)]
        for name, cls, first, m in (("F", nr < nf, 0, nf), ("C", nr >= nf, nf, n - nf)):
            copies.append((f"{name} [N|L]", off & cls, same_lower, first, m, 4, True))
            copies.append((f"{name} L", same_lower & cls, None, first, m, 8 if m >= 80000 else 4, False))
        for name, sel, seg, first, m, gg, two in copies:
            if m == 0 or not sel.any():
                continue
            s = seg[sel].astype(np.int64) if seg is not None else np.zeros(int(sel.sum()), np.int64)
            cnt, nnz, nd, ne = narrow_counts(nr[sel] - first, nc[sel], s, m, gg, a.w, two)
            print(f"{l:5d} {name:9s} {gg:2d} {cnt[0]:10d} {cnt[1]:10d} {cnt[2]:10d} {cnt[3]:10d} {cnt[4]:12d} "
                  f"{(10.0 * nnz + 16.0 * nd + 4.0 * ne) / max(nnz, 1):9.3f}", flush=True)


if __name__ == "__main__":
    main()
