"""Batch composition of the merged-group two-stage copies of a saved hierarchy, host-side.

    python tools/merged_shares.py HIERARCHY.bin [--n 400] [--levels 5-10] [--g 4] [--w 4] [--u 6]

(HIERARCHY.bin: a file of bench.py --hier-cache; when it cannot be loaded the 7-pt n^3 hierarchy is
set up instead.)

Per level and class (F, C) the [N | L] copy ts_stage0 reads is rebuilt as the engine groups it: the
class's rows in ascending order, G consecutive rows per group, the group's off-diagonal entries cut
into W shares of ceil(len / W).  Prints the distribution of chunks of 64 per share and how many
shares end in a batch of one or two chunks when a wave takes U chunks per batch.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import amg_amd as A  # noqa: E402
from amg_amd._native import csr_arrays  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("hier")
    ap.add_argument("--n", type=int, default=400)
    ap.add_argument("--levels", default="5-10")
    ap.add_argument("--g", type=int, default=4)
    ap.add_argument("--w", type=int, default=4)
    ap.add_argument("--u", type=int, default=6)
    a = ap.parse_args()
    lo, hi = (int(t) for t in a.levels.split("-"))
    try:
        H = A.Hierarchy.load(a.hier)
    except OSError:
        H = A.Hierarchy(A.generate(7, a.n))
    print(f"G = {a.g}, W = {a.w}, U = {a.u} chunks per batch")
    print("level class   groups  entries/share: mean   chunks/share: p10 p50 p90 max   last batch 1 chunk  2 chunks   batches/share mean")
    for l in range(lo, min(hi, H.num_levels - 2) + 1):
        L = H.level(l)
        rp, ci, _ = csr_arrays(L.A, copy=False)
        n = len(rp) - 1
        mark = np.ctypeslib.as_array(L.cfmark.d, shape=(n,))
        row = np.repeat(np.arange(n), np.diff(rp))
        off = np.bincount(row[ci != row], minlength=n)
        for name, sel in (("F", mark != 1), ("C", mark == 1)):
            lens = off[sel]
            m = len(lens)
            if m == 0:
                continue
            cs = np.concatenate([[0], np.cumsum(lens)])
            glen = cs[np.minimum(np.arange(a.g, m + a.g, a.g), m)] - cs[np.arange(0, m, a.g)]
            per = (glen + a.w - 1) // a.w
            sh = np.concatenate([np.minimum(glen, (p + 1) * per) - np.minimum(glen, p * per) for p in range(a.w)])
            ch = (sh + 63) // 64
            last = np.where(ch > 0, (ch - 1) % a.u + 1, 0)
            nb = (ch + a.u - 1) // a.u
            p10, p50, p90 = np.percentile(ch, [10, 50, 90])
            print(f"{l:5d} {name:>5s} {len(glen):8d} {sh.mean():20.1f} {p10:18.0f} {p50:3.0f} {p90:3.0f} {ch.max():3d} "
                  f"{100.0 * (last == 1).mean():16.1f} % {100.0 * (last == 2).mean():7.1f} % {nb.mean():20.2f}")


if __name__ == "__main__":
    main()
