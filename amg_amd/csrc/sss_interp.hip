// sss_interp.hip — the standard interpolation of the setup (interp_type intERP_STD) on the GPU: the
// P pattern (amg_amd/host/sss_setup.c std_pattern) and the weights with the coarse renumbering and the
// truncation (interp_STD, interp_trunc_par), bit for bit the host result.
//
// Both are row-independent; G lanes of one wavefront share a row, G chosen from the average row of S.
// What makes the host result depend on order is kept per row:
//
//   pattern  the candidates of an F row i are the C points of S_i and, for every F point k != i of
//            S_i, the C points of S_k, numbered in the host's discovery order.  Each candidate claims
//            its column's slot of a per-row hash table with an atomicMin of its number; a second walk
//            keeps the candidates that own their slot, at offsets from an in-order ballot of the group.
//   weights  hat a lives in a per-row hash table keyed by column.  A slot has one owner lane
//            (slot mod G), and only the owner adds to it: the contributions of a chunk of G entries
//            are handed to the owners lane by lane, in stored order, so every slot sees its terms in
//            the host's (j, m) order.  The scalars of the row (hat a_ii, alN, alP) are computed by
//            every lane of the group from the same loads in the same order.
//   ext+i    the weights of interp_type intERP_EXTI (interp_EXTI) on the same pattern, with
//            the same table and owner rule.  The stored entries of row i are classified G at a time (one
//            table lookup each: membership in the pattern is the lookup) and applied in stored order; a
//            strong F neighbour k has row k of A walked twice by the group, first for den, then for the
//            terms f a_kl, the qualifying entries of a chunk taken lane by lane from an in-order ballot.
//            d and den are computed by every lane of the group.
//   cap      the truncation with at most pmax entries per row (SSS_SETUP_PMAX): the cut of a
//            capped row is found in pmax rounds of a group-wide arg-max, the sums the host makes in stored
//            order are made in stored order by every lane of the group from the same values.
//
// The table of a row is in LDS when the row's candidate bound (its S row plus the S rows of its strong
// F neighbours) fits the group's share of it, else in a global array sized from the bound inside the
// same call.  Probe loops are bounded by the capacity, every index read from A, S and P is
// range-checked, and what cannot happen on consistent input (a strong column absent from the A row,
// a C column absent from the pattern row, a full table) raises a flag the host reads back: the call
// then fails with P untouched.  Ordinary launches only; nothing waits on another workgroup.
#include "sss_engine.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <initializer_list>
#include <cstring>
#include <string>

namespace sss {

namespace {

constexpr int kLdsSlots = 2048;          // table slots per workgroup (8 G per group of G lanes)
constexpr int kMaxBound = 1 << 27;       // candidate bound of one row (its table has twice as many slots)
enum : int { kErrIndex = 1, kErrStrongCol = 2, kErrPatternCol = 4, kErrTableFull = 8, kErrBound = 16 };

struct Csr {
    int n, nnz;
    const int *rp, *ci;
    const double *v;
};

__host__ __device__ __forceinline__ int tab_cap(int need)
{
    int c = 2;
    while (c < 2 * need) c <<= 1;
    return c;
}

__device__ __forceinline__ unsigned tab_hash(int col, int cap) { return ((unsigned)col * 2654435761u >> 7) & (unsigned)(cap - 1); }

__device__ __forceinline__ void span(const Csr &M, int i, int &lo, int &hi)
{
    lo = max(M.rp[i], 0);
    hi = max(min(M.rp[i + 1], M.nnz), lo);
}

// slot of col (inserted when absent), -1 when the table is full
__device__ __forceinline__ int tab_insert(int *key, int cap, int col)
{
    unsigned s = tab_hash(col, cap);
    for (int p = 0; p < cap; ++p, s = (s + 1) & (unsigned)(cap - 1)) {
        const int prev = atomicCAS(&key[s], -1, col);
        if (prev == -1 || prev == col) return (int)s;
    }
    return -1;
}

// slot of col, -1 when absent
__device__ __forceinline__ int tab_find(const int *key, int cap, int col)
{
    unsigned s = tab_hash(col, cap);
    for (int p = 0; p < cap; ++p, s = (s + 1) & (unsigned)(cap - 1)) {
        const int k = key[s];
        if (k == col) return (int)s;
        if (k == -1) return -1;
    }
    return -1;
}

// Candidate bound of every F row (at least plen, the row's pattern length, when prp is given), the
// capacity of its global table (0: the row's table is in LDS) and the rows that have one.
__global__ __launch_bounds__(kBlock) void interp_bound(Csr S, const int *__restrict__ mark, const int *__restrict__ prp,
                                                       int pnnz, int slots, int *__restrict__ need,
                                                       long long *__restrict__ gcap, int *__restrict__ ctr)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= S.n) return;
    long long b = 0;
    if (mark[i] == FGPT) {
        int lo, hi;
        span(S, i, lo, hi);
        b = hi - lo;
        for (int q = lo; q < hi; ++q) {
            const int k = S.ci[q];
            if ((unsigned)k >= (unsigned)S.n) {
                atomicOr(&ctr[0], kErrIndex);
                continue;
            }
            if (mark[k] == FGPT && k != i) {
                int klo, khi;
                span(S, k, klo, khi);
                b += khi - klo;
            }
        }
        if (prp) b = max(b, (long long)(min(prp[i + 1], pnnz) - max(prp[i], 0)));
    }
    if (b > kMaxBound) {
        atomicOr(&ctr[0], kErrBound);
        b = 0;
    }
    need[i] = (int)b;
    const bool glob = b > slots;
    gcap[i] = glob ? tab_cap((int)b) : 0;
    if (glob) atomicAdd(&ctr[1], 1);
}

// the table of row i: in the group's share of LDS, or at goff[i] of the global arrays
__device__ __forceinline__ int row_table(int i, int grp, int slots, const int *need, const long long *goff, int *lkey,
                                         int *gkey, int *&key, long long &off)
{
    const int b = need[i];
    if (b > slots) {
        off = goff[i];
        key = gkey + off;
        return tab_cap(b);
    }
    off = -1 - (long long)grp * slots;
    key = lkey + grp * slots;
    return min(slots, tab_cap(b));
}

template <int G>
__device__ __forceinline__ unsigned long long group_ballot(bool p, int gl)
{
    const unsigned long long b = __ballot(p);
    if (G == 64) return b;
    const int gbase = (int)(threadIdx.x & 63) - gl;
    return (b >> gbase) & ((1ull << (G & 63)) - 1ull);
}

// One walk over the candidates of F row i in discovery order.  CLAIM: every candidate claims its slot
// with its sequence number.  Else: the candidates that own their slot are counted, and with FILL
// written to out[] in order.  Returns the count (the same on every lane of the group).
template <int G, bool CLAIM, bool FILL>
__device__ __forceinline__ int pattern_walk(const Csr &S, const int *__restrict__ mark, int i, int gl, int *key, int *seq,
                                            int cap, int *out, int room, int *err)
{
    int lo, hi, base = 0, kept = 0;
    span(S, i, lo, hi);
    for (int q = lo; q < hi; ++q) {
        const int k = S.ci[q];
        if ((unsigned)k >= (unsigned)S.n) continue;   // flagged by interp_bound
        const int mk = mark[k];
        int klo = q, khi = q + 1;                     // a C point: the one candidate k itself
        if (mk == FGPT && k != i) span(S, k, klo, khi);
        else if (mk != CGPT) continue;
        for (int r0 = klo; r0 < khi; r0 += G) {
            const int r = r0 + gl;
            int h = -1;
            if (r < khi) {
                h = S.ci[r];
                if ((unsigned)h >= (unsigned)S.n) {
                    atomicOr(err, kErrIndex);
                    h = -1;
                } else if (mark[h] != CGPT) {
                    h = -1;
                }
            }
            const int s = base + (r - klo);
            if (CLAIM) {
                if (h >= 0) {
                    const int slot = tab_insert(key, cap, h);
                    if (slot < 0) atomicOr(err, kErrTableFull);
                    else atomicMin(&seq[slot], s);
                }
            } else {
                bool own = false;
                if (h >= 0) {
                    const int slot = tab_find(key, cap, h);
                    if (slot < 0) atomicOr(err, kErrTableFull);
                    else own = seq[slot] == s;
                }
                const unsigned long long m = group_ballot<G>(own, gl);
                if (FILL && own) {
                    const int o = kept + __popcll(m & ((1ull << gl) - 1ull));
                    if (o < room) out[o] = h;
                }
                kept += __popcll(m);
            }
        }
        base += khi - klo;
    }
    return kept;
}

// count (FILL false: cnt[i]) or fill (pci at prp[i]) of the pattern; G lanes per row
template <int G, bool FILL>
__global__ __launch_bounds__(kBlock) void pattern_rows(Csr S, const int *__restrict__ mark, int slots,
                                                       const int *__restrict__ need, const long long *__restrict__ goff,
                                                       int *__restrict__ gkey, int *__restrict__ gseq, int *__restrict__ cnt,
                                                       const int *__restrict__ prp, int pnnz, int *__restrict__ pci,
                                                       int *__restrict__ err)
{
    __shared__ int lkey[kLdsSlots], lseq[kLdsSlots];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (kBlock / G) + grp;
    const int i = row < S.n ? (int)row : -1;
    const int mi = i >= 0 ? mark[i] : UNPT;
    int *key = nullptr, *seq = nullptr, cap = 0;
    if (mi == FGPT) {
        long long off;
        cap = row_table(i, grp, slots, need, goff, lkey, gkey, key, off);
        seq = off >= 0 ? gseq + off : lseq + (-1 - off);
        for (int s = gl; s < cap; s += G) {
            key[s] = -1;
            seq[s] = INT_MAX;
        }
    }
    __syncthreads();
    if (mi == FGPT) pattern_walk<G, true, false>(S, mark, i, gl, key, seq, cap, nullptr, 0, err);
    __syncthreads();
    if (mi == FGPT) {
        int o = 0, room = 0;
        if (FILL) {
            o = max(prp[i], 0);
            room = min(prp[i + 1], pnnz) - o;
        }
        // the fill writes what the count counted: the same walk over the same table
        const int kept = pattern_walk<G, false, FILL>(S, mark, i, gl, key, seq, cap, pci + o, room, err);
        if (FILL) {
            if (kept != room && gl == 0) atomicOr(err, kErrPatternCol);
        } else if (gl == 0) {
            cnt[i] = kept;
        }
    } else if (i >= 0 && gl == 0) {
        if (!FILL) cnt[i] = mi == CGPT ? 1 : 0;
        else if (mi == CGPT) {
            const int o = prp[i];
            if ((unsigned)o < (unsigned)pnnz) pci[o] = i;
        }
    }
}

// ---- the distance-two graph S2 of aggressive coarsening (amg_amd/host/sss_setup.c agg_graph) ----
// Row c of S2 belongs to C point i = crow[c].  Its candidates, in the host's discovery order: for each
// k != i of S_i the block (k, then the entries of S_k), of which the C points other than i count.  The
// first-occurrence rule is the pattern's: claim the column's slot with the sequence number, keep the
// candidates that own their slot, offsets from an in-order ballot.  Columns are written in C numbering.

// every column of S in range, as the host form checks before it builds anything
__global__ __launch_bounds__(kBlock) void agg_check_cols(Csr S, int *__restrict__ err)
{
    const long long q = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (q < S.nnz && (unsigned)S.ci[q] >= (unsigned)S.n) atomicOr(err, kErrIndex);
}

// the fine row of every C point, in C numbering (cmap: exclusive sum of the C flags)
__global__ __launch_bounds__(kBlock) void agg_crow(int n, const int *__restrict__ mark, const int *__restrict__ cmap,
                                                   int nc, int *__restrict__ crow)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || mark[i] != CGPT) return;
    const int c = cmap[i];
    if ((unsigned)c < (unsigned)nc) crow[c] = i;
}

// candidate bound of every row of S2, the capacity of its global table (0: in LDS), the rows that have one
__global__ __launch_bounds__(kBlock) void agg_bound(Csr S, const int *__restrict__ crow, int nc, int slots,
                                                    int *__restrict__ need, long long *__restrict__ gcap,
                                                    int *__restrict__ ctr)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= nc) return;
    const int i = crow[c];
    long long b = 0;
    if ((unsigned)i >= (unsigned)S.n) {
        atomicOr(&ctr[0], kErrIndex);
    } else {
        int lo, hi;
        span(S, i, lo, hi);
        for (int q = lo; q < hi; ++q) {
            const int k = S.ci[q];
            if ((unsigned)k >= (unsigned)S.n) {
                atomicOr(&ctr[0], kErrIndex);
                continue;
            }
            if (k == i) continue;
            int klo, khi;
            span(S, k, klo, khi);
            b += 1 + (khi - klo);
        }
    }
    if (b > kMaxBound) {
        atomicOr(&ctr[0], kErrBound);
        b = 0;
    }
    need[c] = (int)b;
    const bool glob = b > slots;
    gcap[c] = glob ? tab_cap((int)b) : 0;
    if (glob) atomicAdd(&ctr[1], 1);
}

// One walk over the candidates of C row i in discovery order; CLAIM and FILL as pattern_walk.
template <int G, bool CLAIM, bool FILL>
__device__ __forceinline__ int agg_walk(const Csr &S, const int *__restrict__ mark, const int *__restrict__ cmap, int i,
                                        int gl, int *key, int *seq, int cap, int *out, int room, int *err)
{
    int lo, hi, base = 0, kept = 0;
    span(S, i, lo, hi);
    for (int q = lo; q < hi; ++q) {
        const int k = S.ci[q];
        if ((unsigned)k >= (unsigned)S.n || k == i) continue;   // out of range: flagged by agg_bound
        int klo, khi;
        span(S, k, klo, khi);
        const int total = 1 + (khi - klo);                      // k itself, then row k of S
        for (int r0 = 0; r0 < total; r0 += G) {
            const int r = r0 + gl;
            int h = -1;
            if (r < total) {
                h = r == 0 ? k : S.ci[klo + r - 1];
                if ((unsigned)h >= (unsigned)S.n) {
                    atomicOr(err, kErrIndex);
                    h = -1;
                } else if (h == i || mark[h] != CGPT) {
                    h = -1;
                }
            }
            const int s = base + r;
            if (CLAIM) {
                if (h >= 0) {
                    const int slot = tab_insert(key, cap, h);
                    if (slot < 0) atomicOr(err, kErrTableFull);
                    else atomicMin(&seq[slot], s);
                }
            } else {
                bool own = false;
                if (h >= 0) {
                    const int slot = tab_find(key, cap, h);
                    if (slot < 0) atomicOr(err, kErrTableFull);
                    else own = seq[slot] == s;
                }
                const unsigned long long m = group_ballot<G>(own, gl);
                if (FILL && own) {
                    const int o = kept + __popcll(m & ((1ull << gl) - 1ull));
                    if (o < room) out[o] = cmap[h];
                }
                kept += __popcll(m);
            }
        }
        base += total;
    }
    return kept;
}

// count (FILL false: cnt[c]) or fill (s2ci at s2rp[c]) of S2; G lanes per row
template <int G, bool FILL>
__global__ __launch_bounds__(kBlock) void agg_rows(Csr S, const int *__restrict__ mark, const int *__restrict__ cmap,
                                                   const int *__restrict__ crow, int nc, int slots,
                                                   const int *__restrict__ need, const long long *__restrict__ goff,
                                                   int *__restrict__ gkey, int *__restrict__ gseq, int *__restrict__ cnt,
                                                   const int *__restrict__ s2rp, int s2nnz, int *__restrict__ s2ci,
                                                   int *__restrict__ err)
{
    __shared__ int lkey[kLdsSlots], lseq[kLdsSlots];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (kBlock / G) + grp;
    const int c = row < nc ? (int)row : -1;
    int i = c >= 0 ? crow[c] : -1;
    if ((unsigned)i >= (unsigned)S.n) i = -1;                   // flagged by agg_bound
    int *key = nullptr, *seq = nullptr, cap = 0;
    if (i >= 0) {
        long long off;
        cap = row_table(c, grp, slots, need, goff, lkey, gkey, key, off);
        seq = off >= 0 ? gseq + off : lseq + (-1 - off);
        for (int s = gl; s < cap; s += G) {
            key[s] = -1;
            seq[s] = INT_MAX;
        }
    }
    __syncthreads();
    if (i >= 0) agg_walk<G, true, false>(S, mark, cmap, i, gl, key, seq, cap, nullptr, 0, err);
    __syncthreads();
    if (i >= 0) {
        int o = 0, room = 0;
        if (FILL) {
            o = max(s2rp[c], 0);
            room = min(s2rp[c + 1], s2nnz) - o;
        }
        const int kept = agg_walk<G, false, FILL>(S, mark, cmap, i, gl, key, seq, cap, s2ci + o, room, err);
        if (FILL) {
            if (kept != room && gl == 0) atomicOr(err, kErrPatternCol);
        } else if (gl == 0) {
            cnt[c] = kept;
        }
    } else if (c >= 0 && gl == 0 && !FILL) {
        cnt[c] = 0;
    }
}

// ---- multipass interpolation (amg_amd/host/sss_setup.c mpass_build) ----
// Pass numbers by relaxation sweeps, then one round of launches per pass over that pass's rows.  The
// rows of a pass read only the rows of P of the pass before, which sit in that pass's block (pcol,
// pval; row k at off[k], len[k] entries, fine columns).  The pattern of a row keeps first occurrences
// in the order of the walk (the stored entries (i, k) of A with k in N_i, row k of P inside); hat w
// sits in the row's table, a slot owned by lane slot mod G, its terms handed over lane by lane in walk
// order.  d, tot and sub are computed by every lane of the group.

// consistent input: every index in range, and every strong column k != i of a row in the row of A
__global__ __launch_bounds__(kBlock) void mpass_check_rows(Csr A, Csr S, int *__restrict__ err)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n) return;
    int lo, hi, slo, shi;
    span(A, i, lo, hi);
    span(S, i, slo, shi);
    if (A.rp[i] != lo || A.rp[i + 1] != hi || S.rp[i] != slo || S.rp[i + 1] != shi) atomicOr(err, kErrIndex);
    for (int j = lo; j < hi; ++j)
        if ((unsigned)A.ci[j] >= (unsigned)A.n) atomicOr(err, kErrIndex);
    for (int q = slo; q < shi; ++q) {
        const int k = S.ci[q];
        if ((unsigned)k >= (unsigned)A.n) {
            atomicOr(err, kErrIndex);
            continue;
        }
        bool found = k == i;
        for (int j = lo; j < hi && !found; ++j) found = A.ci[j] == k;
        if (!found) atomicOr(err, kErrStrongCol);
    }
}

// pass 0: a C row is its own column with 1.0, at its coarse number in block 0
__global__ __launch_bounds__(kBlock) void mpass_init(int n, const int *__restrict__ mark, const int *__restrict__ cmap,
                                                     int nc, int *__restrict__ pass, int *__restrict__ len,
                                                     int *__restrict__ off, int *__restrict__ pcol,
                                                     double *__restrict__ pval)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int c = mark[i] == CGPT ? cmap[i] : -1;
    const bool coarse = (unsigned)c < (unsigned)nc;
    pass[i] = coarse ? 0 : -1;
    len[i] = coarse ? 1 : 0;
    off[i] = coarse ? c : 0;
    if (coarse) {
        pcol[c] = i;
        pval[c] = 1.0;
    }
}

// sweep p: an F point without a number that has a neighbour numbered p - 1 gets p (a reader of pass[]
// sees -1 or p there, never p - 1); stat[0] counts the points numbered
__global__ __launch_bounds__(kBlock) void mpass_relax(Csr S, const int *__restrict__ mark, int *pass, int p,
                                                      unsigned long long *__restrict__ stat)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool hit = false;
    if (i < S.n && mark[i] == FGPT && pass[i] == -1) {
        int lo, hi;
        span(S, i, lo, hi);
        for (int q = lo; q < hi && !hit; ++q) {
            const int k = S.ci[q];
            hit = (unsigned)k < (unsigned)S.n && k != i && pass[k] == p - 1;
        }
        if (hit) pass[i] = p;
    }
    const unsigned long long b = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&stat[0], (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(kBlock) void mpass_select(int n, const int *__restrict__ pass, int p, int *__restrict__ flag)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i <= n) flag[i] = i < n && pass[i] == p;
}

__global__ __launch_bounds__(kBlock) void mpass_scatter(int n, const int *__restrict__ pass, int p,
                                                        const int *__restrict__ pos, int cnt, int *__restrict__ rows)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n && pass[i] == p && (unsigned)pos[i] < (unsigned)cnt) rows[pos[i]] = i;
}

// whether the stored entry (i, k) of A has k in N_i: k != i, in S_i, of the pass before
__device__ __forceinline__ bool mpass_in_n(const Csr &S, int slo, int shi, const int *__restrict__ pass, int i, int k,
                                           int p)
{
    if (k == i || pass[k] != p - 1) return false;
    for (int q = slo; q < shi; ++q)
        if (S.ci[q] == k) return true;
    return false;
}

// the block of the pass before: row k of P at off[k], len[k] entries (checked against the block)
struct PrevBlock {
    const int *len, *off, *col;
    const double *val;
    int nnz;
};
__device__ __forceinline__ bool prev_row(const PrevBlock &B, int k, int &o, int &l, int *err)
{
    o = B.off[k], l = B.len[k];
    if (o < 0 || l < 0 || (long long)o + l > B.nnz) {
        atomicOr(err, kErrIndex);
        return false;
    }
    return true;
}

// candidate bound of the rows of a pass (the rows of P of N_i, one after the other); stat[1] their sum
__global__ __launch_bounds__(kBlock) void mpass_bound(Csr A, Csr S, const int *__restrict__ pass, PrevBlock B,
                                                      const int *__restrict__ rows, int cnt, int p, int *__restrict__ need,
                                                      unsigned long long *__restrict__ stat, int *__restrict__ ctr)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    long long b = 0;
    if (t < cnt) {
        const int i = rows[t];
        int lo, hi, slo, shi;
        span(A, i, lo, hi);
        span(S, i, slo, shi);
        for (int j = lo; j < hi; ++j) {
            const int k = A.ci[j];
            if ((unsigned)k >= (unsigned)A.n) continue;   // flagged by mpass_check_rows
            int o, l;
            if (mpass_in_n(S, slo, shi, pass, i, k, p) && prev_row(B, k, o, l, &ctr[0])) b += l;
        }
        if (b > kMaxBound) {
            atomicOr(&ctr[0], kErrBound);
            b = 0;
        }
        need[t] = (int)b;
    }
    unsigned long long sum = (unsigned long long)b;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&stat[1], sum);
}

// the capacity of every row's global table (0: in LDS) and the rows that have one
__global__ __launch_bounds__(kBlock) void mpass_gcap(int cnt, int slots, const int *__restrict__ need,
                                                     long long *__restrict__ gcap, int *__restrict__ ctr)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t > cnt) return;
    const bool glob = t < cnt && need[t] > slots;
    gcap[t] = glob ? tab_cap(need[t]) : 0;
    if (glob) atomicAdd(&ctr[1], 1);
}

// One walk over the candidates of row i of pass p in discovery order; CLAIM and FILL as pattern_walk.
template <int G, bool CLAIM, bool FILL>
__device__ __forceinline__ int mpass_walk(const Csr &A, const Csr &S, const int *__restrict__ pass, const PrevBlock &B, int i,
                                          int p, int gl, int *key, int *seq, int cap, int *out, int room, int *err)
{
    int lo, hi, slo, shi, base = 0, kept = 0;
    span(A, i, lo, hi);
    span(S, i, slo, shi);
    for (int j = lo; j < hi; ++j) {
        const int k = A.ci[j];
        int ko, kl;
        if ((unsigned)k >= (unsigned)A.n || !mpass_in_n(S, slo, shi, pass, i, k, p) || !prev_row(B, k, ko, kl, err)) continue;
        for (int r0 = 0; r0 < kl; r0 += G) {
            const int r = r0 + gl;
            int h = -1;
            if (r < kl) {
                h = B.col[ko + r];
                if ((unsigned)h >= (unsigned)A.n) {
                    atomicOr(err, kErrIndex);
                    h = -1;
                }
            }
            const int s = base + r;
            if (CLAIM) {
                if (h >= 0) {
                    const int slot = tab_insert(key, cap, h);
                    if (slot < 0) atomicOr(err, kErrTableFull);
                    else atomicMin(&seq[slot], s);
                }
            } else {
                bool own = false;
                if (h >= 0) {
                    const int slot = tab_find(key, cap, h);
                    if (slot < 0) atomicOr(err, kErrTableFull);
                    else own = seq[slot] == s;
                }
                const unsigned long long m = group_ballot<G>(own, gl);
                if (FILL && own) {
                    const int o = kept + __popcll(m & ((1ull << gl) - 1ull));
                    if (o < room) out[o] = h;
                }
                kept += __popcll(m);
            }
        }
        base += kl;
    }
    return kept;
}

// The rows of pass p, G lanes per row.  FILL false: the pattern lengths into cnt[t].  FILL true: the
// pattern and the weights into the pass's block at boff[t], and the row's len and off for the next pass.
template <int G, bool FILL>
__global__ __launch_bounds__(kBlock) void mpass_rows(Csr A, Csr S, const int *__restrict__ pass, PrevBlock B,
                                                     const int *__restrict__ rows, int nrows, int p, int slots,
                                                     const int *__restrict__ need, const long long *__restrict__ goff,
                                                     int *__restrict__ gkey, int *__restrict__ gseq, double *__restrict__ gacc,
                                                     int *__restrict__ cnt, const int *__restrict__ boff, int bnnz,
                                                     int *__restrict__ bcol, double *__restrict__ bval, int *len, int *off,
                                                     int *__restrict__ err)
{
    __shared__ int lkey[kLdsSlots], lseq[kLdsSlots];
    __shared__ double lacc[FILL ? kLdsSlots : 1];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (kBlock / G) + grp;
    const int t = row < nrows ? (int)row : -1;
    int i = t >= 0 ? rows[t] : -1;
    if ((unsigned)i >= (unsigned)A.n) i = -1;
    int *key = nullptr, *seq = nullptr, cap = 0;
    double *acc = nullptr;
    if (i >= 0) {
        long long toff;
        cap = row_table(t, grp, slots, need, goff, lkey, gkey, key, toff);
        seq = toff >= 0 ? gseq + toff : lseq + (-1 - toff);
        if (FILL) acc = toff >= 0 ? gacc + toff : lacc + (-1 - toff);
        for (int s = gl; s < cap; s += G) {
            key[s] = -1;
            seq[s] = INT_MAX;
            if (FILL) acc[s] = 0.0;
        }
    }
    __syncthreads();
    if (i >= 0) mpass_walk<G, true, false>(A, S, pass, B, i, p, gl, key, seq, cap, nullptr, 0, err);
    __syncthreads();
    int o = 0, room = 0;
    if (i >= 0) {
        if (FILL) {
            o = max(boff[t], 0);
            room = max(min(boff[t + 1], bnnz) - o, 0);
        }
        const int kept = mpass_walk<G, false, FILL>(A, S, pass, B, i, p, gl, key, seq, cap, bcol + o, room, err);
        if (FILL) {
            if (kept != room && gl == 0) atomicOr(err, kErrPatternCol);
        } else if (gl == 0) {
            cnt[t] = kept;
        }
    }
    if (!FILL) return;
    __syncthreads();
    double d = 0.0, tot = 0.0, sub = 0.0;
    if (i >= 0) {
        int lo, hi, slo, shi;
        span(A, i, lo, hi);
        span(S, i, slo, shi);
        for (int j = lo; j < hi; ++j) {
            const int k = A.ci[j];
            if ((unsigned)k >= (unsigned)A.n) continue;   // flagged by mpass_check_rows
            const double a = A.v[j];
            if (k == i) {
                d = a;
                continue;
            }
            tot += a;
            int ko, kl;
            if (!mpass_in_n(S, slo, shi, pass, i, k, p)) continue;
            sub += a;
            if (!prev_row(B, k, ko, kl, err)) continue;
            for (int r0 = 0; r0 < kl; r0 += G) {
                const int r = r0 + gl;
                int slot = -1;
                double prod = 0.0;
                if (r < kl) {
                    const int c = B.col[ko + r];
                    if ((unsigned)c < (unsigned)A.n) {
                        slot = tab_find(key, cap, c);
                        if (slot < 0) atomicOr(err, kErrPatternCol);
                        prod = a * B.val[ko + r];
                    }
                }
                // handed to the owners in walk order: lane u's term is applied before lane u + 1's
                const int nl = min(G, kl - r0);
                for (int u = 0; u < nl; ++u) {
                    const int su = __shfl(slot, u, G);
                    const double vu = __shfl(prod, u, G);
                    if (su >= 0 && (su & (G - 1)) == gl) acc[su] += vu;
                }
            }
        }
    }
    __syncthreads();
    if (i >= 0) {
        const bool zero = sub == 0.0 || d == 0.0;
        const double f = zero ? 0.0 : tot / sub;
        for (int q = gl; q < room; q += G) {
            const int c = bcol[o + q];
            const int slot = (unsigned)c < (unsigned)A.n ? tab_find(key, cap, c) : -1;
            if (slot >= 0) bval[o + q] = zero ? 0.0 : -(f * acc[slot]) / d;
        }
        if (gl == 0) {
            len[i] = room;
            off[i] = o;
        }
    }
}

// P in row order (fine columns) from the blocks: row i of pass q is in block q at off[i]
__global__ __launch_bounds__(kBlock) void mpass_assemble(int n, const int *__restrict__ pass, const int *__restrict__ len,
                                                         const int *__restrict__ off, int nblocks,
                                                         const int *const *__restrict__ bcol,
                                                         const double *const *__restrict__ bval,
                                                         const int *__restrict__ bnnz, const int *__restrict__ prp, int pnnz,
                                                         int *__restrict__ pci, double *__restrict__ pv, int *__restrict__ err)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int l = len[i], b = pass[i];
    if (l <= 0) return;
    const int o = off[i], w = prp[i];
    if ((unsigned)b >= (unsigned)nblocks || o < 0 || (long long)o + l > bnnz[b] || w < 0 || (long long)w + l > pnnz) {
        atomicOr(err, kErrIndex);
        return;
    }
    for (int q = 0; q < l; ++q) {
        pci[w + q] = bcol[b][o + q];
        pv[w + q] = bval[b][o + q];
    }
}

// step 0 of interp_STD for the F rows: the row's last diagonal entry, and in stored order the sums of
// the strong-C entries, of the off-diagonal entries and of those whose column is not isolated
__global__ __launch_bounds__(kBlock) void weights_sums(Csr A, Csr S, const int *__restrict__ mark, double *__restrict__ diag,
                                                       double *__restrict__ csum, double *__restrict__ nsum,
                                                       double *__restrict__ psum, int *__restrict__ err)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n || mark[i] != FGPT) return;
    int lo, hi, slo, shi;
    span(A, i, lo, hi);
    span(S, i, slo, shi);
    double cs = 0.0, ns = 0.0, ps = 0.0, d = 0.0;
    for (int j = lo; j < hi; ++j) {
        const int k = A.ci[j];
        if ((unsigned)k >= (unsigned)A.n) {
            atomicOr(err, kErrIndex);
            continue;
        }
        const int mk = mark[k];
        bool strong_c = false;
        if (mk == CGPT)
            for (int q = slo; q < shi && !strong_c; ++q) strong_c = S.ci[q] == k;
        const double a = A.v[j];
        if (strong_c) cs += a;
        if (k == i) {
            d = a;
        } else {
            ns += a;
            if (mk != ISPT) ps += a;
        }
    }
    diag[i] = d, csum[i] = cs, nsum[i] = ns, psum[i] = ps;
}

// position of the last entry of A's row [lo, hi) with column col, searched by the G lanes; -1 if none
template <int G>
__device__ __forceinline__ int group_find_last(const Csr &A, int lo, int hi, int col, int gl)
{
    int best = -1;
    for (int m = lo + gl; m < hi; m += G)
        if (A.ci[m] == col) best = m;
    for (int o = G / 2; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, G));
    return best;
}

// step 1 of interp_STD: the weights of the F rows on the pattern (fine column numbers), 1 for the C rows
template <int G>
__global__ __launch_bounds__(kBlock) void weights_rows(Csr A, Csr S, const int *__restrict__ mark, int slots,
                                                       const int *__restrict__ need, const long long *__restrict__ goff,
                                                       int *__restrict__ gkey, double *__restrict__ gacc,
                                                       const int *__restrict__ prp, int pnnz, const int *__restrict__ pci,
                                                       double *__restrict__ pv, const double *__restrict__ diag,
                                                       const double *__restrict__ csum, const double *__restrict__ nsum,
                                                       const double *__restrict__ psum, int *__restrict__ err)
{
    __shared__ int lkey[kLdsSlots];
    __shared__ double lacc[kLdsSlots];
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (kBlock / G) + grp;
    const int i = row < A.n ? (int)row : -1;
    const int mi = i >= 0 ? mark[i] : UNPT;
    int *key = nullptr, cap = 0, plo = 0, phi = 0;
    double *acc = nullptr;
    if (mi == FGPT) {
        long long off;
        cap = row_table(i, grp, slots, need, goff, lkey, gkey, key, off);
        acc = off >= 0 ? gacc + off : lacc + (-1 - off);
        for (int s = gl; s < cap; s += G) {
            key[s] = -1;
            acc[s] = 0.0;
        }
        plo = max(prp[i], 0);
        phi = max(min(prp[i + 1], pnnz), plo);
    }
    __syncthreads();
    if (mi == FGPT)
        for (int j = plo + gl; j < phi; j += G) {
            const int c = pci[j];
            if ((unsigned)c >= (unsigned)A.n) atomicOr(err, kErrIndex);
            else if (tab_insert(key, cap, c) < 0) atomicOr(err, kErrTableFull);
        }
    __syncthreads();
    double ahat_i = 0.0, alN = 0.0, alP = 0.0;
    if (mi == FGPT) {
        int lo, hi, slo, shi;
        span(A, i, lo, hi);
        span(S, i, slo, shi);
        ahat_i = diag[i], alN = psum[i], alP = csum[i];
        for (int j = slo; j < shi; ++j) {
            const int k = S.ci[j];
            if ((unsigned)k >= (unsigned)A.n) {
                if (gl == 0) atomicOr(err, kErrIndex);
                continue;
            }
            const int pik = group_find_last<G>(A, lo, hi, k, gl);
            if (pik < 0) {
                if (gl == 0) atomicOr(err, kErrStrongCol);
                continue;
            }
            const double aik = A.v[pik];
            const int mk = mark[k];
            if (mk == CGPT) {
                const int slot = tab_find(key, cap, k);
                if (slot < 0) {
                    if (gl == 0) atomicOr(err, kErrPatternCol);
                } else if ((slot & (G - 1)) == gl) {
                    acc[slot] += aik;
                }
            } else if (mk == FGPT) {
                int klo, khi, sklo, skhi;
                span(A, k, klo, khi);
                span(S, k, sklo, skhi);
                const double akk = diag[k], factor = aik / akk;
                double aki = 0.0;
                for (int m = klo; m < khi; ++m)
                    if (A.ci[m] == i) {
                        aki = A.v[m];
                        ahat_i -= factor * aki;
                    }
                for (int m0 = sklo; m0 < skhi; m0 += G) {
                    const int m = m0 + gl;
                    int slot = -1;
                    double prod = 0.0;
                    if (m < skhi) {
                        const int l = S.ci[m];
                        if ((unsigned)l >= (unsigned)A.n) {
                            atomicOr(err, kErrIndex);
                        } else {
                            int pkl = -1;   // the last entry of row k with column l
                            for (int t = klo; t < khi; ++t)
                                if (A.ci[t] == l) pkl = t;
                            if (pkl < 0) {
                                atomicOr(err, kErrStrongCol);
                            } else if (mark[l] == CGPT) {
                                slot = tab_find(key, cap, l);
                                if (slot < 0) atomicOr(err, kErrPatternCol);
                                prod = factor * A.v[pkl];
                            }
                        }
                    }
                    if (group_ballot<G>(slot >= 0, gl) == 0ull) continue;
                    // handed to the owners in stored order: lane t's term is applied before lane t + 1's
                    const int cnt = min(G, skhi - m0);
                    for (int t = 0; t < cnt; ++t) {
                        const int st = __shfl(slot, t, G);
                        const double vt = __shfl(prod, t, G);
                        if (st >= 0 && (st & (G - 1)) == gl) acc[st] -= vt;
                    }
                }
                alN -= factor * (nsum[k] - aki + akk);
                alP -= factor * csum[k];
            }
        }
    }
    __syncthreads();
    if (mi == FGPT) {
        double alpha = 0.0;
        if (phi > plo) alpha = alN / alP;
        for (int j = plo + gl; j < phi; j += G) {
            const int c = pci[j];
            const int slot = (unsigned)c < (unsigned)A.n ? tab_find(key, cap, c) : -1;
            if (slot >= 0) pv[j] = -alpha * acc[slot] / ahat_i;
        }
    } else if (mi == CGPT && gl == 0) {
        const int o = prp[i];
        if ((unsigned)o < (unsigned)pnnz) pv[o] = 1.0;
    }
}

// the last diagonal entry of every row (0 when it has none): a_ii of interp_EXTI
__global__ __launch_bounds__(kBlock) void exti_diag(Csr A, double *__restrict__ diag)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n) return;
    int lo, hi;
    span(A, i, lo, hi);
    double d = 0.0;
    for (int j = lo; j < hi; ++j)
        if (A.ci[j] == i) d = A.v[j];
    diag[i] = d;
}

// One pass of the group over row k of A for F row i: lane gl takes entry m0 + gl.  An entry (k, l)
// qualifies when l != k, l == i or l is in the table of row i, and a_kl a_kk < 0.  Returns the group's
// mask of qualifying lanes; val, slot (-1 for l == i) of this lane's entry.
template <int G>
__device__ __forceinline__ unsigned long long exti_chunk(const Csr &A, int i, int k, double akk, int m0, int khi, int gl,
                                                         const int *key, int cap, double &val, int &slot, int *err)
{
    const int m = m0 + gl;
    bool q = false;
    val = 0.0, slot = -1;
    if (m < khi) {
        const int l = A.ci[m];
        if ((unsigned)l >= (unsigned)A.n) {
            atomicOr(err, kErrIndex);
        } else if (l != k) {
            val = A.v[m];
            if (l == i) q = true;
            else q = (slot = tab_find(key, cap, l)) >= 0;
            q = q && val * akk < 0;
        }
    }
    return group_ballot<G>(q, gl);
}

// interp_EXTI: the weights of the F rows on the pattern (fine column numbers), 1 for the C rows.  The
// stored entries of row i are classified G at a time and applied in stored order; a strong F neighbour
// k has row k of A walked twice by the group (den, then f a_kl to the owners or to d), the qualifying
// entries of a chunk taken lane by lane in stored order.  d and den are computed by every lane of the
// group from the same values in the same order.
template <int G>
__global__ __launch_bounds__(kBlock) void exti_rows(Csr A, Csr S, const int *__restrict__ mark, int slots,
                                                    const int *__restrict__ need, const long long *__restrict__ goff,
                                                    int *__restrict__ gkey, double *__restrict__ gacc,
                                                    const int *__restrict__ prp, int pnnz, const int *__restrict__ pci,
                                                    double *__restrict__ pv, const double *__restrict__ diag,
                                                    int *__restrict__ err)
{
    __shared__ int lkey[kLdsSlots];
    __shared__ double lacc[kLdsSlots];
    enum { kSkip = 0, kDirect = 1, kStrongF = 2, kDiag = 3 };
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (kBlock / G) + grp;
    const int i = row < A.n ? (int)row : -1;
    const int mi = i >= 0 ? mark[i] : UNPT;
    int *key = nullptr, cap = 0, plo = 0, phi = 0;
    double *acc = nullptr;
    if (mi == FGPT) {
        plo = max(prp[i], 0);
        phi = max(min(prp[i + 1], pnnz), plo);
    }
    const bool frow = mi == FGPT && phi > plo;   // an F row with an empty pattern gets nothing
    if (frow) {
        long long off;
        cap = row_table(i, grp, slots, need, goff, lkey, gkey, key, off);
        acc = off >= 0 ? gacc + off : lacc + (-1 - off);
        for (int s = gl; s < cap; s += G) {
            key[s] = -1;
            acc[s] = 0.0;
        }
    }
    __syncthreads();
    if (frow)
        for (int j = plo + gl; j < phi; j += G) {
            const int c = pci[j];
            if ((unsigned)c >= (unsigned)A.n) atomicOr(err, kErrIndex);
            else if (tab_insert(key, cap, c) < 0) atomicOr(err, kErrTableFull);
        }
    __syncthreads();
    double d = 0.0;
    if (frow) {
        int lo, hi, slo, shi;
        span(A, i, lo, hi);
        span(S, i, slo, shi);
        d = diag[i];
        // consistent input has every strong column in the row of A
        for (int q = slo; q < shi; ++q) {
            const int k = S.ci[q];
            if ((unsigned)k >= (unsigned)A.n) {
                if (gl == 0) atomicOr(err, kErrIndex);
            } else if (group_find_last<G>(A, lo, hi, k, gl) < 0 && gl == 0) {
                atomicOr(err, kErrStrongCol);
            }
        }
        for (int j0 = lo; j0 < hi; j0 += G) {
            const int j = j0 + gl;
            int cls = kSkip, k = -1, slot = -1;
            double a = 0.0;
            if (j < hi) {
                k = A.ci[j];
                if ((unsigned)k >= (unsigned)A.n) {
                    atomicOr(err, kErrIndex);
                } else if (k != i) {
                    a = A.v[j];
                    slot = tab_find(key, cap, k);
                    cls = kDiag;
                    if (slot >= 0) {
                        cls = kDirect;
                    } else if (mark[k] == FGPT) {
                        for (int q = slo; q < shi; ++q)
                            if (S.ci[q] == k) cls = kStrongF;
                    }
                }
            }
            const int cnt = min(G, hi - j0);
            for (int t = 0; t < cnt; ++t) {
                const int ct = __shfl(cls, t, G);
                if (ct == kSkip) continue;
                const double at = __shfl(a, t, G);
                if (ct == kDirect) {
                    const int st = __shfl(slot, t, G);
                    if ((st & (G - 1)) == gl) acc[st] += at;
                } else if (ct == kDiag) {
                    d += at;
                } else {
                    const int kt = __shfl(k, t, G);
                    const double akk = diag[kt];
                    int klo, khi, sl;
                    double val, den = 0.0;
                    span(A, kt, klo, khi);
                    for (int m0 = klo; m0 < khi; m0 += G) {
                        unsigned long long b = exti_chunk<G>(A, i, kt, akk, m0, khi, gl, key, cap, val, sl, err);
                        for (; b; b &= b - 1) den += __shfl(val, __ffsll((long long)b) - 1, G);
                    }
                    if (den != 0.0) {
                        const double f = at / den;
                        for (int m0 = klo; m0 < khi; m0 += G) {
                            unsigned long long b = exti_chunk<G>(A, i, kt, akk, m0, khi, gl, key, cap, val, sl, err);
                            for (; b; b &= b - 1) {
                                const int u = __ffsll((long long)b) - 1;
                                const double tt = f * __shfl(val, u, G);
                                const int su = __shfl(sl, u, G);
                                if (su < 0) d += tt;
                                else if ((su & (G - 1)) == gl) acc[su] += tt;
                            }
                        }
                    } else {
                        d += at;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (frow) {
        for (int j = plo + gl; j < phi; j += G) {
            const int c = pci[j];
            const int slot = (unsigned)c < (unsigned)A.n ? tab_find(key, cap, c) : -1;
            if (slot >= 0) pv[j] = -acc[slot] / d;
        }
    } else if (mi == CGPT && gl == 0) {
        const int o = prp[i];
        if ((unsigned)o < (unsigned)pnnz) pv[o] = 1.0;
    }
}

__global__ __launch_bounds__(kBlock) void flag_coarse(int n, const int *__restrict__ mark, int *__restrict__ flag)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i <= n) flag[i] = i < n && mark[i] == CGPT;
}

__global__ __launch_bounds__(kBlock) void renumber(int nnz, int n, const int *__restrict__ cmap, int *__restrict__ ci,
                                                   int *__restrict__ err)
{
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= nnz) return;
    const int c = ci[q];
    if ((unsigned)c < (unsigned)n) ci[q] = cmap[c];
    else atomicOr(err, kErrIndex);
}

// interp_trunc_par, one row per lane (the sums of a row are in stored order): FILL false counts the
// kept entries of every row into cnt, FILL true writes them at nrp
template <bool FILL>
__global__ __launch_bounds__(kBlock) void trunc_rows(int n, int pnnz, const int *__restrict__ prp, const int *__restrict__ pci,
                                                     const double *__restrict__ pv, double eps, int *__restrict__ cnt,
                                                     const int *__restrict__ nrp, int kept, int *__restrict__ nci,
                                                     double *__restrict__ nv)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int lo = max(prp[i], 0), hi = max(min(prp[i + 1], pnnz), lo);
    double pos_max = 0, neg_min = 0, pos_sum = 0, neg_sum = 0, pos_kept = 0, neg_kept = 0;
    for (int k = lo; k < hi; ++k) {
        const double v = pv[k];
        if (v > 0) {
            pos_sum += v;
            pos_max = pos_max > v ? pos_max : v;
        } else if (v < 0) {
            neg_sum += v;
            neg_min = neg_min < v ? neg_min : v;
        }
    }
    pos_max *= eps;
    neg_min *= eps;
    if (!FILL) {
        int c = 0;
        for (int k = lo; k < hi; ++k) c += (pv[k] >= pos_max) || (pv[k] <= neg_min);
        cnt[i] = c;
        return;
    }
    const int o0 = max(nrp[i], 0), room = min(nrp[i + 1], kept) - o0;
    int o = 0;
    for (int k = lo; k < hi && o < room; ++k) {
        const double v = pv[k];
        if (v >= pos_max) {
            nci[o0 + o++] = pci[k];
            pos_kept += v;
        } else if (v <= neg_min) {
            nci[o0 + o++] = pci[k];
            neg_kept += v;
        }
    }
    const double pos_fac = pos_kept > SMALLFLOAT ? pos_sum / pos_kept : 1.0;
    const double neg_fac = neg_kept < -SMALLFLOAT ? neg_sum / neg_kept : 1.0;
    o = 0;
    for (int k = lo; k < hi && o < room; ++k) {
        const double v = pv[k];
        if (v >= pos_max) nv[o0 + o++] = v * pos_fac;
        else if (v <= neg_min) nv[o0 + o++] = v * neg_fac;
    }
}

// The truncation with the cap on the entries per row (pmax > 0; the rule: amg_amd/host/sss_setup.c
// trunc_cut and interp_trunc_par), G lanes per row.  The thresholds and the number of
// survivors come from strided walks and shuffle reductions (max, min and a count do not depend on
// order).  A row with more than pmax survivors is cut in pmax rounds: each round is the group-wide
// arg-max of the key (|v|, then the smaller position) over the survivors strictly after the previous
// round's pick in that order, every lane over its stride and then log2 G shuffle steps; the last pick is
// the cut.  Nothing is kept per entry and no array is indexed per lane.  What the host sums in stored
// order (pos_sum, neg_sum, pos_kept, neg_kept) every lane of the group sums in stored order from the
// same values, G loaded at a time and handed round by shuffles.  FILL false: the kept count into cnt[i].
// FILL true: the kept entries in stored order at nrp[i], offsets from an in-order ballot of the group.
// Loops are bounded by the row length or pmax; writes are bounded by the row's room in the new arrays.
__device__ __forceinline__ bool trunc_kept(double v, int k, double tp, double tn, bool capped, double cut_a, int cut_k)
{
    const double a = fabs(v);
    return (v >= tp || v <= tn) && (!capped || a > cut_a || (a == cut_a && k <= cut_k));
}

template <int G, bool FILL>
__global__ __launch_bounds__(kBlock) void trunc_rows_cap(int n, int pnnz, const int *__restrict__ prp,
                                                         const int *__restrict__ pci, const double *__restrict__ pv,
                                                         double eps, int pmax, int *__restrict__ cnt,
                                                         const int *__restrict__ nrp, int kept, int *__restrict__ nci,
                                                         double *__restrict__ nv)
{
    const int grp = threadIdx.x / G, gl = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (kBlock / G) + grp;
    if (row >= n) return;   // the whole group leaves
    const int i = (int)row;
    const int lo = max(prp[i], 0), hi = max(min(prp[i + 1], pnnz), lo);
    // thresholds
    double tp = 0, tn = 0;
    for (int k = lo + gl; k < hi; k += G) {
        const double v = pv[k];
        if (v > 0) tp = tp > v ? tp : v;
        else if (v < 0) tn = tn < v ? tn : v;
    }
    for (int o = G / 2; o > 0; o >>= 1) {
        const double a = __shfl_xor(tp, o, G), b = __shfl_xor(tn, o, G);
        tp = tp > a ? tp : a;
        tn = tn < b ? tn : b;
    }
    tp *= eps;
    tn *= eps;
    // survivors
    int ns = 0;
    for (int k = lo + gl; k < hi; k += G) ns += (pv[k] >= tp) || (pv[k] <= tn);
    for (int o = G / 2; o > 0; o >>= 1) ns += __shfl_xor(ns, o, G);
    const bool capped = ns > pmax;
    if (!FILL) {
        if (gl == 0) cnt[i] = capped ? pmax : ns;
        return;
    }
    // the cut of a capped row: pmax rounds
    double cut_a = 0.0;
    int cut_k = -1;
    if (capped) {
        for (int r = 0; r < pmax; ++r) {
            double ba = -1.0;
            int bk = -1;
            for (int k = lo + gl; k < hi; k += G) {
                const double v = pv[k], a = fabs(v);
                if (!(v >= tp || v <= tn)) continue;
                if (r > 0 && !(a < cut_a || (a == cut_a && k > cut_k))) continue;   // picked by an earlier round
                if (a > ba) ba = a, bk = k;   // k grows: on ties the earlier position stays
            }
            for (int o = G / 2; o > 0; o >>= 1) {
                const double oa = __shfl_xor(ba, o, G);
                const int ok = __shfl_xor(bk, o, G);
                if (ok >= 0 && (bk < 0 || oa > ba || (oa == ba && ok < bk))) ba = oa, bk = ok;
            }
            if (bk < 0) break;   // the same on every lane
            cut_a = ba;
            cut_k = bk;
        }
    }
    // pos_sum and neg_sum in stored order; the kept columns and pos_kept, neg_kept in stored order
    const int o0 = max(nrp[i], 0), room = min(nrp[i + 1], kept) - o0;
    double pos_sum = 0, neg_sum = 0, pos_kept = 0, neg_kept = 0;
    int o = 0;
    for (int k0 = lo; k0 < hi; k0 += G) {
        const int k = k0 + gl, m = min(G, hi - k0);
        const double v = k < hi ? pv[k] : 0.0;
        for (int t = 0; t < m; ++t) {
            const double vt = __shfl(v, t, G);
            if (vt > 0) pos_sum += vt;
            else if (vt < 0) neg_sum += vt;
        }
        const bool keep = k < hi && trunc_kept(v, k, tp, tn, capped, cut_a, cut_k);
        const unsigned long long mask = group_ballot<G>(keep, gl);
        if (keep) {
            const int w = o + __popcll(mask & ((1ull << gl) - 1ull));
            if (w < room) nci[o0 + w] = pci[k];
        }
        for (unsigned long long b = mask; b; b &= b - 1) {
            const double vt = __shfl(v, __ffsll((long long)b) - 1, G);
            if (vt >= tp) pos_kept += vt;
            else neg_kept += vt;
        }
        o += __popcll(mask);
    }
    const bool pos_has = pos_kept > SMALLFLOAT, neg_has = neg_kept < -SMALLFLOAT;
    double pos_fac = pos_has ? pos_sum / pos_kept : 1.0;
    double neg_fac = neg_has ? neg_sum / neg_kept : 1.0;
    if (capped) {
        // a class the cap removed entirely hands its sum to the other one
        if (pos_sum > 0 && !pos_has && neg_has) neg_fac = (pos_sum + neg_sum) / neg_kept;
        if (neg_sum < 0 && !neg_has && pos_has) pos_fac = (pos_sum + neg_sum) / pos_kept;
    }
    o = 0;
    for (int k0 = lo; k0 < hi; k0 += G) {
        const int k = k0 + gl;
        const double v = k < hi ? pv[k] : 0.0;
        const bool keep = k < hi && trunc_kept(v, k, tp, tn, capped, cut_a, cut_k);
        const unsigned long long mask = group_ballot<G>(keep, gl);
        if (keep) {
            const int w = o + __popcll(mask & ((1ull << gl) - 1ull));
            if (w < room) nv[o0 + w] = v >= tp ? v * pos_fac : v * neg_fac;
        }
        o += __popcll(mask);
    }
}

int copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind k, hipStream_t st)
{
    if (bytes == 0) return 0;
    SSS_HIP(hipMemcpyAsync(dst, src, bytes, k, st));
    SSS_HIP(hipStreamSynchronize(st));
    return 0;
}

// lanes per row from the average row of S: an F row has about avg + avg^2 / 2 candidates, and a group
// of G lanes has 8 G table slots in LDS (SSS_HIP_INTERP_LANES, tests: 1, 4, 16 or 64 whatever the rows)
int lanes_for_candidates(double est)
{
    const char *e = getenv("SSS_HIP_INTERP_LANES");
    if (e && *e) {
        const int g = atoi(e);
        if (g == 1 || g == 4 || g == 16 || g == 64) return g;
    }
    return est <= 4.0 ? 1 : est <= 16.0 ? 4 : est <= 64.0 ? 16 : 64;
}
int lanes_for(int n, int snnz)
{
    const double avg = (double)snnz / (double)std::max(n, 1);
    return lanes_for_candidates(avg * (1.0 + 0.5 * avg));
}

// table slots of one group in LDS, a power of two (SSS_HIP_INTERP_LDS_SLOTS lowers it: the tests
// reach the global tables at small shapes)
int slots_for(int G)
{
    int slots = kLdsSlots / (kBlock / G);
    const char *e = getenv("SSS_HIP_INTERP_LDS_SLOTS");
    if (e && *e) {
        const int want = std::max(atoi(e), 2);
        while (slots > want) slots >>= 1;
    }
    return slots;
}

struct Dev {
    hipStream_t st = nullptr;
    std::vector<void *> mem;
    double t_copy = 0.0, t_kern = 0.0, t_last = PhaseTimer::now();
    double t_trunc = 0.0;        // seconds of the truncation, when it was timed
    int cap = 0, cap_lanes = 0;  // the cap on the entries per row the truncation ran with, its lanes per row
    bool trunc_timed = false;
    bool oom = false;
    ~Dev()
    {
        for (void *p : mem) dev_free(p);
        if (st) (void)hipStreamDestroy(st);
    }
    template <class T>
    T *alloc(size_t count)
    {
        T *p = dev_alloc<T>(count);
        if (p) mem.push_back(p);
        else oom = true;
        return p;
    }
    template <class T>
    T *upload(const T *src, size_t count)
    {
        T *p = alloc<T>(count);
        if (p && count && h2d(p, src, sizeof(T) * count)) oom = true;
        return p;
    }
    // frees what was allocated since mem held `from` arrays, but for the arrays of `keep`
    void free_from(size_t from, std::initializer_list<void *> keep)
    {
        std::vector<void *> kept;
        for (size_t q = from; q < mem.size(); ++q) {
            if (std::find(keep.begin(), keep.end(), mem[q]) != keep.end()) kept.push_back(mem[q]);
            else dev_free(mem[q]);
        }
        mem.resize(from);
        mem.insert(mem.end(), kept.begin(), kept.end());
    }
    // the time since the last call goes to the copies or to the kernels
    void lap(bool copy)
    {
        const double t = PhaseTimer::now();
        (copy ? t_copy : t_kern) += t - t_last;
        t_last = t;
    }
};

template <class T>
int exclusive_sum(Dev &d, const T *in, T *out, size_t count)
{
    size_t bytes = 0;
    SSS_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, out, (int)count, d.st));
    void *tmp = d.alloc<char>(bytes);
    if (!tmp) return hip_fail(hipErrorOutOfMemory, "hipMalloc(scan)", __FILE__, __LINE__);
    SSS_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, (int)count, d.st));
    return 0;
}

int check_s(const SSS_IMAT *S, const int *mark)
{
    if (!S || !mark || S->num_rows <= 0 || !S->row_ptr) return ERROR_INPUT_PAR;
    const int n = S->num_rows, nnz = S->row_ptr[n];
    if (S->row_ptr[0] != 0 || nnz < 0 || (nnz > 0 && !S->col_idx)) return ERROR_INPUT_PAR;
    // n * 64 lanes must fit the grid (2^31 - 1 blocks)
    if ((long long)n * 64 / kBlock >= 0x7fffffffLL) return ERROR_MAT_SIZE;
    return 0;
}

int flag_error(const char *what, int flags)
{
    fprintf(stderr, "[sss_hip] %s: inconsistent input (%s%s%s%s%s)\n", what, flags & kErrIndex ? " index out of range" : "",
            flags & kErrStrongCol ? " strong column absent from the row of A" : "",
            flags & kErrPatternCol ? " C column absent from the pattern row" : "", flags & kErrTableFull ? " table full" : "",
            flags & kErrBound ? " row too long" : "");
    return ERROR_DATA_STRUCTURE;
}

// What both entry points share: S and the marks uploaded, the rows' table needs and global tables.
struct Tables {
    Csr S{};
    int *mark = nullptr, *need = nullptr, *ctr = nullptr, *gkey = nullptr;
    long long *goff = nullptr, total = 0;
    int G = 1, slots = 2, global_rows = 0;
};

unsigned grid_for(long long items) { return (unsigned)((items + kBlock - 1) / kBlock); }

int read_flags(Dev &d, const Tables &t, const char *what, int *h_ctr)
{
    SSS_HIP(hipGetLastError());
    if (copy_sync(h_ctr, t.ctr, sizeof(int) * 2, hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    return h_ctr[0] ? flag_error(what, h_ctr[0]) : 0;
}

int make_tables(Dev &d, Tables &t, const SSS_IMAT *S, const int *mark, const int *d_prp, int pnnz, const char *what)
{
    const int n = S->num_rows, nnz = S->row_ptr[n];
    t.S.n = n, t.S.nnz = nnz, t.S.v = nullptr;
    t.S.rp = d.upload(S->row_ptr, (size_t)n + 1);
    t.S.ci = d.upload(S->col_idx, (size_t)nnz);
    t.mark = d.upload(mark, (size_t)n);
    t.need = d.alloc<int>((size_t)n);
    t.ctr = d.alloc<int>(2);
    long long *gcap = d.alloc<long long>((size_t)n + 1);
    t.goff = d.alloc<long long>((size_t)n + 1);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(interpolation tables)", __FILE__, __LINE__);
    d.lap(true);
    t.G = lanes_for(n, nnz);
    t.slots = slots_for(t.G);
    SSS_HIP(hipMemsetAsync(t.ctr, 0, sizeof(int) * 2, d.st));
    SSS_HIP(hipMemsetAsync(gcap + n, 0, sizeof(long long), d.st));
    hipLaunchKernelGGL(interp_bound, dim3(grid_for(n)), dim3(kBlock), 0, d.st, t.S, t.mark, d_prp, pnnz, t.slots, t.need, gcap,
                       t.ctr);
    if (int rc = exclusive_sum(d, gcap, t.goff, (size_t)n + 1)) return rc;
    int h_ctr[2];
    if (int rc = read_flags(d, t, what, h_ctr)) return rc;
    if (copy_sync(&t.total, t.goff + n, sizeof(long long), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    t.global_rows = h_ctr[1];
    t.gkey = d.alloc<int>((size_t)t.total);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(global tables)", __FILE__, __LINE__);
    d.lap(false);
    return 0;
}

// what a timing line says about the cap on the entries per row: nothing unless the truncation was timed
// (in a setup: when SSS_SETUP_PMAX is set; set to 0 the cap is off and the note gives the uncapped seconds)
std::string cap_note(const Dev &d)
{
    if (!d.trunc_timed) return "";
    char buf[128];
    if (d.cap > 0) snprintf(buf, sizeof buf, ", cap %d at %d lanes per row, truncation %.4f s", d.cap, d.cap_lanes, d.t_trunc);
    else snprintf(buf, sizeof buf, ", no cap, truncation %.4f s", d.t_trunc);
    return buf;
}

void timing_line(const char *step, const Dev &d, const Tables &t, int rows, int nnz, const char *rule = "standard")
{
    if (getenv("SSS_SETUP_TIMING"))
        fprintf(stderr, "[setup]   %s P: device %s, %d rows, %d entries, %d lanes per row, %d rows on global tables, "
                        "copies %.4f s, kernels %.4f s%s\n", rule, step, rows, nnz, t.G, t.global_rows, d.t_copy, d.t_kern,
                cap_note(d).c_str());
}

template <class T>
struct HostArr {   // SSS_calloc'd, freed unless released into the result
    T *p;
    explicit HostArr(size_t count) : p((T *)SSS_calloc(std::max<size_t>(count, 1), sizeof(T))) {}
    ~HostArr() { free(p); }
    T *release()
    {
        T *q = p;
        p = nullptr;
        return q;
    }
};

}  // namespace

}  // namespace sss

using namespace sss;

// the row kernels at G lanes per row
#define SSS_INTERP_LAUNCH(kernel, ...)                                                                             \
    switch (G) {                                                                                                   \
    case 1: hipLaunchKernelGGL((kernel<1, ##__VA_ARGS__>), dim3(grid_for(n)), dim3(kBlock), 0, st, a...); break;   \
    case 4: hipLaunchKernelGGL((kernel<4, ##__VA_ARGS__>), dim3(grid_for(4LL * n)), dim3(kBlock), 0, st, a...); break;   \
    case 16: hipLaunchKernelGGL((kernel<16, ##__VA_ARGS__>), dim3(grid_for(16LL * n)), dim3(kBlock), 0, st, a...); break; \
    default: hipLaunchKernelGGL((kernel<64, ##__VA_ARGS__>), dim3(grid_for(64LL * n)), dim3(kBlock), 0, st, a...); break; \
    }
template <bool FILL, class... Args>
static void launch_pattern(int G, hipStream_t st, int n, Args... a)
{
    SSS_INTERP_LAUNCH(pattern_rows, FILL)
}
template <class... Args>
static void launch_weights(int G, hipStream_t st, int n, Args... a)
{
    SSS_INTERP_LAUNCH(weights_rows)
}
template <class... Args>
static void launch_exti(int G, hipStream_t st, int n, Args... a)
{
    SSS_INTERP_LAUNCH(exti_rows)
}
template <bool FILL, class... Args>
static void launch_agg(int G, hipStream_t st, int n, Args... a)
{
    SSS_INTERP_LAUNCH(agg_rows, FILL)
}
#undef SSS_INTERP_LAUNCH

extern "C" int sss_hip_agg_graph(const SSS_IMAT *S, const int *mark, SSS_IMAT *S2)
{
    const char *what = "aggressive S2";
    if (!S2) return ERROR_INPUT_PAR;
    if (int rc = check_s(S, mark)) return rc;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const int n = S->num_rows, nnz = S->row_ptr[n];
    Dev d;
    if (hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
    Tables t;
    t.S.n = n, t.S.nnz = nnz, t.S.v = nullptr;
    t.S.rp = d.upload(S->row_ptr, (size_t)n + 1);
    t.S.ci = d.upload(S->col_idx, (size_t)nnz);
    t.mark = d.upload(mark, (size_t)n);
    t.ctr = d.alloc<int>(2);
    int *flag = d.alloc<int>((size_t)n + 1), *cmap = d.alloc<int>((size_t)n + 1);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(aggressive S2)", __FILE__, __LINE__);
    d.lap(true);
    // the C numbering and the fine row of every C point
    int nc = 0, h_ctr[2];
    SSS_HIP(hipMemsetAsync(t.ctr, 0, sizeof(int) * 2, d.st));
    if (nnz > 0) hipLaunchKernelGGL(agg_check_cols, dim3(grid_for(nnz)), dim3(kBlock), 0, d.st, t.S, t.ctr);
    hipLaunchKernelGGL(flag_coarse, dim3(grid_for((long long)n + 1)), dim3(kBlock), 0, d.st, n, t.mark, flag);
    if (int rc = exclusive_sum(d, flag, cmap, (size_t)n + 1)) return rc;
    if (int rc = read_flags(d, t, what, h_ctr)) return rc;
    if (copy_sync(&nc, cmap + n, sizeof(int), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    if (nc < 0 || nc > n) return ERROR_MISC;
    int *crow = d.alloc<int>((size_t)nc), *cnt = d.alloc<int>((size_t)nc + 1), *s2rp = d.alloc<int>((size_t)nc + 1);
    long long *gcap = d.alloc<long long>((size_t)nc + 1);
    t.need = d.alloc<int>((size_t)nc);
    t.goff = d.alloc<long long>((size_t)nc + 1);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(aggressive S2)", __FILE__, __LINE__);
    // every k of a row is an intermediate point: about avg (1 + avg) candidates
    const double avg = (double)nnz / (double)n;
    t.G = lanes_for_candidates(avg * (1.0 + avg));
    t.slots = slots_for(t.G);
    int *s2ci = nullptr, s2nnz = 0;
    if (nc > 0) {
        hipLaunchKernelGGL(agg_crow, dim3(grid_for(n)), dim3(kBlock), 0, d.st, n, t.mark, cmap, nc, crow);
        SSS_HIP(hipMemsetAsync(gcap + nc, 0, sizeof(long long), d.st));
        hipLaunchKernelGGL(agg_bound, dim3(grid_for(nc)), dim3(kBlock), 0, d.st, t.S, crow, nc, t.slots, t.need, gcap, t.ctr);
        if (int rc = exclusive_sum(d, gcap, t.goff, (size_t)nc + 1)) return rc;
        if (int rc = read_flags(d, t, what, h_ctr)) return rc;
        if (copy_sync(&t.total, t.goff + nc, sizeof(long long), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
        t.global_rows = h_ctr[1];
        t.gkey = d.alloc<int>((size_t)t.total);
        int *gseq = d.alloc<int>((size_t)t.total);
        if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(global tables)", __FILE__, __LINE__);
        SSS_HIP(hipMemsetAsync(cnt + nc, 0, sizeof(int), d.st));
        launch_agg<false>(t.G, d.st, nc, t.S, t.mark, cmap, crow, nc, t.slots, t.need, t.goff, t.gkey, gseq, cnt, s2rp, s2nnz,
                          s2ci, t.ctr);
        if (int rc = exclusive_sum(d, cnt, s2rp, (size_t)nc + 1)) return rc;
        if (int rc = read_flags(d, t, what, h_ctr)) return rc;
        if (copy_sync(&s2nnz, s2rp + nc, sizeof(int), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
        if (s2nnz < 0) return ERROR_MAT_SIZE;
        s2ci = d.alloc<int>((size_t)s2nnz);
        if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(aggressive S2)", __FILE__, __LINE__);
        launch_agg<true>(t.G, d.st, nc, t.S, t.mark, cmap, crow, nc, t.slots, t.need, t.goff, t.gkey, gseq, cnt, s2rp, s2nnz,
                         s2ci, t.ctr);
        if (int rc = read_flags(d, t, what, h_ctr)) return rc;
    }
    d.lap(false);

    // into arrays of its own first: S2 stays untouched if a copy fails
    HostArr<int> rp((size_t)nc + 1), ci((size_t)s2nnz);
    if (nc > 0 && copy_sync(rp.p, s2rp, sizeof(int) * ((size_t)nc + 1), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    if (copy_sync(ci.p, s2ci, sizeof(int) * (size_t)s2nnz, hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    d.lap(true);
    memset(S2, 0, sizeof(*S2));
    S2->num_rows = S2->num_cols = nc;
    S2->num_nnzs = s2nnz;
    S2->row_ptr = rp.release();
    S2->col_idx = ci.release();
    if (getenv("SSS_SETUP_TIMING"))
        fprintf(stderr, "[setup]   aggressive S2: device, %d rows, %d entries, %d lanes per row, %d rows on global tables, "
                        "copies %.4f s, kernels %.4f s\n", nc, s2nnz, t.G, t.global_rows, d.t_copy, d.t_kern);
    return 0;
}

extern "C" int sss_hip_std_pattern(const SSS_IMAT *S, const int *mark, int ncoarse, SSS_MAT *P)
{
    if (!P) return ERROR_INPUT_PAR;
    if (int rc = check_s(S, mark)) return rc;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const int n = S->num_rows;
    Dev d;
    if (hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
    Tables t;
    if (int rc = make_tables(d, t, S, mark, nullptr, 0, "standard pattern")) return rc;
    int *gseq = d.alloc<int>((size_t)t.total);
    int *cnt = d.alloc<int>((size_t)n + 1), *prp = d.alloc<int>((size_t)n + 1);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(standard pattern)", __FILE__, __LINE__);
    SSS_HIP(hipMemsetAsync(cnt + n, 0, sizeof(int), d.st));
    int *pci = nullptr, pnnz = 0, h_ctr[2];
    launch_pattern<false>(t.G, d.st, n, t.S, t.mark, t.slots, t.need, t.goff, t.gkey, gseq, cnt, prp, pnnz, pci, t.ctr);
    if (int rc = exclusive_sum(d, cnt, prp, (size_t)n + 1)) return rc;
    if (int rc = read_flags(d, t, "standard pattern", h_ctr)) return rc;
    if (copy_sync(&pnnz, prp + n, sizeof(int), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    if (pnnz < 0) return ERROR_MAT_SIZE;
    pci = d.alloc<int>((size_t)pnnz);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(standard pattern)", __FILE__, __LINE__);
    launch_pattern<true>(t.G, d.st, n, t.S, t.mark, t.slots, t.need, t.goff, t.gkey, gseq, cnt, prp, pnnz, pci, t.ctr);
    if (int rc = read_flags(d, t, "standard pattern", h_ctr)) return rc;
    d.lap(false);

    // into arrays of its own first: P stays untouched if a copy fails
    HostArr<int> rp((size_t)n + 1), ci((size_t)pnnz);
    HostArr<double> val((size_t)pnnz);
    if (copy_sync(rp.p, prp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    if (copy_sync(ci.p, pci, sizeof(int) * (size_t)pnnz, hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    d.lap(true);
    P->num_rows = n;
    P->num_cols = ncoarse;
    P->num_nnzs = pnnz;
    P->row_ptr = rp.release();
    P->col_idx = ci.release();
    P->val = val.release();
    timing_line("pattern", d, t, n, pnnz);
    return 0;
}

template <bool FILL, class... Args>
static void launch_trunc_cap(int G, hipStream_t st, int n, Args... a)
{
    switch (G) {
    case 1: hipLaunchKernelGGL((trunc_rows_cap<1, FILL>), dim3(grid_for(n)), dim3(kBlock), 0, st, a...); break;
    case 4: hipLaunchKernelGGL((trunc_rows_cap<4, FILL>), dim3(grid_for(4LL * n)), dim3(kBlock), 0, st, a...); break;
    case 16: hipLaunchKernelGGL((trunc_rows_cap<16, FILL>), dim3(grid_for(16LL * n)), dim3(kBlock), 0, st, a...); break;
    default: hipLaunchKernelGGL((trunc_rows_cap<64, FILL>), dim3(grid_for(64LL * n)), dim3(kBlock), 0, st, a...); break;
    }
}

// The truncation of (prp, pci, pv) on the device at threshold eps with at most pmax entries per row
// (0: no cap, one lane per row): count, prefix, fill.  *nrp, *nci, *nv are the new arrays, *kept their entries;
// `timing` measures it on its own (a stream synchronisation before and after).
static int truncate_rows(Dev &d, int n, const int *prp, const int *pci, const double *pv, int pnnz, double eps, int pmax,
                         bool timing, int **nrp_out, int **nci_out, double **nv_out, int *kept_out)
{
    int *cnt = d.alloc<int>((size_t)n + 1), *nrp = d.alloc<int>((size_t)n + 1);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(truncation)", __FILE__, __LINE__);
    double t0 = 0.0;
    d.trunc_timed = timing;
    if (timing) {
        SSS_HIP(hipStreamSynchronize(d.st));
        t0 = PhaseTimer::now();
    }
    // lanes per row of the capped kernels from the mean row of the untruncated P
    const int G = pmax > 0 ? lanes_for_candidates((double)pnnz / (double)std::max(n, 1)) : 1;
    d.cap = pmax, d.cap_lanes = G;
    SSS_HIP(hipMemsetAsync(cnt + n, 0, sizeof(int), d.st));
    if (pmax > 0)
        launch_trunc_cap<false>(G, d.st, n, n, pnnz, prp, pci, pv, eps, pmax, cnt, (const int *)nrp, 0, (int *)nullptr,
                                (double *)nullptr);
    else
        hipLaunchKernelGGL((trunc_rows<false>), dim3(grid_for(n)), dim3(kBlock), 0, d.st, n, pnnz, prp, pci, pv, eps, cnt, nrp, 0,
                           nullptr, nullptr);
    if (int rc = exclusive_sum(d, cnt, nrp, (size_t)n + 1)) return rc;
    int kept = 0;
    SSS_HIP(hipGetLastError());
    if (copy_sync(&kept, nrp + n, sizeof(int), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    if (kept < 0 || kept > pnnz) return ERROR_MAT_SIZE;
    int *nci = d.alloc<int>((size_t)kept);
    double *nv = d.alloc<double>((size_t)kept);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(truncation)", __FILE__, __LINE__);
    if (pmax > 0)
        launch_trunc_cap<true>(G, d.st, n, n, pnnz, prp, pci, pv, eps, pmax, cnt, (const int *)nrp, kept, nci, nv);
    else
        hipLaunchKernelGGL((trunc_rows<true>), dim3(grid_for(n)), dim3(kBlock), 0, d.st, n, pnnz, prp, pci, pv, eps, cnt, nrp, kept,
                           nci, nv);
    SSS_HIP(hipGetLastError());
    if (timing) {
        SSS_HIP(hipStreamSynchronize(d.st));
        d.t_trunc = PhaseTimer::now() - t0;
    }
    *nrp_out = nrp, *nci_out = nci, *nv_out = nv, *kept_out = kept;
    return 0;
}

// (nrp, nci, nv) into P: into arrays of its own first, so that P stays untouched if a copy fails
static int download_p(Dev &d, int n, const int *nrp, const int *nci, const double *nv, int kept, SSS_MAT *P, bool replace)
{
    HostArr<int> rp((size_t)n + 1), ci((size_t)kept);
    HostArr<double> val((size_t)kept);
    if (copy_sync(rp.p, nrp, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    if (copy_sync(ci.p, nci, sizeof(int) * (size_t)kept, hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    if (copy_sync(val.p, nv, sizeof(double) * (size_t)kept, hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    d.lap(true);
    if (replace) {
        free(P->row_ptr);
        free(P->col_idx);
        free(P->val);
    } else {
        memset(P, 0, sizeof(*P));
        P->num_rows = n;
    }
    P->num_nnzs = kept;
    P->row_ptr = rp.release();
    P->col_idx = ci.release();
    P->val = val.release();
    return 0;
}

// The tail of every interpolation: the coarse numbers of the columns of (prp, pci, pv), the truncation
// (with the cap of SSS_SETUP_PMAX), the download.  P is written after the last copy only; `replace` frees
// the arrays it held.
static int renumber_truncate(Dev &d, const Tables &t, const char *what, int n, const int *prp, int *pci, const double *pv,
                             int pnnz, double trunc_threshold, SSS_MAT *P, bool replace)
{
    int *cmap = d.alloc<int>((size_t)n + 1), *flag = d.alloc<int>((size_t)n + 1);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(truncation)", __FILE__, __LINE__);
    hipLaunchKernelGGL(flag_coarse, dim3(grid_for((long long)n + 1)), dim3(kBlock), 0, d.st, n, t.mark, flag);
    if (int rc = exclusive_sum(d, flag, cmap, (size_t)n + 1)) return rc;
    if (pnnz > 0) hipLaunchKernelGGL(renumber, dim3(grid_for(pnnz)), dim3(kBlock), 0, d.st, pnnz, n, cmap, pci, t.ctr);
    int *nrp = nullptr, *nci = nullptr, h_ctr[2], kept = 0, ncoarse = 0;
    double *nv = nullptr;
    if (int rc = truncate_rows(d, n, prp, pci, pv, pnnz, trunc_threshold, sss_setup_pmax(),
                               getenv("SSS_SETUP_TIMING") && getenv("SSS_SETUP_PMAX"), &nrp, &nci, &nv, &kept))
        return rc;
    if (int rc = read_flags(d, t, what, h_ctr)) return rc;
    if (copy_sync(&ncoarse, cmap + n, sizeof(int), hipMemcpyDeviceToHost, d.st)) return ERROR_MISC;
    d.lap(false);
    if (int rc = download_p(d, n, nrp, nci, nv, kept, P, replace)) return rc;
    P->num_cols = ncoarse;
    return 0;
}

extern "C" int sss_hip_interp_trunc(SSS_MAT *P, double eps, int pmax)
{
    if (pmax < 0 || !P || P->num_rows <= 0 || !P->row_ptr || P->row_ptr[0] != 0) return ERROR_INPUT_PAR;
    const int n = P->num_rows, pnnz = P->row_ptr[n];
    for (int i = 0; i < n; ++i)
        if (P->row_ptr[i + 1] < P->row_ptr[i]) return ERROR_INPUT_PAR;
    if (pnnz != P->num_nnzs || (pnnz > 0 && (!P->col_idx || !P->val))) return ERROR_INPUT_PAR;
    // n * 64 lanes must fit the grid (2^31 - 1 blocks)
    if ((long long)n * 64 / kBlock >= 0x7fffffffLL) return ERROR_MAT_SIZE;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    Dev d;
    if (hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
    const int *prp = d.upload(P->row_ptr, (size_t)n + 1), *pci = d.upload(P->col_idx, (size_t)pnnz);
    const double *pv = d.upload(P->val, (size_t)pnnz);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(truncation)", __FILE__, __LINE__);
    d.lap(true);
    int *nrp = nullptr, *nci = nullptr, kept = 0;
    double *nv = nullptr;
    if (int rc = truncate_rows(d, n, prp, pci, pv, pnnz, eps, pmax, getenv("SSS_SETUP_TIMING") != nullptr, &nrp, &nci, &nv, &kept))
        return rc;
    SSS_HIP(hipStreamSynchronize(d.st));
    d.lap(false);
    const int ncols = P->num_cols;
    if (int rc = download_p(d, n, nrp, nci, nv, kept, P, true)) return rc;
    P->num_cols = ncols;
    if (getenv("SSS_SETUP_TIMING"))
        fprintf(stderr, "[setup]   truncation: device, %d rows, %d of %d entries kept, copies %.4f s, kernels %.4f s%s\n", n, kept,
                pnnz, d.t_copy, d.t_kern, cap_note(d).c_str());
    return 0;
}

template <bool FILL, class... Args>
static void launch_mpass(int G, hipStream_t st, int n, Args... a)
{
    switch (G) {
    case 1: hipLaunchKernelGGL((mpass_rows<1, FILL>), dim3(grid_for(n)), dim3(kBlock), 0, st, a...); break;
    case 4: hipLaunchKernelGGL((mpass_rows<4, FILL>), dim3(grid_for(4LL * n)), dim3(kBlock), 0, st, a...); break;
    case 16: hipLaunchKernelGGL((mpass_rows<16, FILL>), dim3(grid_for(16LL * n)), dim3(kBlock), 0, st, a...); break;
    default: hipLaunchKernelGGL((mpass_rows<64, FILL>), dim3(grid_for(64LL * n)), dim3(kBlock), 0, st, a...); break;
    }
}

extern "C" int sss_hip_interp_mpass(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold,
                                    int *passes)
{
    const char *what = "multipass interpolation";
    if (!A || !P || !A->row_ptr) return ERROR_INPUT_PAR;
    if (int rc = check_s(S, mark)) return rc;
    const int n = S->num_rows, snnz = S->row_ptr[n];
    if (A->num_rows != n || A->row_ptr[0] != 0) return ERROR_INPUT_PAR;
    const int annz = A->row_ptr[n];
    if (annz <= 0 || !A->col_idx || !A->val) return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    Dev d;
    if (hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
    hipStream_t st = d.st;
    Tables t;
    t.S.n = n, t.S.nnz = snnz, t.S.v = nullptr;
    t.S.rp = d.upload(S->row_ptr, (size_t)n + 1);
    t.S.ci = d.upload(S->col_idx, (size_t)snnz);
    t.mark = d.upload(mark, (size_t)n);
    Csr Ad{n, annz, nullptr, nullptr, nullptr};
    Ad.rp = d.upload(A->row_ptr, (size_t)n + 1);
    Ad.ci = d.upload(A->col_idx, (size_t)annz);
    Ad.v = d.upload(A->val, (size_t)annz);
    t.ctr = d.alloc<int>(2);
    unsigned long long *stat = d.alloc<unsigned long long>(2), h_stat[2] = {0, 0};
    int *flag = d.alloc<int>((size_t)n + 1), *pos = d.alloc<int>((size_t)n + 1);
    int *pass = d.alloc<int>((size_t)n), *len = d.alloc<int>((size_t)n), *off = d.alloc<int>((size_t)n);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(multipass interpolation)", __FILE__, __LINE__);
    d.lap(true);

    // consistency, the coarse numbers, pass 0 (block 0: the C rows)
    int h_ctr[2], nc = 0;
    SSS_HIP(hipMemsetAsync(t.ctr, 0, sizeof(int) * 2, st));
    hipLaunchKernelGGL(mpass_check_rows, dim3(grid_for(n)), dim3(kBlock), 0, st, Ad, t.S, t.ctr);
    hipLaunchKernelGGL(flag_coarse, dim3(grid_for((long long)n + 1)), dim3(kBlock), 0, st, n, t.mark, flag);
    if (int rc = exclusive_sum(d, flag, pos, (size_t)n + 1)) return rc;
    if (int rc = read_flags(d, t, what, h_ctr)) return rc;
    if (copy_sync(&nc, pos + n, sizeof(int), hipMemcpyDeviceToHost, st)) return ERROR_MISC;
    if (nc < 0 || nc > n) return ERROR_MISC;
    std::vector<int *> bcol{d.alloc<int>((size_t)nc)};
    std::vector<double *> bval{d.alloc<double>((size_t)nc)};
    std::vector<int> bnnz{nc};
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(multipass interpolation)", __FILE__, __LINE__);
    hipLaunchKernelGGL(mpass_init, dim3(grid_for(n)), dim3(kBlock), 0, st, n, t.mark, pos, nc, pass, len, off, bcol[0], bval[0]);

    // pass numbers: sweeps until one numbers nobody (at most n of them number somebody)
    std::vector<int> rows_of{nc};
    long long numbered = nc;
    for (int p = 1; p <= n; ++p) {
        SSS_HIP(hipMemsetAsync(stat, 0, sizeof(unsigned long long) * 2, st));
        hipLaunchKernelGGL(mpass_relax, dim3(grid_for(n)), dim3(kBlock), 0, st, t.S, t.mark, pass, p, stat);
        SSS_HIP(hipGetLastError());
        if (copy_sync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, st)) return ERROR_MISC;
        if (h_stat[0] == 0) break;
        if (h_stat[0] > (unsigned long long)n) return ERROR_MISC;
        rows_of.push_back((int)h_stat[0]);
        numbered += (long long)h_stat[0];
    }
    const int npass = (int)rows_of.size() - 1;

    // one round of launches per pass, over that pass's rows
    long long total_nnz = nc;
    int max_lanes = 1;
    for (int p = 1; p <= npass; ++p) {
        const size_t scope = d.mem.size();
        const int cnt = rows_of[p];
        int *rows = d.alloc<int>((size_t)cnt), *rcnt = d.alloc<int>((size_t)cnt + 1), *boff = d.alloc<int>((size_t)cnt + 1);
        long long *gcap = d.alloc<long long>((size_t)cnt + 1);
        t.need = d.alloc<int>((size_t)cnt);
        t.goff = d.alloc<long long>((size_t)cnt + 1);
        if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(multipass interpolation)", __FILE__, __LINE__);
        hipLaunchKernelGGL(mpass_select, dim3(grid_for((long long)n + 1)), dim3(kBlock), 0, st, n, pass, p, flag);
        if (int rc = exclusive_sum(d, flag, pos, (size_t)n + 1)) return rc;
        hipLaunchKernelGGL(mpass_scatter, dim3(grid_for(n)), dim3(kBlock), 0, st, n, pass, p, pos, cnt, rows);
        const PrevBlock B{len, off, bcol[p - 1], bval[p - 1], bnnz[p - 1]};
        SSS_HIP(hipMemsetAsync(stat, 0, sizeof(unsigned long long) * 2, st));
        hipLaunchKernelGGL(mpass_bound, dim3(grid_for(cnt)), dim3(kBlock), 0, st, Ad, t.S, pass, B, rows, cnt, p, t.need, stat,
                           t.ctr);
        if (int rc = read_flags(d, t, what, h_ctr)) return rc;
        if (copy_sync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, st)) return ERROR_MISC;
        // the bound is at least the pass's entries: the device gives up where they might not fit an int
        if (total_nnz + (long long)h_stat[1] > INT_MAX) return ERROR_MAT_SIZE;
        // G from the pass's average candidate bound
        t.G = lanes_for_candidates((double)h_stat[1] / (double)cnt);
        t.slots = slots_for(t.G);
        max_lanes = std::max(max_lanes, t.G);
        hipLaunchKernelGGL(mpass_gcap, dim3(grid_for((long long)cnt + 1)), dim3(kBlock), 0, st, cnt, t.slots, t.need, gcap, t.ctr);
        if (int rc = exclusive_sum(d, gcap, t.goff, (size_t)cnt + 1)) return rc;
        if (int rc = read_flags(d, t, what, h_ctr)) return rc;
        if (copy_sync(&t.total, t.goff + cnt, sizeof(long long), hipMemcpyDeviceToHost, st)) return ERROR_MISC;
        t.global_rows = h_ctr[1];
        t.gkey = d.alloc<int>((size_t)t.total);
        int *gseq = d.alloc<int>((size_t)t.total);
        double *gacc = d.alloc<double>((size_t)t.total);
        if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(global tables)", __FILE__, __LINE__);
        SSS_HIP(hipMemsetAsync(rcnt + cnt, 0, sizeof(int), st));
        launch_mpass<false>(t.G, st, cnt, Ad, t.S, (const int *)pass, B, (const int *)rows, cnt, p, t.slots, (const int *)t.need,
                            (const long long *)t.goff, t.gkey, gseq, gacc, rcnt, (const int *)boff, 0, (int *)nullptr,
                            (double *)nullptr, len, off, t.ctr);
        if (int rc = exclusive_sum(d, rcnt, boff, (size_t)cnt + 1)) return rc;
        if (int rc = read_flags(d, t, what, h_ctr)) return rc;
        int nnz_p = 0;
        if (copy_sync(&nnz_p, boff + cnt, sizeof(int), hipMemcpyDeviceToHost, st)) return ERROR_MISC;
        if (nnz_p < 0 || (unsigned long long)nnz_p > h_stat[1]) return ERROR_MISC;
        bcol.push_back(d.alloc<int>((size_t)nnz_p));
        bval.push_back(d.alloc<double>((size_t)nnz_p));
        bnnz.push_back(nnz_p);
        if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(multipass interpolation)", __FILE__, __LINE__);
        launch_mpass<true>(t.G, st, cnt, Ad, t.S, (const int *)pass, B, (const int *)rows, cnt, p, t.slots, (const int *)t.need,
                           (const long long *)t.goff, t.gkey, gseq, gacc, rcnt, (const int *)boff, nnz_p, bcol[p], bval[p], len, off,
                           t.ctr);
        if (int rc = read_flags(d, t, what, h_ctr)) return rc;
        total_nnz += nnz_p;
        // the pass's scratch goes, its block stays
        d.free_from(scope, {bcol[p], bval[p]});
        t.need = nullptr, t.goff = nullptr, t.gkey = nullptr;
    }
    const int global_rows_all = h_ctr[1];   // ctr[1] is never reset: the rows on global tables of all passes

    // P in row order, fine columns
    const int pnnz = (int)total_nnz;
    int *prp = d.alloc<int>((size_t)n + 1), *pci = d.alloc<int>((size_t)pnnz), *d_bnnz = d.upload(bnnz.data(), bnnz.size());
    double *pv = d.alloc<double>((size_t)pnnz);
    int **d_bcol = d.upload(bcol.data(), bcol.size());
    double **d_bval = d.upload(bval.data(), bval.size());
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(multipass interpolation)", __FILE__, __LINE__);
    SSS_HIP(hipMemcpyAsync(flag, len, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, st));
    SSS_HIP(hipMemsetAsync(flag + n, 0, sizeof(int), st));
    if (int rc = exclusive_sum(d, flag, prp, (size_t)n + 1)) return rc;
    hipLaunchKernelGGL(mpass_assemble, dim3(grid_for(n)), dim3(kBlock), 0, st, n, pass, len, off, (int)bcol.size(), d_bcol, d_bval,
                       d_bnnz, prp, pnnz, pci, pv, t.ctr);
    if (int rc = read_flags(d, t, what, h_ctr)) return rc;
    t.G = max_lanes;
    t.global_rows = global_rows_all;
    if (int rc = renumber_truncate(d, t, what, n, prp, pci, pv, pnnz, trunc_threshold, P, false)) return rc;
    if (passes) *passes = npass;
    if (getenv("SSS_SETUP_TIMING"))
        fprintf(stderr, "[setup]   multipass P: device, %d passes, %lld rows unreached, %d rows, %d entries, up to %d lanes per row, "
                        "%d rows on global tables, copies %.4f s, kernels %.4f s%s\n", npass, (long long)n - numbered, n, P->num_nnzs,
                max_lanes, global_rows_all, d.t_copy, d.t_kern, cap_note(d).c_str());
    return 0;
}

// the weights of interp_STD or (exti) interp_EXTI on a pattern, the coarse renumbering, the truncation
static int interp_weights(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold, bool exti)
{
    const char *what = exti ? "extended+i weights" : "standard weights";
    if (!A || !P || !A->row_ptr || !P->row_ptr) return ERROR_INPUT_PAR;
    if (int rc = check_s(S, mark)) return rc;
    const int n = S->num_rows, annz = A->row_ptr[A->num_rows > 0 ? A->num_rows : 0];
    if (A->num_rows != n || P->num_rows != n || A->row_ptr[0] != 0 || P->row_ptr[0] != 0) return ERROR_INPUT_PAR;
    const int pnnz = P->row_ptr[n];
    if (annz <= 0 || !A->col_idx || !A->val || pnnz < 0 || (pnnz > 0 && (!P->col_idx || !P->val))) return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    Dev d;
    if (hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
    const int *prp = d.upload(P->row_ptr, (size_t)n + 1);
    int *pci = d.upload(P->col_idx, (size_t)pnnz);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(standard weights)", __FILE__, __LINE__);
    Tables t;
    if (int rc = make_tables(d, t, S, mark, prp, pnnz, what)) return rc;
    Csr Ad{n, annz, nullptr, nullptr, nullptr};
    Ad.rp = d.upload(A->row_ptr, (size_t)n + 1);
    Ad.ci = d.upload(A->col_idx, (size_t)annz);
    Ad.v = d.upload(A->val, (size_t)annz);
    d.lap(true);
    double *gacc = d.alloc<double>((size_t)t.total), *pv = d.alloc<double>((size_t)pnnz);
    double *diag = d.alloc<double>((size_t)n), *csum = nullptr, *nsum = nullptr, *psum = nullptr;
    if (!exti) csum = d.alloc<double>((size_t)n), nsum = d.alloc<double>((size_t)n), psum = d.alloc<double>((size_t)n);
    if (d.oom) return hip_fail(hipErrorOutOfMemory, "hipMalloc(standard weights)", __FILE__, __LINE__);
    SSS_HIP(hipMemsetAsync(pv, 0, sizeof(double) * (size_t)std::max(pnnz, 1), d.st));
    if (exti) {
        hipLaunchKernelGGL(exti_diag, dim3(grid_for(n)), dim3(kBlock), 0, d.st, Ad, diag);
        launch_exti(t.G, d.st, n, Ad, t.S, t.mark, t.slots, t.need, t.goff, t.gkey, gacc, prp, pnnz, (const int *)pci, pv,
                    (const double *)diag, t.ctr);
    } else {
        hipLaunchKernelGGL(weights_sums, dim3(grid_for(n)), dim3(kBlock), 0, d.st, Ad, t.S, t.mark, diag, csum, nsum, psum, t.ctr);
        launch_weights(t.G, d.st, n, Ad, t.S, t.mark, t.slots, t.need, t.goff, t.gkey, gacc, prp, pnnz, (const int *)pci, pv,
                       (const double *)diag, (const double *)csum, (const double *)nsum, (const double *)psum, t.ctr);
    }
    if (int rc = renumber_truncate(d, t, what, n, prp, pci, pv, pnnz, trunc_threshold, P, true)) return rc;
    timing_line("weights", d, t, n, P->num_nnzs, exti ? "extended+i" : "standard");
    return 0;
}

extern "C" int sss_hip_interp_std(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold)
{
    return interp_weights(A, S, mark, P, trunc_threshold, false);
}

extern "C" int sss_hip_interp_exti(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold)
{
    return interp_weights(A, S, mark, P, trunc_threshold, true);
}
