/*
 * sss_setup.c — AMG setup phase (host C).  Out of the GPU hot-path scope (SURVEY.md §2 rows
 * 10-12), but it builds the hierarchy the hot path consumes, so it reproduces the reference's
 * setup semantics exactly ("uncapped" reference):
 *
 *   strong couplings ............ Setup/SSS_coarsen.c:106-181
 *   weak-coupling compression ... Setup/SSS_coarsen.c:185-212
 *   classical RS C/F split ...... Setup/SSS_coarsen.c:294-498 (bucketed measure lists)
 *   F-F cleanup ................. Setup/SSS_coarsen.c:501-574
 *   direct P pattern ............ Setup/SSS_coarsen.c:577-630
 *   direct interpolation ........ Setup/SSS_inter.cu:400-547 (the host twin interp_DIR)
 *   standard P pattern .......... Setup/SSS_coarsen.c:633-725 (interp_type 2)
 *   standard interpolation ...... Setup/SSS_inter.cu:550-715 (interp_STD)
 *   truncation .................. Setup/SSS_inter.cu:16-102
 *   Galerkin RAP ................ SSS_matvec.c:398-534
 *   level loop .................. Setup/SSS_SETUP.cu:36-178
 *
 * One engine extension, off unless asked for: cs_type SSS_COARSE_PMIS (3) replaces the serial RS
 * first pass by the parallel PMIS split (pmis_split below; on the device sss_hip_pmis,
 * amg_amd/csrc/sss_pmis.hip).  No F-F cleanup runs after it; interp_type 2 is its partner.  With
 * cs_type 1 nothing here differs from the reference.  On large levels the standard pattern and
 * interpolation run on the device (sss_hip_std_pattern, sss_hip_interp_std, amg_amd/csrc/sss_interp.hip):
 * the same P bit for bit, with the code below as the fallback.  A second extension, interp_type
 * intERP_EXTI (3): the extended+i weights on the standard pattern (interp_EXTI below; on the device
 * sss_hip_interp_exti, the same file).
 *
 * The measure lists are kept as an array of FIFO buckets indexed by measure instead of the
 * reference's heap-allocated sorted list of list nodes with element-level linked lists
 * (lists/where); every insert/remove happens in the same order, so the head of the maximal
 * bucket — the next C point — is the same.  RAP runs the reference's row-by-row
 * marker algorithm independently per coarse row (OpenMP), which yields identical rows
 * (diagonal first, then discovery order; identical summation order).
 */
#include "sss_internal.h"

#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <unistd.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ======================================================================================
 * Strength of connection
 * ====================================================================================== */
static void strong_couplings(const SSS_MAT *A, SSS_IMAT *S, const SSS_AMG_PARS *pars)
{
    const int n = A->num_rows;
    const double theta = pars->strong_threshold;
    const double row_sum_bound = 2.0 - pars->max_row_sum;
    const int *ia = A->row_ptr, *ja = A->col_idx;
    const double *a = A->val;

    S->num_rows = n;
    S->num_cols = A->num_cols;
    S->num_nnzs = A->num_nnzs;
    S->val = NULL;
    S->row_ptr = (int *)SSS_calloc((size_t)n + 1, sizeof(int));
    S->col_idx = (int *)SSS_calloc((size_t)A->num_nnzs, sizeof(int));
    memcpy(S->row_ptr, ia, ((size_t)n + 1) * sizeof(int));
    memcpy(S->col_idx, ja, (size_t)A->num_nnzs * sizeof(int));

#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) {
        double abs_sum = 0.0, max_off = 0.0, dii = 0.0;
        int have_diag = 0;
        for (int k = ia[i]; k < ia[i + 1]; ++k) {
            double m = SSS_ABS(a[k]);
            abs_sum += m;
            if (ja[k] != i) max_off = SSS_max(max_off, m);
            else if (!have_diag) { dii = a[k]; have_diag = 1; }
        }
        max_off *= theta;
        for (int k = ia[i]; k < ia[i + 1]; ++k)     /* first diagonal entry is never strong */
            if (ja[k] == i) { S->col_idx[k] = -1; break; }
        if (abs_sum < row_sum_bound * SSS_ABS(dii)) {
            for (int k = ia[i]; k < ia[i + 1]; ++k) S->col_idx[k] = -1;
        } else {
            for (int k = ia[i]; k < ia[i + 1]; ++k)
                if (-a[k] <= max_off) S->col_idx[k] = -1;
        }
    }
}

/* Drops entries marked -1; returns -99 when nothing strong is left (reference's ERROR_UNKNOWN). */
static int drop_weak(SSS_IMAT *S)
{
    const int n = S->num_rows;
    if (S->num_nnzs < (1 << 20)) {
        int out = 0;
        for (int i = 0; i < n; ++i) {
            int lo = S->row_ptr[i], hi = S->row_ptr[i + 1];
            S->row_ptr[i] = out;
            for (int k = lo; k < hi; ++k)
                if (S->col_idx[k] > -1) S->col_idx[out++] = S->col_idx[k];
        }
        S->row_ptr[n] = out;
        S->num_nnzs = out;
        return out > 0 ? 0 : -99;
    }
    /* same compaction in parallel: kept counts per row, prefix sum, copy into a new array */
    int *cnt = (int *)SSS_calloc((size_t)n + 1, sizeof(int));
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) {
        int c = 0;
        for (int k = S->row_ptr[i]; k < S->row_ptr[i + 1]; ++k) c += S->col_idx[k] > -1;
        cnt[i + 1] = c;
    }
    for (int i = 0; i < n; ++i) cnt[i + 1] += cnt[i];
    const int out = cnt[n];
    int *ci = (int *)SSS_calloc((size_t)(out > 0 ? out : 1), sizeof(int));
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) {
        int o = cnt[i];
        for (int k = S->row_ptr[i]; k < S->row_ptr[i + 1]; ++k)
            if (S->col_idx[k] > -1) ci[o++] = S->col_idx[k];
    }
    free(S->col_idx);
    free(S->row_ptr);
    S->col_idx = ci;
    S->row_ptr = cnt;
    S->num_nnzs = out;
    return out > 0 ? 0 : -99;
}

/* ======================================================================================
 * Measure buckets.  The reference keeps one doubly linked list per measure (SSS_coarsen.c
 * lists/where + list nodes): inserts append at the tail, the next C point is the head of the
 * largest non-empty list -- i.e. among the points of maximal measure, the one inserted
 * earliest.  Here each bucket is an append-only FIFO array of (point, version) entries and a
 * removal only bumps the point's version (its entry goes stale and is skipped when it reaches
 * the head).  Same head, same order of picks, but a move is two sequential writes instead of
 * four dependent pointer updates scattered over the grid (the serial first pass is
 * memory-latency bound).  Buckets are compacted in place (order kept) when most of their
 * entries are stale.
 * ====================================================================================== */
typedef struct {
    int pt;
    unsigned ver;
} bucket_entry;

typedef struct {
    bucket_entry *e;
    size_t head, tail, cap;
    int live;                /* live entries = points in this bucket */
} bucket_fifo;

/* Per-point state of the first pass in one 8-byte record (one cache line holds eight points; the
 * pass touches measure, mark and version of the same neighbours).  A point's version moves once
 * per bucket move -- a few dozen times at most -- so 29 bits never wrap. */
typedef struct {
    int lambda;              /* measure */
    int mark : 3;            /* UNPT / CGPT / FGPT / ISPT */
    unsigned ver : 29;       /* current version: a bucket entry is live iff it matches */
} rs_point;

typedef struct {
    bucket_fifo *b;          /* per measure */
    int cap;                 /* allocated measures */
    int top;                 /* upper bound on the largest non-empty measure */
    rs_point *pts;
} measure_buckets;

static void buckets_grow(measure_buckets *B, int m)
{
    int old = B->cap, cap = B->cap;
    while (cap <= m) cap = cap * 2 + 16;
    B->b = (bucket_fifo *)realloc(B->b, sizeof(bucket_fifo) * (size_t)cap);
    memset(B->b + old, 0, sizeof(bucket_fifo) * (size_t)(cap - old));
    B->cap = cap;
}

static void bucket_compact(bucket_fifo *q, const rs_point *pts)
{
    size_t o = 0;
    for (size_t k = q->head; k < q->tail; ++k)
        if (q->e[k].ver == pts[q->e[k].pt].ver) q->e[o++] = q->e[k];
    q->head = 0;
    q->tail = o;
}

static inline void bucket_insert(measure_buckets *B, int m, int pt)
{
    if (m >= B->cap) buckets_grow(B, m);
    bucket_fifo *q = &B->b[m];
    if (q->tail == q->cap) {
        if (q->tail - q->head > 2 * (size_t)q->live + 64 || q->head > q->cap / 2) bucket_compact(q, B->pts);
        if (q->tail == q->cap) {
            q->cap = q->cap * 2 + 256;
            q->e = (bucket_entry *)realloc(q->e, sizeof(bucket_entry) * q->cap);
        }
    }
    q->e[q->tail].pt = pt;
    q->e[q->tail].ver = ++B->pts[pt].ver;
    q->tail++;
    q->live++;
    if (m > B->top) B->top = m;
}

static inline void bucket_remove(measure_buckets *B, int m, int pt)
{
    if (m < 0 || m >= B->cap || B->b[m].live == 0) {
        printf("### ERROR: This list is empty! %s : %d\n", __FILE__, __LINE__);
        return;
    }
    B->pts[pt].ver++;
    if (--B->b[m].live == 0) B->b[m].head = B->b[m].tail = 0;
}

/* bucket_remove(from) + bucket_insert(to) with one version step: the insert's new version already
 * makes the old entry stale (same buckets, same order as the two calls). */
static inline void bucket_move(measure_buckets *B, int from, int to, int pt)
{
    if (from < 0 || from >= B->cap || B->b[from].live == 0) {
        printf("### ERROR: This list is empty! %s : %d\n", __FILE__, __LINE__);
        return;
    }
    if (--B->b[from].live == 0) B->b[from].head = B->b[from].tail = 0;
    bucket_insert(B, to, pt);
}

/* Head point of the largest non-empty bucket, or -1 if every bucket is empty. */
static int bucket_max_head(measure_buckets *B)
{
    while (B->top > 0 && B->b[B->top].live == 0) B->top--;
    if (B->top <= 0) return -1;
    bucket_fifo *q = &B->b[B->top];
    while (q->e[q->head].ver != B->pts[q->e[q->head].pt].ver) q->head++;
    for (size_t t = q->head + 1; t < q->tail && t < q->head + 4; ++t) __builtin_prefetch(&B->pts[q->e[t].pt]);
    return q->e[q->head].pt;
}

/* Rows that can change in the C1 and F-F passes below.  Both passes visit the F rows in order and
 * act only on a row with a strongly coupled F neighbour j that shares no strong C point with it
 * (an "unshared pair").  Between rows, marks only ever move F -> C (a tentative C point that is
 * reverted was F before), so the C set only grows: a row with no unshared pair under the marks
 * before the pass never gets one, and the pass does nothing there but per-row bookkeeping.  This
 * flags the rows that have an unshared pair under the starting marks, row-parallel; the serial
 * passes run their exact logic on the flagged rows only.  owner (n ints) is a scratch marker
 * shared by the threads: a concurrent overwrite can only hide a shared C point, so it can add
 * rows (checked serially anyway), never drop one.  Returns owner reset to -1. */
static char *flag_unshared_rows(const SSS_IMAT *S, const int *mark, int *owner)
{
    const int n = S->num_rows;
    char *flag = (char *)SSS_calloc((size_t)(n > 0 ? n : 1), 1);
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) __atomic_store_n(&owner[i], -1, __ATOMIC_RELAXED);
#pragma omp parallel for schedule(dynamic, 4096)
    for (int i = 0; i < n; ++i) {
        if (mark[i] != FGPT) continue;
        for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q)
            if (mark[S->col_idx[q]] == CGPT) __atomic_store_n(&owner[S->col_idx[q]], i, __ATOMIC_RELAXED);
        for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1] && !flag[i]; ++q) {
            const int j = S->col_idx[q];
            int shares = 0;
            if (mark[j] != FGPT) continue;
            for (int r = S->row_ptr[j]; r < S->row_ptr[j + 1]; ++r)
                if (__atomic_load_n(&owner[S->col_idx[r]], __ATOMIC_RELAXED) == i) { shares = 1; break; }
            if (!shares) flag[i] = 1;
        }
    }
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) owner[i] = -1;
    return flag;
}

#ifndef PF_DEPTH
#define PF_DEPTH 5
#endif

/* Classical Ruge-Stueben first pass + C1 fix-up.  Returns the C-point count (or <0). */
static int rs_split(const SSS_MAT *A, SSS_IMAT *S, SSS_IVEC *vertices)
{
    const int n = A->num_rows;
    int *mark = vertices->d;
    int ncoarse, undecided = 0;
    int *lambda, *owner;
    SSS_IMAT ST;
    measure_buckets B;

    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const double t0 = SSS_get_time();
    ncoarse = drop_weak(S);
    if (ncoarse < 0) return ncoarse;
    const double tdrop = SSS_get_time();
    ST = SSS_imat_trans(S);
    const double t1 = SSS_get_time();

    memset(&B, 0, sizeof(B));
    B.pts = (rs_point *)SSS_calloc((size_t)n, sizeof(rs_point));
    rs_point *P = B.pts;
    buckets_grow(&B, 64);

#pragma omp parallel for schedule(static) reduction(+ : undecided) if (n > 65536)
    for (int i = 0; i < n; ++i) {
        if (S->row_ptr[i + 1] == S->row_ptr[i]) {
            P[i].mark = ISPT;
            P[i].lambda = 0;
        } else {
            P[i].mark = UNPT;
            P[i].lambda = ST.row_ptr[i + 1] - ST.row_ptr[i];
            undecided++;
        }
    }

    /* Initial lists; points with no influence become F immediately. */
    for (int i = 0; i < n; ++i) {
        if (P[i].mark == ISPT) continue;
        if (P[i].lambda > 0) {
            bucket_insert(&B, P[i].lambda, i);
            continue;
        }
        if (P[i].lambda < 0) printf("### WARNING: Negative lambda[%d]!\n", i);
        P[i].mark = FGPT;
        undecided--;
        for (int k = S->row_ptr[i]; k < S->row_ptr[i + 1]; ++k) {
            int j = S->col_idx[k];
            if (P[j].mark == ISPT) continue;
            if (j < i) {
                if (P[j].lambda > 0) bucket_remove(&B, P[j].lambda, j);
                P[j].lambda++;
                bucket_insert(&B, P[j].lambda, j);
            } else {
                P[j].lambda++;
            }
        }
    }

    const double t2 = SSS_get_time();
    while (undecided > 0) {
        int c = bucket_max_head(&B);
        int mc;
        if (c < 0) {
            printf("### ERROR: RS coarsening ran out of candidates (%d undecided)\n", undecided);
            break;
        }
        /* The pass is bound by cache misses on the neighbourhood of each pick (≈35 dependent
         * record / row accesses per pick, spread over three grid planes): request them all up
         * front -- the records of c's neighbours, their S rows, and the records of the S rows of
         * the neighbours that are about to become F. */
        {   /* and, pipelined, the neighbourhoods of the next candidates in the top bucket (the
             * likely next picks): row pointers PF_DEPTH picks ahead, their rows two ahead, the
             * records of their neighbours one ahead -- each stage reads only what an earlier pick
             * has already requested */
            const bucket_fifo *tq = &B.b[B.top];
            const size_t end = tq->tail < tq->head + 1 + PF_DEPTH ? tq->tail : tq->head + 1 + PF_DEPTH;
            for (size_t t = tq->head + 1; t < end; ++t) {
                const int nx = tq->e[t].pt;
                const size_t d = t - tq->head;
                if (d >= 3) {
                    __builtin_prefetch(&ST.row_ptr[nx]);
                    __builtin_prefetch(&S->row_ptr[nx]);
                } else if (d == 2) {
                    __builtin_prefetch(ST.col_idx + ST.row_ptr[nx]);
                    __builtin_prefetch(S->col_idx + S->row_ptr[nx]);
                } else {
                    for (int q = ST.row_ptr[nx]; q < ST.row_ptr[nx + 1]; ++q) __builtin_prefetch(&P[ST.col_idx[q]], 1);
                    for (int q = S->row_ptr[nx]; q < S->row_ptr[nx + 1]; ++q) __builtin_prefetch(&P[S->col_idx[q]], 1);
                }
            }
        }
        for (int q = ST.row_ptr[c]; q < ST.row_ptr[c + 1]; ++q) {
            const int j = ST.col_idx[q];
            __builtin_prefetch(&P[j], 1);
            __builtin_prefetch(&S->row_ptr[j]);
        }
        for (int q = S->row_ptr[c]; q < S->row_ptr[c + 1]; ++q) __builtin_prefetch(&P[S->col_idx[q]], 1);
        for (int q = ST.row_ptr[c]; q < ST.row_ptr[c + 1]; ++q) __builtin_prefetch(S->col_idx + S->row_ptr[ST.col_idx[q]]);
        for (int q = ST.row_ptr[c]; q < ST.row_ptr[c + 1]; ++q) {
            const int j = ST.col_idx[q];
            if (P[j].mark != UNPT) continue;
            for (int r = S->row_ptr[j]; r < S->row_ptr[j + 1]; ++r) __builtin_prefetch(&P[S->col_idx[r]], 1);
        }
        mc = P[c].lambda;
        if (mc == 0) printf("### WARNING: Head of the list has measure 0!\n");
        P[c].mark = CGPT;
        P[c].lambda = 0;
        undecided--;
        bucket_remove(&B, mc, c);
        ncoarse++;

        /* points that c strongly influences become F */
        for (int q = ST.row_ptr[c]; q < ST.row_ptr[c + 1]; ++q) {
            int j = ST.col_idx[q];
            if (P[j].mark != UNPT) continue;
            P[j].mark = FGPT;
            bucket_remove(&B, P[j].lambda, j);
            undecided--;
            for (int r = S->row_ptr[j]; r < S->row_ptr[j + 1]; ++r) {
                int k = S->col_idx[r];
                if (P[k].mark != UNPT) continue;
                bucket_move(&B, P[k].lambda, P[k].lambda + 1, k);
                P[k].lambda++;
            }
        }
        /* points that strongly influence c lose one unit of measure */
        for (int q = S->row_ptr[c]; q < S->row_ptr[c + 1]; ++q) {
            int j = S->col_idx[q], m;
            if (P[j].mark != UNPT) continue;
            m = P[j].lambda;
            if (m - 1 > 0) {
                bucket_move(&B, m, m - 1, j);
                P[j].lambda = m - 1;
                continue;
            }
            bucket_remove(&B, m, j);
            P[j].lambda = --m;
            P[j].mark = FGPT;
            undecided--;
            for (int r = S->row_ptr[j]; r < S->row_ptr[j + 1]; ++r) {
                int k = S->col_idx[r];
                if (P[k].mark != UNPT) continue;
                bucket_move(&B, P[k].lambda, P[k].lambda + 1, k);
                P[k].lambda++;
            }
        }
    }

    const double t3 = SSS_get_time();
    lambda = (int *)SSS_calloc((size_t)n, sizeof(int));
    for (int i = 0; i < n; ++i) mark[i] = P[i].mark;
    free(B.pts);
    /* C1 criterion: two strongly coupled F points must share a strong C point. */
    owner = lambda;
    char *maybe = flag_unshared_rows(S, mark, owner);   /* the rows this pass can change */
    for (int i = 0; i < n; ++i) {
        int promoted = -1, have_promoted = 0;
        if (!maybe[i] || mark[i] != FGPT) continue;
        for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q)
            if (mark[S->col_idx[q]] == CGPT) owner[S->col_idx[q]] = i;
        for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q) {
            int j = S->col_idx[q], shares = 0;
            if (mark[j] != FGPT) continue;
            for (int r = S->row_ptr[j]; r < S->row_ptr[j + 1]; ++r)
                if (owner[S->col_idx[r]] == i) { shares = 1; break; }
            if (shares) continue;
            if (!have_promoted) {
                mark[j] = CGPT;
                ncoarse++;
                owner[j] = i;
                promoted = j;
                have_promoted = 1;
            } else {
                mark[i] = CGPT;
                mark[promoted] = FGPT;
                break;
            }
        }
    }
    free(maybe);

    if (timing)
        fprintf(stderr, "[setup]   RS split: drop %.3f s, transpose %.3f s, lists %.3f s, first pass %.3f s, C1 %.3f s\n",
                tdrop - t0, t1 - tdrop, t2 - t1, t3 - t2, SSS_get_time() - t3);
    SSS_imat_destroy(&ST);
    for (int m = 0; m < B.cap; ++m) free(B.b[m].e);
    free(B.b);
    free(lambda);
    return ncoarse;
}

/* ======================================================================================
 * PMIS C/F split (cs_type SSS_COARSE_PMIS; an engine extension, DESIGN.md "PMIS coarsening").
 * Input: the compacted S.  lambda_i = stored entries of S with column i; key_i = lambda_i << 32 |
 * h(i) with h a bijection of uint32, so keys are pairwise distinct and there is no tie rule.
 * Start: empty S row -> ISPT, else lambda_i = 0 -> FGPT, else undecided.  One round, on the marks
 * as they stand at its start: (a) an undecided i whose key exceeds the key of every undecided j in
 * S_i u S^T_i becomes CGPT; (b) then a still undecided i with a CGPT point in S_i becomes FGPT.
 * Rounds repeat until nobody is undecided (the largest undecided key always becomes C).  The marks
 * depend on S alone: this row-parallel host form and the device form (amg_amd/csrc/sss_pmis.hip)
 * agree bit for bit, whatever the thread count.
 * ====================================================================================== */
static inline uint32_t pmis_hash(uint32_t i)
{
    i ^= i >> 16;
    i *= 0x7feb352dU;
    i ^= i >> 15;
    i *= 0x846ca68bU;
    i ^= i >> 16;
    return i;
}

enum { kPmisMaxRounds = 4096 };

/* Host PMIS split of a compacted S.  Returns the C-point count, or ERROR_UNKNOWN past the round cap. */
static int pmis_split(SSS_IMAT *S, int *mark, int *rounds_out)
{
    const int n = S->num_rows;
    const int *ia = S->row_ptr, *ja = S->col_idx;
    SSS_IMAT ST;
    if (ia[n] > 0) {
        ST = SSS_imat_trans(S);
    } else {   /* no entry at all (never from the setup: drop_weak has failed then) */
        memset(&ST, 0, sizeof(ST));
        ST.row_ptr = (int *)SSS_calloc((size_t)n + 1, sizeof(int));
    }
    const int *ta = ST.row_ptr, *tj = ST.col_idx;
    uint64_t *key = (uint64_t *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(uint64_t));
    int *next = (int *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(int));
    long long undecided = 0;
    int ncoarse = 0, rounds = 0;

#pragma omp parallel for schedule(static) reduction(+ : undecided) if (n > 4096)
    for (int i = 0; i < n; ++i) {
        const int lambda = ta[i + 1] - ta[i];
        key[i] = (uint64_t)(uint32_t)lambda << 32 | pmis_hash((uint32_t)i);
        if (ia[i + 1] == ia[i]) mark[i] = ISPT;
        else if (lambda == 0) mark[i] = FGPT;
        else mark[i] = UNPT, undecided++;
    }
    while (undecided > 0 && rounds < kPmisMaxRounds) {
        int newc = 0;
        rounds++;
        /* (a) local maxima of the key among the undecided become C (reads mark, writes next) */
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : newc) if (n > 4096)
        for (int i = 0; i < n; ++i) {
            int top = mark[i] == UNPT;
            for (int q = ia[i]; top && q < ia[i + 1]; ++q)
                top = !(mark[ja[q]] == UNPT && key[ja[q]] > key[i]);
            for (int q = ta[i]; top && q < ta[i + 1]; ++q)
                top = !(mark[tj[q]] == UNPT && key[tj[q]] > key[i]);
            next[i] = top ? CGPT : mark[i];
            newc += top;
        }
        ncoarse += newc;
        /* (b) the undecided that depend on a C point become F (reads next, writes mark) */
        undecided = 0;
#pragma omp parallel for schedule(dynamic, 1024) reduction(+ : undecided) if (n > 4096)
        for (int i = 0; i < n; ++i) {
            int m = next[i];
            if (m == UNPT) {
                for (int q = ia[i]; q < ia[i + 1]; ++q)
                    if (next[ja[q]] == CGPT) { m = FGPT; break; }
                undecided += m == UNPT;
            }
            mark[i] = m;
        }
    }
    free(key);
    free(next);
    SSS_imat_destroy(&ST);
    if (rounds_out) *rounds_out = rounds;
    return undecided > 0 ? ERROR_UNKNOWN : ncoarse;
}

/* The host split on a given compacted S (tests; what the device split is checked against). */
int sss_pmis_host(const SSS_IMAT *S, int *mark, int *ncoarse, int *rounds)
{
    if (!S || !mark || S->num_rows <= 0) return ERROR_INPUT_PAR;
    SSS_IMAT s = *S;
    const int nc = pmis_split(&s, mark, rounds);
    if (nc < 0) return nc;
    if (ncoarse) *ncoarse = nc;
    return 0;
}

/* drop_weak + the PMIS split: on the device when one is present, the level has at least
 * SSS_SETUP_GPU_PMIS_MIN strong entries and SSS_SETUP_GPU_PMIS is not 0; else, or when the device
 * split fails, on the host.  Returns the C-point count (or <0). */
static int pmis_coarsen(SSS_IMAT *S, SSS_IVEC *vertices)
{
    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const char *gp = getenv("SSS_SETUP_GPU_PMIS"), *gpm = getenv("SSS_SETUP_GPU_PMIS_MIN");
    const int gpu_min = (gpm && *gpm) ? atoi(gpm) : SSS_SETUP_GPU_PMIS_MIN_DEFAULT;
    int ncoarse, rounds = 0, on_device = 0;
    const double t0 = SSS_get_time();
    ncoarse = drop_weak(S);
    if (ncoarse < 0) return ncoarse;
    const double t1 = SSS_get_time();
    if (!(gp && gp[0] == '0') && S->num_nnzs >= gpu_min && sss_hip_device_count() > 0)
        on_device = sss_hip_pmis(S, vertices->d, &ncoarse, &rounds) == 0;
    if (!on_device) ncoarse = pmis_split(S, vertices->d, &rounds);
    if (timing)
        fprintf(stderr, "[setup]   PMIS split: drop %.3f s, %s split %.4f s, %d rounds, %d strong entries\n", t1 - t0,
                on_device ? "device" : "host", SSS_get_time() - t1, rounds, S->num_nnzs);
    return ncoarse;
}

/* Setup/SSS_coarsen.c:501-574.  Note: the tentative-C state (pending, pending_owner,
 * tentative) deliberately persists across rows exactly as in the reference. */
static int cleanup_ff(const SSS_IMAT *S, SSS_IVEC *vertices, int n, int ncoarse)
{
    int *mark = vertices->d;
    int *tag = (int *)SSS_calloc((size_t)n, sizeof(int));
    int pending = FALSE, pending_owner = -1, tentative = -1;
    char *maybe = flag_unshared_rows(S, mark, tag);   /* the rows this pass can change; tag = -1 */

    for (int i = 0; i < n; ++i) {
        if (mark[i] != FGPT) continue;
        if (!maybe[i]) {   /* no unshared pair: the row only resets the tentative C point */
            if (pending_owner != i) tentative = -1;
            continue;
        }
        for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q) {
            int j = S->col_idx[q];
            tag[j] = (mark[j] == CGPT) ? i : -1;
        }
        if (pending_owner != i) tentative = -1;
        for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q) {
            int j = S->col_idx[q], linked = 0;
            if (mark[j] != FGPT) continue;
            for (int r = S->row_ptr[j]; r < S->row_ptr[j + 1]; ++r)
                if (tag[S->col_idx[r]] == i) { linked = 1; break; }
            if (linked) continue;
            if (pending) {
                mark[i] = CGPT;
                ncoarse++;
                if (tentative > -1) {
                    mark[tentative] = FGPT;
                    ncoarse--;
                    tentative = -1;
                }
                pending = FALSE;
            } else {
                mark[j] = CGPT;
                ncoarse++;
                tentative = j;
                pending_owner = i;
                pending = TRUE;
                i--;                    /* revisit i with j as a C point */
            }
            break;
        }
    }
    free(maybe);
    free(tag);
    return ncoarse;
}

/* Setup/SSS_coarsen.c:577-630: F rows take their strong C neighbours, C rows themselves. */
static void direct_pattern(SSS_MAT *P, const SSS_IMAT *S, const SSS_IVEC *vertices, int n, int ncoarse)
{
    const int *mark = vertices->d;
    int pos = 0;
    P->num_rows = n;
    P->num_cols = ncoarse;
    P->row_ptr = (int *)SSS_calloc((size_t)n + 1, sizeof(int));
    /* row counts in parallel, prefix, then each row fills its own span (same arrays as the
     * reference's sequential pass) */
#pragma omp parallel for schedule(static) if (n > 65536)
    for (int i = 0; i < n; ++i) {
        int cnt = 0;
        if (mark[i] == FGPT) {
            for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q)
                if (mark[S->col_idx[q]] == CGPT) cnt++;
        } else if (mark[i] == CGPT) {
            cnt = 1;
        }
        P->row_ptr[i + 1] = cnt;
    }
    for (int i = 0; i < n; ++i) P->row_ptr[i + 1] += P->row_ptr[i];
    P->num_nnzs = P->row_ptr[n] - P->row_ptr[0];
    P->col_idx = (int *)SSS_calloc((size_t)P->num_nnzs, sizeof(int));
    P->val = (double *)SSS_calloc((size_t)P->num_nnzs, sizeof(double));
    (void)pos;
#pragma omp parallel for schedule(static) if (n > 65536)
    for (int i = 0; i < n; ++i) {
        int o = P->row_ptr[i];
        if (mark[i] == FGPT) {
            for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q)
                if (mark[S->col_idx[q]] == CGPT) P->col_idx[o++] = S->col_idx[q];
        } else if (mark[i] == CGPT) {
            P->col_idx[o] = i;
        }
    }
}

/* Per-thread scratch of a row-parallel loop: one buffer of `bytes` for each of up to
 * omp_get_max_threads() threads (at most 256), all of them together within a quarter of the
 * machine's memory (at least 2 GiB), fewer threads when an allocation fails.  Returns the threads
 * that got one; the loop runs on that many.  With none (even one buffer failed) the setup cannot go
 * on: the reference's allocation failure path (a warning, then the error exit). */
enum { kScratchMax = 256 };
static int scratch_alloc(size_t bytes, void **buf)
{
    const long pages = sysconf(_SC_PHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
    size_t budget = (pages > 0 && psz > 0) ? (size_t)pages * (size_t)psz / 4 : 0;
    if (budget < ((size_t)2 << 30)) budget = (size_t)2 << 30;
    if (bytes == 0) bytes = 1;
    int T = omp_get_max_threads();
    if (T > kScratchMax) T = kScratchMax;
    while (T > 1 && (size_t)T * bytes > budget) T--;
    int got = 0;
    while (got < T && (buf[got] = malloc(bytes)) != NULL) ++got;
    if (got == 0) {
        printf("### WARNING: Cannot allocate %.3lf MB RAM!\n", (double)bytes / 1048576);
        SSS_exit_on_errcode(ERROR_ALLOC_MEM, __func__);
    }
    return got;
}
static void scratch_free(void **buf, int T)
{
    for (int t = 0; t < T; ++t) free(buf[t]);
}

/* Setup/SSS_coarsen.c:633-725 (form_P_pattern_std): an F row takes its strong C neighbours and the
 * strong C neighbours of its strong F neighbours, each once, in discovery order; a C row its own
 * index; any other row nothing.  The reference's one `visited` array only ever answers "taken by
 * this row already?", so rows are independent: two row-parallel passes (count, then fill at the
 * prefix offsets), each thread with its own row-stamped array. */
static void std_pattern(SSS_MAT *P, const SSS_IMAT *S, const SSS_IVEC *vertices, int n, int ncoarse)
{
    const int *mark = vertices->d;
    void *scr[kScratchMax];
    const int T = scratch_alloc(sizeof(int) * (size_t)(n > 0 ? n : 1), scr);
    P->num_rows = n;
    P->num_cols = ncoarse;
    P->row_ptr = (int *)SSS_calloc((size_t)n + 1, sizeof(int));
    for (int fill = 0; fill < 2; ++fill) {
        if (fill) {
            for (int i = 0; i < n; ++i) P->row_ptr[i + 1] += P->row_ptr[i];
            P->num_nnzs = P->row_ptr[n] - P->row_ptr[0];
            P->col_idx = (int *)SSS_calloc((size_t)(P->num_nnzs > 0 ? P->num_nnzs : 1), sizeof(int));
            P->val = (double *)SSS_calloc((size_t)(P->num_nnzs > 0 ? P->num_nnzs : 1), sizeof(double));
        }
#pragma omp parallel num_threads(T) if (n > 4096)
        {
            int *seen = (int *)scr[omp_get_thread_num()];
            for (int i = 0; i < n; ++i) seen[i] = -1;
#pragma omp for schedule(dynamic, 1024)
            for (int i = 0; i < n; ++i) {
                int cnt = 0, o = fill ? P->row_ptr[i] : 0;
                if (mark[i] == FGPT) {
                    for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q) {
                        const int k = S->col_idx[q];
                        if (mark[k] == CGPT && seen[k] != i) {
                            seen[k] = i;
                            if (fill) P->col_idx[o++] = k;
                            cnt++;
                        } else if (mark[k] == FGPT && k != i) {
                            for (int r = S->row_ptr[k]; r < S->row_ptr[k + 1]; ++r) {
                                const int h = S->col_idx[r];
                                if (mark[h] == CGPT && seen[h] != i) {
                                    seen[h] = i;
                                    if (fill) P->col_idx[o++] = h;
                                    cnt++;
                                }
                            }
                        }
                    }
                } else if (mark[i] == CGPT) {
                    cnt = 1;
                    if (fill) P->col_idx[o] = i;
                }
                if (!fill) P->row_ptr[i + 1] = cnt;
            }
        }
    }
    scratch_free(scr, T);
}

/* The host pattern on a given compacted S and marks (tests; what the device pattern is checked against). */
int sss_std_pattern_host(const SSS_IMAT *S, const int *mark, int ncoarse, SSS_MAT *P)
{
    if (!S || !mark || !P || S->num_rows <= 0 || !S->row_ptr) return ERROR_INPUT_PAR;
    SSS_IVEC v = {S->num_rows, (int *)mark};
    std_pattern(P, S, &v, S->num_rows, ncoarse);
    return 0;
}

/* ======================================================================================
 * Aggressive coarsening (cs_type SSS_COARSE_PMIS_AGG; an engine extension): the PMIS
 * split, then a second PMIS split over the distance-two graph S2 of its C points.
 *
 * S2 has one row per stage-one C point, numbered c(i) in increasing i.  Row c(i) is one walk of S_i in
 * stored order: for each k != i of S_i, k itself when it is a C point, then (whatever k's mark) every
 * C point l != i of S_k in stored order; each candidate once, at its first occurrence, as column c(l).
 * It is std_pattern's rule with C rows in place of F rows and every k as an intermediate point, and
 * row-parallel in the same way (count, prefix, fill; per-thread row-stamped array).
 * ====================================================================================== */
static void agg_graph(const SSS_IMAT *S, const int *mark, SSS_IMAT *S2)
{
    const int n = S->num_rows;
    const int *ia = S->row_ptr, *ja = S->col_idx;
    int *cnum = (int *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(int));
    int *crow = (int *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(int));
    int nc = 0;
    for (int i = 0; i < n; ++i) {
        cnum[i] = -1;
        if (mark[i] == CGPT) cnum[i] = nc, crow[nc++] = i;
    }
    void *scr[kScratchMax];
    const int T = scratch_alloc(sizeof(int) * (size_t)(n > 0 ? n : 1), scr);
    int *rp = (int *)SSS_calloc((size_t)nc + 1, sizeof(int)), *ci = NULL;
    for (int fill = 0; fill < 2; ++fill) {
        if (fill) {
            for (int c = 0; c < nc; ++c) rp[c + 1] += rp[c];
            ci = (int *)SSS_calloc((size_t)(rp[nc] > 0 ? rp[nc] : 1), sizeof(int));
        }
#pragma omp parallel num_threads(T) if (nc > 4096)
        {
            int *seen = (int *)scr[omp_get_thread_num()];
            for (int i = 0; i < n; ++i) seen[i] = -1;
#pragma omp for schedule(dynamic, 1024)
            for (int c = 0; c < nc; ++c) {
                const int i = crow[c];
                int cnt = 0, o = fill ? rp[c] : 0;
                for (int q = ia[i]; q < ia[i + 1]; ++q) {
                    const int k = ja[q];
                    if (k == i) continue;
                    if (mark[k] == CGPT && seen[k] != i) {
                        seen[k] = i;
                        if (fill) ci[o++] = cnum[k];
                        cnt++;
                    }
                    for (int r = ia[k]; r < ia[k + 1]; ++r) {
                        const int l = ja[r];
                        if (l != i && mark[l] == CGPT && seen[l] != i) {
                            seen[l] = i;
                            if (fill) ci[o++] = cnum[l];
                            cnt++;
                        }
                    }
                }
                if (!fill) rp[c + 1] = cnt;
            }
        }
    }
    scratch_free(scr, T);
    free(cnum);
    free(crow);
    memset(S2, 0, sizeof(*S2));
    S2->num_rows = S2->num_cols = nc;
    S2->num_nnzs = rp[nc];
    S2->row_ptr = rp;
    S2->col_idx = ci;
}

static int agg_check(const SSS_IMAT *S, const int *mark)
{
    if (!S || !mark || S->num_rows <= 0 || !S->row_ptr) return ERROR_INPUT_PAR;
    const int n = S->num_rows, nnz = S->row_ptr[n];
    if (S->row_ptr[0] != 0 || nnz < 0 || (nnz > 0 && !S->col_idx)) return ERROR_INPUT_PAR;
    for (int i = 0; i < n; ++i)
        if (S->row_ptr[i + 1] < S->row_ptr[i]) return ERROR_DATA_STRUCTURE;
    for (int q = 0; q < nnz; ++q)
        if ((unsigned)S->col_idx[q] >= (unsigned)n) return ERROR_DATA_STRUCTURE;
    return 0;
}

/* The host graph on a given compacted S and stage-one marks (tests; what the device graph is checked
 * against).  S2 is written on success only; its arrays are the library's (SSS_imat_destroy). */
int sss_agg_graph_host(const SSS_IMAT *S, const int *mark, SSS_IMAT *S2)
{
    if (!S2) return ERROR_INPUT_PAR;
    const int rc = agg_check(S, mark);
    if (rc) return rc;
    agg_graph(S, mark, S2);
    return 0;
}

/* The final marks: a stage-one C point stays C when stage two made it C or found its S2 row empty
 * (ISPT: nobody to interpolate from), else it becomes F; every other point keeps its mark.  m2 is in
 * the C numbering.  Returns the C-point count. */
static int agg_final_marks(int n, int *mark, const int *m2)
{
    int c = 0, ncoarse = 0;
    for (int i = 0; i < n; ++i) {
        if (mark[i] != CGPT) continue;
        if (m2[c] == CGPT || m2[c] == ISPT) ncoarse++;
        else mark[i] = FGPT;
        c++;
    }
    return ncoarse;
}

/* Whether S2 and the stage-two split of a level with nnz nonzeros in A go to the device: a device is
 * present, SSS_SETUP_GPU_AGG is not 0 and nnz is at least SSS_SETUP_GPU_AGG_MIN (include/sss_hip.h). */
static int agg_on_device(int nnz)
{
    const char *g = getenv("SSS_SETUP_GPU_AGG"), *gm = getenv("SSS_SETUP_GPU_AGG_MIN");
    const int gpu_min = (gm && *gm) ? atoi(gm) : SSS_SETUP_GPU_AGG_MIN_DEFAULT;
    return !(g && g[0] == '0') && nnz >= gpu_min && sss_hip_device_count() > 0;
}

/* Stage two on marks that hold the stage-one split of S: S2, the existing split on it, the final
 * marks.  device: S2 may come from the GPU, and the split of S2 then follows its own SSS_SETUP_GPU_PMIS*
 * switches on S2's entry count; the host runs on any error code.  Returns the C-point count (or <0). */
static int agg_stage_two(const SSS_IMAT *S, int *mark, int device)
{
    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const char *gp = getenv("SSS_SETUP_GPU_PMIS"), *gpm = getenv("SSS_SETUP_GPU_PMIS_MIN");
    const int pmis_min = (gpm && *gpm) ? atoi(gpm) : SSS_SETUP_GPU_PMIS_MIN_DEFAULT;
    SSS_IMAT S2;
    const double t0 = SSS_get_time();
    /* the device graph is the host's, array for array (it prints its own timing line) */
    if (!(device && sss_hip_agg_graph(S, mark, &S2) == 0)) {
        agg_graph(S, mark, &S2);
        if (timing)
            fprintf(stderr, "[setup]   aggressive S2: host %.4f s, %d rows, %d entries\n", SSS_get_time() - t0, S2.num_rows,
                    S2.num_nnzs);
    }
    const double t1 = SSS_get_time();
    int *m2 = (int *)SSS_calloc((size_t)(S2.num_rows > 0 ? S2.num_rows : 1), sizeof(int));
    int nc2 = 0, rounds = 0, on_device = 0, ncoarse;
    if (device && !(gp && gp[0] == '0') && S2.num_nnzs >= pmis_min)
        on_device = sss_hip_pmis(&S2, m2, &nc2, &rounds) == 0;
    if (!on_device) nc2 = pmis_split(&S2, m2, &rounds);
    if (timing)
        fprintf(stderr, "[setup]   aggressive stage-two split: %s %.4f s, %d rounds, %d rows, %d entries\n",
                on_device ? "device" : "host", SSS_get_time() - t1, rounds, S2.num_rows, S2.num_nnzs);
    ncoarse = nc2 < 0 ? nc2 : agg_final_marks(S->num_rows, mark, m2);
    free(m2);
    SSS_imat_destroy(&S2);
    return ncoarse;
}

/* The two-stage split on a given compacted S, on the host (tests).  mark and *ncoarse are written on
 * success only. */
int sss_pmis_agg_host(const SSS_IMAT *S, int *mark, int *ncoarse)
{
    int rc = agg_check(S, mark);
    if (rc) return rc;
    SSS_IMAT s = *S;
    int *m = (int *)SSS_calloc((size_t)S->num_rows, sizeof(int));
    rc = pmis_split(&s, m, NULL);
    if (rc > 0) rc = agg_stage_two(S, m, 0);
    if (rc >= 0) {
        memcpy(mark, m, sizeof(int) * (size_t)S->num_rows);
        if (ncoarse) *ncoarse = rc;
    }
    free(m);
    return rc < 0 ? rc : 0;
}

/* Levels on which cs_type SSS_COARSE_PMIS_AGG is aggressive (SSS_SETUP_AGG_LEVELS, default 1, 0
 * allowed): SSS_AMG_PARS keeps the reference's layout, so the count cannot live there. */
static int agg_levels(void)
{
    const char *e = getenv("SSS_SETUP_AGG_LEVELS");
    const int v = (e && *e) ? atoi(e) : 1;
    return v > 0 ? v : 0;
}

/* Whether a level with nnz nonzeros in A takes the device pattern and weights: a device is present,
 * SSS_SETUP_GPU_INTERP is not 0 and nnz is at least SSS_SETUP_GPU_INTERP_MIN (include/sss_hip.h). */
static int interp_on_device(int nnz)
{
    const char *g = getenv("SSS_SETUP_GPU_INTERP"), *gm = getenv("SSS_SETUP_GPU_INTERP_MIN");
    const int gpu_min = (gm && *gm) ? atoi(gm) : SSS_SETUP_GPU_INTERP_MIN_DEFAULT;
    return !(g && g[0] == '0') && nnz >= gpu_min && sss_hip_device_count() > 0;
}

/* SSS_amg_coarsen on level lvl of the hierarchy: cs_type SSS_COARSE_PMIS_AGG is aggressive on the
 * first SSS_SETUP_AGG_LEVELS levels and SSS_COARSE_PMIS after them. */
static int amg_coarsen_level(SSS_MAT *A, SSS_IVEC *vertices, SSS_MAT *P, SSS_IMAT *S, SSS_AMG_PARS *pars, int lvl)
{
    int ncoarse = 0;
    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const double t0 = SSS_get_time();
    strong_couplings(A, S, pars);
    const double t1 = SSS_get_time();
    const int agg = pars->cs_type == SSS_COARSE_PMIS_AGG && lvl < agg_levels();
    const int pmis = pars->cs_type == SSS_COARSE_PMIS || pars->cs_type == SSS_COARSE_PMIS_AGG;
    const char *split = agg ? "aggressive PMIS" : pmis ? "PMIS" : "RS";
    if (pars->cs_type == SSS_COARSE_RS) ncoarse = rs_split(A, S, vertices);
    else if (pmis) ncoarse = pmis_coarsen(S, vertices);
    else if (pars->cs_type != SSS_COARSE_RSP) SSS_exit_on_errcode(ERROR_AMG_COARSE_TYPE, __func__);
    if (agg && ncoarse > 0) ncoarse = agg_stage_two(S, vertices->d, agg_on_device(A->num_nnzs));
    if (ncoarse <= 0) return ERROR_UNKNOWN;
    const double t2 = SSS_get_time();
    if (agg || pars->interp_type == intERP_MPASS) {
        /* multipass interpolation builds its pattern pass by pass with the weights (interp_MPASS):
         * P leaves here with its sizes and no arrays, which is how SSS_amg_interp knows the level */
        if (pars->interp_type < intERP_DIR || pars->interp_type > intERP_MPASS)
            SSS_exit_on_errcode(ERROR_AMG_interp_type, __func__);
        memset(P, 0, sizeof(*P));
        P->num_rows = A->num_rows;
        P->num_cols = ncoarse;
        if (timing)
            fprintf(stderr, "[setup]   coarsen: strength %.3f s, %s split %.3f s, multipass P follows\n", t1 - t0, split,
                    t2 - t1);
    } else if (pars->interp_type == intERP_DIR) {
        /* the F-F cleanup never runs after PMIS: it promotes until every strong F-F pair shares a
         * C point, which undoes the split (DESIGN.md "PMIS coarsening") */
        if (!pmis) ncoarse = cleanup_ff(S, vertices, A->num_rows, ncoarse);
        const double t3 = SSS_get_time();
        direct_pattern(P, S, vertices, A->num_rows, ncoarse);
        if (timing)
            fprintf(stderr, "[setup]   coarsen: strength %.3f s, %s split %.3f s, F-F cleanup %.3f s, P pattern %.3f s\n",
                    t1 - t0, split, t2 - t1, t3 - t2, SSS_get_time() - t3);
    } else if (pars->interp_type == intERP_STD || pars->interp_type == intERP_EXTI) {
        /* no F-F cleanup before the standard pattern; the extended+i weights use the same pattern */
        const double t3 = SSS_get_time();
        /* the device pattern is the host's, array for array; on any error code the host builds it */
        if (!(interp_on_device(A->num_nnzs) && sss_hip_std_pattern(S, vertices->d, ncoarse, P) == 0)) {
            std_pattern(P, S, vertices, A->num_rows, ncoarse);
            if (timing)
                fprintf(stderr, "[setup]   standard P: host pattern %.4f s, %d rows, %d entries\n", SSS_get_time() - t3,
                        P->num_rows, P->num_nnzs);
        }
        if (timing)
            fprintf(stderr, "[setup]   coarsen: strength %.3f s, %s split %.3f s, standard P pattern %.3f s\n", t1 - t0,
                    split, t2 - t1, SSS_get_time() - t3);
    } else {
        SSS_exit_on_errcode(ERROR_AMG_interp_type, __func__);
    }
    return 0;
}

/* One level on its own is the finest one. */
int SSS_amg_coarsen(SSS_MAT *A, SSS_IVEC *vertices, SSS_MAT *P, SSS_IMAT *S, SSS_AMG_PARS *pars)
{
    return amg_coarsen_level(A, vertices, P, S, pars, 0);
}

/* ======================================================================================
 * Interpolation and truncation
 * ====================================================================================== */
/* The cap on the entries per row of P (SSS_SETUP_PMAX, 0 = off; include/sss_hip.h): SSS_AMG_PARS keeps
 * the reference's layout, so the value cannot live there. */
int sss_setup_pmax(void)
{
    const char *e = getenv("SSS_SETUP_PMAX");
    const int v = (e && *e) ? atoi(e) : 0;
    return v > 0 ? v : 0;
}

/* Whether the cap cuts row [lo, hi) of val, whose thresholds are tp and tn: it does when more than pmax
 * entries survive them.  Then (*cut_a, *cut_k) is the key (|v|, stored position) of the pmax-th survivor
 * in the order "larger |v| first, earlier position on ties": the kept entries are the survivors at or
 * before it in that order.  Found in pmax rounds, each the largest key strictly after the previous
 * round's pick, so that nothing is stored per entry (the device kernel does the same rounds). */
static int trunc_cut(const double *val, int lo, int hi, double tp, double tn, int pmax, double *cut_a, int *cut_k)
{
    int survivors = 0;
    if (pmax <= 0) return 0;
    for (int k = lo; k < hi; ++k) survivors += (val[k] >= tp) || (val[k] <= tn);
    if (survivors <= pmax) return 0;
    double pa = 0.0;
    int pk = -1;
    for (int r = 0; r < pmax; ++r) {
        double ba = -1.0;
        int bk = -1;
        for (int k = lo; k < hi; ++k) {
            const double v = val[k], a = fabs(v);
            if (!(v >= tp || v <= tn)) continue;
            if (r > 0 && !(a < pa || (a == pa && k > pk))) continue;   /* picked by an earlier round */
            if (a > ba) { ba = a; bk = k; }                             /* ties: the earlier position stays */
        }
        if (bk < 0) break;
        pa = ba;
        pk = bk;
    }
    *cut_a = pa;
    *cut_k = pk;
    return 1;
}

/* The factors of a capped row: the SMALLFLOAT rule, and a class the cap removed entirely hands its sum
 * to the other one, so that the row sum of P survives the cap. */
static void trunc_capped_factors(double pos_sum, double neg_sum, double pos_kept, double neg_kept, double *pos_fac,
                                 double *neg_fac)
{
    const int pos_has = pos_kept > SMALLFLOAT, neg_has = neg_kept < -SMALLFLOAT;
    *pos_fac = pos_has ? pos_sum / pos_kept : 1.0;
    *neg_fac = neg_has ? neg_sum / neg_kept : 1.0;
    if (pos_sum > 0 && !pos_has && neg_has) *neg_fac = (pos_sum + neg_sum) / neg_kept;
    if (neg_sum < 0 && !neg_has && pos_has) *pos_fac = (pos_sum + neg_sum) / pos_kept;
}

#define TRUNC_KEPT(v, k) (((v) >= pos_max || (v) <= neg_min) && \
                          (!capped || fabs(v) > cut_a || (fabs(v) == cut_a && (k) <= cut_k)))

/* Per-row form of the truncation below for large P: the same kept entries and scaled values,
 * computed row-parallel into new arrays (kept counts, prefix, fill). */
static void interp_trunc_par(SSS_MAT *P, double eps, int pmax)
{
    const int n = P->num_rows;
    int *nrp = (int *)SSS_calloc((size_t)n + 1, sizeof(int));
#pragma omp parallel for schedule(dynamic, 1024)
    for (int i = 0; i < n; ++i) {
        const int lo = P->row_ptr[i], hi = P->row_ptr[i + 1];
        double pos_max = 0, neg_min = 0;
        int c = 0;
        for (int k = lo; k < hi; ++k) {
            double v = P->val[k];
            if (v > 0) pos_max = SSS_max(pos_max, v);
            else if (v < 0) neg_min = SSS_MIN(neg_min, v);
        }
        pos_max *= eps;
        neg_min *= eps;
        for (int k = lo; k < hi; ++k) c += (P->val[k] >= pos_max) || (P->val[k] <= neg_min);
        nrp[i + 1] = (pmax > 0 && c > pmax) ? pmax : c;
    }
    for (int i = 0; i < n; ++i) nrp[i + 1] += nrp[i];
    const int kept = nrp[n];
    int *nci = (int *)SSS_calloc((size_t)(kept > 0 ? kept : 1), sizeof(int));
    double *nv = (double *)SSS_calloc((size_t)(kept > 0 ? kept : 1), sizeof(double));
#pragma omp parallel for schedule(dynamic, 1024)
    for (int i = 0; i < n; ++i) {
        const int lo = P->row_ptr[i], hi = P->row_ptr[i + 1];
        double pos_max = 0, neg_min = 0, pos_sum = 0, neg_sum = 0, pos_kept = 0, neg_kept = 0;
        double pos_fac, neg_fac, cut_a = 0.0;
        int cut_k = -1;
        for (int k = lo; k < hi; ++k) {
            double v = P->val[k];
            if (v > 0) { pos_sum += v; pos_max = SSS_max(pos_max, v); }
            else if (v < 0) { neg_sum += v; neg_min = SSS_MIN(neg_min, v); }
        }
        pos_max *= eps;
        neg_min *= eps;
        const int capped = trunc_cut(P->val, lo, hi, pos_max, neg_min, pmax, &cut_a, &cut_k);
        int o = nrp[i];
        const int end = nrp[i + 1];
        for (int k = lo; k < hi && o < end; ++k) {
            double v = P->val[k];
            if (!TRUNC_KEPT(v, k)) continue;
            nci[o++] = P->col_idx[k];
            if (v >= pos_max) pos_kept += v;
            else neg_kept += v;
        }
        if (capped) {
            trunc_capped_factors(pos_sum, neg_sum, pos_kept, neg_kept, &pos_fac, &neg_fac);
        } else {
            pos_fac = pos_kept > SMALLFLOAT ? pos_sum / pos_kept : 1.0;
            neg_fac = neg_kept < -SMALLFLOAT ? neg_sum / neg_kept : 1.0;
        }
        o = nrp[i];
        for (int k = lo; k < hi && o < end; ++k) {
            double v = P->val[k];
            if (!TRUNC_KEPT(v, k)) continue;
            nv[o++] = v >= pos_max ? v * pos_fac : v * neg_fac;
        }
    }
    free(P->row_ptr);
    free(P->col_idx);
    free(P->val);
    P->row_ptr = nrp;
    P->col_idx = nci;
    P->val = nv;
    P->num_nnzs = kept;
}

/* 0 when P is a CSR matrix the truncation can walk: monotone row pointers from 0, arrays where there
 * are entries (include/sss_hip.h sss_interp_trunc_host). */
static int trunc_check(const SSS_MAT *P, int pmax)
{
    if (pmax < 0 || !P || P->num_rows <= 0 || !P->row_ptr || P->row_ptr[0] != 0) return ERROR_INPUT_PAR;
    for (int i = 0; i < P->num_rows; ++i)
        if (P->row_ptr[i + 1] < P->row_ptr[i]) return ERROR_INPUT_PAR;
    const int nnz = P->row_ptr[P->num_rows];
    if (nnz != P->num_nnzs || (nnz > 0 && (!P->col_idx || !P->val))) return ERROR_INPUT_PAR;
    return 0;
}

int sss_interp_trunc_host(SSS_MAT *P, double eps, int pmax)
{
    const int rc = trunc_check(P, pmax);
    if (rc) return rc;
    interp_trunc_par(P, eps, pmax);
    return 0;
}

void SSS_amg_interp_trunc(SSS_MAT *P, SSS_AMG_PARS *pars)
{
    const double eps = pars->trunc_threshold;
    const int pmax = sss_setup_pmax();
    int kept = 0, wcol = 0, wval = 0;
    if (P->num_nnzs >= (1 << 20)) {
        /* one timing line of its own, only when SSS_SETUP_PMAX is set (0: the uncapped truncation) */
        const int timing = getenv("SSS_SETUP_TIMING") && getenv("SSS_SETUP_PMAX");
        const int before = P->num_nnzs;
        const double t0 = SSS_get_time();
        interp_trunc_par(P, eps, pmax);
        if (timing)
            fprintf(stderr, "[setup]   truncation: host, cap %d, %d rows, %d of %d entries kept, %.4f s\n", pmax, P->num_rows,
                    P->num_nnzs, before, SSS_get_time() - t0);
        return;
    }
    for (int i = 0; i < P->num_rows; ++i) {
        const int lo = P->row_ptr[i], hi = P->row_ptr[i + 1];
        double pos_max = 0, neg_min = 0, pos_sum = 0, neg_sum = 0, pos_kept = 0, neg_kept = 0;
        double pos_fac, neg_fac, cut_a = 0.0;
        int cut_k = -1;
        P->row_ptr[i] = kept;
        for (int k = lo; k < hi; ++k) {
            double v = P->val[k];
            if (v > 0) { pos_sum += v; pos_max = SSS_max(pos_max, v); }
            else if (v < 0) { neg_sum += v; neg_min = SSS_MIN(neg_min, v); }
        }
        pos_max *= eps;
        neg_min *= eps;
        /* the cut is found before the row is compacted in place (the writes below stay behind the reads) */
        const int capped = trunc_cut(P->val, lo, hi, pos_max, neg_min, pmax, &cut_a, &cut_k);
        for (int k = lo; k < hi; ++k) {
            double v = P->val[k];
            if (!TRUNC_KEPT(v, k)) continue;
            kept++;
            P->col_idx[wcol++] = P->col_idx[k];
            if (v >= pos_max) pos_kept += v;
            else neg_kept += v;
        }
        if (capped) {
            trunc_capped_factors(pos_sum, neg_sum, pos_kept, neg_kept, &pos_fac, &neg_fac);
        } else {
            pos_fac = pos_kept > SMALLFLOAT ? pos_sum / pos_kept : 1.0;
            neg_fac = neg_kept < -SMALLFLOAT ? neg_sum / neg_kept : 1.0;
        }
        for (int k = lo; k < hi; ++k) {
            double v = P->val[k];
            if (!TRUNC_KEPT(v, k)) continue;
            P->val[wval++] = v >= pos_max ? v * pos_fac : v * neg_fac;
        }
    }
    P->num_nnzs = P->row_ptr[P->num_rows] = kept;
    P->col_idx = (int *)SSS_realloc(P->col_idx, (size_t)kept * sizeof(int));
    P->val = (double *)SSS_realloc(P->val, (size_t)kept * sizeof(double));
}
#undef TRUNC_KEPT

/*
 * Setup/SSS_inter.cu:400-547.  `aii` is carried from row to row exactly as the host twin
 * does (a row without a diagonal entry reuses the previous row's value, including the
 * apN correction) — resolved up front so the weight computation can run row-parallel.
 */
void interp_DIR(SSS_MAT *A, SSS_IVEC *vertices, SSS_MAT *P, SSS_AMG_PARS *pars)
{
    const int n = A->num_rows;
    const int *mark = vertices->d;
    const int *ia = A->row_ptr, *ja = A->col_idx;
    const double *a = A->val;
    double *aii_row = (double *)sss_big_malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    int *diag_pos = (int *)sss_big_malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
    int *cmap;
    double t0 = SSS_get_time(), carried = 0.0;
    int ncoarse = 0;

    /* pass 1: diagonal positions; apN corrections are needed only where the chain matters */
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) {
        int d = ia[i + 1];
        for (int k = ia[i]; k < ia[i + 1]; ++k)
            if (ja[k] == i) { d = k; break; }
        diag_pos[i] = d;
    }
    /* pass 2: the per-row apN correction (row-parallel; stored in aii_row), then the carried aii
     * resolved in row order (a row without a diagonal entry takes the previous row's value) */
#pragma omp parallel for schedule(static)
    for (int i = 0; i < n; ++i) {
        double apN = 0.0;
        int npos = 0, corr = 0;
        if (mark[i] == FGPT) {
            for (int k = ia[i]; k < ia[i + 1]; ++k) {
                if (k == diag_pos[i] || !(a[k] > 0)) continue;
                apN += a[k];
                for (int q = P->row_ptr[i]; q < P->row_ptr[i + 1]; ++q)
                    if (P->col_idx[q] == ja[k]) { npos++; break; }
            }
            corr = npos == 0;
        }
        aii_row[i] = apN;
        if (!corr) diag_pos[i] = -2 - diag_pos[i];   /* flag "no correction", position kept */
    }
    for (int i = 0; i < n; ++i) {
        const int corr = diag_pos[i] >= 0;
        const int d = corr ? diag_pos[i] : -2 - diag_pos[i];
        if (!corr) diag_pos[i] = d;
        double aii = d < ia[i + 1] ? a[d] : carried;
        if (corr) aii += aii_row[i];
        aii_row[i] = aii;
        carried = aii;
    }
    /* pass 3: weights, row-parallel */
#pragma omp parallel for schedule(dynamic, 4096)
    for (int i = 0; i < n; ++i) {
        const double aii = aii_row[i];
        if (mark[i] == FGPT) {
            double amN = 0.0, amP = 0.0, apN = 0.0, apP = 0.0, alpha, beta;
            int npos = 0;
            for (int k = ia[i]; k < ia[i + 1]; ++k) {
                int strong = FALSE;
                if (k == diag_pos[i]) continue;
                for (int q = P->row_ptr[i]; q < P->row_ptr[i + 1]; ++q)
                    if (P->col_idx[q] == ja[k]) { strong = TRUE; break; }
                if (a[k] > 0) {
                    apN += a[k];
                    if (strong) { apP += a[k]; npos++; }
                } else {
                    amN += a[k];
                    if (strong) amP += a[k];
                }
            }
            alpha = amN / amP;
            beta = npos > 0 ? apN / apP : 0.0;
            for (int q = P->row_ptr[i]; q < P->row_ptr[i + 1]; ++q) {
                int k = ia[i];
                while (k < ia[i + 1] && ja[k] != P->col_idx[q]) ++k;
                P->val[q] = a[k] > 0 ? -beta * a[k] / aii : -alpha * a[k] / aii;
            }
        } else if (mark[i] == CGPT) {
            P->val[P->row_ptr[i]] = 1.0;
        }
    }
    printf("-------------cpu_step1_time = %f ms -------------------\n", (SSS_get_time() - t0) * 1000.0);

    /* coarse renumbering */
    cmap = (int *)SSS_calloc((size_t)n, sizeof(int));
    for (int i = 0; i < n; ++i)
        if (mark[i] == CGPT) cmap[i] = ncoarse++;
    P->num_cols = ncoarse;
#pragma omp parallel for schedule(static)
    for (int q = 0; q < P->num_nnzs; ++q) P->col_idx[q] = cmap[P->col_idx[q]];
    free(cmap);
    free(aii_row);
    free(diag_pos);
    SSS_amg_interp_trunc(P, pars);
}

/*
 * Setup/SSS_inter.cu:550-715 (interp_STD), on the pattern std_pattern built.  Per F row i, with
 * hat a the row's entries eliminated through its strong F neighbours k:
 *   hat a_ii = a_ii - sum_k (a_ik / a_kk) a_ki,   hat a_il = a_il [l in C_i^s] - sum_k (a_ik / a_kk) a_kl [l in C_k^s]
 *   alpha = (psum_i - sum_k f_k (nsum_k - a_ki + a_kk)) / (csum_i - sum_k f_k csum_k),
 *   p_il = -alpha hat a_il / hat a_ii
 * (psum: off-diagonal entries whose column is not isolated; nsum: all off-diagonal entries; csum:
 * the entries of strong C neighbours; every sum in stored order).  The reference's per-row scratch
 * (reverse indices of rows i and k, hat a) is reset or fully rewritten for each row before it is
 * read, so the rows are computed in parallel with per-thread scratch; each row's arithmetic is the
 * reference's, in its order.  (The reference also sets the process's OpenMP thread count to 8 here,
 * a speed-only side effect not reproduced.)  Then the coarse renumbering and the truncation.
 */
static void interp_STD(SSS_MAT *A, SSS_IVEC *vertices, SSS_MAT *P, SSS_IMAT *S, SSS_AMG_PARS *pars)
{
    const int n = A->num_rows, nc = A->num_cols > n ? A->num_cols : n;
    const int *mark = vertices->d;
    const int *ia = A->row_ptr, *ja = A->col_idx;
    const double *a = A->val;
    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const double t0 = SSS_get_time();
    /* the device weights (renumbered, truncated) are the host's bit for bit; on any error code P is
     * untouched and the host computes them */
    if (interp_on_device(A->num_nnzs) && sss_hip_interp_std(A, S, mark, P, pars->trunc_threshold) == 0) return;
    double *csum = (double *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(double));
    double *psum = (double *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(double));
    double *nsum = (double *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(double));
    double *diag = (double *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(double));

    /* step 0: diagonal (the row's last diagonal entry), strong-C, off-diagonal and non-isolated sums */
#pragma omp parallel for schedule(dynamic, 4096) if (n > 65536)
    for (int i = 0; i < n; ++i) {
        double cs = 0.0, ns = 0.0, ps = 0.0, d = 0.0;
        for (int j = ia[i]; j < ia[i + 1]; ++j) {
            const int k = ja[j];
            int strong_c = 0;
            if (mark[k] == CGPT)
                for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1] && !strong_c; ++q) strong_c = S->col_idx[q] == k;
            if (strong_c) cs += a[j];
            if (k == i) {
                d = a[j];
            } else {
                ns += a[j];
                if (mark[k] != ISPT) ps += a[j];
            }
        }
        csum[i] = cs, nsum[i] = ns, psum[i] = ps, diag[i] = d;
    }

    /* step 1: the weights */
    /* per thread: rindi and rindk (ints) and ahat (doubles), nc each, in one buffer */
    void *scr[kScratchMax];
    const size_t ncs = (size_t)(nc > 0 ? nc : 1);
    const int T = scratch_alloc(ncs * (2 * sizeof(int) + sizeof(double)), scr);
#pragma omp parallel num_threads(T) if (n > 4096)
    {
        double *ahat = (double *)scr[omp_get_thread_num()];
        int *rindi = (int *)(ahat + ncs), *rindk = rindi + ncs;
#pragma omp for schedule(dynamic, 1024)
        for (int i = 0; i < n; ++i) {
            if (mark[i] == CGPT) {
                P->val[P->row_ptr[i]] = 1.0;
                continue;
            }
            if (mark[i] != FGPT) continue;
            double alN = psum[i], alP = csum[i], alpha = 0.0;
            for (int j = ia[i]; j < ia[i + 1]; ++j) rindi[ja[j]] = j;
            for (int j = P->row_ptr[i]; j < P->row_ptr[i + 1]; ++j) ahat[P->col_idx[j]] = 0.0;
            ahat[i] = diag[i];
            for (int j = S->row_ptr[i]; j < S->row_ptr[i + 1]; ++j) {
                const int k = S->col_idx[j];
                const double aik = a[rindi[k]];
                if (mark[k] == CGPT) {
                    ahat[k] += aik;
                } else if (mark[k] == FGPT) {
                    const double akk = diag[k];
                    for (int m = ia[k]; m < ia[k + 1]; ++m) rindk[ja[m]] = m;
                    const double factor = aik / akk;
                    double aki = 0.0;
                    for (int m = ia[k]; m < ia[k + 1]; ++m)
                        if (ja[m] == i) {
                            aki = a[m];
                            ahat[i] -= factor * aki;
                        }
                    for (int m = S->row_ptr[k]; m < S->row_ptr[k + 1]; ++m) {
                        const int l = S->col_idx[m];
                        const double akl = a[rindk[l]];
                        if (mark[l] == CGPT) ahat[l] -= factor * akl;
                    }
                    alN -= factor * (nsum[k] - aki + akk);
                    alP -= factor * csum[k];
                }
            }
            if (P->row_ptr[i + 1] > P->row_ptr[i]) alpha = alN / alP;
            for (int j = P->row_ptr[i]; j < P->row_ptr[i + 1]; ++j) P->val[j] = -alpha * ahat[P->col_idx[j]] / ahat[i];
        }
    }
    scratch_free(scr, T);

    /* step 2: coarse renumbering of the columns */
    int *cmap = (int *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(int));
    int ncoarse = 0;
    for (int i = 0; i < n; ++i)
        if (mark[i] == CGPT) cmap[i] = ncoarse++;
    P->num_cols = ncoarse;
#pragma omp parallel for schedule(static) if (P->num_nnzs > 65536)
    for (int q = 0; q < P->row_ptr[P->num_rows]; ++q) P->col_idx[q] = cmap[P->col_idx[q]];
    free(cmap);
    free(csum);
    free(psum);
    free(nsum);
    free(diag);
    /* step 3 */
    SSS_amg_interp_trunc(P, pars);
    if (timing)
        fprintf(stderr, "[setup]   standard P: host weights %.4f s, %d rows, %d entries\n", SSS_get_time() - t0, P->num_rows,
                P->num_nnzs);
}

/*
 * Extended+i interpolation (interp_type intERP_EXTI, an engine extension; De Sterck, Falgout, Nolting,
 * Yang 2008) on the pattern std_pattern built.  Per F row i with pattern C_i, d = a_ii
 * (the row's last diagonal entry) and hat a = 0, the stored entries (i, k), k != i, in stored order:
 *   k in C_i (strongly or weakly coupled) ............ hat a_k += a_ik
 *   k a strong F neighbour (k in S_i, mark F) ........ over the entries (k, l), l != k, of row k with
 *       l in C_i or l == i, and a_kl a_kk < 0, in stored order: den = sum a_kl; when den != 0,
 *       f = a_ik / den and f a_kl goes to d (l == i) or to hat a_l; when den == 0, d += a_ik
 *   anything else ..................................... d += a_ik
 *   p_ic = -hat a_c / d
 * There is no alpha: a strong F neighbour is eliminated through the part of its row inside
 * C_i u {i}, so a row of A with zero sum gives a row of P with sum 1.  Rows are independent (per-thread
 * scratch: hat a, and two arrays stamped with the row for "in C_i" and "in S_i").  Then the coarse
 * renumbering and the truncation, as interp_STD.
 */
static void interp_EXTI(SSS_MAT *A, SSS_IVEC *vertices, SSS_MAT *P, SSS_IMAT *S, SSS_AMG_PARS *pars)
{
    const int n = A->num_rows, nc = A->num_cols > n ? A->num_cols : n;
    const int *mark = vertices->d;
    const int *ia = A->row_ptr, *ja = A->col_idx;
    const double *a = A->val;
    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const double t0 = SSS_get_time();
    /* the device weights (renumbered, truncated) are the host's bit for bit; on any error code P is
     * untouched and the host computes them */
    if (interp_on_device(A->num_nnzs) && sss_hip_interp_exti(A, S, mark, P, pars->trunc_threshold) == 0) return;
    double *diag = (double *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(double));
#pragma omp parallel for schedule(static) if (n > 65536)
    for (int i = 0; i < n; ++i) {
        double d = 0.0;
        for (int j = ia[i]; j < ia[i + 1]; ++j)
            if (ja[j] == i) d = a[j];
        diag[i] = d;
    }

    /* per thread: ahat (doubles), inpat and ins (ints), nc each, in one buffer */
    void *scr[kScratchMax];
    const size_t ncs = (size_t)(nc > 0 ? nc : 1);
    const int T = scratch_alloc(ncs * (2 * sizeof(int) + sizeof(double)), scr);
#pragma omp parallel num_threads(T) if (n > 4096)
    {
        double *ahat = (double *)scr[omp_get_thread_num()];
        int *inpat = (int *)(ahat + ncs), *ins = inpat + ncs;
        for (size_t c = 0; c < ncs; ++c) inpat[c] = ins[c] = -1;
#pragma omp for schedule(dynamic, 1024)
        for (int i = 0; i < n; ++i) {
            if (mark[i] == CGPT) {
                P->val[P->row_ptr[i]] = 1.0;
                continue;
            }
            if (mark[i] != FGPT || P->row_ptr[i + 1] == P->row_ptr[i]) continue;
            double d = diag[i];
            for (int j = P->row_ptr[i]; j < P->row_ptr[i + 1]; ++j) {
                ahat[P->col_idx[j]] = 0.0;
                inpat[P->col_idx[j]] = i;
            }
            for (int j = S->row_ptr[i]; j < S->row_ptr[i + 1]; ++j) ins[S->col_idx[j]] = i;
            for (int j = ia[i]; j < ia[i + 1]; ++j) {
                const int k = ja[j];
                if (k == i) continue;
                const double aik = a[j];
                if (inpat[k] == i) {
                    ahat[k] += aik;
                } else if (ins[k] == i && mark[k] == FGPT) {
                    const double akk = diag[k];
                    double den = 0.0;
                    for (int m = ia[k]; m < ia[k + 1]; ++m) {
                        const int l = ja[m];
                        if (l != k && (l == i || inpat[l] == i) && a[m] * akk < 0) den += a[m];
                    }
                    if (den != 0.0) {
                        const double f = aik / den;
                        for (int m = ia[k]; m < ia[k + 1]; ++m) {
                            const int l = ja[m];
                            if (l != k && (l == i || inpat[l] == i) && a[m] * akk < 0) {
                                const double t = f * a[m];
                                if (l == i) d += t;
                                else ahat[l] += t;
                            }
                        }
                    } else {
                        d += aik;
                    }
                } else {
                    d += aik;
                }
            }
            for (int j = P->row_ptr[i]; j < P->row_ptr[i + 1]; ++j) P->val[j] = -ahat[P->col_idx[j]] / d;
        }
    }
    scratch_free(scr, T);

    /* coarse renumbering of the columns, then the truncation */
    int *cmap = (int *)SSS_calloc((size_t)(n > 0 ? n : 1), sizeof(int));
    int ncoarse = 0;
    for (int i = 0; i < n; ++i)
        if (mark[i] == CGPT) cmap[i] = ncoarse++;
    P->num_cols = ncoarse;
#pragma omp parallel for schedule(static) if (P->num_nnzs > 65536)
    for (int q = 0; q < P->row_ptr[P->num_rows]; ++q) P->col_idx[q] = cmap[P->col_idx[q]];
    free(cmap);
    free(diag);
    SSS_amg_interp_trunc(P, pars);
    if (timing)
        fprintf(stderr, "[setup]   extended+i P: host weights %.4f s, %d rows, %d entries\n", SSS_get_time() - t0, P->num_rows,
                P->num_nnzs);
}

/*
 * Multipass interpolation (interp_type intERP_MPASS and the aggressive levels of cs_type
 * SSS_COARSE_PMIS_AGG; an engine extension after Stueben), on the final marks.
 *
 * Pass numbers: 0 for a C point; an F point gets 1 + the least number among the j != i of S_i that
 * have one.  Sweep p gives p to every F point without a number that has a neighbour numbered p - 1
 * (nobody numbered less is left among its neighbours, or it would have been numbered before), until a
 * sweep numbers nobody.  F points never numbered and ISPT points keep empty rows of P.
 *
 * Row i of pass p >= 1, N_i = { j in S_i : j != i, pass(j) = p - 1 }: one walk of the stored entries
 * (i, k) of A; d = the last stored diagonal entry, tot = the sum of the entries with k != i, sub = the
 * sum of those with k in N_i, and for k in N_i the entries (k, c) of P in stored order: c joins the
 * pattern at its first occurrence, hat w_c (from 0.0) receives a_ik p_kc.  Then
 *   p_ic = -((tot / sub) hat w_c) / d,
 * and all 0.0 when sub or d is 0.  No sign splitting; a row of A with zero sum gives a row of P with
 * sum 1.  C rows hold one stored 1.0.  The rows of a pass are independent given the passes before it
 * (per-thread scratch stamped with the row); they land in a staging pool, one block per pass, and are
 * assembled into P in row order after the last pass.  Then the coarse renumbering and the truncation,
 * as interp_STD.  Returns 0 or an error code with P untouched; *passes = the largest pass number.
 */
static int mpass_build(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, SSS_AMG_PARS *pars, int *passes,
                       int *unreached)
{
    const int n = A->num_rows;
    const int *ia = A->row_ptr, *ja = A->col_idx, *sa = S->row_ptr, *sj = S->col_idx;
    const double *a = A->val;
    const size_t ns = (size_t)(n > 0 ? n : 1);
    int *pass = (int *)SSS_calloc(ns, sizeof(int)), *len = (int *)SSS_calloc(ns, sizeof(int));
    int *todo = (int *)SSS_calloc(ns, sizeof(int)), *rows = (int *)SSS_calloc(ns, sizeof(int));
    char *hit = (char *)SSS_calloc(ns, 1);
    size_t *off = (size_t *)SSS_calloc(ns, sizeof(size_t)), pool = 0;
    int *pc = NULL, ntodo = 0, left = 0, p = 0, rc = 0;
    double *pv = NULL;

    /* pass 0: the C rows */
    for (int i = 0; i < n; ++i) {
        pass[i] = -1;
        if (mark[i] == CGPT) pass[i] = 0, len[i] = 1, off[i] = pool++;
        else if (mark[i] == FGPT) todo[ntodo++] = i;
        else left++;
    }
    pc = (int *)SSS_calloc(pool > 0 ? pool : 1, sizeof(int));
    pv = (double *)SSS_calloc(pool > 0 ? pool : 1, sizeof(double));
    for (int i = 0; i < n; ++i)
        if (mark[i] == CGPT) pc[off[i]] = i, pv[off[i]] = 1.0;

    /* per thread: seen, pos and ins (ints), n each, in one buffer */
    void *scr[kScratchMax];
    const int T = scratch_alloc(ns * 3 * sizeof(int), scr);
    for (int t = 0; t < T; ++t) {
        int *s = (int *)scr[t];
        for (size_t c = 0; c < 3 * ns; ++c) s[c] = INT_MIN;
    }
    while (ntodo > 0) {
        /* the rows of pass p + 1: in increasing i */
        int nrows = 0, keep = 0;
#pragma omp parallel for schedule(static) if (ntodo > 4096)
        for (int t = 0; t < ntodo; ++t) {
            const int i = todo[t];
            char h = 0;
            for (int q = sa[i]; q < sa[i + 1] && !h; ++q) h = sj[q] != i && pass[sj[q]] == p;
            hit[t] = h;
        }
        for (int t = 0; t < ntodo; ++t) {
            if (hit[t]) rows[nrows++] = todo[t];
            else todo[keep++] = todo[t];
        }
        ntodo = keep;
        if (nrows == 0) break;
        p++;
        /* count (the stamp is the row), offsets in the pool, fill (the stamp is ~row) */
#pragma omp parallel num_threads(T) if (nrows > 1024)
        {
            int *seen = (int *)scr[omp_get_thread_num()], *ins = seen + 2 * ns;
#pragma omp for schedule(dynamic, 256)
            for (int t = 0; t < nrows; ++t) {
                const int i = rows[t];
                int cnt = 0;
                for (int q = sa[i]; q < sa[i + 1]; ++q) ins[sj[q]] = i;
                for (int j = ia[i]; j < ia[i + 1]; ++j) {
                    const int k = ja[j];
                    if (k == i || ins[k] != i || pass[k] != p - 1) continue;
                    for (size_t q = off[k]; q < off[k] + (size_t)len[k]; ++q)
                        if (seen[pc[q]] != i) seen[pc[q]] = i, cnt++;
                }
                len[i] = cnt;
            }
        }
        const size_t old = pool;
        for (int t = 0; t < nrows; ++t) off[rows[t]] = pool, pool += (size_t)len[rows[t]];
        if (pool > (size_t)INT_MAX) {
            rc = ERROR_MAT_SIZE;
            break;
        }
        if (pool > old) {
            pc = (int *)SSS_realloc(pc, pool * sizeof(int));
            pv = (double *)SSS_realloc(pv, pool * sizeof(double));
        }
#pragma omp parallel num_threads(T) if (nrows > 1024)
        {
            int *seen = (int *)scr[omp_get_thread_num()], *pos = seen + ns, *ins = seen + 2 * ns;
#pragma omp for schedule(dynamic, 256)
            for (int t = 0; t < nrows; ++t) {
                const int i = rows[t];
                int *ci = pc + off[i], m = 0;
                double *w = pv + off[i], d = 0.0, tot = 0.0, sub = 0.0;
                for (int q = sa[i]; q < sa[i + 1]; ++q) ins[sj[q]] = i;
                for (int j = ia[i]; j < ia[i + 1]; ++j) {
                    const int k = ja[j];
                    if (k == i) {
                        d = a[j];
                        continue;
                    }
                    tot += a[j];
                    if (ins[k] != i || pass[k] != p - 1) continue;
                    sub += a[j];
                    for (size_t q = off[k]; q < off[k] + (size_t)len[k]; ++q) {
                        const int c = pc[q];
                        if (seen[c] != ~i) seen[c] = ~i, pos[c] = m, ci[m] = c, w[m++] = 0.0;
                        w[pos[c]] += a[j] * pv[q];
                    }
                }
                if (sub == 0.0 || d == 0.0) {
                    for (int q = 0; q < m; ++q) w[q] = 0.0;
                } else {
                    const double f = tot / sub;
                    for (int q = 0; q < m; ++q) w[q] = -(f * w[q]) / d;
                }
            }
        }
        /* the rows of this pass carry their number only now: nobody of the pass read it */
        for (int t = 0; t < nrows; ++t) pass[rows[t]] = p;
    }
    scratch_free(scr, T);

    if (rc == 0) {
        SSS_MAT Q;
        memset(&Q, 0, sizeof(Q));
        Q.num_rows = n;
        Q.row_ptr = (int *)SSS_calloc((size_t)n + 1, sizeof(int));
        for (int i = 0; i < n; ++i) Q.row_ptr[i + 1] = Q.row_ptr[i] + len[i];
        Q.num_nnzs = Q.row_ptr[n];
        Q.col_idx = (int *)SSS_calloc((size_t)(Q.num_nnzs > 0 ? Q.num_nnzs : 1), sizeof(int));
        Q.val = (double *)SSS_calloc((size_t)(Q.num_nnzs > 0 ? Q.num_nnzs : 1), sizeof(double));
        /* coarse numbers of the columns while the rows are copied */
        int *cmap = todo, ncoarse = 0;
        for (int i = 0; i < n; ++i)
            if (mark[i] == CGPT) cmap[i] = ncoarse++;
        Q.num_cols = ncoarse;
#pragma omp parallel for schedule(static) if (n > 65536)
        for (int i = 0; i < n; ++i)
            for (int q = 0; q < len[i]; ++q) {
                Q.col_idx[Q.row_ptr[i] + q] = cmap[pc[off[i] + (size_t)q]];
                Q.val[Q.row_ptr[i] + q] = pv[off[i] + (size_t)q];
            }
        SSS_amg_interp_trunc(&Q, pars);
        *P = Q;
        if (passes) *passes = p;
        if (unreached) *unreached = ntodo + left;
    }
    free(pc);
    free(pv);
    free(off);
    free(hit);
    free(rows);
    free(todo);
    free(len);
    free(pass);
    return rc;
}

static int mpass_check(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, const SSS_MAT *P)
{
    if (!A || !P || !A->row_ptr) return ERROR_INPUT_PAR;
    int rc = agg_check(S, mark);
    if (rc) return rc;
    const int n = S->num_rows;
    if (A->num_rows != n || A->row_ptr[0] != 0) return ERROR_INPUT_PAR;
    const int annz = A->row_ptr[n];
    if (annz <= 0 || !A->col_idx || !A->val) return ERROR_INPUT_PAR;
    for (int i = 0; i < n; ++i)
        if (A->row_ptr[i + 1] < A->row_ptr[i]) return ERROR_DATA_STRUCTURE;
    for (int q = 0; q < annz; ++q)
        if ((unsigned)A->col_idx[q] >= (unsigned)n) return ERROR_DATA_STRUCTURE;
    /* a strong column k != i of a row is in the row of A */
    for (int i = 0; i < n; ++i)
        for (int q = S->row_ptr[i]; q < S->row_ptr[i + 1]; ++q) {
            int found = S->col_idx[q] == i;
            for (int j = A->row_ptr[i]; j < A->row_ptr[i + 1] && !found; ++j) found = A->col_idx[j] == S->col_idx[q];
            if (!found) return ERROR_DATA_STRUCTURE;
        }
    return 0;
}

/* The host multipass interpolation on a given A, compacted S and final marks (tests; what the device
 * form is checked against).  P is written on success only (whatever it held is not freed); its
 * arrays are the library's. */
int sss_interp_mpass_host(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold,
                          int *passes)
{
    const int rc = mpass_check(A, S, mark, P);
    if (rc) return rc;
    SSS_AMG_PARS pars;
    memset(&pars, 0, sizeof(pars));
    pars.trunc_threshold = trunc_threshold;
    return mpass_build(A, S, mark, P, &pars, passes, NULL);
}

static void interp_MPASS(SSS_MAT *A, SSS_IVEC *vertices, SSS_MAT *P, SSS_IMAT *S, SSS_AMG_PARS *pars)
{
    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const double t0 = SSS_get_time();
    int passes = 0, unreached = 0;
    /* the device P (renumbered, truncated) is the host's bit for bit; on any error code P is untouched
     * and the host computes it */
    if (interp_on_device(A->num_nnzs) && sss_hip_interp_mpass(A, S, vertices->d, P, pars->trunc_threshold, &passes) == 0)
        return;
    const int rc = mpass_build(A, S, vertices->d, P, pars, &passes, &unreached);
    if (rc) SSS_exit_on_errcode(rc, __func__);
    if (timing)
        fprintf(stderr, "[setup]   multipass P: host %.4f s, %d passes, %d rows unreached, %d rows, %d entries\n",
                SSS_get_time() - t0, passes, unreached, P->num_rows, P->num_nnzs);
}

void SSS_amg_interp(SSS_MAT *A, SSS_IVEC *vertices, SSS_MAT *P, SSS_IMAT *S, SSS_AMG_PARS *pars)
{
    /* a level whose P came from SSS_amg_coarsen without a pattern is a multipass level: interp_type
     * intERP_MPASS, or an aggressive level of cs_type SSS_COARSE_PMIS_AGG whatever interp_type says */
    if (pars->interp_type == intERP_MPASS || P->row_ptr == NULL) interp_MPASS(A, vertices, P, S, pars);
    else if (pars->interp_type == intERP_DIR) interp_DIR(A, vertices, P, pars);
    else if (pars->interp_type == intERP_STD) interp_STD(A, vertices, P, S, pars);
    else if (pars->interp_type == intERP_EXTI) interp_EXTI(A, vertices, P, S, pars);
    else SSS_exit_on_errcode(ERROR_AMG_interp_type, __func__);
}

/* ======================================================================================
 * Galerkin product A_c = R A P (SSS_matvec.c:398-534), row-parallel.
 * ====================================================================================== */
SSS_MAT SSS_blas_mat_rap(const SSS_MAT *R, const SSS_MAT *A, const SSS_MAT *P)
{
    const int nc = R->num_rows, nf = A->num_rows;
    const int *ri = R->row_ptr, *rj = R->col_idx, *ai = A->row_ptr, *aj = A->col_idx;
    const int *pi = P->row_ptr, *pj = P->col_idx;
    const double *rv = R->val, *av = A->val, *pv = P->val;
    int64_t *start = (int64_t *)sss_big_calloc((size_t)nc + 1, sizeof(int64_t));
    SSS_MAT C;
    int too_big = 0;

    C.num_rows = nc;
    C.num_cols = nc;
    C.row_ptr = (int *)SSS_calloc((size_t)nc + 1, sizeof(int));
    C.col_idx = NULL;
    C.val = NULL;
    C.num_nnzs = 0;

    /* One parallel region for both passes: each thread's marker arrays are initialised once.
     * Markers hold the coarse row being built: ic in the counting pass, nc + ic in the filling
     * pass, so the second pass needs no reset. */
#pragma omp parallel
    {
        int *seen_f = (int *)sss_big_malloc(sizeof(int) * (size_t)(nf > 0 ? nf : 1));
        int *seen_c = (int *)sss_big_malloc(sizeof(int) * (size_t)(nc > 0 ? nc : 1));
        int *slot = (int *)sss_big_malloc(sizeof(int) * (size_t)(nc > 0 ? nc : 1));
        for (int i = 0; i < nf; ++i) seen_f[i] = -1;
        for (int i = 0; i < nc; ++i) seen_c[i] = -1;
#pragma omp for schedule(dynamic, 256)
        for (int ic = 0; ic < nc; ++ic) {
            int64_t cnt = 1;
            seen_c[ic] = ic;
            for (int q1 = ri[ic]; q1 < ri[ic + 1]; ++q1) {
                int i1 = rj[q1];
                for (int q2 = ai[i1]; q2 < ai[i1 + 1]; ++q2) {
                    int i2 = aj[q2];
                    if (seen_f[i2] == ic) continue;
                    seen_f[i2] = ic;
                    for (int q3 = pi[i2]; q3 < pi[i2 + 1]; ++q3)
                        if (seen_c[pj[q3]] != ic) { seen_c[pj[q3]] = ic; cnt++; }
                }
            }
            start[ic + 1] = cnt;
        }
#pragma omp single
        {
            for (int ic = 0; ic < nc; ++ic) start[ic + 1] += start[ic];
            if (start[nc] > INT32_MAX) {
                too_big = 1;
            } else {
                C.num_nnzs = (int)start[nc];
                for (int ic = 0; ic <= nc; ++ic) C.row_ptr[ic] = (int)start[ic];
                C.col_idx = (int *)SSS_calloc((size_t)C.num_nnzs, sizeof(int));
                C.val = (double *)SSS_calloc((size_t)C.num_nnzs, sizeof(double));
            }
        }   /* implicit barrier */
        if (!too_big) {
#pragma omp for schedule(dynamic, 256)
            for (int ic = 0; ic < nc; ++ic) {
                const int mk = nc + ic;
                int pos = C.row_ptr[ic];
                seen_c[ic] = mk;
                slot[ic] = pos;
                C.col_idx[pos] = ic;
                C.val[pos] = 0.0;
                pos++;
                for (int q1 = ri[ic]; q1 < ri[ic + 1]; ++q1) {
                    const double r = rv[q1];
                    const int i1 = rj[q1];
                    for (int q2 = ai[i1]; q2 < ai[i1 + 1]; ++q2) {
                        const double ra = r * av[q2];
                        const int i2 = aj[q2];
                        if (seen_f[i2] != mk) {
                            seen_f[i2] = mk;
                            for (int q3 = pi[i2]; q3 < pi[i2 + 1]; ++q3) {
                                const double rap = ra * pv[q3];
                                const int i3 = pj[q3];
                                if (seen_c[i3] != mk) {
                                    seen_c[i3] = mk;
                                    slot[i3] = pos;
                                    C.val[pos] = rap;
                                    C.col_idx[pos] = i3;
                                    pos++;
                                } else {
                                    C.val[slot[i3]] += rap;
                                }
                            }
                        } else {
                            for (int q3 = pi[i2]; q3 < pi[i2 + 1]; ++q3) C.val[slot[pj[q3]]] += ra * pv[q3];
                        }
                    }
                }
            }
        }
        free(seen_f);
        free(seen_c);
        free(slot);
    }
    if (too_big) {
        printf("### ERROR: RAP product has %lld nonzeros (int32 index limit)\n", (long long)start[nc]);
        SSS_exit_on_errcode(ERROR_MAT_SIZE, __func__);
    }
    free(start);
    return C;
}

/* The values of C = R A P on the pattern C already has (the pattern SSS_blas_mat_rap gives for
 * operators with these patterns): the rule above in one row-parallel pass.  The row's columns go
 * into the thread's marker arrays with their positions, the diagonal starts at 0.0, every other
 * slot at -0.0, and every product adds -- x + -0.0 is x for every x, -0.0 included, so a slot's
 * first product lands as the reference's assignment does.  0, or ERROR_INPUT_PAR (shapes) /
 * ERROR_DATA_STRUCTURE (an index out of range, a row of C that does not start with its diagonal or
 * repeats a column, a product whose column the row does not hold) with C->val untouched. */
int sss_rap_values_host(const SSS_MAT *R, const SSS_MAT *A, const SSS_MAT *P, SSS_MAT *C)
{
    if (!R || !A || !P || !C || !C->row_ptr || !C->col_idx || !C->val) return ERROR_INPUT_PAR;
    const int nc = R->num_rows, nf = A->num_rows, np = P->num_rows;
    if (nc <= 0 || C->num_rows != nc || C->num_cols != nc || P->num_cols != nc || R->num_cols != nf ||
        A->num_cols != np || C->num_nnzs < nc || C->row_ptr[0] != 0 || C->row_ptr[nc] != C->num_nnzs)
        return ERROR_INPUT_PAR;
    const int *ri = R->row_ptr, *rj = R->col_idx, *ai = A->row_ptr, *aj = A->col_idx;
    const int *pi = P->row_ptr, *pj = P->col_idx, *ci = C->row_ptr, *cj = C->col_idx;
    const double *rv = R->val, *av = A->val, *pv = P->val;
    const int nnz = C->num_nnzs;
    double *val = (double *)sss_big_malloc(sizeof(double) * (size_t)nnz);
    int bad = 0;
    if (!val) return ERROR_ALLOC_MEM;
#pragma omp parallel
    {
        int *seen = (int *)sss_big_malloc(sizeof(int) * (size_t)nc);
        int *slot = (int *)sss_big_malloc(sizeof(int) * (size_t)nc);
        for (int i = 0; i < nc; ++i) seen[i] = -1;
#pragma omp for schedule(dynamic, 256)
        for (int ic = 0; ic < nc; ++ic) {
            const int c0 = ci[ic], len = ci[ic + 1] - c0;
            int ok = len >= 1 && c0 >= 0 && ci[ic + 1] <= nnz && cj[c0] == ic;
            for (int k = 0; ok && k < len; ++k) {
                const int c = cj[c0 + k];
                if (c < 0 || c >= nc || seen[c] == ic) {
                    ok = 0;
                    break;
                }
                seen[c] = ic;
                slot[c] = c0 + k;
                val[c0 + k] = k == 0 ? 0.0 : -0.0;
            }
            for (int q1 = ri[ic]; ok && q1 < ri[ic + 1]; ++q1) {
                const double r = rv[q1];
                const int i1 = rj[q1];
                if (i1 < 0 || i1 >= nf) {
                    ok = 0;
                    break;
                }
                for (int q2 = ai[i1]; ok && q2 < ai[i1 + 1]; ++q2) {
                    const double ra = r * av[q2];
                    const int i2 = aj[q2];
                    if (i2 < 0 || i2 >= np) {
                        ok = 0;
                        break;
                    }
                    for (int q3 = pi[i2]; q3 < pi[i2 + 1]; ++q3) {
                        const int i3 = pj[q3];
                        if (i3 < 0 || i3 >= nc || seen[i3] != ic) {
                            ok = 0;
                            break;
                        }
                        val[slot[i3]] += ra * pv[q3];
                    }
                }
            }
            if (!ok) {
#pragma omp atomic write
                bad = 1;
            }
        }
        free(seen);
        free(slot);
    }
    if (!bad) {
#pragma omp parallel for schedule(static)
        for (int k = 0; k < nnz; ++k) C->val[k] = val[k];
    }
    free(val);
    return bad ? ERROR_DATA_STRUCTURE : 0;
}

/* The setup's rule for a level's Galerkin product on the GPU: a device is present and
 * SSS_SETUP_GPU_RAP is not 0; A_l has at least SSS_SETUP_GPU_RAP_MIN nonzeros (default 10^6) and
 * at most SSS_SETUP_GPU_RAP_MAXROW of them per row on average (default 48). */
static int gpu_rap_enabled(void)
{
    const char *gr = getenv("SSS_SETUP_GPU_RAP");
    return !(gr && gr[0] == '0') && sss_hip_device_count() > 0;
}
static int gpu_rap_level(const SSS_MAT *A)
{
    const char *grm = getenv("SSS_SETUP_GPU_RAP_MIN"), *grx = getenv("SSS_SETUP_GPU_RAP_MAXROW");
    const int gpu_rap_min = (grm && *grm) ? atoi(grm) : 1000000;
    const int gpu_rap_maxrow = (grx && *grx) ? atoi(grx) : 48;
    return A->num_nnzs >= gpu_rap_min && (double)A->num_nnzs <= (double)gpu_rap_maxrow * A->num_rows;
}

/* ======================================================================================
 * Level loop (Setup/SSS_SETUP.cu:5-178)
 * ====================================================================================== */
void SSS_amg_complexity_print(SSS_AMG *mg)
{
    static const char *rule = "-----------------------------------------------------------\n";
    double grid = 0.0, op = 0.0;
    fputs(rule, stdout);
    printf("  Level   Num of rows   Num of nonzeros   Avg. NNZ / row   \n");
    fputs(rule, stdout);
    for (int l = 0; l < mg->num_levels; ++l) {
        const SSS_MAT *A = &mg->cg[l].A;
        printf("%5d %13d %17d %14.2lf\n", l, A->num_rows, A->num_nnzs, (double)A->num_nnzs / A->num_rows);
        grid += A->num_rows;
        op += A->num_nnzs;
    }
    fputs(rule, stdout);
    grid /= mg->cg[0].A.num_rows;
    op /= mg->cg[0].A.num_nnzs;
    printf("  Grid complexity = %.3lf  |", grid);
    printf("  Operator complexity = %.3lf\n", op);
    fputs(rule, stdout);
}

void SSS_amg_setup(SSS_AMG *mg, SSS_MAT *A, SSS_AMG_PARS *pars) { sss_amg_setup_hooked(mg, A, pars, NULL, NULL); }

/* SSS_amg_setup with a progress hook: hook(ctx, mg, done, 0) each time level done - 1 has been
 * completed (its P, R, C/F marks and the next operator are final and it is not the coarsest
 * level), hook(ctx, mg, num_levels - 1, 1) at the end.  sss_hip_setup_create uploads the
 * completed levels to the GPU while the later ones are still being coarsened. */
void sss_amg_setup_hooked(SSS_AMG *mg, SSS_MAT *A, SSS_AMG_PARS *pars, sss_setup_hook hook, void *ctx)
{
    const int min_cdof = SSS_max(pars->coarse_dof, MIN_CDOF);
    const int max_lvls = pars->max_levels;
    const int n0 = A->num_rows;
    const double t0 = SSS_get_time();
    SSS_IVEC vertices;
    int lvl = 0;
    const int use_gpu_rap = gpu_rap_enabled();

    *mg = SSS_amg_data_create(pars);
    vertices = SSS_ivec_create(n0);
    mg->cg[0].A = SSS_mat_struct_create(n0, n0, A->num_nnzs);
    SSS_mat_cp(A, &mg->cg[0].A);

    while (mg->cg[lvl].A.num_rows > min_cdof && lvl < max_lvls - 1) {
        SSS_AMG_COMP *L = &mg->cg[lvl];
        SSS_IMAT S;
        int status;
        memset(&S, 0, sizeof(S));

        const double tc0 = SSS_get_time();
        sss_trace_push("SSS_amg_setup level %d", lvl);
        sss_trace_push("coarsen");
        status = amg_coarsen_level(&L->A, &vertices, &L->P, &S, pars, lvl);
        sss_trace_pop();
        const double tc1 = SSS_get_time();
        if (status < 0) {
            free(S.row_ptr);
            free(S.col_idx);
            printf("### WARNING: Could not find any C-variables!\n");
            printf("### WARNING: RS coarsening on level-%d failed!\n", lvl);
            sss_trace_pop();
            break;
        }
        if (L->P.num_cols < min_cdof) {
            free(S.row_ptr);
            free(S.col_idx);
            sss_trace_pop();
            break;
        }
        if (L->P.num_rows > L->P.num_cols * 10) {
            printf("### WARNING: Coarsening might be too aggressive!\n");
            printf("### WARNING: Lvl = %d ,Fine level = %d, coarse level = %d. Discard!\n", lvl,
                   L->P.num_rows, L->P.num_cols);
        }
        if (L->P.num_cols * 1.5 > L->A.num_rows) pars->cs_type = SSS_COARSE_RS;

        L->cfmark = SSS_ivec_create(L->A.num_rows);
        memcpy(L->cfmark.d, vertices.d, (size_t)L->A.num_rows * sizeof(int));

        sss_trace_push("interpolation");
        SSS_amg_interp(&L->A, &vertices, &L->P, &S, pars);
        sss_trace_pop();
        const double tc2 = SSS_get_time();
        sss_trace_push("R = P^T");
        L->R = SSS_mat_trans(&L->P);
        sss_trace_pop();
        const double tc3 = SSS_get_time();
        sss_trace_push("RAP");
        /* the device walks each coarse row's (R entry, A entry) steps in order, so it wins on the
         * wide levels of short rows (7-pt 400^3 levels 0-2: 3.1 -> 1.1, 2.0 -> 0.75, 0.59 -> 0.37 s)
         * and loses on the narrow levels of long rows (level 3 and below: 0.75 -> 1.2 s) */
        const int gpu_here = use_gpu_rap && gpu_rap_level(&L->A);
        if (!(gpu_here && sss_hip_rap(&L->R, &L->A, &L->P, &mg->cg[lvl + 1].A) == 0))
            mg->cg[lvl + 1].A = SSS_blas_mat_rap(&L->R, &L->A, &L->P);
        sss_trace_pop();
        sss_trace_pop();   /* the level */
        if (getenv("SSS_SETUP_TIMING"))   /* phase times on stderr (stdout stays the reference's) */
            fprintf(stderr, "[setup] level %d: coarsen %.3f s, interp %.3f s, transpose %.3f s, RAP %.3f s\n", lvl,
                    tc1 - tc0, tc2 - tc1, tc3 - tc2, SSS_get_time() - tc3);
        free(S.row_ptr);
        free(S.col_idx);

        /* "too dense" test on the finer level (integer nnz/rows, SSS_SETUP.cu:142) */
        if (L->A.num_nnzs / L->A.num_rows > L->A.num_cols * 0.2) {
            printf("### WARNING: Coarse matrix is too dense!\n");
            printf("### WARNING: m = n = %d, nnz = %d!\n", L->A.num_cols, L->A.num_nnzs);
            SSS_mat_destroy(&mg->cg[lvl + 1].A);
            break;
        }
        lvl++;
        if (hook) hook(ctx, mg, lvl, 0);
    }

    mg->num_levels = lvl + 1;
    mg->cg[0].wp = SSS_vec_create(n0);
    for (int l = 1; l < mg->num_levels; ++l) {
        int m = mg->cg[l].A.num_rows;
        mg->cg[l].b = SSS_vec_create(m);
        mg->cg[l].x = SSS_vec_create(m);
        mg->cg[l].wp = SSS_vec_create(2 * m);
    }
    SSS_ivec_destroy(&vertices);
    SSS_amg_complexity_print(mg);
    printf("AMG setup time: %g s\n", SSS_get_time() - t0);
    if (hook) hook(ctx, mg, mg->num_levels - 1, 1);
}

/* ======================================================================================
 * Refresh of a set-up hierarchy for new operator values on the same pattern: C/F marks, P and R
 * stay, the Galerkin chain is recomputed as values-only products.
 * ====================================================================================== */
int SSS_amg_refresh(SSS_AMG *mg, const SSS_MAT *A)
{
    if (!mg || !A || !mg->cg || mg->num_levels < 1) return ERROR_INPUT_PAR;
    SSS_MAT *A0 = &mg->cg[0].A;
    if (A->num_rows != A0->num_rows || A->num_cols != A0->num_cols || A->num_nnzs != A0->num_nnzs || !A->row_ptr ||
        !A->col_idx || !A->val ||
        memcmp(A->row_ptr, A0->row_ptr, sizeof(int) * ((size_t)A0->num_rows + 1)) != 0 ||
        memcmp(A->col_idx, A0->col_idx, sizeof(int) * (size_t)A0->num_nnzs) != 0)
        return ERROR_INPUT_PAR;
    const int timing = getenv("SSS_SETUP_TIMING") != NULL;
    const int use_gpu_rap = gpu_rap_enabled();
    if (A->val != A0->val) memcpy(A0->val, A->val, sizeof(double) * (size_t)A0->num_nnzs);
    for (int l = 0; l + 1 < mg->num_levels; ++l) {
        SSS_AMG_COMP *L = &mg->cg[l];
        SSS_MAT *C = &mg->cg[l + 1].A;
        const double t0 = SSS_get_time();
        int on_device = use_gpu_rap && gpu_rap_level(&L->A) && sss_hip_rap_values(&L->R, &L->A, &L->P, C) == 0;
        if (!on_device) {
            const int rc = sss_rap_values_host(&L->R, &L->A, &L->P, C);
            if (rc) return rc;
        }
        if (timing) {
            double t[2] = {0.0, 0.0};
            if (on_device) sss_hip_rap_times(t);
            if (on_device)
                fprintf(stderr, "[refresh] level %d: device %.3f s (copies %.3f s, kernels %.3f s)\n", l,
                        SSS_get_time() - t0, t[0], t[1]);
            else
                fprintf(stderr, "[refresh] level %d: host %.3f s\n", l, SSS_get_time() - t0);
        }
    }
    /* the drop-in path's mirror follows; one that cannot is dropped, and the next solve builds it again */
    sss_hip_hier *h = sss_dev_mirror_peek(mg->cg);
    if (h && sss_hip_hier_refresh(h, mg) != 0) sss_dev_release_mirror(mg->cg);
    return 0;
}
