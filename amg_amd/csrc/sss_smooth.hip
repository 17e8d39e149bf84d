// sss_smooth.hip — smoothers of the V-cycle (gfx950, fp64, no contraction).
//
// Exact GS-CF (replaces SSS_amg_smoother_gs_cf, Solve/SSS_smooth.c:4-87; dispatched from
// SSS_amg_smoother_pre/post :138-304).  Per sweep the reference runs an F pass (mark != 1,
// ascending rows) then a C pass (mark == 1, ascending rows), updating x in place:
//     t = b_i - sum_{k: j_k != i} a_k * x_{j_k}   (in stored order), x_i = t / d
// where d is the last diagonal entry seen so far in the call (it is stale for a row without a
// diagonal entry).  Inside one pass, row i needs the NEW x_j of same-class rows j < i it is
// coupled to and the OLD x_j of same-class rows j > i.  Level scheduling reproduces exactly
// that: depth(i) = 1 + max depth of coupled same-class rows j < i (read-after-write), and
// every coupled same-class row j > i is pushed below i (write-after-read, for nonsymmetric
// patterns).  Rows of equal depth are independent; each depth is one launch.  The result is
// bitwise identical to the sequential reference (same per-row operation order).
//
// On level 0 of the 7-point Poisson operator the RS split is red-black, so each pass has depth
// 1 — a single fully parallel, HBM-bound launch.  Coarser levels have
// depth in the hundreds; there the passes are launch-latency-bound.
//
// C/F-Jacobi (engine extension; SSS_SM_JACOBI): F pass then C pass, every row of a pass
// reading the values from before the pass (ping-pong buffers), d = the row's last diagonal.
#include "sss_smooth_plan.hpp"
#include "sss_spmv_dev.hpp"

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <cmath>

namespace sss {

// ---- plan upload: each step builds on the host (sss_smooth_plan.hip), uploads, sets the plan's
// fields and lets its host arrays go ------------------------------------------------------------
static const char *const kPlanArray = "hipMalloc(plan array)";   // the error line of a failed plan upload

static int alloc_vec(double *&p, size_t count, const char *what, int line = __builtin_LINE())
{
    p = dev_alloc<double>(count);
    return p ? 0 : hip_fail(hipErrorOutOfMemory, what, __FILE__, line);
}

// exact GS depth launches hold few rows each: a wave per row pays from short lengths on
static bool long_rows_of(long long nnz, int rows) { return rows > 0 && nnz >= (long long)std::min(32, wave_row_min()) * rows; }

static int upload_buckets(PassSchedule &ps, DepthBuckets &bk)
{
    ps.depth = bk.depth, ps.nrows = bk.nrows, ps.max_width = bk.max_width;
    ps.h_off = std::move(bk.h_off);
    return dev_upload(ps.rows, bk.rows, kPlanArray);
}

// contiguous class?  (relabeled level: F rows first, then C rows): the pass runs on the level matrix's
// own row blocks; C/F-Jacobi gets the iterate buffers of the class
static int setup_range(PassSchedule &ps, const ClassRange &r, int kind, int inner)
{
    if (!r.contiguous) return 0;
    ps.range = r.blocks, ps.blo = r.blo, ps.bhi = r.bhi, ps.lo = r.lo, ps.hi = r.hi;
    if (!ps.range || kind != SSS_HIP_SMOOTH_JACOBI) return 0;
    int rc = alloc_vec(ps.y, (size_t)(r.hi - r.lo), "hipMalloc(y)");
    if (!rc && inner > 0) rc = alloc_vec(ps.y2, (size_t)(r.hi - r.lo), "hipMalloc(y2)");
    return rc;
}

static int upload_compact(PassSchedule &ps, const SSS_MAT &A, const int *cls, int c, int kind)
{
    CompactRows cr;
    build_compact_rows(A, cls, c, cr);
    const SSS_MAT sub = cr.mat(A.num_cols);
    int rc;
    if ((rc = devcsr_upload(ps.sub, sub)) || (rc = dev_upload(ps.map, cr.map, kPlanArray))) return rc;
    return kind == SSS_HIP_SMOOTH_JACOBI ? alloc_vec(ps.y, cr.map.size(), "hipMalloc(y)") : 0;
}

// exact GS passes with intra-class chains: one launch per pass where the class is contiguous; then
// every pass of a call in one launch (both passes on the flow engine; 2 sweeps, SSS_amg_pars_init's
// pre/post count)
static int build_one_launch(SmootherPlan &sp, const SSS_MAT &A, const int *mark, const DevCSR *dA, const int *cls,
                            const SmootherSwitches &sw)
{
    int rc;
    for (int c = 0; c < 2; ++c) {
        PassSchedule &ps = sp.pass[c];
        if (ps.compact || ps.depth <= 1 || ps.nrows == 0) continue;
        const ClassRange r = class_range(cls, A.num_rows, c);
        if (r.contiguous && (rc = gs_persist_build(ps, A, r.lo, r.hi, sp.long_rows))) return rc;
    }
    if (sw.gs_fused && mark && sp.pass[0].gp.engine == 1 && sp.pass[1].gp.engine == 1)
        return gs_fused_build(sp.fz, A, dA, sp.pass, cls, 2);
    return 0;
}

static int upload_two_stage(PassSchedule &ps, const SSS_MAT &A, int c, const int *gcls, int enc, PhaseTimer &pt)
{
    const int m = ps.hi - ps.lo;
    TwoStageSplit ts;
    two_stage_count(A, ps.lo, m, c, gcls, ts);
    pt.mark("ts count");
    two_stage_fill(A, ps.lo, m, c, gcls, ts);
    pt.mark("ts fill");
    const SSS_MAT Mn = ts.Mn(A.num_cols), Ml = ts.Ml(A.num_cols);
    // read by the ts_* kernels only: merged groups, or the column ELL
    const int tenc = (enc & ~kEncDict) | kEncMergedOnly;
    int rc;
    if ((rc = devcsr_upload(ps.ts_nl, Mn, -1, tenc, ts.split.data())) || (rc = devcsr_upload(ps.ts_lo, Ml, -1, tenc)))
        return rc;
    pt.mark("ts upload");
    if ((rc = dev_upload(ps.ts_split, ts.split, kPlanArray))) return rc;
    return alloc_vec(ps.ts_P, (size_t)m, "hipMalloc(P)");
}

int smoother_build(SmootherPlan &sp, const SSS_MAT &A, const int *mark, int kind, const DevCSR *dA, int inner,
                   const int *gcls, int enc)
{
    const int n = A.num_rows;
    const bool jacobi = kind == SSS_HIP_SMOOTH_JACOBI;
    const SmootherSwitches sw = smoother_switches();
    PhaseTimer pt("plan");
    double lap[5] = {PhaseTimer::now()};
    int rc;
    sp.kind = kind;
    RowClasses rw;
    plan_row_classes(A, mark, rw);
    StaleDivisors stale;
    plan_stale_divisors(rw, n, stale);
    sp.long_rows = long_rows_of(A.row_ptr[n], n);
    const bool coupled = plan_coupled(A, rw);
    pt.mark("classes+coupled");
    // red-black levels (no coupling) keep depth 0 everywhere; so do C/F-Jacobi levels, whose
    // passes read only the other iterate (their schedule is never walked by depth)
    if (coupled && !jacobi) schedule_classes(A, rw);
    pt.mark("depth");
    for (int c = 0; c < 2; ++c) {
        PassSchedule &ps = sp.pass[c];
        DepthBuckets bk;
        bucket_rows(0, n, rw.cls.data(), c, rw.depth.data(), bk);
        if ((rc = upload_buckets(ps, bk))) return rc;
        ps.compact = jacobi || ps.depth <= 1;
        if (ps.compact && ps.nrows > 0 && dA && rw.single_diag &&
            (rc = setup_range(ps, class_range(rw.cls.data(), n, c, dA), kind, inner)))
            return rc;
        if (ps.compact && ps.nrows > 0 && !ps.range && (rc = upload_compact(ps, A, rw.cls.data(), c, kind))) return rc;
    }
    if ((rc = dev_upload(sp.cls, rw.cls, kPlanArray))) return rc;
    lap[1] = PhaseTimer::now();
    if (kind == SSS_HIP_SMOOTH_EXACT && !gcls && A.num_cols == n && (rc = build_one_launch(sp, A, mark, dA, rw.cls.data(), sw)))
        return rc;
    lap[2] = PhaseTimer::now();
    if (jacobi && inner > 0 && sp.pass[0].range == (sp.pass[0].nrows > 0) && sp.pass[1].range == (sp.pass[1].nrows > 0)) {
        sp.inner = inner;
        for (int c = 0; c < 2; ++c)
            if (sp.pass[c].nrows > 0 && (rc = upload_two_stage(sp.pass[c], A, c, gcls, enc, pt))) return rc;
    }
    lap[3] = PhaseTimer::now();
    if (sp.pass[0].range || sp.pass[1].range)
        if ((rc = dev_upload(sp.diag_pos, rw.diag_pos, kPlanArray))) return rc;
    if (const int cs = plan_nocopy_split(sp, A, gcls, sw); cs >= 0) {
        sp.csplit = cs;
        if ((rc = alloc_vec(sp.x2, (size_t)n, "hipMalloc(x2)"))) return rc;
    }
    const double *d_first = rw.all_diag ? rw.last_diag.data() : stale.first.data();
    const double *d_later = rw.all_diag ? rw.last_diag.data() : stale.later.data();
    sp.own_diag = plan_own_diag(rw, sw);
    sp.finite = plan_finite(A, sw);
    sp.f_overwritten = plan_f_overwritten(sp, rw, d_first, d_later, sw);
    plan_fused_flags(sp, A, dA, rw, sw);
    lap[4] = PhaseTimer::now();
    if (getenv("SSS_HIP_TIMING"))
        fprintf(stderr, "[sss_hip]   smoother plan n=%d: schedule %.2f s, one-launch GS %.2f s, two-stage %.2f s, rest %.2f s\n",
                n, lap[1] - lap[0], lap[2] - lap[1], lap[3] - lap[2], lap[4] - lap[3]);
    if (jacobi || rw.all_diag) {   // Jacobi: row's own diagonal
        if ((rc = dev_upload(sp.d_first, rw.last_diag, kPlanArray))) return rc;
        sp.d_later = sp.d_first;
    } else {
        if ((rc = dev_upload(sp.d_first, stale.first, kPlanArray))) return rc;
        if ((rc = dev_upload(sp.d_later, stale.later, kPlanArray))) return rc;
    }
    return 0;
}

int smoother_build_natural(SmootherPlan &sp, const SSS_MAT &A, int lo, int hi)
{
    int rc;
    sp.kind = SSS_HIP_SMOOTH_EXACT;
    sp.natural = true;
    sp.long_rows = long_rows_of(A.row_ptr[hi] - A.row_ptr[lo], hi - lo);
    NaturalDivisors nd;
    plan_natural_divisors(A, lo, hi, nd);
    // level schedules: ascending (row i reads the new x_j of coupled j < i, the old x_j of j > i,
    // which must wait for it) and descending (mirrored)
    for (int dir = 0; dir < 2; ++dir) {
        PassSchedule &ps = sp.pass[dir];
        std::vector<int> depth;
        schedule_natural(A, lo, hi, dir == 1, depth);
        DepthBuckets bk;
        bucket_rows(lo, hi, nullptr, 0, depth.data(), bk);
        if ((rc = upload_buckets(ps, bk))) return rc;
        if (ps.depth > 1 && (rc = gs_persist_build(ps, A, lo, hi, sp.long_rows, true, dir == 1))) return rc;
    }
    if ((rc = dev_upload(sp.d_first, nd.first[0], kPlanArray)) || (rc = dev_upload(sp.d_later, nd.later[0], kPlanArray)) ||
        (rc = dev_upload(sp.nd_first, nd.first[1], kPlanArray)) || (rc = dev_upload(sp.nd_later, nd.later[1], kPlanArray)))
        return rc;
    return 0;
}

void smoother_free(SmootherPlan &sp)
{
    for (auto &ps : sp.pass) {
        dev_free(ps.rows);
        devcsr_free(ps.sub);
        dev_free(ps.map);
        dev_free(ps.y);
        dev_free(ps.y2);
        devcsr_free(ps.ts_nl);
        devcsr_free(ps.ts_lo);
        dev_free(ps.ts_split);
        dev_free(ps.ts_P);
        gs_persist_free(ps);
    }
    gs_fused_free(sp.fz);
    if (sp.d_later != sp.d_first) dev_free(sp.d_later);
    dev_free(sp.d_first);
    dev_free(sp.nd_first);
    dev_free(sp.nd_later);
    dev_free(sp.cls);
    dev_free(sp.diag_pos);
    dev_free(sp.x2);
    sp = SmootherPlan();
}

// ---- kernels -------------------------------------------------------------------------------
// exact GS, one thread per row of the current depth.  NAT: natural-order GS (Solve/SSS_smooth.c:
// 90-137), x_i = t * d with d the carried reciprocal of the diagonal, written unconditionally.
template <bool NAT>
__global__ __launch_bounds__(kBlock) void gs_depth_thread(const int *__restrict__ rows, int cnt,
                                                          const int *__restrict__ rp, const int *__restrict__ ci,
                                                          const double *__restrict__ v, const double *__restrict__ b,
                                                          double *x, const double *__restrict__ deff)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= cnt) return;
    const int i = rows[t];
    double acc = b[i];
    for (int k = rp[i]; k < rp[i + 1]; ++k) {
        const int j = ci[k];
        if (j != i) acc -= v[k] * x[j];
    }
    const double d = deff[i];
    if (NAT) x[i] = acc * d;
    else if (div_ok(d)) x[i] = acc / d;
}

// exact GS on long rows: four rows of the current depth per workgroup, one per wave; lanes
// gather the products, lane 0 subtracts them in CSR order (sss_spmv_dev.hpp wave_row_chain).
template <bool NAT>
__global__ __launch_bounds__(kBlock) void gs_depth_wave(const int *__restrict__ rows, int cnt,
                                                        const int *__restrict__ rp, const int *__restrict__ ci,
                                                        const double *__restrict__ v, const double *__restrict__ b,
                                                        double *x, const double *__restrict__ deff)
{
    __shared__ __attribute__((aligned(16))) double strips[4][kWaveStage];
    const int wave = threadIdx.x >> 6;
    const int t = blockIdx.x * 4 + wave;
    if (t >= cnt) return;
    const int i = rows[t];
    const double acc = wave_row_chain<true>(
        rp[i], rp[i + 1], ci, v, [&](int c, double a) { return c == i ? 0.0 : a * x[c]; }, b[i], strips[wave]);
    if ((threadIdx.x & 63) == 0) {
        const double d = deff[i];
        if (NAT) x[i] = acc * d;
        else if (div_ok(d)) x[i] = acc / d;
    }
}

// Independent-row pass over the class-compacted CSR: GS with depth 1 (in place) or the
// relaxation half of a C/F-Jacobi pass (into y, scattered afterwards).
template <bool INPLACE>
__global__ __launch_bounds__(kBlock) void relax_compact(const int *__restrict__ blk, const int *__restrict__ rp,
                                                        const int *__restrict__ ci, const double *__restrict__ v,
                                                        const int *__restrict__ map, const double *__restrict__ b,
                                                        double *x, double *__restrict__ y,
                                                        const double *__restrict__ deff)
{
    __shared__ SpmvSmem sm;
    csr_block_relax(blk, rp, ci, v, map, b, x, sm, [&](int r, int i, double acc) {
        const double d = deff[i];
        if (INPLACE) {
            if (div_ok(d)) x[i] = acc / d;
        } else {
            y[r] = div_ok(d) ? acc / d : x[i];
        }
    });
}

template <bool INPLACE>
__global__ __launch_bounds__(kBlock) void relax_wave(int m, const int *__restrict__ rp, const int *__restrict__ ci,
                                                     const double *__restrict__ v, const int *__restrict__ map,
                                                     const double *__restrict__ b, double *x, double *__restrict__ y,
                                                     const double *__restrict__ deff)
{
    __shared__ __attribute__((aligned(16))) double strips[4][kWaveStage];
    const int wave = threadIdx.x >> 6;
    const int r = xcd_bid() * 4 + wave;
    if (r >= m) return;
    const int i = map[r];
    const double acc = wave_row_chain<true>(
        rp[r], rp[r + 1], ci, v, [&](int c, double a) { return (c < 0 || c == i) ? 0.0 : a * x[c]; }, b[i],
        strips[wave]);
    if ((threadIdx.x & 63) == 0) {
        const double d = deff[i];
        if (INPLACE) {
            if (div_ok(d)) x[i] = acc / d;
        } else {
            y[r] = div_ok(d) ? acc / d : x[i];
        }
    }
}

// Class pass over rows [lo, hi) of a relabeled level, blocks [blo, ...) of its own CSR.
//   MODE 0: GS-CF pass of depth 1, in place (x[r] = t / d).
//   MODE 1: C/F-Jacobi pass / two-stage stage 0: y[r - lo] = t / d, every x from before the pass.
//   MODE 3: the residual of the row with x unchanged (rr, partial, as the residual SpMV) and the
//           GS value the pass's MODE 0 would write, into y[r - lo] (SmootherPlan::pend_ok).
//   MODE 2: MODE 0, then the residual of the updated row (ResidFuse, sss_engine.hpp):
//           rr[r] = b_r - (sum of a_k x_k in stored order from 0.0), the diagonal product formed
//           with the new x_r -- exactly the residual SpMV's chain, since in a depth-1 pass no
//           other product of the row changes; per-block sums of squares into partial[bid].
// t = b_r - sum over off-diagonal entries in stored order (diag_pos skips the diagonal); rows with
// |d| <= 1e-20 keep their value.
// Dictionary ELL rows (DICT == 2): the same per-row arithmetic, the row's products in registers in
// stored (slot) order instead of staged in LDS.
// The row formula of all four modes over a row's products in stored order, whatever holds them:
// pr.sub(s, a, e) / pr.add(s, a, e) = s -/+ the products of slots [a, e) (EllProds: registers;
// XellProds: column-ELL codes and LDS values; TileProds: the LDS tile).  The row's slots are [a, e),
// its diagonal at slot ds when diag; br = b_r, div() the divisor (asked for after the chain: the tile
// path reads it only then), keep() the value a row with a failing divisor keeps (read only then).  xn: the relaxed value; res: the row's residual (MODE 2: with the
// new x_r in the diagonal product, MODE 3: with x unchanged); upd: the divisor passed div_ok.
struct RelaxRow {
    double xn, res;
    bool upd;
};
// br - the row's off-diagonal products in stored order (Solve/SSS_smooth.c:21-26)
template <class Prods>
__device__ __forceinline__ double relax_acc(const Prods &pr, int a, bool diag, int ds, int e, double br)
{
    if (!diag) return pr.sub(br, a, e);
    return pr.sub(pr.sub(br, a, ds), ds + 1, e);
}
template <int MODE, class Prods, class Div, class Keep>
__device__ __forceinline__ RelaxRow relax_row(const Prods &pr, int a, bool diag, int ds, int e, double br, Div div,
                                              Keep keep)
{
    const double acc = relax_acc(pr, a, diag, ds, e, br);
    const double d = div();
    RelaxRow o;
    o.upd = div_ok(d);
    o.xn = o.upd ? acc / d : keep();
    o.res = 0.0;
    if constexpr (MODE == 2) {   // plans guarantee one diagonal per row here
        double t = pr.add(0.0, a, ds);
        t += d * o.xn;
        t = pr.add(t, ds + 1, e);
        o.res = br + t * -1.0;
    } else if constexpr (MODE == 3) {
        o.res = br + pr.add(0.0, a, e) * -1.0;
    }
    return o;
}
template <int W>
struct EllProds {
    const double (&p)[W];
    __device__ __forceinline__ double sub(double s, int a, int e) const { return ell_sub(s, p, a, e); }
    __device__ __forceinline__ double add(double s, int a, int e) const { return ell_add(s, p, a, e); }
};
template <int W>
struct XellProds {
    const unsigned (&w)[W];
    const double (&xv)[W];
    const XellSmem &es;
    int shift;
    __device__ __forceinline__ double sub(double s, int a, int e) const { return xell_sum_g<true>(s, w, xv, es, shift, a, e); }
    __device__ __forceinline__ double add(double s, int a, int e) const { return xell_sum_g<false>(s, w, xv, es, shift, a, e); }
};
struct TileProds {
    const double *v;
    __device__ __forceinline__ double sub(double s, int a, int e) const { return chain_sub(s, v, a, e); }
    __device__ __forceinline__ double add(double s, int a, int e) const { return chain_add(s, v, a, e); }
};

template <int MODE, int W>
__device__ __forceinline__ void relax_range_ell(int blo, const int2 *__restrict__ blk, int lo,
                                                const double *__restrict__ b, double *x, double *__restrict__ y,
                                                const double *__restrict__ deff, double *__restrict__ rr,
                                                double *__restrict__ partial, XSrc xs, const DevDict &dt)
{
    constexpr int RPT = kEllRpt;
    __shared__ EllSmem es[RPT];
    const int g = (int)blockIdx.x;
    EllRow<W> row[RPT];
    double br[RPT], dr[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {   // every row's codes, b and divisor in flight across the barrier
        br[j] = dr[j] = 0.0;
        row[j] = ell_row_begin<W>(blk, blo + g * RPT + j, dt, es[j], [&](int r) {
            br[j] = b[r];
            if (deff) dr[j] = deff[r];
        });
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
        double sq = 0.0;
        if (row[j].live) {
            const int rj = row[j].r;
            double p[W];
            int dsl;
            double dv;
            // the pass's own x_r only in MODE 3 (the residual of the row with x unchanged)
            const int len = ell_decode<W, MODE == 3>(row[j].w, rj, es[j], [&](int c) -> double { return xs(c); }, p, dsl, dv);
            const RelaxRow o = relax_row<MODE>(EllProds<W>{p}, 0, dsl >= 0, dsl, len, br[j], [&] { return deff ? dr[j] : dv; }, [&]() -> double {
                return MODE == 0 ? 0.0 : MODE == 1 ? xs(rj) : x[rj];   // (MODE 0 stores only an updated row)
            });
            if constexpr (MODE == 0 || MODE == 2) {
                if (o.upd) x[rj] = o.xn;
            } else {
                y[rj - lo] = o.xn;
            }
            if constexpr (MODE >= 2) {
                rr[rj] = o.res;
                sq = o.res * o.res;
            }
        }
        if constexpr (MODE >= 2) {
            if (partial && row[j].valid) {   // (valid is uniform over the workgroup)
                const double t = block_sum(sq, es[j].red);
                if (threadIdx.x == 0) partial[blo + g * RPT + j] = t;
            }
        }
    }
}

// relax_range_ell for W = 8 with two consecutive rows per thread (sss_spmv_dev.hpp ell_pair_rows):
// every row's arithmetic exactly as relax_range_ell's, x / y / rr / b moved as 16-byte pairs.
template <int MODE>
__device__ __forceinline__ void relax_range_ell2(int blo, const int2 *__restrict__ blk, int lo,
                                                 const double *__restrict__ b, double *x, double *__restrict__ y,
                                                 const double *__restrict__ deff, double *__restrict__ rr,
                                                 double *__restrict__ partial, XSrc xs, const DevDict &dt)
{
    __shared__ EllSmem es[2];
    const int g = (int)blockIdx.x;
    const EllPairRows pr = ell_pair_rows(blk, blo + 2 * g, dt.bend);
    unsigned w[2][2];
    double br[2], dr[2] = {0.0, 0.0};
    ell_pair_codes(dt.ell, pr, w);   // every row's codes, b and divisor in flight across the barrier
    pair_load(b, pr.r, pr.l0, pr.l1, br);
    if (deff) pair_load(deff, pr.r, pr.l0, pr.l1, dr);
    if (pr.v0) ell_load_dicts_nosync(dt, pr.b0, es[0]);
    if (pr.v1) ell_load_dicts_nosync(dt, pr.b0 + 1, es[1]);
    __syncthreads();
    double xo[2] = {0.0, 0.0}, ro[2] = {0.0, 0.0}, sq[2] = {0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int rj = pr.r + i;
        if (!(i == 0 ? pr.l0 : pr.l1)) continue;
        const int j = rj < pr.mid ? 0 : 1;
        double p[8];
        int dsl;
        double dv;
        const int len = ell_decode<8, MODE == 3>(w[i], rj, es[j], [&](int c) -> double { return xs(c); }, p, dsl, dv);
        // (the pair is stored whole: a row with a failing divisor stores the value it keeps)
        const RelaxRow o = relax_row<MODE>(EllProds<8>{p}, 0, dsl >= 0, dsl, len, br[i], [&] { return deff ? dr[i] : dv; },
                                           [&]() -> double { return MODE == 1 ? xs(rj) : x[rj]; });
        xo[i] = o.xn;
        if constexpr (MODE >= 2) {
            ro[i] = o.res;
            sq[j] += ro[i] * ro[i];
        }
    }
    if constexpr (MODE == 0 || MODE == 2) pair_store(x, pr.r, pr.l0, pr.l1, xo);
    if constexpr (MODE == 1 || MODE == 3) pair_store(y, pr.r - lo, pr.l0, pr.l1, xo);
    if constexpr (MODE >= 2) pair_store(rr, pr.r, pr.l0, pr.l1, ro);
    if constexpr (MODE >= 2) {
        // per-block sums of squares in the residual SpMV's order (one row per thread, block_sum's
        // fixed tree): each row's square goes through LDS to the thread that row has there, so the
        // norm is bitwise the unfused residual's (tests/test_gpu_parity.py test_fused_residual_bitwise)
        __shared__ double sqrow[2 * kBlock];
        if (partial && pr.v0) {   // (uniform over the workgroup)
            const int ra = pr.r - 2 * (int)threadIdx.x;
            if (pr.l0) sqrow[pr.r - ra] = ro[0] * ro[0];
            if (pr.l1) sqrow[pr.r + 1 - ra] = ro[1] * ro[1];
            __syncthreads();
            const int n0 = pr.mid - ra, n1 = pr.v1 ? ell_block_rows(pr) - n0 : 0;
            const double t0 = block_sum((int)threadIdx.x < n0 ? sqrow[threadIdx.x] : 0.0, es[0].red);
            if (threadIdx.x == 0) partial[pr.b0] = t0;
            if (pr.v1) {
                const double t1 = block_sum((int)threadIdx.x < n1 ? sqrow[n0 + threadIdx.x] : 0.0, es[1].red);
                if (threadIdx.x == 0) partial[pr.b0 + 1] = t1;
            }
        }
        (void)sq;
    }
}

// Column ELL rows (DICT = kXell + W): relax_range_ell's per-row arithmetic, one row block per
// workgroup, the row's products in registers from its explicit-column codes.
template <int MODE, int W>
__device__ __forceinline__ void relax_range_xell(int blo, const int2 *__restrict__ blk, int lo,
                                                 const double *__restrict__ b, double *x, double *__restrict__ y,
                                                 const double *__restrict__ deff, double *__restrict__ rr,
                                                 double *__restrict__ partial, XSrc xs, const DevDict &dt)
{
    __shared__ XellSmem es;
    const int bid = blo + (int)blockIdx.x;
    const bool valid = bid < dt.bend;
    double br = 0.0, dr = 0.0;
    const XellRow<W> row = xell_row_begin<W>(valid, blk, bid, dt.xell, dt.pd, dt.vd, es, [&](int r) {
        br = b[r];
        if (deff) dr = deff[r];
    });
    const unsigned(&w)[W] = row.w;
    const int r = row.r;
    __syncthreads();
    double sq = 0.0;
    if (row.live) {
        double xv[W];
        int dsl;
        unsigned dcode;
        const int len = xell_gather<W, MODE == 3>(w, r, dt.xshift, [&](int c) -> double { return xs(c); }, xv, dsl, dcode);
        const double dv = dsl < 0 ? 0.0 : es.vd[dcode >> dt.xshift];
        const RelaxRow o = relax_row<MODE>(XellProds<W>{w, xv, es, dt.xshift}, 0, dsl >= 0, dsl, len, br, [&] { return deff ? dr : dv; },
                                           [&]() -> double { return MODE == 0 ? 0.0 : MODE == 1 ? xs(r) : x[r]; });
        if constexpr (MODE == 0 || MODE == 2) {
            if (o.upd) x[r] = o.xn;
        } else {
            y[r - lo] = o.xn;
        }
        if constexpr (MODE >= 2) {
            rr[r] = o.res;
            sq = o.res * o.res;
        }
    }
    if constexpr (MODE >= 2) {
        if (partial && valid) {   // (valid is uniform over the workgroup)
            const double t = block_sum(sq, es.red);
            if (threadIdx.x == 0) partial[bid] = t;
        }
    }
}

template <int MODE, int DICT = 0>   // DICT: with_tile_kind (8/16/32: dictionary ELL, kXell + W: column ELL)
__device__ __forceinline__ void relax_range_body(int blo, const int2 *__restrict__ blk, const int *__restrict__ rp,
                                                      const int *__restrict__ ci, const double *__restrict__ v,
                                                      const int *__restrict__ diag_pos, int lo,
                                                      const double *__restrict__ b, double *x,
                                                      const double *__restrict__ yp, double *__restrict__ y,
                                                      const double *__restrict__ deff, const unsigned *__restrict__ pk,
                                                      const double *__restrict__ pv, const int2 *__restrict__ pb,
                                                      double *__restrict__ rr, double *__restrict__ partial, XSrc xs,
                                                      DevDict dt = DevDict())
{
    if constexpr (DICT >= kXell) {
        relax_range_xell<MODE, DICT - kXell>(blo, blk, lo, b, x, y, deff, rr, partial, xs, dt);
    } else if constexpr (DICT == 8 && kEllPairs) {
        relax_range_ell2<MODE>(blo, blk, lo, b, x, y, deff, rr, partial, xs, dt);
    } else if constexpr (DICT >= 8) {
        relax_range_ell<MODE, DICT>(blo, blk, lo, b, x, y, deff, rr, partial, xs, dt);
    } else {
    __shared__ SpmvSmem sm;
    __shared__ std::conditional_t<DICT != 0, DictSmem, char> dsm;
    DictSmem *ds = nullptr;
    if constexpr (DICT != 0) ds = &dsm;
    const int bid = blo + xcd_bid();
    const int2 ba = blk[bid], be = blk[bid + 1];
    const int r0 = ba.x, r1 = be.x, k0 = ba.y, k1 = be.y;
    auto fetch = [&](int c) -> double { return xs(c); };
    // deff null: the plan's divisor is each row's own diagonal, staged from the sorted tile
    auto dval = [&](int r) -> double { return deff ? deff[r] : sm.d[r - r0]; };
    auto finish = [&](int r, double acc) {
        const double d = dval(r);
        if (MODE != 1) {
            if (div_ok(d)) x[r] = acc / d;
        } else {
            y[r - lo] = div_ok(d) ? acc / d : xs(r);
        }
    };
    if (k1 - k0 <= kTileEntries) {
        const int r = r0 + (int)threadIdx.x;
        int a = 0, e = 0, dp = -1;
        double br = 0.0;
        if (r < r1) a = rp[r] - k0, e = rp[r + 1] - k0, dp = diag_pos[r], br = b[r];   // ahead of the tile
        stage_any(sm.v, k0, k1, ci, v, pk, pv, pb, bid, r0, deff ? (double *)nullptr : sm.d, fetch, dt, ds, r1, rp);
        __syncthreads();
        double sq = 0.0;
        if (r < r1) {
            if constexpr (MODE >= 2) {
                const RelaxRow o = relax_row<MODE>(TileProds{sm.v}, a, dp >= 0, dp - k0, e, br, [&] { return dval(r); },
                                                   [&]() -> double { return x[r]; });
                if constexpr (MODE == 2) {
                    if (o.upd) x[r] = o.xn;
                } else {
                    y[r - lo] = o.xn;
                }
                rr[r] = o.res;
                sq = o.res * o.res;
            } else {
                // (not relax_row: with it the dictionary-tile relax_range_occ<0, 1> compiled to 34
                // scalar-register spills instead of 22)
                finish(r, relax_acc(TileProds{sm.v}, a, dp >= 0, dp - k0, e, br));
            }
        }
        if constexpr (MODE >= 2) {
            if (partial) {
                const double t = block_sum(sq, sm.red);
                if (threadIdx.x == 0) partial[bid] = t;
            }
        }
    } else if constexpr (MODE < 2) {   // MODE 2 / 3 plans have no long-row block
        const int r = r0, dp = diag_pos[r];
        const double acc = long_row_chunks(
            k0, k1, b[r],
            [&](int base, int m) {
                stage_any(sm.v, base, base + m, ci, v, pk, pv, pb, bid, r0, deff ? (double *)nullptr : sm.d, fetch, dt,
                          ds, r1, rp);
            },
            [&](int base, int m, double acc) {
                if (dt.tree_long) {   // free order: acc -= tree sum of the chunk's off-diagonal products
                    if (threadIdx.x == 0 && dp >= base && dp < base + m) sm.v[dp - base] = 0.0;
                    __syncthreads();
                    const double c = block_tree_sum(sm.v, 0, m, sm.red);
                    if (threadIdx.x == 0) acc -= c;
                } else if (threadIdx.x == 0) {
                    if (dp >= base && dp < base + m) {
                        acc = chain_sub(acc, sm.v, 0, dp - base);
                        acc = chain_sub(acc, sm.v, dp - base + 1, m);
                    } else {
                        acc = chain_sub(acc, sm.v, 0, m);
                    }
                }
                return acc;
            });
        if (threadIdx.x == 0) finish(r, acc);
    }
    }
}

#define SSS_RELAX_ARGS                                                                                          \
    int blo, const int2 *__restrict__ blk, const int *__restrict__ rp, const int *__restrict__ ci,                 \
        const double *__restrict__ v, const int *__restrict__ diag_pos, int lo, const double *__restrict__ b,      \
        double *x, const double *__restrict__ yp, double *__restrict__ y, const double *__restrict__ deff,          \
        const unsigned *__restrict__ pk, const double *__restrict__ pv, const int2 *__restrict__ pb,               \
        double *__restrict__ rr, double *__restrict__ partial, XSrc xs, DevDict dt
#define SSS_RELAX_PASS blo, blk, rp, ci, v, diag_pos, lo, b, x, yp, y, deff, pk, pv, pb, rr, partial, xs, dt
template <int MODE, int DICT = 0>
__global__ __launch_bounds__(kBlock) void relax_range(SSS_RELAX_ARGS)
{
    relax_range_body<MODE, DICT>(SSS_RELAX_PASS);
}
// The tile paths (plain / sorted / dictionary tiles, K < 8) held to 5 waves per SIMD: the value-
// dictionary tiles of level 1 otherwise take 107 VGPRs (4 waves per SIMD, 14 resident per CU in
// profiles/r03_kernels_sq_pmc_400.txt) and wait on memory 70 % of their cycles.  Measured at
// 400^3 (tools/gpu/ab.sh): level-1 smoothing 4.61 -> 4.23 ms per V-cycle at 5 waves (96 VGPRs);
// 6 waves (the LDS limit) spill to scratch and take 6.90 ms.
template <int MODE, int DICT = 0>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(5, 8))) void relax_range_occ(SSS_RELAX_ARGS)
{
    relax_range_body<MODE, DICT>(SSS_RELAX_PASS);
}
// relax_range / relax_range_occ over the row blocks [blo, blo + nb): one workgroup per block, or
// per kEllRpt blocks on dictionary ELL (K >= 8)
template <int M, int K, class... Args>
static void launch_relax_range(int blo, int nb, hipStream_t s, DevDict dt, Args... args)
{
    if constexpr (K < 8) {
        hipLaunchKernelGGL((relax_range_occ<M, K>), dim3(nb), dim3(kBlock), 0, s, blo, args..., dt);
    } else {
        dt.bend = blo + nb;
        hipLaunchKernelGGL((relax_range<M, K>), dim3((nb + rows_per_wg(K) - 1) / rows_per_wg(K)), dim3(kBlock), 0, s, blo,
                           args..., dt);
    }
}

// relax_range for long-row levels: one wave per row (rows lo + 4 * blockIdx.x + wave).  The
// diagonal (single per row on range levels) contributes an exact 0.0 to the chain.
// TREE: free sum order (DevCSR::vec_rows), t = b_r - (tree sum of the off-diagonal products).
template <int MODE, bool TREE>
__global__ __launch_bounds__(kBlock) void relax_range_wave(int lo, int hi, const int *__restrict__ rp,
                                                           const int *__restrict__ ci, const double *__restrict__ v,
                                                           const double *__restrict__ b, double *x,
                                                           const double *__restrict__ yp, double *__restrict__ y,
                                                           const double *__restrict__ deff, XSrc xs)
{
    __shared__ __attribute__((aligned(16))) double strips[TREE ? 1 : 4][TREE ? 1 : kWaveStage];
    const int wave = threadIdx.x >> 6;
    const int r = lo + xcd_bid() * 4 + wave;
    if (r >= hi) return;
    auto prod = [&](int c, double a) -> double { return c == r ? 0.0 : a * (MODE == 1 ? xs(c) : x[c]); };
    const double acc = TREE ? b[r] - wave_row_sum(rp[r], rp[r + 1], ci, v, prod)
                            : wave_row_chain<true>(rp[r], rp[r + 1], ci, v, prod, b[r], strips[TREE ? 0 : wave]);
    if ((threadIdx.x & 63) == 0) {
        const double d = deff[r];
        if (MODE == 0) {
            if (div_ok(d)) x[r] = acc / d;
        } else {
            y[r - lo] = div_ok(d) ? acc / d : xs(r);
        }
    }
}

// ---- two-stage GS-CF (oracle: ora_cf_twostage) ----------------------------------------------
// Stage 0 over the reordered pass rows [N_i | L_i] (local row q = global lo + q):
//   P_q = b - sum_{N_i} a x;  y_q = (P_q - sum_{L_i} a x) / d   (x from before the pass)
// (LDSACC: merged groups with the lanes' accumulators in LDS, DevCSR::mg_acc)
// (K16: narrow keys, DevCSR::mg_k16)
template <int PATH, bool LDSACC = false, bool K16 = false>   // 0 tile, 1 wave chain, 2 wave tree (free order)
__global__ __launch_bounds__(kBlock) void ts_stage0(int lo, DevCSR M, const int *__restrict__ split,
                                                    const double *__restrict__ b, XSrc x,
                                                    const double *__restrict__ deff, double *__restrict__ P,
                                                    double *__restrict__ y)
{
    auto finish = [&](int q, double acc) {
        const int r = lo + q;
        const double d = deff[r];
        y[q] = div_ok(d) ? acc / d : x(r);
    };
    if constexpr (PATH >= kXell) {   // column ELL rows of width PATH - kXell: one thread per row
        constexpr int W = PATH - kXell;
        __shared__ XellSmem es;
        const int bq = blockIdx.x;
        double bq_v = 0.0, dq = 0.0;
        int sp = 0;
        // (the row's b, divisor and its [N | L] cut with the codes)
        const XellRow<W> row = xell_row_begin<W>(true, M.bk, bq, M.dv_xell, M.dv_pd, M.dv_vd, es, [&](int q) {
            bq_v = b[lo + q];
            dq = deff[lo + q];
            sp = split[q] - M.rp[q];
        });
        const unsigned(&w)[W] = row.w;
        const int q = row.r;
        const bool live = row.live;
        __syncthreads();
        if (live) {
            double xv[W];
            int ds;
            unsigned dcode;
            const int len = xell_gather<W>(w, -1, M.xell_shift, [&](int c) -> double { return x(c); }, xv, ds, dcode);
            const double Pq = xell_sum_bf<true>(bq_v, w, xv, es, M.xell_shift, 0, sp);
            P[q] = Pq;
            const double acc = xell_sum_bf<true>(Pq, w, xv, es, M.xell_shift, sp, len);
            y[q] = div_ok(dq) ? acc / dq : x(lo + q);   // finish() with the divisor loaded early
        }
        return;
    } else if constexpr (PATH >= 3) {   // merged row groups, G = PATH, M.mg_W waves per group
        constexpr int G = PATH;
        __shared__ double red[8 * G];
        __shared__ double acc[LDSACC ? 4 * 2 * G * kMergeAccDoubles : 1];
        int g = 0, u = 0;
        double n_sum = 0.0, l_sum = 0.0;
        constexpr bool K = K16 && 2 * G <= 8;   // (three accumulator bits; G = 8 is never uploaded narrow)
        if (merged_block<G, 2, LDSACC, K>(M.mg_gp, M.mg_ng, M.mg_W, merged_keys_of(M), M.mg_v,
                                          [&](int c) -> double { return x(c); }, red, acc, g, u, n_sum, l_sum)) {
            const int q = g * G + u;
            if (q < M.n) {
                const double Pq = b[lo + q] - n_sum;
                P[q] = Pq;
                finish(q, Pq - l_sum);
            }
        }
        return;
    } else if constexpr (PATH == 2) {
        const int q = xcd_bid() * 4 + (threadIdx.x >> 6);
        if (q >= M.n) return;
        auto prod = [&](int c, double a) { return a * x(c); };
        const int a = M.rp[q], sp = split[q], e = M.rp[q + 1];
        const double Pq = b[lo + q] - wave_row_sum(a, sp, M.ci, M.v, prod);
        const double acc = Pq - wave_row_sum(sp, e, M.ci, M.v, prod);
        if ((threadIdx.x & 63) == 0) {
            P[q] = Pq;
            finish(q, acc);
        }
        return;
    } else if constexpr (PATH == 1) {
        __shared__ __attribute__((aligned(16))) double strips[4][kWaveStage];
        const int wave = threadIdx.x >> 6, q = xcd_bid() * 4 + wave;
        if (q >= M.n) return;
        auto prod = [&](int c, double a) { return a * x(c); };
        const int a = M.rp[q], sp = split[q], e = M.rp[q + 1];
        double acc = wave_row_chain<true>(a, sp, M.ci, M.v, prod, b[lo + q], strips[wave]);
        acc = __shfl(acc, 0, 64);
        if ((threadIdx.x & 63) == 0) P[q] = acc;
        acc = wave_row_chain<true>(sp, e, M.ci, M.v, prod, acc, strips[wave]);
        if ((threadIdx.x & 63) == 0) finish(q, acc);
        return;
    } else {
        __shared__ SpmvSmem sm;
        const int bq = xcd_bid();
        const BlockBounds bb = block_bounds(M.bk, M.rp, bq);
        const int q0 = bb.r0, q1 = bb.r1, k0 = bb.k0, k1 = bb.k1;
        if (k1 - k0 <= kTileEntries) {
            const int q = q0 + (int)threadIdx.x;
            int a = 0, sp = 0, e = 0;
            double acc = 0.0;
            if (q < q1) a = M.rp[q] - k0, sp = split[q] - k0, e = M.rp[q + 1] - k0, acc = b[lo + q];
            stage_any(sm.v, k0, k1, M.ci, M.v, M.pk, M.pv, M.pb, bq, q0, (double *)nullptr, [&](int c) -> double { return x(c); });
            __syncthreads();
            if (q < q1) {
                acc = chain_sub(acc, sm.v, a, sp);
                P[q] = acc;
                acc = chain_sub(acc, sm.v, sp, e);
                finish(q, acc);
            }
        } else {   // one long row, chunk by chunk, thread 0 carries the chain
            const int q = q0, sp = split[q];
            const double acc = long_row_chunks(
                k0, k1, b[lo + q],
                [&](int base, int m) {
                    stage_any(sm.v, base, base + m, M.ci, M.v, M.pk, M.pv, M.pb, bq, q0, (double *)nullptr, [&](int c) -> double { return x(c); });
                },
                [&](int base, int m, double acc) {
                    if (M.tree_long) {   // free order: the N part and the L part of the chunk tree-summed
                        const int cut = min(max(sp - base, 0), m);
                        const double c1 = block_tree_sum(sm.v, 0, cut, sm.red);
                        const double c2 = block_tree_sum(sm.v, cut, m, sm.red);
                        if (threadIdx.x == 0) {
                            acc -= c1;
                            if (sp >= base && sp < base + m) P[q] = acc;
                            acc -= c2;
                        }
                    } else if (threadIdx.x == 0) {
                        if (sp >= base && sp < base + m) {
                            acc = chain_sub(acc, sm.v, 0, sp - base);
                            P[q] = acc;
                            acc = chain_sub(acc, sm.v, sp - base, m);
                        } else {
                            acc = chain_sub(acc, sm.v, 0, m);
                        }
                    }
                    return acc;
                });
            if (threadIdx.x == 0) {
                if (sp == k1) P[q] = acc;   // no L entries
                finish(q, acc);
            }
        }
    }
}

// Inner step over the L-only rows:  y_q = (P_q - sum_{L_i} a yp[j - lo]) / d  (keeps yp_q if |d| small)
// (column c reads ycols[c - col_off]; a row with |d| small keeps ykeep[q]; rows are lo + q)
template <int PATH, bool LDSACC = false, bool K16 = false>   // 0 tile, 1 wave chain, 2 wave tree (free order)
__global__ __launch_bounds__(kBlock) void ts_inner(int lo, DevCSR M, const double *__restrict__ deff,
                                                   const double *__restrict__ P, const double *ycols, int col_off,
                                                   const double *ykeep, double *__restrict__ y)
{
    auto fetch = [&](int c) -> double { return ycols[c - col_off]; };
    auto finish = [&](int q, double acc) {
        const double d = deff[lo + q];
        y[q] = div_ok(d) ? acc / d : ykeep[q];
    };
    if constexpr (PATH >= kXell) {   // column ELL rows of width PATH - kXell: one thread per row
        constexpr int W = PATH - kXell;
        __shared__ XellSmem es;
        const int bq = blockIdx.x;
        double pq = 0.0, dq = 0.0;
        // (P_q and the divisor with the codes)
        const XellRow<W> row = xell_row_begin<W>(true, M.bk, bq, M.dv_xell, M.dv_pd, M.dv_vd, es, [&](int q) {
            pq = P[q];
            dq = deff[lo + q];
        });
        const unsigned(&w)[W] = row.w;
        const int q = row.r;
        const bool live = row.live;
        __syncthreads();
        if (live) {
            double xv[W];
            int ds;
            unsigned dcode;
            const int len = xell_gather<W>(w, -1, M.xell_shift, fetch, xv, ds, dcode);
            const double acc = xell_sum_g<true>(pq, w, xv, es, M.xell_shift, 0, len);
            y[q] = div_ok(dq) ? acc / dq : ykeep[q];   // finish() with the divisor loaded early
        }
        return;
    } else if constexpr (PATH >= 3) {   // merged row groups, G = PATH, M.mg_W waves per group
        constexpr int G = PATH;
        __shared__ double red[8 * G];
        __shared__ double acc[LDSACC ? 4 * G * kMergeAccDoubles : 1];
        int g = 0, u = 0;
        double l_sum = 0.0, unused = 0.0;
        if (merged_block<G, 1, LDSACC, K16>(M.mg_gp, M.mg_ng, M.mg_W, merged_keys_of(M), M.mg_v, fetch, red, acc, g, u,
                                            l_sum, unused)) {
            const int q = g * G + u;
            if (q < M.n) finish(q, P[q] - l_sum);
        }
        return;
    } else if constexpr (PATH == 2) {
        const int q = xcd_bid() * 4 + (threadIdx.x >> 6);
        if (q >= M.n) return;
        const double acc =
            P[q] - wave_row_sum(M.rp[q], M.rp[q + 1], M.ci, M.v, [&](int c, double a) { return a * fetch(c); });
        if ((threadIdx.x & 63) == 0) finish(q, acc);
        return;
    } else if constexpr (PATH == 1) {
        __shared__ __attribute__((aligned(16))) double strips[4][kWaveStage];
        const int wave = threadIdx.x >> 6, q = xcd_bid() * 4 + wave;
        if (q >= M.n) return;
        const double acc = wave_row_chain<true>(
            M.rp[q], M.rp[q + 1], M.ci, M.v, [&](int c, double a) { return a * fetch(c); }, P[q], strips[wave]);
        if ((threadIdx.x & 63) == 0) finish(q, acc);
        return;
    } else {
        __shared__ SpmvSmem sm;
        const int bq = xcd_bid();
        const BlockBounds bb = block_bounds(M.bk, M.rp, bq);
        const int q0 = bb.r0, q1 = bb.r1, k0 = bb.k0, k1 = bb.k1;
        if (k1 - k0 <= kTileEntries) {
            const int q = q0 + (int)threadIdx.x;
            int a = 0, e = 0;
            double acc = 0.0;
            if (q < q1) a = M.rp[q] - k0, e = M.rp[q + 1] - k0, acc = P[q];
            stage_any(sm.v, k0, k1, M.ci, M.v, M.pk, M.pv, M.pb, bq, q0, (double *)nullptr, fetch);
            __syncthreads();
            if (q < q1) finish(q, chain_sub(acc, sm.v, a, e));
        } else {
            const int q = q0;
            const double acc = long_row_chunks(
                k0, k1, P[q],
                [&](int base, int m) {
                    stage_any(sm.v, base, base + m, M.ci, M.v, M.pk, M.pv, M.pb, bq, q0, (double *)nullptr, fetch);
                },
                [&](int, int m, double acc) {
                    if (M.tree_long) {
                        const double c = block_tree_sum(sm.v, 0, m, sm.red);
                        if (threadIdx.x == 0) acc -= c;
                    } else if (threadIdx.x == 0) {
                        acc = chain_sub(acc, sm.v, 0, m);
                    }
                    return acc;
                });
            if (threadIdx.x == 0) finish(q, acc);
        }
    }
}

// ledger (sss_engine.hpp ByteLedger): a pass's matrix bytes -- the rows [lo, hi) of a contiguous class,
// else the pass's share of A -- + the x it gathers (8 B per row) + `vec` bytes of row vectors per row
static void ledger_pass(const DevCSR &A, const PassSchedule &ps, double vec)
{
    if (!ledger_on()) return;
    const double mat = ps.range ? matrix_bytes_rows(A, ps.lo, ps.hi)
                                : (A.n ? (double)A.stream_bytes * ps.nrows / A.n : 0.0);
    ledger_add(mat + (8.0 + vec) * ps.nrows);
}

void launch_ts_stage0(const DevCSR &M, int lo, const int *split, const double *b, XSrc x, const double *deff,
                      double *P, double *y, hipStream_t s)
{
    if (M.n == 0) return;
    ledger_add((double)M.stream_bytes + 40.0 * M.n);   // + x gathers, b, deff, P and y
    if (M.mg_two && with_merged_kind(M, [&](auto G, auto ACC, auto K16) {
            hipLaunchKernelGGL((ts_stage0<decltype(G)::value, decltype(ACC)::value, decltype(K16)::value>), dim3(M.ngrid),
                               dim3(kBlock), 0, s, lo, M, split, b, x, deff, P, y);
        }))
        return;
    if (M.vec_rows)
        hipLaunchKernelGGL(ts_stage0<2>, dim3((M.n + 3) / 4), dim3(kBlock), 0, s, lo, M, split, b, x, deff, P, y);
    else if (M.wave_rows)
        hipLaunchKernelGGL(ts_stage0<1>, dim3(M.ngrid), dim3(kBlock), 0, s, lo, M, split, b, x, deff, P, y);
    else if (M.dv_xell)
        with_tile_kind(M, [&](auto K) {
            constexpr int KK = decltype(K)::value;
            if constexpr (KK >= kXell)
                hipLaunchKernelGGL(ts_stage0<KK>, dim3(M.nblk), dim3(kBlock), 0, s, lo, M, split, b, x, deff, P, y);
        });
    else
        hipLaunchKernelGGL(ts_stage0<0>, dim3(M.nblk), dim3(kBlock), 0, s, lo, M, split, b, x, deff, P, y);
}

void launch_ts_inner(const DevCSR &M, int lo, const double *deff, const double *P, const double *ycols, int col_off,
                     const double *ykeep, double *y, hipStream_t s)
{
    if (M.n == 0) return;
    ledger_add((double)M.stream_bytes + 40.0 * M.n);   // + y gathers, deff, P, ykeep and y
    if (with_merged_kind(M, [&](auto G, auto ACC, auto K16) {
            hipLaunchKernelGGL((ts_inner<decltype(G)::value, decltype(ACC)::value, decltype(K16)::value>), dim3(M.ngrid),
                               dim3(kBlock), 0, s, lo, M, deff, P, ycols, col_off, ykeep, y);
        }))
        return;
    if (M.vec_rows)
        hipLaunchKernelGGL(ts_inner<2>, dim3((M.n + 3) / 4), dim3(kBlock), 0, s, lo, M, deff, P, ycols, col_off, ykeep, y);
    else if (M.wave_rows)
        hipLaunchKernelGGL(ts_inner<1>, dim3(M.ngrid), dim3(kBlock), 0, s, lo, M, deff, P, ycols, col_off, ykeep, y);
    else if (M.dv_xell)
        with_tile_kind(M, [&](auto K) {
            constexpr int KK = decltype(K)::value;
            if constexpr (KK >= kXell)
                hipLaunchKernelGGL(ts_inner<KK>, dim3(M.nblk), dim3(kBlock), 0, s, lo, M, deff, P, ycols, col_off, ykeep,
                                   y);
        });
    else
        hipLaunchKernelGGL(ts_inner<0>, dim3(M.nblk), dim3(kBlock), 0, s, lo, M, deff, P, ycols, col_off, ykeep, y);
}

// First pass of a smoother call on a zero iterate (C/F-Jacobi pass or two-stage stage 0 right after
// the cycle zeroed x): every product a_k * x_k is +-0.0, so t = b - (a_1 x_1) - (a_2 x_2) - ... is
// exactly b -- except b == -0.0 with a summed value whose sign bit is set (its product -0.0 turns
// -0.0 into +0.0), which is order-independent.  The pass then reads no matrix entries (the rare
// -0.0 rows scan their values).  Requires finite matrix values (SmootherPlan::finite).
__device__ __forceinline__ double zero_x_sum(double t, const int *__restrict__ ci, const double *__restrict__ v, int a,
                                             int e, int skip_col)
{
    if (t == 0.0 && signbit(t))
        for (int k = a; k < e; ++k)
            if (ci[k] != skip_col && signbit(v[k])) return 0.0;
    return t;
}

template <bool TWO>
__global__ __launch_bounds__(kBlock) void zero_first_pass(int lo, int m, const int *__restrict__ rp,
                                                          const int *__restrict__ ci, const double *__restrict__ v,
                                                          const int *__restrict__ split, const double *__restrict__ b,
                                                          const double *__restrict__ deff, double *__restrict__ P,
                                                          double *__restrict__ y)
{
    const int q = blockIdx.x * kBlock + threadIdx.x;
    if (q >= m) return;
    const int r = lo + q;
    double t;
    if (TWO) {   // rows of the pass's [N | L] matrix (local numbering): P = b - N x, t = P - L x
        const double Pq = zero_x_sum(b[r], ci, v, rp[q], split[q], -1);
        P[q] = Pq;
        t = zero_x_sum(Pq, ci, v, split[q], rp[q + 1], -1);
    } else {     // rows of the level matrix: every entry but the diagonal
        t = zero_x_sum(b[r], ci, v, rp[r], rp[r + 1], r);
    }
    const double d = deff[r];
    y[q] = div_ok(d) ? t / d : 0.0;   // a row that keeps its value keeps x_r = +0.0
}

// The tile-path relaxation (relax_range, MODE M) of the row blocks [b0, b1) of pass ps: new values into
// y (MODE 0 / 2: into x), the divisor from the staged diagonal when deff is null; MODE 2 / 3 also write
// the rows' residual r and its per-block sums of squares.
template <int M>
static void launch_tile(const SmootherPlan &sp, const DevCSR &A, const PassSchedule &ps, int b0, int b1, const double *b,
                        double *x, double *y, const double *deff, double *r, double *partial, XSrc xs, hipStream_t s)
{
    with_tile_kind(A, [&](auto K) {
        launch_relax_range<M, decltype(K)::value>(b0, b1 - b0, s, devdict(A, 0), A.bk, A.rp, A.ci, A.v, sp.diag_pos, ps.lo,
                                                  b, x, (const double *)nullptr, y, deff, A.pk, A.pv, A.pb, r, partial, xs);
    });
}
// tile passes take each row's divisor from its staged diagonal (no deff stream)
static bool tile_diag(const SmootherPlan &sp, const DevCSR &A) { return sp.own_diag && (A.pk != nullptr || has_dict(A)); }

int launch_f_residual_pending(const SmootherPlan &sp, const DevCSR &A, const double *b, const double *x, double *r,
                              double *partial, double *pend, hipStream_t s)
{
    if (!sp.pend_ok) return ERROR_INPUT_PAR;
    const PassSchedule &F = sp.pass[0];
    const double *deff = tile_diag(sp, A) ? nullptr : sp.d_first;
    ledger_pass(A, F, deff ? 40.0 : 32.0);   // b, r, pend (and deff)
    launch_tile<3>(sp, A, F, F.blo, F.bhi, b, const_cast<double *>(x), pend, deff, r, partial, xsrc_of(x), s);
    SSS_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(kBlock) void scatter_rows(int m, const int *__restrict__ map, const double *__restrict__ y,
                                                       double *__restrict__ x)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r < m) x[map[r]] = y[r];
}

// One launch per DAG depth of an exact pass (the schedule of PassSchedule::h_off).
static int depth_launches(const PassSchedule &ps, bool long_rows, bool nat, const DevCSR &A, const double *b, double *x,
                          const double *deff, hipStream_t s)
{
    ledger_pass(A, ps, 24.0);   // b, deff, x written
    for (int l = 0; l < ps.depth; ++l) {
        const int off = ps.h_off[l], cnt = ps.h_off[l + 1] - off;
        if (cnt == 0) continue;
        if (long_rows)
            hipLaunchKernelGGL(nat ? gs_depth_wave<true> : gs_depth_wave<false>, dim3((cnt + 3) / 4), dim3(kBlock), 0, s,
                               ps.rows + off, cnt, A.rp, A.ci, A.v, b, x, deff);
        else
            hipLaunchKernelGGL(nat ? gs_depth_thread<true> : gs_depth_thread<false>, dim3((cnt + kBlock - 1) / kBlock),
                               dim3(kBlock), 0, s, ps.rows + off, cnt, A.rp, A.ci, A.v, b, x, deff);
    }
    SSS_HIP(hipGetLastError());
    return 0;
}

// ---- smoother_run: decide the form of each pass, then run it --------------------------------------
enum class PassForm {
    Skip,            // no rows, or the first F pass came with the last residual (pre_f)
    TwoStageHooks,   // two-stage on a distributed level: iterates in the hooks' full-length vectors
    NoCopy,          // C/F-Jacobi or two-stage alternating between x and the plan's x2
    TwoStage,        // two-stage through y / y2, copied back
    ZeroFirst,       // C/F-Jacobi on a zero x, in place
    Jacobi,          // C/F-Jacobi through y, copied back
    FusedResid,      // exact range pass that also writes its rows' residual (MODE 2)
    Range,           // exact range pass (MODE 0)
    CompactJacobi,   // C/F-Jacobi on the class's sub-CSR + scatter
    CompactExact,    // exact depth-1 pass on the class's sub-CSR
    Flow,            // one-launch exact pass
    Depths           // one launch per DAG depth
};
// What of a smoother_run call decides the form of its passes.
struct PassCall {
    bool hooks, halo_split;   // PassHooks given; with a split hook
    bool x_zero, resid, pre_f, wave, nocopy;
    int sweeps;
};
struct PassChoice {
    PassForm form;
    bool zfirst;   // first pass on a just-zeroed iterate (C/F-Jacobi / two-stage): t = b, no matrix read
    bool split;    // a plain tile-path relaxation pass (exact depth-1 GS-CF, or C/F-Jacobi) overlaps the
                   // halo with its interior blocks (PassHooks::split)
};
static PassChoice pass_form(const SmootherPlan &sp, int c, int sw, const PassCall &k)
{
    const PassSchedule &ps = sp.pass[c];
    const bool jacobi = sp.kind == SSS_HIP_SMOOTH_JACOBI;
    PassChoice r{PassForm::Skip, false, false};
    if (ps.nrows == 0 || (k.pre_f && sw == 0 && c == 0)) return r;
    r.zfirst = k.x_zero && sw == 0 && c == 0 && sp.finite && jacobi;
    r.split = k.halo_split && !r.zfirst && !k.wave && ps.range && (!jacobi || sp.inner == 0) && !k.nocopy;
    if (!ps.range)
        r.form = jacobi ? PassForm::CompactJacobi : ps.compact ? PassForm::CompactExact : ps.gp.engine ? PassForm::Flow : PassForm::Depths;
    else if (jacobi)
        r.form = sp.inner > 0 && k.hooks ? PassForm::TwoStageHooks : k.nocopy ? PassForm::NoCopy : sp.inner > 0 ? PassForm::TwoStage
                 : r.zfirst ? PassForm::ZeroFirst : PassForm::Jacobi;
    else
        r.form = k.resid && sp.fuse_resid && c == 1 && sw + 1 == k.sweeps ? PassForm::FusedResid : PassForm::Range;
    return r;
}

struct PassRun {   // one pass as its form takes it
    const SmootherPlan &sp;
    const DevCSR &A;
    const PassSchedule &ps;
    const double *b;
    double *x;
    const double *deff;
    XSrc xs;
    hipStream_t s;
    const PassHooks *hk;
    bool zfirst, split;
    int m() const { return ps.hi - ps.lo; }
    int zgrid() const { return (m() + kBlock - 1) / kBlock; }
};

// A relaxation of the whole range pass (MODE M: 0 in place, 1 into y, 2 in place + residual): wave
// kernels on a long-row level, else the tile path, around the halo when the pass is split.
template <int M>
static int relax_pass(const PassRun &p, double *y, ResidFuse *rf = nullptr)
{
    const DevCSR &A = p.A;
    const PassSchedule &ps = p.ps;
    const bool wave = A.wave_rows || A.vec_rows, tile_d = tile_diag(p.sp, A);
    if (rf) ledger_pass(A, ps, tile_d ? 24.0 : 32.0);   // b, x and r written (and deff)
    else ledger_pass(A, ps, (tile_d && !wave) ? 16.0 : 24.0);   // b, the written row (and deff)
    if constexpr (M != 2)   // a long-row level never fuses the residual (SmootherPlan::fuse_resid)
        if (wave) {
            hipLaunchKernelGGL((A.vec_rows ? relax_range_wave<M, true> : relax_range_wave<M, false>), dim3((p.m() + 3) / 4),
                               dim3(kBlock), 0, p.s, ps.lo, ps.hi, A.rp, A.ci, A.v, p.b, p.x, (const double *)nullptr, y,
                               p.deff, p.xs);
            return 0;
        }
    auto go = [&](int b0, int b1) {
        launch_tile<M>(p.sp, A, ps, b0, b1, p.b, p.x, y, tile_d ? nullptr : p.deff, rf ? rf->r : nullptr,
                       rf ? rf->partial : nullptr, p.xs, p.s);
    };
    if (p.split) return p.hk->split(p.x, ps.blo, ps.bhi, go);
    go(ps.blo, ps.bhi);
    return 0;
}

static int copy_rows(double *dst, const double *src, int m, hipStream_t s)
{
    ledger_add(16.0 * m);
    SSS_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, s));
    return 0;
}
// zero_first_pass on the [N | L] rows (P kept) or on the level matrix's rows
static void launch_zero_first(const PassRun &p, bool two, double *y)
{
    const PassSchedule &ps = p.ps;
    if (two)
        hipLaunchKernelGGL(zero_first_pass<true>, dim3(p.zgrid()), dim3(kBlock), 0, p.s, ps.lo, p.m(), ps.ts_nl.rp,
                           ps.ts_nl.ci, ps.ts_nl.v, ps.ts_split, p.b, p.deff, ps.ts_P, y);
    else
        hipLaunchKernelGGL(zero_first_pass<false>, dim3(p.zgrid()), dim3(kBlock), 0, p.s, ps.lo, p.m(), p.A.rp, p.A.ci,
                           p.A.v, (const int *)nullptr, p.b, p.deff, (double *)nullptr, y);
}

// iterates live in full-length work vectors whose ghosts (lower-rank rows of this class) are
// refreshed after every stage
static int pass_two_stage_hooks(const PassRun &p)
{
    const PassSchedule &ps = p.ps;
    double *wcur = p.hk->w0, *wnxt = p.hk->w1;
    int rc;
    if (p.zfirst) {
        ledger_add(32.0 * p.m());
        launch_zero_first(p, true, wcur + ps.lo);
    } else
        launch_ts_stage0(ps.ts_nl, ps.lo, ps.ts_split, p.b, xsrc_of(p.x), p.deff, ps.ts_P, wcur + ps.lo, p.s);
    for (int st = 0; st < p.sp.inner; ++st) {
        if ((rc = p.hk->exchange(p.hk->ctx, wcur))) return rc;
        launch_ts_inner(ps.ts_lo, ps.lo, p.deff, ps.ts_P, wcur, 0, wcur + ps.lo, wnxt + ps.lo, p.s);
        std::swap(wcur, wnxt);
    }
    return copy_rows(p.x + ps.lo, wcur + ps.lo, p.m(), p.s);
}

// stage 0 (or the Jacobi pass) writes the other buffer; inner steps read only this class's previous
// iterate, so they alternate between the two buffers in place.  cur: where the class's values are.
static int pass_nocopy(const PassRun &p, double *&cur)
{
    const PassSchedule &ps = p.ps;
    const int inner = p.sp.inner;
    double *prev = cur == p.x ? p.sp.x2 : p.x, *next = cur;
    int rc;
    if (p.zfirst) {
        ledger_add((inner > 0 ? 32.0 : 24.0) * p.m());   // b, deff, y (and P)
        launch_zero_first(p, inner > 0, prev + ps.lo);
    } else if (inner > 0)
        launch_ts_stage0(ps.ts_nl, ps.lo, ps.ts_split, p.b, p.xs, p.deff, ps.ts_P, prev + ps.lo, p.s);
    else if ((rc = relax_pass<1>(p, prev + ps.lo)))
        return rc;
    for (int st = 0; st < inner; ++st) {
        launch_ts_inner(ps.ts_lo, ps.lo, p.deff, ps.ts_P, prev, 0, prev + ps.lo, next + ps.lo, p.s);
        std::swap(prev, next);
    }
    cur = prev;
    return 0;
}

static int pass_two_stage(const PassRun &p)
{
    const PassSchedule &ps = p.ps;
    launch_ts_stage0(ps.ts_nl, ps.lo, ps.ts_split, p.b, xsrc_of(p.x), p.deff, ps.ts_P, ps.y, p.s);
    double *ycur = ps.y, *ynxt = ps.y2;
    for (int st = 0; st < p.sp.inner; ++st) {
        launch_ts_inner(ps.ts_lo, ps.lo, p.deff, ps.ts_P, ycur, ps.lo, ycur, ynxt, p.s);
        std::swap(ycur, ynxt);
    }
    return copy_rows(p.x + ps.lo, ycur, p.m(), p.s);
}

// the pass reads no x at all, so it may write x in place
static int pass_zero_first(const PassRun &p)
{
    ledger_add(24.0 * p.m());
    launch_zero_first(p, false, p.x + p.ps.lo);
    return 0;
}

static int pass_jacobi(const PassRun &p)
{
    int rc = relax_pass<1>(p, p.ps.y);
    return rc ? rc : copy_rows(p.x + p.ps.lo, p.ps.y, p.m(), p.s);
}

static int pass_fused_resid(const PassRun &p, ResidFuse *rf)
{
    int rc = relax_pass<2>(p, nullptr, rf);
    if (!rc) rf->done = true;
    return rc;
}

// jacobi: new values into y, then scattered; else exact, in place
static int pass_compact(const PassRun &p, bool jacobi)
{
    const PassSchedule &ps = p.ps;
    const DevCSR &S = ps.sub;
    ledger_add((double)S.stream_bytes + (8.0 + 24.0 + (jacobi ? 20.0 : 4.0)) * ps.nrows);   // + the scatter / the row map
    double *y = jacobi ? ps.y : nullptr;
    const double *d = jacobi ? p.sp.d_first : p.deff;
    if (S.wave_rows)
        hipLaunchKernelGGL(jacobi ? relax_wave<false> : relax_wave<true>, dim3(S.ngrid), dim3(kBlock), 0, p.s, ps.nrows, S.rp,
                           S.ci, S.v, ps.map, p.b, p.x, y, d);
    else
        hipLaunchKernelGGL(jacobi ? relax_compact<false> : relax_compact<true>, dim3(S.nblk), dim3(kBlock), 0, p.s, S.blk,
                           S.rp, S.ci, S.v, ps.map, p.b, p.x, y, d);
    if (jacobi)
        hipLaunchKernelGGL(scatter_rows, dim3((ps.nrows + kBlock - 1) / kBlock), dim3(kBlock), 0, p.s, ps.nrows, ps.map,
                           ps.y, p.x);
    return 0;
}

static int pass_flow(const PassRun &p)
{
    ledger_pass(p.A, p.ps, 24.0);
    return gs_persist_run(p.ps, p.A, p.b, p.x, p.deff, p.s);
}

// natural-order GS: ascending pre-smoother, descending post-smoother
static int run_natural(const SmootherPlan &sp, const DevCSR &A, const double *b, double *x, int sweeps, hipStream_t s, bool post)
{
    const PassSchedule &ps = sp.pass[post ? 1 : 0];
    if (ps.nrows == 0) return 0;
    for (int sw = 0; sw < sweeps; ++sw) {
        const double *deff = post ? (sw == 0 ? sp.nd_first : sp.nd_later) : (sw == 0 ? sp.d_first : sp.d_later);
        PassRun p{sp, A, ps, b, x, deff, xsrc_of(x), s, nullptr, false, false};
        int rc = ps.gp.engine ? pass_flow(p) : depth_launches(ps, sp.long_rows, true, A, b, x, deff, s);
        if (rc) return rc;
    }
    return 0;
}

int smoother_run(const SmootherPlan &sp, const DevCSR &A, const double *b, double *x, int sweeps, hipStream_t s,
                 const PassHooks *hk, ResidFuse *rf, const double *pre_f, bool x_zero, bool post)
{
    if (rf) rf->done = false;
    if (sp.natural) return (hk || pre_f) ? ERROR_INPUT_PAR : run_natural(sp, A, b, x, sweeps, s, post);
    if (pre_f && (!sp.pend_ok || hk || sweeps < 1)) return ERROR_INPUT_PAR;
    if (sp.fz.engine && sweeps == sp.fz.sweeps && !hk && !pre_f) {
        for (int sw = 0; sw < sweeps; ++sw)
            for (const auto &ps : sp.pass) ledger_pass(A, ps, 24.0);
        return gs_fused_run(sp.fz, A, b, x, sp.d_first, sp.d_later, x_zero, s);
    }
    if (A.n == 0) return 0;
    int rc;
    // no-copy C/F-Jacobi: where each class's current values live (x or sp.x2)
    const bool nocopy = sp.x2 && !hk;
    const PassCall call{hk != nullptr, hk && hk->split, x_zero, rf != nullptr, pre_f != nullptr, A.wave_rows || A.vec_rows,
                        nocopy, sweeps};
    double *cur[2] = {x, x};
    for (int sw = 0; sw < sweeps; ++sw)
        for (int c = 0; c < 2; ++c) {
            const PassChoice ch = pass_form(sp, c, sw, call);
            if (ch.form == PassForm::Skip) continue;
            const PassSchedule &ps = sp.pass[c];
            if (hk) {   // distributed level: refresh x's ghosts; only contiguous passes qualify
                if (!ps.range) return ERROR_INPUT_PAR;
                // a zeroed x has zero ghosts (the descent clears own rows and ghosts); `finite` is
                // agreed over the ranks, so every rank skips this exchange together
                if (!ch.zfirst && !ch.split && (rc = hk->exchange(hk->ctx, x))) return rc;
            }
            XSrc xs = nocopy ? XSrc{cur[0], cur[1], sp.csplit} : xsrc_of(x);
            if (pre_f && sw == 0) xs = XSrc{pre_f, x, sp.pass[0].hi};   // this sweep's F values
            const PassRun p{sp, A, ps, b, x, sw == 0 ? sp.d_first : sp.d_later, xs, s, hk, ch.zfirst, ch.split};
            switch (ch.form) {
            case PassForm::TwoStageHooks: rc = pass_two_stage_hooks(p); break;
            case PassForm::NoCopy: rc = pass_nocopy(p, cur[c]); break;
            case PassForm::TwoStage: rc = pass_two_stage(p); break;
            case PassForm::ZeroFirst: rc = pass_zero_first(p); break;
            case PassForm::Jacobi: rc = pass_jacobi(p); break;
            case PassForm::FusedResid: rc = pass_fused_resid(p, rf); break;
            case PassForm::Range: rc = relax_pass<0>(p, nullptr); break;
            case PassForm::CompactJacobi: rc = pass_compact(p, true); break;
            case PassForm::CompactExact: rc = pass_compact(p, false); break;
            case PassForm::Flow: rc = pass_flow(p); break;
            default: rc = depth_launches(ps, sp.long_rows, false, A, b, x, p.deff, s); break;
            }
            if (rc) return rc;
            // the F values came with the last residual and no later F pass overwrites x_F
            if (ps.range && pre_f && sw == 0 && c == 1 && sweeps == 1 && (rc = copy_rows(x, pre_f, sp.pass[0].hi, s)))
                return rc;
        }
    for (int c = 0; c < 2; ++c)   // odd number of writes to a class (odd sweeps x (1 + inner))
        if (cur[c] != x && (rc = copy_rows(x + sp.pass[c].lo, cur[c] + sp.pass[c].lo, sp.pass[c].hi - sp.pass[c].lo, s)))
            return rc;
    SSS_HIP(hipGetLastError());
    return 0;
}

}  // namespace sss
