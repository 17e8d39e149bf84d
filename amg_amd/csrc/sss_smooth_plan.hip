// sss_smooth_plan.hip — host planner of the smoothers (sss_smooth_plan.hpp; the plan itself: struct
// SmootherPlan in sss_engine.hpp).  Pure host code on the worker pool: no HIP runtime call and no
// kernel, so every step can be called and checked without a GPU (tools/smooth_plan_hash.cpp).
#include "sss_smooth_plan.hpp"

#include <algorithm>
#include <cmath>

namespace sss {

SmootherSwitches smoother_switches()
{
    auto on = [](const char *name) {
        const char *e = getenv(name);
        return !(e && *e == '0');
    };
    SmootherSwitches s;
    s.tile_diag = on("SSS_HIP_TILE_DIAG");
    s.gs_fused = on("SSS_HIP_GS_FUSED");
    s.nocopy = on("SSS_HIP_NOCOPY");
    s.zero_first = on("SSS_HIP_ZERO_FIRST");
    s.dead_prolong = on("SSS_HIP_DEAD_PROLONG");
    s.fuse_resid = on("SSS_HIP_FUSE_RESID");
    s.pend_f = on("SSS_HIP_PEND_F");
    return s;
}

void plan_row_classes(const SSS_MAT &A, const int *mark, RowClasses &o)
{
    const int n = A.num_rows;
    const int *rp = A.row_ptr, *ci = A.col_idx;
    const double *v = A.val;
    // filled by the row-parallel pass below (no serial zero-fill of n-length arrays)
    o.cls.resize(n), o.depth.resize(n), o.pushed.resize(n), o.diag_pos.resize(n), o.last_diag.resize(n), o.has_diag.resize(n);
    std::atomic<bool> all{true}, single{true};
    parallel_chunks(n, 1 << 16, [&](int lo, int hi) {
        bool a = true, s1 = true;
        for (int i = lo; i < hi; ++i) {
            o.cls[i] = mark ? (mark[i] == 1 ? 1 : 0) : 0;
            o.depth[i] = o.pushed[i] = 0;
            o.last_diag[i] = 0.0;
            o.has_diag[i] = 0;
            o.diag_pos[i] = -1;
            for (int k = rp[i]; k < rp[i + 1]; ++k)
                if (ci[k] == i) {
                    o.last_diag[i] = v[k];
                    if (o.has_diag[i]) s1 = false;
                    o.has_diag[i] = 1;
                    o.diag_pos[i] = k;
                }
            a = a && o.has_diag[i];
        }
        if (!a) all = false;
        if (!s1) single = false;
    });
    o.all_diag = all;
    o.single_diag = single;
}

bool plan_coupled(const SSS_MAT &A, const RowClasses &rc)
{
    const int n = A.num_rows;
    const int *rp = A.row_ptr, *ci = A.col_idx;
    std::atomic<bool> coupled{false};
    parallel_chunks(n, 1 << 16, [&](int lo, int hi) {
        for (int i = lo; i < hi && !coupled; ++i)
            for (int k = rp[i]; k < rp[i + 1]; ++k) {
                const int j = ci[k];
                if (j != i && j < n && rc.cls[j] == rc.cls[i]) {
                    coupled = true;
                    break;
                }
            }
    });
    return coupled;
}

void plan_stale_divisors(const RowClasses &rc, int n, StaleDivisors &o)
{
    if (rc.all_diag) return;
    o.first.resize(n), o.later.resize(n);
    double d = 0.0;
    for (int sweep = 0; sweep < 2; ++sweep)
        for (int c = 0; c < 2; ++c)
            for (int i = 0; i < n; ++i) {
                if (rc.cls[i] != c) continue;
                if (rc.has_diag[i]) d = rc.last_diag[i];
                (sweep == 0 ? o.first : o.later)[i] = d;
            }
}

void plan_natural_divisors(const SSS_MAT &A, int lo, int hi, NaturalDivisors &o)
{
    const int n = A.num_rows, m = hi - lo;
    const int *rp = A.row_ptr, *ci = A.col_idx;
    const double *v = A.val;
    for (int dir = 0; dir < 2; ++dir) {
        o.first[dir].assign(n, 0.0), o.later[dir].assign(n, 0.0);
        double d = 0.0;
        for (int sweep = 0; sweep < 2; ++sweep)
            for (int q = 0; q < m; ++q) {
                const int i = dir == 0 ? lo + q : hi - 1 - q;
                for (int k = rp[i]; k < rp[i + 1]; ++k)
                    if (ci[k] == i && SSS_ABS(v[k]) > SMALLFLOAT) d = 1.e+0 / v[k];
                (sweep == 0 ? o.first : o.later)[dir][i] = d;
            }
    }
}

// The m rows of an order (ascending from `first`, or descending from it); same(i, j): column j of row
// i is a row of the same pass.
template <bool desc, class Same>
static void schedule_depths(const SSS_MAT &A, int first, int m, Same same, int *depth, int *pushed)
{
    const int *rp = A.row_ptr, *ci = A.col_idx;
    for (int q = 0; q < m; ++q) {
        const int i = desc ? first - q : first + q;
        int dep = pushed[i];
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            const int j = ci[k];
            if ((desc ? j > i : j < i) && same(i, j)) dep = std::max(dep, depth[j] + 1);
        }
        depth[i] = dep;
        for (int k = rp[i]; k < rp[i + 1]; ++k) {
            const int j = ci[k];
            if ((desc ? j < i : j > i) && same(i, j)) pushed[j] = std::max(pushed[j], dep + 1);
        }
    }
}

void schedule_classes(const SSS_MAT &A, RowClasses &rc)
{
    const int n = A.num_rows;
    const int *cls = rc.cls.data();
    schedule_depths<false>(A, 0, n, [=](int i, int j) { return j < n && cls[j] == cls[i]; }, rc.depth.data(),
                           rc.pushed.data());
}

void schedule_natural(const SSS_MAT &A, int lo, int hi, bool desc, std::vector<int> &depth)
{
    std::vector<int> pushed(A.num_rows, 0);
    depth.assign(A.num_rows, 0);
    auto same = [=](int, int j) { return j >= lo && j < hi; };
    if (desc) schedule_depths<true>(A, hi - 1, hi - lo, same, depth.data(), pushed.data());
    else schedule_depths<false>(A, lo, hi - lo, same, depth.data(), pushed.data());
}

void bucket_rows(int lo, int hi, const int *cls, int c, const int *depth, DepthBuckets &o)
{
    auto in = [&](int i) { return !cls || cls[i] == c; };
    int maxd = -1;
    for (int i = lo; i < hi; ++i)
        if (in(i)) maxd = std::max(maxd, depth[i]);
    o.depth = maxd + 1;
    o.h_off.assign(o.depth + 1, 0);
    for (int i = lo; i < hi; ++i)
        if (in(i)) o.h_off[depth[i] + 1]++;
    o.max_width = 0;
    for (int l = 0; l < o.depth; ++l) {
        o.max_width = std::max(o.max_width, o.h_off[l + 1]);
        o.h_off[l + 1] += o.h_off[l];
    }
    o.nrows = o.h_off[o.depth];
    std::vector<int> fill(o.h_off);
    o.rows.assign(std::max(o.nrows, 1), 0);
    for (int i = lo; i < hi; ++i)
        if (in(i)) o.rows[fill[depth[i]]++] = i;
}

ClassRange class_range(const int *cls, int n, int c, const DevCSR *dA)
{
    ClassRange r;
    for (int i = 0; i < n && r.contiguous; ++i) {
        if (cls[i] != c) continue;
        if (r.lo < 0) r.lo = i;
        else if (i != r.hi) r.contiguous = false;
        r.hi = i + 1;
    }
    if (!r.contiguous || !dA) return r;
    // the pass must be a whole number of the level's row blocks
    if (r.lo == 0 && r.hi == n) r.blocks = true, r.blo = 0, r.bhi = dA->nblk;
    else if (r.lo == 0 && r.hi == dA->split_row) r.blocks = true, r.blo = 0, r.bhi = dA->split_blk;
    else if (r.lo == dA->split_row && r.hi == n) r.blocks = true, r.blo = dA->split_blk, r.bhi = dA->nblk;
    return r;
}

static SSS_MAT host_mat(int rows, int ncols, std::vector<int> &rp, int *ci, double *v)
{
    SSS_MAT M;
    M.num_rows = rows;
    M.num_cols = ncols;
    M.num_nnzs = rp[rows];
    M.row_ptr = rp.data();
    M.col_idx = ci;
    M.val = v;
    return M;
}

SSS_MAT CompactRows::mat(int ncols) { return host_mat((int)map.size(), ncols, rp, ci.data(), v.data()); }

void build_compact_rows(const SSS_MAT &A, const int *cls, int c, CompactRows &o)
{
    for (int i = 0; i < A.num_rows; ++i) {
        if (cls[i] != c) continue;
        o.map.push_back(i);
        for (int k = A.row_ptr[i]; k < A.row_ptr[i + 1]; ++k) {
            o.ci.push_back(A.col_idx[k] == i ? -1 : A.col_idx[k]);   // diagonal -> product +0.0 (identity)
            o.v.push_back(A.val[k]);
        }
        o.rp.push_back((int)o.ci.size());
    }
}

SSS_MAT TwoStageSplit::Mn(int ncols) { return host_mat((int)split.size(), ncols, nrp, nci.data(), nv.data()); }
SSS_MAT TwoStageSplit::Ml(int ncols) { return host_mat((int)split.size(), ncols, lrp, lci.data(), lv.data()); }

static inline bool ts_lower(int n, int lo, int c, const int *gcls, int i, int j)
{
    return j < n ? (j >= lo && j < i) : (gcls && gcls[j - n] == c);
}

// two row-parallel passes: count, then fill at the prefix offsets (same order as a sequential
// build: N_i entries in stored order, then L_i entries in stored order)
void two_stage_count(const SSS_MAT &A, int lo, int m, int c, const int *gcls, TwoStageSplit &o)
{
    const int n = A.num_rows;
    const int *rp = A.row_ptr, *ci = A.col_idx;
    o.nrp.assign((size_t)m + 1, 0), o.lrp.assign((size_t)m + 1, 0), o.split.resize(m);
    parallel_chunks(m, 1 << 12, [&](int a, int e) {
        for (int q = a; q < e; ++q) {
            const int i = lo + q;
            int nn = 0, nl = 0;
            for (int k = rp[i]; k < rp[i + 1]; ++k) {
                const int j = ci[k];
                if (ts_lower(n, lo, c, gcls, i, j)) ++nl;
                else if (j != i) ++nn;
            }
            o.nrp[q + 1] = nn + nl;
            o.lrp[q + 1] = nl;
        }
    });
    for (int q = 0; q < m; ++q) o.nrp[q + 1] += o.nrp[q], o.lrp[q + 1] += o.lrp[q];
}

void two_stage_fill(const SSS_MAT &A, int lo, int m, int c, const int *gcls, TwoStageSplit &o)
{
    const int n = A.num_rows;
    const int *rp = A.row_ptr, *ci = A.col_idx;
    const double *v = A.val;
    o.nci.resize((size_t)o.nrp[m]), o.lci.resize((size_t)o.lrp[m]), o.nv.resize((size_t)o.nrp[m]), o.lv.resize((size_t)o.lrp[m]);
    parallel_chunks(m, 1 << 12, [&](int a, int e) {
        for (int q = a; q < e; ++q) {
            const int i = lo + q;
            int p = o.nrp[q], pl = o.lrp[q];
            for (int k = rp[i]; k < rp[i + 1]; ++k) {   // N_i: off-diagonal, not same-class lower
                const int j = ci[k];
                if (j != i && !ts_lower(n, lo, c, gcls, i, j)) o.nci[p] = j, o.nv[p] = v[k], ++p;
            }
            o.split[q] = p;
            for (int k = rp[i]; k < rp[i + 1]; ++k) {   // L_i
                const int j = ci[k];
                if (ts_lower(n, lo, c, gcls, i, j)) {
                    o.nci[p] = j, o.nv[p] = v[k], ++p;
                    o.lci[pl] = j, o.lv[pl] = v[k], ++pl;
                }
            }
        }
    });
}

bool plan_own_diag(const RowClasses &rc, const SmootherSwitches &sw)
{
    return rc.all_diag && rc.single_diag && sw.tile_diag;
}

bool plan_finite(const SSS_MAT &A, const SmootherSwitches &sw)
{
    const int *rp = A.row_ptr;
    const double *v = A.val;
    std::atomic<bool> fin{sw.zero_first};
    if (fin)
        parallel_chunks(A.num_rows, 1 << 16, [&](int lo, int hi) {
            for (int k = rp[lo]; k < rp[hi] && fin; ++k)
                if (!std::isfinite(v[k])) fin = false;
        });
    return fin;
}

int plan_nocopy_split(const SmootherPlan &sp, const SSS_MAT &A, const int *gcls, const SmootherSwitches &sw)
{
    const int n = A.num_rows;
    if (!sw.nocopy || sp.kind != SSS_HIP_SMOOTH_JACOBI || gcls || A.num_cols != n) return -1;
    const PassSchedule &F = sp.pass[0], &Cp = sp.pass[1];
    const bool f_ok = F.nrows == 0 || (F.range && F.lo == 0), c_ok = Cp.nrows == 0 || (Cp.range && Cp.hi == n);
    const int cs = F.nrows > 0 ? F.hi : 0;
    return f_ok && c_ok && (Cp.nrows == 0 || Cp.lo == cs) && (F.nrows > 0 || Cp.nrows > 0) ? cs : -1;
}

bool plan_f_overwritten(const SmootherPlan &sp, const RowClasses &rc, const double *d_first, const double *d_later,
                        const SmootherSwitches &sw)
{
    const PassSchedule &F = sp.pass[0];
    bool ok = sw.dead_prolong && sp.kind != SSS_HIP_SMOOTH_JACOBI && F.range && F.lo == 0 && F.nrows > 0 && F.depth <= 1 &&
              rc.single_diag;
    for (int i = F.lo; ok && i < F.hi; ++i) ok = std::fabs(d_first[i]) > SMALLFLOAT && std::fabs(d_later[i]) > SMALLFLOAT;
    return ok;
}

void plan_fused_flags(SmootherPlan &sp, const SSS_MAT &A, const DevCSR *dA, const RowClasses &rc, const SmootherSwitches &sw)
{
    const int n = A.num_rows;
    const int *rp = A.row_ptr;
    if (!sw.fuse_resid || sp.kind == SSS_HIP_SMOOTH_JACOBI || !dA || dA->wave_rows || dA->vec_rows || !rc.all_diag ||
        !rc.single_diag || dA->split_row <= 0 || dA->split_row >= n || !sp.pass[0].range || !sp.pass[1].range ||
        sp.pass[0].lo != 0 || sp.pass[0].hi != dA->split_row || sp.pass[1].lo != dA->split_row || sp.pass[1].hi != n)
        return;
    // the MODE 2 / 3 passes have no long-row path: every block of the pass within one tile (the
    // ELL formats take one row per thread and rows of at most 32 entries)
    std::vector<int> blk;
    const bool ell = dA->dv_ell || dA->dv_xell;
    if (!ell) build_row_blocks(rp, n, blk, dA->split_row);
    auto all_short = [&](int b0, int b1) {
        bool ok = true;
        for (int q = b0; !ell && q < b1 && ok; ++q) ok = rp[blk[q + 1]] - rp[blk[q]] <= kTileEntries;
        return ok;
    };
    sp.fuse_resid = all_short(dA->split_blk, dA->nblk);
    sp.pend_ok = sp.fuse_resid && all_short(0, dA->split_blk) && sp.f_overwritten && sw.pend_f;
}

}  // namespace sss
