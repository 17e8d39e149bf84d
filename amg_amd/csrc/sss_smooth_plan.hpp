// sss_smooth_plan.hpp — host planner of the smoothers (sss_smooth_plan.hip).  Pure host code: no HIP
// runtime call, no kernel.  Each step fills one plain struct with the arrays exactly as smoother_build
// / smoother_build_natural (sss_smooth.hip) upload them; a decision that depends on an environment
// switch takes it from a SmootherSwitches argument.
#pragma once

#include "sss_engine.hpp"

namespace sss {

// The environment switches a smoother build reads (SSS_HIP_<name>; "0" turns the form off, tests
// compare both ways), as smoother_switches() finds them at the time of the call.
struct SmootherSwitches {
    bool tile_diag;      // TILE_DIAG: 0 = divisors from the deff stream
    bool gs_fused;       // GS_FUSED: 0 = per-pass launches instead of one launch per call
    bool nocopy;         // NOCOPY: 0 = C/F-Jacobi through per-pass copies
    bool zero_first;     // ZERO_FIRST: 0 = run the first pass on a zero x in full
    bool dead_prolong;   // DEAD_PROLONG: 0 = always prolong into every row
    bool fuse_resid;     // FUSE_RESID: 0 = never fuse the residual into the last C pass
    bool pend_f;         // PEND_F: 0 = never precompute the first F pass
};
SmootherSwitches smoother_switches();

// Per row: class (1 = C), CSR position and value of the last diagonal entry (-1 / 0.0: none), whether
// there is one; depth / pushed: the scheduler's state of the C/F order, zeroed by the same pass.
struct RowClasses {
    HostBuf<int> cls, diag_pos, depth, pushed;
    HostBuf<double> last_diag;
    HostBuf<char> has_diag;
    bool all_diag = true, single_diag = true;   // every row has a diagonal entry; no row has two
};
void plan_row_classes(const SSS_MAT &A, const int *mark, RowClasses &out);
// any same-class off-diagonal entry at all?
bool plan_coupled(const SSS_MAT &A, const RowClasses &rc);

// Stale divisors of the C/F order: the reference's divisor register over two sweeps of (F pass, C pass).
// Empty when every row has a diagonal (each row then divides by its own last diagonal entry).
struct StaleDivisors {
    HostBuf<double> first, later;
};
void plan_stale_divisors(const RowClasses &rc, int n, StaleDivisors &out);

// The carried reciprocal d of the natural order over the rows [lo, hi) (Solve/SSS_smooth.c:106-109), per
// direction (0 ascending, 1 descending): first sweep from d = 0, later sweeps from the sweep before.
struct NaturalDivisors {
    std::vector<double> first[2], later[2];
};
void plan_natural_divisors(const SSS_MAT &A, int lo, int hi, NaturalDivisors &out);

// Depth of every row in its pass: 1 + the deepest coupled row of the pass taken before it
// (read-after-write), every coupled row of the pass taken after it pushed below it (write-after-read).
// C/F order: a pass is a class, rows ascending; depth and pushed of rc are updated in place.
void schedule_classes(const SSS_MAT &A, RowClasses &rc);
// Natural order: the pass is the rows [lo, hi), ascending or descending; depth: n entries.
void schedule_natural(const SSS_MAT &A, int lo, int hi, bool desc, std::vector<int> &depth);

// The rows [lo, hi) of class c (cls null: all of them) grouped by depth: PassSchedule::h_off / rows.
struct DepthBuckets {
    int depth = 0, nrows = 0, max_width = 0;
    std::vector<int> h_off, rows;
};
void bucket_rows(int lo, int hi, const int *cls, int c, const int *depth, DepthBuckets &out);

// The rows of class c as a range [lo, hi) when they are contiguous, and as whole row blocks
// [blo, bhi) of the level matrix when the range is all of it or one side of its class split.
struct ClassRange {
    bool contiguous = true, blocks = false;
    int lo = -1, hi = -1, blo = 0, bhi = 0;
};
ClassRange class_range(const int *cls, int n, int c, const DevCSR *dA = nullptr);

// Row-compacted CSR of class c (rows ascending; a diagonal entry's column is -1) and its row map.
struct CompactRows {
    std::vector<int> rp{0}, ci, map;
    std::vector<double> v;
    SSS_MAT mat(int ncols);
};
void build_compact_rows(const SSS_MAT &A, const int *cls, int c, CompactRows &out);

// Two-stage split of the pass of class c over the rows [lo, lo + m): every row's off-diagonal entries
// as [N_i | L_i] (nl; split = the absolute cut of each row) and L_i alone (lo_), both in stored order.
// L_i: same class, j < i in the global order -- own rows of the pass below i, or (gcls, distributed
// levels) ghost columns of this class owned by lower ranks.
struct TwoStageSplit {
    std::vector<int> nrp, lrp, split;
    HostBuf<int> nci, lci;   // every slot written by the fill (no serial zero-fill)
    HostBuf<double> nv, lv;
    SSS_MAT Mn(int ncols), Ml(int ncols);
};
void two_stage_count(const SSS_MAT &A, int lo, int m, int c, const int *gcls, TwoStageSplit &out);
void two_stage_fill(const SSS_MAT &A, int lo, int m, int c, const int *gcls, TwoStageSplit &out);

// ---- eligibility flags of SmootherPlan (the pass fields of sp are set by then) -----------------
bool plan_own_diag(const RowClasses &rc, const SmootherSwitches &sw);
bool plan_finite(const SSS_MAT &A, const SmootherSwitches &sw);
// first row of the no-copy form's C class, or -1: the form does not apply
int plan_nocopy_split(const SmootherPlan &sp, const SSS_MAT &A, const int *gcls, const SmootherSwitches &sw);
// d_first / d_later: the divisors as they are uploaded
bool plan_f_overwritten(const SmootherPlan &sp, const RowClasses &rc, const double *d_first, const double *d_later,
                        const SmootherSwitches &sw);
// sets sp.fuse_resid and sp.pend_ok (after sp.f_overwritten)
void plan_fused_flags(SmootherPlan &sp, const SSS_MAT &A, const DevCSR *dA, const RowClasses &rc,
                      const SmootherSwitches &sw);

}  // namespace sss
