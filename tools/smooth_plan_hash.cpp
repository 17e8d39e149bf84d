// One 64-bit hash per array and per flag of a smoother plan (amg_amd/csrc/sss_smooth_plan.hip, and the
// steps of smoother_build / smoother_build_natural in sss_smooth.hip that hand its arrays to the
// device), on small matrices chosen to reach every branch.  No GPU: the units are included textually,
// the worker pool is replaced by inline execution, and the upload entry points (dev_upload,
// devcsr_upload, dev_alloc) are tapped by macros: a tap hashes the host array it is given, in the order
// of the calls, and hands out an address that is never dereferenced.  No HIP call is made.
//
//   hipcc -O2 -std=c++17 -x hip --offload-arch=gfx950 -ffp-contract=off -Iamg_amd/csrc \
//       tools/smooth_plan_hash.cpp -o tools/smooth_plan_hash && tools/smooth_plan_hash > hashes.txt
//
// Two builds of the planner produce the same bytes in the same upload order iff the two lists are
// identical.  The same main runs against a commit from before the planner had a unit of its own: add
// -DPLAN_PARENT and point -I at that commit's amg_amd/csrc.  The program also checks the definition of
// a level schedule on every exact plan (exit status 1 if it fails): for every stored entry (i, j),
// i != j, of one pass the lower-numbered row is strictly shallower (strictly deeper for the descending
// natural order).  (-Xarch_host -fsanitize=address,undefined works on this stand-alone program.)
#include "sss_engine.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

static std::string g_case;
static int g_seq = 0;
static std::map<const void *, std::vector<int>> g_ints;   // the int arrays "uploaded" in this case

static void put(const std::string &name, const void *p, size_t bytes)
{
    uint64_t h = 1469598103934665603ull;   // FNV-1a
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    printf("%-44s %016llx %zu\n", (g_case + "." + name).c_str(), (unsigned long long)h, bytes);
}
static void put(const std::string &name, long long x) { put(name, &x, sizeof(x)); }
static std::string step(const char *what) { return std::to_string(g_seq++) + "." + what; }
template <class T>
static T *fake_address()
{
    static uintptr_t next = 1 << 20;
    return reinterpret_cast<T *>(next += 64);
}

namespace sss {
template <class T>
T *tap_alloc(size_t count)
{
    put(step("alloc"), (long long)(count * sizeof(T)));
    return fake_address<T>();
}
template <class T>
int tap_upload(T *&dst, const T *src, size_t count, const char *)
{
    put(step("upload"), src, sizeof(T) * count);
    dst = fake_address<T>();
    if constexpr (std::is_same<T, int>::value) g_ints[dst].assign(src, src + count);
    return 0;
}
template <class T, class Array>
int tap_upload(T *&dst, const Array &src, const char *what)
{
    return tap_upload(dst, src.data(), src.size(), what);
}
int tap_csr(DevCSR &d, const SSS_MAT &h, int split = -1, int enc = 0, const int *seg = nullptr)
{
    const std::string t = step("csr");
    put(t + ".shape", h.num_rows * 1000000000LL + h.num_cols * 10000LL + (split + 1) * 100 + enc);
    put(t + ".nnz", h.num_nnzs);
    put(t + ".rp", h.row_ptr, sizeof(int) * ((size_t)h.num_rows + 1));
    put(t + ".ci", h.col_idx, sizeof(int) * (size_t)h.num_nnzs);
    put(t + ".v", h.val, sizeof(double) * (size_t)h.num_nnzs);
    if (seg) put(t + ".seg", seg, sizeof(int) * (size_t)h.num_rows);
    d.n = h.num_rows, d.ncols = h.num_cols, d.nnz = h.num_nnzs;
    return 0;
}
}   // namespace sss
#define dev_alloc tap_alloc
#define dev_upload tap_upload
#define devcsr_upload tap_csr

#include "sss_formats.hip"   // build_row_blocks
#ifndef PLAN_PARENT
#include "sss_smooth_plan.hip"
#endif
#include "sss_smooth.hip"

#undef dev_alloc
#undef dev_upload
#undef devcsr_upload

// what the two units call and this program never reaches, and the one-launch builders as recorders
extern "C" void sss_huge_hint(void *, size_t) {}
namespace sss {
int host_pool_threads() { return 1; }   // parallel_chunks runs inline
bool host_pool_run(const std::function<void()> &) { return false; }
int hip_fail(hipError_t, const char *, const char *, int) { return ERROR_MISC; }
int wave_row_min() { return 12; }
thread_local ByteLedger *g_ledger = nullptr;
double matrix_bytes_rows(const DevCSR &, int, int) { return 0.0; }
DevDict devdict(const DevCSR &, int) { return DevDict{}; }
int gs_persist_build(PassSchedule &ps, const SSS_MAT &A, int lo, int hi, bool long_rows, bool natural, bool desc)
{
    put(step("gs_persist_build"), A.num_rows * 100000000LL + lo * 10000LL + hi * 8 + long_rows * 4 + natural * 2 + desc);
    ps.gp.engine = 1;
    return 0;
}
void gs_persist_free(PassSchedule &) {}
int gs_persist_run(const PassSchedule &, const DevCSR &, const double *, double *, const double *, hipStream_t) { return 0; }
int gs_fused_build(GsFused &f, const SSS_MAT &A, const DevCSR *dA, const PassSchedule *pass, const int *cls, int sweeps)
{
    const std::string t = step("gs_fused_build");
    put(t + ".cls", cls, sizeof(int) * (size_t)A.num_rows);
    put(t + ".args", sweeps * 1000000LL + (dA ? dA->split_row : -1) * 100 + pass[0].depth * 10 + pass[1].depth);
    f.engine = 1, f.sweeps = sweeps;
    return 0;
}
int gs_fused_run(const GsFused &, const DevCSR &, const double *, double *, const double *, const double *, bool, hipStream_t)
{
    return 0;
}
void gs_fused_free(GsFused &) {}
void devcsr_free(DevCSR &) {}
}   // namespace sss

using namespace sss;

struct Mat {
    std::vector<int> rp{0}, ci;
    std::vector<double> v;
    int ncols = 0;
    int n() const { return (int)rp.size() - 1; }
    void add(int c, double a) { ci.push_back(c), v.push_back(a); }
    void end_row() { rp.push_back((int)ci.size()); }
    SSS_MAT mat()
    {
        SSS_MAT m;
        m.num_rows = n(), m.num_cols = ncols, m.num_nnzs = (int)ci.size();
        m.row_ptr = rp.data(), m.col_idx = ci.data(), m.val = v.data();
        return m;
    }
};

static Mat poisson7(int N)
{
    Mat m;
    m.ncols = N * N * N;
    for (int z = 0; z < N; ++z)
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) {
                const int i = (z * N + y) * N + x;
                if (z > 0) m.add(i - N * N, -1.0);
                if (y > 0) m.add(i - N, -1.0);
                if (x > 0) m.add(i - 1, -1.0);
                m.add(i, 6.0 + 0.125 * (i % 5));
                if (x < N - 1) m.add(i + 1, -1.0);
                if (y < N - 1) m.add(i + N, -1.0);
                if (z < N - 1) m.add(i + N * N, -1.0);
                m.end_row();
            }
    return m;
}
static std::vector<int> red_black(int N)
{
    std::vector<int> mark;
    for (int z = 0; z < N; ++z)
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) mark.push_back((x + y + z) % 2);
    return mark;
}
static std::vector<int> every_third(int n)   // leaves F-F couplings, and C-C ones along z (12^2 = 0 mod 3)
{
    std::vector<int> mark(n);
    for (int i = 0; i < n; ++i) mark[i] = i % 3 == 0;
    return mark;
}
// rows relabeled F first, then C (each class ascending), every row's entries in their stored order
static Mat relabel(const Mat &a, std::vector<int> &mark)
{
    const int n = a.n();
    std::vector<int> order, pos(n);
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < n; ++i)
            if ((mark[i] == 1) == (c == 1)) pos[i] = (int)order.size(), order.push_back(i);
    Mat m;
    m.ncols = a.ncols;
    std::vector<int> nm(n);
    for (int q = 0; q < n; ++q) {
        const int i = order[q];
        for (int k = a.rp[i]; k < a.rp[i + 1]; ++k) m.add(pos[a.ci[k]], a.v[k]);
        m.end_row();
        nm[q] = mark[i];
    }
    mark = nm;
    return m;
}
// a nonsymmetric band: row i reads rows above it that do not read row i (write-after-read pushes)
static Mat band_nonsym(int n)
{
    Mat m;
    m.ncols = n;
    for (int i = 0; i < n; ++i) {
        for (int d : {-7, -3, -1, 0, 1, 2, 6})
            if (i + d >= 0 && i + d < n && (d == 0 || (i * 5 + d * 3 + 40) % 4 != 0)) m.add(i + d, d == 0 ? 9.0 : -1.0 - 0.25 * ((i + d) % 3));
        m.end_row();
    }
    return m;
}
// rows `none` lose their diagonal entry, row `twice` gets a second one
static Mat edit_diagonals(const Mat &a, const std::vector<int> &none, int twice)
{
    Mat m;
    m.ncols = a.ncols;
    for (int i = 0; i < a.n(); ++i) {
        const bool drop = std::find(none.begin(), none.end(), i) != none.end();
        for (int k = a.rp[i]; k < a.rp[i + 1]; ++k)
            if (!(drop && a.ci[k] == i)) m.add(a.ci[k], a.v[k]);
        if (i == twice) m.add(i, 2.5);
        m.end_row();
    }
    return m;
}
// every fifth row also reads one of g ghost columns
static Mat with_ghosts(const Mat &a, int g)
{
    Mat m;
    m.ncols = a.ncols + g;
    for (int i = 0; i < a.n(); ++i) {
        for (int k = a.rp[i]; k < a.rp[i + 1]; ++k) {
            if (i % 5 == 0 && k == a.rp[i] + 1) m.add(a.n() + (i / 5) % g, -0.5);
            m.add(a.ci[k], a.v[k]);
        }
        m.end_row();
    }
    return m;
}

static DevCSR blocked(const SSS_MAT &h, int split)   // the fields of an uploaded level matrix a plan reads
{
    DevCSR d;
    std::vector<int> blk;
    d.n = h.num_rows, d.ncols = h.num_cols, d.nnz = h.num_nnzs;
    d.nblk = build_row_blocks(h.row_ptr, h.num_rows, blk, split);
    d.split_row = split;
    for (int q = 0; q < d.nblk; ++q)
        if (blk[q] == split) d.split_blk = q;
    return d;
}

static int g_bad = 0;
// the definition of a level schedule, on the rows and depth offsets of the plan's two passes
static void check_schedule(const SmootherPlan &sp, const SSS_MAT &A)
{
    for (int c = 0; c < 2; ++c) {
        const PassSchedule &ps = sp.pass[c];
        const std::vector<int> &rows = g_ints[ps.rows];
        std::vector<int> depth((size_t)A.num_rows, -1);
        for (int l = 0; l < ps.depth; ++l)
            for (int q = ps.h_off[l]; q < ps.h_off[l + 1]; ++q) depth[rows[q]] = l;
        const bool desc = sp.natural && c == 1;
        long long bad = 0;
        for (int q = 0; q < ps.nrows; ++q) {
            const int i = rows[q];
            for (int k = A.row_ptr[i]; k < A.row_ptr[i + 1]; ++k) {
                const int j = A.col_idx[k];
                if (j == i || j >= A.num_rows || depth[j] < 0) continue;   // not a row of this pass
                const int lower = std::min(i, j), upper = std::max(i, j);
                bad += desc ? !(depth[lower] > depth[upper]) : !(depth[lower] < depth[upper]);
            }
        }
        if (bad) fprintf(stderr, "%s: pass %d breaks the schedule's definition at %lld entries\n", g_case.c_str(), c, bad);
        g_bad += bad != 0;
    }
}

static void put_plan(const SmootherPlan &sp, const SSS_MAT &A)
{
    put("kind_natural_long_inner", sp.kind * 1000 + sp.natural * 100 + sp.long_rows * 10 + sp.inner);
    put("csplit_x2", sp.csplit * 10LL + (sp.x2 != nullptr));
    put("flags.own_diag", sp.own_diag), put("flags.finite", sp.finite), put("flags.f_overwritten", sp.f_overwritten);
    put("flags.fuse_resid", sp.fuse_resid), put("flags.pend_ok", sp.pend_ok);
    put("d_later_aliases_d_first", sp.d_later == sp.d_first);
    put("diag_pos_cls_fused", (sp.diag_pos != nullptr) * 100 + (sp.cls != nullptr) * 10 + sp.fz.engine);
    for (int c = 0; c < 2; ++c) {
        const PassSchedule &ps = sp.pass[c];
        const std::string t = "pass" + std::to_string(c);
        put(t + ".depth_nrows", ps.depth * 100000LL + ps.nrows);
        if (!sp.natural) put(t + ".max_width", ps.max_width);
        put(t + ".h_off", ps.h_off.data(), sizeof(int) * ps.h_off.size());
        put(t + ".compact_range_engine", ps.compact * 100 + ps.range * 10 + ps.gp.engine);
        put(t + ".lo_hi", ps.lo * 100000LL + ps.hi), put(t + ".blo_bhi", ps.blo * 100000LL + ps.bhi);
        put(t + ".y_y2_map_split_P", (ps.y != nullptr) * 10000 + (ps.y2 != nullptr) * 1000 + (ps.map != nullptr) * 100 +
                                         (ps.ts_split != nullptr) * 10 + (ps.ts_P != nullptr));
    }
    // C/F-Jacobi schedules are never walked by depth (every row keeps depth 0)
    if (sp.kind == SSS_HIP_SMOOTH_EXACT) check_schedule(sp, A);
}

static void begin(const std::string &name)
{
    g_case = name, g_seq = 0;
    g_ints.clear();
}
static void plan(const std::string &name, Mat &m, const std::vector<int> &mark, int kind, int split, int inner = 0,
                 const int *gcls = nullptr, int enc = 0)
{
    begin(name);
    const SSS_MAT A = m.mat();
    const DevCSR dA = blocked(A, split);
    SmootherPlan sp;
    put("rc", smoother_build(sp, A, mark.empty() ? nullptr : mark.data(), kind, split == -2 ? nullptr : &dA, inner, gcls, enc));
    put_plan(sp, A);
}
static void natural(const std::string &name, Mat &m, int lo, int hi)
{
    begin(name);
    const SSS_MAT A = m.mat();
    SmootherPlan sp;
    put("rc", smoother_build_natural(sp, A, lo, hi));
    put_plan(sp, A);
}
static int count_f(const std::vector<int> &mark) { return (int)std::count(mark.begin(), mark.end(), 0); }

int main()
{
    const int E = SSS_HIP_SMOOTH_EXACT, J = SSS_HIP_SMOOTH_JACOBI;
    const Mat P = poisson7(12);
    const int n = P.n();

    // red-black, relabeled: depth 1, range passes over the two sides of the block split
    std::vector<int> rb = red_black(12);
    Mat R = relabel(P, rb);
    const int nF = count_f(rb);
    plan("redblack.exact", R, rb, E, nF);
    plan("redblack.jacobi", R, rb, J, nF);
    plan("redblack.exact.no_matrix", R, rb, E, -2);   // no DevCSR given: compact passes

    // F-F and C-C couplings: depth > 1, one-launch passes and the fused engine
    std::vector<int> third = every_third(n);
    Mat T = relabel(P, third);
    const int tF = count_f(third);
    plan("coupled.exact", T, third, E, tF);
    plan("coupled.jacobi", T, third, J, tF);

    // interleaved classes: the compact sub-CSR and its row map
    Mat Pi = P;
    const std::vector<int> rbi = red_black(12), thirdi = every_third(n);
    plan("interleaved.exact", Pi, rbi, E, -1);
    plan("interleaved.jacobi", Pi, rbi, J, -1);
    plan("interleaved.coupled.exact", Pi, thirdi, E, -1);

    // nonsymmetric band: the write-after-read push; no marker (one class), and two classes
    Mat B = band_nonsym(900);
    std::vector<int> halves(900);
    for (int i = 0; i < 900; ++i) halves[i] = i >= 500;
    plan("band.one_class", B, {}, E, -1);
    plan("band.two_classes", B, halves, E, 500);

    // the first F row and some C rows without a diagonal entry, one row with two: stale divisors
    Mat D = edit_diagonals(R, {0, nF + 3, nF + 4, n - 1}, 17), Di = edit_diagonals(P, {1, 6, 7, n - 2}, 40);
    plan("diagonals.exact", D, rb, E, nF);
    plan("diagonals.jacobi", D, rb, J, nF);
    plan("diagonals.interleaved.exact", Di, rbi, E, -1);

    // two-stage: [N_i | L_i] with own lower rows, and with ghost columns of lower ranks
    const int enc = kEncSortedTiles | kEncFreeOrder | kEncDict;
    plan("twostage.inner1", T, third, J, tF, 1, nullptr, enc);
    plan("twostage.inner2", T, third, J, tF, 2, nullptr, enc);
    Mat G = with_ghosts(T, 6);
    const int gcls[6] = {0, 1, -1, 1, 0, -1};
    plan("twostage.ghosts.inner1", G, third, J, tF, 1, gcls, enc);
    plan("twostage.ghosts.inner2", G, third, J, tF, 2, gcls, kEncFreeOrder);
    plan("ghosts.exact", G, third, E, tF, 0, gcls, enc);

    // natural order, both directions, on the whole matrix and on a sub-range
    natural("natural.band.all", B, 0, 900);
    natural("natural.band.sub", B, 123, 777);
    natural("natural.7pt.sub", Pi, 100, 1500);
    natural("natural.diagonals.sub", Di, 0, 300);
    natural("natural.empty", B, 50, 50);

    // an infinity among the values
    Mat I = R;
    I.v[I.rp[700] + 2] = INFINITY;
    plan("infinity.jacobi", I, rb, J, nF);
    plan("infinity.exact", I, rb, E, nF);

    // every switch at 0 once, where it decides something
    struct { const char *name; Mat *m; const std::vector<int> *mark; int kind, split; } sw[] = {
        {"SSS_HIP_TILE_DIAG", &R, &rb, E, nF},  {"SSS_HIP_FUSE_RESID", &R, &rb, E, nF}, {"SSS_HIP_PEND_F", &R, &rb, E, nF},
        {"SSS_HIP_DEAD_PROLONG", &R, &rb, E, nF}, {"SSS_HIP_GS_FUSED", &T, &third, E, tF}, {"SSS_HIP_NOCOPY", &R, &rb, J, nF},
        {"SSS_HIP_ZERO_FIRST", &R, &rb, J, nF}};
    for (auto &s : sw) {
        setenv(s.name, "0", 1);
        plan(std::string("switch.") + s.name, *s.m, *s.mark, s.kind, s.split);
        unsetenv(s.name);
    }
    return g_bad ? 1 : 0;
}
