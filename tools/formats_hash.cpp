// One 64-bit hash per output array of every host format builder (amg_amd/csrc/sss_formats.hip), on
// small matrices chosen to reach every branch.  No GPU: the unit is included textually, the worker
// pool is replaced by inline execution and no HIP call is made.
//
//   hipcc -O2 -std=c++17 -x hip --offload-arch=gfx950 -ffp-contract=off -Iamg_amd/csrc \
//       tools/formats_hash.cpp -o tools/formats_hash && tools/formats_hash > hashes.txt
//
// Two builds of the builders produce the same bytes iff the two lists are identical.  To compare with
// a commit from before the builders had a unit of their own, add -DFORMATS_PARENT and point -I at
// that commit's amg_amd/csrc: the same main then runs against its sss_spmv.hip through the adapters
// below.  (-Xarch_host -fsanitize=address,undefined works on this stand-alone program.)
#ifdef FORMATS_PARENT
#include "sss_spmv.hip"
namespace sss {
bool device_builders_on() { return false; }
int merged_build_device(DevCSR &, const int *) { return ERROR_MISC; }
int sort_rows_device(DevCSR &, const int *) { return ERROR_MISC; }
// the result structs and signatures of sss_formats.hpp over the old reference-parameter builders
struct BlockDicts {
    std::vector<int4> pd;
    std::vector<int> dd;
    std::vector<double> vd;
};
struct SortedTiles { HostBuf<unsigned> pk; HostBuf<double> pv; std::vector<int2> pb; };
struct SortedRows { HostBuf<int> ci; HostBuf<double> v; };
struct MergedGroups { std::vector<int> gp; HostBuf<unsigned> mk; HostBuf<double> mv; };
struct DictTiles : BlockDicts { HostBuf<unsigned> code; };
struct ValueDict : BlockDicts { HostBuf<unsigned char> vi; };
struct EllFormat : BlockDicts { HostBuf<unsigned char> ell; int W = 0; std::vector<int> base; };
struct XellFormat : BlockDicts { std::vector<int> blk; HostBuf<unsigned> codes; };
static bool build_sorted_tiles(const SSS_MAT &h, const std::vector<int> &blk, SortedTiles &o)
{
    return build_sorted_tiles(h, blk, o.pk, o.pv, o.pb);
}
static void sort_row_segments(const SSS_MAT &h, const int *seg, SortedRows &o) { sort_row_segments(h, seg, o.ci, o.v); }
static void build_merged(const SSS_MAT &h, const int *seg, int G, MergedGroups &o) { build_merged(h, seg, G, o.gp, o.mk, o.mv); }
static bool build_dict_tiles(const SSS_MAT &h, const std::vector<int> &blk, DictTiles &o)
{
    return build_dict_tiles(h, blk, o.code, o.pd, o.dd, o.vd);
}
static bool build_value_dict(const std::vector<int> &blk, const int *rp, const HostBuf<double> &pv, ValueDict &o)
{
    return build_value_dict(blk, rp, pv, o.vi, o.pd, o.vd);
}
static bool build_ell(const SSS_MAT &h, const std::vector<int> &blk, bool based, EllFormat &o)
{
    o.base.clear();
    if (based) {   // as devcsr_upload computed them
        o.base.resize((size_t)h.num_rows);
        for (int r = 0; r < h.num_rows; ++r) o.base[r] = h.row_ptr[r] < h.row_ptr[r + 1] ? h.col_idx[h.row_ptr[r]] : 0;
    }
    return build_ell(h, blk, o.ell, o.W, o.pd, o.dd, o.vd, based ? o.base.data() : nullptr);
}
static bool build_xell(const SSS_MAT &h, int split, int W, int S, XellFormat &o)
{
    return build_xell(h, split, W, S, o.blk, o.codes, o.pd, o.vd);
}
}   // namespace sss
#else
#include "sss_formats.hip"
namespace sss {
int host_pool_threads() { return 1; }   // parallel_chunks runs inline
bool host_pool_run(const std::function<void()> &) { return false; }
}   // namespace sss
#endif
extern "C" void sss_huge_hint(void *, size_t) {}

#include <cstdint>
#include <cstdio>
#include <string>

using namespace sss;

static void put(const std::string &name, const void *p, size_t bytes)
{
    uint64_t h = 1469598103934665603ull;   // FNV-1a
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    printf("%-40s %016llx %zu\n", name.c_str(), (unsigned long long)h, bytes);
}
template <class T>
static void put(const std::string &name, const std::vector<T> &v) { put(name, v.data(), sizeof(T) * v.size()); }
template <class T>
static void put(const std::string &name, const HostBuf<T> &v) { put(name, v.data(), sizeof(T) * v.size()); }
static void put(const std::string &name, long long x) { put(name, &x, sizeof(x)); }

struct Mat {
    std::vector<int> rp{0}, ci;
    std::vector<double> v;
    int ncols = 0;
    void add(int c, double a) { ci.push_back(c), v.push_back(a); }
    void end_row() { rp.push_back((int)ci.size()); }
    SSS_MAT mat()
    {
        SSS_MAT m;
        m.num_rows = (int)rp.size() - 1, m.num_cols = ncols, m.num_nnzs = (int)ci.size();
        m.row_ptr = rp.data(), m.col_idx = ci.data(), m.val = v.data();
        return m;
    }
    std::vector<int> halves()   // a split position inside every row (two-segment rows)
    {
        std::vector<int> s(rp.size() - 1);
        for (size_t r = 0; r + 1 < rp.size(); ++r) s[r] = rp[r] + (rp[r + 1] - rp[r]) / 2;
        return s;
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
                m.add(i, 6.0);
                if (x < N - 1) m.add(i + 1, -1.0);
                if (y < N - 1) m.add(i + N, -1.0);
                if (z < N - 1) m.add(i + N * N, -1.0);
                m.end_row();
            }
    return m;
}
// 19 entries per row (fewer at the ends), 8 distinct values
static Mat banded(int n)
{
    Mat m;
    m.ncols = n;
    for (int i = 0; i < n; ++i) {
        for (int d = -9; d <= 9; ++d)
            if (i + d >= 0 && i + d < n) m.add(i + d, d == 0 ? 20.0 : -0.25 * (1 + (d + 9) % 7));
        m.end_row();
    }
    return m;
}
// rows with a near, a middle and (every third row) a far column range, stored in rotated order
static Mat near_far(int n)
{
    Mat m;
    m.ncols = 1 << 21;
    for (int r = 0; r < n; ++r) {
        std::vector<int> c;
        for (int j = 0; j < 6; ++j) c.push_back(r + 3 * j);
        for (int j = 0; j < 6; ++j) c.push_back(700000 + 2 * r + 5 * j);
        if (r % 3 == 0)
            for (int j = 0; j < 6; ++j) c.push_back(1500000 + r + 7 * j);
        for (size_t j = 0; j < c.size(); ++j) {
            const size_t k = (j + r) % c.size();
            m.add(c[k], 1.0 + 0.001 * (double)((r * 7 + (int)k * 13) % 50));
        }
        m.end_row();
    }
    return m;
}
// three entries per row and one hub row of 2500
static Mat hub(int n)
{
    Mat m;
    m.ncols = n;
    for (int i = 0; i < n; ++i) {
        if (i == 1234) {
            for (int j = 0; j < 2500; ++j) m.add((j * 3 + 1) % n, j % 11 == 0 ? 2.0 : -0.5 - 0.125 * (j % 5));
        } else {
            if (i > 0) m.add(i - 1, -1.0);
            m.add(i, 2.0);
            if (i < n - 1) m.add(i + 1, -1.0);
        }
        m.end_row();
    }
    return m;
}
// 36 entries per row, three values of its own per row: 256 rows hold 768 distinct values
static Mat many_values(int n)
{
    Mat m;
    m.ncols = n;
    for (int r = 0; r < n; ++r) {
        for (int j = 0; j < 36; ++j) m.add((r + 5 * j) % n, 1.0 + r * 3 + j % 3);
        m.end_row();
    }
    return m;
}

static void dicts(const std::string &t, const BlockDicts &b)
{
    put(t + ".pd", b.pd), put(t + ".dd", b.dd), put(t + ".vd", b.vd);
}
static std::vector<int> blocks(const std::string &t, const SSS_MAT &h, int split)
{
    std::vector<int> blk;
    put(t + ".nblk", build_row_blocks(h.row_ptr, h.num_rows, blk, split));
    put(t + ".blk", blk);
    return blk;
}
static void ell(const std::string &t, const SSS_MAT &h, const std::vector<int> &blk, bool based)
{
    EllFormat f;
    const bool ok = build_ell(h, blk, based, f);
    put(t + ".ok", ok);
    if (!ok) return;
    put(t + ".W", f.W), put(t + ".ell", f.ell), put(t + ".base", f.base), dicts(t, f);
}
static void xell(const std::string &t, const SSS_MAT &h, int split, int W)
{
    XellFormat f;
    const int S = xell_shift_for(h.num_cols);
    const bool ok = W > 0 && S > 0 && build_xell(h, split, W, S, f);
    put(t + ".W_S_ok", W * 10000 + S * 10 + ok);
    if (!ok) return;
    put(t + ".blk", f.blk), put(t + ".codes", f.codes), dicts(t, f);
}
static void tiles(const std::string &t, const SSS_MAT &h, const std::vector<int> &blk)
{
    DictTiles d;
    const bool dok = build_dict_tiles(h, blk, d);
    put(t + ".dict.ok", dok);
    if (dok) put(t + ".dict.code", d.code), dicts(t + ".dict", d);
    SortedTiles s;
    const bool sok = build_sorted_tiles(h, blk, s);
    put(t + ".sorted.ok", sok);
    if (!sok) return;
    put(t + ".sorted.pk", s.pk), put(t + ".sorted.pv", s.pv), put(t + ".sorted.pb", s.pb);
    ValueDict v;
    const bool vok = build_value_dict(blk, h.row_ptr, s.pv, v);
    put(t + ".vdict.ok", vok);
    if (vok) put(t + ".vdict.vi", v.vi), dicts(t + ".vdict", v);
}
static void merged(const std::string &t0, const SSS_MAT &h, const int *seg)
{
    SortedRows s;
    sort_row_segments(h, seg, s);
    put(t0 + ".rows.ci", s.ci), put(t0 + ".rows.v", s.v);
    for (int G : {4, 8}) {
        const std::string t = t0 + ".G" + std::to_string(G);
        MergedGroups m;
        build_merged(h, seg, G, m);
        put(t + ".gp", m.gp), put(t + ".mk", m.mk), put(t + ".mv", m.mv);
        if (seg && G > 4) continue;   // three accumulator bits: never narrowed
        const int ng = (int)m.gp.size() - 1;
        for (int W : {1, 2, 4}) {
            const std::string u = t + ".W" + std::to_string(W);
            std::vector<unsigned short> k16((size_t)h.num_nnzs);
            std::vector<int> desc(4 * (size_t)merged_desc_slots(h.num_nnzs, ng, W));
            std::vector<unsigned> esc;
            long long cnt[5];
            merged_narrow(m.mk.data(), h.num_nnzs, m.gp.data(), ng, seg != nullptr, W, k16.data(), desc.data(), esc, cnt);
            put(u + ".k16", k16), put(u + ".desc", desc), put(u + ".esc", esc), put(u + ".cnt", cnt, sizeof(cnt));
            put(u + ".n_esc", (long long)esc.size());
        }
    }
}

int main()
{
    Mat A = poisson7(12), B = banded(3000), C = near_far(2048), D = hub(4000), E = many_values(2048);
    const SSS_MAT a = A.mat(), b = B.mat(), c = C.mat(), d = D.mat(), e = E.mat();
    put("xell_width.7_19_2500", xell_width(7) * 1000000LL + xell_width(19) * 1000 + xell_width(2500));

    const std::vector<int> ablk = blocks("7pt", a, -1), asplit = blocks("7pt.split", a, 801);
    ell("7pt.ell", a, ablk, false), ell("7pt.split.ell", a, asplit, false), ell("7pt.ellbase", a, ablk, true);
    xell("7pt.xell8", a, -1, 8), xell("7pt.split.xell8", a, 801, 8);
    tiles("7pt", a, ablk), tiles("7pt.split", a, asplit);

    const std::vector<int> bblk = blocks("band", b, -1), bsplit = blocks("band.split", b, 1000);
    ell("band.ell", b, bblk, false), ell("band.ellbase", b, bsplit, true);
    xell("band.xell20", b, -1, 20), xell("band.split.xell20", b, 1000, 20);
    tiles("band", b, bblk);

    const std::vector<int> cblk = blocks("nearfar", c, 1024), cseg = C.halves();
    ell("nearfar.ell", c, cblk, false), ell("nearfar.ellbase", c, cblk, true);
    xell("nearfar.xell24", c, 1024, 24);
    tiles("nearfar", c, cblk);
    merged("nearfar.one", c, nullptr), merged("nearfar.two", c, cseg.data());

    const std::vector<int> dblk = blocks("hub", d, -1), dseg = D.halves();
    ell("hub.ell", d, dblk, false);
    tiles("hub", d, dblk);
    merged("hub.one", d, nullptr), merged("hub.two", d, dseg.data());

    const std::vector<int> eblk = blocks("values", e, -1);
    xell("values.xell40", e, -1, 40);   // every 256-row chunk is halved
    tiles("values", e, eblk);
    merged("band.one", b, nullptr);
    return 0;
}
