// sss_formats.hip — host builders of the matrix storage formats (sss_formats.hpp; the formats
// themselves: struct DevCSR in sss_engine.hpp).  Pure host code on the worker pool: no HIP runtime call
// and no kernel, so every builder can be called and checked without a GPU (tools/formats_hash.cpp).
#include "sss_formats.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <type_traits>

namespace sss {

int build_row_blocks(const int *h_rp, int n, std::vector<int> &blk, int split)
{
    blk.clear();
    int r = 0;
    while (r < n) {
        blk.push_back(r);
        const int base = h_rp[r];
        const int lim = (split > r && split < n) ? split : n;   // never straddle the class split
        int e = r + 1;
        if (h_rp[e] - base <= kTileEntries) {
            while (e < lim && e - r < kBlock && h_rp[e + 1] - base <= kTileEntries) ++e;
        }
        r = e;
    }
    blk.push_back(n);
    return (int)blk.size() - 1;
}

int build_rows_blocks(int n, std::vector<int> &blk, int split)
{
    blk.clear();
    for (int r = 0; r < n;) {
        blk.push_back(r);
        const int lim = (split > r && split < n) ? split : n;
        r = std::min(lim, r + kBlock);
    }
    blk.push_back(n);
    return (int)blk.size() - 1;
}

int longest_row(const int *rp, int n)
{
    std::atomic<int> Lmax{0};
    parallel_chunks(n, 1 << 16, [&](int lo, int hi) {
        int L = 0;
        for (int r = lo; r < hi; ++r) L = std::max(L, rp[r + 1] - rp[r]);
        int cur = Lmax.load();
        while (L > cur && !Lmax.compare_exchange_weak(cur, L)) {}
    });
    return Lmax.load();
}

static inline unsigned long long bits_of(double d)
{
    unsigned long long u;
    std::memcpy(&u, &d, sizeof(u));
    return u;
}
static inline double double_of(unsigned long long u)
{
    double d;
    std::memcpy(&d, &u, sizeof(d));
    return d;
}

constexpr int log2_of(int x) { return x <= 1 ? 0 : 1 + log2_of(x / 2); }

// Distinct 64-bit patterns of one block (at most Cap), collected by open addressing over 4 Cap slots;
// rk[id] is the pattern's position in ascending order -- what sort + unique + lower_bound gives, at a
// hash probe per entry instead of a sort of the whole block.
template <int Cap>
struct HashDict {
    static constexpr int kSlots = 4 * Cap;
    static constexpr int kShift = 64 - log2_of(kSlots);   // the hash: the product's top bits
    static_assert((kSlots & (kSlots - 1)) == 0, "power of two");
    unsigned long long key[kSlots];
    short slot[kSlots];                 // -1: empty; else local id
    unsigned long long val[Cap];        // local id -> pattern (insertion order)
    unsigned short rk[Cap];             // local id -> rank
    int n = 0;
    void clear()
    {
        std::memset(slot, 0xff, sizeof(slot));
        n = 0;
    }
    int insert(unsigned long long u, int cap)   // local id, or -1 past cap distinct patterns
    {
        for (unsigned h = (unsigned)((u * 0x9E3779B97F4A7C15ull) >> kShift) & (kSlots - 1);; h = (h + 1) & (kSlots - 1)) {
            if (slot[h] < 0) {
                if (n >= cap) return -1;
                slot[h] = (short)n;
                key[h] = u;
                val[n] = u;
                return n++;
            }
            if (key[h] == u) return slot[h];
        }
    }
    // ranks + the patterns in ascending order as T (signed offsets, bit patterns; double: the values
    // in the order of their bit patterns)
    template <class T>
    void finish(std::vector<T> &sorted)
    {
        using K = std::conditional_t<std::is_same<T, double>::value, unsigned long long, T>;
        int ord[Cap];
        for (int t = 0; t < n; ++t) ord[t] = t;
        std::sort(ord, ord + n, [&](int a, int b) { return (K)val[a] < (K)val[b]; });
        sorted.resize((size_t)n);
        for (int t = 0; t < n; ++t) {
            rk[ord[t]] = (unsigned short)t;
            if constexpr (std::is_same<T, double>::value) sorted[t] = double_of(val[ord[t]]);
            else sorted[t] = (T)val[ord[t]];
        }
    }
};
using SmallDict = HashDict<256>;
using XellValues = HashDict<kXellValueCap>;

// Sorted tile segments of a blocking: a block's entries, or kTileEntries chunks of a long row
// (exactly the segments the tile kernels stage, sss_spmv_dev.hpp csr_block_rows).  Per block the
// columns are cut into two clusters at their widest gap; returns false when a cluster spans
// 2^kTileColBits columns or more (the matrix then keeps stored-order staging).  One sort of
// (column << 32 | position) keys per segment gives both the column order and, on ties, the
// stored order (a stable sort by column).
bool build_sorted_tiles(const SSS_MAT &h, const std::vector<int> &blk, SortedTiles &out)
{
    const int *rp = h.row_ptr, *ci = h.col_idx;
    const int nb = (int)blk.size() - 1;
    constexpr long long kSpan = kTileDiagMark;   // larger offsets mark diagonal entries
    out.pk.resize((size_t)h.num_nnzs);
    out.pv.resize((size_t)h.num_nnzs);
    out.pb.resize((size_t)std::max(nb, 1));
    std::atomic<int> ok{1};
    parallel_chunks(nb, 512, [&](int qlo, int qhi) {
        std::vector<unsigned long long> key, seg;
        std::vector<int> rowof;
        for (int q = qlo; q < qhi && ok; ++q) {
            const int a0 = rp[blk[q]], e0 = rp[blk[q + 1]];
            if (a0 == e0) {
                out.pb[q] = make_int2(0, 0);
                continue;
            }
            rowof.resize((size_t)(e0 - a0));   // entry position -> its row (one pass over the block)
            for (int r = blk[q]; r < blk[q + 1]; ++r)
                for (int k = rp[r]; k < rp[r + 1]; ++k) rowof[(size_t)(k - a0)] = r;
            key.resize((size_t)(e0 - a0));
            for (int k = a0; k < e0; ++k) key[(size_t)(k - a0)] = (unsigned long long)(unsigned)ci[k] << 32 | (unsigned)(k - a0);
            std::sort(key.begin(), key.end());
            auto col = [&](size_t t) { return (int)(key[t] >> 32); };
            const size_t m = key.size();
            size_t gap = 0;   // cut after col(gap)
            for (size_t t = 1; t < m; ++t)
                if (col(t) - col(t - 1) > col(gap + 1) - col(gap)) gap = t - 1;
            const int b0 = col(0), b1 = m > 1 ? col(gap + 1) : col(0);
            const int cut = b1;   // columns >= cut go to cluster 1
            if (m > 1 && ((long long)col(gap) - b0 >= kSpan || (long long)col(m - 1) - b1 >= kSpan)) {
                ok = 0;
                return;
            }
            out.pb[q] = make_int2(b0, b1);
            const int r0 = blk[q];
            for (int a = a0; a < e0; a += kTileEntries) {
                const int e = std::min(e0, a + kTileEntries);
                const unsigned long long *sk = key.data();
                if (e - a != e0 - a0) {   // a long row's chunk: its own column order
                    seg.resize((size_t)(e - a));
                    for (int k = a; k < e; ++k) seg[(size_t)(k - a)] = (unsigned long long)(unsigned)ci[k] << 32 | (unsigned)(k - a0);
                    std::sort(seg.begin(), seg.end());
                    sk = seg.data();
                }
                for (int t = 0; t < e - a; ++t) {
                    const int k = a0 + (int)(unsigned)sk[t], c = ci[k];
                    const int r = rowof[(size_t)(k - a0)];   // the entry's row
                    const unsigned cl = (m > 1 && c >= cut) ? 1u : 0u;
                    const unsigned off = c == r ? kTileDiagMark + (unsigned)(r - r0) : (unsigned)(c - (cl ? b1 : b0));
                    out.pk[(size_t)a + t] = (cl << 31) | (off << kTileShift) | (unsigned)(k - a);
                    out.pv[(size_t)a + t] = h.val[k];
                }
            }
        }
    });
    return ok != 0;
}

// Rows of a free-order (tree-summed) matrix, stored column-sorted within each segment.
void sort_row_segments(const SSS_MAT &h, const int *seg, SortedRows &out)
{
    const int n = h.num_rows;
    const int *rp = h.row_ptr;
    out.ci.resize((size_t)h.num_nnzs);
    out.v.resize((size_t)h.num_nnzs);
    parallel_chunks(n, 256, [&](int rlo, int rhi) {
        std::vector<unsigned long long> key;   // column << 32 | position: a stable sort by column
        for (int r = rlo; r < rhi; ++r) {
            const int cut[3] = {rp[r], seg ? seg[r] : rp[r + 1], rp[r + 1]};
            for (int part = 0; part < 2; ++part) {
                const int a = cut[part], e = cut[part + 1];
                key.resize((size_t)std::max(0, e - a));
                for (int t = 0; t < e - a; ++t) key[t] = (unsigned long long)(unsigned)h.col_idx[a + t] << 32 | (unsigned)t;
                std::sort(key.begin(), key.end());
                for (int t = 0; t < e - a; ++t) {
                    const int k = a + (int)(unsigned)key[t];
                    out.ci[(size_t)a + t] = h.col_idx[k], out.v[(size_t)a + t] = h.val[k];
                }
            }
        }
    });
}

// Merged row groups of a free-order matrix: group g = rows [gG, gG + G); its entries keep their CSR
// span [rp[gG], rp[gG + G]), sorted by (column, segment, row); segment 1 = [seg[r], rp[r+1]) of a
// two-segment row.
void build_merged(const SSS_MAT &h, const int *seg, int G, MergedGroups &out)
{
    const int n = h.num_rows, ng = (n + G - 1) / G;
    const int *rp = h.row_ptr, *ci = h.col_idx;
    out.gp.resize((size_t)ng + 1);
    out.mk.resize((size_t)h.num_nnzs);
    out.mv.resize((size_t)h.num_nnzs);
    parallel_chunks(ng, 64, [&](int glo, int ghi) {
        std::vector<std::pair<unsigned long long, int>> ent;   // ((col << 4 | seg << 3 | row), position)
        std::vector<unsigned long long> key;   // the same order as one integer: merged key << 24 | position
        for (int g = glo; g < ghi; ++g) {
            const int r0 = g * G, r1 = std::min(n, r0 + G);
            const int base = rp[r0], cnt = rp[r1] - base;
            if (cnt < (1 << 24)) {
                key.resize((size_t)cnt);
                for (int r = r0; r < r1; ++r)
                    for (int k = rp[r]; k < rp[r + 1]; ++k) {
                        const unsigned long long sg = (seg && k >= seg[r]) ? 1u : 0u;
                        key[(size_t)(k - base)] =
                            ((((unsigned long long)ci[k] << kMergeShift) | (sg << 3) | (unsigned)(r - r0)) << 24) |
                            (unsigned)(k - base);
                    }
                std::sort(key.begin(), key.end());
                out.gp[g] = base;
                for (int t = 0; t < cnt; ++t) {
                    out.mk[(size_t)base + t] = (unsigned)(key[t] >> 24);
                    out.mv[(size_t)base + t] = h.val[base + (int)(key[t] & 0xffffff)];
                }
                continue;
            }
            ent.clear();
            for (int r = r0; r < r1; ++r)
                for (int k = rp[r]; k < rp[r + 1]; ++k) {
                    const unsigned sg = (seg && k >= seg[r]) ? 1u : 0u;
                    ent.emplace_back(((unsigned long long)ci[k] << kMergeShift) | (sg << 3) | (unsigned)(r - r0), k);
                }
            std::sort(ent.begin(), ent.end());
            int pos = rp[r0];
            out.gp[g] = pos;
            for (const auto &e : ent) {
                out.mk[pos] = (unsigned)e.first;
                out.mv[pos] = h.val[e.second];
                ++pos;
            }
        }
    });
    out.gp[ng] = rp[n];
}

// Narrow keys of a merged copy (DevCSR::mg_k16 / mg_d / mg_ke).  Within a group the entries are
// sorted by column, so the 64 columns of a chunk lie close together, but for the chunk that crosses
// from a row's F-range columns to its C-range columns.  Per chunk: `split` is the first lane after
// the widest column gap (the lowest such lane on ties); one base if last - first < 2^13, else two
// bases cut at `split` if both halves span < 2^13, else the chunk is wide and its whole share (one
// wave's entries: the kernels branch once per wave, not per chunk) keeps 32-bit keys.
void merged_narrow(const unsigned *keys, long long nnz, const int *gp, int ng, bool two, int W, unsigned short *k16,
                   int *desc, std::vector<unsigned> &esc, long long cnt[5])
{
    constexpr int kSpan = 1 << kMergeDeltaBits;
    const long long nd = merged_desc_slots(nnz, ng, W);
    std::memset(desc, 0, sizeof(int) * 4 * (size_t)nd);
    std::vector<long long> eoff((size_t)ng * W + 1, 0);   // per share: its escaped keys (then their first position)
    std::mutex mu;
    for (int i = 0; i < 5; ++i) cnt[i] = 0;
    auto acc_of = [two](unsigned q) { return two ? ((q >> 1) & 4u) | (q & 3u) : q & 7u; };
    parallel_chunks(ng, 64, [&](int glo, int ghi) {
        long long c[5] = {};
        for (int g = glo; g < ghi; ++g) {
            const long long k0 = gp[g], len = gp[g + 1] - k0, per = (len + W - 1) / W;
            for (int part = 0; part < W; ++part) {
                const long long a = k0 + std::min(len, part * per), e = k0 + std::min(len, (part + 1) * per);
                if (a >= e) continue;
                const long long d0 = (a >> 6) + (long long)g * W + part;
                bool wide = false;
                for (long long kb = a, ch = 0; kb < e; kb += 64, ++ch) {
                    const int m = (int)std::min<long long>(64, e - kb);
                    int *d = desc + 4 * (d0 + ch);
                    const int first = (int)(keys[kb] >> kMergeShift), last = (int)(keys[kb + m - 1] >> kMergeShift);
                    int split = 64, gap = 0;
                    for (int l = 1; l < m; ++l) {
                        const int w = (int)(keys[kb + l] >> kMergeShift) - (int)(keys[kb + l - 1] >> kMergeShift);
                        if (w > gap) gap = w, split = l;
                    }
                    ++c[0];
                    int lo = first, hi = first, kind;
                    if (last - first < kSpan) {
                        kind = 1, split = 64;
                    } else {
                        hi = (int)(keys[kb + split] >> kMergeShift);
                        const int below = (int)(keys[kb + split - 1] >> kMergeShift) - first;
                        kind = (below < kSpan && last - hi < kSpan) ? 2 : 3;
                    }
                    ++c[kind];
                    if (kind == 3) {   // no narrow form: zero keys, the share escapes
                        wide = true;
                        d[0] = d[1] = 0, d[2] = 64, d[3] = -1;
                        for (int l = 0; l < m; ++l) k16[kb + l] = 0;
                        continue;
                    }
                    d[0] = lo, d[1] = hi, d[2] = split, d[3] = -1;
                    for (int l = 0; l < m; ++l) {
                        const unsigned q = keys[kb + l];
                        const unsigned delta = (q >> kMergeShift) - (unsigned)(l < split ? lo : hi);
                        k16[kb + l] = (unsigned short)(delta << 3 | acc_of(q));
                    }
                }
                if (wide) {
                    eoff[(size_t)g * W + part] = e - a;
                    c[4] += (e - a + 63) >> 6;
                }
            }
        }
        std::lock_guard<std::mutex> lk(mu);
        for (int i = 0; i < 5; ++i) cnt[i] += c[i];
    });
    long long run = 0;
    for (auto &x : eoff) {
        const long long l = x;
        x = run, run += l;
    }
    esc.resize((size_t)run);
    parallel_chunks(ng, 64, [&](int glo, int ghi) {
        for (int g = glo; g < ghi; ++g) {
            const long long k0 = gp[g], len = gp[g + 1] - k0, per = (len + W - 1) / W;
            for (int part = 0; part < W; ++part) {
                const size_t s = (size_t)g * W + part;
                if (eoff[s + 1] == eoff[s]) continue;
                const long long a = k0 + std::min(len, part * per), e = k0 + std::min(len, (part + 1) * per);
                const long long d0 = (a >> 6) + (long long)g * W + part;
                std::memcpy(esc.data() + eoff[s], keys + a, sizeof(unsigned) * (size_t)(e - a));
                for (long long kb = a, ch = 0; kb < e; kb += 64, ++ch) desc[4 * (d0 + ch) + 3] = (int)(eoff[s] + 64 * ch);
            }
        }
    });
}

// (tests: the narrowing without a GPU.  esc holds up to esc_cap keys -- nnz always suffices;
// *n_esc receives the count; desc: merged_desc_slots x 4 ints, *n_desc the slots)
extern "C" int sss_hip_merged_narrow(const unsigned *keys, long long nnz, const int *gp, int ng, int two, int W,
                                     unsigned short *k16, int *desc, long long desc_cap, long long *n_desc,
                                     unsigned *esc, long long esc_cap, long long *n_esc, long long *counts)
{
    if (!keys || !gp || ng < 0 || nnz < 0 || (W != 1 && W != 2 && W != 4) || !k16 || !desc || !n_desc || !n_esc || !counts)
        return ERROR_INPUT_PAR;
    if (nnz >= (1ll << 31) || gp[ng] != nnz) return ERROR_INPUT_PAR;
    const long long nd = merged_desc_slots(nnz, ng, W);
    *n_desc = nd;
    if (desc_cap < nd) return ERROR_INPUT_PAR;
    std::vector<unsigned> e;
    merged_narrow(keys, nnz, gp, ng, two != 0, W, k16, desc, e, counts);
    *n_esc = (long long)e.size();
    if ((long long)e.size() > esc_cap || (!e.empty() && !esc)) return ERROR_INPUT_PAR;
    if (!e.empty()) std::memcpy(esc, e.data(), sizeof(unsigned) * e.size());
    return 0;
}

// out.pd / dd / vd from every block's offsets bd (null: none, dd untouched) and value bit patterns bv
static void pack_dicts(const std::vector<std::vector<int>> *bd, const std::vector<std::vector<unsigned long long>> &bv,
                       BlockDicts &out)
{
    const size_t nb = bv.size();
    out.pd.resize(nb);
    size_t nd = 0, nv = 0;
    for (size_t q = 0; q < nb; ++q) {
        const size_t cd = bd ? (*bd)[q].size() : 0;
        out.pd[q] = make_int4((int)nd, (int)cd, (int)nv, (int)bv[q].size());
        nd += cd;
        nv += bv[q].size();
    }
    if (bd) out.dd.resize(std::max<size_t>(nd, 1));
    out.vd.resize(std::max<size_t>(nv, 1));
    for (size_t q = 0; q < nb; ++q) {
        if (bd) std::copy((*bd)[q].begin(), (*bd)[q].end(), out.dd.begin() + out.pd[q].x);
        for (size_t t = 0; t < bv[q].size(); ++t) out.vd[(size_t)out.pd[q].z + t] = double_of(bv[q][t]);
    }
}

// Dictionary tiles of a square matrix (DevCSR::dv_*): per block, the distinct column offsets
// col - row and the distinct value bit patterns, each at most 256 (false when a block has more);
// the codes of each staging segment (the block, or a kTileEntries chunk of a longer row) in
// column order.
bool build_dict_tiles(const SSS_MAT &h, const std::vector<int> &blk, DictTiles &out)
{
    HostBuf<unsigned> &code = out.code;
    const int *rp = h.row_ptr, *ci = h.col_idx;
    const double *v = h.val;
    const int nb = (int)blk.size() - 1;
    if (h.num_rows != h.num_cols || nb <= 0) return false;
    std::vector<std::vector<int>> bd(nb);
    std::vector<std::vector<unsigned long long>> bv(nb);
    code.resize((size_t)h.num_nnzs);
    std::atomic<int> ok{1};
    parallel_chunks(nb, 256, [&](int qlo, int qhi) {
        std::unique_ptr<SmallDict> Dd(new SmallDict()), Vd(new SmallDict());
        std::vector<unsigned long long> key;
        std::vector<int> rowof;
        std::vector<unsigned char> did, vid;   // entry -> local dictionary ids
        for (int q = qlo; q < qhi && ok; ++q) {
            const int a0 = rp[blk[q]], e0 = rp[blk[q + 1]];
            rowof.resize((size_t)(e0 - a0));
            did.resize((size_t)(e0 - a0));
            vid.resize((size_t)(e0 - a0));
            Dd->clear();
            Vd->clear();
            for (int r = blk[q]; r < blk[q + 1]; ++r)
                for (int k = rp[r]; k < rp[r + 1]; ++k) {
                    rowof[(size_t)(k - a0)] = r;
                    const int di = Dd->insert((unsigned long long)(long long)(ci[k] - r), 256);
                    const int vi = Vd->insert(bits_of(v[k]), 256);
                    if (di < 0 || vi < 0) {
                        ok = 0;
                        return;
                    }
                    did[(size_t)(k - a0)] = (unsigned char)di;
                    vid[(size_t)(k - a0)] = (unsigned char)vi;
                }
            std::vector<long long> ds;
            Dd->finish(ds);
            Vd->finish(bv[q]);
            bd[q].assign(ds.begin(), ds.end());
            for (int a = a0; a < e0; a += kTileEntries) {   // staging segments, column-sorted
                const int e = std::min(e0, a + kTileEntries);
                key.resize((size_t)(e - a));
                for (int k = a; k < e; ++k) key[(size_t)(k - a)] = (unsigned long long)(unsigned)ci[k] << 32 | (unsigned)(k - a);
                std::sort(key.begin(), key.end());
                for (int t = 0; t < e - a; ++t) {
                    const int k = a + (int)(unsigned)key[t];
                    const unsigned dix = Dd->rk[did[(size_t)(k - a0)]], vix = Vd->rk[vid[(size_t)(k - a0)]];
                    code[(size_t)a + t] = vix << (kTileShift + 8) | dix << kTileShift | (unsigned)(k - a);
                }
            }
        }
    });
    if (!ok) return false;
    pack_dicts(&bd, bv, out);
    return true;
}

// Value dictionaries over the sorted tiles' values pv (slot order): per block at most 256 distinct
// bit patterns (false when a block has more), vi = each slot's index; pd[block] = {0, 0, base, count}.
bool build_value_dict(const std::vector<int> &blk, const int *rp, const HostBuf<double> &pv, ValueDict &out)
{
    HostBuf<unsigned char> &vi = out.vi;
    const int nb = (int)blk.size() - 1;
    if (nb <= 0) return false;
    std::vector<std::vector<unsigned long long>> bv(nb);
    vi.resize(pv.size());
    std::atomic<int> ok{1};
    parallel_chunks(nb, 256, [&](int qlo, int qhi) {
        std::unique_ptr<SmallDict> Vd(new SmallDict());
        for (int q = qlo; q < qhi && ok; ++q) {
            const int a0 = rp[blk[q]], e0 = rp[blk[q + 1]];
            Vd->clear();
            for (int k = a0; k < e0; ++k) {
                const int id = Vd->insert(bits_of(pv[(size_t)k]), 256);
                if (id < 0) {
                    ok = 0;
                    return;
                }
                vi[(size_t)k] = (unsigned char)id;
            }
            Vd->finish(bv[q]);
            for (int k = a0; k < e0; ++k) vi[(size_t)k] = (unsigned char)Vd->rk[vi[(size_t)k]];
        }
    });
    if (!ok) return false;
    pack_dicts(nullptr, bv, out);
    return true;
}

// Dictionary ELL (DevCSR::dv_ell): every row at most 32 entries, every block at most 31 distinct
// column offsets and 8 distinct value bit patterns (false otherwise); width W = 8, 16 or 32 bytes
// per row, codes in stored order, 0xFF pads.  Rectangular matrices (a restriction) too: offsets
// col - row, no diagonal meaning; based: col - the row's first column (0 for an empty row).
bool build_ell(const SSS_MAT &h, const std::vector<int> &blk, bool based, EllFormat &out)
{
    int &W = out.W;
    const int *rp = h.row_ptr, *ci = h.col_idx;
    const double *v = h.val;
    const int n = h.num_rows, nb = (int)blk.size() - 1;
    out.base.clear();
    if (based) {
        out.base.resize((size_t)n);
        parallel_chunks(n, 1 << 16, [&](int lo, int hi) {
            for (int r = lo; r < hi; ++r) out.base[r] = rp[r] < rp[r + 1] ? ci[rp[r]] : 0;
        });
    }
    const int *base = based ? out.base.data() : nullptr;
    if (nb <= 0 || n <= 0) return false;
    const int L = longest_row(rp, n);
    if (L > 32) return false;
    W = L <= 8 ? 8 : L <= 16 ? 16 : 32;
    // per block at most 31 offsets and 8 values: fixed slots, compacted afterwards
    std::vector<int> bdf((size_t)nb * 31), nd_of(nb), nv_of(nb);
    std::vector<double> bvf((size_t)nb * 8);
    out.ell.resize((size_t)n * W);
    std::atomic<int> ok{1};
    parallel_chunks(nb, 256, [&](int qlo, int qhi) {
        std::unique_ptr<SmallDict> Dd(new SmallDict()), Vd(new SmallDict());
        std::vector<long long> ds;
        std::vector<unsigned long long> vs;
        for (int q = qlo; q < qhi && ok; ++q) {
            Dd->clear();
            Vd->clear();
            unsigned char *row0 = out.ell.data() + (size_t)blk[q] * W;
            std::memset(row0, 0xff, (size_t)(blk[q + 1] - blk[q]) * W);
            for (int r = blk[q]; r < blk[q + 1]; ++r)
                for (int k = rp[r]; k < rp[r + 1]; ++k) {
                    const int di = Dd->insert((unsigned long long)(long long)(ci[k] - (base ? base[r] : r)), 31);
                    const int vi = Vd->insert(bits_of(v[k]), 8);
                    if (di < 0 || vi < 0) {
                        ok = 0;
                        return;
                    }
                    out.ell[(size_t)r * W + (k - rp[r])] = (unsigned char)(vi << 5 | di);
                }
            Dd->finish(ds);
            Vd->finish(vs);
            nd_of[q] = (int)ds.size();
            nv_of[q] = (int)vs.size();
            std::copy(ds.begin(), ds.end(), bdf.begin() + (size_t)q * 31);
            for (size_t t = 0; t < vs.size(); ++t) bvf[(size_t)q * 8 + t] = double_of(vs[t]);
            for (int r = blk[q]; r < blk[q + 1]; ++r)
                for (int k = 0; k < rp[r + 1] - rp[r]; ++k) {
                    unsigned char &c = out.ell[(size_t)r * W + k];
                    c = (unsigned char)(Vd->rk[c >> 5] << 5 | Dd->rk[c & 31]);
                }
        }
    });
    if (!ok) return false;
    out.pd.resize((size_t)nb);
    size_t nd = 0, nv = 0;
    for (int q = 0; q < nb; ++q) {
        out.pd[q] = make_int4((int)nd, nd_of[q], (int)nv, nv_of[q]);
        nd += nd_of[q];
        nv += nv_of[q];
    }
    out.dd.resize(std::max<size_t>(nd, 1));
    out.vd.resize(std::max<size_t>(nv, 1));
    parallel_chunks(nb, 4096, [&](int qlo, int qhi) {
        for (int q = qlo; q < qhi; ++q) {
            std::copy(bdf.begin() + (size_t)q * 31, bdf.begin() + (size_t)q * 31 + nd_of[q], out.dd.begin() + out.pd[q].x);
            std::copy(bvf.begin() + (size_t)q * 8, bvf.begin() + (size_t)q * 8 + nv_of[q], out.vd.begin() + out.pd[q].z);
        }
    });
    return true;
}

// Column ELL of a square matrix (DevCSR::dv_xell) over blocks of 256 rows: W 32-bit codes per row
// (stored order, 0xFFFFFFFF pads), each block's distinct values (ascending) in vd at pd[q].z / .w.
// W = the longest row rounded up to 8, 16, 20, 24, 32 or 40.
int xell_width(int L) { return L <= 8 ? 8 : L <= 16 ? 16 : L <= 20 ? 20 : L <= 24 ? 24 : L <= 32 ? 32 : L <= 40 ? 40 : 0; }
// column bits of a code: the smallest S >= 23 with ncols < 2^S (so the all-ones pad is never a
// column), 0 past 28 (fewer than 16 value slots)
int xell_shift_for(int ncols)
{
    for (int S = 23; S <= 28; ++S)
        if ((long long)ncols < (1LL << S)) return S;
    return 0;
}
// Column ELL codes and blocking: the rows in chunks of 256 (cut at the class split); a chunk whose
// rows hold more distinct values than a code can index (2^(32 - S), at most kXellValueCap) is halved
// until its parts fit (false below 16 rows).  Blocks, their value dictionaries (ascending) and every
// row's W codes in stored order.
bool build_xell(const SSS_MAT &h, int split, int W, int S, XellFormat &out)
{
    const int vcap = std::min(kXellValueCap, 1 << (32 - S));
    const int *rp = h.row_ptr, *ci = h.col_idx;
    const double *v = h.val;
    std::vector<int> chunks;
    const int nc = build_rows_blocks(h.num_rows, chunks, split);
    out.codes.resize((size_t)h.num_rows * W);
    struct Part {
        int r0;
        std::vector<double> vals;
    };
    std::vector<std::vector<Part>> parts((size_t)nc);
    std::atomic<int> ok{1};
    parallel_chunks(nc, 64, [&](int clo, int chi) {
        std::unique_ptr<XellValues> D(new XellValues());
        // rows [r0, r1) as one block if their values fit, else halved
        std::function<bool(int, int, std::vector<Part> &)> fit = [&](int r0, int r1, std::vector<Part> &dst) -> bool {
            D->clear();
            bool fits = true;
            for (int k = rp[r0]; k < rp[r1] && fits; ++k) fits = D->insert(bits_of(v[k]), vcap) >= 0;
            if (!fits) {
                if (r1 - r0 <= 16) return false;
                const int mid = r0 + (r1 - r0) / 2;
                return fit(r0, mid, dst) && fit(mid, r1, dst);
            }
            Part p;
            p.r0 = r0;
            D->finish(p.vals);
            for (int r = r0; r < r1; ++r) {
                unsigned *row = out.codes.data() + (size_t)r * W;
                int s = 0;
                for (int k = rp[r]; k < rp[r + 1]; ++k, ++s)
                    row[s] = (unsigned)D->rk[D->insert(bits_of(v[k]), vcap)] << S | (unsigned)ci[k];
                for (; s < W; ++s) row[s] = 0xffffffffu;
            }
            dst.push_back(std::move(p));
            return true;
        };
        for (int c = clo; c < chi && ok; ++c)
            if (!fit(chunks[c], chunks[c + 1], parts[c])) ok = 0;
    });
    if (!ok) return false;
    out.blk.clear();
    out.pd.clear();
    out.vd.clear();
    for (int c = 0; c < nc; ++c)
        for (const Part &p : parts[c]) {
            out.blk.push_back(p.r0);
            out.pd.push_back(make_int4(0, 0, (int)out.vd.size(), (int)p.vals.size()));
            out.vd.insert(out.vd.end(), p.vals.begin(), p.vals.end());
        }
    out.blk.push_back(h.num_rows);
    if (out.vd.empty()) out.vd.push_back(0.0);
    return true;
}

}  // namespace sss
