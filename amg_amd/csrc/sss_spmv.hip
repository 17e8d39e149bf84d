// sss_spmv.hip — CSR SpMV family for every level (gfx950, wave64, fp64, no contraction).
//
// Replaces SSS_blas_mv_amxpy / SSS_blas_mv_mxy (SSS_utils.c:161-201) and the coarse-grid
// spmv_kernel / alpha_spmv_kernel (Solve/SSS_cuda.cu:77-118, which launch <<<64,64>>> and
// re-upload the whole CSR per call).  Here the CSR lives in HBM for the whole solve.
//
// Kernel: CSR-adaptive.  At upload each matrix is cut into row blocks of <= 256 rows holding
// <= kTileEntries nonzeros.  A workgroup stages its block's val/col slice into LDS with
// coalesced loads (the slice is contiguous in CSR), then each thread walks ONE row from LDS
// and accumulates in stored CSR order starting from 0.0 — the reference's exact summation
// order, so results are bitwise identical to the host reference.  A row longer than the
// tile forms a block on its own: the workgroup computes the products a_k*x_{c_k} in parallel
// (identically rounded), stages them in LDS and one lane adds them in order (bitwise again).
//
// Roofline: HBM-bound, 12 B/nnz (fp64 value + int32 column) + 4 B/row (row_ptr) + 8 B/row
// per vector stream (x compulsory, y, b); no MFMA (≈0.13 flop/byte).
// The matrix upload (devcsr_upload) chooses and stores the formats the kernels read; their host
// builders are in sss_formats.hip, the worker pool and the host -> device copy in sss_host.hip.
#include "sss_engine.hpp"
#include "sss_formats.hpp"

#include <cstdlib>
#include "sss_spmv_dev.hpp"

#include <algorithm>
#include <type_traits>

namespace sss {

static_assert(kXellValueCap == kXellValues, "the column ELL builder's value cap is the kernels'");

// Every switch an upload reads, from the environment at each call: the tests flip them between
// uploads in one process, so nothing here may be cached.
UploadSwitches upload_switches()
{
    auto off = [](const char *name) {   // "0...": off; unset or anything else: on
        const char *e = getenv(name);
        return e && *e == '0';
    };
    auto num = [](const char *name, int unset) {
        const char *e = getenv(name);
        return (e && *e) ? atoi(e) : unset;
    };
    UploadSwitches s;
    s.dict = !off("SSS_HIP_DICT");             // 0: no dictionary format (tests compare both ways)
    s.ell = !off("SSS_HIP_ELL");               // 0: no dictionary ELL (dictionary tiles where they qualify)
    s.ell_base = !off("SSS_HIP_ELL_BASE");     // 0: no per-row-based dictionary ELL for R
    s.xell = !off("SSS_HIP_XELL");             // 0: no column ELL
    // 0: 32-bit merged keys.  Default 1, measured on 7-pt 400^3 against the previous commit's library, four
    // runs each alternating in one job (profiles/merged_key16/): 18.27-18.34 -> 17.90-18.00 ms per step
    s.key16 = !off("SSS_HIP_MERGE_KEY16");
    s.gpu_build = !off("SSS_HIP_GPU_BUILD");   // 0: the host builders (tests compare both)
    const char *g = getenv("SSS_HIP_MERGE_G");
    s.merge_g = (g && *g) ? (atoi(g) <= 0 ? 0 : atoi(g) >= 8 ? 8 : 4) : -1;   // kernel instances: 4 and 8
    s.merge_min_rows = num("SSS_HIP_MERGE_MIN_ROWS", 2000);
    // waves per group: 4 (fewer -- longer waves over shorter groups -- measured no better on
    // 7-pt 400^3: levels 5-10 6.6 ms per V-cycle with W = 1/2 by group size, 6.5 ms with 4)
    const int w = num("SSS_HIP_MERGE_W", 4);
    s.merge_w = w >= 4 ? 4 : w >= 2 ? 2 : 1;
    // Where the lanes of the merged-group kernels keep their accumulators (DevCSR::mg_acc): 0 registers,
    // 1 LDS (merged_sums_lds).  SSS_HIP_MERGE_ACC forces one form; unset, LDS: for every (G, two
    // segments) pair the cycle selects, measured on 7-pt 400^3 against the previous commit's library
    // (profiles/merged_acc/prof_shapes_*.txt, kernel time summed over the six traced cycles): G = 4 two
    // segments (ts_stage0<4>) 22.39 -> 20.75 ms over its 12 launch shapes, G = 4 one segment
    // (ts_inner<4>, spmv_merged<.,.,4>) 8.60 -> 8.03 ms, G = 8 one segment (spmv_merged<.,.,8>)
    // 2.31 -> 2.17 ms.  Two shapes of ts_stage0<4> with the shortest per-wave shares (~180 entries:
    // 17,164 and 25,478 workgroups) are 2-4 % slower in LDS, the ten others 5-24 % faster.
    // G = 8 with two segments is instantiated but never selected (devcsr_upload caps those at G = 4);
    // its LDS form holds 32.5 KB per workgroup, 4 waves per SIMD against the register form's 5.
    const char *a = getenv("SSS_HIP_MERGE_ACC");
    s.merge_acc = (a && *a) ? *a != '0' : 1;
    // average entries per row from which a matrix takes the wave-per-row kernels, and the free-order
    // threshold (the tests use the overrides to cover both paths)
    s.wave_min = num("SSS_HIP_WAVE_MIN", kWaveRowMin);
    s.free_min = num("SSS_HIP_FREE_MIN", kFreeRowMin);
    return s;
}
int wave_row_min() { return upload_switches().wave_min; }
int free_row_min() { return upload_switches().free_min; }
bool merge_key16_on() { return upload_switches().key16; }
bool device_builders_on() { return upload_switches().gpu_build; }

// Rows per merged group for a free-order matrix of n rows (0: wave-per-row kernels).  Measured on
// 7-pt 400^3 (tools/lab_rows.hip, residual, one wave per group): G = 8 from ~100K rows (level 6:
// 204 vs 311 us), G = 4 below (levels 7-9: 1.1-1.4x).  With one workgroup per group (4 waves split
// the entries) small matrices gain too: from 2,000 rows the V-cycle's levels 9-10 took 0.97 ms
// against 1.09 ms with 12,000 (tools/gpu/prof.sh).  SSS_HIP_MERGE_G / _MIN_ROWS override (tests).
static int merge_group_size(int n, const UploadSwitches &sw)
{
    if (n < sw.merge_min_rows) return 0;
    if (sw.merge_g >= 0) return sw.merge_g;
    return n >= 80000 ? 8 : 4;
}

// {first row, first entry} of every block, so a block's bounds are one independent load.
int upload_block_bounds(int2 **dst, const std::vector<int> &blk, const int *h_rp, const int2 **host)
{
    std::vector<int2> bk(blk.size());
    for (size_t q = 0; q < blk.size(); ++q) bk[q] = make_int2(blk[q], h_rp[blk[q]]);
    if (int rc = dev_upload(*dst, bk, "hipMalloc(bk)")) return rc;
    if (host) {
        delete[] *host;
        int2 *c = new int2[bk.size()];
        std::copy(bk.begin(), bk.end(), c);
        *host = c;
    }
    return 0;
}

thread_local ByteLedger *g_ledger = nullptr;

double matrix_bytes(const DevCSR &A, int blo, int bhi)
{
    if (bhi <= blo || A.n == 0) return 0.0;
    if (!A.h_bk || A.nblk == 0 || (blo == 0 && bhi >= A.nblk)) return (double)A.stream_bytes;
    const bool by_rows = A.dv_ell || A.dv_xell || A.nnz == 0;
    const double part = by_rows ? (double)(A.h_bk[bhi].x - A.h_bk[blo].x) / A.n
                                : (double)(A.h_bk[bhi].y - A.h_bk[blo].y) / A.nnz;
    return part * (double)A.stream_bytes;
}

double matrix_bytes_rows(const DevCSR &A, int lo, int hi)
{
    if (hi <= lo || A.n == 0) return 0.0;
    if (!A.h_bk || A.nblk == 0) return (double)A.stream_bytes * (hi - lo) / A.n;
    auto blk_of = [&](int r) {   // first block starting at or after row r
        int a = 0, b = A.nblk;
        while (a < b) {
            const int m = (a + b) / 2;
            if (A.h_bk[m].x < r) a = m + 1;
            else b = m;
        }
        return a;
    };
    return matrix_bytes(A, blk_of(lo), blk_of(hi));
}

DevDict devdict(const DevCSR &A, int blo)
{
    DevDict t;
    t.tree_long = A.tree_long ? 1 : 0;
    if (!has_dict(A)) return t;
    t.code = A.dv_code;
    t.ell = A.dv_ell;
    t.ellb = A.dv_ell_base;
    t.ellw = A.ell_w;
    t.xell = A.dv_xell;
    t.xshift = A.xell_shift;
    t.pd = A.dv_pd + blo;
    t.dd = A.dv_dd;
    t.vd = A.dv_vd;
    if (A.dv_vi) {
        t.pk = A.pk;
        t.vi = A.dv_vi;
        t.pb = A.pb + blo;
    }
    return t;
}

// d's merged copy (mg_G, mg_ng, mg_W, mg_two set) with narrow keys from its sorted 32-bit keys and
// group bounds on the host
static int merged_upload_narrow(DevCSR &d, const unsigned *hk, const int *hgp)
{
    const long long nd = merged_desc_slots(d.nnz, d.mg_ng, d.mg_W);
    HostBuf<unsigned short> k16;
    HostBuf<int> desc;
    std::vector<unsigned> esc;
    k16.resize((size_t)d.nnz);
    desc.resize(4 * (size_t)nd);
    merged_narrow(hk, d.nnz, hgp, d.mg_ng, d.mg_two, d.mg_W, k16.data(), desc.data(), esc, d.mg_cnt);
    d.mg_nd = nd, d.mg_ne = (long long)esc.size();
    const char *what = "hipMalloc(merged)";
    if (int rc = dev_upload(d.mg_k16, k16.data(), (size_t)d.nnz, what)) return rc;
    if (int rc = dev_upload(d.mg_d, reinterpret_cast<const int4 *>(desc.data()), (size_t)nd, what)) return rc;
    return dev_upload(d.mg_ke, esc, what);
}

// d.ci / d.v <- h's rows, each (segment) column-sorted on the host
static int upload_sorted_rows(DevCSR &d, const SSS_MAT &h, const int *seg)
{
    SortedRows s;
    sort_row_segments(h, seg, s);
    if (int rc = h2d(d.ci, s.ci.data(), sizeof(int) * (size_t)d.nnz)) return rc;
    if (int rc = h2d(d.v, s.v.data(), sizeof(double) * (size_t)d.nnz)) return rc;
    d.rows_sorted = true;
    return 0;
}

namespace {
// One devcsr_upload call: its arguments and switches, the current row blocking, and one step per
// format -- "qualifies? build, upload, set d's fields" -- in the order devcsr_upload tries them.
struct Upload {
    DevCSR &d;
    const SSS_MAT &h;
    const int split, enc;
    const int *const seg;
    const UploadSwitches sw;
    std::vector<int> blk;
    long long dict_bytes = 0;   // the stored format's block dictionaries (stream_bytes)

    // the tile path: every format below the merged copy is for these matrices only
    bool tile_rows() const { return !d.wave_rows && !d.vec_rows && d.nnz > 0; }
    // free-order rows are read column-sorted by the wave-tree kernels; a two-stage split copy
    // with a merged copy (kEncMergedOnly) is read only through that (launch_ts_*): stored order
    bool wants_sorted_rows() const { return d.vec_rows && !((enc & kEncMergedOnly) && d.mg_G > 0); }

    int csr(PhaseTimer &pt)
    {
        d.rp = dev_alloc<int>((size_t)d.n + 1);
        d.ci = dev_alloc<int>((size_t)d.nnz);
        d.v = dev_alloc<double>((size_t)d.nnz);
        if (!d.rp || !d.ci || !d.v) return hip_fail(hipErrorOutOfMemory, "hipMalloc(CSR)", __FILE__, __LINE__);
        pt.mark("alloc");
        if (int rc = h2d(d.rp, h.row_ptr, sizeof(int) * ((size_t)d.n + 1))) return rc;
        if (d.nnz > 0 && wants_sorted_rows() && !sw.gpu_build) return upload_sorted_rows(d, h, seg);
        if (int rc = h2d(d.ci, h.col_idx, sizeof(int) * (size_t)d.nnz)) return rc;
        return h2d(d.v, h.val, sizeof(double) * (size_t)d.nnz);
    }

    // d's blocking <- blk (the CSR-adaptive blocks, later perhaps the column ELL's)
    int blocks()
    {
        dev_free(d.blk);
        dev_free(d.bk);
        d.blk = nullptr, d.bk = nullptr;
        d.nblk = (int)blk.size() - 1;
        d.split_blk = d.nblk;
        if (split >= 0)   // the block that starts at the class split
            for (int q = 0; q <= d.nblk; ++q)
                if (blk[q] >= split) { d.split_blk = q; break; }
        d.ngrid = (d.wave_rows || d.vec_rows) ? (d.n + 3) / 4 : d.nblk;
        if (int rc = dev_upload(d.blk, blk, "hipMalloc(blk)")) return rc;
        return upload_block_bounds(&d.bk, blk, h.row_ptr, &d.h_bk);
    }

    // merged row groups of a free-order matrix: device builder (from the stored-order CSR just
    // uploaded) or host builder, then narrow keys where they apply
    int merged()
    {
        if (d.mg_G > 0) {
            d.mg_two = seg != nullptr;
            d.mg_W = sw.merge_w;
            d.mg_acc = sw.merge_acc;
            if (sw.gpu_build) {
                if (int rc = merged_build_device(d, seg)) return rc;
            } else {
                MergedGroups m;
                build_merged(h, seg, d.mg_G, m);
                d.mg_ng = (int)m.gp.size() - 1;
                const char *what = "hipMalloc(merged)";
                if (int rc = dev_upload(d.mg_gp, m.gp, what)) return rc;
                if (merged_key16_ok(d)) {
                    if (int rc = merged_upload_narrow(d, m.mk.data(), m.gp.data())) return rc;
                } else if (int rc = dev_upload(d.mg_k, m.mk, what)) {
                    return rc;
                }
                if (int rc = dev_upload(d.mg_v, m.mv, what)) return rc;
            }
            d.ngrid = (d.mg_ng + 4 / d.mg_W - 1) / (4 / d.mg_W);
        }
        // (after the merged build, which reads the stored order)
        if (wants_sorted_rows() && sw.gpu_build && d.nnz > 0) return sort_rows_device(d, seg);
        return 0;
    }

    int upload_dicts(const BlockDicts &b, bool with_dd, const char *what)
    {
        if (int rc = dev_upload(d.dv_pd, b.pd, what)) return rc;
        if (with_dd)
            if (int rc = dev_upload(d.dv_dd, b.dd, what)) return rc;
        dict_bytes = b.bytes();
        return dev_upload(d.dv_vd, b.vd, what);
    }

    // dictionary ELL first (one thread per row), else dictionary tiles (the tile kernels then stage
    // from them instead of the sorted copy)
    int ell()
    {
        const bool based = (enc & kEncEllBase) && d.n != d.ncols;
        if (!((enc & (kEncDict | kEncEll | kEncEllBase)) && sw.dict && sw.ell && tile_rows() &&
              ((enc & kEncEll) || based || d.n == d.ncols)))
            return 0;
        EllFormat f;
        if (!build_ell(h, blk, based, f)) return 0;
        if (based)
            if (int rc = dev_upload(d.dv_ell_base, f.base, "hipMalloc(ELL bases)")) return rc;
        d.ell_w = f.W;
        if (int rc = dev_upload(d.dv_ell, f.ell, "hipMalloc(dictionary ELL)")) return rc;
        return upload_dicts(f, true, "hipMalloc(dictionary ELL)");
    }

    // column ELL where the 1-byte dictionary did not fit: its own 256-row blocking replaces the
    // CSR-adaptive one (no tile staging, so no entry limit per block)
    int xell()
    {
        const int xshift = xell_shift_for(d.ncols);
        if (!((enc & kEncXell) && sw.dict && sw.xell && !d.dv_ell && tile_rows() && xshift > 0)) return 0;
        // rows padded to W: not where that makes the codes larger than the CSR entries (4 W bytes
        // per row against 12 per entry: at least W / 3 entries per row on average; 7-pt level-1
        // prolongation, 3.2 entries in 8 slots: 362 -> 294 us per V-cycle)
        int W = xell_width(longest_row(h.row_ptr, d.n));
        if ((long long)d.nnz * 3 < (long long)W * d.n) W = 0;
        // 40-slot rows only where no range relaxation reads them (two-stage levels' matrices and split
        // copies): the relaxation kernels spill at that width
        if (W == 40 && !(enc & kEncMergedOnly)) W = 0;
        XellFormat f;
        if (W <= 0 || !build_xell(h, split, W, xshift, f)) return 0;
        blk.swap(f.blk);
        if (int rc = blocks()) return rc;
        d.xell_w = W;
        d.xell_shift = xshift;
        if (int rc = dev_upload(d.dv_xell, f.codes, "hipMalloc(column ELL)")) return rc;
        return upload_dicts(f, false, "hipMalloc(column ELL)");
    }

    int dict_tiles()
    {
        if (!((enc & kEncDict) && sw.dict && !d.dv_ell && !d.dv_xell && tile_rows())) return 0;
        DictTiles f;
        if (!build_dict_tiles(h, blk, f)) return 0;
        if (int rc = dev_upload(d.dv_code, f.code, "hipMalloc(dictionary tiles)")) return rc;
        return upload_dicts(f, true, "hipMalloc(dictionary tiles)");
    }

    // column-sorted tiles, their values through per-block dictionaries where those fit (the tile
    // kernels of a wave-path matrix never run on the hierarchy; no sorted copy for them)
    int sorted_tiles(PhaseTimer &pt)
    {
        SortedTiles t;
        if (!((enc & kEncSortedTiles) && !d.dv_code && !d.dv_ell && !d.dv_xell && tile_rows() &&
              build_sorted_tiles(h, blk, t)))
            return 0;
        if (int rc = dev_upload(d.pk, t.pk.data(), (size_t)d.nnz, "hipMalloc(sorted tiles)")) return rc;
        if (int rc = dev_upload(d.pb, t.pb, "hipMalloc(sorted tiles)")) return rc;
        pt.mark("sorted");
        ValueDict f;
        if ((enc & kEncDict) && sw.dict && build_value_dict(blk, h.row_ptr, t.pv, f)) {
            if (int rc = dev_upload(d.dv_vi, f.vi, "hipMalloc(value dictionaries)")) return rc;
            return upload_dicts(f, false, "hipMalloc(value dictionaries)");
        }
        return dev_upload(d.pv, t.pv.data(), (size_t)d.nnz, "hipMalloc(sorted tiles)");
    }

    // what one SpMV over the stored format reads besides the vectors (reported for the roofline)
    long long stream_bytes() const
    {
        const long long nnz = d.nnz, nb = d.nblk, rows = d.n, dict = dict_bytes;
        long long b;
        if (has_dict(d))
            b = d.dv_xell ? 4LL * d.xell_w * rows + 8 * (nb + 1) + 16 * nb + dict
                : d.dv_ell ? (long long)(d.ell_w + (d.dv_ell_base ? 4 : 0)) * rows + 8 * (nb + 1) + 16 * nb + dict
                           : (d.dv_vi ? 5 * nnz + 8 * nb : 4 * nnz) + 4 * (rows + 1) + 8 * (nb + 1) + 16 * nb + dict;
        else if (d.pk)
            b = 12 * nnz + 4 * (rows + 1) + 8 * (nb + 1) + 8 * nb;
        else
            b = 12 * nnz + 4 * (rows + 1) + 8 * (nb + 1);
        // narrow merged keys: 2 B per entry, the descriptors and the escaped shares' 32-bit keys
        if (d.mg_k16) b += 2 * nnz + 16 * d.mg_nd + 4 * d.mg_ne - 4 * nnz;
        return b;
    }
};
}   // namespace

int devcsr_upload(DevCSR &d, const SSS_MAT &h, int split, int enc, const int *seg)
{
    PhaseTimer pt("devcsr");
    Upload u{d, h, split, enc, seg, upload_switches()};
    d.n = h.num_rows;
    d.ncols = h.num_cols;
    d.nnz = h.num_nnzs;
    d.wave_rows = d.n > 0 && (long long)d.nnz >= (long long)u.sw.wave_min * d.n;
    d.vec_rows = d.n > 0 && (enc & kEncFreeOrder) && (long long)d.nnz >= (long long)u.sw.free_min * d.n;
    d.tree_long = (enc & kEncFreeOrder) && !d.vec_rows;
    if (d.vec_rows && (unsigned long long)std::max(d.ncols, 1) < (1ull << (32 - kMergeShift))) {
        d.mg_G = merge_group_size(d.n, u.sw);
        if (seg && d.mg_G > 4) d.mg_G = 4;   // two segments: 2G accumulators per lane
    }
    d.split_row = split;
    if (int rc = u.csr(pt)) return rc;
    pt.mark("csr");
    build_row_blocks(h.row_ptr, d.n, u.blk, split);
    if (int rc = u.blocks()) return rc;
    pt.mark("blocks");
    if (int rc = u.merged()) return rc;
    pt.mark("merged");
    if (int rc = u.ell()) return rc;
    pt.mark("ell");
    if (int rc = u.xell()) return rc;
    pt.mark("xell");
    if (int rc = u.dict_tiles()) return rc;
    pt.mark("dict");
    if (int rc = u.sorted_tiles(pt)) return rc;
    pt.mark("tiles");
    d.stream_bytes = u.stream_bytes();
    return 0;
}

int devcsr_sort_rows(DevCSR &d, const SSS_MAT &h, const int *seg)
{
    if (!d.vec_rows || d.rows_sorted || d.nnz == 0) return 0;
    if (device_builders_on()) return sort_rows_device(d, seg);
    return upload_sorted_rows(d, h, seg);
}

void devcsr_free(DevCSR &d)
{
    for (void *p : {(void *)d.rp, (void *)d.ci, (void *)d.v, (void *)d.blk, (void *)d.bk, (void *)d.pk, (void *)d.pv,
                    (void *)d.pb, (void *)d.mg_gp, (void *)d.mg_k, (void *)d.mg_v, (void *)d.mg_k16, (void *)d.mg_d,
                    (void *)d.mg_ke, (void *)d.dv_code, (void *)d.dv_ell, (void *)d.dv_ell_base, (void *)d.dv_xell,
                    (void *)d.dv_vi, (void *)d.dv_pd, (void *)d.dv_dd, (void *)d.dv_vd})
        dev_free(p);
    delete[] d.h_bk;
    d = DevCSR();
}

// ---- kernel -------------------------------------------------------------------------------
// The epilogue of every SpMV kernel: y_r from the row's sum s (br = b_r, read by RESID only); returns
// the row's contribution to the norm, out^2 (NORM) or 0.
template <int OP, bool NORM>
__device__ __forceinline__ double spmv_row_out(int r, double s, double alpha, double br, double *__restrict__ y, int cap)
{
    double out;
    if constexpr (OP == SSS_HIP_SPMV_MXY) out = s;
    else if constexpr (OP == SSS_HIP_SPMV_AMXPY) out = y[r] + s * alpha;
    else if constexpr (OP == SSS_HIP_SPMV_RESID) out = br + s * alpha;
    else {
        if (cap > 0 && r >= cap) return 0.0;   // as-shipped <<<64,64>>> row cap
        out = y[r] + s;
    }
    y[r] = out;
    return NORM ? out * out : 0.0;
}
// ... with b_r read here (the ELL branches load it ahead of their barrier and pass it in)
template <int OP, bool NORM>
__device__ __forceinline__ double spmv_row_out(int r, double s, double alpha, const double *__restrict__ b,
                                               double *__restrict__ y, int cap)
{
    double br = 0.0;
    if constexpr (OP == SSS_HIP_SPMV_RESID) br = b[r];
    return spmv_row_out<OP, NORM>(r, s, alpha, br, y, cap);
}

template <int OP, bool NORM, int DICT = 0>   // DICT: with_tile_kind (8/16/32: dictionary ELL, that width)
__global__ __launch_bounds__(kBlock) void spmv_adaptive(const int2 *__restrict__ blk, const int *__restrict__ rp,
                                                        const int *__restrict__ ci, const double *__restrict__ v,
                                                        const double *__restrict__ x, const double *__restrict__ b,
                                                        double *__restrict__ y, double alpha, int cap,
                                                        double *__restrict__ partial, const unsigned *__restrict__ pk,
                                                        const double *__restrict__ pv, const int2 *__restrict__ pb,
                                                        DevDict dt = DevDict())
{
    if constexpr (DICT >= kXell) {   // column ELL rows of width DICT - kXell: one thread per row
        constexpr int W = DICT - kXell;
        __shared__ XellSmem es;
        const int bid = blockIdx.x;
        double br = 0.0;
        const bool valid = bid < dt.bend;
        const XellRow<W> row = xell_row_begin<W>(valid, blk, bid, dt.xell, dt.pd, dt.vd, es, [&](int r) {
            if constexpr (OP == SSS_HIP_SPMV_RESID) br = b[r];
        });
        const unsigned(&w)[W] = row.w;
        const int r = row.r;
        __syncthreads();
        double sq = 0.0;
        if (row.live) {
            double xv[W];
            int ds;
            unsigned dcode;
            const int len = xell_gather<W>(w, r, dt.xshift, [&](int c) -> double { return x[c]; }, xv, ds, dcode);
            sq = spmv_row_out<OP, NORM>(r, xell_sum_g<false>(0.0, w, xv, es, dt.xshift, 0, len), alpha, br, y, cap);
        }
        if (NORM && valid) {
            const double t = block_sum(sq, es.red);
            if (threadIdx.x == 0) partial[bid] = t;
        }
    } else if constexpr (DICT >= 8) {   // dictionary ELL rows of width DICT: one thread per row, its sum
        constexpr int W = DICT;   // from 0.0 in stored order; kEllRpt row blocks per workgroup
        constexpr int RPT = kEllRpt;
        __shared__ EllSmem es[RPT];
        const int g = (int)blockIdx.x;
        EllRow<W> row[RPT];
        double br[RPT];
        int rb[RPT];   // the row's offset base (its own index, or dt.ellb[r])
#pragma unroll
        for (int j = 0; j < RPT; ++j) {   // codes (and b) in flight across the dictionaries' barrier
            br[j] = 0.0;
            rb[j] = 0;
            row[j] = ell_row_begin<W>(blk, g * RPT + j, dt, es[j], [&](int r) {
                rb[j] = dt.ellb ? dt.ellb[r] : r;
                if constexpr (OP == SSS_HIP_SPMV_RESID) br[j] = b[r];
            });
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RPT; ++j) {
            double sq = 0.0;
            if (row[j].live) {
                double p[W];
                int ds;
                double dv;
                const int len = ell_decode<W>(row[j].w, rb[j], es[j], [&](int c) -> double { return x[c]; }, p, ds, dv);
                sq = spmv_row_out<OP, NORM>(row[j].r, ell_add(0.0, p, 0, len), alpha, br[j], y, cap);
            }
            if (NORM && row[j].valid) {
                const double t = block_sum(sq, es[j].red);
                if (threadIdx.x == 0) partial[g * RPT + j] = t;
            }
        }
    } else {
        __shared__ SpmvSmem sm;
        __shared__ std::conditional_t<DICT != 0, DictSmem, char> dsm;
        DictSmem *ds = nullptr;
        if constexpr (DICT != 0) ds = &dsm;
        const double sq = csr_block_rows(
            blk, rp, ci, v, x, sm, [&](int r, double s) -> double { return spmv_row_out<OP, NORM>(r, s, alpha, b, y, cap); },
            pk, pv, pb, &dt, ds);
        if (NORM) {
            const double t = block_sum(sq, sm.red);
            if (threadIdx.x == 0) partial[xcd_bid()] = t;
        }
    }
}

// Long rows: one wave per row.  TREE = false: lane 0 chains the products in stored order
// (bitwise); TREE = true: free-order tree sum (DevCSR::vec_rows).
template <int OP, bool NORM, bool TREE>
__global__ __launch_bounds__(kBlock) void spmv_wave(int n, const int *__restrict__ rp, const int *__restrict__ ci,
                                                    const double *__restrict__ v, const double *__restrict__ x,
                                                    const double *__restrict__ b, double *__restrict__ y, double alpha,
                                                    int cap, double *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) double strips[TREE ? 1 : 4][TREE ? 1 : kWaveStage];
    __shared__ double red[kBlock / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = xcd_bid() * 4 + wave;
    double sq = 0.0;
    if (r < n) {
        auto prod = [&](int c, double a) { return a * x[c]; };
        const double s = TREE ? wave_row_sum(rp[r], rp[r + 1], ci, v, prod)
                              : wave_row_chain<false>(rp[r], rp[r + 1], ci, v, prod, 0.0, strips[TREE ? 0 : wave]);
        if (lane == 0) sq = spmv_row_out<OP, NORM>(r, s, alpha, b, y, cap);
    }
    if (NORM) {
        const double t = block_sum(sq, red);
        if (threadIdx.x == 0) partial[xcd_bid()] = t;
    }
}

// Free order, merged row groups (DevCSR::mg_*): W waves per group of G rows (merged_block).
// (LDSACC: the lanes' accumulators in LDS, DevCSR::mg_acc)
// (K16: narrow keys, DevCSR::mg_k16)
template <int OP, bool NORM, int G, bool LDSACC = false, bool K16 = false>
__global__ __launch_bounds__(kBlock) void spmv_merged(int n, int ng, int W, const int *__restrict__ gp,
                                                      MergedKeys mk, const double *__restrict__ mv,
                                                      const double *__restrict__ x, const double *__restrict__ b,
                                                      double *__restrict__ y, double alpha, int cap,
                                                      double *__restrict__ partial)
{
    __shared__ double red[8 * G];
    __shared__ double nred[kBlock / 64];
    __shared__ double acc[LDSACC ? 4 * G * kMergeAccDoubles : 1];
    int g = 0, u = 0;
    double sr = 0.0, unused = 0.0, sq = 0.0;
    if (merged_block<G, 1, LDSACC, K16>(gp, ng, W, mk, mv, [&](int c) -> double { return x[c]; }, red, acc, g, u, sr,
                                        unused)) {
        const int r = g * G + u;
        if (r < n) sq = spmv_row_out<OP, NORM>(r, sr, alpha, b, y, cap);
    }
    if (NORM) {
        const double t = block_sum(sq, nred);
        if (threadIdx.x == 0) partial[xcd_bid()] = t;
    }
}

template <int OP, bool NORM>
static void launch_op(const DevCSR &A, double alpha, const double *x, const double *b, double *y, int cap,
                      double *partial, hipStream_t s)
{
    if (with_merged_kind(A, [&](auto G, auto ACC, auto K16) {
            hipLaunchKernelGGL((spmv_merged<OP, NORM, decltype(G)::value, decltype(ACC)::value, decltype(K16)::value>),
                               dim3(A.ngrid), dim3(kBlock), 0, s, A.n, A.mg_ng, A.mg_W, A.mg_gp, merged_keys_of(A), A.mg_v,
                               x, b, y, alpha, cap, partial);
        }))
        return;
    if (A.vec_rows)
        hipLaunchKernelGGL((spmv_wave<OP, NORM, true>), dim3(A.ngrid), dim3(kBlock), 0, s, A.n, A.rp, A.ci, A.v, x,
                           b, y, alpha, cap, partial);
    else if (A.wave_rows)
        hipLaunchKernelGGL((spmv_wave<OP, NORM, false>), dim3(A.ngrid), dim3(kBlock), 0, s, A.n, A.rp, A.ci, A.v, x,
                           b, y, alpha, cap, partial);
    else
        with_tile_kind(A, [&](auto K) {
            constexpr int KK = decltype(K)::value;
            DevDict dt = devdict(A, 0);
            dt.bend = A.nblk;
            const int grid = (A.nblk + rows_per_wg(KK) - 1) / rows_per_wg(KK);
            hipLaunchKernelGGL((spmv_adaptive<OP, NORM, KK>), dim3(grid), dim3(kBlock), 0, s, A.bk, A.rp, A.ci, A.v, x,
                               b, y, alpha, cap, partial, A.pk, A.pv, A.pb, dt);
        });
}

// ledger: row vectors an SpMV op streams besides the gathered x (MXY writes y; the others read b or y
// and write y)
static double spmv_row_bytes(int op) { return op == SSS_HIP_SPMV_MXY ? 8.0 : 16.0; }

// f(std::integral_constant<int, OP>, std::bool_constant<NORM>) for a run-time op; NORM (per-block sums
// of squares into `partial`) exists for RESID only.  False, f not called, for an unknown op.
template <class F>
static bool with_spmv_op(int op, bool partial, F f)
{
    switch (op) {
    case SSS_HIP_SPMV_MXY: f(std::integral_constant<int, SSS_HIP_SPMV_MXY>(), std::false_type()); break;
    case SSS_HIP_SPMV_AMXPY: f(std::integral_constant<int, SSS_HIP_SPMV_AMXPY>(), std::false_type()); break;
    case SSS_HIP_SPMV_RESID:
        if (partial) f(std::integral_constant<int, SSS_HIP_SPMV_RESID>(), std::true_type());
        else f(std::integral_constant<int, SSS_HIP_SPMV_RESID>(), std::false_type());
        break;
    case SSS_HIP_SPMV_ACC: f(std::integral_constant<int, SSS_HIP_SPMV_ACC>(), std::false_type()); break;
    default: return false;
    }
    return true;
}

int launch_spmv(const DevCSR &A, int op, double alpha, const double *x, const double *b, double *y, int cap,
                double *partial, hipStream_t stream)
{
    if (A.n == 0 || A.nblk == 0) return 0;
    if (ledger_on()) ledger_add(matrix_bytes(A, 0, A.nblk) + xgather_bytes(A, A.n) + spmv_row_bytes(op) * A.n);
    if (!with_spmv_op(op, partial != nullptr, [&](auto O, auto NM) {
            launch_op<decltype(O)::value, decltype(NM)::value>(A, alpha, x, b, y, cap,
                                                               decltype(NM)::value ? partial : nullptr, stream);
        }))
        return ERROR_INPUT_PAR;
    SSS_HIP(hipGetLastError());
    return 0;
}

// x_r += P e over C rows whose prolongation row is one stored 1.0 (the injection of the C point's
// coarse value; sss_hier.hip hb_level_pr finds them): the tile AMXPY epilogue's arithmetic --
// s = 0.0 + 1.0 * e_c from the stored-order chain, out = x_r + s * 1.0 -- without the CSR arrays,
// their row blocks or the LDS staging.
__global__ __launch_bounds__(kBlock) void prolong_inject(int m, int lo, const int *__restrict__ col,
                                                         const double *__restrict__ e, double *__restrict__ x)
{
    const int q = blockIdx.x * kBlock + (int)threadIdx.x;
    if (q < m) {
        const double s = 0.0 + 1.0 * e[col[q]];
        x[lo + q] = x[lo + q] + s * 1.0;
    }
}

int launch_prolong_inject(int m, int lo, const int *col, const double *e, double *x, hipStream_t s)
{
    if (m <= 0) return 0;
    ledger_add(28.0 * m);   // col, the gathered e, x read and written
    hipLaunchKernelGGL(prolong_inject, dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, s, m, lo, col, e, x);
    SSS_HIP(hipGetLastError());
    return 0;
}

int launch_spmv_range(const DevCSR &A, int blo, int bhi, int op, double alpha, const double *x, const double *b,
                      double *y, double *partial, hipStream_t s)
{
    if (A.wave_rows || A.vec_rows || blo < 0 || bhi > A.nblk) return ERROR_INPUT_PAR;
    // (ACC, whose row cap has no meaning on a block range, and unknown ops: refused before anything is
    // counted or launched, so with_spmv_op below always finds the op)
    if (op != SSS_HIP_SPMV_RESID && op != SSS_HIP_SPMV_AMXPY && op != SSS_HIP_SPMV_MXY) return ERROR_INPUT_PAR;
    const int nb = bhi - blo;
    if (nb <= 0) return 0;
    if (ledger_on()) {
        const double rows = A.h_bk ? A.h_bk[bhi].x - A.h_bk[blo].x : (double)A.n * nb / A.nblk;
        ledger_add(matrix_bytes(A, blo, bhi) + xgather_bytes(A, rows) + spmv_row_bytes(op) * rows);
    }
    // the kernel indexes blocks from 0: shift the block-indexed arrays
    const int2 *pb = A.pb ? A.pb + blo : nullptr;
    double *pp = partial ? partial + blo : nullptr;
    DevDict dt = devdict(A, blo);
    dt.bend = nb;   // the kernel sees blocks [0, nb)
    with_spmv_op(op, partial != nullptr, [&](auto op_c, auto norm_c) {
        constexpr int O = decltype(op_c)::value;
        constexpr bool NM = decltype(norm_c)::value;
        with_tile_kind(A, [&](auto K) {
            constexpr int KK = decltype(K)::value;
            const int grid = (nb + rows_per_wg(KK) - 1) / rows_per_wg(KK);
            hipLaunchKernelGGL((spmv_adaptive<O, NM, KK>), dim3(grid), dim3(kBlock), 0, s, A.bk + blo, A.rp, A.ci, A.v,
                               x, b, y, alpha, 0, pp, A.pk, A.pv, pb, dt);
        });
    });
    SSS_HIP(hipGetLastError());
    return 0;
}

// ---- deterministic final reduction ----------------------------------------------------------
// Two fixed-order stages: kFinalChunks workgroups each reduce one contiguous chunk of the partials
// (lane-strided sums + xor tree + waves in order) into scratch[b]; one workgroup then sums those.
// A single workgroup streaming all 250,000 level-0 partials took ~100 us; two stages take ~10 us.
constexpr int kFinalChunks = kFinalScratch;

__device__ __forceinline__ double block_sum_1024(double v, double *red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < 1024 / 64; ++w) t += red[w];
    return t;
}

__global__ __launch_bounds__(1024) void final_sum_chunks(const double *__restrict__ partials, int n, int chunk,
                                                         double *__restrict__ scratch)
{
    __shared__ double red[1024 / 64];
    const int a = blockIdx.x * chunk, e = min(n, a + chunk);
    double v = 0.0;
    for (int i = a + (int)threadIdx.x; i < e; i += 1024) v += partials[i];
    const double t = block_sum_1024(v, red);
    if (threadIdx.x == 0) scratch[blockIdx.x] = t;
}

__global__ __launch_bounds__(1024) void final_sum_kernel(const double *__restrict__ partials, int n,
                                                         double *__restrict__ out, int take_sqrt)
{
    __shared__ double red[1024 / 64];
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) v += partials[i];
    const double t = block_sum_1024(v, red);
    if (threadIdx.x == 0) *out = take_sqrt ? sqrt(t) : t;
}

// partials must have room for n + kFinalChunks doubles (the tail is the first stage's scratch)
int launch_final_sum(double *partials, int n, double *out, bool take_sqrt, hipStream_t s)
{
    ledger_add(8.0 * n);
    if (n > 4 * 1024) {
        const int chunk = (n + kFinalChunks - 1) / kFinalChunks, nb = (n + chunk - 1) / chunk;
        hipLaunchKernelGGL(final_sum_chunks, dim3(nb), dim3(1024), 0, s, partials, n, chunk, partials + n);
        hipLaunchKernelGGL(final_sum_kernel, dim3(1), dim3(1024), 0, s, partials + n, nb, out, take_sqrt ? 1 : 0);
    } else {
        hipLaunchKernelGGL(final_sum_kernel, dim3(1), dim3(1024), 0, s, partials, n, out, take_sqrt ? 1 : 0);
    }
    SSS_HIP(hipGetLastError());
    return 0;
}

}  // namespace sss

// ---- C ABI: plans over caller-owned device CSR ----------------------------------------------
struct sss_hip_spmv_plan {
    sss::DevCSR csr;   // rp/ci/v borrowed from the caller (not owned); blk owned
};

extern "C" sss_hip_spmv_plan *sss_hip_spmv_plan_create(int n, int nnz, const int *d_rp, const int *h_rp)
{
    auto *p = new sss_hip_spmv_plan();
    std::vector<int> blk;
    p->csr.n = n;
    p->csr.nnz = nnz;
    p->csr.rp = const_cast<int *>(d_rp);
    p->csr.nblk = sss::build_row_blocks(h_rp, n, blk);
    p->csr.wave_rows = n > 0 && (long long)nnz >= (long long)sss::wave_row_min() * n;
    p->csr.ngrid = p->csr.wave_rows ? (n + 3) / 4 : p->csr.nblk;
    p->csr.blk = sss::dev_alloc<int>(blk.size());
    if (!p->csr.blk || hipMemcpy(p->csr.blk, blk.data(), sizeof(int) * blk.size(), hipMemcpyHostToDevice) != hipSuccess ||
        sss::upload_block_bounds(&p->csr.bk, blk, h_rp)) {
        sss::dev_free(p->csr.blk);
        sss::dev_free(p->csr.bk);
        delete p;
        return nullptr;
    }
    return p;
}

extern "C" void sss_hip_spmv_plan_destroy(sss_hip_spmv_plan *p)
{
    if (!p) return;
    sss::dev_free(p->csr.blk);
    sss::dev_free(p->csr.bk);
    delete p;
}

extern "C" int sss_hip_spmv(const sss_hip_spmv_plan *p, int op, double alpha, const int *d_rp, const int *d_ci,
                            const double *d_v, const double *d_x, const double *d_b, double *d_y, int cap,
                            void *stream)
{
    sss::DevCSR A = p->csr;
    A.rp = const_cast<int *>(d_rp);
    A.ci = const_cast<int *>(d_ci);
    A.v = const_cast<double *>(d_v);
    return sss::launch_spmv(A, op, alpha, d_x, d_b, d_y, cap, nullptr, (hipStream_t)stream);
}
