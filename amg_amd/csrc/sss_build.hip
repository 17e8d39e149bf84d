// sss_build.hip — device-side builders of the free-order storage formats (upload time).
//
// The long-row levels of a throughput-mode hierarchy (levels 5-10 of 7-pt 400^3) are read through
//   * merged row groups (DevCSR::mg_*): the entries of G consecutive rows, sorted by the unique
//     key  col << 4 | segment << 3 | row-in-group  (sss_engine.hpp), and
//   * column-sorted row segments (DevCSR::rows_sorted): each row -- or each of its two segments
//     [rp, seg) / [seg, rp + 1) -- sorted by column.
// The host builders (sss_formats.hip build_merged / sort_row_segments) sort these on the CPU, 3-4 ns
// per entry on the 16-core box, which was most of the mirror construction left after an
// overlapped setup (profiles/r03_host_phases_seq_400.txt: 0.5-0.8 s per coarse level).  Here the
// stored-order CSR already resident in HBM is sorted in place on the GPU by a segmented radix sort.
// Every key is unique inside its segment (a row's columns are distinct, and the segment / row bits
// separate the rows of a group), so the result does not depend on the sort's stability: it is the
// host builder's output bit for bit (tests/test_gpu_setup_pipeline.py compares whole solves).
#include <hipcub/hipcub.hpp>

#include "sss_engine.hpp"

namespace sss {

namespace {

// key[k] of every entry of row r: col << kMergeShift | segment << 3 | (r mod G)
__global__ __launch_bounds__(kBlock) void merged_keys(int n, int G, const int *__restrict__ rp,
                                                      const int *__restrict__ ci, const int *__restrict__ seg,
                                                      unsigned *__restrict__ key)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const unsigned rig = (unsigned)(r % G);
    const int s = seg ? seg[r] : rp[r + 1];
    for (int k = rp[r]; k < rp[r + 1]; ++k)
        key[k] = ((unsigned)ci[k] << kMergeShift) | ((k >= s ? 1u : 0u) << 3) | rig;
}

// gp[g] = rp[g G] (g < ng), gp[ng] = rp[n]
__global__ __launch_bounds__(kBlock) void group_bounds(int n, int G, int ng, const int *__restrict__ rp,
                                                       int *__restrict__ gp)
{
    const int g = blockIdx.x * kBlock + threadIdx.x;
    if (g < ng) gp[g] = rp[g * G];
    else if (g == ng) gp[g] = rp[n];
}

// segment offsets of two-segment rows: off[2r] = rp[r], off[2r + 1] = seg[r], off[2n] = rp[n]
__global__ __launch_bounds__(kBlock) void segment_offsets(int n, const int *__restrict__ rp, const int *__restrict__ seg,
                                                          int *__restrict__ off)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r < n) {
        off[2 * r] = rp[r];
        off[2 * r + 1] = seg[r];
    } else if (r == n) {
        off[2 * n] = rp[n];
    }
}

// out = in sorted within each segment [off[s], off[s + 1]) by the 32-bit key (keys unique per
// segment), values carried along
int segmented_sort(const unsigned *kin, unsigned *kout, const double *vin, double *vout, int nnz, int nseg,
                   const int *off, hipStream_t s)
{
    if (nnz == 0 || nseg == 0) return 0;
    size_t tb = 0;
    SSS_HIP(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tb, kin, kout, vin, vout, nnz, nseg, off, off + 1, 0,
                                                        32, s));
    void *tmp = nullptr;
    SSS_HIP(hipMalloc(&tmp, std::max<size_t>(tb, 1)));
    const hipError_t e = hipcub::DeviceSegmentedRadixSort::SortPairs(tmp, tb, kin, kout, vin, vout, nnz, nseg, off,
                                                                     off + 1, 0, 32, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(tmp);
    SSS_HIP(e);
    SSS_HIP(e2);
    return 0;
}

// Narrow keys of a sorted merged key list (DevCSR::mg_k16 / mg_d; the host's merged_narrow bit for
// bit): one wave per share (group s / W, part s % W), a chunk of 64 keys per step.  elen[s] = the
// share's entries if one of its chunks is wide (the share then keeps 32-bit keys), else 0; cnt as
// DevCSR::mg_cnt.  desc is zero-filled by the caller.
struct ShareSpan {
    int a, e;         // entries [a, e)
    long long d0;     // first descriptor
};
__device__ __forceinline__ ShareSpan share_span(long long s, int W, const int *__restrict__ gp)
{
    const int g = (int)(s / W), part = (int)(s % W);
    const long long k0 = gp[g], len = gp[g + 1] - k0, per = (len + W - 1) / W;
    ShareSpan sp;
    sp.a = (int)(k0 + min(len, part * per));
    sp.e = (int)(k0 + min(len, (part + 1) * per));
    sp.d0 = (sp.a >> 6) + (long long)g * W + part;
    return sp;
}
__global__ __launch_bounds__(kBlock) void narrow_chunks(int ng, int W, int two, const int *__restrict__ gp,
                                                        const unsigned *__restrict__ key,
                                                        unsigned short *__restrict__ k16, int4 *__restrict__ desc,
                                                        int *__restrict__ elen, unsigned long long *__restrict__ cnt)
{
    constexpr int kSpan = 1 << kMergeDeltaBits;
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (s >= (long long)ng * W) return;
    const ShareSpan sp = share_span(s, W, gp);
    unsigned c[4] = {0, 0, 0, 0};
    bool wide = false;
    int ch = 0;
    for (int kb = sp.a; kb < sp.e; kb += 64, ++ch) {
        const int m = min(64, sp.e - kb);
        const bool live = lane < m;
        const unsigned q = live ? key[kb + lane] : 0u;
        const int col = (int)(q >> kMergeShift);
        const int prev = __shfl_up(col, 1, 64);
        const int w = (live && lane >= 1) ? col - prev : 0;   // the gap before this lane (sorted: >= 0)
        // the widest gap, the lowest lane on ties
        unsigned long long best = ((unsigned long long)(unsigned)w << 6) | (unsigned)(63 - lane);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(best, off, 64);
            best = o > best ? o : best;
        }
        int split = (best >> 6) > 0 ? 63 - (int)(best & 63) : 64;
        const int first = __shfl(col, 0, 64), last = __shfl(col, m - 1, 64);
        int lo = first, hi = first, kind;
        if (last - first < kSpan) {
            kind = 1, split = 64;
        } else {
            hi = __shfl(col, split, 64);
            const int below = __shfl(col, split - 1, 64) - first;
            kind = (below < kSpan && last - hi < kSpan) ? 2 : 3;
        }
        ++c[0], ++c[kind];
        unsigned short k = 0;
        int4 d = make_int4(0, 0, 64, -1);
        if (kind == 3) {
            wide = true;
        } else {
            d = make_int4(lo, hi, split, -1);
            const unsigned acc = two ? ((q >> 1) & 4u) | (q & 3u) : q & 7u;
            k = (unsigned short)((unsigned)(col - (lane < split ? lo : hi)) << 3 | acc);
        }
        if (live) k16[kb + lane] = k;
        if (lane == 0) desc[sp.d0 + ch] = d;
    }
    if (lane == 0) {
        elen[s] = wide ? sp.e - sp.a : 0;
        for (int i = 0; i < 4; ++i)
            if (c[i]) atomicAdd(&cnt[i], (unsigned long long)c[i]);
        if (wide) atomicAdd(&cnt[4], (unsigned long long)ch);
    }
}
// the escaped shares' 32-bit keys at eoff[s] (the exclusive sum of elen), and their chunks' positions
__global__ __launch_bounds__(kBlock) void narrow_escape(int ng, int W, const int *__restrict__ gp,
                                                        const unsigned *__restrict__ key, const int *__restrict__ eoff,
                                                        int4 *__restrict__ desc, unsigned *__restrict__ ke)
{
    const int lane = threadIdx.x & 63;
    const long long s = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (s >= (long long)ng * W) return;
    const int o = eoff[s];
    if (eoff[s + 1] == o) return;
    const ShareSpan sp = share_span(s, W, gp);
    const int m = sp.e - sp.a;
    for (int i = lane; i < m; i += 64) ke[o + i] = key[sp.a + i];
    for (int c = lane; c < (m + 63) >> 6; c += 64) desc[sp.d0 + c].w = o + 64 * c;
}

int upload_seg(const int *h_seg, int n, int **d_seg)
{
    *d_seg = nullptr;
    if (!h_seg) return 0;
    return dev_upload(*d_seg, h_seg, (size_t)n, "hipMalloc(seg)");
}

// d.mg_k16 / mg_d / mg_ke from the sorted 32-bit keys (d.mg_gp, mg_ng, mg_W, mg_two set)
int merged_narrow_device(DevCSR &d, const unsigned *sorted)
{
    const int ng = d.mg_ng, W = d.mg_W;
    const long long ns = (long long)ng * W, nd = merged_desc_slots(d.nnz, ng, W);
    d.mg_nd = nd;
    d.mg_k16 = dev_alloc<unsigned short>((size_t)d.nnz);
    d.mg_d = dev_alloc<int4>((size_t)nd);
    int *elen = dev_alloc<int>((size_t)ns + 1), *eoff = dev_alloc<int>((size_t)ns + 1);
    unsigned long long *cnt = dev_alloc<unsigned long long>(5);
    void *tmp = nullptr;
    int rc = (!d.mg_k16 || !d.mg_d || !elen || !eoff || !cnt) ? hip_fail(hipErrorOutOfMemory, "hipMalloc(narrow)", __FILE__, __LINE__) : 0;
    auto check = [&](hipError_t e, const char *what) {
        if (!rc && e != hipSuccess) rc = hip_fail(e, what, __FILE__, __LINE__);
    };
    if (!rc) {
        check(hipMemsetAsync(d.mg_d, 0, sizeof(int4) * (size_t)nd, nullptr), "hipMemset(narrow)");
        check(hipMemsetAsync(elen, 0, sizeof(int) * ((size_t)ns + 1), nullptr), "hipMemset(narrow)");
        check(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * 5, nullptr), "hipMemset(narrow)");
    }
    const unsigned grid = (unsigned)((ns + kBlock / 64 - 1) / (kBlock / 64));
    int total = 0;
    if (!rc && ns > 0) {
        hipLaunchKernelGGL(narrow_chunks, dim3(grid), dim3(kBlock), 0, nullptr, ng, W, d.mg_two ? 1 : 0, d.mg_gp, sorted,
                           d.mg_k16, d.mg_d, elen, cnt);
        check(hipGetLastError(), "narrow_chunks");
        size_t tb = 0;
        check(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, elen, eoff, (int)(ns + 1), nullptr), "scan(narrow)");
        check(hipMalloc(&tmp, std::max<size_t>(tb, 1)), "hipMalloc(narrow)");
        if (!rc) check(hipcub::DeviceScan::ExclusiveSum(tmp, tb, elen, eoff, (int)(ns + 1), nullptr), "scan(narrow)");
        if (!rc) check(hipMemcpy(&total, eoff + ns, sizeof(int), hipMemcpyDeviceToHost), "hipMemcpy(narrow)");
    }
    if (!rc) {
        unsigned long long c[5] = {};
        check(hipMemcpy(c, cnt, sizeof(c), hipMemcpyDeviceToHost), "hipMemcpy(narrow)");
        for (int i = 0; i < 5; ++i) d.mg_cnt[i] = (long long)c[i];
        d.mg_ne = total;
        d.mg_ke = dev_alloc<unsigned>((size_t)std::max(total, 1));
        if (!d.mg_ke) rc = hip_fail(hipErrorOutOfMemory, "hipMalloc(narrow)", __FILE__, __LINE__);
    }
    if (!rc && total > 0) {
        hipLaunchKernelGGL(narrow_escape, dim3(grid), dim3(kBlock), 0, nullptr, ng, W, d.mg_gp, sorted, eoff, d.mg_d,
                           d.mg_ke);
        check(hipGetLastError(), "narrow_escape");
    }
    check(hipStreamSynchronize(nullptr), "narrow");   // `sorted` is freed by the caller
    (void)hipFree(tmp);
    dev_free(elen);
    dev_free(eoff);
    dev_free(cnt);
    return rc;
}

}  // namespace

// d: rp / ci / v resident in stored order, d.mg_G > 0.  Fills mg_gp, mg_k, mg_v, mg_ng.
int merged_build_device(DevCSR &d, const int *h_seg)
{
    const int n = d.n, G = d.mg_G, ng = (n + G - 1) / G;
    d.mg_ng = ng;
    const bool narrow = merged_key16_ok(d);
    d.mg_gp = dev_alloc<int>((size_t)ng + 1);
    unsigned *sorted = dev_alloc<unsigned>((size_t)d.nnz);   // the 32-bit keys: mg_k, or scratch of the narrowing
    d.mg_v = dev_alloc<double>((size_t)d.nnz);
    unsigned *key = dev_alloc<unsigned>((size_t)d.nnz);
    int *dseg = nullptr;
    int rc = (!d.mg_gp || !sorted || !d.mg_v || !key) ? hip_fail(hipErrorOutOfMemory, "hipMalloc(merged)", __FILE__, __LINE__)
                                                       : upload_seg(h_seg, n, &dseg);
    if (!rc) {
        hipLaunchKernelGGL(group_bounds, dim3((ng + kBlock) / kBlock), dim3(kBlock), 0, nullptr, n, G, ng, d.rp, d.mg_gp);
        if (n > 0)
            hipLaunchKernelGGL(merged_keys, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, n, G, d.rp, d.ci,
                               dseg, key);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = hip_fail(e, "merged_keys", __FILE__, __LINE__);
    }
    if (!rc) rc = segmented_sort(key, sorted, d.v, d.mg_v, d.nnz, ng, d.mg_gp, nullptr);
    dev_free(key);
    dev_free(dseg);
    if (!narrow || rc) {
        d.mg_k = sorted;
        return rc;
    }
    rc = merged_narrow_device(d, sorted);
    dev_free(sorted);
    return rc;
}

// d.ci / d.v (stored order) sorted by column within each row, or each row segment when h_seg is
// given; sets d.rows_sorted.
int sort_rows_device(DevCSR &d, const int *h_seg)
{
    const int n = d.n;
    unsigned *kin = dev_alloc<unsigned>((size_t)d.nnz);
    double *vin = dev_alloc<double>((size_t)d.nnz);
    int *dseg = nullptr, *off = nullptr;
    int rc = (!kin || !vin) ? hip_fail(hipErrorOutOfMemory, "hipMalloc(row sort)", __FILE__, __LINE__) : 0;
    if (!rc && h_seg) {
        rc = upload_seg(h_seg, n, &dseg);
        off = rc ? nullptr : dev_alloc<int>(2 * (size_t)n + 1);
        if (!rc && !off) rc = hip_fail(hipErrorOutOfMemory, "hipMalloc(row sort)", __FILE__, __LINE__);
        if (!rc) hipLaunchKernelGGL(segment_offsets, dim3((n + kBlock) / kBlock), dim3(kBlock), 0, nullptr, n, d.rp, dseg, off);
    }
    if (!rc && hipMemcpy(kin, d.ci, sizeof(int) * (size_t)d.nnz, hipMemcpyDeviceToDevice) != hipSuccess) rc = ERROR_MISC;
    if (!rc && hipMemcpy(vin, d.v, sizeof(double) * (size_t)d.nnz, hipMemcpyDeviceToDevice) != hipSuccess) rc = ERROR_MISC;
    if (!rc)   // columns are non-negative, so their unsigned order is the column order
        rc = segmented_sort(kin, reinterpret_cast<unsigned *>(d.ci), vin, d.v, d.nnz, h_seg ? 2 * n : n,
                            h_seg ? off : d.rp, nullptr);
    if (!rc) d.rows_sorted = true;
    dev_free(kin);
    dev_free(vin);
    dev_free(dseg);
    dev_free(off);
    return rc;
}

}  // namespace sss
