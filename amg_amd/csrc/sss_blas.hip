// sss_blas.hip — device BLAS-1 for the AMG-preconditioned CG, fp64.
//
// dot: fixed-order two-level reduction (per-workgroup lane-strided sums + xor tree + waves in
// order into partials, then launch_final_sum), so results are deterministic run to run.  The
// vector updates are elementwise.  All HBM-bound: 16 B per element for a dot, 24 B for an axpy.
//
// Fused forms for the row-partitioned CG (sss_hip_dist_pcg, sss_dist.hip), where every launch and
// every reduction is a latency cost:
//   pcg_update    x += a p, r_old = r, r -= a q and the partials of r.r in one pass: 56 B per row in
//                 one launch, against 80 B in four (two axpy, a copy, a dot).  Elementwise bits are
//                 axpy_dev's.
//   dot2_partials r.z and r_old.z in one pass over z: 24 B per row against 32 B.
// Both run a fixed grid of kDotBlocks contiguous chunks with 16-byte loads where the vectors are
// 16-byte aligned; no atomics, fixed order, nothing waits on another workgroup.
#include "sss_engine.hpp"
#include "sss_spmv_dev.hpp"

namespace sss {

constexpr int kDotBlocks = 1024;   // partial sums per dot (fills the chip, fixed order)

__global__ __launch_bounds__(kBlock) void dot_partials(int n, const double *__restrict__ a, const double *__restrict__ b,
                                                       double *__restrict__ partial)
{
    __shared__ double red[kBlock / 64];
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per, hi = min(n, lo + per);
    double s = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += kBlock) s += a[i] * b[i];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

int launch_dot(int n, const double *a, const double *b, double *partial, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(dot_partials, dim3(kDotBlocks), dim3(kBlock), 0, s, n, a, b, partial);
    SSS_HIP(hipGetLastError());
    return launch_final_sum(partial, kDotBlocks, out, false, s);
}

// y = y + alpha * x  (alpha read from device memory: *alpha_num / *alpha_den, sign)
__global__ __launch_bounds__(kBlock) void axpy_dev(int n, const double *__restrict__ num, const double *__restrict__ den,
                                                   double sign, const double *__restrict__ x, double *__restrict__ y)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) y[i] += (sign * (*num / *den)) * x[i];
}

// p = z + beta * p, beta = (num - numold) / den (Polak-Ribiere; numold null: Fletcher-Reeves)
__global__ __launch_bounds__(kBlock) void xpby_dev(int n, const double *__restrict__ num, const double *__restrict__ numold,
                                                   const double *__restrict__ den, const double *__restrict__ z,
                                                   double *__restrict__ p)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) {
        const double beta = (numold ? *num - *numold : *num) / *den;
        p[i] = z[i] + beta * p[i];
    }
}

int launch_axpy_ratio(int n, const double *num, const double *den, double sign, const double *x, double *y,
                      hipStream_t s)
{
    hipLaunchKernelGGL(axpy_dev, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, num, den, sign, x, y);
    SSS_HIP(hipGetLastError());
    return 0;
}

int launch_xpby_ratio(int n, const double *num, const double *numold, const double *den, const double *z, double *p,
                      hipStream_t s)
{
    hipLaunchKernelGGL(xpby_dev, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, num, numold, den, z, p);
    SSS_HIP(hipGetLastError());
    return 0;
}

// dot2's partials are summed by launch_multi_final, and the fused kernels take dot_chunk's chunks
static_assert(kDotBlocks == kOrthBlocks, "one fixed grid for the fused BLAS-1 and the orthogonalisation");

// a = *num / *den:  x += a p,  r_old = r,  r += (-a) q,  partial[block] = sum of the new r[i]^2 over
// the block's chunk.  V2: every vector is 16-byte aligned (two rows per access).
template <bool V2>
__global__ __launch_bounds__(kBlock) void pcg_update_dev(int n, const double *__restrict__ num,
                                                         const double *__restrict__ den, const double *__restrict__ p,
                                                         const double *__restrict__ q, double *__restrict__ x,
                                                         double *__restrict__ r, double *__restrict__ r_old,
                                                         double *__restrict__ partial)
{
    __shared__ double red[kBlock / 64];
    int lo, hi;
    dot_chunk(n, lo, hi);
    const double a = *num / *den;
    const double ap = 1.0 * a, am = -1.0 * a;   // axpy_dev's (sign * (*num / *den))
    double s = 0.0;
    for (int i = lo + 2 * (int)threadIdx.x; i < hi; i += 2 * kBlock) {
        if (V2 && i + 1 < hi) {
            const double2 pv = *reinterpret_cast<const double2 *>(p + i);
            const double2 qv = *reinterpret_cast<const double2 *>(q + i);
            double2 xv = *reinterpret_cast<const double2 *>(x + i);
            double2 rv = *reinterpret_cast<const double2 *>(r + i);
            *reinterpret_cast<double2 *>(r_old + i) = rv;
            xv.x += ap * pv.x;
            xv.y += ap * pv.y;
            rv.x += am * qv.x;
            rv.y += am * qv.y;
            *reinterpret_cast<double2 *>(x + i) = xv;
            *reinterpret_cast<double2 *>(r + i) = rv;
            s += rv.x * rv.x;
            s += rv.y * rv.y;
        } else {
            for (int k = i; k < min(i + 2, hi); ++k) {
                const double rv0 = r[k];
                r_old[k] = rv0;
                x[k] += ap * p[k];
                const double rv = rv0 + am * q[k];
                r[k] = rv;
                s += rv * rv;
            }
        }
    }
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// partial[block] = sum of r[i] z[i], partial[kDotBlocks + block] = sum of r_old[i] z[i] over the chunk
template <bool V2>
__global__ __launch_bounds__(kBlock) void dot2_partials(int n, const double *__restrict__ r,
                                                        const double *__restrict__ r_old, const double *__restrict__ z,
                                                        double *__restrict__ partial)
{
    __shared__ double red[2][kBlock / 64];
    int lo, hi;
    dot_chunk(n, lo, hi);
    double s0 = 0.0, s1 = 0.0;
    for (int i = lo + 2 * (int)threadIdx.x; i < hi; i += 2 * kBlock) {
        if (V2 && i + 1 < hi) {
            const double2 zv = *reinterpret_cast<const double2 *>(z + i);
            const double2 rv = *reinterpret_cast<const double2 *>(r + i);
            const double2 ov = *reinterpret_cast<const double2 *>(r_old + i);
            s0 += rv.x * zv.x;
            s0 += rv.y * zv.y;
            s1 += ov.x * zv.x;
            s1 += ov.y * zv.y;
        } else {
            for (int k = i; k < min(i + 2, hi); ++k) {
                const double zv = z[k];
                s0 += r[k] * zv;
                s1 += r_old[k] * zv;
            }
        }
    }
    const double t0 = block_sum(s0, red[0]);
    const double t1 = block_sum(s1, red[1]);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = t0;
        partial[kDotBlocks + blockIdx.x] = t1;
    }
}

int launch_pcg_update(int n, const double *num, const double *den, const double *p, const double *q, double *x,
                      double *r, double *r_old, double *partial, hipStream_t s)
{
    if (n < 0) return ERROR_INPUT_PAR;
    ledger_add(56.0 * n);
    if (aligned16(p) && aligned16(q) && aligned16(x) && aligned16(r) && aligned16(r_old))
        hipLaunchKernelGGL(pcg_update_dev<true>, dim3(kDotBlocks), dim3(kBlock), 0, s, n, num, den, p, q, x, r, r_old,
                           partial);
    else
        hipLaunchKernelGGL(pcg_update_dev<false>, dim3(kDotBlocks), dim3(kBlock), 0, s, n, num, den, p, q, x, r, r_old,
                           partial);
    SSS_HIP(hipGetLastError());
    return 0;
}

int launch_dot2(int n, const double *r, const double *r_old, const double *z, double *partial, hipStream_t s)
{
    if (n < 0) return ERROR_INPUT_PAR;
    ledger_add(24.0 * n);
    if (aligned16(r) && aligned16(r_old) && aligned16(z))
        hipLaunchKernelGGL(dot2_partials<true>, dim3(kDotBlocks), dim3(kBlock), 0, s, n, r, r_old, z, partial);
    else
        hipLaunchKernelGGL(dot2_partials<false>, dim3(kDotBlocks), dim3(kBlock), 0, s, n, r, r_old, z, partial);
    SSS_HIP(hipGetLastError());
    return 0;
}

}  // namespace sss

using namespace sss;

// pcg_update on host data, through the same kernel: a = alpha_num / alpha_den; x and r are updated
// in place, r_old receives the old r and *rr the sum of squares of the new r.
extern "C" int sss_hip_host_pcg_update(int n, double alpha_num, double alpha_den, const double *p, const double *q,
                                       double *x, double *r, double *r_old, double *rr)
{
    if (n < 1 || !p || !q || !x || !r || !r_old || !rr) return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const size_t ld = (size_t)n + (n & 1), bytes = sizeof(double) * (size_t)n;
    double *v = dev_alloc<double>(5 * ld), *part = dev_alloc<double>(kDotBlocks + kFinalScratch), *sc = dev_alloc<double>(3);
    int rc = (!v || !part || !sc) ? ERROR_ALLOC_MEM : 0;
    double *dp = v, *dq = dp + ld, *dx = dq + ld, *dr = dx + ld, *dro = dr + ld;
    const double a[2] = {alpha_num, alpha_den};
    if (!rc && (hipMemcpy(sc, a, sizeof(a), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dp, p, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dq, q, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dr, r, bytes, hipMemcpyHostToDevice) != hipSuccess))
        rc = ERROR_MISC;
    if (!rc) rc = launch_pcg_update(n, sc, sc + 1, dp, dq, dx, dr, dro, part, nullptr);
    if (!rc) rc = launch_final_sum(part, kDotBlocks, sc + 2, false, nullptr);
    if (!rc && (hipMemcpy(x, dx, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(r, dr, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(r_old, dro, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(rr, sc + 2, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
        rc = ERROR_MISC;
    dev_free(v);
    dev_free(part);
    dev_free(sc);
    return rc;
}

// dot2_partials on host data: out[0] = r . z, out[1] = r_old . z
extern "C" int sss_hip_host_dot2(int n, const double *r, const double *r_old, const double *z, double *out)
{
    if (n < 1 || !r || !r_old || !z || !out) return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const size_t ld = (size_t)n + (n & 1), bytes = sizeof(double) * (size_t)n;
    double *v = dev_alloc<double>(3 * ld), *part = dev_alloc<double>(2 * kDotBlocks), *sc = dev_alloc<double>(2);
    int rc = (!v || !part || !sc) ? ERROR_ALLOC_MEM : 0;
    if (!rc && (hipMemcpy(v, r, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(v + ld, r_old, bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(v + 2 * ld, z, bytes, hipMemcpyHostToDevice) != hipSuccess))
        rc = ERROR_MISC;
    if (!rc) rc = launch_dot2(n, v, v + ld, v + 2 * ld, part, nullptr);
    if (!rc) rc = launch_multi_final(2, part, sc, nullptr);
    if (!rc && hipMemcpy(out, sc, 2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = ERROR_MISC;
    dev_free(v);
    dev_free(part);
    dev_free(sc);
    return rc;
}

// Lab timing (not in the public header): milliseconds of one CG iteration's level-0 vector work on n
// rows, averaged over reps after one warm-up -- the fused pair (pcg_update + the sum of its partials,
// dot2_partials + the sum of its two columns) and the chain it replaces (two launch_axpy_ratio, a
// device copy, launch_dot of r.r, then launch_dot of r.z and of r_old.z).  The two alternate rep by
// rep on the same vectors; a = 1e-3 keeps the values bounded over the reps.
extern "C" int sss_lab_time_pcg_fused(int n, int reps, double *fused_ms, double *chain_ms)
{
    if (n < 1 || reps < 1 || !fused_ms || !chain_ms) return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const size_t ld = (size_t)n + (n & 1), bytes = sizeof(double) * (size_t)n;
    double *v = dev_alloc<double>(6 * ld), *part = dev_alloc<double>(2 * kDotBlocks + kFinalScratch), *sc = dev_alloc<double>(5);
    int rc = (!v || !part || !sc) ? ERROR_ALLOC_MEM : 0;
    double *p = v, *q = p + ld, *x = q + ld, *r = x + ld, *ro = r + ld, *z = ro + ld;
    {
        std::vector<double> col((size_t)n);
        for (int c = 0; c < 6 && !rc; ++c) {
            for (int i = 0; i < n; ++i) col[(size_t)i] = ((i + c) % (c + 2) == 0) ? 1.0 : -0.5;
            if (hipMemcpy(v + (size_t)c * ld, col.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
        }
    }
    const double a[2] = {1.0, 1000.0};
    if (!rc && hipMemcpy(sc, a, sizeof(a), hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = ERROR_MISC;
    double tf = 0.0, tc = 0.0;
    for (int rep = -1; rep < reps && !rc; ++rep) {   // rep = -1: warm-up
        for (int which = 0; which < 2 && !rc; ++which) {
            if (hipEventRecord(e0, nullptr) != hipSuccess) rc = ERROR_MISC;
            if (which == 0) {
                if (!rc) rc = launch_pcg_update(n, sc, sc + 1, p, q, x, r, ro, part, nullptr);
                if (!rc) rc = launch_final_sum(part, kDotBlocks, sc + 2, false, nullptr);
                if (!rc) rc = launch_dot2(n, r, ro, z, part, nullptr);
                if (!rc) rc = launch_multi_final(2, part, sc + 3, nullptr);
            } else {
                if (!rc) rc = launch_axpy_ratio(n, sc, sc + 1, 1.0, p, x, nullptr);
                if (!rc && hipMemcpyAsync(ro, r, bytes, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) rc = ERROR_MISC;
                if (!rc) rc = launch_axpy_ratio(n, sc, sc + 1, -1.0, q, r, nullptr);
                if (!rc) rc = launch_dot(n, r, r, part, sc + 2, nullptr);
                if (!rc) rc = launch_dot(n, r, z, part, sc + 3, nullptr);
                if (!rc) rc = launch_dot(n, ro, z, part, sc + 4, nullptr);
            }
            if (!rc && (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) rc = ERROR_MISC;
            float ms = 0.0f;
            if (!rc && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = ERROR_MISC;
            if (rep >= 0) (which ? tc : tf) += ms;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    dev_free(v);
    dev_free(part);
    dev_free(sc);
    if (rc) return rc;
    *fused_ms = tf / reps;
    *chain_ms = tc / reps;
    return 0;
}
