// sss_fgmres.hip — fused multi-vector orthogonalisation for the AMG-preconditioned flexible GMRES
// (sss_hip_fgmres, sss_hier.hip), fp64.
//
// One Arnoldi step orthogonalises w against the basis V = [v_0 .. v_{k-1}] (columns back to back,
// leading dimension ld, every column 16-byte aligned) by classical Gram-Schmidt applied twice:
//
//   c1 = V^T w;  w -= V c1;  c2 = V^T w;  w -= V c2;  h = c1 + c2;  ||w||
//
//   multi_dot   c[i] = <w, v_i> for all i in one pass: w is read once per kOrthCols columns, the
//               columns in register blocks of kOrthWidth.  Fixed grid (kOrthBlocks contiguous
//               chunks), lane-strided sums, xor tree, waves in order -> part[i][block].
//   multi_final one workgroup per column sums its kOrthBlocks partials in a fixed order; the second
//               pass adds its coefficients into the Hessenberg column on the device.
//   multi_axpy  w += sign * sum_i c[i] v_i, coefficients from device memory; the same launch leaves
//               the per-workgroup partials of ||w||^2 of the new w (same chunks, same order).
//   scale       w /= *nrm (the next basis vector; the norm stays on the device).
//
// No atomics anywhere: results are bitwise reproducible run to run.  All HBM-bound: a step at
// k columns moves (4k + 6) * 8n bytes in 8 launches (2 x (dot, final, axpy), the norm's final sum,
// the scale's 16n on top), against (5k) * 8n and 3k launches for a chain of dot + axpy pairs.
#include "sss_engine.hpp"
#include "sss_spmv_dev.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace sss {

constexpr int kOrthWidth = 8;                 // columns per register block
constexpr int kOrthMaxNB = 3;                 // register blocks one multi_dot launch holds (200 VGPRs, 2 waves/SIMD)
constexpr int kOrthCols = kOrthWidth * kOrthMaxNB;

// The chunk of workgroup b: [lo, hi), lo even so that the 16-byte loads stay aligned.
__device__ __forceinline__ void orth_chunk(int n, int &lo, int &hi)
{
    int per = (n + kOrthBlocks - 1) / kOrthBlocks;
    per += per & 1;
    const long long a = (long long)blockIdx.x * per;
    lo = a < n ? (int)a : n;
    hi = a + per < n ? (int)(a + per) : n;
}

// part[c * kOrthBlocks + block] = sum over the block's chunk of w[i] * v_c[i], c < k <= NB * kOrthWidth.
// Columns k .. NB * kOrthWidth - 1 of the last register block alias column 0 (loads that hit the
// cache, results dropped), so every load of an iteration is issued before the first use.
template <int NB>
__global__ __launch_bounds__(kBlock) void multi_dot_partials(int n, int k, const double *__restrict__ V, size_t ld,
                                                             const double *__restrict__ w, double *__restrict__ part)
{
    constexpr int KC = NB * kOrthWidth;
    __shared__ double red[KC * (kBlock / 64)];
    int lo, hi;
    orth_chunk(n, lo, hi);
    double acc[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[c] = 0.0;
    for (int i = lo + 2 * (int)threadIdx.x; i < hi; i += 2 * kBlock) {
        if (i + 1 < hi) {
            const double2 wv = *reinterpret_cast<const double2 *>(w + i);
            double2 vv[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) vv[c] = *reinterpret_cast<const double2 *>(V + (size_t)(c < k ? c : 0) * ld + i);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                acc[c] += wv.x * vv[c].x;
                acc[c] += wv.y * vv[c].y;
            }
        } else {   // the last element of an odd n
            const double wv = w[i];
#pragma unroll
            for (int c = 0; c < KC; ++c) acc[c] += wv * V[(size_t)(c < k ? c : 0) * ld + i];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        double v = acc[c];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red[c * (kBlock / 64) + wave] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < k) {
        double t = 0.0;
        for (int wv = 0; wv < kBlock / 64; ++wv) t += red[threadIdx.x * (kBlock / 64) + wv];
        part[(size_t)threadIdx.x * kOrthBlocks + blockIdx.x] = t;
    }
}

// c[b] = sum of column b's partials; hcol[b] = c[b] (first pass) or hcol[b] + c[b] (second pass)
__global__ __launch_bounds__(kBlock) void multi_final(const double *__restrict__ part, double *__restrict__ c,
                                                      double *__restrict__ hcol, int first)
{
    __shared__ double red[kBlock / 64];
    const double *p = part + (size_t)blockIdx.x * kOrthBlocks;
    double s = 0.0;
    for (int i = threadIdx.x; i < kOrthBlocks; i += kBlock) s += p[i];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) {
        c[blockIdx.x] = t;
        if (hcol) hcol[blockIdx.x] = first ? t : hcol[blockIdx.x] + t;
    }
}

// w[i] += sign * (coef[0] v_0[i] + coef[1] v_1[i] + ...), the sum formed first, in column order;
// npart (optional): npart[block] = sum over the block's chunk of the new w[i]^2.
__global__ __launch_bounds__(kBlock) void multi_axpy_dev(int n, int k, const double *__restrict__ V, size_t ld,
                                                         const double *__restrict__ coef, double sign,
                                                         double *__restrict__ w, double *__restrict__ npart)
{
    __shared__ double red[kBlock / 64];
    int lo, hi;
    orth_chunk(n, lo, hi);
    double nrm = 0.0;
    for (int i = lo + 2 * (int)threadIdx.x; i < hi; i += 2 * kBlock) {
        if (i + 1 < hi) {
            double2 wv = *reinterpret_cast<const double2 *>(w + i);
            double sx = 0.0, sy = 0.0;
#pragma unroll 8
            for (int c = 0; c < k; ++c) {
                const double cc = coef[c];
                const double2 vv = *reinterpret_cast<const double2 *>(V + (size_t)c * ld + i);
                sx += cc * vv.x;
                sy += cc * vv.y;
            }
            wv.x += sign * sx;
            wv.y += sign * sy;
            *reinterpret_cast<double2 *>(w + i) = wv;
            nrm += wv.x * wv.x;
            nrm += wv.y * wv.y;
        } else {
            double sx = 0.0;
#pragma unroll 8
            for (int c = 0; c < k; ++c) sx += coef[c] * V[(size_t)c * ld + i];
            const double wv = w[i] + sign * sx;
            w[i] = wv;
            nrm += wv * wv;
        }
    }
    if (npart) {
        const double t = block_sum(nrm, red);
        if (threadIdx.x == 0) npart[blockIdx.x] = t;
    }
}

// w /= *nrm (a zero norm -- the happy breakdown -- leaves w as it is)
__global__ __launch_bounds__(kBlock) void scale_inv_dev(int n, double *__restrict__ w, const double *__restrict__ nrm)
{
    const double d = *nrm;
    if (d == 0.0) return;
    const long long i = 2 * ((long long)blockIdx.x * kBlock + threadIdx.x);
    if (i + 1 < n) {
        double2 wv = *reinterpret_cast<const double2 *>(w + i);
        wv.x /= d;
        wv.y /= d;
        *reinterpret_cast<double2 *>(w + i) = wv;
    } else if (i < n) {
        w[i] /= d;
    }
}

static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int launch_multi_dot(int n, int k, const double *V, size_t ld, const double *w, double *part, hipStream_t s)
{
    if (n < 0 || k < 1 || ld < (size_t)n || (ld & 1) || !aligned16(V) || !aligned16(w)) return ERROR_INPUT_PAR;
    ledger_add(8.0 * n * (k + (k + kOrthCols - 1) / kOrthCols));
    for (int c0 = 0; c0 < k; c0 += kOrthCols) {
        const int kk = std::min(k - c0, kOrthCols);
        const double *Vc = V + (size_t)c0 * ld;
        double *pc = part + (size_t)c0 * kOrthBlocks;
        switch ((kk + kOrthWidth - 1) / kOrthWidth) {
        case 1: hipLaunchKernelGGL(multi_dot_partials<1>, dim3(kOrthBlocks), dim3(kBlock), 0, s, n, kk, Vc, ld, w, pc); break;
        case 2: hipLaunchKernelGGL(multi_dot_partials<2>, dim3(kOrthBlocks), dim3(kBlock), 0, s, n, kk, Vc, ld, w, pc); break;
        default: hipLaunchKernelGGL(multi_dot_partials<3>, dim3(kOrthBlocks), dim3(kBlock), 0, s, n, kk, Vc, ld, w, pc); break;
        }
        static_assert(kOrthMaxNB == 3, "one case per register-block count");
    }
    SSS_HIP(hipGetLastError());
    return 0;
}

int launch_multi_final(int k, const double *part, double *c, double *hcol, bool first, hipStream_t s)
{
    if (k < 1) return ERROR_INPUT_PAR;
    hipLaunchKernelGGL(multi_final, dim3(k), dim3(kBlock), 0, s, part, c, hcol, first ? 1 : 0);
    SSS_HIP(hipGetLastError());
    return 0;
}

int launch_multi_axpy(int n, int k, const double *V, size_t ld, const double *coef, double sign, double *w,
                      double *npart, hipStream_t s)
{
    if (n < 0 || k < 1 || ld < (size_t)n || (ld & 1) || !aligned16(V) || !aligned16(w)) return ERROR_INPUT_PAR;
    ledger_add(8.0 * n * (k + 2));
    hipLaunchKernelGGL(multi_axpy_dev, dim3(kOrthBlocks), dim3(kBlock), 0, s, n, k, V, ld, coef, sign, w, npart);
    SSS_HIP(hipGetLastError());
    return 0;
}

int launch_scale_inv(int n, double *w, const double *nrm, hipStream_t s)
{
    if (n < 0 || !aligned16(w)) return ERROR_INPUT_PAR;
    if (n == 0) return 0;
    ledger_add(16.0 * n);
    hipLaunchKernelGGL(scale_inv_dev, dim3((unsigned)(((long long)n + 2 * kBlock - 1) / (2 * kBlock))), dim3(kBlock), 0, s, n,
                       w, nrm);
    SSS_HIP(hipGetLastError());
    return 0;
}

// One orthogonalisation step (CGS2) of w against the k columns of V.  hcol gets the k Hessenberg
// coefficients and, in hcol[k], ||w|| of the orthogonalised w; c: k doubles of scratch; part:
// orth_part_doubles(k) doubles.  Everything stays on the device.
int launch_orth_step(int n, int k, const double *V, size_t ld, double *w, double *part, double *c, double *hcol,
                     hipStream_t s)
{
    double *npart = part, *dpart = part + kOrthBlocks + kFinalScratch;
    int rc;
    for (int pass = 0; pass < 2; ++pass) {
        if ((rc = launch_multi_dot(n, k, V, ld, w, dpart, s))) return rc;
        if ((rc = launch_multi_final(k, dpart, c, hcol, pass == 0, s))) return rc;
        if ((rc = launch_multi_axpy(n, k, V, ld, c, -1.0, w, pass ? npart : nullptr, s))) return rc;
    }
    return launch_final_sum(npart, kOrthBlocks, hcol + k, true, s);
}

}  // namespace sss

using namespace sss;

// The device step on host data: V holds k columns of n doubles back to back.  w comes back
// orthogonalised (not normalised), hcol[0 .. k) the coefficients, *norm = ||w||.
extern "C" int sss_hip_host_orth(int n, int k, const double *V, double *w, double *hcol, double *norm)
{
    if (n < 1 || k < 1 || !V || !w || !hcol || !norm) return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const size_t ld = (size_t)n + (n & 1);
    double *dV = dev_alloc<double>(ld * k), *dw = dev_alloc<double>(ld), *part = dev_alloc<double>(orth_part_doubles(k));
    double *sc = dev_alloc<double>((size_t)2 * k + 1);
    int rc = (!dV || !dw || !part || !sc) ? ERROR_ALLOC_MEM : 0;
    if (!rc && hipMemcpy2D(dV, ld * sizeof(double), V, (size_t)n * sizeof(double), (size_t)n * sizeof(double), k,
                           hipMemcpyHostToDevice) != hipSuccess)
        rc = ERROR_MISC;
    if (!rc && hipMemcpy(dw, w, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
    if (!rc) rc = launch_orth_step(n, k, dV, ld, dw, part, sc, sc + k, nullptr);
    if (!rc && hipMemcpy(w, dw, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) rc = ERROR_MISC;
    if (!rc && hipMemcpy(hcol, sc + k, sizeof(double) * k, hipMemcpyDeviceToHost) != hipSuccess) rc = ERROR_MISC;
    if (!rc && hipMemcpy(norm, sc + 2 * k, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = ERROR_MISC;
    dev_free(dV);
    dev_free(dw);
    dev_free(part);
    dev_free(sc);
    return rc;
}

// Lab timing (not in the public header): milliseconds of one orthogonalisation step of a vector
// against j + 1 orthonormal-sized columns of n, averaged over reps after one warm-up -- the fused
// step above, and the same step as a modified Gram-Schmidt chain of launch_dot + launch_axpy_ratio.
// The two alternate rep by rep on the same vectors.
extern "C" int sss_lab_time_orth(int n, int j, int reps, double *fused_ms, double *chain_ms)
{
    if (n < 1 || j < 0 || reps < 1) return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const int k = j + 1;
    const size_t ld = (size_t)n + (n & 1);
    double *dV = dev_alloc<double>(ld * k), *dw = dev_alloc<double>(ld), *part = dev_alloc<double>(orth_part_doubles(k));
    double *sc = dev_alloc<double>((size_t)2 * k + 3);
    std::vector<double> col((size_t)n);
    int rc = (!dV || !dw || !part || !sc) ? ERROR_ALLOC_MEM : 0;
    // columns of magnitude n^-1/2 with a per-column pattern (the time does not depend on the values)
    const double a = 1.0 / std::sqrt((double)n);
    for (int c = 0; c <= k && !rc; ++c) {
        for (int i = 0; i < n; ++i) col[(size_t)i] = ((i + c) % (c + 2) == 0) ? a : -a;
        double *dst = c < k ? dV + (size_t)c * ld : dw;
        if (hipMemcpy(dst, col.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
    }
    const double one = 1.0;
    double *d_one = sc + 2 * k + 1, *d_dot = sc + 2 * k + 2;
    if (!rc && hipMemcpy(d_one, &one, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = ERROR_MISC;
    double tf = 0.0, tc = 0.0;
    for (int r = -1; r < reps && !rc; ++r) {   // r = -1: warm-up
        for (int which = 0; which < 2 && !rc; ++which) {
            if (hipEventRecord(e0, nullptr) != hipSuccess) rc = ERROR_MISC;
            if (which == 0) {
                if (!rc) rc = launch_orth_step(n, k, dV, ld, dw, part, sc, sc + k, nullptr);
            } else {
                for (int c = 0; c < k && !rc; ++c) {
                    rc = launch_dot(n, dw, dV + (size_t)c * ld, part, d_dot, nullptr);
                    if (!rc) rc = launch_axpy_ratio(n, d_dot, d_one, -1.0, dV + (size_t)c * ld, dw, nullptr);
                }
            }
            if (!rc && (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess)) rc = ERROR_MISC;
            float ms = 0.0f;
            if (!rc && hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = ERROR_MISC;
            if (r >= 0) (which ? tc : tf) += ms;
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    dev_free(dV);
    dev_free(dw);
    dev_free(part);
    dev_free(sc);
    if (rc) return rc;
    *fused_ms = tf / reps;
    *chain_ms = tc / reps;
    return 0;
}
