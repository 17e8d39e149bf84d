// sss_fgmres.hip — the AMG-preconditioned flexible GMRES of every engine (sss_hip_fgmres,
// sss_hip_dist_fgmres): the solver loop fgmres_solve over the KrylovEngine interface of
// sss_engine.hpp, its workspace, and the fused multi-vector orthogonalisation it runs on, fp64.
//
// One Arnoldi step orthogonalises w against the basis V = [v_0 .. v_{k-1}] (columns back to back,
// leading dimension ld, every column 16-byte aligned) by classical Gram-Schmidt applied twice:
//
//   c1 = V^T w;  w -= V c1;  c2 = V^T w;  w -= V c2;  h = c1 + c2;  ||w||
//
//   multi_dot   c[i] = <w, v_i> for all i in one pass: w is read once per kOrthCols columns, the
//               columns in register blocks of kOrthWidth.  Fixed grid (kOrthBlocks contiguous
//               chunks), lane-strided sums, xor tree, waves in order -> part[i][block].
//   multi_final one workgroup per column sums its kOrthBlocks partials in a fixed order.
//   multi_axpy  w += sign * sum_i c[i] v_i, coefficients from device memory; the same launch leaves
//               the per-workgroup partials of ||w||^2 of the new w (same chunks, same order).
//   arnoldi_finish  h = c1 + c2 and the root of ||w||^2, from the coefficients and the sum as the
//               engine's reduction over the ranks left them (one small workgroup).
//   scale       w /= *nrm (the next basis vector; the norm stays on the device).
//
// No atomics anywhere: results are bitwise reproducible run to run.  All HBM-bound: a step at
// k columns moves (4k + 6) * 8n bytes in 9 launches (2 x (dot, final, axpy), the norm's final sum,
// the finish, the scale's 16n on top), against (5k) * 8n and 3k launches for a chain of dot + axpy
// pairs.  An engine with a stall word adds the one-thread launch that folds it into the read-back.
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
    dot_chunk(n, lo, hi);
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

// c[b] = sum of column b's partials
__global__ __launch_bounds__(kBlock) void multi_final(const double *__restrict__ part, double *__restrict__ c)
{
    __shared__ double red[kBlock / 64];
    const double *p = part + (size_t)blockIdx.x * kOrthBlocks;
    double s = 0.0;
    for (int i = threadIdx.x; i < kOrthBlocks; i += kBlock) s += p[i];
    const double t = block_sum(s, red);
    if (threadIdx.x == 0) c[blockIdx.x] = t;
}

// w[i] += sign * (coef[0] v_0[i] + coef[1] v_1[i] + ...), the sum formed first, in column order;
// npart (optional): npart[block] = sum over the block's chunk of the new w[i]^2.
__global__ __launch_bounds__(kBlock) void multi_axpy_dev(int n, int k, const double *__restrict__ V, size_t ld,
                                                         const double *__restrict__ coef, double sign,
                                                         double *__restrict__ w, double *__restrict__ npart)
{
    __shared__ double red[kBlock / 64];
    int lo, hi;
    dot_chunk(n, lo, hi);
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

// hcol[i] = c1[i] + c2[i] for i < k (the Hessenberg column from the reduced coefficients of the two
// Gram-Schmidt passes), hcol[k] = sqrt(ns[0]) (the norm, root taken after the reduction),
// hcol[k + 1] = ns[1] (the stall flag, for the same read-back)
__global__ __launch_bounds__(256) void arnoldi_finish(int k, const double *__restrict__ c1, const double *__restrict__ c2,
                                                       const double *__restrict__ ns, double *__restrict__ hcol)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) hcol[i] = c1[i] + c2[i];
    else if (i == k) hcol[k] = sqrt(ns[0]);
    else if (i == k + 1) hcol[k + 1] = ns[1];
}

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

int launch_multi_final(int k, const double *part, double *c, hipStream_t s)
{
    if (k < 1) return ERROR_INPUT_PAR;
    hipLaunchKernelGGL(multi_final, dim3(k), dim3(kBlock), 0, s, part, c);
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

int launch_arnoldi_finish(int k, const double *c1, const double *c2, const double *ns, double *hcol, hipStream_t s)
{
    if (k < 0) return ERROR_INPUT_PAR;
    hipLaunchKernelGGL(arnoldi_finish, dim3((k + 2 + 255) / 256), dim3(256), 0, s, k, c1, c2, ns, hcol);
    SSS_HIP(hipGetLastError());
    return 0;
}

// One orthogonalisation step (CGS2) of w against the k columns of V, the same for every engine:
// each of the three partial results -- c1, c2, {||w||^2, stall flag} -- goes through the engine's
// reduction over the ranks before it is used.  Everything stays on the device.
int launch_orth_step(int n, int k, const double *V, size_t ld, double *w, double *part, const OrthScalars &sc,
                     KrylovEngine *eng, hipStream_t s)
{
    double *npart = part, *dpart = part + kOrthBlocks + kFinalScratch;
    auto reduce = [&](double *dv, int count) { return eng ? eng->reduce(dv, sc.mirror + (dv - sc.c1), count) : 0; };
    int rc;
    for (int pass = 0; pass < 2; ++pass) {
        double *c = pass ? sc.c2 : sc.c1;
        if ((rc = launch_multi_dot(n, k, V, ld, w, dpart, s)) || (rc = launch_multi_final(k, dpart, c, s)) ||
            (rc = reduce(c, k)) || (rc = launch_multi_axpy(n, k, V, ld, c, -1.0, w, pass ? npart : nullptr, s)))
            return rc;
    }
    if ((rc = launch_final_sum(npart, kOrthBlocks, sc.ns, false, s))) return rc;
    unsigned *stall = eng ? eng->stall_word() : nullptr;
    if (stall && (rc = launch_err_flag(stall, sc.ns + 1, s))) return rc;
    if ((rc = reduce(sc.ns, 2))) return rc;
    return launch_arnoldi_finish(k, sc.c1, sc.c2, sc.ns, sc.hcol, s);
}

void FgmresWork::release()
{
    dev_free(v);
    dev_free(part);
    dev_free(s);
    if (h) (void)hipHostFree(h);
    v = part = s = h = nullptr;
    m = 0;
}

int FgmresWork::ensure(int want, size_t ld, hipStream_t stream)
{
    if (want <= m) return 0;
    SSS_HIP(hipStreamSynchronize(stream));
    release();
    const size_t ns = (size_t)4 * want + 4;
    v = dev_alloc<double>(((size_t)2 * want + 3) * ld);
    part = dev_alloc<double>(orth_part_doubles(want));
    s = dev_alloc<double>(ns);
    if (!v || !part || !s) {
        release();
        return hip_fail(hipErrorOutOfMemory, "hipMalloc(fgmres)", __FILE__, __LINE__);
    }
    SSS_HIP(hipHostMalloc((void **)&h, ns * sizeof(double), hipHostMallocDefault));
    SSS_HIP(hipMemsetAsync(s, 0, ns * sizeof(double), stream));   // an engine without a stall word never writes its slot
    m = want;
    return 0;
}

// Right-preconditioned FGMRES(m): z_j = one cycle on (v_j, 0), w = A z_j, w orthogonalised against
// v_0 .. v_j by launch_orth_step, which leaves the Hessenberg column, ||w|| and the stall flag on the
// device; one read-back of j + 3 doubles per iteration.  Givens rotations and the triangular solve
// run on the host; x += Z y at a restart, at convergence of the estimate |g_{j+1}| / ||b|| and at
// maxit.  Every branch and loop exit is taken from reduced values only, so all ranks of a
// partitioned engine leave in the same iteration.
int fgmres_solve(KrylovEngine &eng, FgmresWork &W, int m, double tol, int maxit, int *iters, double *relres,
                 double *hist, int hist_cap, const char *who)
{
    const int n = eng.n, cap = W.m;
    const size_t ld = (size_t)n + (n & 1);   // every column 16-byte aligned
    const hipStream_t s = eng.stream;
    double *V = W.v, *Z = V + ((size_t)cap + 1) * ld, *bs = Z + (size_t)cap * ld, *xs = bs + ld;
    double *dc1 = W.s, *dc2 = dc1 + cap, *dns = dc2 + cap, *dh = dns + 2, *dy = dh + cap + 2;
    double *H0 = W.h, *hns = H0 + (dns - dc1), *hh = H0 + (dh - dc1), *yh = H0 + (dy - dc1);
    double *dpart = W.part + kOrthBlocks + kFinalScratch;
    const OrthScalars sc{dc1, dc2, dns, dh, H0};
    const size_t bytes = sizeof(double) * (size_t)n;
    int it = 0;
    double rel = 1.0;
    auto norm_of = [&](const double *v, double *out) -> int {   // dh[0] = the global ||v||, also returned
        int c = launch_multi_dot(n, 1, v, ld, v, dpart, s);
        if (!c) c = launch_final_sum(dpart, kOrthBlocks, dns, false, s);
        if (!c) c = eng.reduce(dns, hns, 1);
        if (!c) c = launch_arnoldi_finish(0, dc1, dc2, dns, dh, s);
        if (!c) c = eng.fetch(dh, hh, 1);
        *out = hh[0];
        return c;
    };
    auto solve = [&]() -> int {
        int rc;
        SSS_HIP(hipMemcpyAsync(bs, eng.b, bytes, hipMemcpyDeviceToDevice, s));
        SSS_HIP(hipMemcpyAsync(xs, eng.x, bytes, hipMemcpyDeviceToDevice, s));
        double nb = 0.0;
        std::vector<double> R((size_t)(m + 1) * m, 0.0), cs((size_t)m), sn((size_t)m), g((size_t)m + 1);   // R: column-major
        if ((rc = norm_of(bs, &nb))) return rc;
        if (!std::isfinite(nb)) return ERROR_SOLVER_EXIT;
        if (nb == 0.0) {
            SSS_HIP(hipMemsetAsync(xs, 0, bytes, s));
            rel = 0.0;
            return 0;
        }
        bool done = maxit < 1;
        while (!done) {
            double beta = 0.0;
            if ((rc = eng.residual(xs, bs, V))) return rc;   // r = b - A x
            if ((rc = norm_of(V, &beta))) return rc;
            if (!std::isfinite(beta)) return ERROR_SOLVER_EXIT;
            if (it == 0) rel = beta / nb;
            if (beta == 0.0) return 0;   // x solves the system exactly
            if ((rc = launch_scale_inv(n, V, dh, s))) return rc;   // v_0 = r / ||r||
            g[0] = beta;
            int ncols = 0;
            for (int j = 0; j < m && !done; ++j) {
                ++it;
                const int k = j + 1;
                double *w = V + (size_t)(j + 1) * ld, *hj = R.data() + (size_t)j * (m + 1);
                if ((rc = eng.precondition_apply(V + (size_t)j * ld, Z + (size_t)j * ld, w))) return rc;
                if ((rc = launch_orth_step(n, k, V, ld, w, W.part, sc, &eng, s))) return rc;
                if ((rc = launch_scale_inv(n, w, dh + k, s))) return rc;   // v_{j+1} = w / ||w||
                if ((rc = eng.fetch(dh, hh, k + 2))) return rc;
                if (hh[k + 1] != 0.0) return eng.stalled(who);
                if (!std::isfinite(hh[k])) return ERROR_SOLVER_EXIT;
                for (int i = 0; i < k + 1; ++i) hj[i] = hh[i];
                for (int i = 0; i < j; ++i) {   // the earlier rotations, then the one that clears h_{j+1,j}
                    const double t = cs[i] * hj[i] + sn[i] * hj[i + 1];
                    hj[i + 1] = -sn[i] * hj[i] + cs[i] * hj[i + 1];
                    hj[i] = t;
                }
                const double d = std::hypot(hj[j], hj[j + 1]);
                cs[j] = d != 0.0 ? hj[j] / d : 1.0;
                sn[j] = d != 0.0 ? hj[j + 1] / d : 0.0;
                hj[j] = d;
                g[j + 1] = -sn[j] * g[j];
                g[j] = cs[j] * g[j];
                rel = std::fabs(g[j + 1]) / nb;
                if (hist && it <= hist_cap) hist[it - 1] = rel;
                ncols = k;
                // h_{j+1,j} = 0 (happy breakdown) gives g_{j+1} = 0: solved with the columns so far
                done = rel < tol || it >= maxit || hh[k] == 0.0;
            }
            for (int i = ncols - 1; i >= 0; --i) {   // R y = g
                double t = g[i];
                for (int l = i + 1; l < ncols; ++l) t -= R[(size_t)l * (m + 1) + i] * yh[l];
                yh[i] = R[(size_t)i * (m + 1) + i] != 0.0 ? t / R[(size_t)i * (m + 1) + i] : 0.0;
            }
            SSS_HIP(hipMemcpyAsync(dy, yh, sizeof(double) * (size_t)ncols, hipMemcpyHostToDevice, s));
            if ((rc = launch_multi_axpy(n, ncols, Z, ld, dy, 1.0, xs, nullptr, s))) return rc;   // x += Z y
            SSS_HIP(hipStreamSynchronize(s));   // yh is rewritten at the next restart
        }
        return 0;
    };
    const int rc = solve();
    // the caller's b back, and the iterate (after an error: the last one formed)
    SSS_HIP(hipMemcpyAsync(eng.x, xs, bytes, hipMemcpyDeviceToDevice, s));
    SSS_HIP(hipMemcpyAsync(eng.b, bs, bytes, hipMemcpyDeviceToDevice, s));
    SSS_HIP(hipStreamSynchronize(s));
    if (iters) *iters = it;
    if (relres) *relres = rel;
    return rc;
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
    double *sc = dev_alloc<double>((size_t)3 * k + 4);   // c1, c2, {||w||^2, stall slot}, column + norm + stall
    const OrthScalars os{sc, sc + k, sc + 2 * k, sc + 2 * k + 2, nullptr};
    int rc = (!dV || !dw || !part || !sc) ? ERROR_ALLOC_MEM : 0;
    if (!rc && hipMemset(sc, 0, sizeof(double) * ((size_t)3 * k + 4)) != hipSuccess) rc = ERROR_MISC;
    if (!rc && hipMemcpy2D(dV, ld * sizeof(double), V, (size_t)n * sizeof(double), (size_t)n * sizeof(double), k,
                           hipMemcpyHostToDevice) != hipSuccess)
        rc = ERROR_MISC;
    if (!rc && hipMemcpy(dw, w, sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
    if (!rc) rc = launch_orth_step(n, k, dV, ld, dw, part, os, nullptr, nullptr);
    if (!rc && hipMemcpy(w, dw, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess) rc = ERROR_MISC;
    if (!rc && hipMemcpy(hcol, os.hcol, sizeof(double) * k, hipMemcpyDeviceToHost) != hipSuccess) rc = ERROR_MISC;
    if (!rc && hipMemcpy(norm, os.hcol + k, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) rc = ERROR_MISC;
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
    double *sc = dev_alloc<double>((size_t)3 * k + 6);   // as sss_hip_host_orth, then the chain's two scalars
    const OrthScalars os{sc, sc + k, sc + 2 * k, sc + 2 * k + 2, nullptr};
    std::vector<double> col((size_t)n);
    int rc = (!dV || !dw || !part || !sc) ? ERROR_ALLOC_MEM : 0;
    if (!rc && hipMemset(sc, 0, sizeof(double) * ((size_t)3 * k + 6)) != hipSuccess) rc = ERROR_MISC;
    // columns of magnitude n^-1/2 with a per-column pattern (the time does not depend on the values)
    const double a = 1.0 / std::sqrt((double)n);
    for (int c = 0; c <= k && !rc; ++c) {
        for (int i = 0; i < n; ++i) col[(size_t)i] = ((i + c) % (c + 2) == 0) ? a : -a;
        double *dst = c < k ? dV + (size_t)c * ld : dw;
        if (hipMemcpy(dst, col.data(), sizeof(double) * n, hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
    }
    const double one = 1.0;
    double *d_one = sc + 3 * k + 4, *d_dot = sc + 3 * k + 5;
    if (!rc && hipMemcpy(d_one, &one, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = ERROR_MISC;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!rc && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)) rc = ERROR_MISC;
    double tf = 0.0, tc = 0.0;
    for (int r = -1; r < reps && !rc; ++r) {   // r = -1: warm-up
        for (int which = 0; which < 2 && !rc; ++which) {
            if (hipEventRecord(e0, nullptr) != hipSuccess) rc = ERROR_MISC;
            if (which == 0) {
                if (!rc) rc = launch_orth_step(n, k, dV, ld, dw, part, os, nullptr, nullptr);
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
