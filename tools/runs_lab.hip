// runs_lab.hip — merged row groups of a long-row Galerkin level (7-pt 400^3 level 6 shape: ~100K
// rows, ~800 entries per row, the 8 rows of a group sharing ~2.8x their columns) in two layouts
// (lab only, not product code):
//   M: the engine's merged groups -- one 32-bit key  col << 4 | row  and one value per entry,
//      lanes strided over the group's entries, x gathered per entry;
//   R: column runs -- one 32-bit key  col << 8 | row mask  per distinct column of the group, the
//      values of a run contiguous; a wave scan of the runs' popcounts places each lane's values,
//      x gathered once per run.
//   A: the M layout with the lane's accumulators in three forms (kA): registers with one select per
//      accumulator and entry (the engine's merged_sums), LDS with one fp64 LDS add per entry
//      (merged_sums_lds), LDS with an explicit read, add, write per entry; for G = 8 rows in one
//      segment and for G = 4 rows in two segments (the same 8 accumulators: row r of the G = 8
//      group becomes segment r / 4, row r % 4), with every gather issued before any product or
//      each product formed where it is added.  All forms must agree bit for bit, also on
//      subnormal products and on signed zeros.
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off tools/runs_lab.hip -o tools/runs_lab
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define CK(x)                                                                                   \
    do {                                                                                        \
        hipError_t e = (x);                                                                     \
        if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } \
    } while (0)

constexpr int G = 8;

// M: one wave per group (W waves per group: a contiguous share each), U entries in flight per lane
template <int W>
__global__ __launch_bounds__(256) void kM(int ng, const int *gp, const unsigned *mk, const double *mv, const double *x,
                                          double *y)
{
    constexpr int U = 8;
    __shared__ double red[4][G];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, gpb = 4 / W;
    const int g = blockIdx.x * gpb + w / W, part = w % W;
    double s[G];
    for (int u = 0; u < G; ++u) s[u] = 0.0;
    if (g < ng) {
        const int a = gp[g], e = gp[g + 1], len = e - a, per = (len + W - 1) / W;
        const int k0 = a + min(len, part * per), k1 = a + min(len, (part + 1) * per);
        for (int k = k0 + lane; k < k1; k += 64 * U) {
            unsigned q[U];
            double v[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const int kk = k + 64 * t;
                q[t] = kk < k1 ? mk[kk] : 0u;
                v[t] = kk < k1 ? mv[kk] : 0.0;
            }
#pragma unroll
            for (int t = 0; t < U; ++t) {
                if (k + 64 * t >= k1) break;
                const double p = v[t] * x[q[t] >> 4];
#pragma unroll
                for (int u = 0; u < G; ++u) s[u] += (q[t] & 15u) == (unsigned)u ? p : 0.0;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < G; ++u)
        for (int off = 32; off > 0; off >>= 1) s[u] += __shfl_xor(s[u], off, 64);
    if (lane == 0)
        for (int u = 0; u < G; ++u) red[w][u] = s[u];
    __syncthreads();
    const int t = threadIdx.x;
    if (t < gpb * G) {
        const int gi = t / G, u = t % G, gg = blockIdx.x * gpb + gi;
        if (gg < ng) {
            double acc = 0.0;
            for (int v = 0; v < W; ++v) acc += red[gi * W + v][u];
            y[gg * G + u] = acc;
        }
    }
}

// one batch of C chunks of 64 entries, the last of last_n (1 ... 64): straight-line code per C
template <int C, class Add, class Slot>
__device__ __forceinline__ void batch(const unsigned *pk, const double *pv, int last_n, const double *x, Add add, Slot slot_of)
{
    const int lane = threadIdx.x & 63, ll = min(lane, last_n - 1);
    unsigned q[C];
    double v[C], xv[C];
#pragma unroll
    for (int t = 0; t < C; ++t) {
        const int o = 64 * t + (t == C - 1 ? ll : lane);
        q[t] = pk[o];
        v[t] = pv[o];
    }
#pragma unroll
    for (int t = 0; t < C; ++t) xv[t] = x[q[t] >> 4];
#pragma unroll
    for (int t = 0; t < C; ++t) {
        double p = v[t] * xv[t];
        if (t == C - 1) p = lane < last_n ? p : 0.0;
        add(slot_of(q[t]), p);
    }
}

// A: accumulator forms.  MODE 0 registers + selects, 1 LDS fp64 add, 2 LDS read-add-write,
// 3 LDS fp64 add with each batch's chunk count a scalar and straight-line code per count (only
// the last chunk's lanes clamped and masked).
// EARLY: every gather issued before any product.  y[g * 8 + slot], slot = segment * G + row.
template <int GG, int S, int W, int MODE, bool EARLY>
__global__ __launch_bounds__(256) void kA(int ng, const int *gp, const unsigned *mk, const double *mv, const double *x,
                                          double *y)
{
    constexpr int U = 8, NA = S * GG;
    __shared__ double red[4][NA];
    __shared__ double accs[MODE ? 4 * NA * 64 : 1];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, gpb = 4 / W;
    const int g = blockIdx.x * gpb + w / W, part = w % W;
    double s[NA];
    double *mine = accs + (MODE ? w * NA * 64 + lane : 0);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        s[a] = 0.0;
        if (MODE) mine[a * 64] = 0.0;
    }
    auto slot_of = [](unsigned q) -> unsigned {
        const unsigned key = q & 15u;
        return S == 2 ? (key >> 3) * GG + (key & (GG - 1)) : key & (GG - 1);
    };
    auto add = [&](unsigned slot, double p) {
        if (MODE == 1 || MODE == 3) atomicAdd(&mine[slot * 64], p);
        else if (MODE == 2) mine[slot * 64] += p;
        else {
#pragma unroll
            for (int a = 0; a < NA; ++a) s[a] += slot == (unsigned)a ? p : 0.0;
        }
    };
    if (g < ng) {
        const int a0 = gp[g], e = gp[g + 1], len = e - a0, per = (len + W - 1) / W;
        int k0 = a0 + min(len, part * per);
        const int k1 = a0 + min(len, (part + 1) * per);
        if (MODE == 3) {   // the engine's merged_sums_lds
            const int e1 = __builtin_amdgcn_readfirstlane(k1);
            for (int kb = __builtin_amdgcn_readfirstlane(k0); kb < e1; kb += 64 * U) {
                const int rem = min(e1 - kb, 64 * U), nch = (rem + 63) >> 6, last_n = rem - 64 * (nch - 1);
                const unsigned *pk = mk + kb;
                const double *pv = mv + kb;
                switch (nch) {
                case 8: batch<8>(pk, pv, last_n, x, add, slot_of); break;
                case 7: batch<7>(pk, pv, last_n, x, add, slot_of); break;
                case 6: batch<6>(pk, pv, last_n, x, add, slot_of); break;
                case 5: batch<5>(pk, pv, last_n, x, add, slot_of); break;
                case 4: batch<4>(pk, pv, last_n, x, add, slot_of); break;
                case 3: batch<3>(pk, pv, last_n, x, add, slot_of); break;
                case 2: batch<2>(pk, pv, last_n, x, add, slot_of); break;
                default: batch<1>(pk, pv, last_n, x, add, slot_of); break;
                }
            }
            k0 = k1;
        }
        for (int k = k0 + lane; k < k1; k += 64 * U) {
            unsigned q[U];
            double v[U], xv[U];
#pragma unroll
            for (int t = 0; t < U; ++t) {
                const int kk = k + 64 * t, kc = kk < k1 ? kk : k1 - 1;
                q[t] = mk[kc];
                v[t] = mv[kc];
            }
            if (EARLY) {
#pragma unroll
                for (int t = 0; t < U; ++t) xv[t] = k + 64 * t < k1 ? x[q[t] >> 4] : 0.0;
#pragma unroll
                for (int t = 0; t < U; ++t) add(slot_of(q[t]), k + 64 * t < k1 ? v[t] * xv[t] : 0.0);
            } else {
#pragma unroll
                for (int t = 0; t < U; ++t) {
                    if (k + 64 * t >= k1) break;
                    add(slot_of(q[t]), v[t] * x[q[t] >> 4]);
                }
            }
        }
    }
    if (MODE)
#pragma unroll
        for (int a = 0; a < NA; ++a) s[a] = mine[a * 64];
#pragma unroll
    for (int a = 0; a < NA; ++a)
        for (int off = 32; off > 0; off >>= 1) s[a] += __shfl_xor(s[a], off, 64);
    if (lane == 0)
        for (int a = 0; a < NA; ++a) red[w][a] = s[a];
    __syncthreads();
    const int t = threadIdx.x;
    if (t < gpb * NA) {
        const int gi = t / NA, a = t % NA, gg = blockIdx.x * gpb + gi;
        if (gg < ng) {
            double acc = 0.0;
            for (int v = 0; v < W; ++v) acc += red[gi * W + v][a];
            y[gg * NA + a] = acc;
        }
    }
}

// R: one wave per group; per iteration 64 runs (one per lane), an inclusive wave scan of their
// popcounts gives each lane its values' offset
__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}
template <int U>
__global__ __launch_bounds__(256) void kR(int ng, const int *rg, const int *vg, const unsigned *rk, const double *mv,
                                          const double *x, double *y)
{
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + w;
    double s[G];
    for (int u = 0; u < G; ++u) s[u] = 0.0;
    if (g < ng) {
        const int a = rg[g], e = rg[g + 1];
        int vb = vg[g];
        for (int t0 = a; t0 < e; t0 += 64 * U) {
            unsigned key[U];
            double xv[U];
            int cnt[U], off[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int t = t0 + 64 * j + lane;
                key[j] = t < e ? rk[t] : 0u;
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int t = t0 + 64 * j + lane;
                xv[j] = t < e ? x[key[j] >> 8] : 0.0;
                cnt[j] = __popc(key[j] & 0xffu);
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const int incl = wave_incl_scan(cnt[j]);
                off[j] = vb + incl - cnt[j];
                vb += __shfl(incl, 63, 64);
            }
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const unsigned m = key[j] & 0xffu;
                int k = off[j];
#pragma unroll
                for (int u = 0; u < G; ++u)
                    if (m & (1u << u)) s[u] += mv[k++] * xv[j];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < G; ++u)
        for (int off = 32; off > 0; off >>= 1) s[u] += __shfl_xor(s[u], off, 64);
    if (lane == 0 && g < ng)
        for (int u = 0; u < G; ++u) y[g * G + u] = s[u];
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 101911;
    const int per_row = argc > 2 ? atoi(argv[2]) : 822;
    const double share = argc > 3 ? atof(argv[3]) : 2.8;
    const int ng = (n + G - 1) / G;
    const int pool = (int)(per_row * G / share);
    std::mt19937 rng(7);
    std::vector<int> gp(1, 0), rg(1, 0), vg(1, 0);
    std::vector<unsigned> mk, rk;
    std::vector<double> mv, rv;
    std::vector<int> cols(pool);
    for (int g = 0; g < ng; ++g) {
        // the group's column pool: clustered around the group's position
        const int center = g * G;
        cols.assign(pool, 0);
        for (int c = 0; c < pool; ++c) {
            long long v = (long long)center + ((long long)(rng() % (2ull * (unsigned)n)) - (long long)n) / 4;
            cols[c] = (int)((v % n + n) % n);
        }
        std::sort(cols.begin(), cols.end());
        cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
        const double p = std::min(1.0, (double)per_row / cols.size());
        std::uniform_real_distribution<double> U01(0, 1);
        for (int c : cols) {
            unsigned mask = 0;
            for (int r = 0; r < G; ++r)
                if (g * G + r < n && U01(rng) < p) mask |= 1u << r;
            if (!mask) continue;
            rk.push_back((unsigned)c << 8 | mask);
            for (int r = 0; r < G; ++r)
                if (mask & (1u << r)) {
                    const double a = 1.0 + 1e-3 * (rng() % 1000);
                    mk.push_back((unsigned)c << 4 | r);
                    mv.push_back(a);
                }
        }
        gp.push_back((int)mk.size());
        rg.push_back((int)rk.size());
        vg.push_back((int)mv.size());
    }
    printf("rows %d, entries %zu (%.0f per row), runs %zu (%.2f entries per run)\n", n, mv.size(),
           (double)mv.size() / n, rk.size(), (double)mv.size() / rk.size());
    int *d_gp, *d_rg, *d_vg;
    unsigned *d_mk, *d_rk;
    double *d_mv, *x, *y1, *y2;
    CK(hipMalloc(&d_gp, gp.size() * 4));
    CK(hipMalloc(&d_rg, rg.size() * 4));
    CK(hipMalloc(&d_vg, vg.size() * 4));
    CK(hipMalloc(&d_mk, mk.size() * 4));
    CK(hipMalloc(&d_rk, rk.size() * 4));
    CK(hipMalloc(&d_mv, mv.size() * 8));
    CK(hipMalloc(&x, (size_t)n * 8));
    CK(hipMalloc(&y1, (size_t)ng * G * 8));
    CK(hipMalloc(&y2, (size_t)ng * G * 8));
    CK(hipMemcpy(d_gp, gp.data(), gp.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_rg, rg.data(), rg.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_vg, vg.data(), vg.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_mk, mk.data(), mk.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_rk, rk.data(), rk.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_mv, mv.data(), mv.size() * 8, hipMemcpyHostToDevice));
    {
        std::vector<double> h(n);
        for (int i = 0; i < n; ++i) h[i] = 1.0 + 1e-4 * (i % 97);
        CK(hipMemcpy(x, h.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const double bytesM = 12.0 * mv.size() + 4.0 * gp.size() + 8.0 * n * 2;
    const double bytesR = 8.0 * mv.size() + 4.0 * rk.size() + 8.0 * rg.size() + 8.0 * n * 2;
    auto run = [&](const char *name, double bytes, auto launch) {
        for (int i = 0; i < 3; ++i) launch();
        CK(hipDeviceSynchronize());
        const int reps = 20;
        CK(hipEventRecord(e0));
        for (int i = 0; i < reps; ++i) launch();
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        ms /= reps;
        printf("%-22s %8.1f us  %6.0f GB/s of its bytes (%.2f GB)\n", name, ms * 1e3, bytes / (ms * 1e-3) / 1e9, bytes / 1e9);
    };
    run("M merged W=4", bytesM, [&] { hipLaunchKernelGGL(kM<4>, dim3(ng), dim3(256), 0, 0, ng, d_gp, d_mk, d_mv, x, y1); });
    run("M merged W=2", bytesM, [&] { hipLaunchKernelGGL(kM<2>, dim3((ng + 1) / 2), dim3(256), 0, 0, ng, d_gp, d_mk, d_mv, x, y1); });
    run("M merged W=1", bytesM, [&] { hipLaunchKernelGGL(kM<1>, dim3((ng + 3) / 4), dim3(256), 0, 0, ng, d_gp, d_mk, d_mv, x, y1); });
    run("R runs U=1", bytesR, [&] { hipLaunchKernelGGL(kR<1>, dim3((ng + 3) / 4), dim3(256), 0, 0, ng, d_rg, d_vg, d_rk, d_mv, x, y2); });
    run("R runs U=2", bytesR, [&] { hipLaunchKernelGGL(kR<2>, dim3((ng + 3) / 4), dim3(256), 0, 0, ng, d_rg, d_vg, d_rk, d_mv, x, y2); });
    run("R runs U=4", bytesR, [&] { hipLaunchKernelGGL(kR<4>, dim3((ng + 3) / 4), dim3(256), 0, 0, ng, d_rg, d_vg, d_rk, d_mv, x, y2); });
    std::vector<double> a(ng * G), b(ng * G);
    CK(hipMemcpy(a.data(), y1, a.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), y2, b.size() * 8, hipMemcpyDeviceToHost));
    double md = 0;
    for (size_t i = 0; i < a.size(); ++i) md = std::max(md, std::abs(a[i] - b[i]) / std::max(1e-300, std::abs(a[i])));
    printf("max rel diff M vs R: %.3g\n", md);

    // ---- accumulator forms (A) -----------------------------------------------------------------
    // the two-segment copy of the keys: row r of the group -> segment r / 4, row r % 4
    std::vector<unsigned> mk2(mk.size());
    for (size_t i = 0; i < mk.size(); ++i) mk2[i] = (mk[i] & ~15u) | ((mk[i] & 4u) << 1) | (mk[i] & 3u);
    unsigned *d_mk2;
    double *y3;
    CK(hipMalloc(&d_mk2, mk2.size() * 4));
    CK(hipMalloc(&y3, (size_t)ng * G * 8));
    CK(hipMemcpy(d_mk2, mk2.data(), mk2.size() * 4, hipMemcpyHostToDevice));
    struct Form {
        const char *name;
        void (*k)(int, const int *, const unsigned *, const double *, const double *, double *);
        const unsigned *keys;
        int grid;
    };
    const Form forms[] = {
        {"A G8 S1 reg  early", kA<8, 1, 4, 0, true>, d_mk, 0},   {"A G8 S1 reg  late", kA<8, 1, 4, 0, false>, d_mk, 0},
        {"A G8 S1 ldsa early", kA<8, 1, 4, 1, true>, d_mk, 0},   {"A G8 S1 ldsa late", kA<8, 1, 4, 1, false>, d_mk, 0},
        {"A G8 S1 rmw  early", kA<8, 1, 4, 2, true>, d_mk, 0},   {"A G8 S1 rmw  late", kA<8, 1, 4, 2, false>, d_mk, 0},
        {"A G4 S2 reg  early", kA<4, 2, 4, 0, true>, d_mk2, 0},  {"A G4 S2 reg  late", kA<4, 2, 4, 0, false>, d_mk2, 0},
        {"A G4 S2 ldsa early", kA<4, 2, 4, 1, true>, d_mk2, 0},  {"A G4 S2 ldsa late", kA<4, 2, 4, 1, false>, d_mk2, 0},
        {"A G4 S2 rmw  early", kA<4, 2, 4, 2, true>, d_mk2, 0},  {"A G4 S2 rmw  late", kA<4, 2, 4, 2, false>, d_mk2, 0},
        {"A G8 S1 ldsa full", kA<8, 1, 4, 3, true>, d_mk, 0},    {"A G4 S2 ldsa full", kA<4, 2, 4, 3, true>, d_mk2, 0},
        {"A G8 S1 ldsa full W1", kA<8, 1, 1, 3, true>, d_mk, (ng + 3) / 4}, {"A G8 S1 ldsa early W1", kA<8, 1, 1, 1, true>, d_mk, (ng + 3) / 4},
    };
    const int nf = (int)(sizeof forms / sizeof forms[0]);
    for (const Form &f : forms)
        run(f.name, bytesM,
            [&] { hipLaunchKernelGGL(f.k, dim3(f.grid ? f.grid : ng), dim3(256), 0, 0, ng, d_gp, f.keys, d_mv, x, y3); });
    // bitwise agreement with M (W = 4) on three inputs: the timing x, x scaled so that products and
    // partial sums are subnormal, x of signed zeros
    for (int pass = 0; pass < 3; ++pass) {
        std::vector<double> h(n);
        for (int i = 0; i < n; ++i)
            h[i] = pass == 0 ? 1.0 + 1e-4 * (i % 97) : pass == 1 ? ldexp(1.0 + 1e-4 * (i % 97), -1040 - i % 40) * (i % 3 ? 1 : -1)
                                                                  : (i % 2 ? -0.0 : 0.0);
        CK(hipMemcpy(x, h.data(), (size_t)n * 8, hipMemcpyHostToDevice));
        // (the W = 1 forms against M with W = 1: the number of waves per group is part of the sum order)
        std::vector<double> a1(a.size());
        hipLaunchKernelGGL(kM<1>, dim3((ng + 3) / 4), dim3(256), 0, 0, ng, d_gp, d_mk, d_mv, x, y1);
        CK(hipMemcpy(a1.data(), y1, a1.size() * 8, hipMemcpyDeviceToHost));
        hipLaunchKernelGGL(kM<4>, dim3(ng), dim3(256), 0, 0, ng, d_gp, d_mk, d_mv, x, y1);
        CK(hipMemcpy(a.data(), y1, a.size() * 8, hipMemcpyDeviceToHost));
        size_t nonzero = 0, subn = 0;
        for (double v : a) nonzero += v != 0.0, subn += v != 0.0 && std::abs(v) < 2.3e-308;
        printf("input %d (%s): %zu sums nonzero, %zu subnormal\n", pass,
               pass == 0 ? "normal" : pass == 1 ? "subnormal products" : "signed zeros", nonzero, subn);
        for (int f = 0; f < nf; ++f) {
            CK(hipMemset(y3, 0xff, (size_t)ng * G * 8));
            hipLaunchKernelGGL(forms[f].k, dim3(forms[f].grid ? forms[f].grid : ng), dim3(256), 0, 0, ng, d_gp, forms[f].keys,
                               d_mv, x, y3);
            CK(hipMemcpy(b.data(), y3, b.size() * 8, hipMemcpyDeviceToHost));
            size_t bad = 0;
            const std::vector<double> &ref = forms[f].grid ? a1 : a;
            for (int i = 0; i < n; ++i) bad += memcmp(&ref[i], &b[i], 8) != 0;
            printf("  %-20s %s (%zu of %d rows differ)\n", forms[f].name, bad ? "DIFFERS" : "bitwise equal", bad, n);
        }
    }
    return 0;
}
