// sss_pmis.hip — the PMIS C/F split of the setup (cs_type SSS_COARSE_PMIS) on the GPU, mark for mark
// the host split (amg_amd/host/sss_setup.c pmis_split; the rule: DESIGN.md "PMIS coarsening").
//
//   lambda_i = stored entries of S with column i;  key_i = lambda_i << 32 | h(i), h a bijection
//   start: empty S row -> ISPT, else lambda_i = 0 -> FGPT, else undecided
//   round: (a) undecided i with key_i above the key of every undecided j in S_i u S^T_i -> CGPT
//          (b) then still undecided i with a CGPT point in S_i -> FGPT
//
// (a) needs the neighbours in both directions; S^T is never built.  Each undecided i walks row i
// and pushes its key into nbmax[j] of every undecided j there (a 64-bit atomicMax: j sees its S^T
// side), and pushes the largest undecided key it met into nbmax[i] (its S side).  After that launch
// nbmax[i] is the largest key among i's undecided neighbours, and i becomes C when key_i exceeds it.
// Integer max and add do not depend on their order, so the marks depend on S alone.
//
// ukey[i] is key_i while i is undecided and 0 once it is decided (an undecided point has
// lambda >= 1, so its key is never 0), which makes "undecided j, and its key" one 8-byte load.
// One round is three ordinary launches (push, decide C, decide F + count), the round loop is a host
// loop that reads two counters back per round and gives up after kPmisMaxRounds.  G lanes walk one
// row, G chosen from the average row length of S.
#include "sss_engine.hpp"

#include <cstring>

namespace sss {

namespace {

constexpr int kPmisMaxRounds = 4096;
using u64 = unsigned long long;

__host__ __device__ __forceinline__ unsigned pmis_hash(unsigned i)
{
    i ^= i >> 16;
    i *= 0x7feb352du;
    i ^= i >> 15;
    i *= 0x846ca68bu;
    i ^= i >> 16;
    return i;
}

// lambda[j] += 1 for every stored entry (i, j)
__global__ __launch_bounds__(kBlock) void pmis_lambda(long long nnz, int n, const int *__restrict__ ci,
                                                      int *__restrict__ lambda)
{
    const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (k >= nnz) return;
    const int j = ci[k];
    if ((unsigned)j < (unsigned)n) atomicAdd(&lambda[j], 1);
}

// the start marks and keys; ctr[0] += the undecided
__global__ __launch_bounds__(kBlock) void pmis_init(int n, const int *__restrict__ rp, const int *__restrict__ lambda,
                                                    int *__restrict__ mark, u64 *__restrict__ ukey,
                                                    u64 *__restrict__ nbmax, int *__restrict__ ctr)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool und = false;
    if (i < n) {
        const int lam = lambda[i];
        int m = UNPT;
        if (rp[i + 1] <= rp[i]) m = ISPT;
        else if (lam == 0) m = FGPT;
        und = m == UNPT;
        mark[i] = m;
        ukey[i] = und ? ((u64)(unsigned)lam << 32 | pmis_hash((unsigned)i)) : 0ull;
        nbmax[i] = 0ull;
    }
    const u64 b = __ballot(und);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctr[0], __popcll(b));
}

// row bounds of row i, clamped to the stored entries
__device__ __forceinline__ void row_span(const int *__restrict__ rp, int i, int nnz, int &lo, int &hi)
{
    lo = max(rp[i], 0);
    hi = min(rp[i + 1], nnz);
}

// (a), first half: every undecided i pushes its key to its undecided S neighbours and collects theirs
template <int G>
__global__ __launch_bounds__(kBlock) void pmis_push(int n, int nnz, const int *__restrict__ rp,
                                                    const int *__restrict__ ci, const u64 *__restrict__ ukey,
                                                    u64 *__restrict__ nbmax)
{
    const int i = (int)(((long long)blockIdx.x * kBlock + threadIdx.x) / G), gl = threadIdx.x % G;
    const u64 ki = i < n ? ukey[i] : 0ull;
    u64 best = 0ull;
    if (ki) {
        int lo, hi;
        row_span(rp, i, nnz, lo, hi);
        for (int q = lo + gl; q < hi; q += G) {
            const int j = ci[q];
            if ((unsigned)j >= (unsigned)n || j == i) continue;
            const u64 kj = ukey[j];
            if (!kj) continue;
            if (ki > nbmax[j]) atomicMax(&nbmax[j], ki);   // the plain read only skips pushes that cannot raise it
            best = kj > best ? kj : best;
        }
    }
    for (int o = G / 2; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(best, o, G);
        best = other > best ? other : best;
    }
    if (ki && gl == 0 && best) atomicMax(&nbmax[i], best);
}

// (a), second half: the local maxima become C.  ctr[0] (the undecided, counted again by pmis_f) is reset
// here; ctr[1] += the new C points.
__global__ __launch_bounds__(kBlock) void pmis_c(int n, int *__restrict__ mark, u64 *__restrict__ ukey,
                                                 const u64 *__restrict__ nbmax, int *__restrict__ ctr)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool c = false;
    if (i < n) {
        const u64 ki = ukey[i];
        c = ki && ki > nbmax[i];
        if (c) {
            mark[i] = CGPT;
            ukey[i] = 0ull;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr[0] = 0;
    const u64 b = __ballot(c);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctr[1], __popcll(b));
}

// (b): a still undecided i with a C point in its row becomes F; the others are counted into ctr[0]
// and get their nbmax cleared for the next round
template <int G>
__global__ __launch_bounds__(kBlock) void pmis_f(int n, int nnz, const int *__restrict__ rp, const int *__restrict__ ci,
                                                 int *__restrict__ mark, u64 *__restrict__ ukey,
                                                 u64 *__restrict__ nbmax, int *__restrict__ ctr)
{
    const int i = (int)(((long long)blockIdx.x * kBlock + threadIdx.x) / G), gl = threadIdx.x % G;
    const bool und = i < n && ukey[i] != 0ull;
    int has_c = 0;
    if (und) {
        int lo, hi;
        row_span(rp, i, nnz, lo, hi);
        for (int q = lo + gl; q < hi && !has_c; q += G) {
            const int j = ci[q];
            if ((unsigned)j < (unsigned)n && mark[j] == CGPT) has_c = 1;
        }
    }
    for (int o = G / 2; o > 0; o >>= 1) has_c |= __shfl_xor(has_c, o, G);
    bool left = false;
    if (und && gl == 0) {
        if (has_c) {
            mark[i] = FGPT;
            ukey[i] = 0ull;
        } else {
            nbmax[i] = 0ull;
            left = true;
        }
    }
    const u64 b = __ballot(left);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&ctr[0], __popcll(b));
}

template <int G>
void launch_round(int n, int nnz, const int *rp, const int *ci, int *mark, u64 *ukey, u64 *nbmax, int *ctr,
                  hipStream_t st)
{
    const unsigned rows_grid = (unsigned)(((long long)n * G + kBlock - 1) / kBlock);
    const unsigned elem_grid = (unsigned)((n + kBlock - 1) / kBlock);
    hipLaunchKernelGGL((pmis_push<G>), dim3(rows_grid), dim3(kBlock), 0, st, n, nnz, rp, ci, ukey, nbmax);
    hipLaunchKernelGGL(pmis_c, dim3(elem_grid), dim3(kBlock), 0, st, n, mark, ukey, nbmax, ctr);
    hipLaunchKernelGGL((pmis_f<G>), dim3(rows_grid), dim3(kBlock), 0, st, n, nnz, rp, ci, mark, ukey, nbmax, ctr);
}

int copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind k, hipStream_t st)
{
    if (bytes == 0) return 0;
    SSS_HIP(hipMemcpyAsync(dst, src, bytes, k, st));
    SSS_HIP(hipStreamSynchronize(st));
    return 0;
}

// lanes per row from the average row length (SSS_HIP_PMIS_LANES, tests: 1, 4, 16 or 64 whatever the rows)
int lanes_for(int n, int nnz)
{
    const char *e = getenv("SSS_HIP_PMIS_LANES");
    if (e && *e) {
        const int g = atoi(e);
        if (g == 1 || g == 4 || g == 16 || g == 64) return g;
    }
    const double avg = (double)nnz / (double)std::max(n, 1);
    return avg <= 2.0 ? 1 : avg <= 12.0 ? 4 : avg <= 48.0 ? 16 : 64;
}

struct DevArrays {
    int *rp = nullptr, *ci = nullptr, *lambda = nullptr, *mark = nullptr, *ctr = nullptr;
    u64 *ukey = nullptr, *nbmax = nullptr;
    hipStream_t st = nullptr;
    ~DevArrays()
    {
        dev_free(rp);
        dev_free(ci);
        dev_free(lambda);
        dev_free(mark);
        dev_free(ctr);
        dev_free(ukey);
        dev_free(nbmax);
        if (st) (void)hipStreamDestroy(st);
    }
};

}  // namespace

}  // namespace sss

using namespace sss;

extern "C" int sss_hip_pmis(const SSS_IMAT *S, int *mark, int *ncoarse, int *rounds)
{
    if (!S || !mark || S->num_rows <= 0 || !S->row_ptr) return ERROR_INPUT_PAR;
    const int n = S->num_rows;
    const int nnz = S->row_ptr[n];
    if (S->row_ptr[0] != 0 || nnz < 0 || (nnz > 0 && !S->col_idx)) return ERROR_INPUT_PAR;
    // n * 64 lanes must fit the launch arithmetic (long long there) and the grid (2^31 - 1 blocks)
    if ((long long)n * 64 / kBlock >= 0x7fffffffLL) return ERROR_MAT_SIZE;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;

    DevArrays d;
    if (hipStreamCreateWithFlags(&d.st, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
    hipStream_t st = d.st;
    d.rp = dev_alloc<int>((size_t)n + 1);
    d.ci = dev_alloc<int>((size_t)std::max(nnz, 1));
    d.lambda = dev_alloc<int>((size_t)n);
    d.mark = dev_alloc<int>((size_t)n);
    d.ctr = dev_alloc<int>(2);
    d.ukey = dev_alloc<u64>((size_t)n);
    d.nbmax = dev_alloc<u64>((size_t)n);
    if (!d.rp || !d.ci || !d.lambda || !d.mark || !d.ctr || !d.ukey || !d.nbmax)
        return hip_fail(hipErrorOutOfMemory, "hipMalloc(PMIS arrays)", __FILE__, __LINE__);
    if (h2d(d.rp, S->row_ptr, sizeof(int) * ((size_t)n + 1))) return ERROR_MISC;
    if (nnz > 0 && h2d(d.ci, S->col_idx, sizeof(int) * (size_t)nnz)) return ERROR_MISC;

    SSS_HIP(hipMemsetAsync(d.lambda, 0, sizeof(int) * (size_t)n, st));
    SSS_HIP(hipMemsetAsync(d.ctr, 0, sizeof(int) * 2, st));
    if (nnz > 0)
        hipLaunchKernelGGL(pmis_lambda, dim3((unsigned)(((long long)nnz + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           (long long)nnz, n, d.ci, d.lambda);
    hipLaunchKernelGGL(pmis_init, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, n, d.rp, d.lambda,
                       d.mark, d.ukey, d.nbmax, d.ctr);
    SSS_HIP(hipGetLastError());
    int h_ctr[2] = {0, 0};   // {undecided, C points}
    if (copy_sync(h_ctr, d.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st)) return ERROR_MISC;

    const int G = lanes_for(n, nnz);
    int nrounds = 0;
    while (h_ctr[0] > 0) {
        if (nrounds == kPmisMaxRounds) {
            fprintf(stderr, "[sss_hip] PMIS split: %d points undecided after %d rounds\n", h_ctr[0], nrounds);
            return ERROR_UNKNOWN;
        }
        ++nrounds;
        switch (G) {
        case 1: launch_round<1>(n, nnz, d.rp, d.ci, d.mark, d.ukey, d.nbmax, d.ctr, st); break;
        case 4: launch_round<4>(n, nnz, d.rp, d.ci, d.mark, d.ukey, d.nbmax, d.ctr, st); break;
        case 16: launch_round<16>(n, nnz, d.rp, d.ci, d.mark, d.ukey, d.nbmax, d.ctr, st); break;
        default: launch_round<64>(n, nnz, d.rp, d.ci, d.mark, d.ukey, d.nbmax, d.ctr, st); break;
        }
        SSS_HIP(hipGetLastError());
        if (copy_sync(h_ctr, d.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, st)) return ERROR_MISC;
    }
    // into a buffer of its own first: mark stays untouched if the copy fails
    HostBuf<int> out;
    out.resize((size_t)n);
    if (copy_sync(out.data(), d.mark, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st)) return ERROR_MISC;
    parallel_chunks(n, 1 << 20, [&](int lo, int hi) { memcpy(mark + lo, out.data() + lo, sizeof(int) * (size_t)(hi - lo)); });
    if (ncoarse) *ncoarse = h_ctr[1];
    if (rounds) *rounds = nrounds;
    return 0;
}
