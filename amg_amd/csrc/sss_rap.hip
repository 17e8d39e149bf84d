// sss_rap.hip — the Galerkin product A_c = R A P of the setup on the GPU, bit for bit the
// reference's SSS_blas_mat_rap (SSS_matvec.c:398-534; host restatement amg_amd/host/sss_setup.c).
//
// The reference builds coarse row ic by walking, in order, every R entry (q1), every A entry of
// that fine row (q2) and every P entry of the reached fine row (q3), and
//   * the diagonal (ic, ic) is the row's first entry, starting from 0.0 (every product adds),
//   * any other column takes the row's next slot on its first product (assigned), later products
//     of that column add (+=), in walk order,
//   * ra = r * a, rap = ra * p (two roundings, no contraction).
// Its A-marker only skips re-checking columns it has already met, so "first product of a column
// opens a slot, every later one adds" is the whole rule.
//
// Here G lanes walk one coarse row: the (q1, q2) steps go in order, the P row of each step is
// spread over the G lanes (its columns are distinct, so no slot is touched twice in one step and
// every slot still receives its products in walk order).  New columns of a step take consecutive
// slots in q3 order (a ballot prefix).  Columns -> slots live in an LDS hash table per row, values
// and columns in LDS slot arrays; pass 0 counts each row's slots, pass 1 (after the host prefix
// sum) fills the rows.  A row with more slots than its table holds is retried with a larger
// per-row table, and the few left after the largest one are built on the host (the same walk).
#include "sss_engine.hpp"

#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>

namespace sss {

namespace {

constexpr unsigned kEmpty = 0xffffffffu;

__device__ __forceinline__ unsigned rap_hash(unsigned c, int hs) { return (c * 0x9E3779B1u) >> 7 & (unsigned)(hs - 1); }

// One launch: rows list[0 .. nrows) (coarse row ids), G lanes per row, VS slots per row.
// MODE 0: cnt[t] = the row's slot count, or -1 if it needs more than VS slots.
// MODE 1: the row written at C[start[row] ..) (cols, vals).
template <int G, int VS, int RPB, int MODE>
__global__ __launch_bounds__(G * RPB) void rap_rows(int nrows, const int *__restrict__ list, const int *__restrict__ rrp,
                                                const int *__restrict__ rci, const double *__restrict__ rv,
                                                const int *__restrict__ arp, const int *__restrict__ aci,
                                                const double *__restrict__ av, const int *__restrict__ prp,
                                                const int *__restrict__ pci, const double *__restrict__ pv,
                                                int *__restrict__ cnt, const long long *__restrict__ start,
                                                int *__restrict__ cci, double *__restrict__ cval)
{
    constexpr int HS = 2 * VS;
    __shared__ unsigned hkey[RPB][HS];
    __shared__ int hslot[RPB][HS];
    __shared__ int scol[RPB][MODE == 1 ? VS : 1];
    __shared__ double sval[RPB][MODE == 1 ? VS : 1];
    const int lane = threadIdx.x & 63, g = threadIdx.x / G, gl = threadIdx.x % G;
    const int gbase = lane - gl;   // first lane of this row's group within the wave
    const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << gbase;
    const int t = blockIdx.x * RPB + g;
    const bool live = t < nrows;
    const int ic = live ? (list ? list[t] : t) : 0;
    unsigned *hk = hkey[g];
    int *hs = hslot[g];
    for (int k = gl; k < HS; k += G) hk[k] = kEmpty;
    __syncthreads();
    int nslots = 0;
    bool over = false;
    if (live) {
        // the diagonal: slot 0, value 0.0
        if (gl == 0) {
            const unsigned h = rap_hash((unsigned)ic, HS);
            hk[h] = (unsigned)ic;
            hs[h] = 0;
            if (MODE == 1) scol[g][0] = ic, sval[g][0] = 0.0;
        }
        nslots = 1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int q1 = rrp[ic]; q1 < rrp[ic + 1] && !over; ++q1) {
            const double r = rv[q1];
            const int i1 = rci[q1];
            const int a0 = arp[i1], a1 = arp[i1 + 1];
            for (int ab = a0; ab < a1 && !over; ab += G) {
                // this chunk's A entries and their P row bounds, one per lane
                int i2 = 0, p0 = 0, p1 = 0;
                double a = 0.0;
                if (ab + gl < a1) {
                    i2 = aci[ab + gl];
                    a = av[ab + gl];
                    p0 = prp[i2];
                    p1 = prp[i2 + 1];
                }
                const int ne = min(G, a1 - ab);
                for (int e = 0; e < ne && !over; ++e) {
                    const double ae = __shfl(a, gbase + e, 64);
                    const int e0 = __shfl(p0, gbase + e, 64), e1 = __shfl(p1, gbase + e, 64);
                    const double ra = r * ae;
                    for (int pb = e0; pb < e1; pb += G) {
                        const int q3 = pb + gl;
                        const bool act = q3 < e1;
                        unsigned col = 0;
                        double rap = 0.0;
                        if (act) {
                            col = (unsigned)pci[q3];
                            if (MODE == 1) rap = ra * pv[q3];
                        }
                        // look the column up (read-only in this phase)
                        int slot = -1;
                        unsigned h = rap_hash(col, HS);
                        if (act) {
                            for (;;) {
                                const unsigned k = hk[h];
                                if (k == col) {
                                    slot = hs[h];
                                    break;
                                }
                                if (k == kEmpty) break;
                                h = (h + 1) & (HS - 1);
                            }
                        }
                        const bool fresh = act && slot < 0;
                        const unsigned long long m = __ballot(fresh) & gmask;
                        const int nnew = __popcll(m);
                        if (nslots + nnew > VS) {
                            over = true;
                            break;
                        }
                        __builtin_amdgcn_wave_barrier();
                        if (fresh) {
                            slot = nslots + __popcll(m & ((1ull << lane) - 1));
                            for (;;) {   // claim an empty bucket from h on (keys of one step are distinct)
                                const unsigned old = atomicCAS(&hk[h], kEmpty, col);
                                if (old == kEmpty) break;
                                h = (h + 1) & (HS - 1);
                            }
                            hs[h] = slot;
                            if (MODE == 1) scol[g][slot] = (int)col, sval[g][slot] = rap;
                        } else if (act && MODE == 1) {
                            sval[g][slot] += rap;
                        }
                        nslots += nnew;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    }
                }
            }
        }
        if (MODE == 0) {
            if (gl == 0) cnt[t] = over ? -1 : nslots;
        } else if (!over) {
            const long long s0 = start[ic];
            for (int k = gl; k < nslots; k += G) {
                cci[s0 + k] = scol[g][k];
                cval[s0 + k] = sval[g][k];
            }
        }
    }
}

// sss_hip_rap_values: the same walk on a row whose pattern is known.  The row's column -> slot
// table is filled from the row of C itself (a column's slot is its position in the row), the
// diagonal's slot starts at 0.0 and every other one at -0.0, and every product adds: x + -0.0 is x
// for every x (-0.0 included), so the first product of a slot lands as the reference's assignment
// does.  One pass, no slot counting.  flag bits: 1 a product's column is absent from the row of C,
// 2 an index out of range or a row of C that does not start with its diagonal / repeats a column.
template <int G, int VS, int RPB>
__global__ __launch_bounds__(G * RPB) void rap_rows_values(int nrows, const int *__restrict__ list, int nc, int nf, int np,
                                                       const int *__restrict__ rrp, const int *__restrict__ rci,
                                                       const double *__restrict__ rv, const int *__restrict__ arp,
                                                       const int *__restrict__ aci, const double *__restrict__ av,
                                                       const int *__restrict__ prp, const int *__restrict__ pci,
                                                       const double *__restrict__ pv, const int *__restrict__ crp,
                                                       const int *__restrict__ cci, double *__restrict__ cval,
                                                       unsigned *__restrict__ flag)
{
    constexpr int HS = 2 * VS;
    __shared__ unsigned hkey[RPB][HS];
    __shared__ int hslot[RPB][HS];
    __shared__ double sval[RPB][VS];
    const int lane = threadIdx.x & 63, g = threadIdx.x / G, gl = threadIdx.x % G;
    const int gbase = lane - gl;   // first lane of this row's group within the wave
    const int t = blockIdx.x * RPB + g;
    const bool live = t < nrows;
    const int ic = live ? list[t] : 0;
    unsigned *hk = hkey[g];
    int *hs = hslot[g];
    for (int k = gl; k < HS; k += G) hk[k] = kEmpty;
    __syncthreads();
    if (!live || ic < 0 || ic >= nc) {
        if (live && gl == 0) atomicOr(flag, 2u);
        return;
    }
    const int c0 = crp[ic];
    const int len = crp[ic + 1] - c0;
    if (len < 1 || len > VS || cci[c0] != ic) {   // (the host sorted the rows by length: never too long)
        if (gl == 0) atomicOr(flag, 2u);
        return;
    }
    unsigned bad = 0;
    for (int k = gl; k < len; k += G) {
        const int c = cci[c0 + k];
        sval[g][k] = k == 0 ? 0.0 : -0.0;
        if (c < 0 || c >= nc) {
            bad |= 2u;
            continue;
        }
        unsigned h = rap_hash((unsigned)c, HS);
        for (;;) {   // at most VS keys in 2 VS buckets: an empty one is always reached
            const unsigned old = atomicCAS(&hk[h], kEmpty, (unsigned)c);
            if (old == kEmpty) {
                hs[h] = k;
                break;
            }
            if (old == (unsigned)c) {   // a column twice in the row
                bad |= 2u;
                break;
            }
            h = (h + 1) & (HS - 1);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int q1 = rrp[ic]; q1 < rrp[ic + 1]; ++q1) {
        const double r = rv[q1];
        const int i1 = rci[q1];
        if (i1 < 0 || i1 >= nf) {   // (uniform over the group)
            bad |= 2u;
            continue;
        }
        const int a0 = arp[i1], a1 = arp[i1 + 1];
        for (int ab = a0; ab < a1; ab += G) {
            // this chunk's A entries and their P row bounds, one per lane
            int p0 = 0, p1 = 0;
            double a = 0.0;
            if (ab + gl < a1) {
                const int i2 = aci[ab + gl];
                a = av[ab + gl];
                if (i2 < 0 || i2 >= np) bad |= 2u;   // (p0 == p1: the entry is skipped)
                else p0 = prp[i2], p1 = prp[i2 + 1];
            }
            const int ne = min(G, a1 - ab);
            for (int e = 0; e < ne; ++e) {
                const double ae = __shfl(a, gbase + e, 64);
                const int e0 = __shfl(p0, gbase + e, 64), e1 = __shfl(p1, gbase + e, 64);
                const double ra = r * ae;
                for (int pb = e0; pb < e1; pb += G) {
                    const int q3 = pb + gl;
                    if (q3 < e1) {
                        const unsigned col = (unsigned)pci[q3];
                        const double rap = ra * pv[q3];
                        int slot = -1;
                        unsigned h = rap_hash(col, HS);
                        for (;;) {
                            const unsigned k = hk[h];
                            if (k == col) {
                                slot = hs[h];
                                break;
                            }
                            if (k == kEmpty) break;
                            h = (h + 1) & (HS - 1);
                        }
                        // the columns of one P row are distinct: no slot is touched twice in a step
                        if (slot >= 0) sval[g][slot] += rap;
                        else bad |= 1u;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                }
            }
        }
    }
    if (bad) atomicOr(flag, bad);
    for (int k = gl; k < len; k += G) cval[c0 + k] = sval[g][k];
}

struct DevMat {
    int *rp = nullptr, *ci = nullptr;
    double *v = nullptr;
    ~DevMat()
    {
        dev_free(rp);
        dev_free(ci);
        dev_free(v);
    }
    int up(const SSS_MAT &M)
    {
        const char *what = "hipMalloc(RAP operand)";
        if (int rc = dev_upload(rp, M.row_ptr, (size_t)M.num_rows + 1, what)) return rc;
        if (int rc = dev_upload(ci, M.col_idx, (size_t)M.num_nnzs, what)) return rc;
        return dev_upload(v, M.val, (size_t)M.num_nnzs, what);
    }
};

// the host walk of one coarse row (the reference's, sss_setup.c SSS_blas_mat_rap), for the rows no
// device table holds: count (out == nullptr) or fill at cci/cval.  mark/slot: nc ints, mark[] != ic.
// mk: a marker value no other row walk of this mark array used
int host_row(int ic, int mk, const SSS_MAT &R, const SSS_MAT &A, const SSS_MAT &P, int *mark, int *slot, int *cci,
             double *cval)
{
    int n = 0;
    mark[ic] = mk;
    slot[ic] = 0;
    if (cci) cci[0] = ic, cval[0] = 0.0;
    n = 1;
    for (int q1 = R.row_ptr[ic]; q1 < R.row_ptr[ic + 1]; ++q1) {
        const double r = R.val[q1];
        const int i1 = R.col_idx[q1];
        for (int q2 = A.row_ptr[i1]; q2 < A.row_ptr[i1 + 1]; ++q2) {
            const double ra = r * A.val[q2];
            const int i2 = A.col_idx[q2];
            for (int q3 = P.row_ptr[i2]; q3 < P.row_ptr[i2 + 1]; ++q3) {
                const int i3 = P.col_idx[q3];
                if (mark[i3] != mk) {
                    mark[i3] = mk;
                    slot[i3] = n;
                    if (cci) cci[n] = i3, cval[n] = ra * P.val[q3];
                    ++n;
                } else if (cci) {
                    cval[slot[i3]] += ra * P.val[q3];
                }
            }
        }
    }
    return n;
}

template <int G, int VS, int RPB, int MODE>
void launch_rows(int nrows, const int *list, const DevMat &R, const DevMat &A, const DevMat &P, int *cnt,
                 const long long *start, int *cci, double *cval, hipStream_t st)
{
    if (nrows <= 0) return;
    hipLaunchKernelGGL((rap_rows<G, VS, RPB, MODE>), dim3((nrows + RPB - 1) / RPB), dim3(G * RPB), 0, st, nrows,
                       list, R.rp, R.ci, R.v, A.rp, A.ci, A.v, P.rp, P.ci, P.v, cnt, start, cci, cval);
}
// table configurations, each for the rows the previous one could not hold: lanes per row, slots
// per row (LDS 28 B per slot), rows per workgroup
template <int MODE>
void launch_cfg(int c, int nrows, const int *list, const DevMat &R, const DevMat &A, const DevMat &P, int *cnt,
                const long long *start, int *cci, double *cval, hipStream_t st)
{
    switch (c) {
    case 0: launch_rows<8, 32, 32, MODE>(nrows, list, R, A, P, cnt, start, cci, cval, st); break;
    case 1: launch_rows<16, 128, 16, MODE>(nrows, list, R, A, P, cnt, start, cci, cval, st); break;
    case 2: launch_rows<64, 512, 4, MODE>(nrows, list, R, A, P, cnt, start, cci, cval, st); break;
    default: launch_rows<64, 4096, 1, MODE>(nrows, list, R, A, P, cnt, start, cci, cval, st); break;
    }
}
// copies on the product's own stream (non-blocking: the mirror worker's uploads, which may run
// at the same time on the default stream, neither wait for it nor hold it up)
int copy_sync(void *dst, const void *src, size_t bytes, hipMemcpyKind k, hipStream_t st)
{
    if (bytes == 0) return 0;
    SSS_HIP(hipMemcpyAsync(dst, src, bytes, k, st));
    SSS_HIP(hipStreamSynchronize(st));
    return 0;
}
constexpr int kCfgs = 4;
constexpr int kCfgSlots[kCfgs] = {32, 128, 512, 4096};   // VS of launch_cfg's configurations

template <int G, int VS, int RPB>
void launch_values(int nrows, const int *list, const SSS_MAT &Ch, const DevMat &R, const DevMat &A, const DevMat &P,
                   const int *crp, const int *cci, double *cval, unsigned *flag, int nf, int np, hipStream_t st)
{
    if (nrows <= 0) return;
    hipLaunchKernelGGL((rap_rows_values<G, VS, RPB>), dim3((nrows + RPB - 1) / RPB), dim3(G * RPB), 0, st, nrows, list,
                       Ch.num_rows, nf, np, R.rp, R.ci, R.v, A.rp, A.ci, A.v, P.rp, P.ci, P.v, crp, cci, cval, flag);
}
void launch_values_cfg(int c, int nrows, const int *list, const SSS_MAT &Ch, const DevMat &R, const DevMat &A,
                       const DevMat &P, const int *crp, const int *cci, double *cval, unsigned *flag, int nf, int np,
                       hipStream_t st)
{
    switch (c) {
    case 0: launch_values<8, 32, 32>(nrows, list, Ch, R, A, P, crp, cci, cval, flag, nf, np, st); break;
    case 1: launch_values<16, 128, 16>(nrows, list, Ch, R, A, P, crp, cci, cval, flag, nf, np, st); break;
    case 2: launch_values<64, 512, 4>(nrows, list, Ch, R, A, P, crp, cci, cval, flag, nf, np, st); break;
    default: launch_values<64, 4096, 1>(nrows, list, Ch, R, A, P, crp, cci, cval, flag, nf, np, st); break;
    }
}

// the values of one coarse row on the host (sss_rap_values_host's walk, sss_setup.c), for the rows
// longer than the largest device table: out[0 .. row length).  mark/slot: nc ints, mark[] != ic
// on entry.  false: an index out of range or a product whose column the row of C does not hold.
bool host_row_values(int ic, const SSS_MAT &R, const SSS_MAT &A, const SSS_MAT &P, const SSS_MAT &C, int *mark, int *slot,
                     double *out)
{
    const int nc = C.num_rows, c0 = C.row_ptr[ic], len = C.row_ptr[ic + 1] - c0;
    if (len < 1 || C.col_idx[c0] != ic) return false;
    for (int k = 0; k < len; ++k) {
        const int c = C.col_idx[c0 + k];
        if (c < 0 || c >= nc || mark[c] == ic) return false;
        mark[c] = ic;
        slot[c] = k;
        out[k] = k == 0 ? 0.0 : -0.0;
    }
    for (int q1 = R.row_ptr[ic]; q1 < R.row_ptr[ic + 1]; ++q1) {
        const double r = R.val[q1];
        const int i1 = R.col_idx[q1];
        if (i1 < 0 || i1 >= A.num_rows) return false;
        for (int q2 = A.row_ptr[i1]; q2 < A.row_ptr[i1 + 1]; ++q2) {
            const double ra = r * A.val[q2];
            const int i2 = A.col_idx[q2];
            if (i2 < 0 || i2 >= P.num_rows) return false;
            for (int q3 = P.row_ptr[i2]; q3 < P.row_ptr[i2 + 1]; ++q3) {
                const int i3 = P.col_idx[q3];
                if (i3 < 0 || i3 >= nc || mark[i3] != ic) return false;
                out[slot[i3]] += ra * P.val[q3];
            }
        }
    }
    return true;
}

// row pointers of an n-row matrix with nnz entries: 0 first, nnz last, never falling
bool row_ptr_ok(const SSS_MAT &M)
{
    if (M.num_rows < 0 || M.num_nnzs < 0 || !M.row_ptr || M.row_ptr[0] != 0 || M.row_ptr[M.num_rows] != M.num_nnzs) return false;
    std::atomic<int> ok{1};
    parallel_chunks(M.num_rows, 1 << 16, [&](int lo, int hi) {
        for (int i = lo; i < hi; ++i)
            if (M.row_ptr[i + 1] < M.row_ptr[i]) ok = 0;
    });
    return ok != 0;
}

// seconds this thread's last product spent in copies (with allocations) and in kernels
thread_local double g_rap_times[2] = {0.0, 0.0};

}  // namespace

}  // namespace sss

using namespace sss;

// A_c = R A P on the current device (see the file header).  C receives SSS_calloc'd arrays (freed
// by SSS_mat_destroy).  Returns 0, or an error code with C untouched (the caller then runs the
// host product).
extern "C" int sss_hip_rap(const SSS_MAT *Rh, const SSS_MAT *Ah, const SSS_MAT *Ph, SSS_MAT *C)
{
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    const int nc = Rh->num_rows;
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream()
        {
            if (s) (void)hipStreamDestroy(s);
        }
    } stream;
    if (hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
    hipStream_t st = stream.s;
    DevMat R, A, P;
    const double t_begin = PhaseTimer::now();
    if (R.up(*Rh) || A.up(*Ah) || P.up(*Ph)) return ERROR_MISC;
    const double t_up = PhaseTimer::now();   // (sss_hip_rap_times: uploads and downloads against the rest)
    int *cnt = dev_alloc<int>((size_t)std::max(nc, 1));
    int *list = dev_alloc<int>((size_t)std::max(nc, 1));
    if (!cnt || !list) {
        dev_free(cnt);
        dev_free(list);
        return ERROR_MISC;
    }
    // pass 0 over the configurations, each on the rows the previous one could not hold
    std::vector<int> cfg_of((size_t)nc, -1), pending, h_cnt((size_t)std::max(nc, 1));
    std::vector<int> count((size_t)nc, 0);
    int rc = 0;
    const char *ce = getenv("SSS_HIP_RAP_CFGS");   // tests: fewer device tables, more host rows
    const int ncfg = (ce && *ce) ? std::max(0, std::min(kCfgs, atoi(ce))) : kCfgs;
    if (ncfg == 0) pending.resize((size_t)nc), std::iota(pending.begin(), pending.end(), 0);
    for (int c = 0; c < ncfg && !rc; ++c) {
        const int m = c == 0 ? nc : (int)pending.size();
        if (m == 0) break;
        if (c > 0 && copy_sync(list, pending.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, st)) rc = ERROR_MISC;
        launch_cfg<0>(c, m, c == 0 ? nullptr : list, R, A, P, cnt, nullptr, nullptr, nullptr, st);
        if (!rc && (hipGetLastError() != hipSuccess || copy_sync(h_cnt.data(), cnt, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st)))
            rc = ERROR_MISC;
        if (rc) break;
        std::vector<int> next;
        for (int t = 0; t < m; ++t) {
            const int ic = c == 0 ? t : pending[t];
            if (h_cnt[t] < 0) next.push_back(ic);
            else cfg_of[ic] = c, count[ic] = h_cnt[t];
        }
        pending.swap(next);
    }
    // rows no table held (wider than 4,096 entries): counted on the host, in parallel chunks
    // (markers: ic while counting, nc + ic while filling)
    std::vector<long long> start((size_t)nc + 1, 0);
    // one (mark, slot) pair of nc-sized arrays per worker, reused over its chunks and both passes
    // (the markers of distinct rows and passes never collide), not one per 64-row chunk
    std::mutex buf_mu;
    std::vector<std::unique_ptr<std::pair<std::vector<int>, std::vector<int>>>> bufs;
    std::vector<std::pair<std::vector<int>, std::vector<int>> *> idle;
    auto host_rows = [&](bool fill) {
        const int np = (int)pending.size();
        parallel_chunks(np, 64, [&](int a, int e) {
            std::pair<std::vector<int>, std::vector<int>> *bf;
            {
                std::lock_guard<std::mutex> lk(buf_mu);
                if (idle.empty()) {
                    bufs.push_back(std::make_unique<std::pair<std::vector<int>, std::vector<int>>>(
                        std::vector<int>((size_t)nc, -1), std::vector<int>((size_t)nc, 0)));
                    idle.push_back(bufs.back().get());
                }
                bf = idle.back();
                idle.pop_back();
            }
            int *mark = bf->first.data(), *slot = bf->second.data();
            for (int t = a; t < e; ++t) {
                const int ic = pending[t];
                if (fill) host_row(ic, nc + ic, *Rh, *Ah, *Ph, mark, slot, C->col_idx + start[ic], C->val + start[ic]);
                else count[ic] = host_row(ic, ic, *Rh, *Ah, *Ph, mark, slot, nullptr, nullptr);
            }
            std::lock_guard<std::mutex> lk(buf_mu);
            idle.push_back(bf);
        });
    };
    if (!rc && !pending.empty()) host_rows(false);
    for (int ic = 0; ic < nc; ++ic) start[ic + 1] = start[ic] + count[ic];
    if (!rc && start[nc] > INT32_MAX) rc = ERROR_MAT_SIZE;
    long long *d_start = nullptr;
    int *d_ci = nullptr;
    double *d_v = nullptr;
    if (!rc) {
        d_start = dev_alloc<long long>((size_t)nc + 1);
        d_ci = dev_alloc<int>((size_t)std::max<long long>(start[nc], 1));
        d_v = dev_alloc<double>((size_t)std::max<long long>(start[nc], 1));
        if (!d_start || !d_ci || !d_v ||
            copy_sync(d_start, start.data(), sizeof(long long) * ((size_t)nc + 1), hipMemcpyHostToDevice, st))
            rc = ERROR_MISC;
    }
    // pass 1 per configuration, on its rows
    for (int c = 0; c < kCfgs && !rc; ++c) {
        std::vector<int> rows;
        for (int ic = 0; ic < nc; ++ic)
            if (cfg_of[ic] == c) rows.push_back(ic);
        if (rows.empty()) continue;
        if (copy_sync(list, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice, st)) {
            rc = ERROR_MISC;
            break;
        }
        launch_cfg<1>(c, (int)rows.size(), list, R, A, P, nullptr, d_start, d_ci, d_v, st);
        if (hipGetLastError() != hipSuccess) rc = ERROR_MISC;
    }
    if (!rc && hipStreamSynchronize(st) != hipSuccess) rc = ERROR_MISC;
    const double t_kern = PhaseTimer::now();
    if (!rc) {
        const int nnz = (int)start[nc];
        C->num_rows = nc;
        C->num_cols = nc;
        C->num_nnzs = nnz;
        C->row_ptr = (int *)SSS_calloc((size_t)nc + 1, sizeof(int));
        C->col_idx = (int *)SSS_calloc((size_t)std::max(nnz, 1), sizeof(int));
        C->val = (double *)SSS_calloc((size_t)std::max(nnz, 1), sizeof(double));
        for (int ic = 0; ic <= nc; ++ic) C->row_ptr[ic] = (int)start[ic];
        if (nnz > 0 && (copy_sync(C->col_idx, d_ci, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, st) ||
                        copy_sync(C->val, d_v, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, st)))
            rc = ERROR_MISC;
        if (!rc && !pending.empty()) host_rows(true);   // the host-built rows
        if (rc) SSS_mat_destroy(C);
    }
    dev_free(cnt);
    dev_free(list);
    dev_free(d_start);
    dev_free(d_ci);
    dev_free(d_v);
    g_rap_times[0] = (t_up - t_begin) + (PhaseTimer::now() - t_kern);
    g_rap_times[1] = t_kern - t_up;
    return rc;
}

// The values of C = R A P on C's own pattern (see rap_rows_values).  The rows are dealt to the table
// configurations by their length in C, each configuration is one launch, rows longer than the
// largest table allowed (SSS_HIP_RAP_CFGS, as in sss_hip_rap) are walked on the host while the
// kernels run.  The kernels write a device buffer and the host rows a side buffer; C->val receives
// them only when every row has succeeded (the download is then the call's last step that can fail:
// a device lost in it leaves C->val partly written).
extern "C" int sss_hip_rap_values(const SSS_MAT *Rh, const SSS_MAT *Ah, const SSS_MAT *Ph, SSS_MAT *C)
{
    g_rap_times[0] = g_rap_times[1] = 0.0;
    if (!Rh || !Ah || !Ph || !C || !C->row_ptr || !C->col_idx || !C->val) return ERROR_INPUT_PAR;
    const int nc = Rh->num_rows;
    if (nc <= 0 || C->num_rows != nc || C->num_cols != nc || Ph->num_cols != nc || Rh->num_cols != Ah->num_rows ||
        Ah->num_cols != Ph->num_rows || C->num_nnzs < nc)
        return ERROR_INPUT_PAR;
    if (sss_hip_device_count() <= 0) return ERROR_MISC;
    if (!row_ptr_ok(*Rh) || !row_ptr_ok(*Ah) || !row_ptr_ok(*Ph) || !row_ptr_ok(*C)) return ERROR_DATA_STRUCTURE;
    const int nnz = C->num_nnzs;
    const char *ce = getenv("SSS_HIP_RAP_CFGS");   // tests: fewer device tables, more host rows
    const int ncfg = (ce && *ce) ? std::max(0, std::min(kCfgs, atoi(ce))) : kCfgs;
    // the rows of each configuration, back to back in one list; then the host's
    int cfg_n[kCfgs + 1] = {0, 0, 0, 0, 0}, cfg_at[kCfgs + 2] = {0, 0, 0, 0, 0, 0};
    auto cfg_of = [&](int ic) {
        const int len = C->row_ptr[ic + 1] - C->row_ptr[ic];
        int c = 0;
        while (c < ncfg && len > kCfgSlots[c]) ++c;
        return c < ncfg ? c : kCfgs;
    };
    for (int ic = 0; ic < nc; ++ic) ++cfg_n[cfg_of(ic)];
    for (int c = 0; c <= kCfgs; ++c) cfg_at[c + 1] = cfg_at[c] + cfg_n[c];
    std::vector<int> rows((size_t)nc);
    {
        int at[kCfgs + 1];
        std::copy(cfg_at, cfg_at + kCfgs + 1, at);
        for (int ic = 0; ic < nc; ++ic) rows[(size_t)at[cfg_of(ic)]++] = ic;
    }
    const int ndev = cfg_at[kCfgs], nhost = cfg_n[kCfgs];
    const int *hrows = rows.data() + ndev;
    std::vector<long long> hstart((size_t)nhost + 1, 0);   // the host rows' places in their side buffer
    for (int t = 0; t < nhost; ++t) hstart[(size_t)t + 1] = hstart[t] + (C->row_ptr[hrows[t] + 1] - C->row_ptr[hrows[t]]);
    HostBuf<double> hvals;
    hvals.resize((size_t)std::max<long long>(hstart[nhost], 1));
    std::atomic<int> host_ok{1};
    auto host_rows = [&] {
        parallel_chunks(nhost, 64, [&](int a, int e) {
            std::vector<int> mark((size_t)nc, -1), slot((size_t)nc, 0);
            for (int t = a; t < e && host_ok; ++t)
                if (!host_row_values(hrows[t], *Rh, *Ah, *Ph, *C, mark.data(), slot.data(), hvals.data() + hstart[t])) host_ok = 0;
        });
    };
    struct Stream {
        hipStream_t s = nullptr;
        ~Stream()
        {
            if (s) (void)hipStreamDestroy(s);
        }
    } stream;
    int rc = 0;
    double t_copy = 0.0, t_kern = 0.0;
    if (ndev == 0) host_rows();
    if (ndev > 0) {
        double t0 = PhaseTimer::now();
        if (hipStreamCreateWithFlags(&stream.s, hipStreamNonBlocking) != hipSuccess) return ERROR_MISC;
        hipStream_t st = stream.s;
        DevMat R, A, P;
        int *d_crp = nullptr, *d_cci = nullptr, *d_list = nullptr;
        double *d_v = nullptr;
        unsigned *d_flag = nullptr, h_flag = 0;
        const char *what = "hipMalloc(RAP values)";
        if (R.up(*Rh) || A.up(*Ah) || P.up(*Ph) || dev_upload(d_crp, C->row_ptr, (size_t)nc + 1, what) ||
            dev_upload(d_cci, C->col_idx, (size_t)nnz, what) || dev_upload(d_list, rows.data(), (size_t)ndev, what))
            rc = ERROR_MISC;
        if (!rc) {
            d_v = dev_alloc<double>((size_t)std::max(nnz, 1));
            d_flag = dev_alloc<unsigned>(1);
            if (!d_v || !d_flag || hipMemsetAsync(d_flag, 0, sizeof(unsigned), st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                rc = ERROR_MISC;
        }
        double t1 = PhaseTimer::now();
        t_copy += t1 - t0;
        for (int c = 0; c < kCfgs && !rc; ++c) {
            launch_values_cfg(c, cfg_n[c], d_list + cfg_at[c], *C, R, A, P, d_crp, d_cci, d_v, d_flag, Ah->num_rows,
                              Ph->num_rows, st);
            if (hipGetLastError() != hipSuccess) rc = ERROR_MISC;
        }
        host_rows();   // (beside the kernels)
        if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = ERROR_MISC;
        t0 = PhaseTimer::now();
        t_kern += t0 - t1;
        if (!rc && copy_sync(&h_flag, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, st)) rc = ERROR_MISC;
        if (!rc && (h_flag || !host_ok)) rc = ERROR_DATA_STRUCTURE;
        if (!rc && copy_sync(C->val, d_v, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, st)) rc = ERROR_MISC;
        dev_free(d_crp);
        dev_free(d_cci);
        dev_free(d_list);
        dev_free(d_v);
        dev_free(d_flag);
        t_copy += PhaseTimer::now() - t0;
    }
    if (!rc && !host_ok) rc = ERROR_DATA_STRUCTURE;
    if (!rc)
        parallel_chunks(nhost, 64, [&](int a, int e) {
            for (int t = a; t < e; ++t)
                std::memcpy(C->val + C->row_ptr[hrows[t]], hvals.data() + hstart[t], sizeof(double) * (size_t)(hstart[t + 1] - hstart[t]));
        });
    g_rap_times[0] = t_copy;
    g_rap_times[1] = t_kern;
    return rc;
}

// (engine-internal, for the refresh's timing line and tools/refresh_measure.py)
extern "C" void sss_hip_rap_times(double *out)
{
    out[0] = g_rap_times[0];
    out[1] = g_rap_times[1];
}
