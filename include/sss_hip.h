/*
 * sss_hip.h — C ABI of the gfx950 device engine behind the drop-in solve path.
 *
 * The host C side (amg_amd/host/sss_solve.c) implements the reference's SSS_amg_solve loop
 * (Solve/SSS_SOLVE.c:53-80) on top of these calls; bench.py and the GPU tests call them
 * through ctypes.  Plain pointers and sizes only.  All functions return 0 on success and a
 * negative SSS_ERROR_CODE on failure (ERROR_MISC for HIP/RCCL errors, with a message on
 * stderr), except where noted.
 *
 * Reference interfaces these replace (amg/ tree):
 *   sss_hip_cycle ............ SSS_amg_cycle                Solve/SSS_cycle.cu:848-967
 *   sss_hip_residual_norm .... r = b - A*x; ||r||            Solve/SSS_SOLVE.c:59-64
 *   sss_hip_coarse_solve ..... SSS_amg_coarest_solve        Solve/SSS_cycle.cu:819-846
 *   sss_hip_smooth ........... SSS_amg_smoother_pre/post    Solve/SSS_smooth.c:138-304
 *   sss_hip_csr_spmv ......... SSS_blas_mv_amxpy/_mxy, spmv_cuda/alpha_spmv_cuda
 *                              SSS_utils.c:161-201, Solve/SSS_cuda.cu:77-165
 */
#ifndef SSS_HIP_H
#define SSS_HIP_H

#include "sss_amg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- engine options ------------------------------------------------------------------ */
enum {
    SSS_HIP_SMOOTH_EXACT = 0,    /* reference GS-CF on every level (level-scheduled, bitwise) */
    SSS_HIP_SMOOTH_HYBRID = 1,   /* exact GS-CF on level 0 when its C and F classes are independent
                                    sets (red-black: no chains), else two-stage GS-CF there;
                                    C/F-Jacobi (two-stage from inner_from) below */
    SSS_HIP_SMOOTH_JACOBI = 2    /* C/F-Jacobi on every level */
};
enum {
    SSS_HIP_COARSE_KRYLOV = 0,   /* reference CG(beta==1)+GMRES(30), on device */
    SSS_HIP_COARSE_DIRECT = 1    /* explicit inverse of the coarsest operator, one GEMV */
};
enum { SSS_HIP_VEC_B = 0, SSS_HIP_VEC_X = 1, SSS_HIP_VEC_WP = 2 };

typedef struct sss_hip_opts {
    int device;        /* HIP device ordinal; -1 = keep current */
    int smoother;      /* SSS_HIP_SMOOTH_* */
    int coarse;        /* SSS_HIP_COARSE_* */
    int row_cap;       /* 0 = uncapped coarse SpMV; 4096 reproduces <<<64,64>>> (as shipped) */
    int use_graph;     /* capture the V-cycle into a hipGraph once and replay it */
    int verbose;       /* engine diagnostics on stderr */
    int inner;         /* C/F-Jacobi levels: 0 = plain C/F-Jacobi; k > 0 = two-stage GS-CF with k
                          Jacobi-Richardson steps on each pass's same-class lower triangle */
    int inner_from;    /* first level that uses the two-stage form (plain C/F-Jacobi above it) */
    int relabel;       /* renumber levels F-first/C-second on the device (bitwise-neutral):
                          0 off, 1 every level but the coarsest, 2 as 1 but level 0 kept */
    int sorted_tiles;  /* store each SpMV/relaxation staging tile column-sorted with its stored
                          positions (x gathers coalesce across rows; sums unchanged, bitwise) */
    int sum_order;     /* 0: every row sum in the reference's stored CSR order (bitwise);
                          1: rows of long-row levels (>= SSS_HIP_WAVE_MIN entries on average)
                          summed by a wave in a fixed tree order over column-sorted rows --
                          deterministic, within the reordered-summation bound of the reference,
                          not bitwise (throughput mode) */
    int inner_long;    /* extra Jacobi-Richardson steps on the two-stage levels of long rows (at least
                          SSS_HIP_LONG_ROW_MIN = 300 entries per row on average over the whole level):
                          their lower triangles are the densest, and the extra step keeps throughput
                          mode within the reference's iteration count + 2 at 7-pt 512^3 (default 1) */
    int formats;       /* storage formats of the uploaded operators (all bitwise-neutral): 0 = every
                          format a level qualifies for (dictionary / column ELL, dictionary and
                          column-sorted tiles); 1 = plain CSR tiles only (cheapest to build); -1 = auto
                          (default): 1 for the exact smoother, whose cycle is bound by the GS-CF chains,
                          so the formats would only lengthen the mirror's construction, else 0 */
} sss_hip_opts;

#define SSS_HIP_LONG_ROW_MIN 300
/* Defaults, overridable by environment: SSS_HIP_SMOOTHER=exact|hybrid|jacobi,
 * SSS_HIP_COARSE=krylov|direct, SSS_HIP_ROWCAP=<n>, SSS_HIP_GRAPH=0|1, SSS_HIP_DEVICE=<n>,
 * SSS_HIP_VERBOSE=0|1, SSS_HIP_RELABEL=0|1|2 (default 1), SSS_HIP_INNER=<k> (default 1),
 * SSS_HIP_SORTED_TILES=0|1 (default 1), SSS_HIP_SUM_ORDER=0|1 (default 0),
 * SSS_HIP_INNER_FROM=<level> (default 2), SSS_HIP_INNER_LONG=<k> (default 1),
 * SSS_HIP_FORMATS=auto|full|lean (default auto). */
void sss_hip_opts_default(sss_hip_opts *o);

/* Number of usable HIP devices (0 when none; never exits). */
int sss_hip_device_count(void);
/* Free and total HBM of the current device, in bytes (hipMemGetInfo). */
int sss_hip_mem_info(size_t *free_bytes, size_t *total_bytes);

/* ---- hierarchy mirror -------------------------------------------------------------- */
typedef struct sss_hip_hier sss_hip_hier;

/* Uploads every level of mg (A, P, R, cfmark; b/x/wp allocated) to HBM and builds the
 * smoother schedules.  mg->cg[0].x/.b may be unset. Returns NULL on failure. */
sss_hip_hier *sss_hip_hier_create(const SSS_AMG *mg, const sss_hip_opts *o);
void sss_hip_hier_destroy(sss_hip_hier *h);
/* mg is the hierarchy h mirrors, after SSS_amg_refresh: the value-dependent half of the mirror is
 * built again level by level -- A_l in its formats, the smoother plan, the coarse solver, the
 * single-workgroup tail, the captured graphs; a level's old A objects are released before its new
 * ones are built.  The stream, the relabelings, every level's vectors (the level-0 b and x keep
 * their contents), the Krylov workspaces and the P_l / R_l device objects are kept; a level whose
 * plan flag behind P's storage changed with the values rebuilds its P and R as well.  After a
 * return of 0 every engine call on h gives bitwise what it gives on a mirror newly created from mg
 * with h's options, and sss_hip_level_info_get agrees field for field.  Works on mirrors from
 * sss_hip_hier_create and sss_hip_setup_create.  On failure: an error code, and h is good only
 * for sss_hip_hier_destroy. */
int sss_hip_hier_refresh(sss_hip_hier *h, const SSS_AMG *mg);

/* SSS_amg_setup (Setup/SSS_SETUP.cu:36-178 semantics, same printed output, same mg) with the
 * mirror built while the setup runs: every level is relabeled and uploaded on a worker thread as
 * soon as the setup has moved past it, so the uploads overlap the setup's serial RS passes.
 * Equivalent to SSS_amg_setup(mg, A, pars) followed by sss_hip_hier_create(mg, o).  times
 * (optional, 3 doubles): setup seconds (uploads overlapped), seconds of mirror work after the
 * setup returned, of which waiting for the worker.  NULL on failure (mg is set up even then). */
sss_hip_hier *sss_hip_setup_create(SSS_AMG *mg, SSS_MAT *A, SSS_AMG_PARS *pars, const sss_hip_opts *o,
                                   double *times);

/* The setup's Galerkin product A_c = R A P (SSS_blas_mat_rap, SSS_matvec.c:398-534) on the GPU,
 * bit for bit the host product (same entries, same column order, same summation order).  C gets
 * SSS_calloc'd arrays.  Returns 0, or an error code with C untouched (no device, no memory).
 * The setup uses it, when a device is present, for levels with at least SSS_SETUP_GPU_RAP_MIN
 * nonzeros in A (default 10^6) and at most SSS_SETUP_GPU_RAP_MAXROW of them per row on average
 * (default 48); SSS_SETUP_GPU_RAP=0 keeps every product on the host. */
int sss_hip_rap(const SSS_MAT *R, const SSS_MAT *A, const SSS_MAT *P, SSS_MAT *C);
/* The values of that product on a pattern already known (SSS_amg_refresh).
 * C has row_ptr / col_idx of a product of operators with these patterns (SSS_blas_mat_rap or sss_hip_rap);
 * fills C->val with the values that product would give, bit for bit.  0, or an error code with C->val untouched
 * (ERROR_INPUT_PAR: shapes that do not fit; ERROR_DATA_STRUCTURE: an index out of range, a row of C that
 * does not start with its diagonal or repeats a column, a product whose column is absent from the
 * row of C; the device call also: no device, no memory, a failed copy -- the kernels write a device
 * buffer that is downloaded into C->val only after every row has succeeded, so only a device lost
 * during that last download can leave C->val partly written).
 * The rule "the first product of a column opens a slot, every later one adds" makes the pattern a
 * function of the three patterns alone, so here a row's column -> slot table is filled from the row
 * of C, the diagonal starts at 0.0 and every other slot at -0.0, and every product adds in the
 * reference's order (x + -0.0 is x for every x, -0.0 included).  One kernel pass on the device: no
 * count pass, no prefix sum, no retry; the table size is chosen from the row's length, rows longer than
 * the largest table (4,096; SSS_HIP_RAP_CFGS lowers it as for sss_hip_rap) are walked on the host. */
int sss_hip_rap_values(const SSS_MAT *R, const SSS_MAT *A, const SSS_MAT *P, SSS_MAT *C);
int sss_rap_values_host(const SSS_MAT *R, const SSS_MAT *A, const SSS_MAT *P, SSS_MAT *C);   /* OpenMP, row-parallel */

/* The PMIS C/F split (cs_type SSS_COARSE_PMIS; the rule: DESIGN.md "PMIS coarsening") of a compacted
 * strength matrix S (row_ptr, col_idx; square) on the GPU: S is uploaded, the rounds run as ordinary
 * launches steered by the host, mark (n ints: CGPT / FGPT / ISPT) is downloaded.  *ncoarse = the
 * C points, *rounds = the rounds it took (either may be NULL).  The marks depend on S alone and
 * equal the host split's.  Returns 0, or an error code with mark untouched (no device, no rows, no
 * memory, more than 4096 rounds); the setup then runs the host split.  The setup uses it, when a
 * device is present, for levels with at least SSS_SETUP_GPU_PMIS_MIN entries in S (default
 * SSS_SETUP_GPU_PMIS_MIN_DEFAULT = 10^7: measured at 7-pt 400^3, the device split with its copies
 * costs about 6 ms + 0.6 ns per entry, the host split on 16 threads 1.3 ns per entry, DESIGN.md
 * 6.4); SSS_SETUP_GPU_PMIS=0 keeps every split on the host. */
#define SSS_SETUP_GPU_PMIS_MIN_DEFAULT 10000000
int sss_hip_pmis(const SSS_IMAT *S, int *mark, int *ncoarse, int *rounds);
/* The same split on the host (OpenMP, row-parallel): what the setup runs without a device or on
 * small levels, and what the device split is tested against.  0 or an error code. */
int sss_pmis_host(const SSS_IMAT *S, int *mark, int *ncoarse, int *rounds);

/* The standard interpolation (interp_type intERP_STD) on the GPU, bit for bit the host
 * result.  sss_hip_std_pattern builds the pattern of form_P_pattern_std from a compacted S and the
 * marks: P gets row_ptr, col_idx (fine numbering, the host's discovery order), val zeroed, num_cols =
 * ncoarse.  sss_hip_interp_std computes interp_STD on such a pattern: the weights, the coarse
 * renumbering of the columns and the truncation; P's arrays are freed and replaced.  Each call uploads
 * what it reads and downloads what it produces; the output arrays are SSS_calloc'd.  Both return 0, or
 * an error code with P untouched (no device, no rows, no memory, a failed copy, input the kernels found
 * inconsistent: an index out of range, a strong column absent from the row of A, a C column absent
 * from the pattern row); the setup then runs the host code.  SSS_HIP_INTERP_LANES = 1, 4, 16 or 64
 * forces the lanes per row, SSS_HIP_INTERP_LDS_SLOTS lowers the per-row table kept in LDS (longer
 * rows use a table in global memory inside the same call).  Under SSS_SETUP_TIMING each call prints
 * one stderr line: lanes per row, rows on global tables, seconds of copies and of kernels.
 * The setup uses both, when a device is present, for levels whose A has at least
 * SSS_SETUP_GPU_INTERP_MIN nonzeros (default SSS_SETUP_GPU_INTERP_MIN_DEFAULT = 10^7: measured at 7-pt
 * 400^3 with PMIS marks, pattern and weights together cost about 4.4 ms + 1.4 ns per nonzero of A on the
 * device, copies included, and about 5 ns per nonzero on the host on 16 threads; they cross near 1.2 * 10^6,
 * rounded up to a power of ten); SSS_SETUP_GPU_INTERP=0 keeps both on the host. */
#define SSS_SETUP_GPU_INTERP_MIN_DEFAULT 10000000
int sss_hip_std_pattern(const SSS_IMAT *S, const int *mark, int ncoarse, SSS_MAT *P);
int sss_hip_interp_std(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold);
/* The extended+i interpolation (interp_type intERP_EXTI, an engine extension) on the GPU,
 * bit for bit the host's interp_EXTI, on a pattern as sss_hip_std_pattern builds it.  Per F row i with
 * pattern C_i, d = a_ii and hat a = 0, the stored entries (i, k), k != i, in stored order: k in C_i adds
 * a_ik to hat a_k; a strong F neighbour k (k in S_i, marked F) is eliminated through the entries (k, l)
 * of its row with l in C_i or l == i and a_kl a_kk < 0 (den their sum in stored order: f = a_ik / den,
 * f a_kl goes to d for l == i and to hat a_l otherwise; den == 0 adds a_ik to d); anything else adds
 * a_ik to d; p_ic = -hat a_c / d.  No alpha.  Then the coarse renumbering of the columns and the
 * truncation; P's arrays are freed and replaced.  The contract, the switches (SSS_HIP_INTERP_LANES,
 * SSS_HIP_INTERP_LDS_SLOTS, SSS_SETUP_GPU_INTERP, SSS_SETUP_GPU_INTERP_MIN) and the SSS_SETUP_TIMING line
 * are those of sss_hip_interp_std.  Returns 0, or an error code with P untouched: ERROR_INPUT_PAR (a NULL
 * or misshapen argument), ERROR_MAT_SIZE (too many rows for the grid), ERROR_MISC (no device, a failed
 * HIP call or copy), ERROR_DATA_STRUCTURE (input the kernels found inconsistent: an index out of range, a
 * strong column absent from the row of A, a full table); the setup then runs the host code. */
int sss_hip_interp_exti(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold);
/* The pattern on the host (OpenMP, row-parallel): what the setup runs without a device or on small
 * levels, and what the device pattern is tested against.  0 or an error code. */
int sss_std_pattern_host(const SSS_IMAT *S, const int *mark, int ncoarse, SSS_MAT *P);

/* Aggressive coarsening (cs_type SSS_COARSE_PMIS_AGG).  The distance-two graph S2 of the
 * C points of a stage-one split: one row per point with mark CGPT, numbered c(i) in increasing i; row
 * c(i) is one walk of S_i in stored order, for each k != i of S_i first k itself when it is a C point,
 * then, whatever k's mark, every C point l != i of S_k in stored order; a candidate is kept at its first
 * occurrence, in discovery order, as column c(l).  S2 gets num_rows = num_cols = the C points, row_ptr
 * and col_idx (the library's arrays: SSS_imat_destroy), val NULL.  sss_hip_agg_graph builds it on the
 * GPU (count, exclusive sum, fill; per-row hash tables as sss_hip_std_pattern, G lanes per row), array
 * for array the host's.  Both return 0, or an error code with S2 untouched: ERROR_INPUT_PAR,
 * ERROR_MAT_SIZE, ERROR_MISC (no device, a failed HIP call or copy), ERROR_DATA_STRUCTURE (an index out
 * of range, a full table).  All argument checks precede the first HIP call.  With SSS_SETUP_TIMING one
 * stderr line.  The setup uses the device graph, and then the device split of S2 under its own
 * SSS_SETUP_GPU_PMIS* switches on S2's entries, when a device is present and A has at least
 * SSS_SETUP_GPU_AGG_MIN nonzeros (default SSS_SETUP_GPU_AGG_MIN_DEFAULT = 10^7, the sibling switches'
 * value); SSS_SETUP_GPU_AGG=0 keeps both on the host. */
#define SSS_SETUP_GPU_AGG_MIN_DEFAULT 10000000
int sss_agg_graph_host(const SSS_IMAT *S, const int *mark, SSS_IMAT *S2);
int sss_hip_agg_graph(const SSS_IMAT *S, const int *mark, SSS_IMAT *S2);
/* The two-stage split on the host: the PMIS split of S, the PMIS split of S2, and the final marks (a
 * stage-one C point stays C when stage two made it C or its S2 row is empty, else it becomes F).  mark
 * (n ints) and *ncoarse are written on success only.  0 or an error code. */
int sss_pmis_agg_host(const SSS_IMAT *S, int *mark, int *ncoarse);
/* Multipass interpolation (interp_type intERP_MPASS; the rule: amg_amd/host/sss_setup.c mpass_build,
 * DESIGN.md 6.8) from A, a compacted S and the final marks, on the host (OpenMP, row-parallel per
 * pass): the pattern and the weights pass by pass, the coarse renumbering of the columns, the
 * truncation.  P (whatever it held is ignored, not freed) gets the library's arrays; *passes = the
 * largest pass number.  0, or an error code with P untouched. */
int sss_interp_mpass_host(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold,
                          int *passes);
/* The same on the GPU, bit for bit the host's P.  The pass numbers come from relaxation sweeps steered by
 * the host; then one round of ordinary launches per pass over that pass's rows, G lanes (1, 4, 16 or 64,
 * from the pass's average candidate bound, the entries of the rows of P of N_i) per row: first
 * occurrences by an atomicMin of the sequence number in the row's hash table, hat w in the same table
 * with one owner lane per slot and the terms handed over in walk order; d, tot and sub on every lane.
 * A pass writes its rows into a block of its own and reads the block of the pass before; P is assembled
 * in row order after the last pass, then renumbered and truncated as in sss_hip_interp_std.  Tables sit
 * in LDS, or in a global array allocated inside the call when a row's bound does not fit
 * (SSS_HIP_INTERP_LDS_SLOTS, SSS_HIP_INTERP_LANES as there).  Both forms want every strong column k != i
 * of a row present in the row of A.  Returns 0, or an error code with P untouched: ERROR_INPUT_PAR,
 * ERROR_MAT_SIZE, ERROR_MISC, ERROR_DATA_STRUCTURE; all argument checks precede the first HIP call.  The
 * setup uses it under the switches of sss_hip_interp_std (SSS_SETUP_GPU_INTERP, SSS_SETUP_GPU_INTERP_MIN)
 * and runs the host form on any error code.  With SSS_SETUP_TIMING one stderr line. */
int sss_hip_interp_mpass(const SSS_MAT *A, const SSS_IMAT *S, const int *mark, SSS_MAT *P, double trunc_threshold,
                         int *passes);
/* The cap on the entries per row of P, an engine extension that is off by default:
 * SSS_SETUP_PMAX=<n> in the environment, n > 0; anything else (unset, not a number, <= 0) is 0 = off.
 * SSS_AMG_PARS keeps the reference's layout, so the value cannot live there.  SSS_amg_interp_trunc,
 * sss_interp_mpass_host and the device interpolations (sss_hip_interp_std, sss_hip_interp_exti,
 * sss_hip_interp_mpass) read it through this helper. */
int sss_setup_pmax(void);
/* The truncation of an interpolation matrix P (columns already in coarse numbering) with the cap, on
 * the host: OpenMP, row-parallel (count, prefix, fill).  Per row, in stored order: pos_sum, neg_sum,
 * pos_max, neg_min; the survivors are the entries with v >= pos_max * eps || v <= neg_min * eps.  A row
 * with at most pmax survivors (every row when pmax == 0) is SSS_amg_interp_trunc's row, bit for bit.
 * Otherwise the pmax survivors of largest |v| are kept (ties: the earlier stored position), in stored
 * order; pos_kept and neg_kept are their sums in stored order (v >= the positive threshold is the
 * positive class, as in the uncapped branch order) and the factors follow the SMALLFLOAT rule, but for
 * a class the cap removed entirely (pos_sum > 0 and pos_kept not above SMALLFLOAT, or the mirror case):
 * when the other class was kept beyond SMALLFLOAT its factor is (pos_sum + neg_sum) / its kept sum, so
 * the row sum of P survives.  P's arrays are freed and replaced on success.  Returns 0, or
 * ERROR_INPUT_PAR (pmax < 0, a NULL or misshapen P) with P untouched. */
int sss_interp_trunc_host(SSS_MAT *P, double eps, int pmax);
/* The same on the GPU, bit for bit the host's arrays: upload, count, prefix, fill, download.  pmax == 0
 * runs the one-lane-per-row kernels of the uncapped truncation.  pmax > 0 gives a row G lanes (1, 4, 16
 * or 64, from the mean row length of P; SSS_HIP_INTERP_LANES forces it): the sums that depend on order
 * are made in stored order by every lane of the group from the same loads, the cut of a capped row is
 * found in pmax rounds, each a group-wide arg-max (by shuffles) of the key (|v|, then the smaller
 * position) over the survivors strictly below the previous round's pick; no per-entry state, no local
 * array.  Returns 0, or an error code with P untouched: ERROR_INPUT_PAR (as the host form, before the
 * first HIP call), ERROR_MAT_SIZE (too many rows for the grid), ERROR_MISC (no device, a failed HIP
 * call or copy). */
int sss_hip_interp_trunc(SSS_MAT *P, double eps, int pmax);

/* Progress hook of the setup (amg_amd/host/sss_setup.c): hook(ctx, mg, done, 0) once levels
 * 0 .. done-1 are final and none of them is the coarsest; hook(ctx, mg, num_levels - 1, 1) at
 * the end. */
typedef void (*sss_setup_hook)(void *ctx, const SSS_AMG *mg, int done, int final);
void sss_amg_setup_hooked(SSS_AMG *mg, SSS_MAT *A, SSS_AMG_PARS *pars, sss_setup_hook hook, void *ctx);

int sss_hip_upload_vec(sss_hip_hier *h, int level, int which, const double *src, int n);
int sss_hip_download_vec(sss_hip_hier *h, int level, int which, double *dst, int n);

/* One V/W-cycle on the device-resident level vectors (asynchronous on the engine stream). */
int sss_hip_cycle(sss_hip_hier *h);
/* wp0 = b0 - A0*x0 and ||wp0||_2, returned to the host (synchronises the stream). */
int sss_hip_residual_norm(sss_hip_hier *h, double *absres);
/* Binary hierarchy file (engine extension; amg_amd/host/sss_hierio.c): what
 * the solve phase reads of a set-up SSS_AMG -- parameters and per level A, P, R, cfmark.  Loading
 * gives a hierarchy field-for-field equal to the one SSS_amg_setup built (free it with
 * SSS_amg_data_destroy).  0 or ERROR_OPEN_FILE / ERROR_WRONG_FILE. */
int SSS_amg_save(const SSS_AMG *mg, const char *path);
int SSS_amg_load(SSS_AMG *mg, const char *path);
/* New operator values on the pattern of a set-up (or loaded) hierarchy (engine extension, DESIGN.md
 * 6.6): A must have the dimensions, row_ptr and col_idx of mg->cg[0].A, else ERROR_INPUT_PAR with mg
 * untouched.  The values are copied into level 0 and A_{l+1} = R_l A_l P_l is recomputed down the
 * levels as values-only products (sss_hip_rap_values under the rule the setup uses for sss_hip_rap
 * -- SSS_SETUP_GPU_RAP, _MIN, _MAXROW, a device being present -- else, and on any device error,
 * sss_rap_values_host).  P, R, cfmark and the level vectors are untouched; a one-level hierarchy
 * is just the copy.  Nothing on stdout; under SSS_SETUP_TIMING one stderr line per level.  A mirror
 * the drop-in solve path holds for mg is refreshed too (sss_hip_hier_refresh), or released when
 * that fails, so that the next solve builds it again.
 * Frozen P carries the old near-null space: see the limit in DESIGN.md 6.6. */
int SSS_amg_refresh(SSS_AMG *mg, const SSS_MAT *A);

/* AMG-preconditioned flexible CG on level 0 (an engine extension -- the
 * reference's Krylov solvers serve only the coarsest level): right-hand side = the level-0 b
 * vector, initial guess / result = the level-0 x vector, one V-cycle per iteration as the
 * preconditioner.  Stops when ||r_k||/||b|| < tol or after maxit iterations; hist (optional)
 * receives the relative residual of each iteration.  b is restored on return.  ||b|| = 0: x = 0, no
 * iteration.  ||b - A x0|| = 0 exactly: no iteration, x untouched, relres 0.  h == NULL:
 * ERROR_INPUT_PAR; a non-finite ||b||, ||b - A x0|| or r_k . r_k: ERROR_SOLVER_EXIT, with the last
 * finite iterate in x. */
int sss_hip_pcg(sss_hip_hier *h, double tol, int maxit, int *iters, double *relres, double *hist, int hist_cap);
/* AMG-preconditioned flexible GMRES(restart) on level 0, for operators that are not symmetric
 * positive definite (an engine extension, like sss_hip_pcg): right preconditioning with one V-cycle
 * on (v_j, 0) per iteration, Arnoldi by classical Gram-Schmidt applied twice in fused multi-vector
 * kernels (deterministic, no atomics), Givens rotations on the host; one read-back of j + 3 doubles
 * per iteration (the Hessenberg column, ||w|| and a stall slot that stays 0 on this engine: the loop
 * is sss_hip_dist_fgmres's).  Right-hand side = the level-0 b vector (restored on return), initial guess /
 * result = the level-0 x vector.  Stops when the estimate |g_{j+1}| / ||b|| < tol or after maxit
 * iterations in total (restart > maxit is clamped); hist (optional) receives the estimate of each
 * iteration.  ||b|| = 0: x = 0, no iteration.  restart < 1: ERROR_INPUT_PAR; a non-finite norm:
 * ERROR_SOLVER_EXIT.
 * Workspace, allocated at the first call, regrown when restart grows and freed with the hierarchy:
 * (2 restart + 3) vectors of n0 doubles (n0 rounded up to even) -- the bases V (restart + 1) and Z
 * (restart), and the saved b and x -- plus 1024 (restart + 1) + 256 doubles of partial sums.  For
 * the 7-point 400^3 problem with restart 20 that is 43 x 0.512 GB = 22 GB. */
int sss_hip_fgmres(sss_hip_hier *h, double tol, int restart, int maxit, int *iters, double *relres, double *hist,
                   int hist_cap);
/* The coarsest-level solve alone (on the level vectors of the coarsest level). */
int sss_hip_coarse_solve(sss_hip_hier *h);
/* The route the last Krylov coarse solve took, for tests: with a hierarchy, the last
 * sss_hip_coarse_solve on h (a cycle's included); with h == NULL, the last
 * sss_hip_host_coarse_solve on the calling thread.  Copies min(n, SSS_HIP_COARSE_LAST_N) fields and
 * returns their number; ERROR_INPUT_PAR where no Krylov coarse solve has completed (none yet, the
 * explicit inverse, or a solve that returned an error).  Every field is a value the host already
 * holds when the solve returns: reading it costs the cycle nothing. */
enum {
    SSS_HIP_CL_FORM = 0,      /* the CG form that ran: 0 LDS-chunked step, 1 register step, 2 one launch */
    SSS_HIP_CL_CG_STATUS,     /* SSS_solver_cg's return value */
    SSS_HIP_CL_CG_ITER,       /* iter as the loop left it (maxit + 1 after a full run, an error code) */
    SSS_HIP_CL_CG_ITER_BEST,
    SSS_HIP_CL_CG_STAG,
    SSS_HIP_CL_CG_MORE_STEP,
    SSS_HIP_CL_GM_RAN,        /* 1: CG's status was negative and SSS_solver_gmres ran */
    SSS_HIP_CL_GM_STATUS,
    SSS_HIP_CL_GM_ITER,
    SSS_HIP_CL_GM_CYCLES,     /* Krylov cycles (passes of the restart loop) */
    SSS_HIP_COARSE_LAST_N
};
int sss_hip_coarse_last(sss_hip_hier *h, int *out, int n);
/* Pre (post = 0) or post (post = 1) smoothing of one level. */
int sss_hip_smooth(sss_hip_hier *h, int level, int post);
int sss_hip_sync(sss_hip_hier *h);

/* Per-level statistics for reporting: rows, nnz(A), nnz(P), smoother DAG depths; the exact GS
 * engine of the F / C pass (0: one launch per DAG depth, 1: chip-wide dataflow, 2: single CU);
 * whether a one-launch pass ever gave up waiting (gs_stall != 0: results invalid); the storage of
 * A_l in HBM (a_format bits: 1 column-sorted tiles, 2 dictionary tiles (with 1: value
 * dictionaries over the sorted tiles; alone with 64: dictionary ELL rows), 4 free-order rows,
 * 8 merged row groups, 16 wave-per-row;
 * the two-stage inner steps of a C/F-Jacobi level (0: plain C/F-Jacobi). */
typedef struct sss_hip_level_info {
    int rows, nnz, nnz_p, dag_f, dag_c, smoother_kind;
    int gs_engine_f, gs_engine_c, gs_stall, a_format;
    long long a_stream_bytes;   /* bytes of A_l's stored format one tile-path SpMV reads (no vectors) */
    int inner;
    int r_format, p_format;     /* R_l / P_l storage, the a_format bits */
    int pad_;
} sss_hip_level_info;
int sss_hip_level_info_get(sss_hip_hier *h, int level, sss_hip_level_info *out);
int sss_hip_num_levels(sss_hip_hier *h);
/* Narrow keys of the merged row groups (SSS_HIP_MERGE_KEY16=1): per entry a 16-bit key
 * (column delta << 3 | accumulator), per chunk of 64 entries of a wave's share a descriptor
 * {base_lo, base_hi, split, esc} of four ints; a share with a chunk that fits neither one nor two
 * bases keeps 32-bit keys in an escape list (esc >= 0: the chunk's first key there).
 * sss_hip_merged_narrow is the host narrowing both builders reproduce: keys are the nnz sorted
 * 32-bit keys (column << 4 | segment << 3 | row), gp the ng + 1 group bounds, W the waves per group
 * (1, 2, 4); desc holds desc_cap >= *n_desc slots of four ints, esc up to esc_cap keys (nnz always
 * suffices); counts[5] = chunks: all, one base, two bases, wide, stored with 32-bit keys.
 * sss_hip_merged_key_stats: out[8] = those five counts, the entries, descriptor slots and escaped
 * keys of a level's merged copy (which: 0 the level matrix, 1 / 2 the F / C class's [N | L] copy,
 * 3 / 4 its L copy); returns 1 (out zeroed) if the copy has no narrow keys.  sss_hip_merged_keys_get
 * downloads the three arrays of such a copy (sizes as the stats report them). */
int sss_hip_merged_narrow(const unsigned *keys, long long nnz, const int *gp, int ng, int two, int W,
                          unsigned short *k16, int *desc, long long desc_cap, long long *n_desc,
                          unsigned *esc, long long esc_cap, long long *n_esc, long long *counts);
int sss_hip_merged_key_stats(sss_hip_hier *h, int level, int which, long long *out);
int sss_hip_merged_keys_get(sss_hip_hier *h, int level, int which, unsigned short *k16, int *desc,
                            unsigned *esc);
/* First level of the V-cycle's single-workgroup tail (sss_tail.hip: the small coarse levels,
 * descent, coarsest solve and ascent in one launch), or -1 when the cycle has none. */
int sss_hip_tail_from(sss_hip_hier *h);
/* Kernel launches of one V-cycle as captured in its hipGraph (host-steered Krylov coarse solves
 * excluded), or -1 before the first captured cycle / without graphs. */
int sss_hip_cycle_launches(sss_hip_hier *h);
/* Stored-format bytes the kernels of one outer iteration read and write (the next sss_hip_cycle and
 * the residual + norm after it; walked into a discarded stream capture, nothing runs): the stored
 * matrix bytes of the rows each launch covers, the x it gathers counted once per covered row, and
 * 8 B per covered row of every row vector it streams.  out[l] for level l, out[nslots - 2] the outer
 * residual + norm, out[nslots - 1] the coarsest solve; nslots >= sss_hip_num_levels(h) + 2. */
int sss_hip_cycle_bytes(sss_hip_hier *h, double *out, int nslots);

/* ---- kernel-level entry points on device memory (tests, bench, roofline) ------------- */
enum {
    SSS_HIP_SPMV_MXY = 0,    /* y = A*x                         (SSS_blas_mv_mxy)      */
    SSS_HIP_SPMV_AMXPY = 1,  /* y += (A*x)*alpha                (SSS_blas_mv_amxpy)    */
    SSS_HIP_SPMV_RESID = 2,  /* y = b + (A*x)*(-1)              (copy + amxpy(-1))     */
    SSS_HIP_SPMV_ACC = 3     /* y += A*x, rows < cap only       (spmv_cuda)            */
};
/* A plan holds the CSR-adaptive row blocking of one matrix (device pointers). */
typedef struct sss_hip_spmv_plan sss_hip_spmv_plan;
sss_hip_spmv_plan *sss_hip_spmv_plan_create(int n, int nnz, const int *d_rp, const int *h_rp);
void sss_hip_spmv_plan_destroy(sss_hip_spmv_plan *p);
int sss_hip_spmv(const sss_hip_spmv_plan *p, int op, double alpha, const int *d_rp, const int *d_ci,
                 const double *d_v, const double *d_x, const double *d_b, double *d_y, int cap,
                 void *stream);

/* Host-memory convenience wrappers (allocate, copy, run, copy back) used by the exported
 * SSS_blas_mv_* / smoother / coarse-solve entry points. */
int sss_hip_host_spmv(int op, double alpha, const SSS_MAT *A, const double *x, const double *b,
                      double *y, int cap);
/* The same product in the summation order sss_hip_opts.sum_order names (0: the reference's, as
 * sss_hip_host_spmv; 1: the free order of the long-row kernels, deterministic but not the
 * reference's bits). */
int sss_hip_host_spmv_order(int op, double alpha, const SSS_MAT *A, const double *x, const double *b,
                            double *y, int cap, int sum_order);
int sss_hip_host_smooth(const SSS_SMTR *s, int post);

/* ---- one matrix in a chosen storage format (tests of the formats at their limits) ----- */
/* The encoding flags of a matrix upload: which storage formats it may take (those it qualifies for
 * are tried in the order dictionary ELL, column ELL, dictionary tiles, sorted tiles with or without
 * value dictionaries; the SSS_HIP_DICT / ELL / ELL_BASE / XELL switches still apply). */
enum {
    SSS_HIP_ENC_SORTED_TILES = 1,   /* column-sorted tile staging */
    SSS_HIP_ENC_FREE_ORDER = 2,     /* free summation order on long-row matrices */
    SSS_HIP_ENC_DICT = 4,           /* the dictionary formats (square: dictionary ELL, dictionary tiles;
                                       value dictionaries over the sorted tiles) */
    SSS_HIP_ENC_MERGED_ONLY = 8,    /* read through a merged copy / no range relaxation: column ELL up to
                                       40 slots per row */
    SSS_HIP_ENC_XELL = 16,          /* column ELL */
    SSS_HIP_ENC_ELL = 32,           /* dictionary ELL also for a rectangular matrix, no dictionary tiles */
    SSS_HIP_ENC_ELL_BASE = 64       /* rectangular: dictionary ELL with offsets against each row's first column */
};
/* What an upload chose: the a_format bits of sss_hip_level_info, the row widths of the dictionary ELL
 * and the column ELL (0: not taken), the column bits of a column ELL code, whether the dictionary
 * ELL has per-row bases, the row blocks and the block that starts at the class split. */
typedef struct sss_hip_store_info {
    int a_format, ell_w, xell_w, xell_shift, ell_based, nblk, split_blk, pad_;
} sss_hip_store_info;
/* sss_hip_host_spmv with the upload's encoding flags and class split row (-1: none) given by the
 * caller, on a device object built for this call alone (never cached); *info receives what the
 * upload chose. */
int sss_hip_host_spmv_enc(int op, double alpha, const SSS_MAT *A, const double *x, const double *b,
                          double *y, int cap, int enc, int split, sss_hip_store_info *info);
/* One smoother call of a level on host data.  A is laid out as a relabeled level: rows [0, nF) are
 * class F, rows [nF, n) class C.  It is uploaded with a block split at nF and the flags enc, and
 * smoothed by `sweeps` sweeps of `kind` (SSS_HIP_SMOOTH_EXACT or _JACOBI; `inner` two-stage steps),
 * x in place, on a device object built for this call alone.
 *   fuse 0: the smoother alone; then (r and rnorm2 given) r = b - A x by a residual SpMV.
 *   fuse 1: the smoother with the C rows' residual fused into its last pass where the plan allows,
 *           the F rows' (or the whole) residual after it, as the cycle's descent does.
 *   fuse 2: the F rows' residual of the incoming x together with the first F pass, then as fuse 1
 *           with that pass skipped (the cycle after an outer residual); SSS_HIP_STEP_NO_PEND, with
 *           nothing run, where the plan does not allow it.
 * r (n doubles) and *rnorm2 (the sum of squares of r, per-block partials summed in a fixed order)
 * are optional with fuse 0.  plan_info receives SSS_HIP_PLAN_INFO_N ints (SSS_HIP_PI_*). */
enum { SSS_HIP_STEP_NO_PEND = 1 };
enum {
    SSS_HIP_PI_RANGE_F = 0,   /* the F / C pass runs on the level matrix's own row blocks */
    SSS_HIP_PI_RANGE_C,
    SSS_HIP_PI_FUSED,         /* the last C pass wrote its rows' residual */
    SSS_HIP_PI_PEND_OK,       /* the plan allows fuse 2 */
    SSS_HIP_PI_INNER,         /* two-stage inner steps of the plan (0: none) */
    SSS_HIP_PI_NL_F_FORMAT,   /* a_format bits and column ELL width of the two-stage copies: */
    SSS_HIP_PI_NL_F_XELL_W,   /*   the F class's [N | L] rows, */
    SSS_HIP_PI_LO_F_FORMAT,   /*   its L rows, */
    SSS_HIP_PI_LO_F_XELL_W,
    SSS_HIP_PI_NL_C_FORMAT,   /*   the C class's [N | L] rows, */
    SSS_HIP_PI_NL_C_XELL_W,
    SSS_HIP_PI_LO_C_FORMAT,   /*   its L rows */
    SSS_HIP_PI_LO_C_XELL_W,
    SSS_HIP_PI_STALL,         /* the one-launch passes' stall words, or-ed (read and cleared) */
    SSS_HIP_PI_FUSE_RESID,    /* the plan can fuse the C rows' residual */
    SSS_HIP_PI_F_OVERWRITTEN, /* the F pass overwrites x_F from C values only */
    SSS_HIP_PLAN_INFO_N
};
int sss_hip_host_level_step(const SSS_MAT *A, int nF, int enc, int kind, int inner, int sweeps, int post,
                            int fuse, const double *b, double *x, double *r, double *rnorm2,
                            sss_hip_store_info *info, int *plan_info);
/* One orthogonalisation step of sss_hip_fgmres on host data, through the same kernels: V holds k
 * columns of n doubles back to back; w is orthogonalised against them in place (not normalised),
 * hcol[0 .. k) receives the Hessenberg coefficients and *norm the 2-norm of the new w. */
int sss_hip_host_orth(int n, int k, const double *V, double *w, double *hcol, double *norm);
/* The two fused level-0 kernels of sss_hip_dist_pcg on host data.  pcg_update: with a = alpha_num /
 * alpha_den, x += a p and r -= a q in place, r_old = the old r, *rr = the sum of squares of the new
 * r -- one pass; the elementwise results are those of the unfused updates bit for bit.  dot2:
 * out[0] = r . z and out[1] = r_old . z in one pass over z.  Sums are fixed-order (deterministic). */
int sss_hip_host_pcg_update(int n, double alpha_num, double alpha_den, const double *p, const double *q, double *x,
                            double *r, double *r_old, double *rr);
int sss_hip_host_dot2(int n, const double *r, const double *r_old, const double *z, double *out);
/* The three host-memory entry points keep the device form of their operator (keyed by a content
 * hash of the CSR arrays, the use and the device) in a small cache, so a caller that loops over
 * them with the same matrix uploads it once; this releases the cached device objects. */
void sss_hip_host_cache_clear(void);
/* coarse_mode SSS_HIP_COARSE_DIRECT (up to 20,000 rows): the explicit inverse; a matrix with a zero
 * or non-finite pivot, or whose inverse has a non-finite entry, gives ERROR_SOLVER_EXIT and leaves x
 * untouched (sss_hip_hier_create falls back to the Krylov coarse solve for such a coarsest level). */
int sss_hip_host_coarse_solve(SSS_MAT *A, SSS_VEC *b, SSS_VEC *x, double ctol, int coarse_mode,
                              int row_cap);

/* Engine event timer around `reps` launches of the level-0 residual SpMV on the engine
 * stream: average kernel milliseconds (roofline measurement in bench.py). */
int sss_hip_time_level0_spmv(sss_hip_hier *h, int reps, double *avg_ms);
/* level_ms[l] (nslots >= levels): level l's share of an eager cycle -- pre-smoothing, residual,
 * restriction, zero fill, prolongation, post-smoothing (the coarsest: its solve; a single-workgroup
 * tail: at its first level) -- averaged over reps, events between the steps.  Advances the iterate. */
int sss_hip_time_levels(sss_hip_hier *h, int reps, double *level_ms, int nslots);
/* The same launch from level 0's plain CSR arrays (whatever storage the cycle uses for A_0). */
int sss_hip_time_level0_spmv_csr(sss_hip_hier *h, int reps, double *avg_ms);
/* Average milliseconds of `reps` full iterations (cycle + residual + norm) on the engine
 * stream, timed with HIP events; absres of the last iteration is returned. */
int sss_hip_time_iterations(sss_hip_hier *h, int reps, double *avg_ms, double *absres);

/* ---- row-partitioned multi-GPU solve (one process per GPU) ------------------------- */
/* Every level l < nagg is split into contiguous row ranges: level 0 evenly, level l+1 by
 * ownership of the C points of level l (coarse numbering is monotone in the fine index,
 * SSS_coarsen's cmap).  Each rank keeps its rows (F|C relabeled) plus ghost columns; levels
 * >= nagg (fewer than agg_rows rows, and always the coarsest) are replicated on every rank and
 * cycled redundantly.  Halos move over RCCL (xGMI) or, for tests, over a host transport. */
typedef struct sss_hip_comm sss_hip_comm;
typedef struct sss_hip_dist sss_hip_dist;
typedef struct sss_hip_host_transport {
    void *ctx;
    /* one point-to-point round: send scount[i] doubles (concatenated in sbuf) to rank sdst[i]
     * and receive rcount[i] doubles (concatenated into rbuf) from rank rsrc[i]; 0 = success */
    int (*exchange)(void *ctx, int nsend, const int *sdst, const int *scount, const double *sbuf, int nrecv,
                    const int *rsrc, const int *rcount, double *rbuf);
    int (*allreduce_sum)(void *ctx, double *v, int n);
    /* all[displs[q] .. + counts[q]) <- rank q's `mine` */
    int (*allgatherv)(void *ctx, const double *mine, int count, double *all, const int *counts, const int *displs);
} sss_hip_host_transport;

#define SSS_HIP_RCCL_ID_BYTES 128
/* rank 0 creates the id; the caller broadcasts its bytes (e.g. over torch.distributed) */
int sss_hip_rccl_unique_id(unsigned char *id);
/* device >= 0: hipSetDevice(device) first (the communicator binds the current device) */
sss_hip_comm *sss_hip_comm_rccl(int nranks, int rank, const unsigned char *id, int device);
sss_hip_comm *sss_hip_comm_host(int nranks, int rank, const sss_hip_host_transport *t);
/* Timing only: every collective and halo transfer is skipped, the rest of the rank's cycle (its
 * kernels, halo packs, graph capture) runs as over RCCL -- the per-rank compute floor of a multi-GPU
 * run measured one rank at a time on one GPU (tools/n8_floor.py).  The iterates are meaningless. */
sss_hip_comm *sss_hip_comm_timing(int nranks, int rank);
void sss_hip_comm_destroy(sss_hip_comm *c);

/* mg: the global hierarchy (every rank runs the same host setup).  V-cycles only.
 * agg_rows <= 0: SSS_HIP_AGG_ROWS or 20000. */
sss_hip_dist *sss_hip_dist_create(const SSS_AMG *mg, const sss_hip_opts *o, sss_hip_comm *c, int agg_rows);
/* The same engine from a partition set written by sss_part_save: rank r reads only
 * prefix.r<r> (its rows, ghosts, halo lists) and prefix.tail (the replicated coarse levels), so
 * no rank holds the global hierarchy (the 512^3 8-GPU configuration). */
sss_hip_dist *sss_hip_dist_create_from_files(const char *prefix, const sss_hip_opts *o, sss_hip_comm *c);
void sss_hip_dist_destroy(sss_hip_dist *d);
/* own rows [lo, hi) of level 0 in the original numbering; nagg = number of partitioned levels */
int sss_hip_dist_info(sss_hip_dist *d, int *lo, int *hi, int *nagg, int *nghost0);
/* Own rows, ghosts and nonzeros of this rank's partitioned level l. */
int sss_hip_dist_level_size(sss_hip_dist *d, int l, int *m, int *g, long long *nnz);
/* exact eliminations in force on partitioned level l (agreed over the ranks), a bit mask:
 * 1 zero-first pass, 2 fused C-row residual, 4 dead F-row prolongation, 8 the cycle runs as one
 * captured hipGraph (SSS_HIP_DIST_GRAPH=1 over RCCL with a device-side coarse solve).  <0: bad level. */
int sss_hip_dist_level_flags(sss_hip_dist *d, int l);
/* level-0 vectors, the rank's own rows in the original order (n = hi - lo) */
int sss_hip_dist_upload_vec(sss_hip_dist *d, int which, const double *own, int n);
int sss_hip_dist_download_vec(sss_hip_dist *d, int which, double *own, int n);
int sss_hip_dist_cycle(sss_hip_dist *d);
/* global ||b0 - A0 x0||_2 (one 8-byte allreduce), synchronises */
int sss_hip_dist_residual_norm(sss_hip_dist *d, double *absres);
/* sss_hip_pcg and sss_hip_fgmres on the row-partitioned engine: for FGMRES the same loop
 * (right-preconditioned FGMRES(restart) with classical Gram-Schmidt applied twice; one
 * implementation serves both engines), for PCG the same recurrences (flexible CG with the
 * Polak-Ribiere beta) in a loop of its own; the same stop rules, hist / hist_cap / NULL rules and treatment of ||b|| = 0, restart < 1
 * (ERROR_INPUT_PAR, before any collective) and a non-finite norm, with "level-0 b / x vector" read
 * as this rank's own rows of them; b is restored on return.  Collective: every rank calls with the
 * same arguments.  z = one sss_hip_dist_cycle on (r, 0) (the captured graph where there is one);
 * A p and A z use the level-0 local matrix after a halo exchange of the vector.  Every dot product is
 * summed over the ranks before use and every branch is taken from reduced values only, so all ranks
 * leave in the same iteration -- also with ERROR_MISC when a one-launch Gauss-Seidel pass stalled
 * on any rank (the stall word rides on one of the reductions).
 * Reductions per iteration -- PCG: 3 (p.q; r.r with the stall flag; {r.z, r_old.z} together), plus
 * ||b||^2, ||r_0||^2 and the first r.z once per solve (after a non-finite r.r the iterate in x is
 * the last one formed: x and r take their step in one kernel).  FGMRES: 3 per Arnoldi step (the coefficients of the
 * first and of the second Gram-Schmidt pass; ||w||^2 with the stall flag -- the Hessenberg column is
 * formed from the reduced coefficients and the root taken after the reduction), plus ||b||^2 once
 * and ||r||^2 at every restart.  Over RCCL the scalars stay on the device (in-place ncclAllReduce on
 * the engine stream) with one small read-back per iteration; over the host transport each reduction
 * synchronises and goes through allreduce_sum; the timing communicator skips them.
 * The iterates are not bitwise the single-GPU solvers': the dot products are summed in another
 * order; every elementwise operation and the whole preconditioner are the same bit for bit.  (With
 * one rank FGMRES sums in the single-GPU order and its results are the single-GPU solver's bits.)
 * Workspace is allocated at first use (FGMRES: regrown when restart grows) and freed with the
 * engine: PCG 5 vectors of this rank's rows, FGMRES 2 restart + 3. */
int sss_hip_dist_pcg(sss_hip_dist *d, double tol, int maxit, int *iters, double *relres, double *hist, int hist_cap);
int sss_hip_dist_fgmres(sss_hip_dist *d, double tol, int restart, int maxit, int *iters, double *relres, double *hist,
                        int hist_cap);
int sss_hip_dist_sync(sss_hip_dist *d);
/* average ms of `reps` local level-0 residual SpMVs (no exchange): the per-rank roofline */
int sss_hip_dist_time_level0_spmv(sss_hip_dist *d, int reps, double *avg_ms);
/* *cycle_ms: this rank's cycle as it runs (captured graph), averaged over reps; level_ms[l] (l < nagg)
 * one partitioned level's descent + ascent and level_ms[nagg] the replicated tail, from reps eager
 * cycles with events between the steps (nslots >= nagg + 1).  Advances the iterate. */
int sss_hip_dist_time_levels(sss_hip_dist *d, int reps, double *cycle_ms, double *level_ms, int nslots);
/* the replicated tail's per-level times (sss_hip_time_levels on it) */
int sss_hip_dist_time_tail_levels(sss_hip_dist *d, int reps, double *level_ms, int nslots);
/* Per partitioned level: halo exchanges enqueued since the last reset and the doubles this rank sent
 * in them (a captured cycle counts at its capture); the tail all-gather's own / all rows and the
 * number of replicated levels. */
int sss_hip_dist_halo_stats(sss_hip_dist *d, long long *calls, long long *doubles, int nslots, int reset,
                            int *nc_own, int *nc_all, int *tail_levels);

/* Host-only view of the partition (no device needed; used by the CPU multi-process tests).
 * which: 0 = A_l (m x (m+g)), 1 = P_l (m x next-level local), 2 = R_l (own coarse rows x (m+g)).
 * Arrays stay owned by the plan. */
typedef struct sss_part_plan sss_part_plan;
sss_part_plan *sss_part_plan_create(const SSS_AMG *mg, int nranks, int rank, int agg_rows);
/* Partition set of the global hierarchy for nranks ranks: prefix.r0 .. prefix.r<nranks-1> (one
 * rank's plan each, built one at a time) and prefix.tail (levels >= nagg, SSS_amg_save format).
 * Host only.  Returns 0 or an SSS error code. */
int sss_part_save(const SSS_AMG *mg, int nranks, int agg_rows, const char *prefix);
/* One rank's plan read back from its partition file (prefix.r<rank>). */
sss_part_plan *sss_part_plan_load(const char *path);
void sss_part_plan_destroy(sss_part_plan *p);
int sss_part_plan_nagg(const sss_part_plan *p);
/* own range, own count, ghost count of level l (l <= nagg for the range; m/g for l < nagg) */
int sss_part_plan_level(const sss_part_plan *p, int l, int *lo, int *hi, int *m, int *g);
int sss_part_plan_matrix(const sss_part_plan *p, int l, int which, SSS_MAT *out);
/* perm: local id -> global id (m); ghosts: ghost k -> global id (g) */
int sss_part_plan_ids(const sss_part_plan *p, int l, const int **perm, const int **ghosts);
/* halo of level l: nsend/nrecv peers; peer ranks, counts, send local ids (concatenated) */
int sss_part_plan_halo(const sss_part_plan *p, int l, int *nsend, const int **sdst, const int **scount,
                       const int **sidx, int *nrecv, const int **rsrc, const int **rcount);

/* ---- generators (host) -------------------------------------------------------------- */
/* kind 7 or 27; rows of z-planes [z0, z1) of an nx*ny*nz grid, global column indices. */
int sss_gen_stencil(int kind, int nx, int ny, int nz, int z0, int z1, SSS_MAT *A);

#ifdef __cplusplus
}
#endif
#endif
