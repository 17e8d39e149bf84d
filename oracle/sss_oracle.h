/*
 * sss_oracle.h — TEST INFRASTRUCTURE ONLY.  CPU restatement of the reference solve phase,
 * used as the parity checker by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
 * leg.  Never linked into or called by the product (libsss_amg.so).
 *
 * Parity pinning: see oracle/sss_oracle.c header.
 */
#ifndef SSS_ORACLE_H
#define SSS_ORACLE_H

#include "../include/sss_amg.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int row_cap;      /* 0: uncapped coarse SpMV (parity definition); 4096: as-shipped <<<64,64>>> */
    int coarse_mode;  /* 0: reference CG(beta==1)+GMRES(30); 1: dense LU direct solve */
    int smoother;     /* 0: exact smoother per pars (GS-CF); 1: C/F-Jacobi on levels >= jacobi_from */
    int jacobi_from;  /* first level that uses C/F-Jacobi when smoother == 1 */
    int verbose;      /* print the reference iteration table */
    int jacobi_l1;    /* C/F-Jacobi divisor: 0 = a_ii, 1 = a_ii + sum_{j != i} |a_ij| over same-class j (l1) */
    double omega;     /* C/F-Jacobi weight (1.0 = plain) */
    int inner;        /* > 0: two-stage GS-CF instead of C/F-Jacobi, with `inner` Jacobi-Richardson
                         steps on the same-class lower triangle (ora_cf_twostage) */
    int inner_mask;   /* experiments: bit l set = level l uses two-stage (0 = every C/F-Jacobi level) */
    int inner_long;   /* extra inner steps on the two-stage levels whose bit is set in long_mask (the
                         engine's long-row levels, sss_hip_opts::inner_long) */
    int long_mask;
} ora_opts;

void ora_opts_default(ora_opts *o);

/* SSS_utils.c:161-201 (+ the row cap of Solve/SSS_cuda.cu:131,152 when cap > 0) */
/* host threads for the row-parallel loops (results do not depend on it) */
void ora_set_threads(int n);
int ora_get_threads(void);
void ora_mv_amxpy(double alpha, const SSS_MAT *A, const double *x, double *y, int cap);
void ora_mv_mxy(const SSS_MAT *A, const double *x, double *y);
void ora_mv_acc(const SSS_MAT *A, const double *x, double *y, int cap);

/* Solve/SSS_smooth.c */
void ora_gs_cf(double *u, const SSS_MAT *A, const double *b, int sweeps, const int *mark, int order);
void ora_gs(double *u, int i1, int in, int step, const SSS_MAT *A, const double *b, int sweeps);
void ora_cf_jacobi(double *u, const SSS_MAT *A, const double *b, int sweeps, const int *mark);
void ora_cf_jacobi_w(double *u, const SSS_MAT *A, const double *b, int sweeps, const int *mark, double omega,
                     int l1);
void ora_cf_twostage(double *u, const SSS_MAT *A, const double *b, int sweeps, const int *mark, int inner);
void ora_smoother_pre(SSS_SMTR *s);
void ora_smoother_post(SSS_SMTR *s);

/* Solve/SSS_cycle.cu */
int ora_cg(SSS_KRYLOV *ks, int cap);
int ora_gmres(SSS_KRYLOV *ks, int cap);
void ora_coarest_solve(SSS_MAT *A, SSS_VEC *b, SSS_VEC *x, double ctol, const ora_opts *o);
void ora_cycle(SSS_AMG *mg, const ora_opts *o);

/* The route the last ora_cg / ora_gmres / ora_coarest_solve call on this thread took: how often each
 * branch of the two state machines ran, then the statuses and the final counters.  Counting only:
 * no arithmetic depends on it.  ora_cg clears every slot; ora_gmres called on its own clears the CG
 * slots as well; the dense-LU coarse mode leaves every slot at zero. */
enum {
    ORA_EV_CG_BREAKDOWN = 0,   /* |temp2| <= SMALLFLOAT2: goto restore */
    ORA_EV_CG_SOLSTAG,         /* ||u||_inf <= SMALLFLOAT: ERROR_SOLVER_SOLSTAG */
    ORA_EV_CG_CHECK2,          /* check II (stagnation) entered */
    ORA_EV_CG_CHECK2_CONV,     /* ... and its recomputed residual met the tolerance */
    ORA_EV_CG_STAG_EXIT,       /* ... ERROR_SOLVER_STAG */
    ORA_EV_CG_CHECK3,          /* check III (false convergence) entered */
    ORA_EV_CG_CHECK3_CONV,     /* ... and its recomputed residual met the tolerance */
    ORA_EV_CG_TOLSMALL_EXIT,   /* ... ERROR_SOLVER_TOLSMALL */
    ORA_EV_CG_STAG_INC,        /* p zeroed, ++stag */
    ORA_EV_CG_MORE_STEP_INC,   /* p zeroed, ++more_step */
    ORA_EV_CG_BEST_COPIED,     /* the restore block copied u_best into u */
    ORA_EV_CG_IMMEDIATE,       /* relres < tol before the first step */
    ORA_EV_CG_MAXIT,           /* the loop ran to maxit */
    ORA_EV_GM_IMMEDIATE,       /* relres < tol before the first Krylov cycle */
    ORA_EV_GM_CYCLES,          /* Krylov cycles (passes of the outer loop) */
    ORA_EV_GM_EARLY_BREAK,     /* the Arnoldi loop left by its residual estimate */
    ORA_EV_GM_RECHECK_FAILED,  /* the true residual did not confirm the estimate: restart with i = 0 */
    ORA_EV_GM_RECOMBINE,       /* p[0] recombined from the basis (i > 0) */
    ORA_EV_GM_BEST_COPIED,     /* x_best copied into x at the end */
    ORA_EV_GM_MAXIT,           /* iter >= maxit at the end */
    ORA_EV_COUNT,              /* ---- the events end here */
    ORA_KR_CG_STATUS = ORA_EV_COUNT,
    ORA_KR_CG_ITER,            /* iter as the loop left it (maxit + 1 after a full run) */
    ORA_KR_CG_ITER_BEST,
    ORA_KR_CG_STAG,
    ORA_KR_CG_MORE_STEP,
    ORA_KR_GM_RAN,
    ORA_KR_GM_STATUS,
    ORA_KR_GM_ITER,
    ORA_KR_COUNT
};
/* copies min(n, ORA_KR_COUNT) slots */
void ora_krylov_events(int *out, int n);

/* Solve/SSS_SOLVE.c:4-87; relres/absres of iterations 1..nits are stored (if non-NULL) */
SSS_RTN ora_solve(SSS_AMG *mg, SSS_VEC *x, SSS_VEC *b, const ora_opts *o, double *relres_hist,
                  double *absres_hist, int hist_cap);

/* Setup/SSS_inter.cu:550-715 (interp_STD) + :16-102 (SSS_amg_interp_trunc), sequential: fills the
 * values of the standard-interpolation pattern P (fine column indices, as SSS_amg_coarsen returns
 * it), renumbers its columns to coarse indices and truncates with `trunc`. */
void ora_interp_std(const SSS_MAT *A, const int *mark, SSS_MAT *P, const SSS_IMAT *S, double trunc);

/* Seconds spent inside ora_coarest_solve since the last reset (baseline split). */
double ora_coarse_seconds(void);
void ora_reset_timers(void);

#ifdef __cplusplus
}
#endif
#endif
