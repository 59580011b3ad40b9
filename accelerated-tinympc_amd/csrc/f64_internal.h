// f64_internal.h — what the host file of the fp64 library (tinympc_batch64.hip) and its kernel units (admm_f64_*.hip, batch64_helpers.hip) share: the kernel argument
// structs, the lists of instantiated problem classes, and one typed launcher per kernel family.  Every launcher enqueues on the null stream and
// answers hipErrorInvalidValue where there is no instantiation for the class; the host turns that into its own messages.
#pragma once
#include "../../include/tinympc_batch64.h"

#include <hip/hip_runtime.h>

namespace tinympc64
{
constexpr int PS = 2; // doubles per SSE2 packet
constexpr int WAVE64 = 64;
constexpr int ST_SOLVED = 1, ST_UNSOLVED = 11; // admm.cpp:136, :114

struct Params64
{
    int nx, nu, N, batch, bpad;
    double rho, abs_pri_tol, abs_dua_tol;
    int max_iter, check_termination, en_state_bound, en_input_bound;
    double *arr[TINY_ARR_COUNT];
    const double *xref, *xmin, *xmax, *umin, *umax; // [steps][dim][stride]; stride = bpad (per instance) or 1 (shared)
    int xref_stride, xb_stride, ub_stride;
    const double *mats; // Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q, column-major
    double *res;        // [4][bpad]
    int *status, *iter, *n_unsolved;
};
// closed loop on chip: the further arguments of the MPC instantiations of the sixteen-lane kernel (a struct of their own: the one-solve kernels
// take none of them)
struct Mpc64
{
    int mpc_steps, window_advance, table_rows; // table_rows > 0: the reference is a window into `table`
    const double *table;                       // [table_rows][nx]
    int *xref_start;                           // [batch], read at live-in and written back after the last solve
    double *u0_traj;                           // [mpc_steps][batch][nu] or NULL; the kernel stores every step but the last
};
// closed loop against a separate plant (tiny_batch64_set_plant, tiny_batch64_mpc_run_sim): the further argument of the SIM instantiations
struct Sim64
{
    const double *plant;  // the rows of [A_p | B_p] packed for the sixteen lanes, entry (k, r) at k * 16 + r (input lanes hold zeros); NULL: the model's rows
    size_t plant_stride;  // doubles from one instance's table to the next, (nx + nu) * 16; 0: one table for the batch
    const double *w;      // [mpc_steps][batch][nx] or NULL: no addition
    double *x_traj;       // [mpc_steps][batch][nx] or NULL; the kernel stores every step but the last
};
// per-instance models (tiny_batch64_set_models): the further argument of the ",pm" instantiations, the last of a kernel's trailing arguments.  A lane
// (a thread) reads its instance's matrices straight from the record, once per solve: there is no packed per-lane form
struct Models64
{
    const double *rec; // [batch][stride]: Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q of every instance, column-major (the layout of Params64::mats)
    size_t stride;     // doubles from one instance's record to the next
    const double *rho; // [batch]
};
// per-instance settings (tiny_batch64_set_instance_settings): one record per instance, TinySettings (types.hpp:39-47) without the unused fields, and the
// further argument of the ",ps" instantiations, the last of a kernel's trailing arguments.  The host rebuilds the records on every
// set_instance_settings / set_settings; Params64::max_iter of a ps launch carries the batch's largest budget, its other settings are not read
struct InstSettings64
{
    double abs_pri_tol, abs_dua_tol;
    int max_iter, check_termination, en_state_bound, en_input_bound;
};
static_assert(sizeof(InstSettings64) == 32, "one record is two 16-byte loads");
struct Settings64
{
    const InstSettings64 *rec; // [batch]
};
// arguments of plant64_sim_kernel: the plant step of one MPC step on the workspace's x.col(0) / u.col(0)
struct PlantSim64
{
    double *X;
    const double *U, *A, *B;     // A, B column-major: the plant's, or the model's Adyn / Bdyn
    size_t stride_a, stride_b;   // doubles from one instance's matrix to the next; 0: one pair for the batch
    int batch, bpad;
    const double *w;             // this step's [batch][nx] row or NULL: no addition
    double *x_traj, *u0_row;     // this step's [batch][nx] / [batch][nu] rows or NULL: not recorded
    int *start;                  // the window starts or NULL
    int window_advance;
};
// the six functions tiny_solve() is made of (admm.hpp:12-18), one launch each: launch_f64_step
enum { F64_FORWARD_PASS = 0, F64_UPDATE_SLACK, F64_UPDATE_DUAL, F64_UPDATE_LINEAR_COST, F64_TERMINATION_CONDITION, F64_BACKWARD_PASS_GRAD };

// problem classes of the fp64 library (the thread-per-instance kernels; any N).  nx and nu must each be <= 2 or even (the
// reference's order for other sizes depends on alignment, see row_dot) and not both >= 8 (Eigen's GEMV kernel is not restated here)
#define TINY_FOR_EACH_F64DIMS(X) X(12, 4) X(4, 1) X(8, 4) X(12, 2) X(4, 2) X(4, 4) X(16, 4)
#define TINY_FOR_EACH_F64ROWS(X) X(12, 4, 10) X(12, 4, 30) X(12, 4, 20) X(4, 1, 10) X(8, 4, 9)
// classes of the sixteen-lane kernel with a runtime horizon (any N <= 64): the unrolled body has a capacity of 32 or 64 steps
#define TINY_FOR_EACH_F64ROWS_RT(X) X(12, 4) X(4, 1) X(8, 4) X(12, 2) X(4, 2) X(4, 4)
constexpr int F64ROWS_RT_MAX_N = 64;

inline bool rows_unrolled(int nx, int nu, int N)
{
#define TINY_F64ROWS_CHECK(NX, NU, NN) \
    if (nx == NX && nu == NU && N == NN) return true;
    TINY_FOR_EACH_F64ROWS(TINY_F64ROWS_CHECK)
#undef TINY_F64ROWS_CHECK
    return false;
}
inline bool rows_supported(int nx, int nu, int N)
{
    if (rows_unrolled(nx, nu, N)) return true;
#define TINY_F64ROWS_RT_CHECK(NX, NU) \
    if (nx == NX && nu == NU && N >= 2 && N <= F64ROWS_RT_MAX_N) return true;
    TINY_FOR_EACH_F64ROWS_RT(TINY_F64ROWS_RT_CHECK)
#undef TINY_F64ROWS_RT_CHECK
    return false;
}

// admm_f64_thread.hip: one thread per instance, any N.  The fused solve; one of the six step functions (fn: the enum above; conv: the
// [bpad] flags F64_TERMINATION_CONDITION writes, unused by the others)
hipError_t launch_f64_thread(int nx, int nu, const Params64 &P);
hipError_t launch_f64_step(int fn, int nx, int nu, const Params64 &P, int *conv);
// admm_f64_rows.hip: sixteen lanes per instance where rows_supported(nx, nu, N).  mpc == NULL: one solve; else the on-chip closed loop of
// mpc->mpc_steps solves (the unrolled horizons and N <= 32 only)
hipError_t launch_f64_rows(int nx, int nu, int N, const Params64 &P, const double *gains, const Mpc64 *mpc);
// admm_f64_rowsim.hip: mpc_steps > 1 solves of the SIM instantiation for (nx, nu, N) in one launch, wherever there is an MPC one
hipError_t launch_rows64_sim(int nx, int nu, int N, const Params64 &P, const double *gains, const Mpc64 &mpc, const Sim64 &S);
// admm_f64_rows_pm.hip / admm_f64_rowsim_pm.hip / admm_f64_thread_pm.hip: the same kernels with per-instance models.  One solve on the sixteen lanes
// wherever launch_f64_rows has an instantiation; the on-chip closed loop (mpc.mpc_steps >= 1 solves; S.plant == NULL: every instance's own Adyn / Bdyn)
// wherever launch_rows64_sim has one; one solve with a thread per instance.  launch_models64_gather: the caller's eight [batch] device arrays into
// the records and rho (q_plus_rho != 0: Q + rho is stored, the code generator's convention)
hipError_t launch_f64_rows_pm(int nx, int nu, int N, const Params64 &P, const Models64 &M);
hipError_t launch_rows64_loop_pm(int nx, int nu, int N, const Params64 &P, const Mpc64 &mpc, const Sim64 &S, const Models64 &M);
hipError_t launch_f64_thread_pm(int nx, int nu, const Params64 &P, const Models64 &M);
hipError_t launch_models64_gather(const double *rho, const double *Kinf, const double *Pinf, const double *Quu_inv, const double *AmBKt, const double *Adyn,
                                  const double *Bdyn, const double *Q, double *rec, double *rho_out, int batch, int nx, int nu, int q_plus_rho);
// admm_f64_rows_ps.hip / admm_f64_rowloop_ps.hip / admm_f64_thread_ps.hip: the same kernels with per-instance settings.  One solve on the sixteen lanes
// wherever launch_f64_rows has an instantiation; the on-chip closed loop (mpc.mpc_steps >= 1 solves, the nominal plant step; every budget >= 1) wherever
// launch_f64_rows has one; one solve with a thread per instance; F64_UPDATE_SLACK and F64_TERMINATION_CONDITION, the two step functions that read a setting
hipError_t launch_f64_rows_ps(int nx, int nu, int N, const Params64 &P, const double *gains, const Settings64 &S);
hipError_t launch_rows64_loop_ps(int nx, int nu, int N, const Params64 &P, const double *gains, const Mpc64 &mpc, const Settings64 &S);
hipError_t launch_f64_thread_ps(int nx, int nu, const Params64 &P, const Settings64 &S);
hipError_t launch_f64_step_ps(int fn, int nx, int nu, const Params64 &P, int *conv, const Settings64 &S);
// admm_f64_plant.hip: x.col(0) <- Adyn * x.col(0) + Bdyn * u.col(0) on the workspace; the same recording u.col(0) in u0_row and sliding the window
// starts (either may be NULL); the same against a separate plant, with a disturbance and the state trajectory
hipError_t launch_plant64(int nx, int nu, double *X, const double *U, const double *mats, int batch, int bpad);
hipError_t launch_plant64_run(int nx, int nu, double *X, const double *U, const double *mats, int batch, int bpad, double *u0_row, int *start, int window_advance);
hipError_t launch_plant64_sim(int nx, int nu, const PlantSim64 &a);
// batch64_helpers.hip: host layout [nb][steps][dim] (nb = 1: shared, stride 1) into steps [step0, step0 + nsteps) of device [steps][dim][stride]; all steps
// of the device array back into the host layout; a window reference gathered into the per-instance array [N][nx][bpad] the one-solve kernels read
hipError_t launch_pack64(const double *src, double *dst, int nb, int steps, int dim, int stride, int step0, int nsteps);
hipError_t launch_unpack64(const double *src, double *dst, int nb, int steps, int dim, int stride);
hipError_t launch_gather_window64(const double *table, const int *start, double *dst, int rows, int N, int nx, int batch, int bpad);
} // namespace tinympc64
