/*
 * tinympc_batch64.h — C-ABI of the batched TinyMPC ADMM solver for `typedef double tinytype`.
 *
 * The reference ships with tinytype = double (src/tinympc/glob_opts.hpp:3: NSTATES 12, NINPUTS 4, NHORIZON 10 as checked
 * in); its code generator switches to float for microcontrollers (codegen.cpp:152).  tinympc_batch.h is the float
 * library; this header is the same drop-in boundary — tiny_solve() (src/tinympc/admm.cpp:111-152) over a batch of
 * independent instances of one problem class — in double, for callers that run the reference as shipped.
 *
 * Same conventions as tinympc_batch.h: plain C, host pointers, column-major matrices (types.hpp:13-21), batched arrays
 * in the array-of-reference-instances layout ([B][N][nx] / [B][N-1][nu]), device-resident workspace that persists
 * between solves (the warm start), every function returns 0 or a negative TinyBatchError (tinympc_batch.h),
 * tiny_batch_last_error() holds the message.  Arithmetic: every product and sum separately rounded in the order of the
 * reference's SSE2 Eigen build with 2-double packets; results are BITWISE equal to the compiled reference (all twelve
 * work arrays, the residuals, status, iter).
 *
 * Scope: tiny_solve, the six step functions, the examples' closed loop (one step, or a whole run in one launch with a sliding reference window),
 * the same loop against a separate plant with a disturbance per step (tiny_batch64_set_plant, tiny_batch64_mpc_run_sim) and the
 * wrapper-style accessors.  Problem classes with a compiled
 * instantiation: (nx, nu) = (12, 4), (4, 1), (8, 4), (12, 2), (4, 2), (4, 4), (16, 4), any horizon N (TINY_FOR_EACH_F64DIMS).
 * Two kernels with identical results: sixteen lanes per instance with the state on chip for the whole solve (nx + nu <= 16 and N <= 64: unrolled instantiations for the
 * reference's horizons, a launch-parameter horizon otherwise; the default where it applies) and one thread per instance with the state in HBM (any N).
 */
#ifndef TINYMPC_BATCH64_H
#define TINYMPC_BATCH64_H

#include "tinympc_batch.h"

#ifdef __cplusplus
extern "C"
{
#endif

    typedef struct TinyBatch64 TinyBatch64;

    /* Replaces the caller-owned TinyCache/TinyWorkspace/TinySettings/TinySolver (types.hpp:26-107) with tinytype = double
     * (glob_opts.hpp:3).  The workspace starts all zero (quadrotor_hovering.cpp:49-71). */
    const char *tiny_batch64_last_error(void);
    int tiny_batch64_create(TinyBatch64 **out, int nx, int nu, int N, int batch, int device);
    void tiny_batch64_destroy(TinyBatch64 *tb);

    /* TinyCache (types.hpp:26-34) and the per-problem members of TinyWorkspace (types.hpp:82-85), column-major doubles. */
    int tiny_batch64_set_cache(TinyBatch64 *tb, double rho, const double *Kinf, const double *Pinf, const double *Quu_inv, const double *AmBKt);
    int tiny_batch64_set_dynamics(TinyBatch64 *tb, const double *Adyn, const double *Bdyn, const double *Q);
    /* TinySettings (types.hpp:39-47) */
    int tiny_batch64_set_settings(TinyBatch64 *tb, double abs_pri_tol, double abs_dua_tol, int max_iter, int check_termination,
                                  int en_state_bound, int en_input_bound);

    /* wrapper twins (tiny_wrapper.hpp:14-23), batched, double: `shared` != 0 means one [N][nx] / [N-1][nu] array for the batch */
    int tiny_batch64_set_x0(TinyBatch64 *tb, const double *x0);                 /* [B][nx] -> x.col(0) */
    int tiny_batch64_set_xref(TinyBatch64 *tb, const double *xref, int shared); /* [B or 1][N][nx] */
    int tiny_batch64_set_xmin(TinyBatch64 *tb, const double *v, int shared);
    int tiny_batch64_set_xmax(TinyBatch64 *tb, const double *v, int shared);
    int tiny_batch64_set_umin(TinyBatch64 *tb, const double *v, int shared);
    int tiny_batch64_set_umax(TinyBatch64 *tb, const double *v, int shared);
    int tiny_batch64_reset_dual_variables(TinyBatch64 *tb);                     /* y = 0, g = 0 (tiny_wrapper.cpp:131) */
    /* tiny_solve() for every instance (admm.cpp:111-152): 0 = all converged, 1 = some hit max_iter, < 0 = error */
    int tiny_batch64_solve(TinyBatch64 *tb);

    /* The six functions tiny_solve() is made of (admm.hpp:12-18, admm.cpp:15-109), each over the whole batch: one launch that reads
     * and writes the members the reference function does.  termination_condition evaluates `work->iter % check_termination`
     * with the iter field of the workspace (set_status), writes the four residual fields when that holds and returns the
     * function's bool per instance in converged[batch]. */
    int tiny_batch64_forward_pass(TinyBatch64 *tb);
    int tiny_batch64_update_slack(TinyBatch64 *tb);
    int tiny_batch64_update_dual(TinyBatch64 *tb);
    int tiny_batch64_update_linear_cost(TinyBatch64 *tb);
    int tiny_batch64_backward_pass_grad(TinyBatch64 *tb);
    int tiny_batch64_termination_condition(TinyBatch64 *tb, int *converged);

    /* One step of the examples' closed loop (quadrotor_hovering.cpp:95-111) on the device: y = g = 0, tiny_solve, then the plant
     * update x.col(0) <- Adyn * x.col(0) + Bdyn * u.col(0) in the order Eigen evaluates that expression (bitwise equal to
     * the compiled example).  Returns what tiny_batch64_solve returns.  tiny_batch64_get_first_columns reads x.col(0) (after the
     * plant update: the next x0) and u.col(0) (the control just computed) without moving the whole horizon; either may be NULL. */
    int tiny_batch64_mpc_step(TinyBatch64 *tb);
    int tiny_batch64_get_first_columns(TinyBatch64 *tb, double *x0, double *u0);

    /* The tracking example's reference (quadrotor_tracking.cpp:101-102: Xref = Xref_total.block(0, k, nx, N)) without an upload per step: one
     * trajectory table for the batch and a window start per instance, both kept on the device.  Xref_b row i is
     * table[min(start[b] + i, rows - 1)]; needs rows >= N, 0 <= start[b] and start[b] + N <= rows.  tiny_batch64_solve, the six step
     * functions and tiny_batch64_mpc_step (which advances by 0) read the window; a later tiny_batch64_set_xref returns to an array.
     * tiny_batch64_get_xref_start reads the starts back after a run has slid them. */
    int tiny_batch64_set_xref_window(TinyBatch64 *tb, const double *table /*[rows][nx]*/, int rows, const int *start /*[B]*/);
    int tiny_batch64_get_xref_start(TinyBatch64 *tb, int *start /*[B]*/);

    /* `steps` closed-loop steps without the host in between: steps x {y = g = 0; tiny_solve; x.col(0) <- Adyn * x.col(0) + Bdyn * u.col(0);
     * start[b] += window_advance}, results identical to `steps` single steps (and, with an array reference, to `steps` calls of
     * tiny_batch64_mpc_step).  Where the sixteen-lane kernel holds the whole workspace on chip (its unrolled instantiations and horizons <= 32) all
     * solves run in ONE launch and nothing but u.col(0) leaves the chip between two of them; elsewhere the same steps are enqueued as a launch
     * sequence with one read-back at the end.  tiny_batch64_closed_loop_kernel_name says which: the on-chip instantiation carries an ",mpc"
     * suffix ("rows64<12,4,10,mpc>", "rows64<12,2,n<=32,mpc>"), otherwise it is the solve kernel's name.  Returns what the LAST step's
     * tiny_batch64_solve would return; steps < 1 or window_advance < 0 is TINY_BATCH_EINVAL; window_advance without a window is ignored.
     * _traj also records u.col(0) of every step. */
    int tiny_batch64_mpc_run(TinyBatch64 *tb, int steps, int window_advance);
    int tiny_batch64_mpc_run_traj(TinyBatch64 *tb, int steps, int window_advance, double *u0_traj_host /*[steps][B][nu]*/);
    const char *tiny_batch64_closed_loop_kernel_name(TinyBatch64 *tb);

    /* The closed loop against a plant that is not the model (the float library's tiny_batch_set_plant family, in double): one controller, one
     * plant shared by the batch or one per instance, a disturbance per step, the state trajectory as an output.  A, B are column-major,
     * [1 or batch][nx*nx] and [1 or batch][nx*nu] (`shared` != 0: one pair); the solver never reads them.  tiny_batch64_plant_mode: 0 the model's
     * own Adyn / Bdyn, 1 one shared plant, 2 one plant per instance.  A plant set on the handle is honoured by EVERY closed-loop call
     * (tiny_batch64_mpc_step, _mpc_run and _mpc_run_traj included); with none set those calls enqueue exactly what they did before.
     * The plant step is x.col(0) <- (A_p * x.col(0) + B_p * u.col(0)) + w_k: the product in the plant update's order above, then ONE separately
     * rounded addition; with w == NULL no addition is executed.  tiny_batch64_mpc_step_sim is tiny_batch64_mpc_step with this step's [batch][nx]
     * disturbance; tiny_batch64_mpc_run_sim is tiny_batch64_mpc_run_traj (its return value and argument checks) with w [steps][batch][nx],
     * u0_traj [steps][batch][nu] and x_traj [steps][batch][nx], each of which may be NULL: row k of x_traj is x.col(0) after step k's plant step.
     * A run is simulated when a plant is set or w / x_traj is passed.  Where the loop is on chip a simulated run of steps > 1 is ONE launch of the
     * ",sim" instantiation; elsewhere it is the launch sequence with the simulated plant kernel per step.  While a plant is set
     * tiny_batch64_closed_loop_kernel_name carries ",sim" in place of ",mpc" ("rows64<12,4,10,sim>"); a run that only passes w / x_traj takes the
     * same instantiation although the name, which knows the handle alone, says ",mpc". */
    int tiny_batch64_set_plant(TinyBatch64 *tb, const double *A, const double *B, int shared);
    int tiny_batch64_clear_plant(TinyBatch64 *tb);
    int tiny_batch64_plant_mode(TinyBatch64 *tb);
    int tiny_batch64_mpc_step_sim(TinyBatch64 *tb, const double *w /*[batch][nx] or NULL*/);
    int tiny_batch64_mpc_run_sim(TinyBatch64 *tb, int steps, int window_advance, const double *w /*[steps][batch][nx] or NULL*/,
                                 double *u0_traj /*[steps][batch][nu] or NULL*/, double *x_traj /*[steps][batch][nx] or NULL*/);
    /* tiny_batch64_mpc_run_sim with the per-step solver log: row k of iter_log / status_log ([steps][batch] ints, either may be NULL) holds work.iter and
     * work.status of every instance after the solve of step k, as tiny_batch64_get_status would return them there.  A log does not make a run simulated
     * and picks no kernel; with both NULL the call is tiny_batch64_mpc_run_sim.  A run that asks for a log is enqueued as the launch sequence — the
     * solve kernel tiny_batch64_kernel_name() names, per step, with iter[] / status[] copied behind each solve — also where the run without a log is ONE
     * launch: the on-chip loops do not log.  tiny_batch64_closed_loop_kernel_name, which knows the handle alone, does not change. */
    int tiny_batch64_mpc_run_log(TinyBatch64 *tb, int steps, int window_advance, const double *w, double *u0_traj, double *x_traj,
                                 int *iter_log /*[steps][batch] or NULL*/, int *status_log /*[steps][batch] or NULL*/);

    /* Per-instance models (the float library's tiny_batch_set_models family, in double): every instance its own TinyCache{rho, Kinf, Pinf, Quu_inv,
     * AmBKt} (types.hpp:26-34) and its own Adyn, Bdyn, Q (types.hpp:82-85), each array [batch][...] with every instance's matrix column-major.  This
     * satisfies the "cache and dynamics set" readiness check of a solve and replaces the batch-shared cache / dynamics until
     * tiny_batch64_clear_models(); settings stay per batch.  The records live on the device, one per instance in the layout Kinf | Pinf | Quu_inv |
     * AmBKt | Adyn | Bdyn | Q (3 nx^2 + 2 nx nu + nu^2 + nx doubles: 4.4 KB for the quadrotor) with rho beside them; every kernel reads its
     * instance's record directly.  _device takes DEVICE pointers on the handle's device: one gather kernel on the null stream, asynchronous, nothing
     * passes through the host.
     * Served: tiny_batch64_solve on both kernels (every sixteen-lane instantiation, every class of the thread-per-instance kernel), with shared or
     * per-instance bounds and any reference, and every closed-loop call.  A run is ONE launch wherever it is without per-instance models; with no
     * plant set every instance's plant step uses its own Adyn / Bdyn, and a plant that is set stays independent of the models in all three modes.
     * tiny_batch64_kernel_name and _closed_loop_kernel_name carry ",pm" last inside the brackets ("rows64<12,4,10,pm>", "rows64<12,2,n<=32,pm>",
     * "thread64<16,4,pm>", "rows64<12,4,10,mpc,pm>", "rows64<12,4,10,sim,pm>").  Refused with TINY_BATCH_EUNSUPPORTED and a message: the six
     * single-function step calls, which read one shared model. */
    int tiny_batch64_set_models(TinyBatch64 *tb, const double *rho /*[B]*/, const double *Kinf /*[B][nu*nx]*/, const double *Pinf /*[B][nx*nx]*/,
                                const double *Quu_inv /*[B][nu*nu]*/, const double *AmBKt /*[B][nx*nx]*/, const double *Adyn /*[B][nx*nx]*/,
                                const double *Bdyn /*[B][nx*nu]*/, const double *Q /*[B][nx]*/);
    int tiny_batch64_set_models_device(TinyBatch64 *tb, const double *d_rho, const double *d_Kinf, const double *d_Pinf, const double *d_Quu_inv,
                                       const double *d_AmBKt, const double *d_Adyn, const double *d_Bdyn, const double *d_Q);
    /* back to the batch-shared cache / dynamics of tiny_batch64_set_cache / tiny_batch64_set_dynamics; the device memory of the records is released */
    int tiny_batch64_clear_models(TinyBatch64 *tb);
    /* 1 while per-instance models are in force, 0 otherwise */
    int tiny_batch64_models_per_instance(TinyBatch64 *tb);
    /* HOST fp64 systems in ([B][...] as above; Q, R without rho), tiny_batch_riccati_device on the handle's device, the result installed as the handle's
     * per-instance models with the conventions of the code generator and NO rounding: Adyn = A, Bdyn = B, Q = Q + rho, the cache the fp64 result
     * itself.  iters ([B], may be NULL) as tiny_batch_riccati_device.  Any failed system: TINY_BATCH_EINVAL and the handle's models are unchanged. */
    int tiny_batch64_set_systems(TinyBatch64 *tb, const double *A, const double *B, const double *Q, const double *R, const double *rho, int *iters);

    /* Per-instance settings (the float library's tiny_batch_set_instance_settings family, in double): TinySettings (types.hpp:39-47) per instance.  Every
     * pointer is a host array [batch] or NULL; NULL = that field stays the batch's value from tiny_batch64_set_settings (which must have been called:
     * TINY_BATCH_ENOTREADY otherwise; a later tiny_batch64_set_settings moves the NULL fields with it).  The call replaces any earlier per-instance
     * settings.  check_termination[b] < 1: TINY_BATCH_EINVAL, the message names the first such index (admm.cpp:93); the tolerances are doubles, compared
     * with `<` as in the reference (admm.cpp:100-103).  From then on every solve entry point — tiny_batch64_solve, tiny_batch64_mpc_step[_sim],
     * tiny_batch64_mpc_run[_traj|_sim|_log], tiny_batch64_termination_condition, and tiny_batch64_update_slack through the bound flags — treats instance b
     * bit for bit as the reference's fp64 tiny_solve treats a solver whose TinySettings are instance b's.  max_iter[b] <= 0: status 11, iter 1, counted
     * unsolved, nothing else of that instance is written.  tiny_batch64_solve returns 1 if any instance did not converge within its own budget.
     * Kernels: ",ps" last inside the brackets — "rows64<12,4,10,ps>", "rows64<12,2,n<=32,ps>", "rows64<4,2,n<=64,ps>" wherever the sixteen lanes serve the
     * solve, "thread64<16,4,ps>" elsewhere, with shared or per-instance bounds and any reference.  A run is ONE launch ("rows64<12,4,10,mpc,ps>") where it
     * is one without per-instance settings AND every budget is >= 1, no plant is set, the call passes neither w nor x_traj and asks for no log; every
     * other run is the launch sequence of the ",ps" solve kernel and the plant kernel per step, with the same bits.  Unlike the float library, which
     * refuses it, a run in which some instance has no budget is served, by the sequence (as this library has always served a batch-wide max_iter <= 0):
     * that instance's status is 11 at every step and the plant steps on with the u.col(0) its workspace holds.  tiny_batch64_closed_loop_kernel_name,
     * which knows the handle alone, says ",mpc,ps" whenever no plant is set and every budget is >= 1, also for a call that passes w or x_traj and
     * therefore runs as a sequence.  Refused with TINY_BATCH_EUNSUPPORTED and a message, at the next solve, step function or run and with nothing
     * launched: per-instance settings together with per-instance models, in either order of the two setters (the two names then read "unsupported"). */
    int tiny_batch64_set_instance_settings(TinyBatch64 *tb, const double *abs_pri_tol, const double *abs_dua_tol, const int *max_iter,
                                           const int *check_termination, const int *en_state_bound, const int *en_input_bound);
    /* back to the batch's one set of tiny_batch64_set_settings: kernels, kernel names and results are what they were */
    int tiny_batch64_clear_instance_settings(TinyBatch64 *tb);
    /* 1 while per-instance settings are in force, 0 otherwise */
    int tiny_batch64_settings_per_instance(TinyBatch64 *tb);

    /* Implementation: 0 = automatic (the second where (nx, nu, N) has an instantiation, else the first), 1 = one thread per
     * instance with the state in HBM (any N), 2 = sixteen lanes per instance with the state in registers for the whole solve
     * (instantiated (nx, nu, N): (12,4,10) as shipped, (12,4,20), (12,4,30), (4,1,10), (8,4,9)).  Identical results. */
    int tiny_batch64_select_kernel(TinyBatch64 *tb, int which);
    const char *tiny_batch64_kernel_name(TinyBatch64 *tb);

    /* whole workspace, ids of TinyBatchArray */
    int tiny_batch64_set_array(TinyBatch64 *tb, int id, const double *src);
    int tiny_batch64_get_array(TinyBatch64 *tb, int id, double *dst);
    /* work->iter, work->status and the four residual fields (pri_state, pri_input, dua_state, dua_input); NULL = skip */
    int tiny_batch64_get_status(TinyBatch64 *tb, int *iter, int *status, double *residuals);
    int tiny_batch64_set_status(TinyBatch64 *tb, const int *iter, const int *status, const double *residuals);

#ifdef __cplusplus
}
#endif
#endif
