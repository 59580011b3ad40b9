// admm_f64_thread.hip — the thread-per-instance kernels of the fp64 library: admm_f64_kernel (all ADMM iterations in one launch) and
// admm_f64_step_kernel (the six functions tiny_solve() is made of, one launch each), with their launchers.  Under TINY_F64PM_UNIT
// (admm_f64_thread_pm.hip) the unit holds the per-instance-model instantiations of admm_f64_kernel and their launcher instead, under TINY_F64PS_UNIT
// (admm_f64_thread_ps.hip) the per-instance-settings ones.
//
// One thread per instance, state in HBM.  Every per-instance array is stored instance-minor — element (step, row) of
// instance b at ((step * dim + row) * Bpad + b) — so that the 64 instances of a wavefront read and write 512 contiguous
// bytes per element.  A converged instance stops storing exactly where the reference returns (admm.cpp:135-137: before the v/z copy and
// the backward pass).  Arithmetic: tiny_solve() of the reference (admm.cpp:15-152) statement by statement in the orders of f64_math.h.
#include "f64_math.h"

namespace
{
using namespace tinympc64;

__device__ __forceinline__ Models64 models_of(const Models64 &m) { return m; }
__device__ __forceinline__ Settings64 settings_of(const Settings64 &s) { return s; }
#define SETTING_(field) (SET ? my.field : P.field)

// PM (one trailing argument, a Models64: the ",pm" instantiations of admm_f64_thread_pm.hip): a thread reads its own instance's record and rho from
// device memory instead of the block's LDS copy of the one shared model; a thread past the batch addresses the last instance's and stores nothing.
template <int NX, int NU, class... PMA>
__global__ __launch_bounds__(WAVE64) void admm_f64_kernel(const Params64 P, const PMA... pma)
{
    static_assert(!(NX >= 8 && NU >= 8), "both dims >= 8: Eigen switches to its GEMV kernel, not restated here");
    constexpr bool PM = (false || ... || std::is_same<PMA, Models64>::value);
    // SET (one trailing argument, a Settings64: the ",ps" instantiations of admm_f64_thread_ps.hip): a thread reads its own instance's tolerances, budget,
    // check_termination and bound flags from the instance's record; P.max_iter is the batch's largest budget and bounds the loop
    constexpr bool SET = (false || ... || std::is_same<PMA, Settings64>::value);
    static_assert(sizeof...(PMA) == (PM ? 1 : 0) + (SET ? 1 : 0) && !(PM && SET), "at most one trailing argument, a Models64 or a Settings64");
    constexpr int NMAT = NU * NX + NX * NX + NU * NU + NX * NX + NX * NX + NX * NU + NX;
    __shared__ double mats[PM ? 1 : NMAT];
    const double *mats_of_thread = mats;
    double rho_of_thread = P.rho;
    if constexpr (PM)
    {
        const Models64 MO = models_of(pma...);
        const size_t me = blockIdx.x * WAVE64 + threadIdx.x, bm = me < (size_t)P.batch ? me : (size_t)P.batch - 1;
        mats_of_thread = MO.rec + bm * MO.stride;
        rho_of_thread = MO.rho[bm];
    }
    else
    {
        for (int e = threadIdx.x; e < NMAT; e += WAVE64) mats[e] = P.mats[e];
        __syncthreads();
    }
    const double *K = mats_of_thread, *Pinf = K + NU * NX, *Quu = Pinf + NX * NX, *Am = Quu + NU * NU, *A = Am + NX * NX, *Bm = A + NX * NX,
                 *Q = Bm + NX * NU;

    const int b = blockIdx.x * WAVE64 + threadIdx.x;
    const bool valid = b < P.batch;
    const int N = P.N;
    const size_t bp = (size_t)P.bpad;
    const double rho = rho_of_thread;
    auto at = [&](int id, int step, int row, int dim) -> double & { return P.arr[id][((size_t)step * dim + row) * bp + b]; };
    auto in = [&](const double *base, int stride, int step, int row, int dim) {
        return base[((size_t)step * dim + row) * (size_t)stride + (stride > 1 ? b : 0)];
    };

    if (P.max_iter <= 0) // tiny_solve only sets status and iter (admm.cpp:114-117,151)
    {
        if (valid)
        {
            P.status[b] = ST_UNSOLVED; P.iter[b] = 1;
            atomicAdd(P.n_unsolved, 1);
        }
        return;
    }
    // the settings of this thread, SETTING_(field): the batch's, read where they always were, or (SET) its instance's; a thread past the batch reads the
    // last instance's record
    [[maybe_unused]] InstSettings64 my{};
    if constexpr (SET) my = settings_of(pma...).rec[valid ? b : P.batch - 1];
    double x0[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) x0[j] = valid ? at(TINY_ARR_X, 0, j, NX) : 0.0;
    double r_ps = 0, r_pi = 0, r_ds = 0, r_di = 0;
    if (valid)
    {
        r_ps = P.res[0 * bp + b]; r_pi = P.res[1 * bp + b]; r_ds = P.res[2 * bp + b]; r_di = P.res[3 * bp + b];
    }
    int st = ST_UNSOLVED, itn = 1; // admm.cpp:114-115
    bool active = valid;
    if constexpr (SET) active = valid && my.max_iter > 0; // a thread without a budget stays with its wave, inactive: status and iter are all it writes
    for (int it = 0; it < P.max_iter; ++it)
    {
        if (!__any(active)) break;
        if (active)
        {
            itn = it + 1; // admm.cpp:120
            // ---- forward_pass (:27-37) + update_slack (:45-61) + update_dual (:67-71) + update_linear_cost (:77-85) + residuals (:95-98) ----
            double x[NX], pN[NX];
#pragma unroll
            for (int j = 0; j < NX; j++) x[j] = x0[j];
            double pri_x = 0, dua_x = 0, pri_u = 0, dua_u = 0;
            for (int i = 0; i < N; i++)
            {
                double u[NU], xn[NX];
                if (i < N - 1)
                {
#pragma unroll
                    for (int j = 0; j < NU; j++) u[j] = -row_dot<NU, NX>(K, j, x) - at(TINY_ARR_D, i, j, NU);           // :31
#pragma unroll
                    for (int j = 0; j < NX; j++) xn[j] = row_dot<NX, NX>(A, j, x) + row_dot<NX, NU>(Bm, j, u);           // :35
#pragma unroll
                    for (int j = 0; j < NU; j++)
                    {
                        const double y = at(TINY_ARR_Y, i, j, NU);
                        double zn = u[j] + y;                                                                             // :47
                        if (SETTING_(en_input_bound))                                                                   // :51-54
                        {
                            const double lo = in(P.umin, P.ub_stride, i, j, NU), hi = in(P.umax, P.ub_stride, i, j, NU);
                            zn = (lo < zn) ? zn : lo;
                            zn = (zn < hi) ? zn : hi;
                        }
                        const double yn = y + u[j] - zn;                                                                  // :69
                        const double pu = fabs(u[j] - zn), du = fabs(at(TINY_ARR_Z, i, j, NU) - zn);                      // :97-98
                        pri_u = (i == 0 && j == 0) ? pu : (pu > pri_u ? pu : pri_u);
                        dua_u = (i == 0 && j == 0) ? du : (du > dua_u ? du : dua_u);
                        at(TINY_ARR_U, i, j, NU) = u[j];
                        at(TINY_ARR_ZNEW, i, j, NU) = zn;
                        at(TINY_ARR_Y, i, j, NU) = yn;
                        at(TINY_ARR_R, i, j, NU) = -rho * (zn - yn);                                                      // :80
                    }
                }
#pragma unroll
                for (int j = 0; j < NX; j++)
                {
                    const double g = at(TINY_ARR_G, i, j, NX);
                    double vn = x[j] + g;                                                                                 // :48
                    if (SETTING_(en_state_bound))                                                                       // :57-60
                    {
                        const double lo = in(P.xmin, P.xb_stride, i, j, NX), hi = in(P.xmax, P.xb_stride, i, j, NX);
                        vn = (lo < vn) ? vn : lo;
                        vn = (vn < hi) ? vn : hi;
                    }
                    const double gn = g + x[j] - vn;                                                                      // :70
                    const double px = fabs(x[j] - vn), dx = fabs(at(TINY_ARR_V, i, j, NX) - vn);                          // :95-96
                    pri_x = (i == 0 && j == 0) ? px : (px > pri_x ? px : pri_x);
                    dua_x = (i == 0 && j == 0) ? dx : (dx > dua_x ? dx : dua_x);
                    at(TINY_ARR_X, i, j, NX) = x[j];
                    at(TINY_ARR_VNEW, i, j, NX) = vn;
                    at(TINY_ARR_G, i, j, NX) = gn;
                    double q = -(in(P.xref, P.xref_stride, i, j, NX) * Q[j]);                                             // :81
                    q = q - rho * (vn - gn);                                                                              // :82
                    at(TINY_ARR_Q, i, j, NX) = q;
                    if (i == N - 1) pN[j] = rho * (vn - gn); // second half of :84, applied below
                }
                if (i < N - 1)
                {
#pragma unroll
                    for (int j = 0; j < NX; j++) x[j] = xn[j];
                }
            }
            {
                // p.col(N-1) = -(Xref.col(N-1)^T * Pinf)  (:83), then -= rho * (vnew - g)  (:84)
                double xr[NX];
#pragma unroll
                for (int k = 0; k < NX; k++) xr[k] = in(P.xref, P.xref_stride, N - 1, k, NX);
#pragma unroll
                for (int j = 0; j < NX; j++)
                {
                    double t[NX];
#pragma unroll
                    for (int k = 0; k < NX; k++) t[k] = xr[k] * Pinf[j * NX + k];
                    const double pt = -vec_sum(t);
                    pN[j] = pt - pN[j];
                    at(TINY_ARR_P, N - 1, j, NX) = pN[j];
                }
            }
            // ---- termination_condition (:91-109) ----
            bool conv = false;
            if ((it + 1) % SETTING_(check_termination) == 0)
            {
                r_ps = pri_x; r_ds = dua_x * rho; r_pi = pri_u; r_di = dua_u * rho;
                conv = (r_ps < SETTING_(abs_pri_tol)) && (r_pi < SETTING_(abs_pri_tol)) && (r_ds < SETTING_(abs_dua_tol)) && (r_di < SETTING_(abs_dua_tol));
            }
            if (conv)
            {
                st = ST_SOLVED; // :136, returns before the v/z copy and the backward pass
                active = false;
            }
            else
            {
                // ---- v = vnew, z = znew (:141-142) + backward_pass_grad (:15-22) ----
#pragma unroll
                for (int j = 0; j < NX; j++) at(TINY_ARR_V, N - 1, j, NX) = at(TINY_ARR_VNEW, N - 1, j, NX);
                double pn[NX];
#pragma unroll
                for (int j = 0; j < NX; j++) pn[j] = pN[j];
                for (int i = N - 2; i >= 0; i--)
                {
                    double r[NU], tmp[NU], dn[NU], pi[NX];
#pragma unroll
                    for (int j = 0; j < NU; j++)
                    {
                        at(TINY_ARR_Z, i, j, NU) = at(TINY_ARR_ZNEW, i, j, NU);
                        r[j] = at(TINY_ARR_R, i, j, NU);
                    }
#pragma unroll
                    for (int j = 0; j < NU; j++) // Bdyn^T p_{i+1} + r_i: column j of Bdyn is contiguous -> vectorised reduction
                    {
                        double t[NX];
#pragma unroll
                        for (int k = 0; k < NX; k++) t[k] = Bm[j * NX + k] * pn[k];
                        tmp[j] = vec_sum(t) + r[j];
                    }
#pragma unroll
                    for (int j = 0; j < NU; j++) dn[j] = row_dot<NU, NU>(Quu, j, tmp);                                    // :19
#pragma unroll
                    for (int j = 0; j < NX; j++)
                    {
                        at(TINY_ARR_V, i, j, NX) = at(TINY_ARR_VNEW, i, j, NX);
                        double t[NX], tk[NU];
#pragma unroll
                        for (int k = 0; k < NX; k++) t[k] = Am[k * NX + j] * pn[k];
                        const double a = (NU == 1 && NX % PS == 0) ? seq_sum(t) : novec_sum(t);
#pragma unroll
                        for (int m = 0; m < NU; m++) tk[m] = K[j * NU + m] * r[m]; // Kinf^T r: column j of Kinf is contiguous
                        pi[j] = at(TINY_ARR_Q, i, j, NX) + a - vec_sum(tk);                                               // :20
                    }
#pragma unroll
                    for (int j = 0; j < NU; j++) at(TINY_ARR_D, i, j, NU) = dn[j];
#pragma unroll
                    for (int j = 0; j < NX; j++)
                    {
                        at(TINY_ARR_P, i, j, NX) = pi[j];
                        pn[j] = pi[j];
                    }
                }
                if constexpr (SET) active = it + 1 < my.max_iter; // its own budget is used up: the thread leaves behind its last backward pass
            }
        }
    }
    if (valid)
    {
        if (!SET || my.max_iter > 0)
        {
            P.res[0 * bp + b] = r_ps; P.res[1 * bp + b] = r_pi; P.res[2 * bp + b] = r_ds; P.res[3 * bp + b] = r_di;
        }
        P.status[b] = st;
        P.iter[b] = itn;
        if (st != ST_SOLVED) atomicAdd(P.n_unsolved, 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The six functions tiny_solve() is made of (admm.hpp:12-18), one launch each, one thread per instance: each reads and writes
// exactly the members the reference function does, in the same arithmetic as the fused kernels (above, and admm_f64_rows.hip).
// ---------------------------------------------------------------------------------------------------------------------
template <int NX, int NU, int FN>
__global__ __launch_bounds__(WAVE64) void admm_f64_step_kernel(const Params64 P, int *__restrict__ conv_out)
{
    constexpr int NMAT = NU * NX + NX * NX + NU * NU + NX * NX + NX * NX + NX * NU + NX;
    __shared__ double mats[NMAT];
    for (int e = threadIdx.x; e < NMAT; e += WAVE64) mats[e] = P.mats[e];
    __syncthreads();
    const double *K = mats, *Pinf = K + NU * NX, *Quu = Pinf + NX * NX, *Am = Quu + NU * NU, *A = Am + NX * NX, *Bm = A + NX * NX,
                 *Q = Bm + NX * NU;
    const int b = blockIdx.x * WAVE64 + threadIdx.x;
    if (b >= P.batch) return;
    const int N = P.N;
    const size_t bp = (size_t)P.bpad;
    const double rho = P.rho;
    auto at = [&](int id, int step, int row, int dim) -> double & { return P.arr[id][((size_t)step * dim + row) * bp + b]; };
    auto in = [&](const double *base, int stride, int step, int row, int dim) {
        return base[((size_t)step * dim + row) * (size_t)stride + (stride > 1 ? b : 0)];
    };
    if constexpr (FN == F64_FORWARD_PASS) // admm.cpp:27-37
    {
        double x[NX];
#pragma unroll
        for (int j = 0; j < NX; j++) x[j] = at(TINY_ARR_X, 0, j, NX);
        for (int i = 0; i < N - 1; i++)
        {
            double u[NU], xn[NX];
#pragma unroll
            for (int j = 0; j < NU; j++) u[j] = -row_dot<NU, NX>(K, j, x) - at(TINY_ARR_D, i, j, NU);
#pragma unroll
            for (int j = 0; j < NX; j++) xn[j] = row_dot<NX, NX>(A, j, x) + row_dot<NX, NU>(Bm, j, u);
#pragma unroll
            for (int j = 0; j < NU; j++) at(TINY_ARR_U, i, j, NU) = u[j];
#pragma unroll
            for (int j = 0; j < NX; j++) { at(TINY_ARR_X, i + 1, j, NX) = xn[j]; x[j] = xn[j]; }
        }
    }
    else if constexpr (FN == F64_UPDATE_SLACK) // admm.cpp:45-61
    {
        for (int i = 0; i < N - 1; i++)
#pragma unroll
            for (int j = 0; j < NU; j++)
            {
                double zn = at(TINY_ARR_U, i, j, NU) + at(TINY_ARR_Y, i, j, NU);
                if (P.en_input_bound)
                {
                    const double lo = in(P.umin, P.ub_stride, i, j, NU), hi = in(P.umax, P.ub_stride, i, j, NU);
                    zn = (lo < zn) ? zn : lo;
                    zn = (zn < hi) ? zn : hi;
                }
                at(TINY_ARR_ZNEW, i, j, NU) = zn;
            }
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = 0; j < NX; j++)
            {
                double vn = at(TINY_ARR_X, i, j, NX) + at(TINY_ARR_G, i, j, NX);
                if (P.en_state_bound)
                {
                    const double lo = in(P.xmin, P.xb_stride, i, j, NX), hi = in(P.xmax, P.xb_stride, i, j, NX);
                    vn = (lo < vn) ? vn : lo;
                    vn = (vn < hi) ? vn : hi;
                }
                at(TINY_ARR_VNEW, i, j, NX) = vn;
            }
    }
    else if constexpr (FN == F64_UPDATE_DUAL) // admm.cpp:67-71
    {
        for (int i = 0; i < N - 1; i++)
#pragma unroll
            for (int j = 0; j < NU; j++) at(TINY_ARR_Y, i, j, NU) = at(TINY_ARR_Y, i, j, NU) + at(TINY_ARR_U, i, j, NU) - at(TINY_ARR_ZNEW, i, j, NU);
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = 0; j < NX; j++) at(TINY_ARR_G, i, j, NX) = at(TINY_ARR_G, i, j, NX) + at(TINY_ARR_X, i, j, NX) - at(TINY_ARR_VNEW, i, j, NX);
    }
    else if constexpr (FN == F64_UPDATE_LINEAR_COST) // admm.cpp:77-85
    {
        for (int i = 0; i < N - 1; i++)
#pragma unroll
            for (int j = 0; j < NU; j++) at(TINY_ARR_R, i, j, NU) = -rho * (at(TINY_ARR_ZNEW, i, j, NU) - at(TINY_ARR_Y, i, j, NU));
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = 0; j < NX; j++)
            {
                double q = -(in(P.xref, P.xref_stride, i, j, NX) * Q[j]);
                q = q - rho * (at(TINY_ARR_VNEW, i, j, NX) - at(TINY_ARR_G, i, j, NX));
                at(TINY_ARR_Q, i, j, NX) = q;
            }
        double xr[NX];
#pragma unroll
        for (int k = 0; k < NX; k++) xr[k] = in(P.xref, P.xref_stride, N - 1, k, NX);
#pragma unroll
        for (int j = 0; j < NX; j++)
        {
            double t[NX];
#pragma unroll
            for (int k = 0; k < NX; k++) t[k] = xr[k] * Pinf[j * NX + k];
            const double pt = -vec_sum(t);
            at(TINY_ARR_P, N - 1, j, NX) = pt - rho * (at(TINY_ARR_VNEW, N - 1, j, NX) - at(TINY_ARR_G, N - 1, j, NX));
        }
    }
    else if constexpr (FN == F64_TERMINATION_CONDITION) // admm.cpp:91-109
    {
        bool conv = false;
        if (P.iter[b] % P.check_termination == 0)
        {
            double pri_x = 0, dua_x = 0, pri_u = 0, dua_u = 0;
            for (int i = 0; i < N; i++)
#pragma unroll
                for (int j = 0; j < NX; j++)
                {
                    const double vn = at(TINY_ARR_VNEW, i, j, NX);
                    const double px = fabs(at(TINY_ARR_X, i, j, NX) - vn), dx = fabs(at(TINY_ARR_V, i, j, NX) - vn);
                    pri_x = (i == 0 && j == 0) ? px : (px > pri_x ? px : pri_x);
                    dua_x = (i == 0 && j == 0) ? dx : (dx > dua_x ? dx : dua_x);
                }
            for (int i = 0; i < N - 1; i++)
#pragma unroll
                for (int j = 0; j < NU; j++)
                {
                    const double zn = at(TINY_ARR_ZNEW, i, j, NU);
                    const double pu = fabs(at(TINY_ARR_U, i, j, NU) - zn), du = fabs(at(TINY_ARR_Z, i, j, NU) - zn);
                    pri_u = (i == 0 && j == 0) ? pu : (pu > pri_u ? pu : pri_u);
                    dua_u = (i == 0 && j == 0) ? du : (du > dua_u ? du : dua_u);
                }
            const double r_ps = pri_x, r_ds = dua_x * rho, r_pi = pri_u, r_di = dua_u * rho;
            P.res[0 * bp + b] = r_ps; P.res[1 * bp + b] = r_pi; P.res[2 * bp + b] = r_ds; P.res[3 * bp + b] = r_di;
            conv = (r_ps < P.abs_pri_tol) && (r_pi < P.abs_pri_tol) && (r_ds < P.abs_dua_tol) && (r_di < P.abs_dua_tol);
        }
        conv_out[b] = conv ? 1 : 0;
    }
    else // F64_BACKWARD_PASS_GRAD, admm.cpp:15-22
    {
        double pn[NX];
#pragma unroll
        for (int j = 0; j < NX; j++) pn[j] = at(TINY_ARR_P, N - 1, j, NX);
        for (int i = N - 2; i >= 0; i--)
        {
            double r[NU], tmp[NU], dn[NU], pi[NX];
#pragma unroll
            for (int j = 0; j < NU; j++) r[j] = at(TINY_ARR_R, i, j, NU);
#pragma unroll
            for (int j = 0; j < NU; j++)
            {
                double t[NX];
#pragma unroll
                for (int k = 0; k < NX; k++) t[k] = Bm[j * NX + k] * pn[k];
                tmp[j] = vec_sum(t) + r[j];
            }
#pragma unroll
            for (int j = 0; j < NU; j++) dn[j] = row_dot<NU, NU>(Quu, j, tmp);
#pragma unroll
            for (int j = 0; j < NX; j++)
            {
                double t[NX], tk[NU];
#pragma unroll
                for (int k = 0; k < NX; k++) t[k] = Am[k * NX + j] * pn[k];
                const double a = (NU == 1 && NX % PS == 0) ? seq_sum(t) : novec_sum(t);
#pragma unroll
                for (int m = 0; m < NU; m++) tk[m] = K[j * NU + m] * r[m];
                pi[j] = at(TINY_ARR_Q, i, j, NX) + a - vec_sum(tk);
            }
#pragma unroll
            for (int j = 0; j < NU; j++) at(TINY_ARR_D, i, j, NU) = dn[j];
#pragma unroll
            for (int j = 0; j < NX; j++) { at(TINY_ARR_P, i, j, NX) = pi[j]; pn[j] = pi[j]; }
        }
    }
}
} // namespace

namespace tinympc64
{
#if defined(TINY_F64PS_UNIT)
hipError_t launch_f64_thread_ps(int nx, int nu, const Params64 &P, const Settings64 &S)
{
#define TINY_F64_PS_LAUNCH(NX, NU)                                                                                  \
    if (nx == NX && nu == NU)                                                                                       \
    {                                                                                                               \
        hipLaunchKernelGGL((admm_f64_kernel<NX, NU, Settings64>), dim3(P.bpad / WAVE64), dim3(WAVE64), 0, 0, P, S); \
        return hipGetLastError();                                                                                   \
    }
    TINY_FOR_EACH_F64DIMS(TINY_F64_PS_LAUNCH)
    return hipErrorInvalidValue;
}
#elif defined(TINY_F64PM_UNIT)
hipError_t launch_f64_thread_pm(int nx, int nu, const Params64 &P, const Models64 &M)
{
#define TINY_F64_PM_LAUNCH(NX, NU)                                                                                  \
    if (nx == NX && nu == NU)                                                                                       \
    {                                                                                                               \
        hipLaunchKernelGGL((admm_f64_kernel<NX, NU, Models64>), dim3(P.bpad / WAVE64), dim3(WAVE64), 0, 0, P, M);   \
        return hipGetLastError();                                                                                   \
    }
    TINY_FOR_EACH_F64DIMS(TINY_F64_PM_LAUNCH)
    return hipErrorInvalidValue;
}
#else
hipError_t launch_f64_thread(int nx, int nu, const Params64 &P)
{
#define TINY_F64_LAUNCH(NX, NU)                                                                        \
    if (nx == NX && nu == NU)                                                                          \
    {                                                                                                  \
        hipLaunchKernelGGL((admm_f64_kernel<NX, NU>), dim3(P.bpad / WAVE64), dim3(WAVE64), 0, 0, P);   \
        return hipGetLastError();                                                                      \
    }
    TINY_FOR_EACH_F64DIMS(TINY_F64_LAUNCH)
    return hipErrorInvalidValue;
}

hipError_t launch_f64_step(int fn, int nx, int nu, const Params64 &P, int *conv)
{
#define TINY_F64_STEP_FN(NX, NU, FN)                                                                                      \
    case FN:                                                                                                              \
        hipLaunchKernelGGL((admm_f64_step_kernel<NX, NU, FN>), dim3(P.bpad / WAVE64), dim3(WAVE64), 0, 0, P, conv);       \
        return hipGetLastError();
#define TINY_F64_STEP_LAUNCH(NX, NU)                             \
    if (nx == NX && nu == NU) switch (fn)                        \
        {                                                        \
            TINY_F64_STEP_FN(NX, NU, F64_FORWARD_PASS)           \
            TINY_F64_STEP_FN(NX, NU, F64_UPDATE_SLACK)           \
            TINY_F64_STEP_FN(NX, NU, F64_UPDATE_DUAL)            \
            TINY_F64_STEP_FN(NX, NU, F64_UPDATE_LINEAR_COST)     \
            TINY_F64_STEP_FN(NX, NU, F64_TERMINATION_CONDITION)  \
            TINY_F64_STEP_FN(NX, NU, F64_BACKWARD_PASS_GRAD)     \
        }
    TINY_FOR_EACH_F64DIMS(TINY_F64_STEP_LAUNCH)
    return hipErrorInvalidValue;
}
#endif // TINY_F64PM_UNIT
} // namespace tinympc64
