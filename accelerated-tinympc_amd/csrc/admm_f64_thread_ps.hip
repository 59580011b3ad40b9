// admm_f64_thread_ps.hip — per-instance settings of the fp64 library (tiny_batch64_set_instance_settings) on the thread-per-instance kernels: the
// instantiations of admm_f64_kernel that read every thread's own record (the SET blocks of admm_f64_thread.hip) with their launcher, and the ps forms of
// the two step functions that read a setting, update_slack and termination_condition.
#define TINY_F64PS_UNIT 1
#include "admm_f64_thread.hip"

namespace
{
// update_slack (admm.cpp:45-61) under the instance's two bound flags, termination_condition (admm.cpp:91-109) under its check_termination and its two
// tolerances: statement for statement the two branches of admm_f64_step_kernel, which keeps its name and its arguments (a trailing argument there would
// rename every step kernel of admm_f64_thread.hip).  The other four step functions read no setting and have no ps form.
template <int NX, int NU, int FN>
__global__ __launch_bounds__(WAVE64) void admm_f64_step_ps_kernel(const Params64 P, int *__restrict__ conv_out, const Settings64 ST)
{
    static_assert(FN == F64_UPDATE_SLACK || FN == F64_TERMINATION_CONDITION, "the other four step functions read no setting");
    const int b = blockIdx.x * WAVE64 + threadIdx.x;
    if (b >= P.batch) return;
    const InstSettings64 my = ST.rec[b];
    const int N = P.N;
    const size_t bp = (size_t)P.bpad;
    const double rho = P.rho;
    auto at = [&](int id, int step, int row, int dim) -> double & { return P.arr[id][((size_t)step * dim + row) * bp + b]; };
    auto in = [&](const double *base, int stride, int step, int row, int dim) {
        return base[((size_t)step * dim + row) * (size_t)stride + (stride > 1 ? b : 0)];
    };
    if constexpr (FN == F64_UPDATE_SLACK)
    {
        for (int i = 0; i < N - 1; i++)
#pragma unroll
            for (int j = 0; j < NU; j++)
            {
                double zn = at(TINY_ARR_U, i, j, NU) + at(TINY_ARR_Y, i, j, NU);
                if (my.en_input_bound)
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
                if (my.en_state_bound)
                {
                    const double lo = in(P.xmin, P.xb_stride, i, j, NX), hi = in(P.xmax, P.xb_stride, i, j, NX);
                    vn = (lo < vn) ? vn : lo;
                    vn = (vn < hi) ? vn : hi;
                }
                at(TINY_ARR_VNEW, i, j, NX) = vn;
            }
    }
    else
    {
        bool conv = false;
        if (P.iter[b] % my.check_termination == 0)
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
            conv = (r_ps < my.abs_pri_tol) && (r_pi < my.abs_pri_tol) && (r_ds < my.abs_dua_tol) && (r_di < my.abs_dua_tol);
        }
        conv_out[b] = conv ? 1 : 0;
    }
}
} // namespace

namespace tinympc64
{
hipError_t launch_f64_step_ps(int fn, int nx, int nu, const Params64 &P, int *conv, const Settings64 &S)
{
#define TINY_F64_STEP_PS_FN(NX, NU, FN)                                                                                                \
    case FN:                                                                                                                           \
        hipLaunchKernelGGL((admm_f64_step_ps_kernel<NX, NU, FN>), dim3(P.bpad / WAVE64), dim3(WAVE64), 0, 0, P, conv, S);              \
        return hipGetLastError();
#define TINY_F64_STEP_PS_LAUNCH(NX, NU)                             \
    if (nx == NX && nu == NU) switch (fn)                           \
        {                                                           \
            TINY_F64_STEP_PS_FN(NX, NU, F64_UPDATE_SLACK)           \
            TINY_F64_STEP_PS_FN(NX, NU, F64_TERMINATION_CONDITION)  \
        }
    TINY_FOR_EACH_F64DIMS(TINY_F64_STEP_PS_LAUNCH)
    return hipErrorInvalidValue;
}
} // namespace tinympc64
