// admm_f64_plant.hip — the plant step of the fp64 library's closed loops (quadrotor_hovering.cpp:110-111), one thread per instance, in the three
// forms the host enqueues: of one MPC step, of a multi-step run, and against a separate plant.  The step itself is plant64_step (f64_math.h).
#include "f64_math.h"

namespace
{
using namespace tinympc64;

template <int NX, int NU>
__global__ void plant64_kernel(double *__restrict__ X, const double *__restrict__ U, const double *__restrict__ mats, int batch, int bpad)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double u[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = U[(size_t)j * bpad + b];
    plant64_step<NX, NU>(X, u, mats, b, bpad);
}
// The plant step of a multi-step run (tiny_batch64_mpc_run): the same step; it also records u.col(0) in this MPC step's row of the
// trajectory ([B][nu], may be NULL) and slides the instance's reference window (start may be NULL).
template <int NX, int NU>
__global__ void plant64_run_kernel(double *__restrict__ X, const double *__restrict__ U, const double *__restrict__ mats, int batch, int bpad,
                                   double *__restrict__ u0_row, int *__restrict__ start, int window_advance)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double u[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = U[(size_t)j * bpad + b];
    if (u0_row)
    {
#pragma unroll
        for (int j = 0; j < NU; j++) u0_row[(size_t)b * NU + j] = u[j];
    }
    plant64_step<NX, NU>(X, u, mats, b, bpad);
    if (start) start[b] += window_advance;
}

// plant64_run_kernel against a separate plant: x.col(0) <- (A_p * x.col(0) + B_p * u.col(0)) + w in plant64_step's order, then one separately
// rounded add (none without w).  The matrices are the plant's (one pair, or instance b's at + b * stride) or the model's; it records u.col(0) and
// x.col(0) in this step's rows of the trajectories and slides the window, each where asked to.
template <int NX, int NU>
__global__ void plant64_sim_kernel(const PlantSim64 a)
{
    static_assert(!(NX >= 8 && NU >= 8), "Bdyn*u would take the GEMV kernel too");
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const double *const A = a.A + (size_t)b * a.stride_a, *const Bm = a.B + (size_t)b * a.stride_b;
    double u[NU], x[NX], xn[NX];
#pragma unroll
    for (int j = 0; j < NU; j++) u[j] = a.U[(size_t)j * a.bpad + b];
    if (a.u0_row)
    {
#pragma unroll
        for (int j = 0; j < NU; j++) a.u0_row[(size_t)b * NU + j] = u[j];
    }
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = a.X[(size_t)j * a.bpad + b];
#pragma unroll
    for (int i = 0; i < NX; i++)
    {
        double ax;
        if constexpr (NX >= 8)
        {
            double c = 0.0;
#pragma unroll
            for (int j = 0; j < NX; j++) c = A[j * NX + i] * x[j] + c;
            ax = c * 1.0 + 0.0;
        }
        else ax = row_dot<NX, NX>(A, i, x);
        xn[i] = ax + row_dot<NX, NU>(Bm, i, u);
        if (a.w) xn[i] = xn[i] + a.w[(size_t)b * NX + i];
    }
#pragma unroll
    for (int i = 0; i < NX; i++)
    {
        a.X[(size_t)i * a.bpad + b] = xn[i];
        if (a.x_traj) a.x_traj[(size_t)b * NX + i] = xn[i];
    }
    if (a.start) a.start[b] += a.window_advance;
}
} // namespace

namespace tinympc64
{
// (128 threads per block, null stream)
hipError_t launch_plant64(int nx, int nu, double *X, const double *U, const double *mats, int batch, int bpad)
{
#define TINY_F64_PLANT(NX, NU)                                                                                               \
    if (nx == NX && nu == NU)                                                                                                \
    {                                                                                                                        \
        hipLaunchKernelGGL((plant64_kernel<NX, NU>), dim3((batch + 127) / 128), dim3(128), 0, 0, X, U, mats, batch, bpad);   \
        return hipGetLastError();                                                                                            \
    }
    TINY_FOR_EACH_F64DIMS(TINY_F64_PLANT)
    return hipErrorInvalidValue;
}

hipError_t launch_plant64_run(int nx, int nu, double *X, const double *U, const double *mats, int batch, int bpad, double *u0_row, int *start, int window_advance)
{
#define TINY_F64_PLANT_RUN(NX, NU)                                                                                                                \
    if (nx == NX && nu == NU)                                                                                                                     \
    {                                                                                                                                             \
        hipLaunchKernelGGL((plant64_run_kernel<NX, NU>), dim3((batch + 127) / 128), dim3(128), 0, 0, X, U, mats, batch, bpad, u0_row, start,      \
                           window_advance);                                                                                                       \
        return hipGetLastError();                                                                                                                 \
    }
    TINY_FOR_EACH_F64DIMS(TINY_F64_PLANT_RUN)
    return hipErrorInvalidValue;
}

hipError_t launch_plant64_sim(int nx, int nu, const PlantSim64 &a)
{
#define TINY_F64_PLANT_SIM(NX, NU)                                                                           \
    if (nx == NX && nu == NU)                                                                                \
    {                                                                                                        \
        hipLaunchKernelGGL((plant64_sim_kernel<NX, NU>), dim3((a.batch + 127) / 128), dim3(128), 0, 0, a);   \
        return hipGetLastError();                                                                            \
    }
    TINY_FOR_EACH_F64DIMS(TINY_F64_PLANT_SIM)
    return hipErrorInvalidValue;
}
} // namespace tinympc64
