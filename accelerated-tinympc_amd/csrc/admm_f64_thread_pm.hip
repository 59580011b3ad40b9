// admm_f64_thread_pm.hip — per-instance models of the fp64 library (tiny_batch64_set_models) on the thread-per-instance kernel: the instantiations
// of admm_f64_kernel that read every thread's own record (the PM blocks of admm_f64_thread.hip) with their launcher, and the kernel that gathers the
// caller's eight [batch] arrays into the records.
#define TINY_F64PM_UNIT 1
#include "admm_f64_thread.hip"

namespace
{
// One record per instance, Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q column-major (the layout of Params64::mats), and rho beside them.
// q_plus_rho: Q + rho is stored (tiny_batch64_set_systems: the code generator keeps Q + rho in work.Q, codegen.cpp:255).  One thread per element.
__global__ void models64_gather_kernel(const double *__restrict__ rho, const double *__restrict__ Kinf, const double *__restrict__ Pinf,
                                       const double *__restrict__ Quu_inv, const double *__restrict__ AmBKt, const double *__restrict__ Adyn,
                                       const double *__restrict__ Bdyn, const double *__restrict__ Q, double *__restrict__ rec,
                                       double *__restrict__ rho_out, int batch, int nx, int nu, int q_plus_rho)
{
    const int sz[7] = {nu * nx, nx * nx, nu * nu, nx * nx, nx * nx, nx * nu, nx};
    const double *const src[7] = {Kinf, Pinf, Quu_inv, AmBKt, Adyn, Bdyn, Q};
    const int len = 3 * nx * nx + 2 * nx * nu + nu * nu + nx;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)batch * len) return;
    const size_t b = e / len;
    int o = (int)(e % len), k = 0;
    while (o >= sz[k]) o -= sz[k++];
    double v = src[k][b * sz[k] + o];
    if (k == 6 && q_plus_rho) v = v + rho[b];
    rec[e] = v;
    if (e % len == 0) rho_out[b] = rho[b];
}
} // namespace

namespace tinympc64
{
hipError_t launch_models64_gather(const double *rho, const double *Kinf, const double *Pinf, const double *Quu_inv, const double *AmBKt, const double *Adyn,
                                  const double *Bdyn, const double *Q, double *rec, double *rho_out, int batch, int nx, int nu, int q_plus_rho)
{
    const size_t total = (size_t)batch * (3 * nx * nx + 2 * nx * nu + nu * nu + nx);
    hipLaunchKernelGGL(models64_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, rho, Kinf, Pinf, Quu_inv, AmBKt, Adyn, Bdyn, Q, rec,
                       rho_out, batch, nx, nu, q_plus_rho);
    return hipGetLastError();
}
} // namespace tinympc64
