// batch64_helpers.hip — the helper kernels of the fp64 library: they move arrays between the host's layout and the workspace's, and gather a
// window reference.  The host file (tinympc_batch64.hip) reaches them through the typed launchers of f64_internal.h.
#include "f64_internal.h"

namespace
{
using namespace tinympc64;

// host layout [cnt][steps][dim] (cnt = 1: shared, stored once with stride 1)  <->  device [steps][dim][stride]
__global__ void pack64_kernel(const double *__restrict__ src, double *__restrict__ dst, int nb, int steps, int dim, int stride, int step0, int nsteps)
{
    const long long total = (long long)nb * nsteps * dim;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int b = (int)(e % nb);
        const long long t = e / nb;
        const int row = (int)(t % dim), s = (int)(t / dim);
        dst[((long long)(step0 + s) * dim + row) * stride + (stride > 1 ? b : 0)] = src[((long long)b * steps + step0 + s) * dim + row];
    }
}
__global__ void unpack64_kernel(const double *__restrict__ src, double *__restrict__ dst, int nb, int steps, int dim, int stride)
{
    const long long total = (long long)nb * steps * dim;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int b = (int)(e % nb);
        const long long t = e / nb;
        const int row = (int)(t % dim), s = (int)(t / dim);
        dst[((long long)b * steps + s) * dim + row] = src[((long long)s * dim + row) * stride + b];
    }
}
// a window reference as the per-instance array the one-solve kernels read: row i of instance b is table[min(start[b] + i, rows - 1)]
__global__ void gather_window64_kernel(const double *__restrict__ table, const int *__restrict__ start, double *__restrict__ dst, int rows, int N, int nx,
                                       int batch, int bpad)
{
    const long long total = (long long)batch * N * nx;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int b = (int)(e % batch);
        const long long t = e / batch;
        const int row = (int)(t % nx), i = (int)(t / nx);
        const int tr = start[b] + i < rows - 1 ? start[b] + i : rows - 1;
        dst[((long long)i * nx + row) * bpad + b] = table[(long long)tr * nx + row];
    }
}

int grid64(long long total)
{
    long long g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
} // namespace

namespace tinympc64
{
// (256 threads per block, null stream)
hipError_t launch_pack64(const double *src, double *dst, int nb, int steps, int dim, int stride, int step0, int nsteps)
{
    hipLaunchKernelGGL(pack64_kernel, dim3(grid64((long long)nb * nsteps * dim)), dim3(256), 0, 0, src, dst, nb, steps, dim, stride, step0, nsteps);
    return hipGetLastError();
}
hipError_t launch_unpack64(const double *src, double *dst, int nb, int steps, int dim, int stride)
{
    hipLaunchKernelGGL(unpack64_kernel, dim3(grid64((long long)nb * steps * dim)), dim3(256), 0, 0, src, dst, nb, steps, dim, stride);
    return hipGetLastError();
}
hipError_t launch_gather_window64(const double *table, const int *start, double *dst, int rows, int N, int nx, int batch, int bpad)
{
    hipLaunchKernelGGL(gather_window64_kernel, dim3(grid64((long long)batch * N * nx)), dim3(256), 0, 0, table, start, dst, rows, N, nx, batch, bpad);
    return hipGetLastError();
}
} // namespace tinympc64
