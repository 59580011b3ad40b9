// settings_helpers.hip — the helper kernel of the per-instance settings (tiny_batch_set_instance_settings): the ROW layout's per-instance bounds table
// with the two bound flags read PER INSTANCE.  A unit of its own beside batch_helpers.hip, whose kernels keep their code; the launcher is declared in
// batch_helpers.h with theirs.
#include "batch_helpers.h"

namespace tinympc
{

// bounds_table_kernel (batch_helpers.hip) with en_state[b] / en_input[b] in place of its two scalars: {lo, hi} of instance b, step i, row r into
// dst[b][N][rw], +-inf where that instance's flag is off or the row carries nothing, lo := min(lo, hi); *zero_ties as there
__global__ void bounds_table_ps_kernel(const float *__restrict__ xmin, const float *__restrict__ xmax, const float *__restrict__ umin,
                                       const float *__restrict__ umax, int sh_x, int sh_u, float *__restrict__ dst, Geo g, int nb,
                                       const int *__restrict__ en_state, const int *__restrict__ en_input, int h16, int *__restrict__ zero_ties)
{
    const long long total = (long long)nb * g.N * g.rw;
    const float inf = __builtin_inff();
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int r = (int)(e % g.rw);
        const long long t = e / g.rw;
        const int i = (int)(t % g.N), b = (int)(t / g.N);
        float lo = -inf, hi = inf;
        if (r < g.nx && en_state[b])
        {
            const long long o = ((long long)(sh_x ? 0 : b) * g.N + i) * g.nx + r;
            lo = xmin ? xmin[o] : 0.f; hi = xmax ? xmax[o] : 0.f;
        }
        else if (r >= g.nx && r < g.nx + g.nu && i < g.N - 1 && en_input[b])
        {
            const long long o = ((long long)(sh_u ? 0 : b) * (g.N - 1) + i) * g.nu + (r - g.nx);
            lo = umin ? umin[o] : 0.f; hi = umax ? umax[o] : 0.f;
        }
        lo = lo < hi ? lo : hi;
        if (h16)
        {
            reinterpret_cast<_Float16 *>(dst)[2 * e] = (_Float16)lo;
            reinterpret_cast<_Float16 *>(dst)[2 * e + 1] = (_Float16)hi;
            lo = (float)(_Float16)lo; hi = (float)(_Float16)hi;
        }
        else { dst[2 * e] = lo; dst[2 * e + 1] = hi; }
        if (zero_tie_bound(lo, hi)) *zero_ties = 1; // (every writer stores the same word)
    }
}

hipError_t launch_bounds_table_ps(const float *xmin, const float *xmax, const float *umin, const float *umax, int sh_x, int sh_u, float *dst, const Geo &g,
                                  int nb, const int *en_state, const int *en_input, int h16, int *zero_ties, hipStream_t stream)
{
    const long long total = (long long)nb * g.N * g.rw;
    const long long blocks = (total + 255) / 256;
    hipLaunchKernelGGL(bounds_table_ps_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks))), dim3(256), 0, stream, xmin, xmax, umin, umax,
                       sh_x, sh_u, dst, g, nb, en_state, en_input, h16, zero_ties);
    return hipGetLastError();
}

} // namespace tinympc
