// batch_helpers.hip — the helper kernels of the fp32 library: guard zones, layout conversion, the duals' width, the plant step of the closed
// loops, per-instance model records and the per-instance ROW tables.  The host file (tinympc_batch.hip) reaches them through the typed launchers of
// batch_helpers.h; the solve kernels live in units of their own (admm_*.hip).
#include "batch_helpers.h"
#include "eigen_orders.h"

namespace
{
using namespace tinympc;

__global__ void guard_fill_kernel(unsigned *p, size_t nwords)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nwords; e += (size_t)gridDim.x * blockDim.x) p[e] = kGuardWord;
}
__global__ void guard_count_kernel(const unsigned *p, size_t nwords, unsigned long long *bad)
{
    unsigned long long n = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nwords; e += (size_t)gridDim.x * blockDim.x) n += p[e] != kGuardWord;
    if (n) atomicAdd(bad, n);
}

__device__ __forceinline__ long long idx_tile(const Geo g, int fam, int b, int step, int row)
{
    const int tile = b / TILE, c = b % TILE, lane = (row & 3) * 16 + c, ch = row >> 2;
    const int steps = fam ? g.N - 1 : g.N, NC = fam ? g.NUC : g.NXC;
    return (((long long)tile * steps + step) * WAVE + lane) * NC + ch;
}
__device__ __forceinline__ long long idx_row(const Geo g, int fam, int b, int step, int row)
{
    return ((long long)b * g.N + step) * g.rw + (fam ? g.nx + row : row);
}
__device__ __forceinline__ long long idx_of(int layout, const Geo g, int fam, int b, int step, int row)
{
    return layout == LAYOUT_ROW ? idx_row(g, fam, b, step, row) : idx_tile(g, fam, b, step, row);
}

// element access of a device-layout array: fp32, or IEEE binary16 when the handle stores fp16 (ROW layout only)
__device__ __forceinline__ void put_elem(float *dst, long long i, float v, int h16)
{
    if (h16) reinterpret_cast<_Float16 *>(dst)[i] = (_Float16)v; // round to nearest even
    else dst[i] = v;
}
__device__ __forceinline__ float get_elem(const float *src, long long i, int h16)
{
    return h16 ? (float)reinterpret_cast<const _Float16 *>(src)[i] : src[i];
}

// host-layout src [cnt][nsteps][dim] (cnt = 1: shared by all instances)  ->  device layout, steps [step0, step0+nsteps)
// of instances [0, nb).  Rows/instances beyond the source are left untouched (they were zeroed at allocation).
// `mirror` (may be NULL): a plain copy of src, element for element — set_x0_device fills x.col(0) and the [B][nx] state buffer of the closed loop in
// ONE launch (round 4: it was a device-to-device copy plus this kernel)
__global__ void pack_kernel(const float *__restrict__ src, float *__restrict__ dst, int layout, Geo g, int fam, int nb,
                            int shared, int step0, int nsteps, int h16, float *__restrict__ mirror = nullptr)
{
    const int dim = fam ? g.nu : g.nx;
    const long long total = (long long)nb * nsteps * dim;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int row = (int)(e % dim);
        const long long t = e / dim;
        const int s = (int)(t % nsteps), b = (int)(t / nsteps);
        const float val = src[((long long)(shared ? 0 : b) * nsteps + s) * dim + row];
        put_elem(dst, idx_of(layout, g, fam, b, step0 + s, row), val, h16);
        if (mirror) mirror[e] = val;
    }
}

__global__ void unpack_kernel(const float *__restrict__ src, float *__restrict__ dst, int layout, Geo g, int fam, int nb,
                              int step0, int nsteps, int h16)
{
    const int dim = fam ? g.nu : g.nx;
    const long long total = (long long)nb * nsteps * dim;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int row = (int)(e % dim);
        const long long t = e / dim;
        const int s = (int)(t % nsteps), b = (int)(t / nsteps);
        dst[e] = get_elem(src, idx_of(layout, g, fam, b, step0 + s, row), h16);
    }
}

// zero steps [step0, step0+nsteps) of one member of a device array
__global__ void zero_kernel(float *__restrict__ dst, int layout, Geo g, int fam, int nb, int step0, int nsteps, int h16)
{
    const int dim = fam ? g.nu : g.nx;
    const long long total = (long long)nb * nsteps * dim;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int row = (int)(e % dim);
        const long long t = e / dim;
        put_elem(dst, idx_of(layout, g, fam, (int)(t / nsteps), step0 + (int)(t % nsteps), row), 0.f, h16);
    }
}

// the duals pair g | y between fp32 and binary16 (tiny_batch_set_storage(tb, 16) is a preference: the width follows the kernel a call resolves to)
__global__ void dual_width_kernel(const float *__restrict__ src, float *__restrict__ dst, long long n, int to32)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
    {
        if (to32) dst[e] = (float)reinterpret_cast<const _Float16 *>(src)[e];
        else reinterpret_cast<_Float16 *>(dst)[e] = (_Float16)src[e]; // round to nearest even, like every store of the 16-bit mode
    }
}

// x0 <- Adyn*x0 + Bdyn*u.col(0)   (quadrotor_hovering.cpp:110-111), and x.col(0) <- x0 (:95).
// One thread per instance; matrices column-major in global memory (tiny, cache resident).
// Summation order = Eigen's for that expression (pinned bit for bit against that expression compiled from the reference, tests/test_oracle.py:
// test_plant_step_bit_exact_vs_compiled_reference): dst = Adyn*x0, then dst += Bdyn*u0; a product whose rows and depth are both >= 8 takes the column-major
// GEMV kernel (row accumulator starting at +0, products added in ascending column order), a smaller one the lazy product in the order of its
// row count (eigen_orders.h: sequential for nx % 4 == 0, the halving tree for nx = 2, 3, the packet tree for nx = 1)
__device__ __forceinline__ void plant_step_one(int b, float *__restrict__ x0buf, float *__restrict__ xarr, const float *__restrict__ uarr,
                                               const float *__restrict__ A, const float *__restrict__ Bm, int *__restrict__ wstart,
                                               int window_advance, int layout, Geo g, int h16, const float *__restrict__ w = nullptr,
                                               float *__restrict__ x_traj = nullptr)
{
    const int nx = g.nx, nu = g.nu;
    const float *x0 = x0buf + (long long)b * nx;
    const bool gemv_a = nx >= 8, gemv_b = nx >= 8 && nu >= 8;
    float xn[64], u0[64], t[64];
    for (int m = 0; m < nu; m++) u0[m] = get_elem(uarr, idx_of(layout, g, 1, b, 0, m), h16);
    for (int i = 0; i < nx; i++)
    {
        float acc, acc2;
        if (gemv_a)
        {
            acc = 0.f + A[i] * x0[0];
            for (int k = 1; k < nx; k++) acc += A[k * nx + i] * x0[k];
        }
        else acc = gen_row_dot(A, nx, nx, i, x0, t);
        if (gemv_b)
        {
            acc2 = 0.f + Bm[i] * u0[0];
            for (int m = 1; m < nu; m++) acc2 += Bm[m * nx + i] * u0[m];
        }
        else acc2 = gen_row_dot(Bm, nx, nu, i, u0, t);
        xn[i] = acc + acc2;
        if (w) xn[i] = xn[i] + w[(long long)b * nx + i]; // the disturbance: one separately rounded add behind the product
    }
    for (int i = 0; i < nx; i++)
    {
        x0buf[(long long)b * nx + i] = xn[i];
        if (x_traj) x_traj[(long long)b * nx + i] = xn[i];
        put_elem(xarr, idx_of(layout, g, 0, b, 0, i), xn[i], h16);
    }
    if (wstart && window_advance) wstart[b] += window_advance;
}

__global__ void plant_step_kernel(float *__restrict__ x0buf, float *__restrict__ xarr, const float *__restrict__ uarr,
                                  const float *__restrict__ A, const float *__restrict__ Bm, int *__restrict__ wstart,
                                  int window_advance, int batch, int layout, Geo g, int h16)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    plant_step_one(b, x0buf, xarr, uarr, A, Bm, wstart, window_advance, layout, g, h16);
}

// ... with per-instance models: the instance's own Adyn / Bdyn from its record (Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q, pm_gen_floats apart)
__global__ void plant_step_pm_kernel(float *__restrict__ x0buf, float *__restrict__ xarr, const float *__restrict__ uarr,
                                     const float *__restrict__ recs, int *__restrict__ wstart, int window_advance, int batch, int layout, Geo g, int h16)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int nx = g.nx, nu = g.nu;
    const float *r = recs + (size_t)b * pm_gen_floats(nx, nu) + nu * nx + nx * nx + nu * nu + nx * nx;
    plant_step_one(b, x0buf, xarr, uarr, r, r + nx * nx, wstart, window_advance, layout, g, h16);
}

// ... of a simulated closed loop (tiny_batch_set_plant, tiny_batch_mpc_step_sim_async): A / Bm are the plant's matrices (one pair, or one per instance
// a_stride / b_stride floats apart), the model record's where recs is set, else the shared model's; w and x_traj are this step's [batch][nx] rows or NULL
__global__ void plant_step_sim_kernel(float *__restrict__ x0buf, float *__restrict__ xarr, const float *__restrict__ uarr, const float *__restrict__ A,
                                      const float *__restrict__ Bm, unsigned a_stride, unsigned b_stride, const float *__restrict__ recs,
                                      const float *__restrict__ w, float *__restrict__ x_traj, int *__restrict__ wstart, int window_advance, int batch,
                                      int layout, Geo g, int h16)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const int nx = g.nx, nu = g.nu;
    if (recs)
    {
        A = recs + (size_t)b * pm_gen_floats(nx, nu) + nu * nx + nx * nx + nu * nu + nx * nx;
        Bm = A + nx * nx;
    }
    else
    {
        A += (size_t)b * a_stride;
        Bm += (size_t)b * b_stride;
    }
    plant_step_one(b, x0buf, xarr, uarr, A, Bm, wstart, window_advance, layout, g, h16, w, x_traj);
}

// Per-instance models (tiny_batch_set_models_device): the caller's eight [B] arrays into one record per instance in the run-time-dimension kernel's
// order Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q (plain copies), rho into its own array
__global__ void models_gather_kernel(const float *__restrict__ rho, const float *__restrict__ K, const float *__restrict__ Pf, const float *__restrict__ Qi,
                                     const float *__restrict__ Am, const float *__restrict__ A, const float *__restrict__ Bm, const float *__restrict__ Q,
                                     float *__restrict__ dst, float *__restrict__ dst_rho, int batch, int nx, int nu)
{
    const int G = pm_gen_floats(nx, nu);
    const long long total = (long long)batch * G;
    const int sz[7] = {nu * nx, nx * nx, nu * nu, nx * nx, nx * nx, nx * nu, nx};
    const float *src[7] = {K, Pf, Qi, Am, A, Bm, Q};
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const long long b = e / G;
        int o = (int)(e % G), k = 0;
        while (o >= sz[k]) o -= sz[k++];
        dst[e] = src[k][b * sz[k] + o];
        if (o == 0 && k == 0) dst_rho[b] = rho[b];
    }
}

// ... and from those records the gain rows of the 16-lane kernel, element for element what pack_gains writes for one shared model (rows 0 .. 3nx + 2nu:
// M1, M2, M3, M45, Q, PT; the optional-term rows are not instantiated with per-instance models).  fast = 1: the fma form (u rows of M1 and x rows of M45
// hold -K; the exact form holds +K and the kernel negates the sum)
__global__ void models_pack_row_kernel(const float *__restrict__ recs, float *__restrict__ dst, int batch, int nx, int nu, int fast)
{
    const int G = pm_gen_floats(nx, nu), R = pm_row_floats(nx, nu);
    const long long total = (long long)batch * R;
    const float sg = fast ? -1.f : 1.f;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const long long b = e / R;
        const int o = (int)(e % R), reg = o / 16, r = o % 16;
        const float *K = recs + b * G, *Pf = K + nu * nx, *Qi = Pf + nx * nx, *Am = Qi + nu * nu, *A = Am + nx * nx, *Bm = A + nx * nx, *Q = Bm + nx * nu;
        const bool isx = r < nx, isu = r >= nx && r < nx + nu;
        const int mr = r - nx;
        float v = 0.f;
        if (reg < nx) v = isx ? A[reg * nx + r] : (isu ? sg * K[reg * nu + mr] : 0.f); // M1: A(r,k) | K(m,k) (exact), -K(m,k) (fast)
        else if (reg < nx + nu) v = isx ? Bm[(reg - nx) * nx + r] : 0.f;                // M2: B(r,m)
        else if (reg < 2 * nx + nu)
        {
            const int k = reg - nx - nu;                                                // M3: AmBKt(r,k) | B(k,m)
            v = isx ? Am[k * nx + r] : (isu ? Bm[mr * nx + k] : 0.f);
        }
        else if (reg < 2 * nx + 2 * nu)
        {
            const int mm = reg - 2 * nx - nu;                                           // M45: K(m,r) (exact), -K(m,r) (fast) | Quu_inv(mr,m)
            v = isx ? sg * K[r * nu + mm] : (isu ? Qi[mm * nu + mr] : 0.f);
        }
        else if (reg == 2 * nx + 2 * nu) v = isx ? Q[r] : 0.f;                          // Q(r)
        else v = isx ? Pf[r * nx + (reg - 2 * nx - 2 * nu - 1)] : 0.f;                  // PT[k]: Pinf(k,r)
        dst[e] = v;
    }
}

// tiny_batch_set_systems: fp64 systems and their Riccati caches into the fp32 arrays of tiny_batch_set_models_device, with the conventions of
// problems.with_cache(): rho, Kinf ..., Adyn, Bdyn cast, Q = (float)(Q + rho) formed in fp64
__global__ void systems_to_models_kernel(const double *__restrict__ rho, const double *__restrict__ K, const double *__restrict__ Pf, const double *__restrict__ Qi,
                                         const double *__restrict__ Am, const double *__restrict__ A, const double *__restrict__ Bm, const double *__restrict__ Q,
                                         float *__restrict__ dst, int batch, int nx, int nu)
{
    // dst: rho [B] | Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q, each [B][...]
    const int sz[8] = {1, nu * nx, nx * nx, nu * nu, nx * nx, nx * nx, nx * nu, nx};
    const double *src[8] = {rho, K, Pf, Qi, Am, A, Bm, Q};
    const long long total = (long long)batch * (1 + pm_gen_floats(nx, nu));
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        long long o = e;
        int k = 0;
        while (o >= (long long)batch * sz[k]) o -= (long long)batch * sz[k++];
        double v = src[k][o];
        if (k == 7) v = v + rho[o / nx];
        dst[e] = (float)v;
    }
}

// per-instance bounds table of the ROW layout: dst[b][step][r] = {min(lo, hi), hi}, +-inf where a bound is disabled or the
// row carries nothing.  Sources are the canonical inputs ([B or 1][steps][dim], NULL = not set = 0).
__global__ void bounds_table_kernel(const float *__restrict__ xmin, const float *__restrict__ xmax, const float *__restrict__ umin,
                                    const float *__restrict__ umax, int sh_x, int sh_u, float *__restrict__ dst, Geo g, int nb,
                                    int en_state, int en_input, int h16, int *__restrict__ zero_ties)
{
    const long long total = (long long)nb * g.N * g.rw;
    const float inf = __builtin_inff();
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int r = (int)(e % g.rw);
        const long long t = e / g.rw;
        const int i = (int)(t % g.N), b = (int)(t / g.N);
        float lo = -inf, hi = inf;
        if (r < g.nx && en_state)
        {
            const long long o = ((long long)(sh_x ? 0 : b) * g.N + i) * g.nx + r;
            lo = xmin ? xmin[o] : 0.f; hi = xmax ? xmax[o] : 0.f;
        }
        else if (r >= g.nx && r < g.nx + g.nu && i < g.N - 1 && en_input)
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

// Tile images of the ROW tables for the LDS-DMA rings of admm_tile16_pi.hip: dst[tile][step][piece][lane = 16 g + c] (float4) = words 4 (P g + piece) .. + 3 of
// row `step` of instance 16 tile + c, P = pieces per lane (1: the 16-float reference rows, 2: the 32-float {lo, hi} rows) — byte for byte what a ring slot
// holds, so that one DMA reads 1 KB of consecutive memory.  Columns past the batch repeat its last instance (they are computed and never stored).
__global__ void tile16_image_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst, int nb, int N, int pieces, long long inst_stride_f4)
{
    const long long total = (long long)((nb + 15) / 16) * N * pieces * 64;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int lane = (int)(e & 63), piece = (int)((e >> 6) % pieces);
        const long long t = e / (64 * pieces);
        const int step = (int)(t % N), g = lane >> 4, c = lane & 15;
        long long inst = (t / N) * 16 + c;
        inst = inst < nb ? inst : nb - 1;
        dst[e] = src[inst * inst_stride_f4 + (long long)step * 4 * pieces + pieces * g + piece];
    }
}

// Do the per-instance ROW tables change along the horizon?  vary[0]: the {lo, hi} table [nb][N][16] (x rows over all N steps, u rows over the
// N - 1 steps that have an input), vary[1]: the reference [nb][N][16].  Bit patterns are compared.  admm_tile16_pi.hip keeps a table that does
// not as ONE resident row per instance instead of streaming N of them through its ring every iteration (RowParams::pi_flags).
__global__ void rows_vary_kernel(const float2 *__restrict__ bounds, const float *__restrict__ xref, int nb, int N, int nx, int nu, int *__restrict__ vary)
{
    const long long total = (long long)nb * 16;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x)
    {
        const int r = (int)(e & 15);
        const long long b = e >> 4;
        if (bounds && r < nx + nu)
        {
            const int steps = r < nx ? N : N - 1;
            const unsigned long long *p = reinterpret_cast<const unsigned long long *>(bounds) + (b * N) * 16 + r;
            bool differ = false;
            for (int i = 1; i < steps; i++) differ |= p[(size_t)i * 16] != p[0];
            if (differ) vary[0] = 1;
        }
        if (xref && r < nx)
        {
            const unsigned *p = reinterpret_cast<const unsigned *>(xref) + (b * N) * 16 + r;
            bool differ = false;
            for (int i = 1; i < N; i++) differ |= p[(size_t)i * 16] != p[0];
            if (differ) vary[1] = 1;
        }
    }
}

int grid_for(long long total, int block = 256)
{
    long long gsz = (total + block - 1) / block;
    if (gsz > 8192) gsz = 8192;
    if (gsz < 1) gsz = 1;
    return (int)gsz;
}

} // namespace

namespace tinympc
{

hipError_t launch_guard_fill(unsigned *p, size_t nwords, hipStream_t stream)
{
    hipLaunchKernelGGL(guard_fill_kernel, dim3(1), dim3(256), 0, stream, p, nwords);
    return hipGetLastError();
}
hipError_t launch_guard_count(const unsigned *p, size_t nwords, unsigned long long *bad, hipStream_t stream)
{
    hipLaunchKernelGGL(guard_count_kernel, dim3(1), dim3(256), 0, stream, p, nwords, bad);
    return hipGetLastError();
}

hipError_t launch_pack(const float *src, float *dst, int layout, const Geo &g, int fam, int nb, int shared, int step0, int nsteps, int h16, float *mirror,
                       hipStream_t stream)
{
    const long long total = (long long)nb * nsteps * (fam ? g.nu : g.nx);
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for(total)), dim3(256), 0, stream, src, dst, layout, g, fam, nb, shared, step0, nsteps, h16, mirror);
    return hipGetLastError();
}
hipError_t launch_unpack(const float *src, float *dst, int layout, const Geo &g, int fam, int nb, int step0, int nsteps, int h16, hipStream_t stream)
{
    const long long total = (long long)nb * nsteps * (fam ? g.nu : g.nx);
    hipLaunchKernelGGL(unpack_kernel, dim3(grid_for(total)), dim3(256), 0, stream, src, dst, layout, g, fam, nb, step0, nsteps, h16);
    return hipGetLastError();
}
hipError_t launch_zero(float *dst, int layout, const Geo &g, int fam, int nb, int step0, int nsteps, int h16, hipStream_t stream)
{
    const long long total = (long long)nb * nsteps * (fam ? g.nu : g.nx);
    hipLaunchKernelGGL(zero_kernel, dim3(grid_for(total)), dim3(256), 0, stream, dst, layout, g, fam, nb, step0, nsteps, h16);
    return hipGetLastError();
}
hipError_t launch_dual_width(const float *src, float *dst, long long n, int to32, hipStream_t stream)
{
    hipLaunchKernelGGL(dual_width_kernel, dim3(grid_for(n)), dim3(256), 0, stream, src, dst, n, to32);
    return hipGetLastError();
}

hipError_t launch_plant_step(const PlantStepArgs &a, hipStream_t stream)
{
    const dim3 grid((a.batch + 127) / 128), block(128);
    if (a.plant || a.w || a.x_traj)
        hipLaunchKernelGGL(plant_step_sim_kernel, grid, block, 0, stream, a.x0buf, a.xarr, a.uarr, a.A, a.Bm, a.a_stride, a.b_stride, a.recs, a.w, a.x_traj,
                           a.wstart, a.window_advance, a.batch, a.layout, a.g, a.h16);
    else if (a.recs)
        hipLaunchKernelGGL(plant_step_pm_kernel, grid, block, 0, stream, a.x0buf, a.xarr, a.uarr, a.recs, a.wstart, a.window_advance, a.batch, a.layout, a.g,
                           a.h16);
    else
        hipLaunchKernelGGL(plant_step_kernel, grid, block, 0, stream, a.x0buf, a.xarr, a.uarr, a.A, a.Bm, a.wstart, a.window_advance, a.batch, a.layout, a.g,
                           a.h16);
    return hipGetLastError();
}

hipError_t launch_models_gather(const float *rho, const float *K, const float *Pf, const float *Qi, const float *Am, const float *A, const float *Bm,
                                const float *Q, float *dst, float *dst_rho, int batch, int nx, int nu, hipStream_t stream)
{
    const long long total = (long long)batch * pm_gen_floats(nx, nu);
    hipLaunchKernelGGL(models_gather_kernel, dim3(grid_for(total)), dim3(256), 0, stream, rho, K, Pf, Qi, Am, A, Bm, Q, dst, dst_rho, batch, nx, nu);
    return hipGetLastError();
}
hipError_t launch_models_pack_row(const float *recs, float *dst, int batch, int nx, int nu, int fast, hipStream_t stream)
{
    const long long total = (long long)batch * pm_row_floats(nx, nu);
    hipLaunchKernelGGL(models_pack_row_kernel, dim3(grid_for(total)), dim3(256), 0, stream, recs, dst, batch, nx, nu, fast);
    return hipGetLastError();
}
hipError_t launch_systems_to_models(const double *rho, const double *K, const double *Pf, const double *Qi, const double *Am, const double *A,
                                    const double *Bm, const double *Q, float *dst, int batch, int nx, int nu, hipStream_t stream)
{
    const long long total = (long long)batch * (1 + pm_gen_floats(nx, nu));
    hipLaunchKernelGGL(systems_to_models_kernel, dim3(grid_for(total)), dim3(256), 0, stream, rho, K, Pf, Qi, Am, A, Bm, Q, dst, batch, nx, nu);
    return hipGetLastError();
}

hipError_t launch_bounds_table(const float *xmin, const float *xmax, const float *umin, const float *umax, int sh_x, int sh_u, float *dst, const Geo &g,
                               int nb, int en_state, int en_input, int h16, int *zero_ties, hipStream_t stream)
{
    const long long total = (long long)nb * g.N * g.rw;
    hipLaunchKernelGGL(bounds_table_kernel, dim3(grid_for(total)), dim3(256), 0, stream, xmin, xmax, umin, umax, sh_x, sh_u, dst, g, nb, en_state, en_input,
                       h16, zero_ties);
    return hipGetLastError();
}
hipError_t launch_tile16_image(const float4 *src, float4 *dst, int nb, int N, int pieces, long long inst_stride_f4, hipStream_t stream)
{
    const long long total = (long long)((nb + 15) / 16) * N * pieces * 64;
    hipLaunchKernelGGL(tile16_image_kernel, dim3(grid_for(total)), dim3(256), 0, stream, src, dst, nb, N, pieces, inst_stride_f4);
    return hipGetLastError();
}
hipError_t launch_rows_vary(const float2 *bounds, const float *xref, int nb, int N, int nx, int nu, int *vary, hipStream_t stream)
{
    hipLaunchKernelGGL(rows_vary_kernel, dim3(grid_for((long long)nb * 16)), dim3(256), 0, stream, bounds, xref, nb, N, nx, nu, vary);
    return hipGetLastError();
}

} // namespace tinympc
