// batch_helpers.h — what the host file of the fp32 library (tinympc_batch.hip) and the unit of its helper kernels (batch_helpers.hip) share: the
// geometry of the two device layouts, the guard-zone constants, and one typed launcher per helper kernel.  Every launcher enqueues on the stream
// it is given, computes its own grid and answers hipGetLastError().  No solve kernel unit includes this header.
#pragma once
#include "tinympc_internal.h"

namespace tinympc
{

enum { LAYOUT_TILE = 0, LAYOUT_ROW = 1 };

// Debug guard zones (tiny_batch_debug_guards): floats on each side of an allocation, and the word they are filled with
constexpr size_t kGuard = 256;               // (1 KB: keeps the 256-byte alignment of hipMalloc)
constexpr unsigned kGuardWord = 0x7fc0dea1u; // a quiet NaN

// ---------------------------------------------------------------------------------------------
// Element addressing of the two device layouts.  `fam` 0 = state-type (nx rows, N steps),
// 1 = input-type (nu rows, N-1 steps).
//   TILE (admm_stream.hip):  x-family [ntiles][N][64][NXC], u-family [ntiles][N-1][64][NUC]
//   ROW  (row / wave kernels): pair array [batch_pad4][N][rw], rows [0,nx) state member, [nx,nx+nu) input member;
//        rw = 16 (one DPP row per instance) or 64 (one wavefront per instance, admm_wave.hip)
// ---------------------------------------------------------------------------------------------
struct Geo
{
    int nx, nu, N, NXC, NUC;
    int rw; // lanes per instance-step of the ROW layout: 16 (one DPP row) or 64 (one wavefront, 16 < nx + nu <= 64)
};

// A stored {lo, hi} on which v_med3_f32 and the reference's compare-selects can break a tie between zeros differently (tinympc_internal.h: box_project):
// lo = -0 under hi > 0 (t = +0), or hi = +0 over lo < 0 or lo = -0 (t = -0), as the table holds them — folded, rounded to the storage format.  Every other
// pair with a zero in it gives the same bits either way — the box [+0, +0] of bounds never set among them — and a disabled bound is +-inf
__host__ __device__ inline bool zero_tie_bound(float lo, float hi)
{
    const bool lo_neg0 = lo == 0.f && __builtin_signbit(lo), hi_pos0 = hi == 0.f && !__builtin_signbit(hi);
    return (lo_neg0 && hi > 0.f) || (hi_pos0 && (lo < 0.f || lo_neg0));
}

// one block of 256 threads (the guard zones are kGuard words)
hipError_t launch_guard_fill(unsigned *p, size_t nwords, hipStream_t stream);
hipError_t launch_guard_count(const unsigned *p, size_t nwords, unsigned long long *bad, hipStream_t stream);

// the copy kernels: 256-thread blocks, a grid-stride loop over the elements (at most 8192 blocks)
hipError_t launch_pack(const float *src, float *dst, int layout, const Geo &g, int fam, int nb, int shared, int step0, int nsteps, int h16, float *mirror,
                       hipStream_t stream);
hipError_t launch_unpack(const float *src, float *dst, int layout, const Geo &g, int fam, int nb, int step0, int nsteps, int h16, hipStream_t stream);
hipError_t launch_zero(float *dst, int layout, const Geo &g, int fam, int nb, int step0, int nsteps, int h16, hipStream_t stream);
hipError_t launch_dual_width(const float *src, float *dst, long long n, int to32, hipStream_t stream);
hipError_t launch_models_gather(const float *rho, const float *K, const float *Pf, const float *Qi, const float *Am, const float *A, const float *Bm,
                                const float *Q, float *dst, float *dst_rho, int batch, int nx, int nu, hipStream_t stream);
hipError_t launch_models_pack_row(const float *recs, float *dst, int batch, int nx, int nu, int fast, hipStream_t stream);
hipError_t launch_systems_to_models(const double *rho, const double *K, const double *Pf, const double *Qi, const double *Am, const double *A,
                                    const double *Bm, const double *Q, float *dst, int batch, int nx, int nu, hipStream_t stream);
hipError_t launch_bounds_table(const float *xmin, const float *xmax, const float *umin, const float *umax, int sh_x, int sh_u, float *dst, const Geo &g,
                               int nb, int en_state, int en_input, int h16, int *zero_ties, hipStream_t stream);
// the same table with the two bound flags per instance (en_state[nb], en_input[nb]: tiny_batch_set_instance_settings); settings_helpers.hip
hipError_t launch_bounds_table_ps(const float *xmin, const float *xmax, const float *umin, const float *umax, int sh_x, int sh_u, float *dst, const Geo &g,
                                  int nb, const int *en_state, const int *en_input, int h16, int *zero_ties, hipStream_t stream);
hipError_t launch_tile16_image(const float4 *src, float4 *dst, int nb, int N, int pieces, long long inst_stride_f4, hipStream_t stream);
hipError_t launch_rows_vary(const float2 *bounds, const float *xref, int nb, int N, int nx, int nu, int *vary, hipStream_t stream);

// The plant step of the closed loops, x0 <- A x0 + B u.col(0) (+ w), x.col(0) <- x0: one thread per instance, 128-thread blocks.  Three kernels, chosen
// here: plant_step_sim_kernel when a plant, w or x_traj is given, else plant_step_pm_kernel when a model record is, else plant_step_kernel.
struct PlantStepArgs
{
    float *x0buf, *xarr; // [batch][nx] current state; the work array whose x.col(0) follows it
    const float *uarr;   // the work array that holds u.col(0)
    const float *A, *Bm; // column-major: the plant's where `plant`, else the shared model's (not read where recs is set)
    bool plant;          // A / Bm are a separate plant's (tiny_batch_set_plant) ...
    unsigned a_stride, b_stride; // ... one pair per instance this many floats apart, or 0: one pair for the batch
    const float *recs;   // the per-instance model records (pm_gen_floats apart) or NULL
    const float *w;      // this step's [batch][nx] disturbance or NULL: no addition
    float *x_traj;       // this step's [batch][nx] row of the state trajectory or NULL: not recorded
    int *wstart;         // the window starts, slid by window_advance, or NULL
    int window_advance, batch, layout;
    Geo g;
    int h16;
};
hipError_t launch_plant_step(const PlantStepArgs &a, hipStream_t stream);

} // namespace tinympc
