// admm_steps.hip — batched twins of the six step functions the reference exports next to tiny_solve()
// (src/tinympc/admm.hpp:10-18): forward_pass, update_slack, update_dual, update_linear_cost, termination_condition,
// backward_pass_grad.  Each is one launch over the row layout (one DPP row of 16 lanes = one instance, any horizon N,
// nx + nu <= 16) that reads and writes the device-resident workspace exactly as the reference function reads and writes
// TinyWorkspace.  They share the arithmetic of the fused solver (rowlane_math.h), so in exact mode each function is
// bit-identical to the reference's.  The fused kernels do not call these; they exist for callers that drive the
// algorithm step by step (e.g. only roll out a trajectory with forward_pass).
#include "rowlane_math.h"

namespace tinympc
{

// gain rows of the optional terms (pack_gains): R on the u rows, then coeff_d2p(r, m) on the x rows
template <int NX, int NU>
__device__ __forceinline__ float input_cost_row(const float *mats, int r16) { return mats[(3 * NX + 2 * NU + 1) * 16 + r16]; }
template <int NX, int NU>
__device__ __forceinline__ void load_d2p(float (&CD)[NU], const float *mats, int r16)
{
#pragma unroll
    for (int m = 0; m < NU; m++) CD[m] = mats[(3 * NX + 2 * NU + 2 + m) * 16 + r16];
}

// c term of a step (what lin_cost() subtracts rho*(snew - dual) from): x rows -(Xref .* Q) (admm.cpp:81); u rows -0, so that
// r = -rho*(znew - y) keeps the sign of a zero difference, or -(Uref .* R) when the optional input reference is on
template <bool H16>
__device__ __forceinline__ float cost_of(const RowParams &P, bool is_x, bool is_u, float xr, float qrow, float rrow, int uoff)
{
    if (is_x) return rnd<H16>(-(xr * qrow));
    if (P.uref != nullptr && is_u) return rnd<H16>(-(ldw<H16>(P.uref, uoff) * rrow));
    return -0.f;
}

// Both kernels of this file are compiled twice: here, with one set of settings for the launch (the settings view `my` of the frame is P), and as
// admm_steps_ps.hip (TINY_STEPS_PS_UNIT) with per-instance settings: the kernels take a SettingsParams beside P, are named ..._ps_kernel, and `my` is the
// row's own record SP.rec[inst], loaded once at entry.  The text of the bodies is one, so the two forms cannot drift apart; a kernel body behind a function
// call instead moved this unit's code.
#ifdef TINY_STEPS_PS_UNIT
#define TINY_STEP_KERNEL admm_step_ps_kernel
#define TINY_ROWSTREAM_KERNEL admm_rowstream_ps_kernel
#define TINY_SETTINGS_ARG , const SettingsParams SP
#define TINY_SETTINGS_VIEW const InstSettings my = SP.rec[valid ? inst : P.batch - 1]
constexpr bool kPerInstanceSettings = true;
#else
#define TINY_STEP_KERNEL admm_step_kernel
#define TINY_ROWSTREAM_KERNEL admm_rowstream_kernel
#define TINY_SETTINGS_ARG
#define TINY_SETTINGS_VIEW const RowParams &my = P
constexpr bool kPerInstanceSettings = false;
#endif

template <int NX, int NU, bool EXACT, bool H16>
__global__ __launch_bounds__(WAVE) void TINY_STEP_KERNEL(const RowParams P TINY_SETTINGS_ARG, const int fn, int *__restrict__ conv_out)
{
    const int lane = threadIdx.x, r16 = lane & 15;
    const int inst = blockIdx.x * 4 + (lane >> 4);
    const bool valid = inst < P.batch;
    TINY_SETTINGS_VIEW;
    const bool is_x = r16 < NX, is_u = (r16 >= NX) && (r16 < NX + NU);
    const int N = P.N;
    const int rowbase = (inst * N) * 16 + r16;
    const float rho = P.rho;

    if (fn == STEP_FORWARD_PASS) // admm.cpp:27-37  reads x.col(0), d; writes u, x.col(1..N-1)
    {
        RowGains<NX, NU> G;
        G.load(P.mats, r16);
        float s = ldw<H16>(P.xu, rowbase);
        for (int i = 0; i < N - 1; i++)
        {
            float sv, xn;
            lqr_step<NX, NU, EXACT, H16>(G, is_x, is_u, s, ldw<H16>(P.pd, rowbase + i * 16), sv, xn);
            if (valid) stw<H16>(P.xu, rowbase + i * 16, sv);
            s = xn;
        }
        if (valid) stw<H16>(P.xu, rowbase + (N - 1) * 16, is_x ? s : 0.f);
    }
    else if (fn == STEP_UPDATE_SLACK) // admm.cpp:45-61  znew = clip(u + y), vnew = clip(x + g)
    {
        for (int i = 0; i < N; i++)
        {
            const float2 lh = ld_bounds<H16>(P.bounds, inst * (int)P.bounds_inst_stride + i * 16 + r16);
            const float t = ldw<H16>(P.xu, rowbase + i * 16) + ldw<H16>(P.gy, rowbase + i * 16);
            if (valid) stw<H16>(P.vzn, rowbase + i * 16, box_project<EXACT>(t, lh.x, lh.y));
        }
    }
    else if (fn == STEP_UPDATE_DUAL) // admm.cpp:67-71  y += u - znew, g += x - vnew
    {
        for (int i = 0; i < N; i++)
        {
            const float a = ldw<H16>(P.gy, rowbase + i * 16);
            if (valid) stw<H16>(P.gy, rowbase + i * 16, (a + ldw<H16>(P.xu, rowbase + i * 16)) - ldw<H16>(P.vzn, rowbase + i * 16));
        }
    }
    else if (fn == STEP_UPDATE_LINEAR_COST) // admm.cpp:77-85  r, q, p.col(N-1)
    {
        const float qrow = P.mats[(2 * NX + 2 * NU) * 16 + r16], rrow = input_cost_row<NX, NU>(P.mats, r16);
        const RowXref<H16> xref(P, inst, valid, inst, r16);
        const int uref_off = inst * (int)P.uref_inst_stride + r16;
        float xr = 0.f, t1 = 0.f;
        for (int i = 0; i < N; i++)
        {
            xr = xref.at(P, i, r16);
            const float cq = cost_of<H16>(P, is_x, is_u, xr, qrow, rrow, uref_off + i * 16);
            t1 = ldw<H16>(P.vzn, rowbase + i * 16) - ldw<H16>(P.gy, rowbase + i * 16);
            const float lin = lin_cost<EXACT, H16>(cq, rho, t1);
            if (valid) stw<H16>(P.qr, rowbase + i * 16, (i < N - 1 || is_x) ? lin : 0.f);
        }
        const float pterm = terminal_term<NX, NU, EXACT, H16>(P.mats, r16, xr); // xr, t1 are those of step N-1 here
        if (valid && is_x) stw<H16>(P.pd, rowbase + (N - 1) * 16, lin_cost<EXACT, H16>(pterm, rho, t1));
    }
    else if (fn == STEP_TERMINATION_CONDITION) // admm.cpp:91-109  residual fields + the boolean it returns
    {
        bool conv = false;
        const int itn = valid ? P.iter[inst] : 1;
        if (itn % my.check_termination == 0) // row-uniform
        {
            float pri = 0.f, dua = 0.f;
            for (int i = 0; i < N; i++)
            {
                const float sv = ldw<H16>(P.xu, rowbase + i * 16), t = ldw<H16>(P.vzn, rowbase + i * 16);
                pri = fmaxf(pri, fabsf(sv - t));
                dua = fmaxf(dua, fabsf(ldw<H16>(P.vz, rowbase + i * 16) - t));
            }
            RowResiduals res;
            res.measure(pri, dua, is_x, is_u, rho);
            conv = res.below_tol(my);
            if (valid && r16 == 0) res.store(P, inst);
        }
        if (valid && r16 == 0)
        {
            conv_out[inst] = conv ? 1 : 0;
            if (!conv) atomicAdd(P.n_unsolved, 1);
        }
    }
    else if (fn == STEP_BACKWARD_PASS_GRAD) // admm.cpp:15-22  reads p.col(N-1), q, r; writes d, p.col(0..N-2)
    {
        RowGains<NX, NU> G;
        G.load(P.mats, r16);
        float CD[NU];
        load_d2p<NX, NU>(CD, P.mats, r16);
        float p = ldw<H16>(P.pd, rowbase + (N - 1) * 16);
        for (int i = N - 2; i >= 0; i--)
        {
            float pn, dd;
            riccati_step<NX, NU, EXACT, H16>(G, is_x, p, ldw<H16>(P.qr, rowbase + i * 16), pn, dd);
            if (P.en_d2p) pn = d2p_term<NX, NU, EXACT, H16>(CD, pn, dd);
            if (valid) stw<H16>(P.pd, rowbase + i * 16, is_u ? dd : pn);
            p = pn;
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// admm_rowstream_kernel — the fused solve (tiny_solve, admm.cpp:111-152) in the row mapping for ANY horizon N: same
// arithmetic and same per-instance early exit as admm_rowlane_kernel, but the loop-carried state lives in the workspace
// arrays (streamed through L2/HBM every iteration) instead of registers, so nothing is unrolled over N.  It is the
// fallback for (nx, nu) classes whose N has no register-resident instantiation, and keeps exact mode bit-identical
// to the reference there too.
// ---------------------------------------------------------------------------------------------------------------------
// Per-instance settings (see above): the loop bound P.max_iter is then the batch's largest budget, wave-uniform, and a row whose own budget is used up
// leaves `active` behind its last backward sweep, as a converged row does behind its check (see admm_rowlane.hip)
template <int NX, int NU, bool EXACT, bool H16>
__global__ __launch_bounds__(WAVE) void TINY_ROWSTREAM_KERNEL(const RowParams P TINY_SETTINGS_ARG)
{
    const int lane = threadIdx.x, r16 = lane & 15;
    const int inst = blockIdx.x * 4 + (lane >> 4);
    const bool valid = inst < P.batch;
    TINY_SETTINGS_VIEW;
    const bool is_x = r16 < NX, is_u = (r16 >= NX) && (r16 < NX + NU);
    const int N = P.N;
    const int rowbase = (inst * N) * 16 + r16;
    const float rho = P.rho;
    RowGains<NX, NU> G;
    G.load(P.mats, r16);
    const float qrow = P.mats[(2 * NX + 2 * NU) * 16 + r16], rrow = input_cost_row<NX, NU>(P.mats, r16);
    float CD[NU];
    load_d2p<NX, NU>(CD, P.mats, r16);
    const RowXref<H16> xref(P, inst, valid, inst, r16);
    const int uref_off = inst * (int)P.uref_inst_stride + r16;
    const float x0 = ldw<H16>(P.xu, rowbase);
    const float pterm = terminal_term<NX, NU, EXACT, H16>(P.mats, r16, xref.at(P, N - 1, r16));
    SolveFrame F(P, inst, valid);
    bool active = valid && (my.max_iter > 0);
    for (int it = 0; it < P.max_iter; ++it)
    {
        if (!__any(active)) break;
        const bool last_iter = (it == my.max_iter - 1); // the iteration whose x, u an instance that uses up its budget keeps
        const bool zero_state = (it == 0) && (P.cold_start != 0);
        const bool zero_duals = (it == 0) && ((P.cold_start | P.duals_zero) != 0);
        if (active)
        {
            float s = x0, pri = 0.f, dua = 0.f, t1 = 0.f;
            for (int i = 0; i < N; i++)
            {
                const int o = rowbase + i * 16;
                float sv, xn = 0.f;
                if (i < N - 1) lqr_step<NX, NU, EXACT, H16>(G, is_x, is_u, s, zero_state ? 0.f : ldw<H16>(P.pd, o), sv, xn);
                else sv = is_x ? s : 0.f;
                const float2 lh = ld_bounds<H16>(P.bounds, inst * (int)P.bounds_inst_stride + i * 16 + r16);
                const float a = zero_duals ? 0.f : ldw<H16>(P.gy, o);
                const float bprev = zero_state ? 0.f : ldw<H16>(P.vz, o);
                const float t = box_project<EXACT>(rnd<H16>(sv + a), lh.x, lh.y);
                const float an = rnd<H16>((a + sv) - t);
                pri = fmaxf(pri, fabsf(sv - t));
                dua = fmaxf(dua, fabsf(bprev - t));
                stw<H16>(P.vzn, o, t);
                stw<H16>(P.gy, o, an);
                if (last_iter) stw<H16>(P.xu, o, sv);
                t1 = t - an;
                s = xn;
            }
            const float pN = lin_cost<EXACT, H16>(pterm, rho, t1);
            stw<H16>(P.pd, rowbase + (N - 1) * 16, is_x ? pN : 0.f);
            if (F.check(my, it, pri, dua, is_x, is_u, rho)) active = false;
            else
            {
                float p = pN;
                stw<H16>(P.vz, rowbase + (N - 1) * 16, ldw<H16>(P.vzn, rowbase + (N - 1) * 16));
                for (int i = N - 2; i >= 0; i--)
                {
                    const int o = rowbase + i * 16;
                    const float sni = ldw<H16>(P.vzn, o);
                    const float cq = cost_of<H16>(P, is_x, is_u, xref.at(P, i, r16), qrow, rrow, uref_off + i * 16);
                    float pn, dd;
                    riccati_step<NX, NU, EXACT, H16>(G, is_x, p, lin_cost<EXACT, H16>(cq, rho, sni - ldw<H16>(P.gy, o)), pn, dd);
                    if (P.en_d2p) pn = d2p_term<NX, NU, EXACT, H16>(CD, pn, dd);
                    stw<H16>(P.pd, o, is_u ? dd : pn);
                    stw<H16>(P.vz, o, sni);
                    p = pn;
                }
                if constexpr (kPerInstanceSettings) active = !last_iter; // this row's budget is used up; its neighbours in the wave may go on
            }
        }
    }
    if (F.no_iterations(my, P, inst, valid && r16 == 0)) return; // (per-instance settings: this row only)
    {
        // live-out: q, r (admm.cpp:80-82) and, for converged instances, x,u regenerated from the frozen d
        const bool solved = F.solved();
        // reset_workspace() folded into this launch (cold start): an instance that converged in its FIRST iteration ran no
        // backward sweep, which is what writes [p;d] and [v;z] — they are the zeros of the reset, materialised here
        const bool fresh = valid && (P.cold_start != 0) && solved && F.itn == 1;
        float s = x0;
        for (int i = 0; i < N; i++)
        {
            const int o = rowbase + i * 16;
            float sv, xn = 0.f;
            if (i < N - 1) lqr_step<NX, NU, EXACT, H16>(G, is_x, is_u, s, fresh ? 0.f : ldw<H16>(P.pd, o), sv, xn);
            else sv = is_x ? s : 0.f;
            if (fresh)
            {
                if (i < N - 1) stw<H16>(P.pd, o, 0.f);
                stw<H16>(P.vz, o, 0.f);
            }
            if (valid && solved) stw<H16>(P.xu, o, sv);
            s = xn;
            const float cq = cost_of<H16>(P, is_x, is_u, xref.at(P, i, r16), qrow, rrow, uref_off + i * 16);
            const float lin = lin_cost<EXACT, H16>(cq, rho, ldw<H16>(P.vzn, o) - ldw<H16>(P.gy, o));
            if (valid) stw<H16>(P.qr, o, (i < N - 1 || is_x) ? lin : 0.f);
        }
        if (valid && r16 == 0) F.store(P, inst);
    }
}

#ifdef TINY_STEPS_PS_UNIT
hipError_t launch_admm_rowstream_ps(int nx, int nu, bool exact, bool h16, const RowParams &P, const SettingsParams &SP, hipStream_t stream)
{
    const int nblocks = (P.batch + 3) / 4;
    if (!SP.rec) return hipErrorInvalidValue;
#define TINY_ROWSTREAM_PS_LAUNCH(NX, NU, EX, H) \
    hipLaunchKernelGGL((admm_rowstream_ps_kernel<NX, NU, EX, H>), dim3(nblocks), dim3(WAVE), 0, stream, P, SP)
#define TINY_ROWSTREAM_PS_DISPATCH(NX, NU)                                \
    if (nx == NX && nu == NU)                                             \
    {                                                                     \
        TINY_FOR_EXACT_H16(exact, h16, TINY_ROWSTREAM_PS_LAUNCH, NX, NU); \
        return hipGetLastError();                                         \
    }
    TINY_FOR_EACH_ROWDIMS(TINY_ROWSTREAM_PS_DISPATCH)
    return hipErrorInvalidValue;
}

// termination_condition is the one step function that reads a setting the table of bounds does not carry
hipError_t launch_admm_termination_ps(int nx, int nu, bool exact, bool h16, const RowParams &P, const SettingsParams &SP, int *conv_out, hipStream_t stream)
{
    const int nblocks = (P.batch + 3) / 4;
    if (!SP.rec) return hipErrorInvalidValue;
#define TINY_STEP_PS_LAUNCH(NX, NU, EX, H) \
    hipLaunchKernelGGL((admm_step_ps_kernel<NX, NU, EX, H>), dim3(nblocks), dim3(WAVE), 0, stream, P, SP, (int)STEP_TERMINATION_CONDITION, conv_out)
#define TINY_STEP_PS_DISPATCH(NX, NU)                               \
    if (nx == NX && nu == NU)                                       \
    {                                                               \
        TINY_FOR_EXACT_H16(exact, h16, TINY_STEP_PS_LAUNCH, NX, NU); \
        return hipGetLastError();                                   \
    }
    TINY_FOR_EACH_ROWDIMS(TINY_STEP_PS_DISPATCH)
    return hipErrorInvalidValue;
}
#else
hipError_t launch_admm_rowstream(int nx, int nu, bool exact, bool h16, const RowParams &P, hipStream_t stream)
{
    const int nblocks = (P.batch + 3) / 4;
#define TINY_ROWSTREAM_LAUNCH(NX, NU, EX, H) \
    hipLaunchKernelGGL((admm_rowstream_kernel<NX, NU, EX, H>), dim3(nblocks), dim3(WAVE), 0, stream, P)
#define TINY_ROWSTREAM_DISPATCH(NX, NU)                                  \
    if (nx == NX && nu == NU)                                            \
    {                                                                    \
        TINY_FOR_EXACT_H16(exact, h16, TINY_ROWSTREAM_LAUNCH, NX, NU);   \
        return hipGetLastError();                                        \
    }
    TINY_FOR_EACH_ROWDIMS(TINY_ROWSTREAM_DISPATCH)
    return hipErrorInvalidValue;
}

bool rowdims_supported(int nx, int nu)
{
#define TINY_ROWDIMS_CHECK(NX, NU) \
    if (nx == NX && nu == NU) return true;
    TINY_FOR_EACH_ROWDIMS(TINY_ROWDIMS_CHECK)
    return false;
}

hipError_t launch_admm_step(int nx, int nu, bool exact, bool h16, int fn, const RowParams &P, int *conv_out, hipStream_t stream)
{
    const int nblocks = (P.batch + 3) / 4;
#define TINY_STEP_LAUNCH(NX, NU, EX, H) \
    hipLaunchKernelGGL((admm_step_kernel<NX, NU, EX, H>), dim3(nblocks), dim3(WAVE), 0, stream, P, fn, conv_out)
#define TINY_ROWDIMS_DISPATCH(NX, NU)                               \
    if (nx == NX && nu == NU)                                       \
    {                                                               \
        TINY_FOR_EXACT_H16(exact, h16, TINY_STEP_LAUNCH, NX, NU);   \
        return hipGetLastError();                                   \
    }
    TINY_FOR_EACH_ROWDIMS(TINY_ROWDIMS_DISPATCH)
    return hipErrorInvalidValue;
}

#endif // TINY_STEPS_PS_UNIT

} // namespace tinympc
