// admm_f64_rows.hip — the sixteen-lanes-per-instance kernel of the fp64 library, admm_f64_rows_kernel, with its launchers.  Compiled six times: as
// itself (the one-solve and the MPC instantiations, launch_f64_rows), under TINY_F64SIM_UNIT as admm_f64_rowsim.hip (the SIM instantiations,
// launch_rows64_sim), under TINY_F64PM_UNIT = 1 / 2 as admm_f64_rows_pm.hip / admm_f64_rowsim_pm.hip (per-instance models: one solve,
// launch_f64_rows_pm / the closed loop, launch_rows64_loop_pm) and, under TINY_F64PS_UNIT = 1 / 2, as admm_f64_rows_ps.hip / admm_f64_rowloop_ps.hip
// (per-instance settings: one solve, launch_f64_rows_ps / the on-chip closed loop, launch_rows64_loop_ps), so that the families build side by side.
#include "f64_math.h"

namespace
{
using namespace tinympc64;

__device__ __forceinline__ Mpc64 loop_args() { return Mpc64{}; }
__device__ __forceinline__ Mpc64 loop_args(const Mpc64 &l) { return l; }
__device__ __forceinline__ Mpc64 loop_args(const Mpc64 &l, const Sim64 &) { return l; }
__device__ __forceinline__ Sim64 sim_args(const Mpc64 &, const Sim64 &s) { return s; }
template <class... T>
__device__ __forceinline__ Sim64 sim_args(const T &...) { return Sim64{}; }
// per-instance models: a Models64 as the last trailing argument, alone (one solve) or behind Mpc64 and Sim64 (the closed loop)
__device__ __forceinline__ Mpc64 loop_args(const Models64 &) { return Mpc64{}; }
__device__ __forceinline__ Mpc64 loop_args(const Mpc64 &l, const Sim64 &, const Models64 &) { return l; }
__device__ __forceinline__ Sim64 sim_args(const Mpc64 &, const Sim64 &s, const Models64 &) { return s; }
__device__ __forceinline__ Models64 models_args(const Models64 &m) { return m; }
__device__ __forceinline__ Models64 models_args(const Mpc64 &, const Sim64 &, const Models64 &m) { return m; }
template <class... T>
__device__ __forceinline__ Models64 models_args(const T &...) { return Models64{}; }
// per-instance settings: a Settings64 as the last trailing argument, alone (one solve) or behind the Mpc64 (the on-chip closed loop)
__device__ __forceinline__ Mpc64 loop_args(const Settings64 &) { return Mpc64{}; }
__device__ __forceinline__ Mpc64 loop_args(const Mpc64 &l, const Settings64 &) { return l; }
__device__ __forceinline__ Settings64 settings_args(const Settings64 &s) { return s; }
__device__ __forceinline__ Settings64 settings_args(const Mpc64 &, const Settings64 &s) { return s; }
template <class... T>
__device__ __forceinline__ Settings64 settings_args(const T &...) { return Settings64{}; }

// This lane's gain rows from its instance's record (Models64::rec), element for element what pack_row_gains lays out for the shared table: the x rows
// read row r of Adyn, AmBKt, Bdyn, column r of Kinf and Pinf and Q(r), the u rows row m of Kinf, Quu_inv and column m of Bdyn; the other lanes zeros.
template <int NX, int NU>
struct Rec64
{
    static constexpr int K = 0, PINF = NU * NX, QUU = PINF + NX * NX, AM = QUU + NU * NU, A = AM + NX * NX, B = A + NX * NX, Q = B + NX * NU;
};
template <int NX, int NU>
__device__ __forceinline__ void record_gains(const double *__restrict__ rec, bool is_x, bool is_u, int row, double (&M1)[NX], double (&M2)[NU],
                                             double (&M3)[NX], double (&M45)[NU], double &qrow)
{
    using R = Rec64<NX, NU>;
    const bool own = is_x || is_u; // (row = 0 on the lanes that own none: every address below stays inside the record)
    const int o1 = is_x ? R::A + row : R::K + row, s1 = is_x ? NX : NU;          // Adyn(r,k) | Kinf(m,k)
    const int o3 = is_x ? R::AM + row : R::B + row * NX, s3 = is_x ? NX : 1;     // AmBKt(r,k) | Bdyn(k,m)
    const int o45 = is_x ? R::K + row * NU : R::QUU + row, s45 = is_x ? 1 : NU;  // Kinf(m,r) | Quu_inv(mr,m)
#pragma unroll
    for (int k = 0; k < NX; k++)
    {
        const double a = rec[o1 + k * s1], c = rec[o3 + k * s3];
        M1[k] = own ? a : 0.0; M3[k] = own ? c : 0.0;
    }
#pragma unroll
    for (int m = 0; m < NU; m++)
    {
        const double a = rec[R::B + row + m * NX], c = rec[o45 + m * s45];       // Bdyn(r,m)
        M2[m] = is_x ? a : 0.0; M45[m] = own ? c : 0.0;
    }
    const double q = rec[R::Q + row];
    qrow = is_x ? q : 0.0;
}
template <int NX, int NU>
__device__ __forceinline__ void record_pinf_row(const double *__restrict__ rec, bool is_x, int row, double (&PT)[NX])
{
#pragma unroll
    for (int k = 0; k < NX; k++)
    {
        const double a = rec[Rec64<NX, NU>::PINF + row * NX + k]; // Pinf(k,r)
        PT[k] = is_x ? a : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// admm_f64_rows_kernel<NX,NU,N>: the 16-lanes-per-instance mapping of admm_rowlane.hip in double.  Lane r of a DPP row owns
// row r of the stacked vector [x ; u] (nx + nu <= 16), four instances per wavefront, the horizon unrolled, and the whole
// loop-carried state of the solve in registers: per step a = [g;y], c = [-(Xref.*Q) ; d], pd = [p;d] of the last backward
// sweep, b = [v;z], sn = [vnew;znew] (five doubles per lane and step; one wave per SIMD owns the 512-entry register file).
// The workspace arrays are read once before the first and written once after the last iteration — the thread-per-instance
// kernel (admm_f64_thread.hip) moves every array through HBM in every iteration (3.7 GB per iteration of 65 536 quadrotor instances).
// A state element is broadcast within its row by two v_mov_b32_dpp row_newbcast (low and high word), products and sums
// are separately rounded v_mul_f64 / v_add_f64 in the orders of f64_math.h.  Results are bitwise equal to the
// thread-per-instance kernel and to the compiled fp64 reference.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int F64_AHEAD = 4; // bounds are fetched this many steps ahead of their use

// RT = false: the horizon is the template parameter N.  RT = true ("any horizon", round 3): N is the CAPACITY of the unrolled body
// (32 or 64 steps: registers are indexed statically, so the body stays unrolled) and the horizon n = P.N <= N is a launch parameter;
// the steps past it are skipped by wave-uniform branches.  With a capacity of 64 the backward sweep's [p ; d] (live-out only) is
// written through to its arrays instead of being held in 2 x 64 registers.
//
// MPC = true: the examples' closed loop on chip.  L.mpc_steps times
// {y = g = 0; tiny_solve; x.col(0) = Adyn x.col(0) + Bdyn u.col(0); start += window_advance} with the whole workspace staying in registers / LDS
// between two solves; the plant step after the last solve is the host's (plant64_run_kernel).  Only where [p ; d] is held in registers.
//
// SIM = true (with MPC; instantiated in admm_f64_rowsim.hip): the plant step between two solves takes the plant's own rows (S.plant: one table or
// one per instance; NULL the model's), adds the disturbance row with one separately rounded add and stores the state trajectory.  The flag is the
// second trailing argument, a Sim64 behind the Mpc64.
template <int NX, int NU, int N, bool RT = false, bool MPC = false, class... LOOP>
__global__ __launch_bounds__(WAVE64, (N <= 12 ? 2 : 1)) void admm_f64_rows_kernel(const Params64 P, const double *__restrict__ gains, const LOOP... loop)
{
    // PM (the ",pm" instantiations, admm_f64_rows_pm.hip and admm_f64_rowsim_pm.hip): a Models64 as the last trailing argument.  The gain rows and rho
    // of a row are its instance's, read from the instance's record; `gains` is not read.  The closed loop with per-instance models is the SIM one
    constexpr bool PM = (false || ... || std::is_same<LOOP, Models64>::value);
    // SET (the ",ps" instantiations, admm_f64_rows_ps.hip and admm_f64_rowloop_ps.hip): a Settings64 as the last trailing argument.  The tolerances, the
    // budget, check_termination and the two bound flags of a row are its instance's, read from the instance's record; of P's settings only max_iter is
    // read, the batch's LARGEST budget: it bounds the iteration loop, which stays wave-uniform
    constexpr bool SET = (false || ... || std::is_same<LOOP, Settings64>::value);
    static_assert(!(PM && SET), "per-instance settings together with per-instance models are refused by the host");
    constexpr int NLOOP = (int)sizeof...(LOOP) - (PM ? 1 : 0) - (SET ? 1 : 0);
    constexpr bool SIM = NLOOP == 2;
    static_assert(NLOOP == (MPC ? (SIM ? 2 : 1) : 0), "the closed-loop instantiations take one further argument, an Mpc64, the simulated ones a Sim64 behind it; the one-solve kernels none");
    static_assert(!SIM || MPC, "the simulated loop is the on-chip loop's");
    static_assert(!PM || SIM == MPC, "per-instance models: one solve, or the simulated loop");
    [[maybe_unused]] const Mpc64 L = loop_args(loop...);
    [[maybe_unused]] const Sim64 S = sim_args(loop...);
    [[maybe_unused]] const Models64 MO = models_args(loop...);
    [[maybe_unused]] const Settings64 ST = settings_args(loop...);
    static_assert(!MPC || !(RT && N > 32), "the on-chip loop takes the workspace's d from the registers of [p ; d]");
    static_assert(NX + NU <= 16 && !(NX >= 8 && NU >= 8), "16-lane mapping; both dims >= 8 would take Eigen's GEMV kernel");
    static_assert(!RT || N > 20, "the runtime-horizon variant indexes the slack by the horizon: it keeps it in LDS");
    const int n = RT ? P.N : N; // the horizon
    constexpr bool PD_REG = !(RT && N > 32);
    const int lane = threadIdx.x, r16 = lane & 15;
    const int inst = blockIdx.x * 4 + (lane >> 4);
    const bool valid = inst < P.batch;
    const size_t b = valid ? inst : P.batch - 1; // loads of an out-of-range row address the last instance; it stores nothing
    const bool is_x = r16 < NX, is_u = r16 >= NX && r16 < NX + NU;
    const int row = is_x ? r16 : (is_u ? r16 - NX : 0);
    const size_t bp = (size_t)P.bpad;
    double rho_of_row;
    if constexpr (PM) rho_of_row = MO.rho[b];
    else rho_of_row = P.rho;
    const double rho = rho_of_row;
    // This row's record, read again wherever it is needed (here, and once per iteration) through a lane index the compiler cannot see through, as the
    // bounds' offset below: held instead, its eight words would be live across an iteration loop that already sits at 256 registers
    [[maybe_unused]] auto my_settings = [&]() -> InstSettings64 {
        int ia = inst;
        asm volatile("" : "+v"(ia));
        ia = valid ? ia : P.batch - 1;
        return ST.rec[ia];
    };
    [[maybe_unused]] bool budget = true; // SET: this row's max_iter > 0.  A row without one runs along inactive and writes status and iter only
    // element (step, this lane's row) of the pair [x-type array ; u-type array]; u-type arrays have N - 1 steps
    auto ld = [&](int idx, int idu, int i) -> double {
        if (is_x) return P.arr[idx][((size_t)i * NX + row) * bp + b];
        if (is_u && i < n - 1) return P.arr[idu][((size_t)i * NU + row) * bp + b];
        return 0.0;
    };
    auto st = [&](int idx, int idu, int i, double v) {
        if (!valid) return;
        if constexpr (SET) { if (!budget) return; }
        if (is_x) P.arr[idx][((size_t)i * NX + row) * bp + b] = v;
        else if (is_u && i < n - 1) P.arr[idu][((size_t)i * NU + row) * bp + b] = v;
    };
    bool en_b_of_row;
    if constexpr (SET)
    {
        const InstSettings64 my = my_settings();
        en_b_of_row = is_x ? (my.en_state_bound != 0) : (is_u && my.en_input_bound != 0);
        budget = my.max_iter > 0;
    }
    else en_b_of_row = is_x ? (P.en_state_bound != 0) : (is_u && P.en_input_bound != 0);
    const bool en_b = en_b_of_row;
    // this lane's bounds of step i sit at pl0[i * bstep], ph0[i * bstep] (u rows have N - 1 steps; the other lanes read x row 0, unused)
    const size_t bstr = is_u ? (size_t)P.ub_stride : (size_t)P.xb_stride;
    const size_t boff = (size_t)row * bstr + (bstr > 1 ? b : 0);
    const double *const pl0 = (is_u ? P.umin : P.xmin) + boff, *const ph0 = (is_u ? P.umax : P.xmax) + boff;
    const size_t bstep = (is_u ? NU : NX) * bstr;
    if (P.max_iter <= 0) // tiny_solve only sets status and iter (admm.cpp:114-117,151)
    {
        if (valid && r16 == 0)
        {
            P.status[inst] = ST_UNSOLVED; P.iter[inst] = 1;
            atomicAdd(P.n_unsolved, 1);
        }
        return;
    }
    // gains, one register per matrix column: [reg][16] doubles (pack_row_gains on the host)
    double M1[NX], M2[NU], M3[NX], M45[NU], qrow_of_row;
    if constexpr (PM) record_gains<NX, NU>(MO.rec + b * MO.stride, is_x, is_u, row, M1, M2, M3, M45, qrow_of_row);
    else
    {
#pragma unroll
        for (int k = 0; k < NX; k++) { M1[k] = gains[k * 16 + r16]; M3[k] = gains[(NX + NU + k) * 16 + r16]; }
#pragma unroll
        for (int m = 0; m < NU; m++) { M2[m] = gains[(NX + m) * 16 + r16]; M45[m] = gains[(2 * NX + NU + m) * 16 + r16]; }
        qrow_of_row = gains[(2 * NX + 2 * NU) * 16 + r16];
    }
    const double qrow = qrow_of_row;

    // ---- live-in ----
    // long horizons keep the two slack words of a step in LDS (lane-linear, 1 KB per step and wave), short ones in registers
    constexpr bool LDS_SLACK = N > 20;
    constexpr int NREG = LDS_SLACK ? 1 : N;
    __shared__ double slack_lds[LDS_SLACK ? 2 * N * WAVE64 : 1];
    // (two halves: hipcc leaves a statically indexed array of more than 32 doubles in scratch memory)
    constexpr int NLO = N < 32 ? N : 32, NHI = N > 32 ? N - 32 : 1;
    double a_lo[NLO], a_hi[NHI], c_lo[NLO], c_hi[NHI], pd[PD_REG ? N : 1], bb_r[NREG], sn_r[NREG];
#define A_(i) ((i) < 32 ? a_lo[(i) < 32 ? (i) : 0] : a_hi[(i) < 32 ? 0 : (i) - 32])
#define C_(i) ((i) < 32 ? c_lo[(i) < 32 ? (i) : 0] : c_hi[(i) < 32 ? 0 : (i) - 32])
    double *const sl = slack_lds + lane;
#define BB_GET(i) (LDS_SLACK ? sl[(2 * (i)) * WAVE64] : bb_r[LDS_SLACK ? 0 : (i)])
#define SN_GET(i) (LDS_SLACK ? sl[(2 * (i) + 1) * WAVE64] : sn_r[LDS_SLACK ? 0 : (i)])
#define BB_SET(i, v) do { if constexpr (LDS_SLACK) sl[(2 * (i)) * WAVE64] = (v); else bb_r[LDS_SLACK ? 0 : (i)] = (v); } while (0)
#define SN_SET(i, v) do { if constexpr (LDS_SLACK) sl[(2 * (i) + 1) * WAVE64] = (v); else sn_r[LDS_SLACK ? 0 : (i)] = (v); } while (0)
    double xrN = 0.0;
    // row i of a window reference: table[min(start + i, rows - 1)] (the clamp of the window gather); the table is small and stays in L2
    [[maybe_unused]] const bool window = MPC && L.table_rows > 0;
    [[maybe_unused]] int wstart = 0;
    if constexpr (MPC) wstart = window ? L.xref_start[b] : 0;
    [[maybe_unused]] auto win_at = [&](int i) -> double {
        const int tr = wstart + i < L.table_rows - 1 ? wstart + i : L.table_rows - 1;
        return is_x ? L.table[(size_t)tr * NX + row] : 0.0;
    };
#pragma unroll
    for (int i = 0; i < N; i++)
    {
        if (RT && i >= n) continue;
        double xr = 0.0;
        if (MPC && window) xr = win_at(i);
        else if (is_x) xr = P.xref[((size_t)i * NX + row) * (size_t)P.xref_stride + (P.xref_stride > 1 ? b : 0)];
        const double pdi = ld(TINY_ARR_P, TINY_ARR_D, i);
        if constexpr (PD_REG) pd[i] = pdi;
        C_(i) = is_x ? -(xr * qrow) : pdi;            // admm.cpp:81 | d_i
        A_(i) = MPC ? 0.0 : ld(TINY_ARR_G, TINY_ARR_Y, i); // (the closed loop starts every solve from y = g = 0)
        BB_SET(i, ld(TINY_ARR_V, TINY_ARR_Z, i));
        SN_SET(i, 0.0);
        if (i == n - 1) xrN = xr;
    }
    double x0 = ld(TINY_ARR_X, TINY_ARR_U, 0); // x.col(0) on the x rows
    double pterm;
    {
        double PT[NX], t[NX]; // p.col(N-1) = -(Xref.col(N-1)^T * Pinf)  (admm.cpp:83): a vectorised reduction over k
        if constexpr (PM) record_pinf_row<NX, NU>(MO.rec + b * MO.stride, is_x, row, PT);
        else
        {
#pragma unroll
            for (int k = 0; k < NX; k++) PT[k] = gains[(2 * NX + 2 * NU + 1 + k) * 16 + r16];
        }
        row_products<0, NX>(t, xrN, PT);
        pterm = -vec_sum(t);
    }
    double r_ps = 0, r_pi = 0, r_ds = 0, r_di = 0;
    {
        const size_t bi = b;
        r_ps = P.res[0 * bp + bi]; r_pi = P.res[1 * bp + bi]; r_ds = P.res[2 * bp + bi]; r_di = P.res[3 * bp + bi];
    }
    int status = ST_UNSOLVED, itn = 1; // admm.cpp:114-115
    bool active = valid;
    if constexpr (SET) active = valid && budget; // (a run on chip never meets a zero budget: the host sends it through the launch sequence)
    double pN = 0.0;

    [[maybe_unused]] int ms = 0; // the MPC step of the on-chip closed loop
next_solve: // (a label, not a loop around the solve: the one-solve instantiations have no second solve to go round for)
    for (int it = 0; it < P.max_iter; ++it)
    {
        if (!__any(active)) break;
        // No divergent region around the body: a row that has converged keeps executing with its wave and every update of its
        // state is a select on `active` (a compiler-visible `if (active)` would make hipcc keep the old and the new value of
        // all 3N state registers alive across the region: 264 spilled registers at N = 30).
        itn = active ? it + 1 : itn; // admm.cpp:120
        // the last permitted backward sweep must not overwrite d in c: x, u of an instance that exhausts max_iter come from
        // the d its last forward sweep used (regenerated below); the final d itself goes to pd
        // (SET: the row's own last iteration, so that a row whose budget ends before the wave's regenerates x, u from the right d)
        [[maybe_unused]] InstSettings64 my{};
        if constexpr (SET) my = my_settings();
        bool keep_d_of_row;
        if constexpr (SET) keep_d_of_row = (it == my.max_iter - 1);
        else keep_d_of_row = (it == P.max_iter - 1);
        const bool keep_d = keep_d_of_row;
        // ---- forward_pass + update_slack + update_dual + residual maxima (admm.cpp:27-71, 95-98) ----
        double s = x0, pri = 0.0, dua = 0.0, t1 = 0.0;
        double lo[F64_AHEAD], hi[F64_AHEAD];
        // an offset the compiler cannot see through, renewed every iteration: without it LICM hoists the 2N 64-bit bound
        // addresses out of the iteration loop and keeps them in 4N registers
        int oz;
        asm volatile("s_mov_b32 %0, 0" : "=s"(oz));
        const double *const pl = pl0 + oz, *const ph = ph0 + oz;
        auto ld_bounds = [&](int i, double &l, double &h) {
            const size_t o = (size_t)((is_u && i >= n - 1) ? 0 : i) * bstep;
            l = pl[o]; h = ph[o];
        };
#pragma unroll
        for (int k = 0; k < F64_AHEAD; k++) ld_bounds(k < n ? k : n - 1, lo[k], hi[k]);
#pragma unroll
        for (int i = 0; i < N; i++)
        {
            if (RT && i >= n) continue;
            double sv, xn = 0.0;
            if (i < n - 1)
            {
                double t[NX], t2[NU];
                row_products<0, NX>(t, s, M1);
                const double acc = is_x ? lazy_sum<NX>(t) : lazy_sum<NU>(t);   // Adyn*x | Kinf*x
                const double un = -acc - C_(i);                                   // admm.cpp:31
                row_products<NX, NU>(t2, un, M2);
                xn = acc + lazy_sum<NX>(t2);                                     // admm.cpp:35
                sv = is_u ? un : s;
            }
            else sv = is_x ? s : 0.0;
            const double lo_i = lo[i % F64_AHEAD], hi_i = hi[i % F64_AHEAD];
            if (i + F64_AHEAD < n) ld_bounds(i + F64_AHEAD, lo[i % F64_AHEAD], hi[i % F64_AHEAD]);
            const double t0 = sv + A_(i);                                         // admm.cpp:47-48
            double tc = t0;
            if (en_b && (i < n - 1 || is_x))                                     // admm.cpp:51-60: min(max, max(min, t)); u has N - 1 steps
            {
                tc = (lo_i < tc) ? tc : lo_i;
                tc = (tc < hi_i) ? tc : hi_i;
            }
            const double an = (A_(i) + sv) - tc;                                  // admm.cpp:69-70
            pri = fmax(pri, fabs(sv - tc));                                      // admm.cpp:95,97
            dua = fmax(dua, fabs(BB_GET(i) - tc));                               // admm.cpp:96,98
            A_(i) = active ? an : A_(i);
            if constexpr (LDS_SLACK) { if (active) SN_SET(i, tc); }
            else sn_r[LDS_SLACK ? 0 : i] = active ? tc : sn_r[LDS_SLACK ? 0 : i];
            t1 = tc - an;
            s = xn;
        }
        pN = active ? pterm - rho * t1 : pN; // admm.cpp:83-84
        const double pri_x = row_max(is_x ? pri : 0.0), dua_x = row_max(is_x ? dua : 0.0);
        const double pri_u = row_max(is_u ? pri : 0.0), dua_u = row_max(is_u ? dua : 0.0);
        bool conv = false;
        if constexpr (SET)
        {
            // row-uniform, no longer wave-uniform: selects, not a divergent region (as every other update of a row's state)
            const bool due = active && ((it + 1) % my.check_termination == 0);
            r_ps = due ? pri_x : r_ps; r_ds = due ? dua_x * rho : r_ds; r_pi = due ? pri_u : r_pi; r_di = due ? dua_u * rho : r_di;
            conv = due && (r_ps < my.abs_pri_tol) && (r_pi < my.abs_pri_tol) && (r_ds < my.abs_dua_tol) && (r_di < my.abs_dua_tol);
        }
        else if ((it + 1) % P.check_termination == 0) // admm.cpp:91-109 (wave-uniform condition)
        {
            r_ps = active ? pri_x : r_ps; r_ds = active ? dua_x * rho : r_ds; r_pi = active ? pri_u : r_pi; r_di = active ? dua_u * rho : r_di;
            conv = active && (r_ps < P.abs_pri_tol) && (r_pi < P.abs_pri_tol) && (r_ds < P.abs_dua_tol) && (r_di < P.abs_dua_tol);
        }
        status = conv ? ST_SOLVED : status; // admm.cpp:136: returns before the v/z copy and the backward pass
        active = active && !conv;
        if (!__any(active)) break;
        // ---- v = vnew, z = znew (admm.cpp:141-142), update_linear_cost + backward_pass_grad (admm.cpp:15-22, 80-82) ----
        double p = pN;
        if constexpr (LDS_SLACK) { if (active) BB_SET(n - 1, SN_GET(n - 1)); }
        else bb_r[LDS_SLACK ? 0 : N - 1] = active ? sn_r[LDS_SLACK ? 0 : N - 1] : bb_r[LDS_SLACK ? 0 : N - 1];
#pragma unroll
        for (int i = N - 2; i >= 0; i--)
        {
            if (RT && i > n - 2) continue;
            const double sni = SN_GET(i);
            if constexpr (LDS_SLACK) { if (active) BB_SET(i, sni); }
            else bb_r[LDS_SLACK ? 0 : i] = active ? sni : bb_r[LDS_SLACK ? 0 : i];
            const double cq = is_x ? C_(i) : -0.0; // u rows: r = -rho*(znew - y) keeps the sign of a zero difference
            const double lin = cq - rho * (sni - A_(i));
            double t[NX], tk[NU], td[NU];
            row_products<0, NX>(t, p, M3);
            // x rows: AmBKt*p (coefficient-evaluated: halving tree, or sequential when nu = 1); u rows: Bdyn^T*p (vectorised reduction)
            const double dot = is_x ? ((NU == 1 && NX % PS == 0) ? seq_sum(t) : novec_sum(t)) : vec_sum(t);
            const double wv = lin + dot;               // q + AmBKt*p | Bdyn^T*p + r
            row_products<NX, NU>(tk, lin, M45);        // Kinf^T * r
            row_products<NX, NU>(td, wv, M45);         // Quu_inv * (Bdyn^T p + r)
            const double pn = wv - vec_sum(tk);        // admm.cpp:20
            const double dd = lazy_sum<NU>(td);        // admm.cpp:19
            if constexpr (PD_REG) pd[i] = active ? (is_u ? dd : pn) : pd[i];
            else { if (active) st(TINY_ARR_P, TINY_ARR_D, i, is_u ? dd : pn); }
            C_(i) = (active && is_u && !keep_d) ? dd : C_(i);
            p = pn;
        }
        // a row whose own budget is used up leaves behind the backward sweep of its last permitted iteration; its state is frozen by the selects on `active`
        if constexpr (SET) active = active && (it + 1 < my.max_iter);
    }
    if constexpr (MPC)
    if (ms + 1 < L.mpc_steps)
    {
        // ---- advance to the next MPC step (quadrotor_tracking.cpp:101-118): nothing leaves the chip but u.col(0) ----
        double t[NX], t2[NU];
        row_products<0, NX>(t, x0, M1);
        const double acc = is_x ? lazy_sum<NX>(t) : lazy_sum<NU>(t);
        const double u0 = -acc - C_(0); // [. ; u_0] of the solve that just finished: step 0 of the forward recursion (admm.cpp:31)
        if (L.u0_traj && valid && is_u) L.u0_traj[((size_t)ms * P.batch + inst) * NU + row] = u0;
        if constexpr (SIM)
        {
            // x.col(0) = (A_p * x.col(0) + B_p * u.col(0)) + w: the products and sums below with the plant's rows, then one separately rounded add.
            // The lane offsets are remade here from `inst`, opaque to the compiler (as the gains and the bounds: it otherwise carries the 64-bit
            // lane addresses through every iteration loop); an out-of-range row reads the last instance's and stores nothing.
            int ia = inst;
            asm volatile("" : "+v"(ia));
            ia = valid ? ia : P.batch - 1;
            if (S.plant)
            {
                const double *const pl = S.plant + ((size_t)ia * S.plant_stride + r16);
                double Ar[NX], Br[NU]; // transient: this lane's row of [A_p | B_p]
#pragma unroll
                for (int k = 0; k < NX; k++) Ar[k] = pl[k * 16];
#pragma unroll
                for (int m = 0; m < NU; m++) Br[m] = pl[(NX + m) * 16];
                x0 = plant_row<NX, NU>(Ar, Br, x0, u0);
            }
            else x0 = plant_row<NX, NU>(M1, M2, x0, u0);
            const size_t xo = ((size_t)ms * P.batch + ia) * NX + (is_x ? r16 : 0);
            if (S.w && is_x) x0 = x0 + S.w[xo];
            if (S.x_traj && valid && is_x) S.x_traj[xo] = x0;
        }
        else
        {
            // x.col(0) = Adyn * x.col(0) + Bdyn * u.col(0) in plant64_kernel's order: rows and depth >= 8 is the GEMV accumulator from +0
            double ax;
            if constexpr (NX >= 8)
            {
                double c = 0.0;
#pragma unroll
                for (int j = 0; j < NX; j++) c = t[j] + c;
                ax = c * 1.0 + 0.0;
            }
            else ax = lazy_sum<NX>(t);
            row_products<NX, NU>(t2, u0, M2);
            x0 = ax + lazy_sum<NX>(t2); // (x rows; the other lanes' value is never read as a state)
        }
        if (window) wstart += L.window_advance;
        // the gains through an offset the compiler cannot see through (as the bounds above): otherwise it keeps Q and the NX registers of
        // Pinf's row from live-in alive through every solve instead of loading them again here
        int ozg;
        asm volatile("s_mov_b32 %0, 0" : "=s"(ozg));
        const double *const gains_again = gains + ozg;
        // (per-instance models: the record's lane address is remade from `inst` the same way, as the plant rows' above)
        [[maybe_unused]] const double *rec_again = nullptr;
        double qrow_again;
        if constexpr (PM)
        {
            int ig = inst;
            asm volatile("" : "+v"(ig));
            ig = valid ? ig : P.batch - 1;
            rec_again = MO.rec + (size_t)ig * MO.stride;
            const double q = rec_again[Rec64<NX, NU>::Q + row];
            qrow_again = is_x ? q : 0.0;
        }
        else qrow_again = gains_again[(2 * NX + 2 * NU) * 16 + r16];
#pragma unroll
        for (int i = 0; i < N; i++)
        {
            if (RT && i >= n) continue;
            double cx = C_(i);
            if (window)
            {
                const double xr = win_at(i);
                cx = -(xr * qrow_again);
                if (i == n - 1) xrN = xr;
            }
            C_(i) = is_x ? cx : pd[i]; // d of the workspace is that of the last executed backward sweep (keep_d)
            A_(i) = 0.0;               // y = g = 0 (quadrotor_hovering.cpp:100-101)
            __builtin_amdgcn_sched_barrier(0); // one table row in flight at a time: hoisted together the N loads cost 2N registers
        }
        if (window) // admm.cpp:83 for the window's new last row, as at live-in
        {
            double PT[NX], tp[NX];
            if constexpr (PM) record_pinf_row<NX, NU>(rec_again, is_x, row, PT);
            else
            {
#pragma unroll
                for (int k = 0; k < NX; k++) PT[k] = gains_again[(2 * NX + 2 * NU + 1 + k) * 16 + r16];
            }
            row_products<0, NX>(tp, xrN, PT);
            pterm = -vec_sum(tp);
        }
        status = ST_UNSOLVED; itn = 1; active = valid; // the residual fields carry over: they are live-in of the next tiny_solve
        ++ms;
        goto next_solve;
    }
    // ---- live-out: every work array once ----
    {
        const bool solved = status == ST_SOLVED;
        double s = x0;
#pragma unroll
        for (int i = 0; i < N; i++)
        {
            if (RT && i >= n) continue;
            double sv, xn = 0.0;
            if (i < n - 1) // x, u regenerated from the d of the last executed forward sweep by the same instruction sequence
            {
                double t[NX], t2[NU];
                row_products<0, NX>(t, s, M1);
                const double acc = is_x ? lazy_sum<NX>(t) : lazy_sum<NU>(t);
                const double un = -acc - C_(i);
                row_products<NX, NU>(t2, un, M2);
                xn = acc + lazy_sum<NX>(t2);
                sv = is_u ? un : s;
            }
            else sv = is_x ? s : 0.0;
            s = xn;
            st(TINY_ARR_X, TINY_ARR_U, i, sv);
            const double sni = SN_GET(i);
            st(TINY_ARR_Q, TINY_ARR_R, i, (is_x ? C_(i) : -0.0) - rho * (sni - A_(i)));
            if constexpr (PD_REG) st(TINY_ARR_P, TINY_ARR_D, i, i == n - 1 ? pN : pd[i]);
            else { if (i == n - 1) st(TINY_ARR_P, TINY_ARR_D, i, pN); }
            st(TINY_ARR_V, TINY_ARR_Z, i, BB_GET(i));
            st(TINY_ARR_VNEW, TINY_ARR_ZNEW, i, sni);
            st(TINY_ARR_G, TINY_ARR_Y, i, A_(i));
        }
        if (valid && r16 == 0)
        {
            if (!SET || budget)
            {
                P.res[0 * bp + inst] = r_ps; P.res[1 * bp + inst] = r_pi; P.res[2 * bp + inst] = r_ds; P.res[3 * bp + inst] = r_di;
            }
            P.status[inst] = status;
            P.iter[inst] = itn;
            if (!solved) atomicAdd(P.n_unsolved, 1);
            if constexpr (MPC)
                if (window) L.xref_start[inst] = wstart;
        }
    }
#undef A_
#undef C_
#undef BB_GET
#undef SN_GET
#undef BB_SET
#undef SN_SET
}
} // namespace

namespace tinympc64
{
#if defined(TINY_F64PM_UNIT) && TINY_F64PM_UNIT == 1
// per-instance models, one solve: an instantiation wherever launch_f64_rows has one
hipError_t launch_f64_rows_pm(int nx, int nu, int N, const Params64 &P, const Models64 &M)
{
    const int nrow_blocks = (P.batch + 3) / 4;
    const double *const no_gains = nullptr;
#define TINY_F64ROWS_PM_LAUNCH(NX, NU, NN)                                                                                                         \
    if (nx == NX && nu == NU && N == NN)                                                                                                           \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, NN, false, false, Models64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, no_gains, M);     \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS(TINY_F64ROWS_PM_LAUNCH)
#define TINY_F64ROWS_RT_PM_LAUNCH(NX, NU)                                                                                                          \
    if (nx == NX && nu == NU && N >= 2 && N <= F64ROWS_RT_MAX_N)                                                                                   \
    {                                                                                                                                              \
        if (N <= 32) hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 32, true, false, Models64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, no_gains, M); \
        else hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 64, true, false, Models64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, no_gains, M); \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS_RT(TINY_F64ROWS_RT_PM_LAUNCH)
    return hipErrorInvalidValue;
}
#elif defined(TINY_F64PM_UNIT)
// per-instance models, the on-chip closed loop: ONE family, the simulated one, wherever launch_rows64_sim has an instantiation.  A nominal run passes
// S.plant = S.w = S.x_traj = NULL: the plant step on the row's own gain rows is the nominal step bit for bit.  mpc_steps = 1 is served too
hipError_t launch_rows64_loop_pm(int nx, int nu, int N, const Params64 &P, const Mpc64 &L, const Sim64 &S, const Models64 &M)
{
    if (L.mpc_steps < 1 || P.max_iter < 1) return hipErrorInvalidValue;
    const int nrow_blocks = (P.batch + 3) / 4;
    const double *const no_gains = nullptr;
#define TINY_F64ROWS_PM_LOOP_LAUNCH(NX, NU, NN)                                                                                                    \
    if (nx == NX && nu == NU && N == NN)                                                                                                           \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, NN, false, true, Mpc64, Sim64, Models64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, no_gains, L, S, M); \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS(TINY_F64ROWS_PM_LOOP_LAUNCH)
#define TINY_F64ROWS_RT_PM_LOOP_LAUNCH(NX, NU)                                                                                                     \
    if (nx == NX && nu == NU && N >= 2 && N <= 32)                                                                                                 \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 32, true, true, Mpc64, Sim64, Models64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, no_gains, L, S, M); \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS_RT(TINY_F64ROWS_RT_PM_LOOP_LAUNCH)
    return hipErrorInvalidValue;
}
#elif defined(TINY_F64SIM_UNIT)
// a SIM instantiation wherever there is an MPC one: the unrolled horizons and the capacity-32 body of every sixteen-lane class
hipError_t launch_rows64_sim(int nx, int nu, int N, const Params64 &P, const double *gains, const Mpc64 &L, const Sim64 &S)
{
    if (L.mpc_steps <= 1 || P.max_iter < 1) return hipErrorInvalidValue;
    const int nrow_blocks = (P.batch + 3) / 4;
#define TINY_F64ROWS_SIM_LAUNCH(NX, NU, NN)                                                                                                        \
    if (nx == NX && nu == NU && N == NN)                                                                                                           \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, NN, false, true, Mpc64, Sim64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, L, S); \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS(TINY_F64ROWS_SIM_LAUNCH)
#define TINY_F64ROWS_RT_SIM_LAUNCH(NX, NU)                                                                                                         \
    if (nx == NX && nu == NU && N >= 2 && N <= 32)                                                                                                 \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 32, true, true, Mpc64, Sim64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, L, S); \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS_RT(TINY_F64ROWS_RT_SIM_LAUNCH)
    return hipErrorInvalidValue;
}
#elif defined(TINY_F64PS_UNIT) && TINY_F64PS_UNIT == 1
// per-instance settings, one solve: an instantiation wherever launch_f64_rows has one
hipError_t launch_f64_rows_ps(int nx, int nu, int N, const Params64 &P, const double *gains, const Settings64 &S)
{
    const int nrow_blocks = (P.batch + 3) / 4;
#define TINY_F64ROWS_PS_LAUNCH(NX, NU, NN)                                                                                                         \
    if (nx == NX && nu == NU && N == NN)                                                                                                           \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, NN, false, false, Settings64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, S);      \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS(TINY_F64ROWS_PS_LAUNCH)
#define TINY_F64ROWS_RT_PS_LAUNCH(NX, NU)                                                                                                          \
    if (nx == NX && nu == NU && N >= 2 && N <= F64ROWS_RT_MAX_N)                                                                                   \
    {                                                                                                                                              \
        if (N <= 32) hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 32, true, false, Settings64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, S); \
        else hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 64, true, false, Settings64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, S);  \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS_RT(TINY_F64ROWS_RT_PS_LAUNCH)
    return hipErrorInvalidValue;
}
#elif defined(TINY_F64PS_UNIT)
// per-instance settings, the on-chip closed loop with the nominal plant step: wherever launch_f64_rows has an MPC instantiation.  The caller sends no
// run here in which some instance has no budget
hipError_t launch_rows64_loop_ps(int nx, int nu, int N, const Params64 &P, const double *gains, const Mpc64 &L, const Settings64 &S)
{
    if (L.mpc_steps < 1 || P.max_iter < 1) return hipErrorInvalidValue;
    const int nrow_blocks = (P.batch + 3) / 4;
#define TINY_F64ROWS_PS_LOOP_LAUNCH(NX, NU, NN)                                                                                                    \
    if (nx == NX && nu == NU && N == NN)                                                                                                           \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, NN, false, true, Mpc64, Settings64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, L, S); \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS(TINY_F64ROWS_PS_LOOP_LAUNCH)
#define TINY_F64ROWS_RT_PS_LOOP_LAUNCH(NX, NU)                                                                                                     \
    if (nx == NX && nu == NU && N >= 2 && N <= 32)                                                                                                 \
    {                                                                                                                                              \
        hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 32, true, true, Mpc64, Settings64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, L, S); \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS_RT(TINY_F64ROWS_RT_PS_LOOP_LAUNCH)
    return hipErrorInvalidValue;
}
#else
// the unrolled instantiation for (nx, nu, N) where there is one, else the runtime-horizon body of the class at a capacity of 32 or, one solve only, 64
hipError_t launch_f64_rows(int nx, int nu, int N, const Params64 &P, const double *gains, const Mpc64 *L)
{
    const int nrow_blocks = (P.batch + 3) / 4;
#define TINY_F64ROWS_LAUNCH(NX, NU, NN)                                                                                                            \
    if (nx == NX && nu == NU && N == NN)                                                                                                           \
    {                                                                                                                                              \
        if (L) hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, NN, false, true, Mpc64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, *L);    \
        else hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, NN>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains);                              \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS(TINY_F64ROWS_LAUNCH)
#define TINY_F64ROWS_RT_LAUNCH(NX, NU)                                                                                                             \
    if (nx == NX && nu == NU && N >= 2 && N <= F64ROWS_RT_MAX_N)                                                                                   \
    {                                                                                                                                              \
        if (N <= 32 && L) hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 32, true, true, Mpc64>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains, *L); \
        else if (N <= 32) hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 32, true>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains);           \
        else if (L) return hipErrorInvalidValue; /* the capacity-64 body has no on-chip closed loop */                                             \
        else hipLaunchKernelGGL((admm_f64_rows_kernel<NX, NU, 64, true>), dim3(nrow_blocks), dim3(WAVE64), 0, 0, P, gains);                        \
        return hipGetLastError();                                                                                                                  \
    }
    TINY_FOR_EACH_F64ROWS_RT(TINY_F64ROWS_RT_LAUNCH)
    return hipErrorInvalidValue;
}
#endif // TINY_F64SIM_UNIT
} // namespace tinympc64
