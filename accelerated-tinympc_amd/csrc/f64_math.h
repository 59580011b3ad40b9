// f64_math.h — device helpers of the fp64 kernels (admm_f64_*.hip): sums in the orders of the reference's SSE2 Eigen build, whose packets hold
// PS = 2 doubles (sequential for packet-evaluated lazy products, halving tree for coefficient-evaluated ones, packet tree + s0 + s1 for vectorised
// reductions), the DPP row operations of the sixteen-lane mapping, and the plant step in both mappings.  Every product and sum is a separately
// rounded fp64 operation (the library is built with -ffp-contract=off).
#pragma once
#include "f64_internal.h"

namespace tinympc64
{
// ---- reductions in the reference's orders (Eigen 3.4.90: redux_novec_unroller, redux_vec_unroller, etor_product_packet_impl) ----
template <int LO, int CNT, int NN>
__device__ __forceinline__ double tree_sum(const double (&t)[NN])
{
    if constexpr (CNT == 1) return t[LO];
    else
    {
        constexpr int H = CNT / 2;
        return tree_sum<LO, H>(t) + tree_sum<LO + H, CNT - H>(t);
    }
}
template <int PLO, int PCNT, int L, int NN>
__device__ __forceinline__ double ptree_sum(const double (&t)[NN]) // lane L of the packets [PLO, PLO + PCNT)
{
    if constexpr (PCNT == 1) return t[PS * PLO + L];
    else
    {
        constexpr int H = PCNT / 2;
        return ptree_sum<PLO, H, L>(t) + ptree_sum<PLO + H, PCNT - H, L>(t);
    }
}
template <int NN>
__device__ __forceinline__ double seq_sum(const double (&t)[NN])
{
    double acc = t[0];
#pragma unroll
    for (int k = 1; k < NN; k++) acc = acc + t[k];
    return acc;
}
template <int NN>
__device__ __forceinline__ double novec_sum(const double (&t)[NN])
{
    if constexpr (NN == 1) return t[0];
    else if constexpr (3 * NN - 1 <= 110) return tree_sum<0, NN>(t);
    else return seq_sum(t);
}
template <int NN>
__device__ __forceinline__ double vec_sum(const double (&t)[NN])
{
    static_assert(3 * NN - 1 <= 110 * PS, "beyond Eigen's unrolling limit the order is not restated");
    if constexpr (NN < PS) return novec_sum(t);
    else
    {
        constexpr int NPK = NN / PS;
        double res = ptree_sum<0, NPK, 0>(t) + ptree_sum<0, NPK, 1>(t); // predux of a 2-double packet
        if constexpr (NN % PS != 0) res = res + tree_sum<PS * NPK, NN - PS * NPK>(t);
        return res;
    }
}
// (row i of a column-major ROWS x COLS matrix) . xin, as a lazy product whose result has ROWS rows
template <int ROWS, int COLS>
__device__ __forceinline__ double row_dot(const double *M, int i, const double (&xin)[COLS])
{
    static_assert(ROWS <= PS || ROWS % PS == 0, "results with rows > 2 and odd: the reference's order depends on alignment");
    double t[COLS];
#pragma unroll
    for (int k = 0; k < COLS; k++) t[k] = M[k * ROWS + i] * xin[k];
    if constexpr (ROWS > 1 && ROWS % PS == 0) return seq_sum(t);
    else if constexpr (ROWS == 1) return vec_sum(t);
    else return novec_sum(t);
}

template <int CTRL>
__device__ __forceinline__ double dpp64(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// t[k] = M[k] * s[K0 + k], s[j] = the value lane j of this lane's row holds (row_newbcast:j = 0x150 + j)
template <int K0, int CNT, int K = 0>
__device__ __forceinline__ void row_products(double (&t)[CNT], double s, const double (&M)[CNT])
{
    if constexpr (K < CNT)
    {
        t[K] = M[K] * dpp64<0x150 + K0 + K>(s);
        row_products<K0, CNT, K + 1>(t, s, M);
    }
}
__device__ __forceinline__ double row_max(double v) // max over the 16 lanes of a row, every lane gets it
{
    v = fmax(v, dpp64<0x128>(v)); v = fmax(v, dpp64<0x124>(v)); v = fmax(v, dpp64<0x122>(v)); v = fmax(v, dpp64<0x121>(v));
    return v;
}
// the reference's order for a lazy product whose result has ROWS rows (see row_dot above)
template <int ROWS, int CNT>
__device__ __forceinline__ double lazy_sum(const double (&t)[CNT])
{
    static_assert(ROWS <= PS || ROWS % PS == 0, "results with rows > 2 and odd: the reference's order depends on alignment");
    if constexpr (ROWS > 1 && ROWS % PS == 0) return seq_sum(t);
    else if constexpr (ROWS == 1) return vec_sum(t);
    else return novec_sum(t);
}

// One row of the plant step A*x + B*u on the sixteen lanes: Ar / Br are this lane's row of A and B, x and u the lane's element of [x ; u].  The order is
// plant64_step's: a product whose rows and depth are both >= 8 is the GEMV accumulator from +0, anything smaller the lazy product's sequential sum.
template <int NX, int NU>
__device__ __forceinline__ double plant_row(const double (&Ar)[NX], const double (&Br)[NU], double x, double u)
{
    double t[NX], t2[NU];
    row_products<0, NX>(t, x, Ar);
    double ax;
    if constexpr (NX >= 8)
    {
        double c = 0.0;
#pragma unroll
        for (int j = 0; j < NX; j++) c = t[j] + c;
        ax = c * 1.0 + 0.0;
    }
    else ax = lazy_sum<NX>(t);
    row_products<NX, NU>(t2, u, Br);
    return ax + lazy_sum<NX>(t2);
}

// Plant step of the examples' closed loop (quadrotor_hovering.cpp:110-111): x.col(0) <- Adyn * x.col(0) + Bdyn * u.col(0), in
// Eigen's order for that expression over tiny_VectorNx: a product whose rows and depth are both >= 8 runs through the
// column-major GEMV kernel (row accumulator from +0, then alpha * acc + result), anything smaller is the lazy product's
// sequential sum (tests/test_oracle.py: test_plant_step_bit_exact_vs_compiled_reference pins the oracle's restatement of
// this against the compiled expression, fp64 configurations included).
template <int NX, int NU>
__device__ __forceinline__ void plant64_step(double *__restrict__ X, const double (&u)[NU], const double *__restrict__ mats, int b, int bpad)
{
    static_assert(!(NX >= 8 && NU >= 8), "Bdyn*u would take the GEMV kernel too");
    constexpr int OFF_A = NU * NX + NX * NX + NU * NU + NX * NX, OFF_B = OFF_A + NX * NX;
    const double *A = mats + OFF_A, *Bm = mats + OFF_B;
    double x[NX], xn[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) x[j] = X[(size_t)j * bpad + b];
#pragma unroll
    for (int i = 0; i < NX; i++)
    {
        double a;
        if constexpr (NX >= 8)
        {
            double c = 0.0;
#pragma unroll
            for (int j = 0; j < NX; j++) c = A[j * NX + i] * x[j] + c;
            a = c * 1.0 + 0.0;
        }
        else a = row_dot<NX, NX>(A, i, x);
        xn[i] = a + row_dot<NX, NU>(Bm, i, u);
    }
#pragma unroll
    for (int i = 0; i < NX; i++) X[(size_t)i * bpad + b] = xn[i];
}
} // namespace tinympc64
