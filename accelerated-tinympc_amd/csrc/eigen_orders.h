// eigen_orders.h — the reduction orders Eigen 3.4.90 (SSE2, packets of four floats) uses for the reference's lazy products, at run-time
// dimensions (the rules are stated at the top of admm_generic.hip).  Shared by the run-time-dimension kernel and the plant step.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace tinympc
{

__device__ inline float gen_tree(const float *v, int n) // T(0, n), evaluated with an explicit stack (depth <= 7)
{
    int lo_s[8], n_s[8], ph[8];
    float left[8];
    int sp = 0;
    lo_s[0] = 0; n_s[0] = n; ph[0] = 0;
    float ret = 0.f;
    while (sp >= 0)
    {
        const int lo = lo_s[sp], m = n_s[sp];
        if (m == 1) { ret = v[lo]; sp--; continue; }
        const int h = m / 2;
        if (ph[sp] == 0) { ph[sp] = 1; lo_s[sp + 1] = lo; n_s[sp + 1] = h; ph[sp + 1] = 0; sp++; }
        else if (ph[sp] == 1) { left[sp] = ret; ph[sp] = 2; lo_s[sp + 1] = lo + h; n_s[sp + 1] = m - h; ph[sp + 1] = 0; sp++; }
        else { ret = left[sp] + ret; sp--; }
    }
    return ret;
}
// element l of the packets [0, npk) summed by the halving tree over the packets
__device__ inline float gen_ptree_lane(const float *v, int npk, int l)
{
    int lo_s[8], n_s[8], ph[8];
    float left[8];
    int sp = 0;
    lo_s[0] = 0; n_s[0] = npk; ph[0] = 0;
    float ret = 0.f;
    while (sp >= 0)
    {
        const int lo = lo_s[sp], m = n_s[sp];
        if (m == 1) { ret = v[4 * lo + l]; sp--; continue; }
        const int h = m / 2;
        if (ph[sp] == 0) { ph[sp] = 1; lo_s[sp + 1] = lo; n_s[sp + 1] = h; ph[sp + 1] = 0; sp++; }
        else if (ph[sp] == 1) { left[sp] = ret; ph[sp] = 2; lo_s[sp + 1] = lo + h; n_s[sp + 1] = m - h; ph[sp + 1] = 0; sp++; }
        else { ret = left[sp] + ret; sp--; }
    }
    return ret;
}
__device__ inline float gen_seq(const float *t, int n)
{
    float acc = t[0];
    for (int k = 1; k < n; k++) acc = acc + t[k];
    return acc;
}
__device__ inline float gen_novec(const float *t, int n) { return gen_tree(t, n); } // (n <= 36: always inside Eigen's complete-unrolling limit)
__device__ inline float gen_vec(const float *t, int n)
{
    if (n < 4) return gen_novec(t, n);
    const int npk = n / 4, vs = 4 * npk;
    const float s0 = gen_ptree_lane(t, npk, 0), s1 = gen_ptree_lane(t, npk, 1), s2 = gen_ptree_lane(t, npk, 2), s3 = gen_ptree_lane(t, npk, 3);
    float res = (s0 + s2) + (s1 + s3);
    if (vs != n) res = res + gen_tree(t + vs, n - vs);
    return res;
}
__device__ inline float gen_gemv_rm(const float *t, int n) // Eigen's row-major GEMV inner product over the products t[k]
{
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
    const int vs = (n / 4) * 4;
    for (int k = 0; k < vs; k += 4) { c0 = c0 + t[k]; c1 = c1 + t[k + 1]; c2 = c2 + t[k + 2]; c3 = c3 + t[k + 3]; }
    float res = (c0 + c2) + (c1 + c3);
    for (int k = vs; k < n; k++) res = res + t[k];
    return 0.f + res;
}
// (row i of a column-major rows x cols matrix) . xin for a lazy product whose result has `rows` rows
__device__ inline float gen_row_dot(const float *M, int rows, int cols, int i, const float *xin, float *t)
{
    if (rows == 1)
    {
        for (int k = 0; k < cols; k++) t[k] = M[k] * xin[k];
        return gen_vec(t, cols);
    }
    for (int k = 0; k < cols; k++) t[k] = M[(size_t)k * rows + i] * xin[k];
    return (rows % 4 == 0) ? gen_seq(t, cols) : gen_novec(t, cols);
}

} // namespace tinympc
