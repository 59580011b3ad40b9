// riccati_batch.hip — tiny_riccati (riccati.cpp) for many independent systems on the device, fp64, bitwise equal per system.
//
// Mapping: one thread per system.  A system's working matrices (P, Pn, A'P, A - BK, K, Kprev, B'P, the right-hand side and the LU copy of
// R1 + B'PB, about 800 doubles for nx = 12, nu = 4) do not fit a thread's registers and would spill as run-time-indexed arrays, so they live in a
// scratch buffer in global memory, interleaved by wavefront: element e of system s sits at ((s / 64) * E + e) * 64 + s % 64, so that the 64 lanes of a
// wave touch one contiguous 512-byte line per element.  A and B are read from the caller's arrays.  Systems finish after different iteration counts;
// a lane that has converged idles until its wave is done.
//
// Every output element goes through the operation sequence of riccati.cpp (built, like this file, with -ffp-contract=off; fp64 division is
// correctly rounded on gfx950): a product element starts at 0.0 and adds its products in ascending k, add(X, Y, s) is x + s * y, LU with strict
// ">" partial pivoting skipping rows with f == 0.0, the same back substitution, the fmax / fabs stop test at 1e-5, the last iterate kept at 1000.
#include "tinympc_internal.h"

namespace tinympc
{
namespace
{

struct SM // a matrix of the interleaved scratch (column-major, 64 doubles between elements)
{
    double *p;
    int r;
    __device__ double &operator()(int i, int j) const { return p[(size_t)(j * r + i) * 64]; }
};
struct CM // a column-major matrix of one system in a caller's array
{
    double *p;
    int r;
    __device__ double &operator()(int i, int j) const { return p[(size_t)j * r + i]; }
};

// lu_solve of riccati.cpp, in place: G (n x n) and RHS (n x ncols) are overwritten, X = G^-1 RHS; false where G is singular
template <class XM>
__device__ bool lu_solve_dev(const SM &G, const SM &RHS, int n, int ncols, const XM &X)
{
    for (int c = 0; c < n; c++)
    {
        int piv = c;
        for (int r = c + 1; r < n; r++)
            if (fabs(G(r, c)) > fabs(G(piv, c))) piv = r;
        if (G(piv, c) == 0.0) return false;
        if (piv != c)
        {
            for (int j = 0; j < n; j++) { const double t = G(c, j); G(c, j) = G(piv, j); G(piv, j) = t; }
            for (int j = 0; j < ncols; j++) { const double t = RHS(c, j); RHS(c, j) = RHS(piv, j); RHS(piv, j) = t; }
        }
        for (int r = c + 1; r < n; r++)
        {
            const double f = G(r, c) / G(c, c);
            if (f == 0.0) continue;
            for (int j = c; j < n; j++) G(r, j) = G(r, j) - f * G(c, j);
            for (int j = 0; j < ncols; j++) RHS(r, j) = RHS(r, j) - f * RHS(c, j);
        }
    }
    for (int j = 0; j < ncols; j++)
        for (int i = n - 1; i >= 0; i--)
        {
            double s = RHS(i, j);
            for (int k = i + 1; k < n; k++) s = s - G(i, k) * X(k, j);
            X(i, j) = s / G(i, i);
        }
    return true;
}

__global__ __launch_bounds__(64) void riccati_batch_kernel(int nx, int nu, int s0, int count, const double *__restrict__ A_, const double *__restrict__ B_,
                                                           const double *__restrict__ Qd, const double *__restrict__ Rd, const double *__restrict__ rhod,
                                                           double *__restrict__ Kinf, double *__restrict__ Pinf, double *__restrict__ Quu_inv,
                                                           double *__restrict__ AmBKt, double *__restrict__ d2p, int *__restrict__ iters,
                                                           double *__restrict__ scratch, int *__restrict__ nfail)
{
    const int t = blockIdx.x * 64 + threadIdx.x, s = s0 + t;
    if (s >= count) return;
    const int E = riccati_batch_doubles(nx, nu);
    double *base = scratch + (size_t)(t / 64) * E * 64 + (t % 64);
    int off = 0;
    auto take = [&](int rows, int n) { SM m{base + (size_t)off * 64, rows}; off += n; return m; };
    const SM P = take(nx, nx * nx), Pn = take(nx, nx * nx), AtP = take(nx, nx * nx), AmBK = take(nx, nx * nx);
    const SM K = take(nu, nu * nx), Kp = take(nu, nu * nx), BtP = take(nu, nu * nx), RHS = take(nu, nu * (nx > nu ? nx : nu));
    const SM Gm = take(nu, nu * nu), Xq = take(nu, nu * nu);
    const CM A{const_cast<double *>(A_) + (size_t)s * nx * nx, nx}, B{const_cast<double *>(B_) + (size_t)s * nx * nu, nx};
    const double rho = rhod[s];
    const double *Q = Qd + (size_t)s * nx, *R = Rd + (size_t)s * nu;
    auto Q1 = [&](int i, int j) { return i == j ? Q[i] + rho : 0.0; };
    auto R1 = [&](int i, int j) { return i == j ? R[i] + rho : 0.0; };
    for (int j = 0; j < nx; j++)
        for (int i = 0; i < nx; i++) P(i, j) = i == j ? rho : 0.0;
    for (int e = 0; e < nu * nx; e++) Kp(e % nu, e / nu) = 0.0;
    bool ok = true;
    int n_it = 1000;
    for (int it = 0; it < 1000; it++)
    {
        // BtP = B' P ;  G = R1 + BtP B ;  RHS = BtP A ;  K = G^-1 RHS
        for (int j = 0; j < nx; j++)
            for (int i = 0; i < nu; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + B(k, i) * P(k, j);
                BtP(i, j) = acc;
            }
        for (int j = 0; j < nu; j++)
            for (int i = 0; i < nu; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + BtP(i, k) * B(k, j);
                Gm(i, j) = R1(i, j) + 1.0 * acc;
            }
        for (int j = 0; j < nx; j++)
            for (int i = 0; i < nu; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + BtP(i, k) * A(k, j);
                RHS(i, j) = acc;
            }
        if (!lu_solve_dev(Gm, RHS, nu, nx, K)) { ok = false; break; }
        // Pn = Q1 + (A' P) (A - B K)
        for (int j = 0; j < nx; j++)
            for (int i = 0; i < nx; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nu; k++) acc = acc + B(i, k) * K(k, j);
                AmBK(i, j) = A(i, j) + -1.0 * acc;
            }
        for (int j = 0; j < nx; j++)
            for (int i = 0; i < nx; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + A(k, i) * P(k, j);
                AtP(i, j) = acc;
            }
        for (int j = 0; j < nx; j++)
            for (int i = 0; i < nx; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + AtP(i, k) * AmBK(k, j);
                Pn(i, j) = Q1(i, j) + 1.0 * acc;
            }
        double md = 0.0;
        for (int e = 0; e < nu * nx; e++) md = fmax(md, fabs(K(e % nu, e / nu) - Kp(e % nu, e / nu)));
        if (md < 1e-5) { n_it = it + 1; break; }
        for (int e = 0; e < nu * nx; e++) Kp(e % nu, e / nu) = K(e % nu, e / nu);
        for (int e = 0; e < nx * nx; e++) P(e % nx, e / nx) = Pn(e % nx, e / nx);
    }
    if (ok)
    {
        // Quu_inv = (R1 + B' Pn B)^-1
        for (int j = 0; j < nx; j++)
            for (int i = 0; i < nu; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + B(k, i) * Pn(k, j);
                BtP(i, j) = acc;
            }
        for (int j = 0; j < nu; j++)
            for (int i = 0; i < nu; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + BtP(i, k) * B(k, j);
                Gm(i, j) = R1(i, j) + 1.0 * acc;
                RHS(i, j) = i == j ? 1.0 : 0.0;
            }
        ok = lu_solve_dev(Gm, RHS, nu, nu, Xq);
    }
    if (!ok)
    {
        iters[s] = -1;
        atomicAdd(nfail, 1);
        return;
    }
    const CM Ko{Kinf + (size_t)s * nu * nx, nu}, Po{Pinf + (size_t)s * nx * nx, nx}, Qo{Quu_inv + (size_t)s * nu * nu, nu}, Ao{AmBKt + (size_t)s * nx * nx, nx};
    for (int j = 0; j < nx; j++)
        for (int i = 0; i < nu; i++) Ko(i, j) = K(i, j);
    for (int j = 0; j < nx; j++)
        for (int i = 0; i < nx; i++) { Po(i, j) = Pn(i, j); Ao(i, j) = AmBK(j, i); }
    for (int j = 0; j < nu; j++)
        for (int i = 0; i < nu; i++) Qo(i, j) = Xq(i, j);
    if (d2p) // coeff_d2p = K' R1 - (AmBKt Pn) B
    {
        for (int j = 0; j < nx; j++)
            for (int i = 0; i < nx; i++)
            {
                double acc = 0.0;
                for (int k = 0; k < nx; k++) acc = acc + AmBK(k, i) * Pn(k, j);
                AtP(i, j) = acc;
            }
        const CM Co{d2p + (size_t)s * nx * nu, nx};
        for (int j = 0; j < nu; j++)
            for (int i = 0; i < nx; i++)
            {
                double kr = 0.0, y = 0.0;
                for (int k = 0; k < nu; k++) kr = kr + K(k, i) * R1(k, j);
                for (int k = 0; k < nx; k++) y = y + AtP(i, k) * B(k, j);
                Co(i, j) = kr + -1.0 * y;
            }
    }
    iters[s] = n_it;
}

} // namespace

hipError_t launch_riccati_batch(int nx, int nu, int s0, int n, int count, const double *A, const double *B, const double *Q, const double *R, const double *rho,
                                double *Kinf, double *Pinf, double *Quu_inv, double *AmBKt, double *coeff_d2p, int *iters, double *scratch, int *nfail,
                                hipStream_t stream)
{
    hipLaunchKernelGGL(riccati_batch_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, nx, nu, s0, s0 + n < count ? s0 + n : count, A, B, Q, R, rho, Kinf, Pinf,
                       Quu_inv, AmBKt, coeff_d2p, iters, scratch, nfail);
    return hipGetLastError();
}

} // namespace tinympc
