// quadrotor_tracking_montecarlo.cpp — a Monte-Carlo study of ONE controller against MANY plants, written against the C-ABI only
// (include/tinympc_batch.h).  Plain C++17, no HIP/Eigen/torch types:
//
//   g++ -std=c++17 -O2 -Iinclude examples/quadrotor_tracking_montecarlo.cpp -Laccelerated-tinympc_amd/lib -ltinympc_hip
//       -Wl,-rpath,$PWD/accelerated-tinympc_amd/lib -o build/quadrotor_tracking_montecarlo
//   ./build/quadrotor_tracking_montecarlo accelerated-tinympc_amd/data/quadrotor_20hz.bin 4096 60
//
// The controller is the 20 Hz quadrotor's (one cache for the batch, the problem data file of quadrotor_tracking_batched.cpp).  Every instance
// gets its own plant around that model — the columns of Bdyn scaled by 0.9 ... 1.1 (mass and motor gain), the non-zero entries of Adyn by
// 0.98 ... 1.02 — and a random disturbance on the velocities at every step.  All instances track the y_axis_line trajectory from the same
// start; the whole closed loop is ONE call (tiny_batch_mpc_run_log: on the 16-lane kernel one launch), which returns the state trajectory and
// iter / status of every solve, and the study prints the mean and the worst final tracking error over the plants and, per step, how many
// instances returned unsolved.
#include "tinympc_batch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static constexpr int NX = 12, NU = 4, N = 30, NTOTAL = 301;

#define CHECK(call)                                                                        \
    do                                                                                     \
    {                                                                                      \
        int rc_ = (call);                                                                  \
        if (rc_ < 0)                                                                       \
        {                                                                                  \
            std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, tiny_batch_last_error()); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

// row-major (as in the reference's headers) -> column-major float (Eigen's storage, what the ABI takes)
static std::vector<float> colmajor(const double *rm, int rows, int cols)
{
    std::vector<float> cm((size_t)rows * cols);
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < cols; j++) cm[(size_t)j * rows + i] = (float)rm[(size_t)i * cols + j];
    return cm;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s quadrotor_20hz.bin [batch] [steps]\n", argv[0]); return 2; }
    const int B = argc > 2 ? std::atoi(argv[2]) : 1024, steps = std::min(argc > 3 ? std::atoi(argv[3]) : 60, NTOTAL - N - 1);
    if (B < 1 || steps < 1) { std::fprintf(stderr, "batch and steps must be >= 1\n"); return 2; }
    const size_t ndbl = 1 + NX * NX + NX * NU + NU * NX + NX * NX + NU * NU + NX * NX + NX;
    std::vector<double> raw(ndbl);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(raw.data(), sizeof(double), ndbl, f) != ndbl) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
    const double *p = raw.data();
    const float rho = (float)*p++;
    const auto A = colmajor(p, NX, NX); p += NX * NX;
    const auto Bd = colmajor(p, NX, NU); p += NX * NU;
    const auto K = colmajor(p, NU, NX); p += NU * NX;
    const auto Pinf = colmajor(p, NX, NX); p += NX * NX;
    const auto Qi = colmajor(p, NU, NU); p += NU * NU;
    const auto Am = colmajor(p, NX, NX); p += NX * NX;
    std::vector<float> Q(p, p + NX);

    // reference trajectory: z = 1 m, y from 0 to 4 m, dy = 0.2666667 m/s (quadrotor_20hz_y_axis_line.hpp)
    std::vector<float> table((size_t)NTOTAL * NX, 0.f);
    for (int k = 0; k < NTOTAL; k++)
    {
        table[(size_t)k * NX + 1] = (float)(std::round(k * 4.0 / 300.0 * 1e7) / 1e7);
        table[(size_t)k * NX + 2] = 1.f;
        table[(size_t)k * NX + 7] = k < NTOTAL - 1 ? 0.2666667f : 0.f;
    }
    std::vector<int> start(B, 0);
    std::vector<float> x0((size_t)B * NX);
    for (int b = 0; b < B; b++)
        for (int i = 0; i < NX; i++) x0[(size_t)b * NX + i] = table[i]; // x0 = Xref.col(0) (tracking.cpp:88)
    std::vector<float> xmin((size_t)N * NX, -5.f), xmax((size_t)N * NX, 5.f), umin((size_t)(N - 1) * NU, -0.5f), umax((size_t)(N - 1) * NU, 0.5f);

    // the plants (column-major, one per instance) and the disturbance [steps][B][nx]: velocity kicks of 2 cm/s standard deviation
    std::mt19937 rng(20241024);
    std::uniform_real_distribution<float> gain(0.9f, 1.1f), drift(0.98f, 1.02f);
    std::normal_distribution<float> kick(0.f, 0.02f);
    std::vector<float> Ap((size_t)B * NX * NX), Bp((size_t)B * NX * NU), w((size_t)steps * B * NX, 0.f);
    for (int b = 0; b < B; b++)
    {
        for (int e = 0; e < NX * NX; e++) Ap[(size_t)b * NX * NX + e] = A[e] * (e % (NX + 1) == 0 ? 1.f : drift(rng)); // the diagonal stays 1
        for (int m = 0; m < NU; m++)
        {
            const float g = gain(rng);
            for (int r = 0; r < NX; r++) Bp[(size_t)b * NX * NU + (size_t)m * NX + r] = Bd[(size_t)m * NX + r] * g;
        }
    }
    for (size_t e = 0; e < w.size(); e++)
        if (e % NX >= 6 && e % NX < 9) w[e] = kick(rng);

    TinyBatch *tb = nullptr;
    CHECK(tiny_batch_create(&tb, NX, NU, N, B, 0));
    CHECK(tiny_batch_set_cache(tb, rho, K.data(), Pinf.data(), Qi.data(), Am.data()));
    CHECK(tiny_batch_set_dynamics(tb, A.data(), Bd.data(), Q.data()));
    CHECK(tiny_batch_set_settings(tb, 1e-3f, 1e-3f, 100, 1, 1, 1)); // quadrotor_tracking.cpp:75-80
    CHECK(tiny_batch_set_xmin(tb, xmin.data(), 1)); CHECK(tiny_batch_set_xmax(tb, xmax.data(), 1));
    CHECK(tiny_batch_set_umin(tb, umin.data(), 1)); CHECK(tiny_batch_set_umax(tb, umax.data(), 1));
    CHECK(tiny_batch_set_xref_window(tb, table.data(), NTOTAL, start.data()));
    CHECK(tiny_batch_set_x0(tb, x0.data()));
    CHECK(tiny_batch_set_plant(tb, Ap.data(), Bp.data(), /*shared=*/0));
    std::printf("solve kernel: %s, closed-loop kernel: %s, %d plants (plant mode %d), %d steps\n", tiny_batch_kernel_name(tb),
                tiny_batch_closed_loop_kernel_name(tb), B, tiny_batch_plant_mode(tb), steps);

    std::vector<float> xs((size_t)steps * B * NX);
    std::vector<int> iters((size_t)steps * B), status((size_t)steps * B);
    CHECK(tiny_batch_mpc_run_log(tb, steps, /*window_advance=*/1, w.data(), /*u0_traj=*/nullptr, xs.data(), iters.data(), status.data()));

    // the per-step solver log: a trajectory is to be trusted only where its solves converged within max_iter
    for (int k : {0, steps / 2, steps - 1})
    {
        int unsolved = 0, most = 0;
        for (int b = 0; b < B; b++)
        {
            unsolved += status[(size_t)k * B + b] == TINY_STATUS_UNSOLVED;
            most = std::max(most, iters[(size_t)k * B + b]);
        }
        std::printf("step %3d: %d of %d instances unsolved, at most %d iterations\n", k, unsolved, B, most);
    }

    // row k of the state trajectory is the state after step k: it is compared with row k + 1 of the table
    for (int k : {0, steps / 2, steps - 1})
    {
        double mean = 0, worst = 0;
        for (int b = 0; b < B; b++)
        {
            double e2 = 0;
            for (int i = 0; i < NX; i++)
            {
                const double dlt = xs[((size_t)k * B + b) * NX + i] - table[(size_t)(k + 1) * NX + i];
                e2 += dlt * dlt;
            }
            mean += std::sqrt(e2);
            worst = std::max(worst, std::sqrt(e2));
        }
        std::printf("step %3d: mean tracking error %.6f, worst %.6f%s\n", k, mean / B, worst, k == steps - 1 ? "  (final)" : "");
    }
    tiny_batch_destroy(tb);
    return 0;
}
