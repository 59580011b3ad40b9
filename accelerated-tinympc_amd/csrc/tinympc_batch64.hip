// tinympc_batch64.hip — the batched TinyMPC ADMM solver for `typedef double tinytype` (the reference as shipped,
// src/tinympc/glob_opts.hpp:3): the handle, the device workspace, the choice of kernel and the C-ABI of include/tinympc_batch64.h.
//
// Host code only.  Every kernel lives in a translation unit of its own (admm_f64_thread.hip, admm_f64_rows.hip, admm_f64_rowsim.hip,
// admm_f64_plant.hip; admm_f64_rows_pm.hip, admm_f64_rowsim_pm.hip, admm_f64_thread_pm.hip: per-instance models; admm_f64_rows_ps.hip,
// admm_f64_rowloop_ps.hip, admm_f64_thread_ps.hip: per-instance settings; batch64_helpers.hip: the three
// that move arrays between the host's layout and the workspace's) and is reached through the typed launchers of f64_internal.h, so nothing in this
// file — not the order of its functions, not a name in it — has a bearing on device code.
//
// Every per-instance array is stored instance-minor — element (step, row) of instance b at ((step * dim + row) * Bpad + b).  Results are
// bitwise equal to the compiled reference (tests/test_parity_gpu.py: golden vectors of the as-shipped fp64 N = 10 hovering run).
// There is no CPU fallback.
#include "f64_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace
{
using namespace tinympc64;

thread_local std::string g_err64;
int fail64(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err64 = buf;
    return code;
}
#define HIP64(expr)                                                                                         \
    do                                                                                                      \
    {                                                                                                       \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return fail64(TINY_BATCH_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define CHECK64(c, ...) \
    if (!(c)) return fail64(TINY_BATCH_EINVAL, __VA_ARGS__)
// a negative return is an error, already worded; 1 (some instance unsolved) is a result
#define TRY64(expr)              \
    do                           \
    {                            \
        const int rc_ = (expr);  \
        if (rc_ < 0) return rc_; \
    } while (0)

// a temporary device buffer: freed when it goes out of scope, unless release() has handed it on
template <typename T>
struct Scratch64
{
    T *p = nullptr;
    Scratch64() = default;
    Scratch64(const Scratch64 &) = delete;
    Scratch64 &operator=(const Scratch64 &) = delete;
    ~Scratch64() { (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, n * sizeof(T)); }
    hipError_t upload(const T *src, size_t n)
    {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    T *release() { T *q = p; p = nullptr; return q; }
};

bool xfam(int id) { return id == TINY_ARR_X || id == TINY_ARR_Q || id == TINY_ARR_P || id == TINY_ARR_V || id == TINY_ARR_VNEW || id == TINY_ARR_G; }

} // namespace

struct TinyBatch64
{
    int nx = 0, nu = 0, N = 0, batch = 0, bpad = 0, device = 0;
    double *arr[TINY_ARR_COUNT] = {};
    double *in[5] = {};        // xref, xmin, xmax, umin, umax
    int in_stride[5] = {1, 1, 1, 1, 1};
    bool in_set[5] = {};
    double *mats = nullptr, *res = nullptr, *staging = nullptr;
    double *row_gains = nullptr; // [3nx + 2nu + 1 + nx][16]: the matrices as one register per column and lane (admm_f64_rows_kernel)
    int kernel_choice = 0;       // tiny_batch64_select_kernel: 0 auto, 1 thread per instance, 2 sixteen lanes per instance
    int *status = nullptr, *iter = nullptr, *n_unsolved = nullptr;
    // window reference (tiny_batch64_set_xref_window): the table and the per-instance starts live on the device; xwin is the window gathered
    // into a per-instance array for the kernels that read one (allocated on first use, redone after the starts have moved)
    double *table = nullptr, *xwin = nullptr, *u0_traj = nullptr;
    int *xref_start = nullptr;
    int table_rows = 0;      // > 0: the reference is the window
    bool xwin_valid = false;
    size_t u0_traj_cap = 0;  // doubles
    // the simulated plant of the closed-loop calls (tiny_batch64_set_plant): 0 the model's own Adyn / Bdyn, 1 one shared plant, 2 one per instance.
    // Column-major copies for the plant kernel ([1 or batch][nx*nx], [1 or batch][nx*nu]) and, where nx + nu <= 16, the rows of [A | B] packed for the
    // sixteen lanes ([1 or batch][(nx + nu) * 16]: Sim64).  sim_w / sim_x: the device copies of a call's w and x_traj; like u0_traj they grow only
    int plant_mode = 0;
    double *plant_A = nullptr, *plant_B = nullptr, *plant_rows = nullptr, *sim_w = nullptr, *sim_x = nullptr;
    size_t sim_w_cap = 0, sim_x_cap = 0;
    // the device copies of a call's per-step solver log (tiny_batch64_mpc_run_log): [steps][batch] ints each, grow only
    int *log_iter = nullptr, *log_status = nullptr;
    size_t log_iter_cap = 0, log_status_cap = 0;
    // per-instance models (tiny_batch64_set_models): one record per instance in the layout of `mats` ([batch][rec_len()]) and rho [batch]; while pm
    // is set they replace mats, row_gains and rho in every launch
    bool pm = false;
    double *pm_rec = nullptr, *pm_rho = nullptr;
    // per-instance settings (tiny_batch64_set_instance_settings): the caller's arrays as given (an empty vector: the field was NULL and follows the
    // batch's value), the records built from them and from the batch's settings ([batch], rebuilt by every setter), the largest and the smallest budget
    bool ps = false;
    std::vector<double> ps_tol[2];
    std::vector<int> ps_int[4]; // max_iter, check_termination, en_state_bound, en_input_bound
    InstSettings64 *ps_rec = nullptr;
    int ps_max_iter = 0, ps_min_iter = 0;
    std::vector<double> hm; // host copy of the packed matrices
    bool have_cache = false, have_dyn = false, have_settings = false, mats_dirty = true;
    double rho = 0, abs_pri_tol = 0, abs_dua_tol = 0;
    int max_iter = 0, check_termination = 1, en_state_bound = 0, en_input_bound = 0;
};

namespace
{
size_t steps_of(const TinyBatch64 *tb, int id) { return xfam(id) ? tb->N : tb->N - 1; }
int dim_of(const TinyBatch64 *tb, int id) { return xfam(id) ? tb->nx : tb->nu; }
size_t mat_off(const TinyBatch64 *tb, int which) // Kinf, Pinf, Quu_inv, AmBKt, Adyn, Bdyn, Q
{
    const size_t nx = tb->nx, nu = tb->nu;
    const size_t sz[7] = {nu * nx, nx * nx, nu * nu, nx * nx, nx * nx, nx * nu, nx};
    size_t o = 0;
    for (int k = 0; k < which; k++) o += sz[k];
    return o;
}
// lane r of a row holds, per matrix column, the element of the row it owns (x rows r < nx, u rows nx <= r < nx + nu):
//   M1[k]  x rows Adyn(r,k)   | u rows Kinf(m,k)        M2[m]  x rows Bdyn(r,m)
//   M3[k]  x rows AmBKt(r,k)  | u rows Bdyn(k,m)        M45[m] x rows Kinf(m,r) | u rows Quu_inv(mr,m)
//   Q      x rows Q(r)                                  PT[k]  x rows Pinf(k,r)
std::vector<double> pack_row_gains(const TinyBatch64 *tb)
{
    const int nx = tb->nx, nu = tb->nu;
    const double *K = tb->hm.data() + mat_off(tb, 0), *Pinf = tb->hm.data() + mat_off(tb, 1), *Quu = tb->hm.data() + mat_off(tb, 2),
                 *Am = tb->hm.data() + mat_off(tb, 3), *A = tb->hm.data() + mat_off(tb, 4), *B = tb->hm.data() + mat_off(tb, 5),
                 *Q = tb->hm.data() + mat_off(tb, 6);
    std::vector<double> g((size_t)(3 * nx + 2 * nu + 1) * 16, 0.0);
    for (int r = 0; r < 16; r++)
    {
        const bool isx = r < nx, isu = r >= nx && r < nx + nu;
        const int mr = r - nx;
        for (int k = 0; k < nx; k++)
        {
            g[(size_t)k * 16 + r] = isx ? A[k * nx + r] : (isu ? K[k * nu + mr] : 0.0);
            g[(size_t)(nx + nu + k) * 16 + r] = isx ? Am[k * nx + r] : (isu ? B[mr * nx + k] : 0.0);
            g[(size_t)(2 * nx + 2 * nu + 1 + k) * 16 + r] = isx ? Pinf[r * nx + k] : 0.0;
        }
        for (int m = 0; m < nu; m++)
        {
            g[(size_t)(nx + m) * 16 + r] = isx ? B[m * nx + r] : 0.0;
            g[(size_t)(2 * nx + nu + m) * 16 + r] = isx ? K[r * nu + m] : (isu ? Quu[m * nu + mr] : 0.0);
        }
        g[(size_t)(2 * nx + 2 * nu) * 16 + r] = isx ? Q[r] : 0.0;
    }
    return g;
}
int set_input(TinyBatch64 *tb, int which, const double *src, int shared)
{
    CHECK64(tb && src, "NULL argument");
    HIP64(hipSetDevice(tb->device));
    const int dim = which < 3 ? tb->nx : tb->nu, steps = which < 3 ? tb->N : tb->N - 1;
    const int stride = shared ? 1 : tb->bpad, nb = shared ? 1 : tb->batch;
    if (tb->in[which] && tb->in_stride[which] != stride) { (void)hipFree(tb->in[which]); tb->in[which] = nullptr; }
    if (!tb->in[which])
    {
        HIP64(hipMalloc((void **)&tb->in[which], (size_t)steps * dim * stride * sizeof(double)));
        HIP64(hipMemset(tb->in[which], 0, (size_t)steps * dim * stride * sizeof(double)));
    }
    HIP64(hipMemcpy(tb->staging, src, (size_t)nb * steps * dim * sizeof(double), hipMemcpyHostToDevice));
    HIP64(launch_pack64(tb->staging, tb->in[which], nb, steps, dim, stride, 0, steps));
    HIP64(hipDeviceSynchronize());
    tb->in_stride[which] = stride;
    tb->in_set[which] = true;
    if (which == 0) tb->table_rows = 0; // an array reference replaces a window
    return 0;
}
// gathers the window into tb->xwin where the starts have moved since the last gather
int gather_window64(TinyBatch64 *tb)
{
    if (tb->xwin_valid) return 0;
    const size_t bytes = (size_t)tb->N * tb->nx * tb->bpad * sizeof(double);
    if (!tb->xwin)
    {
        HIP64(hipMalloc((void **)&tb->xwin, bytes));
        HIP64(hipMemsetAsync(tb->xwin, 0, bytes, 0));
    }
    HIP64(launch_gather_window64(tb->table, tb->xref_start, tb->xwin, tb->table_rows, tb->N, tb->nx, tb->batch, tb->bpad));
    tb->xwin_valid = true;
    return 0;
}
size_t rec_len(const TinyBatch64 *tb) { return mat_off(tb, 6) + tb->nx; }

// the per-instance settings records from the caller's arrays and, for the fields given as NULL, the batch's settings as they stand now
int rebuild_settings64(TinyBatch64 *tb)
{
    const size_t B = tb->batch;
    std::vector<InstSettings64> rec(B);
    const int batch_int[4] = {tb->max_iter, tb->check_termination, tb->en_state_bound, tb->en_input_bound};
    for (size_t b = 0; b < B; b++)
    {
        int v[4];
        for (int k = 0; k < 4; k++) v[k] = tb->ps_int[k].empty() ? batch_int[k] : tb->ps_int[k][b];
        rec[b] = InstSettings64{tb->ps_tol[0].empty() ? tb->abs_pri_tol : tb->ps_tol[0][b], tb->ps_tol[1].empty() ? tb->abs_dua_tol : tb->ps_tol[1][b], v[0], v[1], v[2], v[3]};
        tb->ps_max_iter = b && tb->ps_max_iter > v[0] ? tb->ps_max_iter : v[0];
        tb->ps_min_iter = b && tb->ps_min_iter < v[0] ? tb->ps_min_iter : v[0];
    }
    HIP64(hipSetDevice(tb->device));
    HIP64(hipDeviceSynchronize()); // a launch still reading the records may be in flight
    if (!tb->ps_rec) HIP64(hipMalloc((void **)&tb->ps_rec, B * sizeof(InstSettings64)));
    HIP64(hipMemcpy(tb->ps_rec, rec.data(), B * sizeof(InstSettings64), hipMemcpyHostToDevice));
    return 0;
}

// ---- what a call launches: resolved ONCE per call by resolve_plan64() and read by everything that names, prepares or launches (DESIGN.md 5.6 has the
// table).  No other function looks at kernel_choice, the lists of instantiated classes, the capacities, max_iter or TINYMPC_F64_LOOP.
enum class Family64 { Thread, Rows };         // one thread per instance (state in HBM, any N); sixteen lanes per instance (state in registers)
enum class Body64 { Unrolled, Cap32, Cap64 }; // Rows only, which instantiation of admm_f64_rows_kernel: N compiled in; any N <= 32; any N <= 64
enum class Loop64 { None, Sequence, OnChip }; // one solve; a run as launches per step; a run in one launch
struct Plan64
{
    Family64 family = Family64::Thread;
    Body64 body = Body64::Unrolled;
    bool pm = false; // per-instance models: the ",pm" instantiations
    bool ps = false; // per-instance settings: the ",ps" instantiations (never with pm)
    Loop64 loop = Loop64::None;
    bool sim = false; // the plant step is the simulated one: a plant is set, the call passes w or asks for x_traj — or pm: the simulated kernels are the
                      // ones that take a matrix pair per instance, here the instance's own model.  Any other call enqueues what it always has
};
struct Call64
{
    enum Kind { StepFn, Solve, Run } kind; // one of the six step functions; one solve (with or without a plant step behind it); a closed-loop run
    bool w = false, x_traj = false;        // the caller passed a disturbance / asks for the state trajectory
    bool log = false;                      // ... asks for the per-step solver log (tiny_batch64_mpc_run_log)
};

// Reads the handle and changes nothing.  The two refusals a resolution can meet are the step functions' under models and per-instance settings together
// with models: tiny_batch64_select_kernel refuses the sixteen lanes where the class has none, so a stored choice can always be served.
int resolve_plan64(const TinyBatch64 *tb, const Call64 &call, Plan64 *out)
{
    if (tb->pm && tb->ps)
        return fail64(TINY_BATCH_EUNSUPPORTED, "per-instance settings together with per-instance models: no kernel reads both records "
                                               "(tiny_batch64_clear_instance_settings() or tiny_batch64_clear_models())");
    if (call.kind == Call64::StepFn && tb->pm)
        return fail64(TINY_BATCH_EUNSUPPORTED, "the six single-function step kernels read one shared model: not available with per-instance models (tiny_batch64_clear_models())");
    Plan64 p;
    const bool rows = tb->kernel_choice == 2 || (tb->kernel_choice == 0 && rows_supported(tb->nx, tb->nu, tb->N));
    if (rows && call.kind != Call64::StepFn) // (the step kernels are thread-per-instance ones)
    {
        p.family = Family64::Rows;
        p.body = rows_unrolled(tb->nx, tb->nu, tb->N) ? Body64::Unrolled : tb->N <= 32 ? Body64::Cap32 : Body64::Cap64;
    }
    p.pm = tb->pm;
    p.ps = tb->ps;
    p.sim = tb->plant_mode != 0 || call.w || call.x_traj || tb->pm;
    if (call.kind == Call64::Run)
    {
        // on chip where the sixteen-lane kernel holds [p ; d] in registers (the unrolled instantiations and the capacity-32 body).  max_iter <= 0 (tiny_solve
        // sets status and iter only) is left to the launch sequence.  Developer aid, read on every resolution: TINYMPC_F64_LOOP=sequence sends every run
        // through the launch sequence (tools/closed_loop64_time.py times the two against each other over the same solve kernel, in one process).
        const char *force = getenv("TINYMPC_F64_LOOP");
        // A run that asks for the per-step solver log is a launch sequence as well: the on-chip loops do not log (their instruction streams are pinned,
        // tests/test_isa_sim64.py), the sequence copies iter[] / status[] behind each solve of the same solve kernel, with the same bits.
        // With per-instance settings the budget that counts is the smallest (an instance without one writes status and iter only: the sequence's solve
        // kernel does that), and the on-chip loop is the nominal one: a plant, w or x_traj make the run a sequence.
        const bool budget = (tb->ps ? tb->ps_min_iter : tb->max_iter) >= 1, ps_nominal = !tb->ps || !(tb->plant_mode || call.w || call.x_traj);
        const bool on_chip = p.family == Family64::Rows && p.body != Body64::Cap64 && budget && ps_nominal && !(force && !strcmp(force, "sequence")) && !call.log;
        p.loop = on_chip ? Loop64::OnChip : Loop64::Sequence;
    }
    *out = p;
    return 0;
}

// every name, printed from the plan.  ",sim" says that a plant is set and nothing else: a run that passes w / x_traj without one, and every run with
// models, takes the simulated family under the name ",mpc" (only the call knows the former; tests assert the latter)
const char *name_of(const TinyBatch64 *tb, const Plan64 &p, char (&nm)[64])
{
    char body[16] = "";
    if (p.family == Family64::Rows && p.body == Body64::Unrolled) snprintf(body, sizeof body, ",%d", tb->N);
    else if (p.family == Family64::Rows) snprintf(body, sizeof body, ",n<=%d", p.body == Body64::Cap32 ? 32 : 64);
    const char *const loop = p.loop != Loop64::OnChip ? "" : tb->plant_mode ? ",sim" : ",mpc";
    snprintf(nm, sizeof nm, "%s<%d,%d%s%s%s>", p.family == Family64::Rows ? "rows64" : "thread64", tb->nx, tb->nu, body, loop, p.pm ? ",pm" : p.ps ? ",ps" : "");
    return nm;
}

// How every call begins: its plan and its launch arguments.  The on-chip closed loop reads a window reference from the table itself; every other launch
// reads it gathered
int prepare64(TinyBatch64 *tb, const Call64 &call, Plan64 &plan, Params64 &P)
{
    TRY64(resolve_plan64(tb, call, &plan));
    if (!(tb->pm || (tb->have_cache && tb->have_dyn)) || !tb->have_settings)
        return fail64(TINY_BATCH_ENOTREADY, "set_cache, set_dynamics (or set_models) and set_settings must be called first");
    CHECK64(tb->in_stride[1] == tb->in_stride[2] && tb->in_stride[3] == tb->in_stride[4], "min and max bounds must both be shared or both be per-instance");
    HIP64(hipSetDevice(tb->device));
    if (tb->mats_dirty)
    {
        HIP64(hipMemcpy(tb->mats, tb->hm.data(), tb->hm.size() * sizeof(double), hipMemcpyHostToDevice));
        const std::vector<double> g = pack_row_gains(tb);
        if (!tb->row_gains) HIP64(hipMalloc((void **)&tb->row_gains, g.size() * sizeof(double)));
        HIP64(hipMemcpy(tb->row_gains, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
        tb->mats_dirty = false;
    }
    P.nx = tb->nx; P.nu = tb->nu; P.N = tb->N; P.batch = tb->batch; P.bpad = tb->bpad;
    P.rho = tb->rho; P.abs_pri_tol = tb->abs_pri_tol; P.abs_dua_tol = tb->abs_dua_tol;
    P.max_iter = plan.ps ? tb->ps_max_iter : tb->max_iter; P.check_termination = tb->check_termination;
    P.en_state_bound = tb->en_state_bound; P.en_input_bound = tb->en_input_bound;
    for (int id = 0; id < TINY_ARR_COUNT; id++) P.arr[id] = tb->arr[id];
    P.xref = tb->in[0]; P.xmin = tb->in[1]; P.xmax = tb->in[2]; P.umin = tb->in[3]; P.umax = tb->in[4];
    P.xref_stride = tb->in_stride[0]; P.xb_stride = tb->in_stride[1]; P.ub_stride = tb->in_stride[3];
    P.mats = tb->mats; P.res = tb->res; P.status = tb->status; P.iter = tb->iter; P.n_unsolved = tb->n_unsolved;
    if (tb->table_rows > 0 && plan.loop != Loop64::OnChip)
    {
        TRY64(gather_window64(tb));
        P.xref = tb->xwin; P.xref_stride = tb->bpad;
    }
    return 0;
}

// one of the six step functions over the whole batch
int run_step64(TinyBatch64 *tb, int fn, int *conv_dev)
{
    CHECK64(tb, "NULL handle");
    Plan64 plan;
    Params64 P;
    TRY64(prepare64(tb, Call64{Call64::StepFn}, plan, P));
    // update_slack and termination_condition are the two that read a setting: with per-instance settings their ",ps" forms; the other four keep their kernels
    if (plan.ps && (fn == F64_UPDATE_SLACK || fn == F64_TERMINATION_CONDITION)) HIP64(launch_f64_step_ps(fn, tb->nx, tb->nu, P, conv_dev, Settings64{tb->ps_rec}));
    else HIP64(launch_f64_step(fn, tb->nx, tb->nu, P, conv_dev));
    HIP64(hipDeviceSynchronize());
    return 0;
}

// The solve kernel of a plan, on the null stream: the one place a solve kernel is launched.  L: the loop arguments of a run on chip (L->mpc_steps solves);
// d_w / d_x: such a run's device copies of w and x_traj or NULL
int launch_solve64(TinyBatch64 *tb, const Plan64 &plan, const Params64 &P, const Mpc64 *L = nullptr, const double *d_w = nullptr, double *d_x = nullptr)
{
    const int nx = tb->nx, nu = tb->nu, N = tb->N;
    const bool rows = plan.family == Family64::Rows;
    const Models64 M{tb->pm_rec, rec_len(tb), tb->pm_rho};
    // a run on chip takes the simulated family with models (whose plant is at least every instance's own) and where the kernel's plant step, which one
    // step never reaches, is to be a simulated one; the MPC instantiation serves the rest
    if (plan.loop == Loop64::OnChip && (plan.pm || (plan.sim && L->mpc_steps > 1)))
    {
        const Sim64 S{tb->plant_mode ? tb->plant_rows : nullptr, tb->plant_mode == 2 ? (size_t)(nx + nu) * 16 : 0, d_w, d_x};
        if (plan.pm) HIP64(launch_rows64_loop_pm(nx, nu, N, P, *L, S, M));
        else HIP64(launch_rows64_sim(nx, nu, N, P, tb->row_gains, *L, S));
    }
    else if (plan.pm)
    {
        if (rows) HIP64(launch_f64_rows_pm(nx, nu, N, P, M));
        else HIP64(launch_f64_thread_pm(nx, nu, P, M));
    }
    else if (plan.ps)
    {
        const Settings64 ST{tb->ps_rec};
        if (plan.loop == Loop64::OnChip) HIP64(launch_rows64_loop_ps(nx, nu, N, P, tb->row_gains, *L, ST));
        else if (rows) HIP64(launch_f64_rows_ps(nx, nu, N, P, tb->row_gains, ST));
        else HIP64(launch_f64_thread_ps(nx, nu, P, ST));
    }
    else if (rows) HIP64(launch_f64_rows(nx, nu, N, P, tb->row_gains, plan.loop == Loop64::OnChip ? L : nullptr));
    else HIP64(launch_f64_thread(nx, nu, P));
    return 0;
}

// The plant step behind a solve of a plan: the one place a plant kernel is launched.  d_w / d_x / d_u0: this step's device rows of w, x_traj and u0_traj or
// NULL; start: the window starts to slide by adv, or NULL.  Simulated: against the handle's plant, else the model's matrices, with models every
// instance's own, inside its record.  Else the model's: behind a lone solve the kernel that records and slides nothing, in a run the one that does
int enqueue_plant64(TinyBatch64 *tb, const Plan64 &plan, const double *d_w, double *d_x, double *d_u0, int *start, int adv)
{
    double *const X = tb->arr[TINY_ARR_X];
    const double *const U = tb->arr[TINY_ARR_U];
    if (plan.sim)
    {
        const bool per = tb->plant_mode == 2, own = tb->pm && !tb->plant_mode;
        const double *const model = own ? tb->pm_rec : tb->mats;
        const double *A = tb->plant_mode ? tb->plant_A : model + mat_off(tb, 4), *Bm = tb->plant_mode ? tb->plant_B : model + mat_off(tb, 5);
        const PlantSim64 a{X, U, A, Bm, own ? rec_len(tb) : per ? (size_t)tb->nx * tb->nx : 0, own ? rec_len(tb) : per ? (size_t)tb->nx * tb->nu : 0,
                           tb->batch, tb->bpad, d_w, d_x, d_u0, start, adv};
        HIP64(launch_plant64_sim(tb->nx, tb->nu, a));
    }
    else if (plan.loop == Loop64::None) HIP64(launch_plant64(tb->nx, tb->nu, X, U, tb->mats, tb->batch, tb->bpad)); // quadrotor_hovering.cpp:110-111
    else HIP64(launch_plant64_run(tb->nx, tb->nu, X, U, tb->mats, tb->batch, tb->bpad, d_u0, start, adv));
    return 0;
}

// tiny_solve over the batch: 1 where some instance is left unsolved
int solve64(TinyBatch64 *tb, const Call64 &call, Plan64 &plan)
{
    Params64 P;
    TRY64(prepare64(tb, call, plan, P));
    HIP64(hipMemset(tb->n_unsolved, 0, sizeof(int)));
    TRY64(launch_solve64(tb, plan, P));
    int n = 0;
    HIP64(hipMemcpy(&n, tb->n_unsolved, sizeof(int), hipMemcpyDeviceToHost));
    return n > 0 ? 1 : 0;
}

// a device buffer kept on the handle between calls: re-allocated only when it has to grow
template <typename T>
int grow64(T **buf, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    (void)hipFree(*buf); *buf = nullptr; *cap = 0;
    HIP64(hipMalloc((void **)buf, need * sizeof(T)));
    *cap = need;
    return 0;
}
} // namespace

extern "C"
{

int tiny_batch64_create(TinyBatch64 **out, int nx, int nu, int N, int batch, int device)
{
    CHECK64(out, "NULL out pointer");
    *out = nullptr;
    CHECK64(nx >= 1 && nu >= 1 && N >= 2 && batch >= 1, "need nx>=1, nu>=1, N>=2, batch>=1 (got %d,%d,%d,%d)", nx, nu, N, batch);
    bool have = false;
#define TINY_F64_HAVE(NX, NU) have = have || (nx == NX && nu == NU);
    TINY_FOR_EACH_F64DIMS(TINY_F64_HAVE)
    if (!have)
        return fail64(TINY_BATCH_EUNSUPPORTED, "no fp64 kernel instantiation for nx=%d nu=%d (add it to TINY_FOR_EACH_F64DIMS)", nx, nu);
    int ndev = 0;
    HIP64(hipGetDeviceCount(&ndev));
    CHECK64(device >= 0 && device < ndev, "device %d out of range (have %d)", device, ndev);
    HIP64(hipSetDevice(device));
    TinyBatch64 *tb = new TinyBatch64();
    tb->nx = nx; tb->nu = nu; tb->N = N; tb->batch = batch; tb->device = device;
    tb->bpad = (batch + WAVE64 - 1) / WAVE64 * WAVE64;
    auto zalloc = [&](void **p, size_t bytes) {
        if (hipMalloc(p, bytes) != hipSuccess) return false;
        return hipMemset(*p, 0, bytes) == hipSuccess;
    };
    bool ok = true;
    for (int id = 0; id < TINY_ARR_COUNT && ok; id++)
        ok = zalloc((void **)&tb->arr[id], steps_of(tb, id) * dim_of(tb, id) * tb->bpad * sizeof(double));
    ok = ok && zalloc((void **)&tb->res, 4 * (size_t)tb->bpad * sizeof(double)) && zalloc((void **)&tb->status, tb->bpad * sizeof(int)) &&
         zalloc((void **)&tb->iter, tb->bpad * sizeof(int)) && zalloc((void **)&tb->n_unsolved, sizeof(int)) &&
         zalloc((void **)&tb->staging, (size_t)batch * N * (nx > nu ? nx : nu) * sizeof(double)) &&
         zalloc((void **)&tb->mats, (mat_off(tb, 6) + nx) * sizeof(double));
    // inputs that were never set read as zero (the reference's zero-initialised members)
    for (int w = 0; w < 5 && ok; w++)
        ok = zalloc((void **)&tb->in[w], (size_t)(w < 3 ? N * nx : (N - 1) * nu) * sizeof(double));
    if (!ok || hipDeviceSynchronize() != hipSuccess)
    {
        tiny_batch64_destroy(tb);
        return fail64(TINY_BATCH_EHIP, "device allocation failed");
    }
    tb->hm.assign(mat_off(tb, 6) + nx, 0.0);
    *out = tb;
    return 0;
}

void tiny_batch64_destroy(TinyBatch64 *tb)
{
    if (!tb) return;
    (void)hipSetDevice(tb->device);
    for (int id = 0; id < TINY_ARR_COUNT; id++) (void)hipFree(tb->arr[id]);
    for (int w = 0; w < 5; w++) (void)hipFree(tb->in[w]);
    (void)hipFree(tb->mats); (void)hipFree(tb->res); (void)hipFree(tb->staging); (void)hipFree(tb->row_gains);
    (void)hipFree(tb->status); (void)hipFree(tb->iter); (void)hipFree(tb->n_unsolved);
    (void)hipFree(tb->table); (void)hipFree(tb->xwin); (void)hipFree(tb->u0_traj); (void)hipFree(tb->xref_start);
    (void)hipFree(tb->log_iter); (void)hipFree(tb->log_status);
    (void)hipFree(tb->plant_A); (void)hipFree(tb->plant_B); (void)hipFree(tb->plant_rows); (void)hipFree(tb->sim_w); (void)hipFree(tb->sim_x);
    (void)hipFree(tb->pm_rec); (void)hipFree(tb->pm_rho); (void)hipFree(tb->ps_rec);
    delete tb;
}

int tiny_batch64_set_cache(TinyBatch64 *tb, double rho, const double *Kinf, const double *Pinf, const double *Quu_inv, const double *AmBKt)
{
    CHECK64(tb && Kinf && Pinf && Quu_inv && AmBKt, "NULL argument");
    const size_t nx = tb->nx, nu = tb->nu;
    tb->rho = rho;
    std::copy(Kinf, Kinf + nu * nx, tb->hm.begin() + mat_off(tb, 0));
    std::copy(Pinf, Pinf + nx * nx, tb->hm.begin() + mat_off(tb, 1));
    std::copy(Quu_inv, Quu_inv + nu * nu, tb->hm.begin() + mat_off(tb, 2));
    std::copy(AmBKt, AmBKt + nx * nx, tb->hm.begin() + mat_off(tb, 3));
    tb->have_cache = true; tb->mats_dirty = true;
    return 0;
}

int tiny_batch64_set_dynamics(TinyBatch64 *tb, const double *Adyn, const double *Bdyn, const double *Q)
{
    CHECK64(tb && Adyn && Bdyn && Q, "NULL argument");
    const size_t nx = tb->nx, nu = tb->nu;
    std::copy(Adyn, Adyn + nx * nx, tb->hm.begin() + mat_off(tb, 4));
    std::copy(Bdyn, Bdyn + nx * nu, tb->hm.begin() + mat_off(tb, 5));
    std::copy(Q, Q + nx, tb->hm.begin() + mat_off(tb, 6));
    tb->have_dyn = true; tb->mats_dirty = true;
    return 0;
}

int tiny_batch64_set_settings(TinyBatch64 *tb, double abs_pri_tol, double abs_dua_tol, int max_iter, int check_termination,
                              int en_state_bound, int en_input_bound)
{
    CHECK64(tb, "NULL handle");
    CHECK64(check_termination >= 1, "check_termination must be >= 1 (the reference computes iter %% check_termination, admm.cpp:93)");
    tb->abs_pri_tol = abs_pri_tol; tb->abs_dua_tol = abs_dua_tol; tb->max_iter = max_iter; tb->check_termination = check_termination;
    tb->en_state_bound = en_state_bound; tb->en_input_bound = en_input_bound;
    tb->have_settings = true;
    if (tb->ps) TRY64(rebuild_settings64(tb)); // the fields given as NULL move with the batch's
    return 0;
}

// ---- per-instance settings ---------------------------------------------------------------------------------------------------
int tiny_batch64_set_instance_settings(TinyBatch64 *tb, const double *abs_pri_tol, const double *abs_dua_tol, const int *max_iter, const int *check_termination,
                                       const int *en_state_bound, const int *en_input_bound)
{
    CHECK64(tb, "NULL handle");
    if (!tb->have_settings) return fail64(TINY_BATCH_ENOTREADY, "tiny_batch64_set_settings must be called first: a NULL field keeps the batch's value");
    const size_t B = tb->batch;
    if (check_termination)
        for (size_t b = 0; b < B; b++)
            CHECK64(check_termination[b] >= 1, "check_termination[%zu] = %d: must be >= 1 (the reference computes iter %% check_termination, admm.cpp:93)", b,
                    check_termination[b]);
    const double *const tol[2] = {abs_pri_tol, abs_dua_tol};
    const int *const ints[4] = {max_iter, check_termination, en_state_bound, en_input_bound};
    for (int k = 0; k < 2; k++) tb->ps_tol[k].assign(tol[k], tol[k] ? tol[k] + B : tol[k]);
    for (int k = 0; k < 4; k++) tb->ps_int[k].assign(ints[k], ints[k] ? ints[k] + B : ints[k]);
    TRY64(rebuild_settings64(tb));
    tb->ps = true;
    return 0;
}

int tiny_batch64_clear_instance_settings(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    if (!tb->ps) return 0;
    HIP64(hipSetDevice(tb->device));
    HIP64(hipDeviceSynchronize()); // a launch still reading the records may be in flight
    (void)hipFree(tb->ps_rec); tb->ps_rec = nullptr;
    for (auto &v : tb->ps_tol) v.clear();
    for (auto &v : tb->ps_int) v.clear();
    tb->ps = false;
    return 0;
}

int tiny_batch64_settings_per_instance(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    return tb->ps ? 1 : 0;
}

int tiny_batch64_set_x0(TinyBatch64 *tb, const double *x0)
{
    CHECK64(tb && x0, "NULL argument");
    HIP64(hipSetDevice(tb->device));
    HIP64(hipMemcpy(tb->staging, x0, (size_t)tb->batch * tb->nx * sizeof(double), hipMemcpyHostToDevice));
    // [B][1][nx] -> step 0 of x
    HIP64(launch_pack64(tb->staging, tb->arr[TINY_ARR_X], tb->batch, 1, tb->nx, tb->bpad, 0, 1));
    HIP64(hipDeviceSynchronize());
    return 0;
}

int tiny_batch64_set_xref(TinyBatch64 *tb, const double *xref, int shared) { return set_input(tb, 0, xref, shared); }
int tiny_batch64_set_xmin(TinyBatch64 *tb, const double *v, int shared) { return set_input(tb, 1, v, shared); }
int tiny_batch64_set_xmax(TinyBatch64 *tb, const double *v, int shared) { return set_input(tb, 2, v, shared); }
int tiny_batch64_set_umin(TinyBatch64 *tb, const double *v, int shared) { return set_input(tb, 3, v, shared); }
int tiny_batch64_set_umax(TinyBatch64 *tb, const double *v, int shared) { return set_input(tb, 4, v, shared); }

int tiny_batch64_reset_dual_variables(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    HIP64(hipSetDevice(tb->device));
    HIP64(hipMemset(tb->arr[TINY_ARR_Y], 0, (size_t)(tb->N - 1) * tb->nu * tb->bpad * sizeof(double)));
    HIP64(hipMemset(tb->arr[TINY_ARR_G], 0, (size_t)tb->N * tb->nx * tb->bpad * sizeof(double)));
    return 0;
}

int tiny_batch64_forward_pass(TinyBatch64 *tb) { return run_step64(tb, F64_FORWARD_PASS, nullptr); }
int tiny_batch64_update_slack(TinyBatch64 *tb) { return run_step64(tb, F64_UPDATE_SLACK, nullptr); }
int tiny_batch64_update_dual(TinyBatch64 *tb) { return run_step64(tb, F64_UPDATE_DUAL, nullptr); }
int tiny_batch64_update_linear_cost(TinyBatch64 *tb) { return run_step64(tb, F64_UPDATE_LINEAR_COST, nullptr); }
int tiny_batch64_backward_pass_grad(TinyBatch64 *tb) { return run_step64(tb, F64_BACKWARD_PASS_GRAD, nullptr); }
int tiny_batch64_termination_condition(TinyBatch64 *tb, int *converged)
{
    CHECK64(tb && converged, "NULL argument");
    HIP64(hipSetDevice(tb->device));
    Scratch64<int> dev;
    HIP64(dev.alloc(tb->bpad));
    TRY64(run_step64(tb, F64_TERMINATION_CONDITION, dev.p));
    HIP64(hipMemcpy(converged, dev.p, (size_t)tb->batch * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int tiny_batch64_solve(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    Plan64 plan;
    return solve64(tb, Call64{Call64::Solve}, plan);
}

// tiny_batch64_mpc_step / _mpc_step_sim: with no plant and no disturbance the launches tiny_batch64_mpc_step has always made
static int mpc_step64(TinyBatch64 *tb, const double *w)
{
    CHECK64(tb, "NULL handle");
    Plan64 plan;
    TRY64(resolve_plan64(tb, Call64{Call64::Solve, w != nullptr}, &plan)); // a refused combination touches nothing
    TRY64(tiny_batch64_reset_dual_variables(tb)); // quadrotor_hovering.cpp:100-101
    const int rc = solve64(tb, Call64{Call64::Solve, w != nullptr}, plan); // :104
    if (rc < 0) return rc;
    if (w)
    {
        const size_t row = (size_t)tb->batch * tb->nx;
        TRY64(grow64(&tb->sim_w, &tb->sim_w_cap, row));
        HIP64(hipMemcpy(tb->sim_w, w, row * sizeof(double), hipMemcpyHostToDevice));
    }
    TRY64(enqueue_plant64(tb, plan, w ? tb->sim_w : nullptr, nullptr, nullptr, nullptr, 0));
    return rc;
}
int tiny_batch64_mpc_step(TinyBatch64 *tb) { return mpc_step64(tb, nullptr); }
int tiny_batch64_mpc_step_sim(TinyBatch64 *tb, const double *w) { return mpc_step64(tb, w); }

int tiny_batch64_clear_plant(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    if (!tb->plant_mode) return 0;
    HIP64(hipSetDevice(tb->device));
    HIP64(hipDeviceSynchronize()); // a plant kernel still reading the matrices may be in flight
    for (double **p : {&tb->plant_A, &tb->plant_B, &tb->plant_rows}) { (void)hipFree(*p); *p = nullptr; }
    tb->plant_mode = 0;
    return 0;
}

int tiny_batch64_set_plant(TinyBatch64 *tb, const double *A, const double *B, int shared)
{
    CHECK64(tb && A && B, "NULL argument");
    HIP64(hipSetDevice(tb->device));
    TRY64(tiny_batch64_clear_plant(tb)); // releases the previous copies
    const size_t nx = tb->nx, nu = tb->nu, cnt = shared ? 1 : (size_t)tb->batch, rl = (nx + nu) * 16;
    // the sixteen-lane kernel's form: entry (k, r) of [A | B] at k * 16 + r, lane r of a row reads 128 contiguous bytes per column with its row
    std::vector<double> packed;
    if (nx + nu <= 16)
    {
        packed.assign(cnt * rl, 0.0);
        for (size_t c = 0; c < cnt; c++)
            for (size_t r = 0; r < nx; r++)
            {
                for (size_t k = 0; k < nx; k++) packed[c * rl + k * 16 + r] = A[c * nx * nx + k * nx + r];
                for (size_t m = 0; m < nu; m++) packed[c * rl + (nx + m) * 16 + r] = B[c * nx * nu + m * nx + r];
            }
    }
    // the handle takes the copies once all of them stand: a failure leaves it without a plant
    Scratch64<double> dA, dB, dRows;
    HIP64(dA.upload(A, cnt * nx * nx));
    HIP64(dB.upload(B, cnt * nx * nu));
    if (!packed.empty()) HIP64(dRows.upload(packed.data(), packed.size()));
    tb->plant_A = dA.release(); tb->plant_B = dB.release(); tb->plant_rows = dRows.release();
    tb->plant_mode = shared ? 1 : 2;
    return 0;
}

int tiny_batch64_plant_mode(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    return tb->plant_mode;
}

// ---- per-instance models ----------------------------------------------------------------------------------------------------
static int install_models64(TinyBatch64 *tb, const double *const d[8], int q_plus_rho)
{
    if (!tb->pm_rec) HIP64(hipMalloc((void **)&tb->pm_rec, (size_t)tb->batch * rec_len(tb) * sizeof(double)));
    if (!tb->pm_rho) HIP64(hipMalloc((void **)&tb->pm_rho, (size_t)tb->batch * sizeof(double)));
    HIP64(launch_models64_gather(d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], tb->pm_rec, tb->pm_rho, tb->batch, tb->nx, tb->nu, q_plus_rho));
    tb->pm = true;
    return 0;
}

int tiny_batch64_set_models_device(TinyBatch64 *tb, const double *d_rho, const double *d_Kinf, const double *d_Pinf, const double *d_Quu_inv,
                                   const double *d_AmBKt, const double *d_Adyn, const double *d_Bdyn, const double *d_Q)
{
    CHECK64(tb && d_rho && d_Kinf && d_Pinf && d_Quu_inv && d_AmBKt && d_Adyn && d_Bdyn && d_Q, "NULL argument");
    HIP64(hipSetDevice(tb->device));
    const double *const d[8] = {d_rho, d_Kinf, d_Pinf, d_Quu_inv, d_AmBKt, d_Adyn, d_Bdyn, d_Q};
    return install_models64(tb, d, 0);
}

int tiny_batch64_set_models(TinyBatch64 *tb, const double *rho, const double *Kinf, const double *Pinf, const double *Quu_inv, const double *AmBKt,
                            const double *Adyn, const double *Bdyn, const double *Q)
{
    CHECK64(tb && rho && Kinf && Pinf && Quu_inv && AmBKt && Adyn && Bdyn && Q, "NULL argument");
    HIP64(hipSetDevice(tb->device));
    const size_t B = tb->batch, nx = tb->nx, nu = tb->nu;
    const double *const src[8] = {rho, Kinf, Pinf, Quu_inv, AmBKt, Adyn, Bdyn, Q};
    const size_t sz[8] = {B, B * nu * nx, B * nx * nx, B * nu * nu, B * nx * nx, B * nx * nx, B * nx * nu, B * nx};
    size_t total = 0;
    for (size_t z : sz) total += z;
    Scratch64<double> buf;
    HIP64(buf.alloc(total));
    const double *d[8];
    size_t o = 0;
    for (int k = 0; k < 8; k++)
    {
        HIP64(hipMemcpy(buf.p + o, src[k], sz[k] * sizeof(double), hipMemcpyHostToDevice));
        d[k] = buf.p + o;
        o += sz[k];
    }
    TRY64(install_models64(tb, d, 0));
    HIP64(hipDeviceSynchronize()); // the gather has read the buffer
    return 0;
}

int tiny_batch64_clear_models(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    if (!tb->pm) return 0;
    HIP64(hipSetDevice(tb->device));
    HIP64(hipDeviceSynchronize()); // a launch still reading the records may be in flight
    for (double **p : {&tb->pm_rec, &tb->pm_rho}) { (void)hipFree(*p); *p = nullptr; }
    tb->pm = false;
    return 0;
}

int tiny_batch64_models_per_instance(TinyBatch64 *tb)
{
    CHECK64(tb, "NULL handle");
    return tb->pm ? 1 : 0;
}

int tiny_batch64_set_systems(TinyBatch64 *tb, const double *A, const double *B, const double *Q, const double *R, const double *rho, int *iters)
{
    CHECK64(tb && A && B && Q && R && rho, "NULL argument");
    HIP64(hipSetDevice(tb->device));
    const size_t Bn = tb->batch, nx = tb->nx, nu = tb->nu;
    // inputs A | B | Q | R | rho, then the outputs Kinf | Pinf | Quu_inv | AmBKt: all of it stays fp64 from the recursion into the records
    const size_t sz[9] = {Bn * nx * nx, Bn * nx * nu, Bn * nx, Bn * nu, Bn, Bn * nu * nx, Bn * nx * nx, Bn * nu * nu, Bn * nx * nx};
    const double *const in[5] = {A, B, Q, R, rho};
    size_t nd = 0;
    for (size_t z : sz) nd += z;
    Scratch64<double> d;
    Scratch64<int> it;
    HIP64(d.alloc(nd));
    HIP64(it.alloc(Bn));
    double *dp[9];
    size_t o = 0;
    for (int k = 0; k < 9; k++) { dp[k] = d.p + o; o += sz[k]; }
    for (int k = 0; k < 5; k++) HIP64(hipMemcpy(dp[k], in[k], sz[k] * sizeof(double), hipMemcpyHostToDevice));
    const int nfail = tiny_batch_riccati_device(tb->nx, tb->nu, tb->batch, dp[0], dp[1], dp[2], dp[3], dp[4], dp[5], dp[6], dp[7], dp[8], nullptr, it.p, nullptr);
    if (nfail < 0) return fail64(nfail, "tiny_batch64_set_systems: %s", tiny_batch_last_error());
    if (iters) HIP64(hipMemcpy(iters, it.p, Bn * sizeof(int), hipMemcpyDeviceToHost));
    if (nfail > 0)
        return fail64(TINY_BATCH_EINVAL, "tiny_batch64_set_systems: the Riccati recursion is singular for %d of %zu systems (iters = -1); models unchanged", nfail, Bn);
    const double *const m[8] = {dp[4], dp[5], dp[6], dp[7], dp[8], dp[0], dp[1], dp[2]}; // rho, the cache, Adyn = A, Bdyn = B, Q (+ rho in the gather)
    TRY64(install_models64(tb, m, 1));
    HIP64(hipDeviceSynchronize()); // the gather has read the buffer
    return 0;
}

int tiny_batch64_set_xref_window(TinyBatch64 *tb, const double *table, int rows, const int *start)
{
    CHECK64(tb && table && start, "NULL argument");
    CHECK64(rows >= tb->N, "trajectory table has %d rows, need at least N=%d", rows, tb->N);
    for (int b = 0; b < tb->batch; b++)
        CHECK64(start[b] >= 0 && start[b] + tb->N <= rows, "window start[%d]=%d out of range for %d rows, N=%d", b, start[b], rows, tb->N);
    HIP64(hipSetDevice(tb->device));
    if (tb->table && tb->table_rows != rows) { (void)hipFree(tb->table); tb->table = nullptr; }
    tb->table_rows = 0;
    if (!tb->table) HIP64(hipMalloc((void **)&tb->table, (size_t)rows * tb->nx * sizeof(double)));
    if (!tb->xref_start)
    {
        HIP64(hipMalloc((void **)&tb->xref_start, (size_t)tb->bpad * sizeof(int)));
        HIP64(hipMemset(tb->xref_start, 0, (size_t)tb->bpad * sizeof(int)));
    }
    HIP64(hipMemcpy(tb->table, table, (size_t)rows * tb->nx * sizeof(double), hipMemcpyHostToDevice));
    HIP64(hipMemcpy(tb->xref_start, start, (size_t)tb->batch * sizeof(int), hipMemcpyHostToDevice));
    tb->table_rows = rows;
    tb->xwin_valid = false;
    return 0;
}

int tiny_batch64_get_xref_start(TinyBatch64 *tb, int *start)
{
    CHECK64(tb && start, "NULL argument");
    CHECK64(tb->table_rows > 0, "no window reference is set (tiny_batch64_set_xref_window)");
    HIP64(hipSetDevice(tb->device));
    HIP64(hipMemcpy(start, tb->xref_start, (size_t)tb->batch * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

int tiny_batch64_mpc_run_log(TinyBatch64 *tb, int steps, int window_advance, const double *w_host, double *u0_traj_host, double *x_traj_host, int *iter_log_host,
                             int *status_log_host)
{
    CHECK64(tb, "NULL handle");
    CHECK64(steps >= 1, "steps must be >= 1 (got %d)", steps);
    CHECK64(window_advance >= 0, "window_advance must be >= 0 (got %d)", window_advance);
    const bool window = tb->table_rows > 0;
    const int adv = window ? window_advance : 0; // without a window there is nothing to slide
    CHECK64((long long)steps * adv + tb->table_rows + tb->N < 0x7fffffffLL, "steps * window_advance = %lld overflows the window start", (long long)steps * adv);
    Plan64 plan;
    Params64 P;
    TRY64(prepare64(tb, Call64{Call64::Run, w_host != nullptr, x_traj_host != nullptr, iter_log_host != nullptr || status_log_host != nullptr}, plan, P));
    const size_t row_len = (size_t)tb->batch * tb->nu, need = u0_traj_host ? (size_t)steps * row_len : 0;
    const size_t xrow = (size_t)tb->batch * tb->nx, need_w = w_host ? (size_t)steps * xrow : 0, need_x = x_traj_host ? (size_t)steps * xrow : 0;
    TRY64(grow64(&tb->u0_traj, &tb->u0_traj_cap, need));
    TRY64(grow64(&tb->sim_w, &tb->sim_w_cap, need_w));
    TRY64(grow64(&tb->sim_x, &tb->sim_x_cap, need_x));
    // the per-step solver log: neither the plan nor the plant step knows of it
    const size_t lrow = (size_t)tb->batch, need_l = (size_t)steps * lrow;
    TRY64(grow64(&tb->log_iter, &tb->log_iter_cap, iter_log_host ? need_l : 0));
    TRY64(grow64(&tb->log_status, &tb->log_status_cap, status_log_host ? need_l : 0));
    int *const d_il = iter_log_host ? tb->log_iter : nullptr, *const d_sl = status_log_host ? tb->log_status : nullptr;
    // row k of the logs: iter[] / status[] as the solve before it left them
    auto log_row = [&](int k) {
        if (d_il) HIP64(hipMemcpyAsync(d_il + (size_t)k * lrow, tb->iter, lrow * sizeof(int), hipMemcpyDeviceToDevice, 0));
        if (d_sl) HIP64(hipMemcpyAsync(d_sl + (size_t)k * lrow, tb->status, lrow * sizeof(int), hipMemcpyDeviceToDevice, 0));
        return 0;
    };
    if (w_host) HIP64(hipMemcpy(tb->sim_w, w_host, need_w * sizeof(double), hipMemcpyHostToDevice));
    double *const traj = u0_traj_host ? tb->u0_traj : nullptr;
    const double *const d_w = w_host ? tb->sim_w : nullptr;
    double *const d_x = x_traj_host ? tb->sim_x : nullptr;
    // step k's plant step, with its rows of w and the two trajectories
    auto plant = [&](int k) {
        return enqueue_plant64(tb, plan, d_w ? d_w + (size_t)k * xrow : nullptr, d_x ? d_x + (size_t)k * xrow : nullptr, traj ? traj + (size_t)k * row_len : nullptr,
                               window ? tb->xref_start : nullptr, adv);
    };
    if (plan.loop == Loop64::OnChip)
    {
        // all solves and the plant steps between them in one launch; the last plant step (the same plant, its own rows of w and x_traj), u.col(0) of the
        // last solve and the last slide follow.  y and g of the workspace are zero from the first solve on: the kernel starts from that without reading them
        const Mpc64 L{steps, adv, tb->table_rows, tb->table, tb->xref_start, traj};
        HIP64(hipMemsetAsync(tb->n_unsolved, 0, sizeof(int), 0));
        TRY64(launch_solve64(tb, plan, P, &L, d_w, d_x));
        TRY64(plant(steps - 1));
    }
    else
        for (int k = 0; k < steps; k++)
        {
            if (window) TRY64(gather_window64(tb));
            HIP64(hipMemsetAsync(tb->arr[TINY_ARR_Y], 0, (size_t)(tb->N - 1) * tb->nu * tb->bpad * sizeof(double), 0));
            HIP64(hipMemsetAsync(tb->arr[TINY_ARR_G], 0, (size_t)tb->N * tb->nx * tb->bpad * sizeof(double), 0));
            HIP64(hipMemsetAsync(tb->n_unsolved, 0, sizeof(int), 0));
            TRY64(launch_solve64(tb, plan, P));
            TRY64(log_row(k));
            TRY64(plant(k));
            if (adv) tb->xwin_valid = false;
        }
    if (adv) tb->xwin_valid = false;
    int n = 0;
    HIP64(hipMemcpy(&n, tb->n_unsolved, sizeof(int), hipMemcpyDeviceToHost)); // the only host synchronisation of the run
    if (u0_traj_host) HIP64(hipMemcpy(u0_traj_host, tb->u0_traj, need * sizeof(double), hipMemcpyDeviceToHost));
    if (x_traj_host) HIP64(hipMemcpy(x_traj_host, tb->sim_x, need_x * sizeof(double), hipMemcpyDeviceToHost));
    if (iter_log_host) HIP64(hipMemcpy(iter_log_host, d_il, need_l * sizeof(int), hipMemcpyDeviceToHost));
    if (status_log_host) HIP64(hipMemcpy(status_log_host, d_sl, need_l * sizeof(int), hipMemcpyDeviceToHost));
    return n > 0 ? 1 : 0;
}

int tiny_batch64_mpc_run_sim(TinyBatch64 *tb, int steps, int window_advance, const double *w_host, double *u0_traj_host, double *x_traj_host)
{
    return tiny_batch64_mpc_run_log(tb, steps, window_advance, w_host, u0_traj_host, x_traj_host, nullptr, nullptr);
}

int tiny_batch64_mpc_run_traj(TinyBatch64 *tb, int steps, int adv, double *u0_traj_host) { return tiny_batch64_mpc_run_sim(tb, steps, adv, nullptr, u0_traj_host, nullptr); }
int tiny_batch64_mpc_run(TinyBatch64 *tb, int steps, int window_advance) { return tiny_batch64_mpc_run_sim(tb, steps, window_advance, nullptr, nullptr, nullptr); }

int tiny_batch64_get_first_columns(TinyBatch64 *tb, double *x0, double *u0)
{
    CHECK64(tb, "NULL handle");
    HIP64(hipSetDevice(tb->device));
    for (int w = 0; w < 2; w++)
    {
        double *dst = w ? u0 : x0;
        if (!dst) continue;
        const int dim = w ? tb->nu : tb->nx;
        HIP64(launch_unpack64(tb->arr[w ? TINY_ARR_U : TINY_ARR_X], tb->staging, tb->batch, 1, dim, tb->bpad));
        HIP64(hipMemcpy(dst, tb->staging, (size_t)tb->batch * dim * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

int tiny_batch64_select_kernel(TinyBatch64 *tb, int which)
{
    CHECK64(tb, "NULL handle");
    CHECK64(which >= 0 && which <= 2, "kernel must be 0 (auto), 1 (one thread per instance) or 2 (sixteen lanes per instance)");
    if (which == 2 && !rows_supported(tb->nx, tb->nu, tb->N))
        return fail64(TINY_BATCH_EUNSUPPORTED, "the sixteen-lane fp64 kernel has no instantiation for nx=%d nu=%d N=%d", tb->nx, tb->nu, tb->N);
    tb->kernel_choice = which;
    return 0;
}

static const char *plan_name64(TinyBatch64 *tb, Call64::Kind kind, char (&nm)[64])
{
    if (!tb) return "";
    Plan64 plan;
    if (resolve_plan64(tb, Call64{kind}, &plan) < 0) return "unsupported"; // per-instance settings with models: tiny_batch64_last_error() says so
    return name_of(tb, plan, nm);
}
const char *tiny_batch64_kernel_name(TinyBatch64 *tb)
{
    static thread_local char nm[64];
    return plan_name64(tb, Call64::Solve, nm);
}
// the kernel a run launches: the solve kernel's name where the run is a launch sequence.  It knows the handle alone, not a call's w / x_traj
const char *tiny_batch64_closed_loop_kernel_name(TinyBatch64 *tb)
{
    static thread_local char nm[64];
    return plan_name64(tb, Call64::Run, nm);
}

int tiny_batch64_set_array(TinyBatch64 *tb, int id, const double *src)
{
    CHECK64(tb && src, "NULL argument");
    CHECK64(id >= 0 && id < TINY_ARR_COUNT, "bad array id %d", id);
    HIP64(hipSetDevice(tb->device));
    const int steps = (int)steps_of(tb, id), dim = dim_of(tb, id);
    HIP64(hipMemcpy(tb->staging, src, (size_t)tb->batch * steps * dim * sizeof(double), hipMemcpyHostToDevice));
    HIP64(launch_pack64(tb->staging, tb->arr[id], tb->batch, steps, dim, tb->bpad, 0, steps));
    HIP64(hipDeviceSynchronize());
    return 0;
}

int tiny_batch64_get_array(TinyBatch64 *tb, int id, double *dst)
{
    CHECK64(tb && dst, "NULL argument");
    CHECK64(id >= 0 && id < TINY_ARR_COUNT, "bad array id %d", id);
    HIP64(hipSetDevice(tb->device));
    const int steps = (int)steps_of(tb, id), dim = dim_of(tb, id);
    HIP64(launch_unpack64(tb->arr[id], tb->staging, tb->batch, steps, dim, tb->bpad));
    HIP64(hipMemcpy(dst, tb->staging, (size_t)tb->batch * steps * dim * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int tiny_batch64_get_status(TinyBatch64 *tb, int *iter, int *status, double *residuals)
{
    CHECK64(tb, "NULL handle");
    HIP64(hipSetDevice(tb->device));
    if (iter) HIP64(hipMemcpy(iter, tb->iter, (size_t)tb->batch * sizeof(int), hipMemcpyDeviceToHost));
    if (status) HIP64(hipMemcpy(status, tb->status, (size_t)tb->batch * sizeof(int), hipMemcpyDeviceToHost));
    if (residuals)
    {
        std::vector<double> tmp(4 * (size_t)tb->bpad);
        HIP64(hipMemcpy(tmp.data(), tb->res, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int b = 0; b < tb->batch; b++)
            for (int k = 0; k < 4; k++) residuals[4 * (size_t)b + k] = tmp[(size_t)k * tb->bpad + b];
    }
    return 0;
}

int tiny_batch64_set_status(TinyBatch64 *tb, const int *iter, const int *status, const double *residuals)
{
    CHECK64(tb, "NULL handle");
    HIP64(hipSetDevice(tb->device));
    if (iter) HIP64(hipMemcpy(tb->iter, iter, (size_t)tb->batch * sizeof(int), hipMemcpyHostToDevice));
    if (status) HIP64(hipMemcpy(tb->status, status, (size_t)tb->batch * sizeof(int), hipMemcpyHostToDevice));
    if (residuals)
    {
        std::vector<double> tmp(4 * (size_t)tb->bpad, 0.0);
        for (int b = 0; b < tb->batch; b++)
            for (int k = 0; k < 4; k++) tmp[(size_t)k * tb->bpad + b] = residuals[4 * (size_t)b + k];
        HIP64(hipMemcpy(tb->res, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return 0;
}

const char *tiny_batch64_last_error(void) { return g_err64.c_str(); }

} // extern "C"
