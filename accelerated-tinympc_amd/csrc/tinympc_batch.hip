// tinympc_batch.hip — host side of the C-ABI declared in include/tinympc_batch.h:
// device-resident batched workspace, gain packing and kernel dispatch.  Host code only: the solver kernels live in
// admm_rowlane.hip (state on chip), admm_stream.hip (state in HBM) and their siblings, the helper kernels (layout
// conversion, plant step, model records, guard zones) in batch_helpers.hip, each behind a typed launcher.
//
// There is deliberately NO CPU fallback in this library: every entry point that computes
// launches a HIP kernel and reports HIP failures as TINY_BATCH_EHIP.
#include "../../include/tinympc_batch.h"
#include "batch_helpers.h"
#include "tinympc_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

using namespace tinympc;

namespace
{

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do                                                                                             \
    {                                                                                              \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(TINY_BATCH_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define TRY(expr)                 \
    do                            \
    {                             \
        int rc_ = (expr);         \
        if (rc_) return rc_;      \
    } while (0)
#define CHECK_TB(tb) \
    if (!(tb)) return fail(TINY_BATCH_EINVAL, "%s: NULL TinyBatch handle", __func__)
#define CHECK_PTR(p) \
    if (!(p)) return fail(TINY_BATCH_EINVAL, "%s: NULL pointer argument '%s'", __func__, #p)

// ---------------------------------------------------------------------------------------------
// Debug guard zones ("a debug bounds-checked kernel variant" — GPU AddressSanitizer does not exist on this pool).
// With tiny_batch_debug_guards(1) every device allocation of this library is made kGuard floats larger at both ends; the guards are filled
// with a quiet-NaN pattern.  An out-of-bounds WRITE of any kernel then lands in a guard and tiny_batch_debug_check() counts the
// damaged words; an out-of-bounds READ returns NaN, which no parity test survives.  It is a mode of the same library — the kernels
// are the shipped ones, unchanged — used by tests/test_parity_gpu.py::test_debug_guard_zones_stay_intact over every kernel family.
// (kGuard, the floats on each side, and the fill and count kernels: batch_helpers.h)
// ---------------------------------------------------------------------------------------------
std::mutex g_guard_mu;
std::map<void *, size_t> g_guarded;          // user pointer -> user bytes
bool g_guards_on = false;

hipError_t guarded_malloc(void **out, size_t bytes)
{
    if (!g_guards_on) return hipMalloc(out, bytes);
    const size_t user = (bytes + 3) / 4 * 4;
    char *raw = nullptr;
    hipError_t e = hipMalloc((void **)&raw, user + 2 * kGuard * sizeof(float));
    if (e != hipSuccess) return e;
    e = launch_guard_fill((unsigned *)raw, kGuard, nullptr);
    if (e == hipSuccess) e = launch_guard_fill((unsigned *)(raw + kGuard * sizeof(float) + user), kGuard, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { (void)hipFree(raw); return e; }
    *out = raw + kGuard * sizeof(float);
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guarded[*out] = user;
    return hipSuccess;
}
hipError_t guarded_free(void *p)
{
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        auto it = g_guarded.find(p);
        if (it != g_guarded.end())
        {
            g_guarded.erase(it);
            return hipFree((char *)p - kGuard * sizeof(float));
        }
    }
    return hipFree(p);
}

enum { VAR_AUTO = 0, VAR_STREAM = 1, VAR_ROW_EXACT = 2, VAR_ROW_FAST = 3, VAR_GENERIC = 4 }; // 4: admm_generic.hip, exact arithmetic for any eligible class

// The solve kernels; kKernelTraits below says everything the host code needs to know about each of them.
enum class Kernel { Rowlane, Rowloop, Rowstream, Wavestream, Quadlane, Tile16, Waveres, Tile48, Stream, Generic };

// pair index of each work array in the ROW layout: x,u | q,r | p,d | v,z | vnew,znew | g,y
const int kPairOf[TINY_ARR_COUNT] = {0, 0, 1, 1, 2, 2, 3, 4, 3, 4, 5, 5};
bool is_xfam(int id)
{
    return id == TINY_ARR_X || id == TINY_ARR_Q || id == TINY_ARR_P || id == TINY_ARR_V || id == TINY_ARR_VNEW ||
           id == TINY_ARR_G;
}

struct InputArr // canonical copy of a caller-provided input, host layout [cnt][steps][dim] on the device
{
    float *dev = nullptr;
    bool shared = true, set = false;
    std::vector<float> host; // kept only when shared (small)
};

} // namespace

// ---------------------------------------------------------------------------------------------
struct TinyBatch
{
    int nx = 0, nu = 0, N = 0, batch = 0, device = 0;
    int NXC = 0, NUC = 0, ntiles = 0, bpad4 = 0;
    int rw = 16; // lanes per instance-step of the ROW layout
    bool row_dims_ok = false, tile_dims_ok = false, rowmath_ok = false, rowloop_ok = false, wave_ok = false, quad_ok = false;
    bool tile16_ok = false; // admm_tile16.hip has an instantiation for (nx, nu, N)
    bool waveres_ok = false; // admm_waveres.hip serves (nx, nu, N): wave class with N <= 50
    bool tile48_ok = false;  // admm_tile48.hip does (nx = 32, nu = 16, N = 50: sixteen instances per workgroup on the matrix cores)
    bool generic_ok = false; // admm_generic.hip: exact arithmetic with run-time dimensions (nx, nu each <= 4 or a multiple of 4)
    float *gen_mats = nullptr; // its gains: Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q, column-major
    int *conv_dev = nullptr; // [batch] result of termination_condition
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr; // created by tiny_batch_group_solve / mpc_run for handles left on the null stream
    hipGraphExec_t graph_exec = nullptr; // tiny_batch_mpc_run_async: captured (solve + plant) x steps
    std::string graph_sig;
    // problem class
    bool have_cache = false, have_dyn = false, have_settings = false, gains_dirty = true;
    float rho = 0.f;
    std::vector<float> Kinf, Pinf, Quu_inv, AmBKt, Adyn, Bdyn, Q;
    float abs_pri_tol = 0.f, abs_dua_tol = 0.f;
    int max_iter = 0, check_termination = 1, en_state_bound = 0, en_input_bound = 0;
    // work arrays: exactly one layout is allocated at a time
    int layout = LAYOUT_TILE;
    float *arr[TINY_ARR_COUNT] = {}; // TILE
    float *pair[6] = {};             // ROW
    size_t xfam_floats = 0, ufam_floats = 0, pair_floats = 0;
    // caller inputs (canonical) and their per-layout derived forms
    InputArr in_xref, in_bnd[4]; // bnd: xmin, xmax, umin, umax
    // the two terms the reference ships commented out (admm.cpp:20, :79); tiny_batch_set_optional_terms
    bool en_uref = false, en_d2p = false, have_rcost = false;
    std::vector<float> Rcost, coeff_d2p; // R [nu], coeff_d2p [nx x nu] column-major
    InputArr in_uref;                    // [batch or 1][N-1][nu]
    float *r_uref = nullptr;             // ROW derived: [batch_pad4 or 1][N][rw], Uref on the u rows
    const int *order_dev = nullptr;      // caller-owned dispatch order of the instance groups (tiny_batch_set_dispatch_order_device)
    int dispatch_mode = -1;              // tiny_batch_set_dispatch: 0 in index order, 1 longest first by the predicted iteration count, -1 (default) automatic:
                                         // longest first for a launch that starts from a reset workspace (dispatch_effective)
    float *u0_stage = nullptr;           // [batch][nu] staging of u.col(0) for the peer copy of tiny_batch_group_gather_u0
    float *key_buf = nullptr;            // [groups] predictor of dispatch_order.hip
    int *order_buf = nullptr;            // [groups] its sorted order
    bool derived_dirty[2] = {true, true};
    float *t_xref = nullptr, *t_bnd[4] = {};              // TILE derived
    float *r_xref = nullptr, *r_bounds = nullptr;         // ROW derived
    float *r_bounds_img = nullptr, *r_xref_img = nullptr; // tile images of the two tables when they go through the rings of admm_tile16_pi.hip
    size_t r_bounds_img_n = 0, r_xref_img_n = 0;
    int *rows_vary_dev = nullptr;                         // [2] rows_vary_kernel's answer for the per-instance ROW tables ...
    unsigned rows_vary = 3u;                              // ... bit 0: bounds, bit 1: reference (set = changes along the horizon)
    int *zero_ties_dev = nullptr;                         // bounds_table_kernel's answer for the per-instance ROW table ...
    bool zero_ties = false;                               // ... and the handle's flag: the ROW bounds table holds an enabled pair with such a zero (zero_tie_bound)
    size_t r_xref_n = 0, r_bounds_n = 0, r_uref_n = 0;    // their allocated sizes in floats (sized_buffer)
    int graph_captures = 0;                               // closed-loop graphs captured so far (tiny_batch_debug_graph_captures)
    int n_cu = 256;                                       // compute units of the handle's device
    int tile_queue = -1;                                  // tiny_batch_set_tile_queue: -1 automatic, 0 plain counter, k every k-th wave from the short end
    int tile_grouping = -1;                               // tiny_batch_set_tile_grouping: -1 automatic, 0 off, 1 tiles formed from instances of one window start
    int *tile_map = nullptr;                              // [16 ceil(batch/16)] tile16's instance map (dispatch_order.hip); allocated once: the address is in captured launches
    bool tile_map_dirty = true;                           // xref_start[] has changed since the map was built
    int tile_map_builds = 0;
    bool last_grouped = false;                            // the most recent solve launch formed its tiles through the map
    float *tab_tile = nullptr, *tab_row = nullptr;        // trajectory table in both forms
    float *tab_row_h = nullptr;                           // ... and [rows][16] binary16 for fp16 storage
    int table_rows = 0;
    int *xref_start = nullptr;
    int xref_mode = 0;
    float *res = nullptr;
    int *status = nullptr, *iter = nullptr, *n_unsolved = nullptr;
    float *opnd = nullptr, *qvec = nullptr;               // TILE gains (MFMA operands)
    float *mats_exact = nullptr, *mats_fast = nullptr;    // ROW gains
    float *dA = nullptr, *dB = nullptr;                   // column-major copies for the plant step
    float *x0buf = nullptr;                               // [B][nx] current state (closed loop)
    float *staging = nullptr;                             // host-layout staging
    size_t staging_floats = 0;
    bool duals_zero_pending = false;
    bool cold_pending = false;
    bool x0_zero_pending = false; // reset_workspace(): x.col(0) and x0buf read as zero until a set_x0 overwrites them
    int variant = VAR_AUTO;
    std::optional<Kernel> row_family_forced; // tiny_batch_set_row_kernel (empty: automatic)
    int last_dispatch = 0;        // what the most recent solve launch did: 0 index order, 1 predicted longest first, 2 the caller's order, 3 longest first by the previous solve's counts
    bool iter_history = false;    // iter[] holds the counts of a solve of THIS workspace's instances (not a reset, not an upload): the history order's key
    // per-instance models (tiny_batch_set_models): one record per instance in the run-time-dimension kernel's form ([batch][pm_gen_floats]: Kinf | Pinf |
    // Quu_inv | AmBKt | Adyn | Bdyn | Q, which is also what the plant step reads), rho [batch]; the 16-lane kernel's two forms of the gain rows
    // ([batch][pm_row_floats], [0] exact, [1] fma) are packed from the records on the device when a launch first needs one, and so are the two wave
    // kernels' ([batch][pm_wave_floats]: the same rows at row width 64 — 33 KB per instance of the nx = 32 class and form)
    bool pm = false;
    float *pm_src = nullptr, *pm_rho = nullptr, *pm_row[2] = {}, *pm_wave[2] = {};
    bool pm_row_dirty[2] = {true, true}, pm_wave_dirty[2] = {true, true};
    // the simulated plant of the closed-loop calls (tiny_batch_set_plant): 0 the model's own Adyn / Bdyn, 1 one shared plant, 2 one per instance.  Column-major
    // copies for the plant kernel ([1 or batch][nx*nx], [1 or batch][nx*nu]) and, where the class has a 16-lane kernel, the rows of [A | B] packed for its
    // on-chip loop ([1 or batch][plant_row_floats]: SimParams)
    int plant_mode = 0;
    float *plant_A = nullptr, *plant_B = nullptr, *plant_rows = nullptr;
    float *sim_stage[5] = {};      // tiny_batch_mpc_run_log's device copies of w, u0_traj, x_traj, iter_log, status_log: kept between calls (sized_buffer), so that their
    size_t sim_stage_n[5] = {};    // addresses, which the captured graph bakes in, hold from call to call
    // per-instance settings (tiny_batch_set_instance_settings).  The caller's arrays as given (empty: NULL, the field follows tiny_batch_set_settings); the records
    // the ps kernels read ([bpad4] InstSettings: admm_rowlane_ps.hip, admm_steps_ps.hip) and, where the bound flags differ between instances, the two flag
    // arrays the bounds table is built from ([2][batch]); the largest and smallest budget; the flags' value where they are uniform over the batch
    bool ps = false;
    std::vector<float> ps_pri, ps_dua;
    std::vector<int> ps_max_iter, ps_check, ps_en_state, ps_en_input;
    InstSettings *ps_dev = nullptr;
    int *ps_flags_dev = nullptr;
    int ps_budget_max = 0, ps_budget_min = 0;
    bool ps_flags_vary = false;
    int ps_en_state_all = 0, ps_en_input_all = 0;
    bool h16 = false; // ROW-layout arrays, Xref and bounds stored as IEEE binary16 (tiny_batch_set_storage)
    bool dual32 = false; // with h16: the duals pair gy IS fp32 right now (the state of the array)
    bool dual32_pref = false;   // tiny_batch_set_storage(tb, 16): fp32 duals wherever the kernel a call resolves to implements them, 16-bit duals elsewhere
    bool dual32_forced = false; // tiny_batch_set_storage_ex(tb, 16, 32): fp32 duals or TINY_BATCH_EUNSUPPORTED
    bool timing = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_valid = false;
    std::string name_buf[2]; // what tiny_batch_kernel_name() [0] / tiny_batch_closed_loop_kernel_name() [1] last returned; nothing else reads or writes them
};

namespace
{

// In ONE table, everything the host code needs to know about each solve kernel (enum class Kernel, in its order).
struct KernelTraits
{
    const char *name;      // what tiny_batch_kernel_name() prints up to the '<' ...
    bool name_has_N;       // ... whether N follows nx, nu (one instantiation per horizon) ...
    bool name_has_storage; // ... and ",h16" / ",h16d" the arithmetic (the kernels that implement fp16 storage)
    int layout;            // device layout of the work arrays
    bool fp32_duals;       // keeps the duals pair fp32 under fp16 storage (register-resident 16-lane and quad kernels)
    int order_unit_solve;  // what a longest-first dispatch order lists for a lone solve: 4 groups of four instances, 16 tiles of sixteen, 0 takes no order
    int order_unit_run;    // ... and for the on-chip closed-loop run
    bool onchip_mpc;       // runs all the MPC steps of tiny_batch_mpc_run_async inside one launch
    int row_kernel_number; // tiny_batch_set_row_kernel's public number (0: not a row kernel)
    bool TinyBatch::*has;  // the handle's flag "this class has an instantiation of it" (set by tiny_batch_create)
};
constexpr KernelTraits kKernelTraits[] = {
    /* Rowlane    */ {"rowlane", true, true, LAYOUT_ROW, true, 4, 4, true, 1, &TinyBatch::row_dims_ok},
    /* Rowloop    */ {"rowloop", false, true, LAYOUT_ROW, false, 4, 0, false, 2, &TinyBatch::rowloop_ok},
    /* Rowstream  */ {"rowstream", false, true, LAYOUT_ROW, false, 0, 0, false, 3, &TinyBatch::rowmath_ok},
    /* Wavestream */ {"wavestream", false, false, LAYOUT_ROW, false, 0, 0, false, 6, &TinyBatch::wave_ok},
    /* Quadlane   */ {"quadlane", true, true, LAYOUT_ROW, true, 0, 0, true, 4, &TinyBatch::quad_ok},
    /* Tile16     */ {"tile16", true, false, LAYOUT_ROW, false, 16, 16, true, 5, &TinyBatch::tile16_ok},
    /* Waveres    */ {"waveres", false, false, LAYOUT_ROW, false, 0, 0, false, 7, &TinyBatch::waveres_ok},
    /* Tile48     */ {"tile48", true, false, LAYOUT_ROW, false, 0, 0, false, 8, &TinyBatch::tile48_ok},
    /* Stream     */ {"stream", false, false, LAYOUT_TILE, false, 0, 0, false, 0, &TinyBatch::tile_dims_ok},
    /* Generic    */ {"generic", false, false, LAYOUT_TILE, false, 0, 0, false, 0, &TinyBatch::generic_ok},
};
constexpr const KernelTraits &traits(Kernel k) { return kKernelTraits[(int)k]; }

Geo geo(const TinyBatch *tb) { return Geo{tb->nx, tb->nu, tb->N, tb->NXC, tb->NUC, tb->rw}; }

int set_device(TinyBatch *tb)
{
    HIP_TRY(hipSetDevice(tb->device));
    return 0;
}

// a handle left on the null stream gets a stream of its own
int leave_null_stream(TinyBatch *tb)
{
    if (tb->stream) return 0;
    TRY(set_device(tb));
    HIP_TRY(hipStreamSynchronize(nullptr)); // work already queued on the null stream (uploads) comes first
    if (!tb->own_stream) HIP_TRY(hipStreamCreateWithFlags(&tb->own_stream, hipStreamNonBlocking));
    tb->stream = tb->own_stream;
    return 0;
}

int dev_alloc_zero(float **p, size_t nfloats)
{
    HIP_TRY(guarded_malloc((void **)p, nfloats * sizeof(float)));
    HIP_TRY(hipMemset(*p, 0, nfloats * sizeof(float)));
    // hipMemset of device memory is enqueued on the null stream and may return early; a handle on a non-blocking
    // stream would not be ordered behind it
    HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

// A derived input buffer of the ROW layout (reference, bounds table, Uref) is re-filled whenever its source changes; it is re-ALLOCATED only when its
// size does: its address is a kernel argument baked into the captured closed-loop graph, and `set_xref; mpc_run(k)` in a loop must replay one graph
// (round-3 advisor: with free + malloc per refill that held only while the allocator happened to return the same address)
int sized_buffer(float **p, size_t *have, size_t nfloats)
{
    if (*p && *have == nfloats) return 0;
    if (*p) { (void)guarded_free(*p); *p = nullptr; }
    *have = 0;
    TRY(dev_alloc_zero(p, nfloats));
    *have = nfloats;
    return 0;
}

float *work_ptr(TinyBatch *tb, int id) { return tb->layout == LAYOUT_ROW ? tb->pair[kPairOf[id]] : tb->arr[id]; }
int h16_of(const TinyBatch *tb, int layout) { return (tb->h16 && layout == LAYOUT_ROW) ? 1 : 0; }
// element type of one device array: the duals pair is fp32 under tiny_batch_set_storage_ex(16, 32)
int h16_at(const TinyBatch *tb, int layout, const float *arr) { return (h16_of(tb, layout) && !(tb->dual32 && arr == tb->pair[5])) ? 1 : 0; }

int alloc_layout(TinyBatch *tb, int layout)
{
    if (layout == LAYOUT_ROW)
    {
        for (int p = 0; p < 6; p++)
            if (!tb->pair[p]) TRY(dev_alloc_zero(&tb->pair[p], (tb->h16 && !(tb->dual32 && p == 5)) ? (tb->pair_floats + 1) / 2 : tb->pair_floats));
    }
    else
    {
        for (int id = 0; id < TINY_ARR_COUNT; id++)
            if (!tb->arr[id]) TRY(dev_alloc_zero(&tb->arr[id], is_xfam(id) ? tb->xfam_floats : tb->ufam_floats));
    }
    return 0;
}

void free_layout(TinyBatch *tb, int layout)
{
    if (layout == LAYOUT_ROW)
        for (int p = 0; p < 6; p++) { (void)guarded_free(tb->pair[p]); tb->pair[p] = nullptr; }
    else
        for (int id = 0; id < TINY_ARR_COUNT; id++) { (void)guarded_free(tb->arr[id]); tb->arr[id] = nullptr; }
}

// the copy kernels of batch_helpers.hip on the handle's stream, with its geometry and the element type of the array
int launch_pack(TinyBatch *tb, const float *src, float *dst, int layout, int fam, int nb, bool shared, int step0, int nsteps, float *mirror = nullptr)
{
    HIP_TRY(tinympc::launch_pack(src, dst, layout, geo(tb), fam, nb, shared ? 1 : 0, step0, nsteps, h16_at(tb, layout, dst), mirror, tb->stream));
    return 0;
}
int launch_unpack(TinyBatch *tb, const float *src, float *dst, int layout, int fam, int nb, int step0, int nsteps)
{
    HIP_TRY(tinympc::launch_unpack(src, dst, layout, geo(tb), fam, nb, step0, nsteps, h16_at(tb, layout, src), tb->stream));
    return 0;
}
int launch_zero(TinyBatch *tb, float *dst, int layout, int fam, int step0, int nsteps)
{
    HIP_TRY(tinympc::launch_zero(dst, layout, geo(tb), fam, tb->batch, step0, nsteps, h16_at(tb, layout, dst), tb->stream));
    return 0;
}

// reset_workspace() zeroes x.col(0) lazily too: the usual next call is set_x0, which overwrites all of it
int flush_x0_zero(TinyBatch *tb)
{
    if (!tb->x0_zero_pending) return 0;
    TRY(launch_zero(tb, work_ptr(tb, TINY_ARR_X), tb->layout, 0, 0, 1));
    HIP_TRY(hipMemsetAsync(tb->x0buf, 0, (size_t)tb->batch * tb->nx * sizeof(float), tb->stream));
    tb->x0_zero_pending = false;
    return 0;
}

// Materialise pending lazy resets (needed before anything other than a solve looks at the arrays).
int flush_pending(TinyBatch *tb)
{
    TRY(flush_x0_zero(tb));
    if (tb->cold_pending)
    {
        // every work array reads as zero after reset_workspace(), except x.col(0) which carries x0
        for (int id = 0; id < TINY_ARR_COUNT; id++)
        {
            const int fam = is_xfam(id) ? 0 : 1;
            const int steps = fam ? tb->N - 1 : tb->N;
            if (id == TINY_ARR_X) TRY(launch_zero(tb, work_ptr(tb, id), tb->layout, 0, 1, tb->N - 1));
            else TRY(launch_zero(tb, work_ptr(tb, id), tb->layout, fam, 0, steps));
        }
        HIP_TRY(hipMemsetAsync(tb->res, 0, (size_t)tb->batch * 4 * sizeof(float), tb->stream));
        HIP_TRY(hipMemsetAsync(tb->status, 0, (size_t)tb->batch * sizeof(int), tb->stream));
        HIP_TRY(hipMemsetAsync(tb->iter, 0, (size_t)tb->batch * sizeof(int), tb->stream));
        tb->cold_pending = false;
        tb->duals_zero_pending = false;
    }
    if (tb->duals_zero_pending)
    {
        TRY(launch_zero(tb, work_ptr(tb, TINY_ARR_Y), tb->layout, 1, 0, tb->N - 1));
        TRY(launch_zero(tb, work_ptr(tb, TINY_ARR_G), tb->layout, 0, 0, tb->N));
        tb->duals_zero_pending = false;
    }
    return 0;
}

// Move the twelve work arrays to another device layout (through the host-layout staging buffer, on the device).
int ensure_layout(TinyBatch *tb, int want)
{
    if (tb->layout == want) return 0;
    TRY(flush_pending(tb));
    const int from = tb->layout;
    TRY(alloc_layout(tb, want));
    for (int id = 0; id < TINY_ARR_COUNT; id++)
    {
        const int fam = is_xfam(id) ? 0 : 1, steps = fam ? tb->N - 1 : tb->N;
        const float *src = from == LAYOUT_ROW ? tb->pair[kPairOf[id]] : tb->arr[id];
        float *dst = want == LAYOUT_ROW ? tb->pair[kPairOf[id]] : tb->arr[id];
        TRY(launch_unpack(tb, src, tb->staging, from, fam, tb->batch, 0, steps));
        TRY(launch_pack(tb, tb->staging, dst, want, fam, tb->batch, false, 0, steps));
    }
    HIP_TRY(hipStreamSynchronize(tb->stream));
    free_layout(tb, from);
    tb->layout = want;
    return 0;
}

// upload a host array ([batch][nsteps][dim]) into steps [step0, ...) of a work array of the current layout
int upload_work(TinyBatch *tb, const float *host, int id, int step0, int nsteps)
{
    const int fam = is_xfam(id) ? 0 : 1;
    const size_t n = (size_t)tb->batch * nsteps * (fam ? tb->nu : tb->nx);
    if (n > tb->staging_floats) return fail(TINY_BATCH_EINVAL, "internal: staging too small");
    HIP_TRY(hipMemcpyAsync(tb->staging, host, n * sizeof(float), hipMemcpyHostToDevice, tb->stream));
    TRY(launch_pack(tb, tb->staging, work_ptr(tb, id), tb->layout, fam, tb->batch, false, step0, nsteps));
    HIP_TRY(hipStreamSynchronize(tb->stream)); // staging and `host` are reusable on return
    return 0;
}

int download_work(TinyBatch *tb, int id, float *host, int step0, int nsteps)
{
    const int fam = is_xfam(id) ? 0 : 1;
    const size_t n = (size_t)tb->batch * nsteps * (fam ? tb->nu : tb->nx);
    if (n > tb->staging_floats) return fail(TINY_BATCH_EINVAL, "internal: staging too small");
    TRY(launch_unpack(tb, work_ptr(tb, id), tb->staging, tb->layout, fam, tb->batch, step0, nsteps));
    HIP_TRY(hipMemcpyAsync(host, tb->staging, n * sizeof(float), hipMemcpyDeviceToHost, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    return 0;
}

// `kind` = hipMemcpyDeviceToDevice: `src` is resident on the handle's device; no host copy is kept (only the bounds are ever read on the host) and the
// call does not wait for the stream
int store_input(TinyBatch *tb, InputArr &in, const float *src, bool shared, int steps, int dim, hipMemcpyKind kind = hipMemcpyHostToDevice)
{
    const size_t n = (size_t)(shared ? 1 : tb->batch) * steps * dim;
    const bool from_host = kind == hipMemcpyHostToDevice;
    if (in.dev && in.shared != shared) { (void)guarded_free(in.dev); in.dev = nullptr; }
    if (!in.dev) HIP_TRY(guarded_malloc((void **)&in.dev, n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(in.dev, src, n * sizeof(float), kind, tb->stream));
    if (from_host) HIP_TRY(hipStreamSynchronize(tb->stream));
    in.shared = shared;
    in.set = true;
    if (shared && from_host) in.host.assign(src, src + n);
    else in.host.clear();
    tb->derived_dirty[0] = tb->derived_dirty[1] = true; // (a captured closed-loop graph carries the mode in its signature)
    return 0;
}

// tiny_batch_set_dispatch(-1), the default: the predictor sweep and the sort pay where the iteration counts of a launch spread widely — a launch that starts from a
// reset workspace (65 536 tracking instances, wall time per solve: 2.20 -> 1.76 ms; 16 384: 0.82 -> 0.68) — and cost 2 - 4 % on warm-started steps (1.62 -> 1.66 ms)
// (second session of round 4) ... and a warm-started launch is ordered by what the predictor cannot see and the workspace already holds: the iteration counts of the
// PREVIOUS solve of the same instances (dispatch_order.hip, history order; mode 2): consecutive MPC steps are strongly correlated.  65 536 tracking instances,
// warm-started step: makespan 108 -> 78 iterations on the true counts (tests/fuzz/sim_history_dispatch.py).
constexpr int kDispatchMinGroups = 4096; // two rounds of waves on 256 CUs x 4 SIMDs x 2 waves
int dispatch_effective(const TinyBatch *tb)
{
    if (tb->dispatch_mode == 2) return tb->iter_history && !tb->cold_pending ? 2 : 0;
    if (tb->dispatch_mode >= 0) return tb->dispatch_mode;
    return tb->cold_pending ? 1 : (tb->iter_history ? 2 : 0);
}

// The settings as a solve of the whole batch sees them.  With per-instance settings (TinyBatch::ps): the largest budget bounds the launch's iteration loop
// (RowParams::max_iter), the smallest decides whether some instance runs no iteration; the bound flags are the arrays' common value where they have one
int budget_max(const TinyBatch *tb) { return tb->ps ? tb->ps_budget_max : tb->max_iter; }
int budget_min(const TinyBatch *tb) { return tb->ps ? tb->ps_budget_min : tb->max_iter; }
int state_bound_on(const TinyBatch *tb) { return tb->ps ? tb->ps_en_state_all : tb->en_state_bound; }
int input_bound_on(const TinyBatch *tb) { return tb->ps ? tb->ps_en_input_all : tb->en_input_bound; }

// one {lo, hi} table serves the batch: the bound inputs are shared, and so are the bound flags (per-instance settings can make them differ)
bool bounds_all_shared(const TinyBatch *tb)
{
    if (tb->ps && tb->ps_flags_vary) return false;
    for (int k = 0; k < 4; k++)
        if (tb->in_bnd[k].set && !tb->in_bnd[k].shared) return false;
    return true;
}

// ---- gains for the streaming kernel: MFMA A operands ---------------------------------------------
// Stacked vector s = [x ; u] in chunks of 4 rows; chunk ch, in-chunk row g  <->  x row 4ch+g (ch < NXC)
// or u row 4(ch-NXC)+g.  For v_mfma_f32_16x16x4_f32 the A operand of lane l is A[i = l&15][k = l>>4];
// the D row i of output tile t is held by lane group i>>2 in register i&3, which we DEFINE to be
// chunk 4t + (i&3), in-chunk row i>>2.  So:  A_{t,ch_in}[l] = M[ out(4t + (i&3), i>>2) ][ in(ch_in, l>>4) ].
struct RowRef { int fam; int idx; }; // fam 0 = x row, 1 = u row, -1 = padding

RowRef stacked_row(const TinyBatch *tb, int ch, int g)
{
    if (ch < tb->NXC) { int r = 4 * ch + g; return r < tb->nx ? RowRef{0, r} : RowRef{-1, 0}; }
    int r = 4 * (ch - tb->NXC) + g;
    return (ch < tb->NXC + tb->NUC && r < tb->nu) ? RowRef{1, r} : RowRef{-1, 0};
}

template <class F>
void pack_one(const TinyBatch *tb, std::vector<float> &out, int t_out, int ch_in, F entry)
{
    for (int l = 0; l < WAVE; l++)
    {
        int i = l & 15, kk = l >> 4;
        RowRef o = stacked_row(tb, 4 * t_out + (i & 3), i >> 2);
        RowRef in = stacked_row(tb, ch_in, kk);
        float v = 0.f;
        if (o.fam >= 0 && in.fam >= 0) v = entry(o, in);
        out.push_back(v);
    }
}

int upload_vec(TinyBatch *tb, float **dst, const std::vector<float> &v)
{
    if (!*dst) HIP_TRY(guarded_malloc((void **)dst, v.size() * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream)); // `v` may be a temporary
    return 0;
}

int pack_gains(TinyBatch *tb)
{
    const int nx = tb->nx, nu = tb->nu, NXC = tb->NXC, NUC = tb->NUC;
    const float *K = tb->Kinf.data(), *Pf = tb->Pinf.data(), *Qi = tb->Quu_inv.data(), *Am = tb->AmBKt.data();
    const float *A = tb->Adyn.data(), *B = tb->Bdyn.data();
    auto Kat = [&](int m, int k) { return K[k * nu + m]; };
    auto Aat = [&](int j, int k) { return A[k * nx + j]; };
    auto Bat = [&](int j, int m) { return B[m * nx + j]; };
    auto Amat = [&](int j, int k) { return Am[k * nx + j]; };
    auto Qiat = [&](int a, int b) { return Qi[b * nu + a]; };
    auto Pat = [&](int k, int j) { return Pf[j * nx + k]; };
    if (tb->tile_dims_ok)
    {
        const int NCH = NXC + NUC, NT = (NCH + 3) / 4, NTX = (NXC + 3) / 4, TU0 = NXC / 4;
        std::vector<float> o;
        for (int t = 0; t < NT; t++) // A1: fwd [A ; -K] * x
            for (int k = 0; k < NXC; k++)
                pack_one(tb, o, t, k, [&](RowRef out, RowRef in) {
                    if (in.fam != 0) return 0.f;
                    return out.fam == 0 ? Aat(out.idx, in.idx) : -Kat(out.idx, in.idx);
                });
        for (int t = 0; t < NTX; t++) // A2: fwd [B] * u
            for (int m = 0; m < NUC; m++)
                pack_one(tb, o, t, NXC + m, [&](RowRef out, RowRef in) { return (out.fam == 0 && in.fam == 1) ? Bat(out.idx, in.idx) : 0.f; });
        for (int t = 0; t < NT; t++) // A3: bwd [AmBKt ; B^T] * p
            for (int k = 0; k < NXC; k++)
                pack_one(tb, o, t, k, [&](RowRef out, RowRef in) {
                    if (in.fam != 0) return 0.f;
                    return out.fam == 0 ? Amat(out.idx, in.idx) : Bat(in.idx, out.idx);
                });
        for (int t = 0; t < NTX; t++) // A4: bwd [-K^T] * r
            for (int m = 0; m < NUC; m++)
                pack_one(tb, o, t, NXC + m, [&](RowRef out, RowRef in) { return (out.fam == 0 && in.fam == 1) ? -Kat(in.idx, out.idx) : 0.f; });
        for (int t = TU0; t < NT; t++) // A5: bwd [Quu_inv] * (B^T p + r)
            for (int m = 0; m < NUC; m++)
                pack_one(tb, o, t, NXC + m, [&](RowRef out, RowRef in) { return (out.fam == 1 && in.fam == 1) ? Qiat(out.idx, in.idx) : 0.f; });
        for (int t = 0; t < NTX; t++) // AP: terminal  p_j = -(sum_k Xref_k Pinf(k,j))
            for (int k = 0; k < NXC; k++)
                pack_one(tb, o, t, k, [&](RowRef out, RowRef in) { return (out.fam == 0 && in.fam == 0) ? -Pat(in.idx, out.idx) : 0.f; });
        std::vector<float> qv((size_t)WAVE * NXC, 0.f);
        for (int l = 0; l < WAVE; l++)
            for (int ch = 0; ch < NXC; ch++)
            {
                int r = 4 * ch + (l >> 4);
                if (r < nx) qv[(size_t)l * NXC + ch] = tb->Q[r];
            }
        TRY(upload_vec(tb, &tb->opnd, o));
        TRY(upload_vec(tb, &tb->qvec, qv));
    }
    if (tb->rowmath_ok || tb->wave_ok)
    {
        const int RW = tb->rw;
        // ---- gains for the rowlane kernel: [3nx + 2nu + 1][16], entry (reg, r) = the value lane r of a row holds.
        //   M1[k]  (k<nx): x rows A(r,k)      | u rows K(m,k) (exact: the kernel negates the SUM, like the reference) / -K(m,k) (fast)
        //   M2[m]  (m<nu): x rows B(r,m)      | u rows  0
        //   M3[k]  (k<nx): x rows AmBKt(r,k)  | u rows  B(k,m)          [= Bdyn^T]
        //   M45[m] (m<nu): x rows K(m,r) (exact) / -K(m,r) (fast)  | u rows  Quu_inv(mr,m)
        //   Q             : x rows Q(r)
        //   PT[k]  (k<nx): x rows Pinf(k,r)
        for (int fast = 0; fast < 2; fast++)
        {
            const float sg = fast ? -1.f : 1.f;
            const int nreg = 3 * nx + 3 * nu + 2; // ... + R (u rows) + coeff_d2p(r, m) (x rows): the optional terms
            std::vector<float> m((size_t)nreg * RW, 0.f);
            for (int r = 0; r < RW; r++)
            {
                const bool isx = r < nx, isu = r >= nx && r < nx + nu;
                const int mr = r - nx;
                for (int k = 0; k < nx; k++)
                {
                    m[(size_t)k * RW + r] = isx ? Aat(r, k) : (isu ? sg * Kat(mr, k) : 0.f); // u rows: K (exact), -K (fast)
                    m[(size_t)(nx + nu + k) * RW + r] = isx ? Amat(r, k) : (isu ? Bat(k, mr) : 0.f);
                    m[(size_t)(2 * nx + 2 * nu + 1 + k) * RW + r] = isx ? Pat(k, r) : 0.f;
                }
                for (int mm = 0; mm < nu; mm++)
                {
                    m[(size_t)(nx + mm) * RW + r] = isx ? Bat(r, mm) : 0.f;
                    m[(size_t)(2 * nx + nu + mm) * RW + r] = isx ? sg * Kat(mm, r) : (isu ? Qiat(mr, mm) : 0.f);
                }
                m[(size_t)(2 * nx + 2 * nu) * RW + r] = isx ? tb->Q[r] : 0.f;
                m[(size_t)(3 * nx + 2 * nu + 1) * RW + r] = (isu && tb->have_rcost) ? tb->Rcost[mr] : 0.f;
                for (int mm = 0; mm < nu; mm++)
                    m[(size_t)(3 * nx + 2 * nu + 2 + mm) * RW + r] = (isx && !tb->coeff_d2p.empty()) ? tb->coeff_d2p[(size_t)mm * nx + r] : 0.f;
            }
            TRY(upload_vec(tb, fast ? &tb->mats_fast : &tb->mats_exact, m));
        }
    }
    if (tb->generic_ok)
    {
        std::vector<float> gm;
        for (const std::vector<float> *m : {&tb->Kinf, &tb->Pinf, &tb->Quu_inv, &tb->AmBKt, &tb->Adyn, &tb->Bdyn, &tb->Q}) gm.insert(gm.end(), m->begin(), m->end());
        TRY(upload_vec(tb, &tb->gen_mats, gm));
    }
    if (!tb->dA) HIP_TRY(guarded_malloc((void **)&tb->dA, (size_t)nx * nx * sizeof(float)));
    if (!tb->dB) HIP_TRY(guarded_malloc((void **)&tb->dB, (size_t)nx * nu * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(tb->dA, A, (size_t)nx * nx * sizeof(float), hipMemcpyHostToDevice, tb->stream));
    HIP_TRY(hipMemcpyAsync(tb->dB, B, (size_t)nx * nu * sizeof(float), hipMemcpyHostToDevice, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    tb->gains_dirty = false;
    return 0;
}

// (re)build the layout-specific forms of the caller's inputs (Xref, bounds)
int prepare_inputs(TinyBatch *tb, int layout)
{
    if (!tb->derived_dirty[layout]) return 0;
    const int N = tb->N, nx = tb->nx, nu = tb->nu;
    if (layout == LAYOUT_TILE)
    {
        for (int k = 0; k < 4; k++)
        {
            const int fam = k < 2 ? 0 : 1;
            const size_t nf = fam ? tb->ufam_floats : tb->xfam_floats;
            if (!tb->t_bnd[k]) TRY(dev_alloc_zero(&tb->t_bnd[k], nf));
            const InputArr &in = tb->in_bnd[k];
            if (in.set) // shared inputs fill tile 0 only (tile stride 0 in the kernel)
                TRY(launch_pack(tb, in.dev, tb->t_bnd[k], LAYOUT_TILE, fam, in.shared ? TILE : tb->batch, in.shared, 0, fam ? N - 1 : N));
        }
        if (!tb->t_xref) TRY(dev_alloc_zero(&tb->t_xref, tb->xfam_floats));
        if (tb->in_xref.set)
            TRY(launch_pack(tb, tb->in_xref.dev, tb->t_xref, LAYOUT_TILE, 0, tb->in_xref.shared ? TILE : tb->batch, tb->in_xref.shared, 0, N));
    }
    else
    {
        // bounds table [N][16]{lo,hi}: +-inf where a bound is disabled or the row carries nothing; lo := min(lo, hi)
        // (min(hi, max(lo, t)) == med3(t, min(lo,hi), hi) for every t, also for the infeasible lo > hi case — as VALUES: the median breaks a tie between
        //  zeros of opposite sign the other way, which zero_ties records for the exact kernels; the reference's two compare-selects on the folded table
        //  return the reference's bits, lo > hi and lo = -0 under hi = +0 included)
        const float inf = std::numeric_limits<float>::infinity();
        const int RW = tb->rw;
        if (!bounds_all_shared(tb)) // per-instance bounds: [bpad4][N][rw]{lo,hi}, built on the device from the canonical inputs
        {
            const size_t nf = (size_t)tb->bpad4 * N * RW * 2;
            TRY(sized_buffer(&tb->r_bounds, &tb->r_bounds_n, tb->h16 ? (nf + 1) / 2 : nf));
            if (!tb->zero_ties_dev) TRY(dev_alloc_zero((float **)&tb->zero_ties_dev, 1));
            HIP_TRY(hipMemsetAsync(tb->zero_ties_dev, 0, sizeof(int), tb->stream));
            const InputArr *in = tb->in_bnd;
            const float *src[4];
            for (int k = 0; k < 4; k++) src[k] = in[k].set ? in[k].dev : nullptr;
            const int sh_x = (in[0].set ? in[0].shared : in[1].shared) ? 1 : 0, sh_u = (in[2].set ? in[2].shared : in[3].shared) ? 1 : 0;
            if (tb->ps && tb->ps_flags_vary) // the flags per instance (settings_helpers.hip); zero_ties sees the folded table as below
                HIP_TRY(launch_bounds_table_ps(src[0], src[1], src[2], src[3], sh_x, sh_u, tb->r_bounds, geo(tb), tb->batch, tb->ps_flags_dev,
                                               tb->ps_flags_dev + tb->batch, tb->h16 ? 1 : 0, tb->zero_ties_dev, tb->stream));
            else
                HIP_TRY(launch_bounds_table(src[0], src[1], src[2], src[3], sh_x, sh_u, tb->r_bounds, geo(tb), tb->batch, state_bound_on(tb),
                                            input_bound_on(tb), tb->h16 ? 1 : 0, tb->zero_ties_dev, tb->stream));
            int h = 0;
            HIP_TRY(hipMemcpyAsync(&h, tb->zero_ties_dev, sizeof h, hipMemcpyDeviceToHost, tb->stream));
            HIP_TRY(hipStreamSynchronize(tb->stream));
            tb->zero_ties = h != 0;
        }
        else
        {
        tb->zero_ties = false;
        std::vector<float> tab((size_t)N * RW * 2);
        for (int i = 0; i < N; i++)
            for (int r = 0; r < RW; r++)
            {
                float lo = -inf, hi = inf;
                if (r < nx && state_bound_on(tb))
                {
                    lo = tb->in_bnd[0].set ? tb->in_bnd[0].host[(size_t)i * nx + r] : 0.f;
                    hi = tb->in_bnd[1].set ? tb->in_bnd[1].host[(size_t)i * nx + r] : 0.f;
                }
                else if (r >= nx && r < nx + nu && i < N - 1 && input_bound_on(tb))
                {
                    lo = tb->in_bnd[2].set ? tb->in_bnd[2].host[(size_t)i * nu + (r - nx)] : 0.f;
                    hi = tb->in_bnd[3].set ? tb->in_bnd[3].host[(size_t)i * nu + (r - nx)] : 0.f;
                }
                lo = lo < hi ? lo : hi;
                tab[((size_t)i * RW + r) * 2 + 0] = lo;
                tab[((size_t)i * RW + r) * 2 + 1] = hi;
                if (tb->h16 ? zero_tie_bound((float)(_Float16)lo, (float)(_Float16)hi) : zero_tie_bound(lo, hi)) tb->zero_ties = true;
            }
        if (tb->h16) // same table in binary16 (bounds round to nearest; +-inf stays +-inf); half the floats
        {
            std::vector<_Float16> th(tab.size() + 1, (_Float16)0.f);
            for (size_t e = 0; e < tab.size(); e++) th[e] = (_Float16)tab[e];
            std::vector<float> packed((tab.size() + 1) / 2);
            std::memcpy(packed.data(), th.data(), packed.size() * sizeof(float));
            TRY(sized_buffer(&tb->r_bounds, &tb->r_bounds_n, packed.size()));
            TRY(upload_vec(tb, &tb->r_bounds, packed));
        }
        else
        {
            TRY(sized_buffer(&tb->r_bounds, &tb->r_bounds_n, tab.size()));
            TRY(upload_vec(tb, &tb->r_bounds, tab));
        }
        }
        const size_t nf = (size_t)(tb->in_xref.set && !tb->in_xref.shared ? tb->bpad4 : 1) * N * RW;
        TRY(sized_buffer(&tb->r_xref, &tb->r_xref_n, tb->h16 ? (nf + 1) / 2 : nf));
        if (!tb->in_xref.set) HIP_TRY(hipMemsetAsync(tb->r_xref, 0, tb->r_xref_n * sizeof(float), tb->stream)); // (a kept buffer of a reference since withdrawn)
        if (tb->in_xref.set)
            TRY(launch_pack(tb, tb->in_xref.dev, tb->r_xref, LAYOUT_ROW, 0, tb->in_xref.shared ? 1 : tb->batch, tb->in_xref.shared, 0, N));
        if (tb->in_uref.set) // Uref on the u rows of an [inst][N][rw] array of its own (row N-1 and the x rows stay zero)
        {
            const size_t nu_f = (size_t)(tb->in_uref.shared ? 1 : tb->bpad4) * N * RW;
            TRY(sized_buffer(&tb->r_uref, &tb->r_uref_n, tb->h16 ? (nu_f + 1) / 2 : nu_f));
            TRY(launch_pack(tb, tb->in_uref.dev, tb->r_uref, LAYOUT_ROW, 1, tb->in_uref.shared ? 1 : tb->batch, tb->in_uref.shared, 0, N - 1));
        }
        // per-instance tables of the class the sixteen-instances-per-wave kernel serves: do they change along the horizon? (one pass, at set time)
        tb->rows_vary = 3u;
        const bool xper = tb->xref_mode != 1 && tb->in_xref.set && !tb->in_xref.shared;
        if (tb->tile16_ok && !tb->ps && !tb->h16 && tb->rw == 16 && (!bounds_all_shared(tb) || xper)) // (per-instance settings never reach tile16)
        {
            if (!tb->rows_vary_dev) TRY(dev_alloc_zero((float **)&tb->rows_vary_dev, 2));
            HIP_TRY(hipMemsetAsync(tb->rows_vary_dev, 0, 2 * sizeof(int), tb->stream));
            HIP_TRY(launch_rows_vary(bounds_all_shared(tb) ? nullptr : reinterpret_cast<const float2 *>(tb->r_bounds), xper ? tb->r_xref : nullptr, tb->batch, N, nx,
                                     nu, tb->rows_vary_dev, tb->stream));
            int h[2] = {1, 1};
            HIP_TRY(hipMemcpyAsync(h, tb->rows_vary_dev, sizeof h, hipMemcpyDeviceToHost, tb->stream));
            HIP_TRY(hipStreamSynchronize(tb->stream));
            tb->rows_vary = (h[0] ? 1u : 0u) | (h[1] ? 2u : 0u);
            const long long ntl = (tb->batch + 15) / 16;
            if (!bounds_all_shared(tb) && (tb->rows_vary & 1u))
            {
                TRY(sized_buffer(&tb->r_bounds_img, &tb->r_bounds_img_n, (size_t)ntl * N * 2 * 64 * 4));
                HIP_TRY(launch_tile16_image(reinterpret_cast<const float4 *>(tb->r_bounds), reinterpret_cast<float4 *>(tb->r_bounds_img), tb->batch, N, 2,
                                            (long long)N * 8, tb->stream));
            }
            if (xper && (tb->rows_vary & 2u))
            {
                TRY(sized_buffer(&tb->r_xref_img, &tb->r_xref_img_n, (size_t)ntl * N * 64 * 4));
                HIP_TRY(launch_tile16_image(reinterpret_cast<const float4 *>(tb->r_xref), reinterpret_cast<float4 *>(tb->r_xref_img), tb->batch, N, 1,
                                            (long long)N * 4, tb->stream));
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(tb->stream));
    tb->derived_dirty[layout] = false;
    return 0;
}

// Automatic choice of the sixteen-instances-per-wave kernel (round 4, re-measured on the final binaries, 65 536-instance tracking workload cut to size, kernel ms,
// tile16 / 16-lane kernel, both longest first): 32 768: 1.03 / 0.97, 36 864: 1.11 / 1.08, 40 960: 1.09 / 1.19, 49 152: 1.24 / 1.40, 65 536: 1.54 / 1.83 — from 160
// instances per CU on; in index order the 16-lane kernel wins or ties at every size (65 536: 2.00 / 1.99), so the choice also asks for the longest-first dispatch
constexpr int kTile16AutoPerCu = 160;
bool tile16_auto_size(const TinyBatch *tb) { return dispatch_effective(tb) == 1 && tb->batch >= kTile16AutoPerCu * tb->n_cu; }
// ... and for a closed-loop run (tiny_batch_mpc_run_async: all MPC steps of a tile inside one launch).  Since the tiles of a run are dispatched by the iteration
// counts of the solve before it (history order, dispatch_order.hip: a tile's total over the steps of a run spreads widely, and four tiles per wave slot in index
// order ended a third above even slots) the warm-started tracking loop measures, ms per MPC step of the second of two 20-step runs, tile16 / 16-lane kernel:
// 24 576: 0.45 / 0.41, 32 768: 0.53 / 0.52, 40 960: 0.59 / 0.65, 49 152: 0.64 / 0.76, 65 536: 0.84 / 0.94, 98 304: 1.13 / 1.38, 131 072: 1.51 / 1.83 — from 160
// instances per CU on (tools/closed_loop_threshold.py; in index order the cross-over was 240: 65 536: 0.96 / 1.02)
constexpr int kTile16ClosedLoopPerCu = 160;
bool tile16_closed_loop_size(const TinyBatch *tb) { return tb->batch >= kTile16ClosedLoopPerCu * tb->n_cu; }

// admm_tile16.hip needs fp32 storage, a reference it does not have to keep resident (a window of a trajectory table that
// fits its LDS share, or one shared reference) and — checked by the caller — batch-shared bounds and no optional terms
// Round 4: per-instance bounds and a per-instance reference are served by the PI instantiations (rows fetched by LDS-DMA into per-wave rings,
// admm_tile16_pi.hip), one solve per launch; a closed-loop run with either keeps the 16-lane kernel.
bool tile16_per_instance(const TinyBatch *tb)
{
    return !bounds_all_shared(tb) || (tb->xref_mode != 1 && tb->in_xref.set && !tb->in_xref.shared);
}
// which tables of a pi launch go through the per-wave LDS-DMA slots, and which of those change along the horizon (RowParams::pi_flags)
struct Tile16Pi { bool bounds_ring, xref_ring, fits; unsigned flags; }; // flags: RowParams::pi_flags
Tile16Pi tile16_pi_plan(const TinyBatch *tb)
{
    Tile16Pi p;
    p.bounds_ring = !bounds_all_shared(tb);
    p.xref_ring = tb->xref_mode != 1 && tb->in_xref.set && !tb->in_xref.shared;
    p.flags = (p.bounds_ring ? (tb->rows_vary & 1u) : 0u) | (p.xref_ring ? (tb->rows_vary & 2u) : 0u);
    const int rows = tb->xref_mode == 1 ? tb->table_rows : tb->N;
    p.fits = tile16_pi_lds_bytes(tb->N, p.bounds_ring, p.xref_ring, p.flags, rows) <= 160 * 1024; // a staged table too long for the LDS share beside the slots
    return p;
}
// automatic choice with per-instance tables: the same rule as with shared ones (65 536 tracking instances, longest first, kernel ms, tile16 pi against the 16-lane
// kernel: bounds constant along the horizon 1.75 / 2.13, reference per step 1.81 / 1.96, both per step 1.95 / 2.15; in index order the rings lose, 2.45 / 2.22)
bool tile16_pi_auto(const TinyBatch *tb) { return !tb->order_dev && tile16_auto_size(tb); }
// The two matrix-core kernels keep v_med3_f32 in both arithmetic modes (tile16 sits at a register cliff, tile48's short-horizon body at 256 registers:
// tests/test_isa.py): in exact arithmetic a handle whose bounds table holds a zero on which the median breaks a tie the other way (TinyBatch::zero_ties)
// is handed over to the next exact family — the 16-lane kernels, the state-on-chip wave kernel — like every combination an instantiation does not serve
bool zero_ties_hand_over(const TinyBatch *tb) { return tb->zero_ties && tb->variant != VAR_ROW_FAST; }
// A closed-loop run is simulated when a plant is set or the call passes a disturbance or asks for the state trajectory: its on-chip loop exists on the
// 16-lane kernel only (admm_rowsim.hip), so tile16 hands such a run over as it does one with per-instance tables; the quad kernel's is replayed.
// What a call asks of the handle.  Solve: one solve per launch (tiny_batch_solve_*, the step functions, a run of ONE step); Run: tiny_batch_mpc_run_*(steps > 1).
// sim: the run is simulated (a question about the handle alone, such as the closed-loop kernel's name, knows the plant only); logs: it asks for the per-step log
struct Call
{
    enum Kind { Solve, Run } kind;
    bool sim, logs;
    bool run() const { return kind == Run; }
};
constexpr Call kLoneSolve{Call::Solve, false, false};
bool tile16_applies(const TinyBatch *tb, const Call &call)
{
    if (!tb->tile16_ok || tb->h16 || zero_ties_hand_over(tb) || (call.run() && call.sim)) return false;
    if (tile16_per_instance(tb)) return !call.run() && tile16_pi_plan(tb).fits;
    if (tb->xref_mode == 1) return tb->table_rows <= tile16_max_table_rows();
    return true;
}

// auto between the two state-on-chip kernels of the nx = 32 class, by rounds of the launch (measured on the 256 CUs of an MI355X,
// bench workload: one round of the wave kernel = 2 048 instances = 5.0 ms, one round of the tile kernel = 4 096 instances = 7.2 ms;
// 2 048: 5.4 against 7.1 ms, 2 304: 8.9 / 7.1, 4 096: 10.1 / 7.4, 4 352: 13.4 / 14.9, 6 144: 15.0 / 14.4, 16 384: 37.5 / 28.6; round 4: tile48 27.6)
bool tile48_pays(int batch, int n_cu)
{
    const long slots_w = 8L * n_cu, slots_t = 16L * n_cu; // resident instances: two waves per SIMD / one workgroup of sixteen per CU
    if (batch <= slots_w) return false;
    const long rounds_w = (batch + slots_w - 1) / slots_w, rounds_t = (batch + slots_t - 1) / slots_t;
    // a launch costs its rounds; ONE ratio carries the comparison (round 4: it used to be two absolute times of one workload): a round of the tile kernel
    // (sixteen instances per CU) takes 1.42 rounds of the wave kernel (eight per CU) — 6.9 against 4.85 ms at N = 50 on the MI355X, and the two scale
    // alike with the horizon and the iteration count; the wave kernel's last, partly filled round overlaps the one before (x 0.93)
    constexpr double kTileRoundInWaveRounds = 1.42;
    return rounds_t * kTileRoundInWaveRounds <= rounds_w * 0.93;
}

// What a call launches: resolved ONCE per call by resolve_plan(), read by everything that names, prepares, orders or launches the kernel.  loop: None, the call is
// one solve; OnChip, all the steps of a run inside one launch; Replay, solve + plant kernel per step, captured once into a hipGraph and replayed
enum class Loop { None, Replay, OnChip };
struct KernelPlan
{
    Kernel kernel = Kernel::Rowlane;
    bool exact = true;   // arithmetic: the reference's summation order, or fma
    bool pm = false;     // per-instance models (the ",pm" instantiations of the 16-lane, the two wave and the run-time-dimension kernel)
    bool ps = false;     // per-instance settings (the ",ps" instantiations of the 16-lane, the streaming row and the two wave kernels: admm_rowlane_ps.hip,
                         // admm_steps_ps.hip, admm_wave_ps.hip, admm_waveres_ps.hip)
    bool pi = false;     // tile16 with per-instance bounds / reference (admm_tile16_pi.hip)
    Tile16Pi pi_tables{}; // ... and which of its tables go through the rings
    Loop loop = Loop::None;
    bool sim{};          // the call's: an on-chip loop then takes the SIM instantiations (admm_rowsim.hip)
};

// the row / wave kernel a row variant launches for this handle (resolve_plan's second half; `forced`: tiny_batch_set_row_kernel)
Kernel row_kernel_for(const TinyBatch *tb, const Call &call)
{
    const std::optional<Kernel> forced = tb->row_family_forced;
    // one wavefront per instance: state on chip where the horizon fits (admm_waveres.hip), else streamed through HBM (admm_wave.hip)
    // (tile48: sixteen instances per workgroup on the matrix cores, admm_tile48.hip: fp32 storage)
    if (tb->wave_ok)
    {
        if (forced == Kernel::Wavestream) return Kernel::Wavestream;
        if (tb->tile48_ok && !tb->h16 && !zero_ties_hand_over(tb) && (forced == Kernel::Tile48 || (!forced && tile48_pays(tb->batch, tb->n_cu)))) return Kernel::Tile48;
        return tb->waveres_ok ? Kernel::Waveres : Kernel::Wavestream;
    }
    // per-instance bounds: the unrolled register-resident kernel (fp32 storage) and the rolled-loop ones (N <= 64, either storage)
    // read them from the [B][N][16] table, the streaming row kernel serves every other case; the quad kernel stages one shared table
    // the optional terms (Uref, coeff_d2p): on the unrolled register-resident kernel since round 4 (fp32 storage, batch-shared bounds, one solve per
    // launch); every other combination — fp16 storage, per-instance bounds, a closed-loop run, another forced family — on the streaming row kernel
    const bool optional_terms = tb->en_uref || tb->en_d2p;
    if (optional_terms && tb->row_dims_ok && !tb->h16 && bounds_all_shared(tb) && !call.run() && (!forced || forced == Kernel::Rowlane))
        return Kernel::Rowlane;
    if (!bounds_all_shared(tb))
    {
        if (optional_terms) return Kernel::Rowstream;
        if (tile16_applies(tb, call) && (forced == Kernel::Tile16 || (!forced && tile16_pi_auto(tb)))) return Kernel::Tile16;
        const std::optional<Kernel> ff = forced == Kernel::Tile16 ? std::nullopt : forced; // tile16 asked for but not applicable (closed-loop run): like auto
        if (tb->row_dims_ok && !tb->h16 && (!ff || ff == Kernel::Rowlane)) return Kernel::Rowlane;
        if (tb->rowloop_ok && (!ff || ff == Kernel::Rowloop)) return Kernel::Rowloop; // one step ahead from global memory
        return Kernel::Rowstream;
    }
    if (optional_terms) return Kernel::Rowstream; // the optional terms live in the streaming row kernel (c's u rows hold d elsewhere)
    // sixteen instances per wave, products on the matrix cores (admm_tile16.hip): on request only; needs fp32 storage and
    // a reference it does not have to keep resident (window of a table, or one shared reference)
    if (forced == Kernel::Tile16)
        return tile16_applies(tb, call) ? Kernel::Tile16 : (tb->row_dims_ok ? Kernel::Rowlane : (tb->rowloop_ok ? Kernel::Rowloop : Kernel::Rowstream));
    if (forced) return *forced;
    if (tb->quad_ok) return Kernel::Quadlane; // four lanes per instance (admm_quadlane.hip): nx = 4, nu = 1
    // auto (round 3): sixteen instances per wave on the matrix cores where the launch is at least two rounds deep for its one
    // wave per SIMD (2 048 tiles) — measured 1.79 against 1.91 ms on 65 536 tracking instances; smaller launches fill the chip
    // better with four instances per wave, and a closed-loop run keeps the kernel whose MPC loop stays on chip
    // (a caller that hands over its own dispatch order lists groups of four instances: the automatic choice then stays with the
    // kernel that order is for)
    // (round 4: tile16's MPC loop stays on chip too — tiny_batch_set_row_kernel(tb, 5) — but the warm-started solves of a closed loop are short and
    //  uneven, and sixteen instances in lock step lose more there than the matrix cores gain: measured 1.02 ms per MPC step of 65 536 tracking
    //  instances against 0.97 ms on the 16-lane kernel, so the automatic choice of a closed-loop run stays with the latter)
    if (tile16_applies(tb, call) && !tb->order_dev && (call.run() ? tile16_closed_loop_size(tb) : tile16_auto_size(tb))) return Kernel::Tile16;
    if (tb->row_dims_ok) return Kernel::Rowlane; // unrolled register-resident (fastest, one instantiation per (nx, nu, N))
    if (tb->rowloop_ok) return Kernel::Rowloop;  // rolled-loop register-resident (any N <= 64)
    return Kernel::Rowstream;                    // any N with the state in HBM
}

// the plan of a resolved variant v (not VAR_AUTO) whose row variants launch `row` (resolve_plan's last step, called from nowhere else)
int plan_of(const TinyBatch *tb, const Call &call, int v, Kernel row, KernelPlan *out)
{
    const Kernel k = out->kernel = v == VAR_STREAM ? Kernel::Stream : (v == VAR_GENERIC ? Kernel::Generic : row);
    out->exact = v == VAR_ROW_EXACT || v == VAR_GENERIC;
    out->pm = tb->pm;
    out->pi = k == Kernel::Tile16 && tile16_per_instance(tb);
    if (out->pi) out->pi_tables = tile16_pi_plan(tb);
    out->sim = call.sim;
    // A run of several steps stays on chip where the kernel has the loop, under fp32 storage and batch-shared bounds; simulated, on the 16-lane kernel only
    // (admm_rowsim.hip); and not with a log on the matrix-core kernel or with per-instance models: their largest instantiations sit at the register allocator's
    // cliff, and the log's store moved their pinned scratch whichever way it was written — such a run replays the same kernel, with the same bits
    const bool on_chip = traits(k).onchip_mpc && !tb->h16 && bounds_all_shared(tb) && (!call.sim || k == Kernel::Rowlane) &&
                         !(call.logs && (k == Kernel::Tile16 || out->pm));
    out->loop = !call.run() ? Loop::None : (on_chip ? Loop::OnChip : Loop::Replay);
    return 0;
}

// THE policy: which kernel serves this call on this handle, in which arithmetic, and how a run loops.  Reads the handle and changes nothing; the answer
// depends on rows_vary, which prepare_inputs() fills.
int resolve_plan(const TinyBatch *tb, const Call &call, KernelPlan *out)
{
    int v = tb->variant;
    if (tb->ps)
    {
        // per-instance settings: the two kernels with a ",ps" form — the unrolled 16-lane kernel where (nx, nu, N) is instantiated, under fp32 storage and
        // without the optional terms (shared or per-instance bounds), the streaming row kernel for everything else with nx + nu <= 16, with the same bits.
        // Nothing else is chosen: tile16 runs sixteen instances in lock step on one set of settings (a launch of its size goes to the 16-lane kernel), the
        // cartpole class leaves the quad kernel for rowlane<4,1,N,..,ps>
        if (tb->pm)
            return fail(TINY_BATCH_EUNSUPPORTED, "per-instance settings (tiny_batch_set_instance_settings) are not implemented together with per-instance models "
                                                 "(tiny_batch_clear_models() or tiny_batch_clear_instance_settings())");
        // The two wave kernels (one wavefront = one workgroup = one instance: its record is a wave-uniform value and its budget the bound of its own loop)
        // serve them too, on request: a forced family 6 or 7 (tiny_batch_set_row_kernel) resolves the automatic choice and the row variants to that family's
        // ",ps" instantiations.  Without one the automatic choice may be tile48 — sixteen instances per workgroup on one set of settings — and stays refused.
        // They have no on-chip loop: a run replays solve + plant kernel per step.  (tiny_batch_set_row_kernel accepts 7 only where N <= 50.)
        const std::optional<Kernel> wave_forced = tb->row_family_forced == Kernel::Wavestream || tb->row_family_forced == Kernel::Waveres ? tb->row_family_forced : std::nullopt;
        if (v == VAR_STREAM || v == VAR_GENERIC)
            return fail(TINY_BATCH_EUNSUPPORTED, "per-instance settings are implemented by the row variants only (tiny_batch_select_kernel 0, 2 or 3): variant %d holds one set "
                                                 "of settings per launch", v);
        if (wave_forced)
        {
            if (tb->en_uref || tb->en_d2p) // as without settings: no wave kernel reads them
                return fail(TINY_BATCH_EUNSUPPORTED, "the optional Uref / coeff_d2p terms (tiny_batch_set_optional_terms) are implemented by the row "
                                                     "kernels for nx + nu <= 16 only (nx=%d nu=%d, variant %d)", tb->nx, tb->nu, v);
            if (v == VAR_ROW_FAST && wave_forced != Kernel::Waveres)
                return fail(TINY_BATCH_EUNSUPPORTED, "fma arithmetic for 16 < nx + nu <= 64 needs the state-on-chip wave kernel (N <= 50); beyond that it is the streaming MFMA kernel (variant 1)");
            out->kernel = *wave_forced;
            out->exact = v != VAR_ROW_FAST;
            out->pm = out->pi = false;
            out->ps = true;
            out->sim = call.sim;
            out->loop = call.run() ? Loop::Replay : Loop::None;
            return 0;
        }
        if (tb->row_family_forced == Kernel::Tile48)
            return fail(TINY_BATCH_EUNSUPPORTED, "the forced row kernel tile48 (tiny_batch_set_row_kernel) has no per-instance-settings form: its sixteen instances per workgroup run on "
                                                 "one set of settings; the two wave kernels (6 or 7) serve tiny_batch_set_instance_settings for this class");
        if (!tb->rowmath_ok && tb->wave_ok)
            return fail(TINY_BATCH_EUNSUPPORTED, "per-instance settings are implemented by the 16-lane row kernels (a compiled nx + nu <= 16) and, on request, by the two wave kernels: "
                                                 "the automatic choice for nx=%d nu=%d may be tile48, which holds one set of settings per launch, so it is not made under them; "
                                                 "tiny_batch_set_row_kernel(tb, 6 or 7) serves this class (or tiny_batch_clear_instance_settings())", tb->nx, tb->nu);
        if (!tb->rowmath_ok)
            return fail(TINY_BATCH_EUNSUPPORTED, "per-instance settings are implemented by the 16-lane row kernels only (a compiled nx + nu <= 16): nx=%d nu=%d runs on the "
                                                 "generic or streaming MFMA kernel, which hold one set of settings per launch (tiny_batch_clear_instance_settings())", tb->nx, tb->nu);
        const std::optional<Kernel> forced = tb->row_family_forced;
        if (forced && forced != Kernel::Rowlane && forced != Kernel::Rowstream)
            return fail(TINY_BATCH_EUNSUPPORTED, "the forced row kernel %s (tiny_batch_set_row_kernel) has no per-instance-settings form: only the 16-lane kernel (1), the "
                                                 "streaming row kernel (3) or auto (0) serve tiny_batch_set_instance_settings", traits(*forced).name);
        const bool unrolled = tb->row_dims_ok && !tb->h16 && !tb->en_uref && !tb->en_d2p && forced != Kernel::Rowstream;
        out->kernel = unrolled ? Kernel::Rowlane : Kernel::Rowstream;
        out->exact = v != VAR_ROW_FAST;
        out->pm = out->pi = false;
        out->ps = true;
        out->sim = call.sim;
        // the on-chip loop's ps instantiations: shared bounds, no plant, logs included; every other run replays the one-solve kernel
        out->loop = !call.run() ? Loop::None : (unrolled && bounds_all_shared(tb) && !call.sim ? Loop::OnChip : Loop::Replay);
        return 0;
    }
    if (tb->pm)
    {
        // per-instance models: the unrolled 16-lane kernel where (nx, nu, N) is instantiated, the run-time-dimension kernel otherwise (both read a gain
        // record per instance).  The two wave kernels (one wavefront = one workgroup = one instance: a per-instance gain table is a wave-uniform base
        // address) serve them too, on request: a forced family 6 or 7 (tiny_batch_set_row_kernel) resolves the automatic choice and the row variants to
        // that family's ",pm" instantiations; the automatic choice without one stays where tests/golden/kernel_choice.json records it.  Every other kernel
        // keeps ONE gain table for the whole launch — tile16's and tile48's MFMA A operand is one gain matrix for all sixteen columns, the streaming
        // kernels stage theirs once per workgroup of several instances — and is never chosen.
        const bool wave_forced = tb->row_family_forced == Kernel::Wavestream || tb->row_family_forced == Kernel::Waveres;
        if (tb->h16)
            return fail(TINY_BATCH_EUNSUPPORTED, "per-instance models (tiny_batch_set_models) are implemented for fp32 storage only: tiny_batch_set_storage(tb, 32) or tiny_batch_clear_models()");
        if (tb->en_uref || tb->en_d2p)
            return fail(TINY_BATCH_EUNSUPPORTED, "the optional Uref / coeff_d2p terms are not implemented with per-instance models (tiny_batch_set_optional_terms(tb, 0, 0) or tiny_batch_clear_models())");
        if (v == VAR_STREAM)
            return fail(TINY_BATCH_EUNSUPPORTED, "the streaming MFMA kernel (variant 1) holds one gain matrix for the whole launch and cannot serve per-instance models");
        if (wave_forced && v != VAR_GENERIC)
        {
            if (v == VAR_ROW_FAST && tb->row_family_forced != Kernel::Waveres)
                return fail(TINY_BATCH_EUNSUPPORTED, "fma arithmetic for 16 < nx + nu <= 64 needs the state-on-chip wave kernel (N <= 50); beyond that it is the streaming MFMA kernel (variant 1)");
            return plan_of(tb, call, v == VAR_AUTO ? VAR_ROW_EXACT : v, *tb->row_family_forced, out);
        }
        if (v == VAR_AUTO)
        {
            if (!tb->row_dims_ok && !tb->generic_ok)
                return fail(TINY_BATCH_EUNSUPPORTED, "per-instance models need the unrolled 16-lane kernel (an instantiated nx, nu, N) or the run-time-dimension exact kernel "
                                                     "(nx, nu each <= 4 or a multiple of 4); nx=%d nu=%d N=%d has neither", tb->nx, tb->nu, tb->N);
            v = tb->row_dims_ok ? VAR_ROW_EXACT : VAR_GENERIC;
        }
        if (v == VAR_ROW_EXACT || v == VAR_ROW_FAST)
        {
            if (!tb->row_dims_ok)
                return fail(TINY_BATCH_EUNSUPPORTED, "with per-instance models the row variants run on the unrolled 16-lane kernel only, which has no instantiation for nx=%d nu=%d N=%d "
                                                     "(variant 4, the run-time-dimension exact kernel, serves it)", tb->nx, tb->nu, tb->N);
            if (tb->row_family_forced && tb->row_family_forced != Kernel::Rowlane)
                return fail(TINY_BATCH_EUNSUPPORTED, "the forced row kernel (tiny_batch_set_row_kernel) keeps one gain table for the whole launch and cannot serve per-instance models "
                                                     "(tile16: its MFMA A operand is one gain matrix for all 16 columns); only the 16-lane kernel (1) or auto (0) can");
        }
        if (v == VAR_GENERIC && !tb->generic_ok)
            return fail(TINY_BATCH_EUNSUPPORTED, "the run-time-dimension exact kernel (variant 4) needs nx, nu each <= 4 or a multiple of 4 (nx=%d nu=%d)", tb->nx, tb->nu);
        return plan_of(tb, call, v, Kernel::Rowlane, out);
    }
    // row variants: register-resident kernel when (nx,nu,N) is instantiated, else the any-N row kernel with the state in HBM
    // per-instance bounds: the streaming row kernel and the wave kernel read them per instance; the register-resident
    // kernels stage ONE table in LDS and need batch-shared bounds
    const bool row_ok = tb->row_dims_ok || tb->rowmath_ok || tb->wave_ok;
    const Kernel row = row_kernel_for(tb, call);
    if (v == VAR_ROW_FAST && tb->wave_ok && row != Kernel::Waveres && row != Kernel::Tile48)
        return fail(TINY_BATCH_EUNSUPPORTED, "fma arithmetic for 16 < nx + nu <= 64 needs the state-on-chip wave kernel (N <= 50); beyond that it is the streaming MFMA kernel (variant 1)");
    if (v == VAR_AUTO)
    {
        // the automatic choice is exact arithmetic or nothing: a class without a compiled exact kernel runs in fma arithmetic on the padded
        // MFMA kernel only when the caller has asked for it by name (round 4: it used to be selected silently)
        if (!row_ok && !tb->generic_ok)
            return fail(TINY_BATCH_EUNSUPPORTED, "nx=%d nu=%d has no exact-arithmetic kernel (the reference's own summation order depends on column alignment "
                                                 "unless nx and nu are each <= 4 or a multiple of 4); tiny_batch_select_kernel(tb, 1) opts into fma arithmetic "
                                                 "on the MFMA streaming kernel", tb->nx, tb->nu);
        v = row_ok ? VAR_ROW_EXACT : VAR_GENERIC; // a class outside the compiled lists: exact arithmetic with run-time dimensions (admm_generic.hip)
    }
    if (v == VAR_GENERIC && (!tb->generic_ok || tb->h16 || tb->en_uref || tb->en_d2p))
        return fail(TINY_BATCH_EUNSUPPORTED, "the run-time-dimension exact kernel (variant 4) needs nx, nu each <= 4 or a multiple of 4 (nx <= 64, nu <= 32), "
                                             "fp32 storage and no optional terms (nx=%d nu=%d)", tb->nx, tb->nu);
    const bool row_variant = v == VAR_ROW_EXACT || v == VAR_ROW_FAST;
    if ((tb->en_uref || tb->en_d2p) && (!tb->rowmath_ok || !row_variant))
        return fail(TINY_BATCH_EUNSUPPORTED, "the optional Uref / coeff_d2p terms (tiny_batch_set_optional_terms) are implemented by the row "
                                             "kernels for nx + nu <= 16 only (nx=%d nu=%d, variant %d)", tb->nx, tb->nu, v);
    if (row_variant && !row_ok)
        return fail(TINY_BATCH_EUNSUPPORTED, "no row kernel instantiation for nx=%d nu=%d (needs nx + nu <= 16)", tb->nx, tb->nu);
    if (v == VAR_STREAM && !tb->tile_dims_ok)
        return fail(TINY_BATCH_EUNSUPPORTED, "no streaming kernel instantiation for nx=%d nu=%d", tb->nx, tb->nu);
    if (v == VAR_STREAM && tb->h16)
        return fail(TINY_BATCH_EUNSUPPORTED, "fp16 storage is implemented by the row kernels only (nx + nu <= 16)");
    return plan_of(tb, call, v, row, out);
}

// the name tiny_batch_kernel_name() reports: "<family><nx,nu[,N],arithmetic[,h16 | ,h16d | ,pi | ,pm][,ps]>"; the streaming kernel is named by its chunk counts
std::string kernel_name(const TinyBatch *tb, const KernelPlan &pl)
{
    const KernelTraits &t = traits(pl.kernel);
    char nm[96];
    if (pl.kernel == Kernel::Stream)
    {
        snprintf(nm, sizeof nm, "stream<%d,%d>", tb->NXC, tb->NUC);
        return nm;
    }
    int n = snprintf(nm, sizeof nm, "%s<%d,%d", t.name, tb->nx, tb->nu);
    if (t.name_has_N) n += snprintf(nm + n, sizeof nm - n, ",%d", tb->N);
    const bool d32 = tb->dual32_forced ? tb->dual32 : (tb->dual32_pref && t.fp32_duals);
    const char *suffix = pl.pm ? ",pm" : pl.pi ? ",pi" : (t.name_has_storage && tb->h16) ? (d32 ? ",h16d" : ",h16") : "";
    snprintf(nm + n, sizeof nm - n, ",%s%s%s>", pl.exact ? "exact" : "fast", suffix, pl.ps ? ",ps" : "");
    return nm;
}

// the name of the kernel a lone solve or a closed-loop run of several steps launches; "unsupported" where no kernel would run.
// One buffer per question and handle: the pointer holds until the same question is asked of the same handle again
const char *plan_name(TinyBatch *tb, const Call &call)
{
    std::string &name = tb->name_buf[call.run() ? 1 : 0];
    const std::string keep = g_err;
    KernelPlan pl;
    name = resolve_plan(tb, call, &pl) ? "unsupported" : kernel_name(tb, pl);
    g_err = keep;
    return name.c_str();
}

// A closed-loop run as the public call states it (tiny_batch_mpc_run_*): every pointer is DEVICE memory and may be NULL
struct RunArgs
{
    const char *who; // the public call, for its messages
    int steps, window_advance;
    const float *d_w;               // [steps][B][nx] disturbance
    float *d_u0_traj, *d_x_traj;    // [steps][B][nu] u.col(0) of every step; [steps][B][nx] the plant's state after every step
    int *d_iter_log, *d_status_log; // [steps][B] the per-step solver log: row k = iter[] / status[] after the solve of MPC step k
    bool from_reset = false;        // the run starts from a reset workspace (mpc_run_sim notes it before it materialises the zeros)
    // the rows of MPC step k; log_row: iter[] / status[] as the solve before it left them (two device-to-device copies on the handle's stream: captured with the rest)
    const float *w_at(const TinyBatch *tb, int k) const { return d_w ? d_w + (size_t)k * tb->batch * tb->nx : nullptr; }
    float *x_at(const TinyBatch *tb, int k) const { return d_x_traj ? d_x_traj + (size_t)k * tb->batch * tb->nx : nullptr; }
    float *u0_at(const TinyBatch *tb, int k) const { return d_u0_traj ? d_u0_traj + (size_t)k * tb->batch * tb->nu : nullptr; }
    hipError_t log_row(const TinyBatch *tb, int k) const
    {
        const size_t o = (size_t)k * tb->batch, bytes = (size_t)tb->batch * sizeof(int);
        hipError_t e = hipSuccess;
        if (d_iter_log) e = hipMemcpyAsync(d_iter_log + o, tb->iter, bytes, hipMemcpyDeviceToDevice, tb->stream);
        if (e == hipSuccess && d_status_log) e = hipMemcpyAsync(d_status_log + o, tb->status, bytes, hipMemcpyDeviceToDevice, tb->stream);
        return e;
    }
};

// The hipGraph cached by tiny_batch_mpc_run_traj_async bakes in every kernel ARGUMENT of its launches (RowParams /
// SolveParams are passed by value): rho, tolerances, bound flags, array pointers and strides, window advance.  Anything
// that can change one of them drops the graph; the next mpc_run captures a fresh one.
void invalidate_graph(TinyBatch *tb)
{
    if (tb->graph_exec)
    {
        (void)hipSetDevice(tb->device);
        (void)hipStreamSynchronize(tb->stream); // a replay may still be in flight
        (void)hipGraphExecDestroy(tb->graph_exec);
        tb->graph_exec = nullptr;
    }
    tb->graph_sig.clear();
}

// ... and a run whose signature equals the cached graph's replays it.  The signature is complete (round 3) — rho, the shared / per-instance modes that set the
// strides, the bound flags and the dispatch order are in it — so setters that only change buffer CONTENTS do not drop the graph: `set_xref; mpc_run(k)` in a loop
// replays one captured graph
std::string graph_signature(const TinyBatch *tb, const KernelPlan &pl, const RunArgs &run)
{
    char sig[768];
    snprintf(sig, sizeof sig, "%d|%p|%p|%p|%p|%p|%p|%p|%p|%p|%d|%d|%d|%s|%d|%d|%g|%g|%d|%d|%p|%p|%p|%d|%p|%p|%p|%p|%d%d|%a|%d%d%d|%d%d|%d|%p|%p|%p|%d|%p|%p|%p|%d", tb->plant_mode, (void *)tb->plant_A,
             (void *)tb->plant_B, (const void *)run.d_w, (void *)run.d_x_traj, (void *)tb->pm_src, (void *)tb->pm_row[0],
             (void *)tb->pm_row[1], (void *)tb->pm_wave[0], (void *)tb->pm_wave[1], run.steps, run.window_advance, tb->variant, kernel_name(tb, pl).c_str(), tb->max_iter,
             tb->check_termination, (double)tb->abs_pri_tol, (double)tb->abs_dua_tol, tb->xref_mode, tb->table_rows, (void *)tb->pair[0],
             (void *)tb->arr[0], (void *)tb->r_bounds, (int)tb->h16, (void *)tb->stream, (void *)run.d_u0_traj, (void *)tb->r_xref,
             (void *)tb->r_uref, (int)tb->en_uref, (int)tb->en_d2p, (double)tb->rho, (int)bounds_all_shared(tb),
             (int)(tb->in_xref.set && tb->in_xref.shared), (int)(tb->in_uref.set && tb->in_uref.shared), state_bound_on(tb), input_bound_on(tb),
             tb->dispatch_mode, (void *)tb->order_dev, (void *)tb->mats_exact, (void *)tb->xref_start, (int)tb->zero_ties,
             (void *)run.d_iter_log, (void *)run.d_status_log, (void *)tb->ps_dev, budget_max(tb));
    return sig;
}

// fp16 storage: bring the duals pair to the width the coming launch implements.  Under tiny_batch_set_storage(tb, 16) fp32 duals are a
// PREFERENCE (the register-resident 16-lane and quad kernels keep them — KernelTraits::fp32_duals — every other kernel — streamed state, per-instance
// bounds under fp16, the optional terms, the six single-function kernels — stores binary16 duals): the array is converted in place of being refused.
// An explicit tiny_batch_set_storage_ex(tb, 16, 32) stays a requirement (the caller is told when a kernel cannot honour it).
int settle_dual_width(TinyBatch *tb, bool kernel_keeps_fp32_duals)
{
    if (!tb->h16 || tb->dual32_forced) return 0;
    const bool want32 = tb->dual32_pref && kernel_keeps_fp32_duals;
    if (tb->dual32 == want32) return 0;
    if (tb->layout == LAYOUT_ROW && tb->pair[5])
    {
        float *nw = nullptr;
        TRY(dev_alloc_zero(&nw, want32 ? tb->pair_floats : (tb->pair_floats + 1) / 2));
        HIP_TRY(launch_dual_width(tb->pair[5], nw, (long long)tb->pair_floats, want32 ? 1 : 0, tb->stream));
        HIP_TRY(hipStreamSynchronize(tb->stream));
        (void)guarded_free(tb->pair[5]);
        tb->pair[5] = nw;
    }
    tb->dual32 = want32;
    invalidate_graph(tb); // the array pointer is a kernel argument
    return 0;
}

void fill_row_params(TinyBatch *tb, RowParams &P, bool exact)
{
    P.nx = tb->nx; P.nu = tb->nu; P.N = tb->N; P.batch = tb->batch;
    P.rho = tb->rho; P.abs_pri_tol = tb->abs_pri_tol; P.abs_dua_tol = tb->abs_dua_tol;
    P.max_iter = budget_max(tb); P.check_termination = tb->check_termination; // (per-instance settings: the loop bound of the launch; the kernel reads the rest per instance)
    P.duals_zero = tb->duals_zero_pending ? 1 : 0;
    P.cold_start = tb->cold_pending ? 1 : 0;
    P.xref_mode = tb->xref_mode;
    P.xu = tb->pair[0]; P.qr = tb->pair[1]; P.pd = tb->pair[2]; P.vz = tb->pair[3]; P.vzn = tb->pair[4]; P.gy = tb->pair[5];
    P.xref = tb->r_xref;
    P.xref_inst_stride = (tb->in_xref.set && !tb->in_xref.shared) ? (unsigned)(tb->N * tb->rw) : 0u;
    P.pi_flags = 0u;
    P.xref_table = tb->h16 ? tb->tab_row_h : tb->tab_row; P.xref_start = tb->xref_start; P.table_rows = tb->table_rows;
    P.bounds = tb->r_bounds;
    P.bounds_inst_stride = bounds_all_shared(tb) ? 0u : (unsigned)(tb->N * tb->rw);
    P.mats = exact ? tb->mats_exact : tb->mats_fast;
    P.uref = tb->en_uref ? tb->r_uref : nullptr;
    P.uref_inst_stride = (tb->in_uref.set && !tb->in_uref.shared) ? (unsigned)(tb->N * tb->rw) : 0u;
    P.en_d2p = tb->en_d2p ? 1 : 0;
    P.order = tb->order_dev;
    P.res = tb->res; P.status = tb->status; P.iter = tb->iter; P.n_unsolved = tb->n_unsolved;
    P.mpc_steps = 1; P.window_advance = 0; P.u0_traj = nullptr; P.x0buf = tb->x0buf;
    P.dual32 = (tb->h16 && tb->dual32) ? 1 : 0;
    P.inst_map = nullptr; // enqueue_dispatch_order sets it for the one launch that reads it
    P.exact_ties = tb->zero_ties ? 1 : 0;
    P.iter_log = P.status_log = nullptr; // enqueue_solve sets them for the on-chip closed loop
}

int check_optional_terms(const TinyBatch *tb)
{
    if (tb->en_uref && (!tb->have_rcost || !tb->in_uref.set))
        return fail(TINY_BATCH_ENOTREADY, "the Uref term is enabled: tiny_batch_set_input_cost and tiny_batch_set_uref must be called first");
    if (tb->en_d2p && tb->coeff_d2p.empty())
        return fail(TINY_BATCH_ENOTREADY, "the coeff_d2p term is enabled: tiny_batch_set_coeff_d2p must be called first");
    return 0;
}

// One of the six step functions of admm.hpp:10-18 over the whole batch (admm_steps.hip).
int run_step(TinyBatch *tb, int fn, int *converged_host, int *n_true)
{
    if (tb->pm)
        return fail(TINY_BATCH_EUNSUPPORTED, "the six single-function step kernels read one shared model: not available with per-instance models (tiny_batch_clear_models())");
    if (!tb->have_cache || !tb->have_dyn || !tb->have_settings)
        return fail(TINY_BATCH_ENOTREADY, "set_cache, set_dynamics and set_settings must be called first");
    if (!tb->rowmath_ok)
        return fail(TINY_BATCH_EUNSUPPORTED, "the single-function kernels need nx + nu <= 16 and an entry in TINY_FOR_EACH_ROWDIMS (nx=%d nu=%d)", tb->nx, tb->nu);
    if (tb->dual32_forced) return fail(TINY_BATCH_EUNSUPPORTED, "the single-function kernels do not implement fp16 storage with fp32 duals (tiny_batch_set_storage_ex(tb, 16, 32))");
    TRY(check_optional_terms(tb));
    TRY(set_device(tb));
    if (tb->gains_dirty) TRY(pack_gains(tb));
    TRY(ensure_layout(tb, LAYOUT_ROW));
    TRY(settle_dual_width(tb, false));
    TRY(prepare_inputs(tb, LAYOUT_ROW));
    TRY(flush_pending(tb));
    if (!tb->conv_dev) TRY(dev_alloc_zero((float **)&tb->conv_dev, tb->batch));
    RowParams P;
    fill_row_params(tb, P, tb->variant != VAR_ROW_FAST);
    HIP_TRY(hipMemsetAsync(tb->n_unsolved, 0, 2 * sizeof(int), tb->stream)); // [0] unsolved count, [1] tile queue of admm_tile16.hip
    // (per-instance settings: termination_condition reads the instance's record; update_slack sees the bound flags through the table; the rest read no setting)
    hipError_t e = tb->ps && fn == STEP_TERMINATION_CONDITION
                       ? launch_admm_termination_ps(tb->nx, tb->nu, tb->variant != VAR_ROW_FAST, tb->h16, P, SettingsParams{tb->ps_dev}, tb->conv_dev, tb->stream)
                       : launch_admm_step(tb->nx, tb->nu, tb->variant != VAR_ROW_FAST, tb->h16, fn, P, tb->conv_dev, tb->stream);
    if (e != hipSuccess) return fail(TINY_BATCH_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (fn == STEP_TERMINATION_CONDITION)
    {
        int n_false = 0;
        HIP_TRY(hipMemcpyAsync(&n_false, tb->n_unsolved, sizeof(int), hipMemcpyDeviceToHost, tb->stream));
        if (converged_host)
            HIP_TRY(hipMemcpyAsync(converged_host, tb->conv_dev, (size_t)tb->batch * sizeof(int), hipMemcpyDeviceToHost, tb->stream));
        HIP_TRY(hipStreamSynchronize(tb->stream));
        if (n_true) *n_true = tb->batch - n_false;
    }
    return 0;
}

// per-instance models: the 16-lane kernel's gain rows in the arithmetic the plan computes in, packed from the records when they changed (the
// run-time-dimension kernel reads the records themselves); the two wave kernels' tables likewise, at row width 64
bool wave_family(Kernel k) { return k == Kernel::Wavestream || k == Kernel::Waveres; }
int pack_models(TinyBatch *tb, const KernelPlan &pl)
{
    const int f = pl.exact ? 0 : 1;
    if (wave_family(pl.kernel))
    {
        if (!tb->pm_wave_dirty[f]) return 0;
        const size_t n = (size_t)tb->batch * pm_wave_floats(tb->nx, tb->nu);
        if (!tb->pm_wave[f]) HIP_TRY(guarded_malloc((void **)&tb->pm_wave[f], n * sizeof(float)));
        HIP_TRY(launch_models_pack_wave(tb->pm_src, tb->pm_wave[f], tb->batch, tb->nx, tb->nu, f, tb->stream));
        tb->pm_wave_dirty[f] = false;
        return 0;
    }
    if (pl.kernel != Kernel::Rowlane) return 0;
    if (!tb->pm_row_dirty[f]) return 0;
    const long long n = (long long)tb->batch * pm_row_floats(tb->nx, tb->nu);
    if (!tb->pm_row[f]) HIP_TRY(guarded_malloc((void **)&tb->pm_row[f], (size_t)n * sizeof(float)));
    HIP_TRY(launch_models_pack_row(tb->pm_src, tb->pm_row[f], tb->batch, tb->nx, tb->nu, f, tb->stream));
    tb->pm_row_dirty[f] = false;
    return 0;
}

ModelParams model_params(const TinyBatch *tb, const KernelPlan &pl)
{
    ModelParams M;
    M.rho = tb->pm_rho;
    if (pl.kernel == Kernel::Generic) { M.mats = tb->pm_src; M.mats_stride = (unsigned)pm_gen_floats(tb->nx, tb->nu); }
    else if (wave_family(pl.kernel)) { M.mats = tb->pm_wave[pl.exact ? 0 : 1]; M.mats_stride = (unsigned)pm_wave_floats(tb->nx, tb->nu); }
    else { M.mats = tb->pm_row[pl.exact ? 0 : 1]; M.mats_stride = (unsigned)pm_row_floats(tb->nx, tb->nu); }
    return M;
}

// Tile grouping (tiny_batch_set_tile_grouping): whether the launch of a lone solve with this plan forms tile16's tiles through the instance map — the
// shared-table cold-start instantiations, a window reference, the predictor's dispatch (no caller's order).  Automatic: where the two-ended tile
// queue is on (at least three tiles per wave slot), which is where the replay of the true counts says it pays (tests/fuzz/sim_tile_regroup.py).
bool tile_grouping_wanted(const TinyBatch *tb, const KernelPlan &pl)
{
    static const int env = [] { const char *e = getenv("TINYMPC_T16_GROUP"); return e ? atoi(e) : -1; }();
    const int mode = tb->tile_grouping >= 0 ? tb->tile_grouping : env; // the setter, then the environment
    if (mode == 0) return false;
    if (pl.kernel != Kernel::Tile16 || pl.pi || pl.pm || tb->xref_mode != 1 || tb->order_dev) return false;
    if (!tb->cold_pending || dispatch_effective(tb) != 1 || tb->max_iter <= 0) return false;
    return mode >= 1 || tile16_two_ended(tb->batch, tb->n_cu, tb->tile_queue);
}

// the map is (re)built on the handle's stream when such a launch is next and the window starts have moved since the last build
int ensure_tile_map(TinyBatch *tb, const KernelPlan &pl)
{
    if (!tile_grouping_wanted(tb, pl) || (tb->tile_map && !tb->tile_map_dirty)) return 0;
    const size_t n = (size_t)((tb->batch + 15) / 16) * 16;
    if (!tb->tile_map) TRY(dev_alloc_zero((float **)&tb->tile_map, n + (size_t)instance_map_scratch_ints())); // the map, then the sort's histogram and cursors
    const hipError_t e = launch_instance_map(tb->xref_start, tb->batch, tb->tile_map, tb->tile_map + n, tb->stream);
    if (e != hipSuccess) return fail(TINY_BATCH_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    tb->tile_map_dirty = false;
    ++tb->tile_map_builds;
    return 0;
}

// everything a solve needs that may allocate, copy or synchronise (not capturable in a hipGraph); *plan: what the solve launches
int prepare_solve(TinyBatch *tb, const Call &call, KernelPlan *plan)
{
    if (!(tb->pm || (tb->have_cache && tb->have_dyn)) || !tb->have_settings)
        return fail(TINY_BATCH_ENOTREADY, "tiny_batch_solve: set_cache, set_dynamics (or set_models) and set_settings must be called first");
    for (int k = 0; k < 4; k += 2)
    {
        const InputArr &lo = tb->in_bnd[k], &hi = tb->in_bnd[k + 1];
        const bool lo_inst = lo.set && !lo.shared, hi_inst = hi.set && !hi.shared;
        if (lo_inst != hi_inst && (lo.set || hi.set))
            return fail(TINY_BATCH_EINVAL, "min and max bounds must both be shared or both be per-instance");
    }
    TRY(check_optional_terms(tb));
    TRY(set_device(tb));
    // Provisional: the layout, the gain form and the dual width have to be settled BEFORE prepare_inputs, whose rows_vary the final plan reads.  The two can
    // differ only between tile16 and another kernel of the ROW layout, in the same arithmetic, under fp32 storage (rows_vary enters through the pi
    // tables' LDS fit alone, and fp16 storage excludes tile16), where settle_dual_width does nothing
    KernelPlan pl;
    TRY(resolve_plan(tb, call, &pl));
    if (tb->pm) TRY(pack_models(tb, pl));
    else if (tb->gains_dirty) TRY(pack_gains(tb));
    // (whatever the mode says NOW: a launch sequence enqueued after one prepare_solve — the captured graph of tiny_batch_mpc_run_async — gains a history with its
    //  first solve, and its second one is then dispatched by it)
    if (!tb->order_buf && tb->bpad4 / 4 >= kDispatchMinGroups)
    {
        TRY(dev_alloc_zero(&tb->key_buf, (size_t)tb->bpad4 / 4 + (size_t)tb->bpad4 / 16 + 16)); // group keys, then tile keys
        TRY(dev_alloc_zero((float **)&tb->order_buf, (size_t)tb->bpad4 / 4));
    }
    const int layout = traits(pl.kernel).layout;
    const bool inputs_rebuilt = tb->derived_dirty[layout];
    TRY(ensure_layout(tb, layout));
    TRY(settle_dual_width(tb, traits(pl.kernel).fp32_duals));
    TRY(prepare_inputs(tb, layout));
    TRY(flush_x0_zero(tb)); // every solve reads x.col(0)
    if (budget_min(tb) <= 0) TRY(flush_pending(tb)); // an instance that runs no iteration must read back as the reset left it
    // A cold start that converges in its first iteration (x0 at the origin) runs no backward sweep, which is what writes p, d, v, z.
    // reset_workspace() is folded into the launch by every fused kernel: the register-resident ones start from zero registers,
    // the streaming ones (MFMA, rowstream, wavestream) read zeros in their first iteration and zero-fill p, d, v, z of such an
    // instance in their epilogue
    if (inputs_rebuilt) TRY(resolve_plan(tb, call, plan));
    else *plan = pl; // rows_vary did not move: the provisional plan is the final one
    return call.run() ? 0 : ensure_tile_map(tb, *plan); // (a run forms no tiles through the map)
}

void fill_solve_params(const TinyBatch *tb, SolveParams &P)
{
    P.nx = tb->nx; P.nu = tb->nu; P.N = tb->N; P.batch = tb->batch; P.ntiles = tb->ntiles;
    P.rho = tb->rho; P.abs_pri_tol = tb->abs_pri_tol; P.abs_dua_tol = tb->abs_dua_tol;
    P.max_iter = tb->max_iter; P.check_termination = tb->check_termination;
    P.en_state_bound = tb->en_state_bound; P.en_input_bound = tb->en_input_bound;
    P.duals_zero = tb->duals_zero_pending ? 1 : 0;
    P.cold_start = tb->cold_pending ? 1 : 0;
    P.xref_mode = tb->xref_mode;
    P.x = tb->arr[TINY_ARR_X]; P.q = tb->arr[TINY_ARR_Q]; P.p = tb->arr[TINY_ARR_P];
    P.v = tb->arr[TINY_ARR_V]; P.vnew = tb->arr[TINY_ARR_VNEW]; P.g = tb->arr[TINY_ARR_G];
    P.u = tb->arr[TINY_ARR_U]; P.r = tb->arr[TINY_ARR_R]; P.d = tb->arr[TINY_ARR_D];
    P.z = tb->arr[TINY_ARR_Z]; P.znew = tb->arr[TINY_ARR_ZNEW]; P.y = tb->arr[TINY_ARR_Y];
    P.xmin = tb->t_bnd[0]; P.xmax = tb->t_bnd[1]; P.umin = tb->t_bnd[2]; P.umax = tb->t_bnd[3]; P.xref = tb->t_xref;
    const long long xt = (long long)tb->N * WAVE * tb->NXC, ut = (long long)(tb->N - 1) * WAVE * tb->NUC;
    P.xb_tile_stride = (tb->in_bnd[0].set && !tb->in_bnd[0].shared) ? xt : 0;
    P.ub_tile_stride = (tb->in_bnd[2].set && !tb->in_bnd[2].shared) ? ut : 0;
    P.xref_tile_stride = (tb->in_xref.set && !tb->in_xref.shared) ? xt : 0;
    P.xref_table = tb->tab_tile; P.xref_start = tb->xref_start; P.table_rows = tb->table_rows;
    P.res = tb->res; P.status = tb->status; P.iter = tb->iter; P.n_unsolved = tb->n_unsolved;
    P.opnd = tb->opnd; P.qvec = tb->qvec;
}

// The dispatch order of one launch (dispatch_order.hip; pays off only when the launch is several rounds of waves deep): enqueues the sort by the previous
// solve's iteration counts (history), the predictor sweep and its sort, or — where neither runs — the reset of the two counters ([0] unsolved count, [1] tile
// queue of admm_tile16.hip; both sorts zero them themselves: one stream node less), and points P.order at the result.  Returns what tiny_batch_dispatch_applied()
// reports (0 index order, 1 predicted, 2 the caller's order, 3 history) or a negative error code.
// run_steps > 1: the launch is the on-chip closed loop of tiny_batch_mpc_run_*; it differs from a lone solve (also each solve of a captured run) in that
//  * it asks tb->dispatch_mode where a lone solve asks dispatch_effective() for the predictor: flush_pending() has already cleared cold_pending, `from_reset` carries it;
//  * history wins over the predictor (in a lone solve dispatch_effective() makes them exclusive);
//  * tile16 orders its tiles by the SUM of the counts (a tile's total over the run), a lone solve by the largest;
//  * the rolled-loop kernel has no on-chip run (KernelTraits::order_unit_run);
//  * max_iter > 1 guards the predictor only: the run's later steps profit from the history order whatever the first one does.
// Common to both: tile16 drops a caller's order, which lists groups of four instances, not tiles of sixteen.
int enqueue_dispatch_order(TinyBatch *tb, const KernelPlan &pl, int run_steps, bool from_reset, RowParams &P)
{
    const bool run = run_steps > 1;
    const int unit = run ? traits(pl.kernel).order_unit_run : traits(pl.kernel).order_unit_solve;
    const bool eligible = unit && !tb->order_dev && tb->bpad4 / 4 >= kDispatchMinGroups && tb->order_buf;
    // a run's tiles / groups go longest first by the counts of the solve before it (the last step of the previous run): a tile's total over the steps
    // of a run spreads 150 ... 700 iterations around a mean of 280 (65 536 tracking instances, 20 steps) and four tiles per wave slot in index order end
    // 33 % above even slots; ordered by the previous step's counts 15 % (tests/fuzz/sim_history_dispatch.py)
    const bool history = eligible && dispatch_effective(tb) == 2 && (run || budget_max(tb) > 1);
    // a run that starts from a reset workspace goes by the predictor of its first, cold solve (which is also its longest: 22 iterations against 11): steps 0 - 19
    // of the tracking loop, makespan 1 522 iterations in index order, 1 299 by the predictor (by the true first-step counts 1 291; 16-lane kernel 2 336 -> 2 175)
    const bool want_predicted = run ? (tb->dispatch_mode == 1 || (tb->dispatch_mode == -1 && from_reset)) : dispatch_effective(tb) == 1;
    // (per-instance models: the predictor sweep reads the shared fma gains, which are unset or stale there — such a launch keeps index order)
    // (per-instance settings: the predictor assumes one tolerance and one budget for the batch — index order)
    const bool predicted = eligible && want_predicted && !history && !pl.pm && !pl.ps && !tb->dual32 && tb->max_iter > 1;
    if (traits(pl.kernel).order_unit_solve == 16) P.order = nullptr; // a caller's order lists groups of four instances, not tiles of sixteen
    // tile16 from a reset workspace: tiles formed from instances of one window start; the predictor's keys are then those tiles' keys
    P.inst_map = (!run && tb->tile_map && tile_grouping_wanted(tb, pl)) ? tb->tile_map : nullptr;
    hipError_t e = hipSuccess;
    if (history) e = launch_dispatch_order_history(tb->iter, tb->batch, unit, tb->order_buf, tb->n_unsolved, tb->stream, run && unit == 16);
    else if (predicted)
    {
        RowParams K;
        fill_row_params(tb, K, false); // fma gains
        K.inst_map = P.inst_map;
        e = launch_dispatch_order(tb->nx, tb->nu, tb->h16, K, tb->key_buf, tb->order_buf, tb->stream, unit == 16);
    }
    else HIP_TRY(hipMemsetAsync(tb->n_unsolved, 0, 2 * sizeof(int), tb->stream));
    if (e != hipSuccess) return fail(TINY_BATCH_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (history || predicted) P.order = tb->order_buf;
    return history ? 3 : predicted ? 1 : (P.order ? 2 : 0);
}

// the ONE place that launches a solve kernel.  P: the row-layout arguments (the two TILE-layout kernels take theirs from fill_solve_params)
// S: the on-chip loop of a simulated run (16-lane kernel only)
hipError_t launch_kernel(const TinyBatch *tb, const KernelPlan &pl, RowParams &P, const SimParams *S)
{
    const int nx = tb->nx, nu = tb->nu, N = tb->N;
    if (S && (pl.kernel != Kernel::Rowlane || pl.ps)) return hipErrorInvalidValue;
    if (pl.ps && pl.kernel != Kernel::Rowlane && pl.kernel != Kernel::Rowstream && pl.kernel != Kernel::Wavestream && pl.kernel != Kernel::Waveres)
        return hipErrorInvalidValue; // a missing ps kernel is an error, never another kernel
    switch (pl.kernel)
    {
    case Kernel::Rowlane:
        if (S)
        {
            const ModelParams M = pl.pm ? model_params(tb, pl) : ModelParams{};
            return launch_admm_rowsim(nx, nu, N, pl.exact, P, pl.pm ? &M : nullptr, *S, tb->stream);
        }
        if (pl.ps) return launch_admm_rowlane_ps(nx, nu, N, pl.exact, P, SettingsParams{tb->ps_dev}, tb->stream);
        return pl.pm ? launch_admm_rowlane_pm(nx, nu, N, pl.exact, P, model_params(tb, pl), tb->stream) : launch_admm_rowlane(nx, nu, N, pl.exact, tb->h16, P, tb->stream);
    case Kernel::Rowloop: return launch_admm_rowloop(nx, nu, pl.exact, tb->h16, P, tb->stream);
    case Kernel::Rowstream:
        if (pl.ps) return launch_admm_rowstream_ps(nx, nu, pl.exact, tb->h16, P, SettingsParams{tb->ps_dev}, tb->stream);
        return launch_admm_rowstream(nx, nu, pl.exact, tb->h16, P, tb->stream);
    case Kernel::Wavestream:
        if (pl.ps) return launch_admm_wavestream_ps(nx, nu, P, SettingsParams{tb->ps_dev}, tb->stream);
        return pl.pm ? launch_admm_wavestream_pm(nx, nu, P, model_params(tb, pl), tb->stream) : launch_admm_wavestream(nx, nu, P, tb->stream);
    case Kernel::Quadlane: return launch_admm_quadlane(N, pl.exact, tb->h16, P, tb->stream);
    case Kernel::Waveres:
        if (pl.ps) return launch_admm_waveres_ps(nx, nu, pl.exact, P, SettingsParams{tb->ps_dev}, tb->stream);
        return pl.pm ? launch_admm_waveres_pm(nx, nu, pl.exact, P, model_params(tb, pl), tb->stream) : launch_admm_waveres(nx, nu, pl.exact, P, tb->stream);
    case Kernel::Tile48: return launch_admm_tile48(N, pl.exact, P, tb->stream);
    case Kernel::Tile16:
    {
        if (!pl.pi) return launch_admm_tile16(N, pl.exact, P, tb->stream, tb->n_cu, tb->tile_queue);
        const Tile16Pi &t = pl.pi_tables;
        P.pi_flags = t.flags;
        // ring tables are read from their tile images (a window of the trajectory table through the ring: from the table's rows)
        if (t.bounds_ring && (t.flags & 1u))
        {
            if (!tb->r_bounds_img) return hipErrorInvalidValue;
            P.bounds = tb->r_bounds_img;
        }
        if (t.xref_ring && (t.flags & 2u))
        {
            if (!tb->r_xref_img) return hipErrorInvalidValue;
            P.xref = tb->r_xref_img;
        }
        return launch_admm_tile16_pi(N, pl.exact, t.bounds_ring, t.xref_ring, P, tb->stream, tb->n_cu, tb->tile_queue);
    }
    case Kernel::Stream:
    case Kernel::Generic:
    {
        SolveParams S;
        fill_solve_params(tb, S);
        if (pl.kernel == Kernel::Stream) return launch_admm_stream(tb->NXC, tb->NUC, S, tb->stream);
        return pl.pm ? launch_admm_generic_pm(S, model_params(tb, pl), tb->NXC, tb->NUC, tb->stream) : launch_admm_generic(S, tb->gen_mats, tb->NXC, tb->NUC, tb->stream);
    }
    }
    return hipErrorInvalidValue;
}

// the stream operations of one solve launch: dispatch order or counter reset + kernel launch (capturable).  run: the launch is the on-chip loop of that run
// (Loop::OnChip; NULL for a lone solve and for each solve of a replayed run): it differs in what the kernel is told and in its dispatch order, and is never timed
int enqueue_solve(TinyBatch *tb, const KernelPlan &pl, bool record_events, const RunArgs *run)
{
    const KernelTraits &t = traits(pl.kernel);
    RowParams P;
    SimParams S;
    if (t.layout == LAYOUT_ROW)
    {
        fill_row_params(tb, P, pl.exact);
        if (run)
        {
            P.mpc_steps = run->steps; P.window_advance = run->window_advance; P.u0_traj = run->d_u0_traj;
            P.iter_log = run->d_iter_log; P.status_log = run->d_status_log;
            if (tb->plant_mode) { S.plant = tb->plant_rows; S.plant_stride = tb->plant_mode == 2 ? (unsigned)plant_row_floats(tb->nx, tb->nu) : 0u; }
            S.w = run->d_w; S.x_traj = run->d_x_traj;
        }
        const int applied = enqueue_dispatch_order(tb, pl, run ? run->steps : 1, run && run->from_reset, P);
        if (applied < 0) return applied;
        tb->last_dispatch = applied;
    }
    else HIP_TRY(hipMemsetAsync(tb->n_unsolved, 0, 2 * sizeof(int), tb->stream)); // [0] unsolved count
    tb->last_grouped = t.layout == LAYOUT_ROW && P.inst_map != nullptr; // (never in a run: the map forms the tiles of a lone solve only)
    if (record_events) HIP_TRY(hipEventRecord(tb->ev0, tb->stream)); // the events bracket the solve kernel itself
    if (t.layout == LAYOUT_ROW && P.dual32 && !t.fp32_duals) // (an on-chip run never meets this: fp32 storage only)
        return fail(TINY_BATCH_EUNSUPPORTED, "fp16 storage with fp32 duals runs on the register-resident 16-lane and quad kernels only "
                                             "(batch-shared bounds, no optional terms, no forced row kernel)");
    // (tile16 gets tb->tile_queue in a run like in a lone solve: its two-ended queue is off whenever mpc_steps > 1 — t16_tail_stride returns 0 — so the setting changes nothing there)
    const hipError_t e = launch_kernel(tb, pl, P, run && pl.sim ? &S : nullptr);
    if (e != hipSuccess) return fail(TINY_BATCH_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (record_events)
    {
        HIP_TRY(hipEventRecord(tb->ev1, tb->stream));
        tb->ev_valid = true;
    }
    // consumed by the kernel's first iteration; iter[] now holds this launch's counts (a run's: its last solve's)
    if (budget_max(tb) > 0) { tb->duals_zero_pending = tb->cold_pending = false; tb->iter_history = true; }
    return 0;
}

// d_w / d_x_traj: this step's [batch][nx] rows (NULL: no disturbance / not recorded).  With neither and no plant set: the launch it has always been
int enqueue_plant_step(TinyBatch *tb, int window_advance, const float *d_w, float *d_x_traj)
{
    if (tb->xref_mode == 1 && window_advance) tb->tile_map_dirty = true; // the kernel slides xref_start[]
    // priority: the plant, then the per-instance model record, then the shared model (launch_plant_step picks the kernel by what is set here)
    const bool plant = tb->plant_mode != 0, per = tb->plant_mode == 2;
    PlantStepArgs a;
    a.x0buf = tb->x0buf;
    a.xarr = work_ptr(tb, TINY_ARR_X);
    a.uarr = work_ptr(tb, TINY_ARR_U);
    a.A = plant ? tb->plant_A : tb->dA;
    a.Bm = plant ? tb->plant_B : tb->dB;
    a.plant = plant;
    a.a_stride = per ? (unsigned)(tb->nx * tb->nx) : 0u;
    a.b_stride = per ? (unsigned)(tb->nx * tb->nu) : 0u;
    a.recs = (!plant && tb->pm) ? tb->pm_src : nullptr;
    a.w = d_w;
    a.x_traj = d_x_traj;
    a.wstart = tb->xref_mode == 1 ? tb->xref_start : nullptr;
    a.window_advance = window_advance;
    a.batch = tb->batch;
    a.layout = tb->layout;
    a.g = geo(tb);
    a.h16 = h16_of(tb, tb->layout);
    HIP_TRY(launch_plant_step(a, tb->stream));
    return 0;
}

// Per-instance settings: the device records and flag arrays from the caller's arrays and, for a field given as NULL, the batch's value; the budgets' range and
// the flags' uniformity for the host's decisions.  Called by tiny_batch_set_instance_settings and, while they are in force, by tiny_batch_set_settings
int rebuild_instance_settings(TinyBatch *tb)
{
    TRY(set_device(tb));
    invalidate_graph(tb);
    HIP_TRY(hipStreamSynchronize(tb->stream)); // a launch still reading the old records may be in flight
    const int B = tb->batch;
    std::vector<InstSettings> rec((size_t)tb->bpad4, InstSettings{0.f, 0.f, 0, 1}); // (the padding rows of the last wave run nothing)
    std::vector<int> flags(2 * (size_t)B);
    for (int b = 0; b < B; b++)
    {
        rec[b].abs_pri_tol = tb->ps_pri.empty() ? tb->abs_pri_tol : tb->ps_pri[b];
        rec[b].abs_dua_tol = tb->ps_dua.empty() ? tb->abs_dua_tol : tb->ps_dua[b];
        rec[b].max_iter = tb->ps_max_iter.empty() ? tb->max_iter : tb->ps_max_iter[b];
        rec[b].check_termination = tb->ps_check.empty() ? tb->check_termination : tb->ps_check[b];
        flags[b] = (tb->ps_en_state.empty() ? tb->en_state_bound : tb->ps_en_state[b]) ? 1 : 0;
        flags[(size_t)B + b] = (tb->ps_en_input.empty() ? tb->en_input_bound : tb->ps_en_input[b]) ? 1 : 0;
    }
    tb->ps_budget_max = tb->ps_budget_min = rec[0].max_iter;
    tb->ps_flags_vary = false;
    for (int b = 1; b < B; b++)
    {
        tb->ps_budget_max = std::max(tb->ps_budget_max, rec[b].max_iter);
        tb->ps_budget_min = std::min(tb->ps_budget_min, rec[b].max_iter);
        if (flags[b] != flags[0] || flags[(size_t)B + b] != flags[B]) tb->ps_flags_vary = true;
    }
    tb->ps_en_state_all = flags[0]; tb->ps_en_input_all = flags[B]; // read only while the flags are uniform
    if (!tb->ps_dev) HIP_TRY(guarded_malloc((void **)&tb->ps_dev, rec.size() * sizeof(InstSettings)));
    HIP_TRY(hipMemcpy(tb->ps_dev, rec.data(), rec.size() * sizeof(InstSettings), hipMemcpyHostToDevice));
    if (!tb->ps_flags_dev) HIP_TRY(guarded_malloc((void **)&tb->ps_flags_dev, flags.size() * sizeof(int)));
    HIP_TRY(hipMemcpy(tb->ps_flags_dev, flags.data(), flags.size() * sizeof(int), hipMemcpyHostToDevice));
    tb->ps = true;
    tb->derived_dirty[LAYOUT_ROW] = true; // the bound flags are folded into the {lo, hi} table
    return 0;
}

int set_bound(TinyBatch *tb, const float *src, int shared, int which)
{
    CHECK_TB(tb);
    CHECK_PTR(src);
    TRY(set_device(tb));
    const bool xf = which < 2;
    return store_input(tb, tb->in_bnd[which], src, shared != 0, xf ? tb->N : tb->N - 1, xf ? tb->nx : tb->nu);
}

// The MFMA streaming kernel is instantiated per (chunks of 4 state rows, chunks of 4 input rows).  A class without its own
// instantiation runs on the smallest one that contains it: the extra chunks are rows that do not exist (zero gains, zero
// state, no bounds — exactly like the unused rows of a partly filled chunk), so any nx <= 64, nu <= 32 is served.
bool stream_dims_supported(int nxc, int nuc, int *pxc, int *puc)
{
    int best = 1 << 30;
    bool found = false;
#define TINY_CHECK_DIMS(NXC, NUC)                                        \
    if (nxc <= NXC && nuc <= NUC && (NXC + NUC) * 64 + NXC < best)       \
    {                                                                    \
        best = (NXC + NUC) * 64 + NXC; *pxc = NXC; *puc = NUC; found = true; \
    }
    TINY_FOR_EACH_DIMS(TINY_CHECK_DIMS)
    return found;
}

} // namespace

extern "C"
{

const char *tiny_batch_last_error(void) { return g_err.c_str(); }

int tiny_batch_create(TinyBatch **out, int nx, int nu, int N, int batch, int device)
{
    CHECK_PTR(out);
    *out = nullptr;
    if (nx < 1 || nu < 1 || N < 2 || batch < 1)
        return fail(TINY_BATCH_EINVAL, "tiny_batch_create: need nx>=1, nu>=1, N>=2, batch>=1 (got %d,%d,%d,%d)", nx, nu, N, batch);
    int nxc = (nx + 3) / 4, nuc = (nu + 3) / 4;
    // the rowlane kernel addresses its arrays with 32-bit element offsets
    const bool tile_ok = stream_dims_supported(nxc, nuc, &nxc, &nuc),
               row_ok = rowlane_supported(nx, nu, N) && ((long long)(batch + 3) * N * 16 < (1ll << 30));
    const bool wave_ok = !rowdims_supported(nx, nu) && wavedims_supported(nx, nu) && ((long long)(batch + 3) * N * 64 < (1ll << 30));
    if (!tile_ok && !row_ok && !rowdims_supported(nx, nu) && !wave_ok)
        return fail(TINY_BATCH_EUNSUPPORTED,
                    "no kernel for nx=%d nu=%d N=%d: exact arithmetic needs a compiled class (TINY_FOR_EACH_ROWDIMS / _WAVEDIMS), fma arithmetic nx <= 64 and nu <= 32",
                    nx, nu, N);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(TINY_BATCH_EINVAL, "device %d out of range (have %d)", device, ndev);
    TinyBatch *tb = new TinyBatch();
    tb->nx = nx; tb->nu = nu; tb->N = N; tb->batch = batch; tb->device = device;
    tb->NXC = nxc; tb->NUC = nuc; tb->ntiles = (batch + TILE - 1) / TILE; tb->bpad4 = (batch + 3) / 4 * 4;
    tb->tile_dims_ok = tile_ok; tb->row_dims_ok = row_ok;
    tb->rowmath_ok = rowdims_supported(nx, nu) && ((long long)(batch + 3) * N * 16 < (1ll << 30));
    tb->rowloop_ok = tb->rowmath_ok && rowloop_supported(nx, nu, N);
    tb->wave_ok = wave_ok;
    tb->quad_ok = tb->rowmath_ok && quadlane_supported(nx, nu, N);
    tb->tile16_ok = tb->rowmath_ok && tile16_supported(nx, nu, N);
    tb->waveres_ok = wave_ok && waveres_supported(nx, nu, N);
    tb->tile48_ok = wave_ok && tile48_supported(nx, nu, N);
    tb->generic_ok = tile_ok && generic_exact_supported(nx, nu);
    tb->rw = wave_ok ? 64 : 16;
    tb->xfam_floats = (size_t)tb->ntiles * N * WAVE * nxc;
    tb->ufam_floats = (size_t)tb->ntiles * (N - 1) * WAVE * nuc;
    tb->pair_floats = (size_t)tb->bpad4 * N * tb->rw;
    tb->layout = (row_ok || wave_ok || !tile_ok) ? LAYOUT_ROW : LAYOUT_TILE;
    auto cleanup = [&](int rc) { tiny_batch_destroy(tb); return rc; };
    if (hipSetDevice(device) != hipSuccess) return cleanup(fail(TINY_BATCH_EHIP, "hipSetDevice(%d) failed", device));
    {
        int ncu = 0; // of THIS handle's device (round-3 advisor: a process-wide static used to cache whichever device was current first)
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0) tb->n_cu = ncu;
    }
    if (int rc = alloc_layout(tb, tb->layout)) return cleanup(rc);
    if (int rc = dev_alloc_zero(&tb->res, (size_t)batch * 4)) return cleanup(rc);
    if (int rc = dev_alloc_zero((float **)&tb->status, batch)) return cleanup(rc);
    if (int rc = dev_alloc_zero((float **)&tb->iter, batch)) return cleanup(rc);
    if (int rc = dev_alloc_zero((float **)&tb->n_unsolved, 2)) return cleanup(rc);
    if (int rc = dev_alloc_zero((float **)&tb->xref_start, batch)) return cleanup(rc);
    if (int rc = dev_alloc_zero(&tb->x0buf, (size_t)batch * nx)) return cleanup(rc);
    tb->staging_floats = (size_t)batch * N * (nx > nu ? nx : nu);
    if (int rc = dev_alloc_zero(&tb->staging, tb->staging_floats)) return cleanup(rc);
    if (hipEventCreate(&tb->ev0) != hipSuccess || hipEventCreate(&tb->ev1) != hipSuccess)
        return cleanup(fail(TINY_BATCH_EHIP, "hipEventCreate failed"));
    tb->cold_pending = true; // a fresh workspace IS a reset one (every array was allocated zero): its first solve is a cold start, like one after tiny_batch_reset_workspace
    *out = tb;
    return TINY_BATCH_OK;
}

void tiny_batch_destroy(TinyBatch *tb)
{
    if (!tb) return;
    (void)hipSetDevice(tb->device);
    free_layout(tb, LAYOUT_TILE);
    free_layout(tb, LAYOUT_ROW);
    (void)guarded_free(tb->in_xref.dev);
    (void)guarded_free(tb->in_uref.dev); (void)guarded_free(tb->r_uref);
    (void)guarded_free(tb->key_buf); (void)guarded_free(tb->order_buf); (void)guarded_free(tb->u0_stage);
    for (int k = 0; k < 4; k++) { (void)guarded_free(tb->in_bnd[k].dev); (void)guarded_free(tb->t_bnd[k]); }
    (void)guarded_free(tb->t_xref); (void)guarded_free(tb->r_xref); (void)guarded_free(tb->r_bounds); (void)guarded_free((float *)tb->rows_vary_dev); (void)guarded_free((float *)tb->zero_ties_dev);
    (void)guarded_free(tb->r_bounds_img); (void)guarded_free(tb->r_xref_img);
    (void)guarded_free(tb->tab_tile); (void)guarded_free(tb->tab_row); (void)guarded_free(tb->tab_row_h); (void)guarded_free(tb->xref_start); (void)guarded_free(tb->tile_map);
    (void)guarded_free(tb->res); (void)guarded_free(tb->status); (void)guarded_free(tb->iter); (void)guarded_free(tb->n_unsolved);
    (void)guarded_free(tb->opnd); (void)guarded_free(tb->qvec); (void)guarded_free(tb->gen_mats); (void)guarded_free(tb->mats_exact); (void)guarded_free(tb->mats_fast);
    (void)guarded_free(tb->pm_src); (void)guarded_free(tb->pm_rho); (void)guarded_free(tb->pm_row[0]); (void)guarded_free(tb->pm_row[1]);
    (void)guarded_free(tb->pm_wave[0]); (void)guarded_free(tb->pm_wave[1]);
    (void)guarded_free(tb->plant_A); (void)guarded_free(tb->plant_B); (void)guarded_free(tb->plant_rows);
    (void)guarded_free(tb->ps_dev); (void)guarded_free(tb->ps_flags_dev);
    for (float *p : tb->sim_stage) (void)guarded_free(p);
    (void)guarded_free(tb->dA); (void)guarded_free(tb->dB); (void)guarded_free(tb->x0buf); (void)guarded_free(tb->staging); (void)guarded_free(tb->conv_dev);
    if (tb->graph_exec) (void)hipGraphExecDestroy(tb->graph_exec);
    if (tb->own_stream) (void)hipStreamDestroy(tb->own_stream);
    if (tb->ev0) (void)hipEventDestroy(tb->ev0);
    if (tb->ev1) (void)hipEventDestroy(tb->ev1);
    delete tb;
}

int tiny_batch_set_stream(TinyBatch *tb, void *hip_stream)
{
    CHECK_TB(tb);
    invalidate_graph(tb); // synchronises the stream a replay may still be running on: before that stream is replaced
    tb->stream = (hipStream_t)hip_stream;
    return 0;
}

int tiny_batch_synchronize(TinyBatch *tb)
{
    CHECK_TB(tb);
    TRY(set_device(tb));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    return 0;
}

int tiny_batch_set_cache(TinyBatch *tb, float rho, const float *Kinf, const float *Pinf, const float *Quu_inv,
                         const float *AmBKt)
{
    CHECK_TB(tb); CHECK_PTR(Kinf); CHECK_PTR(Pinf); CHECK_PTR(Quu_inv); CHECK_PTR(AmBKt);
    const int nx = tb->nx, nu = tb->nu;
    tb->rho = rho;
    tb->Kinf.assign(Kinf, Kinf + (size_t)nu * nx);
    tb->Pinf.assign(Pinf, Pinf + (size_t)nx * nx);
    tb->Quu_inv.assign(Quu_inv, Quu_inv + (size_t)nu * nu);
    tb->AmBKt.assign(AmBKt, AmBKt + (size_t)nx * nx);
    tb->have_cache = true;
    tb->gains_dirty = true;
    invalidate_graph(tb); // rho is a kernel argument
    return 0;
}

int tiny_batch_set_dynamics(TinyBatch *tb, const float *Adyn, const float *Bdyn, const float *Q)
{
    CHECK_TB(tb); CHECK_PTR(Adyn); CHECK_PTR(Bdyn); CHECK_PTR(Q);
    const int nx = tb->nx, nu = tb->nu;
    tb->Adyn.assign(Adyn, Adyn + (size_t)nx * nx);
    tb->Bdyn.assign(Bdyn, Bdyn + (size_t)nx * nu);
    tb->Q.assign(Q, Q + nx);
    tb->have_dyn = true;
    tb->gains_dirty = true;
    invalidate_graph(tb);
    return 0;
}

// ---- per-instance models ----------------------------------------------------------------------------------------------------
int tiny_batch_set_models_device(TinyBatch *tb, const float *d_rho, const float *d_Kinf, const float *d_Pinf, const float *d_Quu_inv,
                                 const float *d_AmBKt, const float *d_Adyn, const float *d_Bdyn, const float *d_Q)
{
    CHECK_TB(tb); CHECK_PTR(d_rho); CHECK_PTR(d_Kinf); CHECK_PTR(d_Pinf); CHECK_PTR(d_Quu_inv); CHECK_PTR(d_AmBKt); CHECK_PTR(d_Adyn); CHECK_PTR(d_Bdyn); CHECK_PTR(d_Q);
    TRY(set_device(tb));
    invalidate_graph(tb); // the record pointers and the kernel choice are baked into a captured graph
    const long long n = (long long)tb->batch * pm_gen_floats(tb->nx, tb->nu);
    if (!tb->pm_src) HIP_TRY(guarded_malloc((void **)&tb->pm_src, (size_t)n * sizeof(float)));
    if (!tb->pm_rho) HIP_TRY(guarded_malloc((void **)&tb->pm_rho, (size_t)tb->batch * sizeof(float)));
    HIP_TRY(launch_models_gather(d_rho, d_Kinf, d_Pinf, d_Quu_inv, d_AmBKt, d_Adyn, d_Bdyn, d_Q, tb->pm_src, tb->pm_rho, tb->batch, tb->nx, tb->nu, tb->stream));
    tb->pm = true;
    tb->pm_row_dirty[0] = tb->pm_row_dirty[1] = tb->pm_wave_dirty[0] = tb->pm_wave_dirty[1] = true; // the packed rows follow the records
    return 0;
}

namespace
{
// the [B] arrays of tiny_batch_set_models, one after the other in one buffer of floats: rho | Kinf | Pinf | Quu_inv | AmBKt | Adyn | Bdyn | Q
int set_models_packed(TinyBatch *tb, const float *d)
{
    const size_t B = tb->batch, nx = tb->nx, nu = tb->nu;
    const float *p = d;
    const float *rho = p; p += B;
    const float *K = p; p += B * nu * nx;
    const float *Pf = p; p += B * nx * nx;
    const float *Qi = p; p += B * nu * nu;
    const float *Am = p; p += B * nx * nx;
    const float *A = p; p += B * nx * nx;
    const float *Bm = p; p += B * nx * nu;
    return tiny_batch_set_models_device(tb, rho, K, Pf, Qi, Am, A, Bm, p);
}
} // namespace

int tiny_batch_set_models(TinyBatch *tb, const float *rho, const float *Kinf, const float *Pinf, const float *Quu_inv, const float *AmBKt,
                          const float *Adyn, const float *Bdyn, const float *Q)
{
    CHECK_TB(tb); CHECK_PTR(rho); CHECK_PTR(Kinf); CHECK_PTR(Pinf); CHECK_PTR(Quu_inv); CHECK_PTR(AmBKt); CHECK_PTR(Adyn); CHECK_PTR(Bdyn); CHECK_PTR(Q);
    TRY(set_device(tb));
    const size_t B = tb->batch, nx = tb->nx, nu = tb->nu;
    const float *src[8] = {rho, Kinf, Pinf, Quu_inv, AmBKt, Adyn, Bdyn, Q};
    const size_t sz[8] = {B, B * nu * nx, B * nx * nx, B * nu * nu, B * nx * nx, B * nx * nx, B * nx * nu, B * nx};
    size_t total = 0;
    for (size_t z : sz) total += z;
    float *d = nullptr;
    HIP_TRY(guarded_malloc((void **)&d, total * sizeof(float)));
    int rc = 0;
    size_t o = 0;
    for (int k = 0; k < 8 && rc == 0; k++)
    {
        if (hipMemcpyAsync(d + o, src[k], sz[k] * sizeof(float), hipMemcpyHostToDevice, tb->stream) != hipSuccess) rc = fail(TINY_BATCH_EHIP, "hipMemcpyAsync failed");
        o += sz[k];
    }
    if (rc == 0) rc = set_models_packed(tb, d);
    if (hipStreamSynchronize(tb->stream) != hipSuccess && rc == 0) rc = fail(TINY_BATCH_EHIP, "hipStreamSynchronize failed");
    (void)guarded_free(d);
    return rc;
}

int tiny_batch_clear_models(TinyBatch *tb)
{
    CHECK_TB(tb);
    if (!tb->pm) return 0;
    TRY(set_device(tb));
    invalidate_graph(tb);
    HIP_TRY(hipStreamSynchronize(tb->stream)); // a launch still reading the records may be in flight
    // the records and the packed rows are released (about 8 KB per quadrotor instance, 33 KB per wave table of the nx = 32 class); a later set_models
    // allocates them again
    for (float **p : {&tb->pm_src, &tb->pm_rho, &tb->pm_row[0], &tb->pm_row[1], &tb->pm_wave[0], &tb->pm_wave[1]})
    {
        (void)guarded_free(*p);
        *p = nullptr;
    }
    tb->pm_row_dirty[0] = tb->pm_row_dirty[1] = tb->pm_wave_dirty[0] = tb->pm_wave_dirty[1] = true;
    tb->pm = false;
    return 0;
}

int tiny_batch_models_per_instance(TinyBatch *tb)
{
    CHECK_TB(tb);
    return tb->pm ? 1 : 0;
}

int tiny_batch_clear_plant(TinyBatch *tb)
{
    CHECK_TB(tb);
    if (!tb->plant_mode) return 0;
    TRY(set_device(tb));
    invalidate_graph(tb);
    HIP_TRY(hipStreamSynchronize(tb->stream)); // a launch still reading the plant may be in flight
    for (float **p : {&tb->plant_A, &tb->plant_B, &tb->plant_rows})
    {
        (void)guarded_free(*p);
        *p = nullptr;
    }
    tb->plant_mode = 0;
    return 0;
}

int tiny_batch_set_plant(TinyBatch *tb, const float *A, const float *Bm, int shared)
{
    CHECK_TB(tb); CHECK_PTR(A); CHECK_PTR(Bm);
    if (tb->nx > 64) return fail(TINY_BATCH_EUNSUPPORTED, "tiny_batch_set_plant: the closed-loop calls support nx <= 64");
    TRY(set_device(tb)); // the copies below belong on the handle's device, whatever device the calling thread last selected
    TRY(tiny_batch_clear_plant(tb)); // releases the previous copies
    invalidate_graph(tb);            // (also where there was no plant before: the captured plant launches read the model's matrices)
    const size_t cnt = shared ? 1 : (size_t)tb->batch, nx = tb->nx, nu = tb->nu;
    const bool rows = nx + nu <= 16; // the 16-lane mapping: the on-chip loop reads the rows of [A | B] in the gain rows' layout, zeros on the input lanes
    const size_t rf = (size_t)plant_row_floats(tb->nx, tb->nu);
    std::vector<float> packed(rows ? cnt * rf : 0, 0.f);
    for (size_t b = 0; rows && b < cnt; b++)
        for (size_t r = 0; r < nx; r++)
        {
            for (size_t k = 0; k < nx; k++) packed[b * rf + k * 16 + r] = A[b * nx * nx + k * nx + r];
            for (size_t m = 0; m < nu; m++) packed[b * rf + (nx + m) * 16 + r] = Bm[b * nx * nu + m * nx + r];
        }
    int rc = 0;
    auto up = [&](float **dst, const float *src, size_t n)
    {
        if (rc == 0 && guarded_malloc((void **)dst, n * sizeof(float)) != hipSuccess) rc = fail(TINY_BATCH_EHIP, "tiny_batch_set_plant: device allocation failed");
        if (rc == 0 && hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) rc = fail(TINY_BATCH_EHIP, "tiny_batch_set_plant: hipMemcpy failed");
    };
    up(&tb->plant_A, A, cnt * nx * nx);
    up(&tb->plant_B, Bm, cnt * nx * nu);
    if (rows) up(&tb->plant_rows, packed.data(), cnt * rf);
    tb->plant_mode = shared ? 1 : 2;
    if (rc) (void)tiny_batch_clear_plant(tb);
    return rc;
}

int tiny_batch_plant_mode(TinyBatch *tb)
{
    CHECK_TB(tb);
    return tb->plant_mode;
}

int tiny_batch_riccati_device(int nx, int nu, int count, const double *d_A, const double *d_B, const double *d_Q, const double *d_R, const double *d_rho,
                              double *d_Kinf, double *d_Pinf, double *d_Quu_inv, double *d_AmBKt, double *d_coeff_d2p, int *d_iters, void *hip_stream)
{
    if (nx < 1 || nx > 64 || nu < 1 || nu > 32) return fail(TINY_BATCH_EINVAL, "tiny_batch_riccati_device: need 1 <= nx <= 64 and 1 <= nu <= 32 (got %d, %d)", nx, nu);
    if (count < 1) return fail(TINY_BATCH_EINVAL, "tiny_batch_riccati_device: count must be >= 1 (got %d)", count);
    CHECK_PTR(d_A); CHECK_PTR(d_B); CHECK_PTR(d_Q); CHECK_PTR(d_R); CHECK_PTR(d_rho); CHECK_PTR(d_Kinf); CHECK_PTR(d_Pinf); CHECK_PTR(d_Quu_inv);
    CHECK_PTR(d_AmBKt); CHECK_PTR(d_iters);
    hipStream_t st = (hipStream_t)hip_stream;
    // scratch for at most ~1 GiB of systems at a time, whole waves
    const size_t per = (size_t)riccati_batch_doubles(nx, nu) * sizeof(double);
    long long chunk = (long long)((1ull << 30) / per) / 64 * 64;
    if (chunk < 64) chunk = 64;
    if (chunk > (long long)(count + 63) / 64 * 64) chunk = (long long)(count + 63) / 64 * 64;
    double *scratch = nullptr;
    int *nfail = nullptr;
    HIP_TRY(guarded_malloc((void **)&scratch, (size_t)chunk * per));
    int rc = 0;
    if (guarded_malloc((void **)&nfail, sizeof(int)) != hipSuccess || hipMemsetAsync(nfail, 0, sizeof(int), st) != hipSuccess)
        rc = fail(TINY_BATCH_EHIP, "tiny_batch_riccati_device: allocation failed");
    for (long long s0 = 0; s0 < count && rc == 0; s0 += chunk)
    {
        hipError_t e = launch_riccati_batch(nx, nu, (int)s0, (int)chunk, count, d_A, d_B, d_Q, d_R, d_rho, d_Kinf, d_Pinf, d_Quu_inv, d_AmBKt, d_coeff_d2p, d_iters,
                                            scratch, nfail, st);
        if (e != hipSuccess) rc = fail(TINY_BATCH_EHIP, "kernel launch failed: %s", hipGetErrorString(e));
    }
    int h = 0;
    if (rc == 0 && hipMemcpyAsync(&h, nfail, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) rc = fail(TINY_BATCH_EHIP, "hipMemcpyAsync failed");
    if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = fail(TINY_BATCH_EHIP, "hipStreamSynchronize failed");
    (void)guarded_free(scratch);
    (void)guarded_free(nfail);
    return rc ? rc : h;
}

int tiny_batch_set_systems(TinyBatch *tb, const double *A, const double *B, const double *Q, const double *R, const double *rho, int *iters)
{
    CHECK_TB(tb); CHECK_PTR(A); CHECK_PTR(B); CHECK_PTR(Q); CHECK_PTR(R); CHECK_PTR(rho);
    TRY(set_device(tb));
    const size_t Bn = tb->batch, nx = tb->nx, nu = tb->nu;
    // inputs A | B | Q | R | rho, outputs Kinf | Pinf | Quu_inv | AmBKt, fp64; then the fp32 arrays of tiny_batch_set_models
    const size_t in_sz[5] = {Bn * nx * nx, Bn * nx * nu, Bn * nx, Bn * nu, Bn};
    const size_t out_sz[4] = {Bn * nu * nx, Bn * nx * nx, Bn * nu * nu, Bn * nx * nx};
    const double *in[5] = {A, B, Q, R, rho};
    size_t nd = 0;
    for (size_t z : in_sz) nd += z;
    for (size_t z : out_sz) nd += z;
    const size_t nf = Bn * (1 + pm_gen_floats(tb->nx, tb->nu));
    double *d = nullptr;
    float *f = nullptr;
    int *it = nullptr;
    int rc = 0;
    if (guarded_malloc((void **)&d, nd * sizeof(double)) != hipSuccess || guarded_malloc((void **)&f, nf * sizeof(float)) != hipSuccess ||
        guarded_malloc((void **)&it, Bn * sizeof(int)) != hipSuccess)
        rc = fail(TINY_BATCH_EHIP, "tiny_batch_set_systems: allocation failed");
    double *dp[9];
    size_t o = 0;
    for (int k = 0; k < 5; k++) { dp[k] = d + o; o += in_sz[k]; }
    for (int k = 0; k < 4; k++) { dp[5 + k] = d + o; o += out_sz[k]; }
    for (int k = 0; k < 5 && rc == 0; k++)
        if (hipMemcpyAsync(dp[k], in[k], in_sz[k] * sizeof(double), hipMemcpyHostToDevice, tb->stream) != hipSuccess) rc = fail(TINY_BATCH_EHIP, "hipMemcpyAsync failed");
    int nfail = 0;
    if (rc == 0)
    {
        nfail = tiny_batch_riccati_device(tb->nx, tb->nu, tb->batch, dp[0], dp[1], dp[2], dp[3], dp[4], dp[5], dp[6], dp[7], dp[8], nullptr, it, tb->stream);
        if (nfail < 0) rc = nfail;
    }
    if (rc == 0 && iters && hipMemcpy(iters, it, Bn * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(TINY_BATCH_EHIP, "hipMemcpy failed");
    if (rc == 0 && nfail > 0) rc = fail(TINY_BATCH_EINVAL, "tiny_batch_set_systems: the Riccati recursion is singular for %d of %zu systems (iters = -1); models unchanged", nfail, Bn);
    if (rc == 0 && launch_systems_to_models(dp[4], dp[5], dp[6], dp[7], dp[8], dp[0], dp[1], dp[2], f, tb->batch, tb->nx, tb->nu, tb->stream) != hipSuccess)
        rc = fail(TINY_BATCH_EHIP, "kernel launch failed");
    if (rc == 0) rc = set_models_packed(tb, f);
    if (hipStreamSynchronize(tb->stream) != hipSuccess && rc == 0) rc = fail(TINY_BATCH_EHIP, "hipStreamSynchronize failed");
    (void)guarded_free(d); (void)guarded_free(f); (void)guarded_free(it);
    return rc;
}

// ---- the two terms the reference ships commented out (admm.cpp:20 and :79), off by default ------------------------------
int tiny_batch_set_optional_terms(TinyBatch *tb, int en_uref, int en_coeff_d2p)
{
    CHECK_TB(tb);
    tb->en_uref = en_uref != 0;
    tb->en_d2p = en_coeff_d2p != 0;
    invalidate_graph(tb);
    return 0;
}

int tiny_batch_set_input_cost(TinyBatch *tb, const float *R)
{
    CHECK_TB(tb); CHECK_PTR(R);
    tb->Rcost.assign(R, R + tb->nu);
    tb->have_rcost = true;
    tb->gains_dirty = true;
    invalidate_graph(tb);
    return 0;
}

int tiny_batch_set_coeff_d2p(TinyBatch *tb, const float *coeff_d2p)
{
    CHECK_TB(tb); CHECK_PTR(coeff_d2p);
    tb->coeff_d2p.assign(coeff_d2p, coeff_d2p + (size_t)tb->nx * tb->nu);
    tb->gains_dirty = true;
    invalidate_graph(tb);
    return 0;
}

int tiny_batch_set_uref(TinyBatch *tb, const float *uref, int shared)
{
    CHECK_TB(tb); CHECK_PTR(uref);
    TRY(set_device(tb));
    TRY(store_input(tb, tb->in_uref, uref, shared != 0, tb->N - 1, tb->nu));
    return 0;
}

int tiny_batch_set_dispatch(TinyBatch *tb, int mode)
{
    CHECK_TB(tb);
    if (mode < -1 || mode > 2) return fail(TINY_BATCH_EINVAL, "tiny_batch_set_dispatch: mode must be 0 (index order), 1 (longest first, predicted), 2 (longest first by the previous solve's iteration counts) or -1 (automatic)");
    tb->dispatch_mode = mode;
    invalidate_graph(tb);
    return 0;
}

int tiny_batch_set_tile_queue(TinyBatch *tb, int stride)
{
    CHECK_TB(tb);
    if (stride < -1 || stride > 255) return fail(TINY_BATCH_EINVAL, "tiny_batch_set_tile_queue: stride must be -1 (automatic), 0 (one counter) or 1 .. 255");
    tb->tile_queue = stride;
    invalidate_graph(tb);
    return TINY_BATCH_OK;
}

int tiny_batch_set_tile_grouping(TinyBatch *tb, int mode)
{
    CHECK_TB(tb);
    if (mode < -1 || mode > 1) return fail(TINY_BATCH_EINVAL, "tiny_batch_set_tile_grouping: mode must be -1 (automatic), 0 (off) or 1 (by window start)");
    tb->tile_grouping = mode;
    invalidate_graph(tb);
    return TINY_BATCH_OK;
}

int tiny_batch_tile_grouping_applied(TinyBatch *tb)
{
    CHECK_TB(tb);
    return tb->last_grouped ? 1 : 0;
}

int tiny_batch_get_tile_map(TinyBatch *tb, int *map, int *builds)
{
    CHECK_TB(tb);
    if (builds) *builds = tb->tile_map_builds;
    if (!tb->tile_map) return 0;
    const int n = (tb->batch + 15) / 16 * 16;
    if (map)
    {
        TRY(set_device(tb));
        HIP_TRY(hipMemcpyAsync(map, tb->tile_map, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, tb->stream));
        HIP_TRY(hipStreamSynchronize(tb->stream));
    }
    return n;
}

int tiny_batch_dispatch_applied(TinyBatch *tb)
{
    CHECK_TB(tb);
    return tb->last_dispatch;
}

int tiny_batch_set_dispatch_order_device(TinyBatch *tb, const int *d_order)
{
    CHECK_TB(tb);
    tb->order_dev = d_order;
    invalidate_graph(tb); // (a caller's order keeps the 16-lane kernel it is written for)
    return 0;
}

int tiny_batch_set_settings(TinyBatch *tb, float abs_pri_tol, float abs_dua_tol, int max_iter, int check_termination,
                            int en_state_bound, int en_input_bound)
{
    CHECK_TB(tb);
    if (check_termination < 1)
        return fail(TINY_BATCH_EINVAL, "check_termination must be >= 1 (the reference computes iter %% check_termination, admm.cpp:93)");
    if (tb->en_state_bound != en_state_bound || tb->en_input_bound != en_input_bound) tb->derived_dirty[LAYOUT_ROW] = true;
    tb->abs_pri_tol = abs_pri_tol; tb->abs_dua_tol = abs_dua_tol;
    tb->max_iter = max_iter; tb->check_termination = check_termination;
    tb->en_state_bound = en_state_bound; tb->en_input_bound = en_input_bound;
    tb->have_settings = true; // tolerances, max_iter, check_termination and the bound flags are in the graph signature
    return tb->ps ? rebuild_instance_settings(tb) : 0; // (the fields a per-instance call left NULL follow the batch's values)
}

int tiny_batch_set_instance_settings(TinyBatch *tb, const float *abs_pri_tol, const float *abs_dua_tol, const int *max_iter, const int *check_termination,
                                     const int *en_state_bound, const int *en_input_bound)
{
    CHECK_TB(tb);
    if (!tb->have_settings) return fail(TINY_BATCH_ENOTREADY, "tiny_batch_set_instance_settings: tiny_batch_set_settings must be called first (a NULL field keeps its value)");
    if (check_termination)
        for (int b = 0; b < tb->batch; b++)
            if (check_termination[b] < 1)
                return fail(TINY_BATCH_EINVAL, "check_termination[%d] = %d: must be >= 1 (the reference computes iter %% check_termination, admm.cpp:93)", b, check_termination[b]);
    const size_t B = (size_t)tb->batch;
    auto take = [B](auto &dst, const auto *src) { if (src) dst.assign(src, src + B); else dst.clear(); };
    take(tb->ps_pri, abs_pri_tol); take(tb->ps_dua, abs_dua_tol);
    take(tb->ps_max_iter, max_iter); take(tb->ps_check, check_termination);
    take(tb->ps_en_state, en_state_bound); take(tb->ps_en_input, en_input_bound);
    return rebuild_instance_settings(tb);
}

int tiny_batch_clear_instance_settings(TinyBatch *tb)
{
    CHECK_TB(tb);
    if (!tb->ps) return 0;
    TRY(set_device(tb));
    invalidate_graph(tb);
    HIP_TRY(hipStreamSynchronize(tb->stream)); // a launch still reading the records may be in flight
    (void)guarded_free(tb->ps_dev); tb->ps_dev = nullptr;
    (void)guarded_free(tb->ps_flags_dev); tb->ps_flags_dev = nullptr;
    for (std::vector<float> *v : {&tb->ps_pri, &tb->ps_dua}) v->clear();
    for (std::vector<int> *v : {&tb->ps_max_iter, &tb->ps_check, &tb->ps_en_state, &tb->ps_en_input}) v->clear();
    tb->ps = tb->ps_flags_vary = false;
    tb->derived_dirty[LAYOUT_ROW] = true; // the bounds table is the batch flags' again
    return 0;
}

int tiny_batch_settings_per_instance(TinyBatch *tb)
{
    CHECK_TB(tb);
    return tb->ps ? 1 : 0;
}

int tiny_batch_set_x0(TinyBatch *tb, const float *x0)
{
    CHECK_TB(tb); CHECK_PTR(x0);
    TRY(set_device(tb));
    tb->x0_zero_pending = false; // all of x.col(0) and x0buf is overwritten
    HIP_TRY(hipMemcpyAsync(tb->x0buf, x0, (size_t)tb->batch * tb->nx * sizeof(float), hipMemcpyHostToDevice, tb->stream));
    return upload_work(tb, x0, TINY_ARR_X, 0, 1);
}

int tiny_batch_set_x0_device(TinyBatch *tb, const float *d_x0)
{
    CHECK_TB(tb); CHECK_PTR(d_x0);
    TRY(set_device(tb));
    tb->x0_zero_pending = false; // all of x.col(0) and x0buf is overwritten
    return launch_pack(tb, d_x0, work_ptr(tb, TINY_ARR_X), tb->layout, 0, tb->batch, false, 0, 1, tb->x0buf); // x.col(0) and the state buffer in one launch
}

int tiny_batch_set_xref(TinyBatch *tb, const float *xref, int shared)
{
    CHECK_TB(tb); CHECK_PTR(xref);
    TRY(set_device(tb));
    TRY(store_input(tb, tb->in_xref, xref, shared != 0, tb->N, tb->nx));
    tb->xref_mode = 0;
    return 0;
}

int tiny_batch_set_xref_window(TinyBatch *tb, const float *table, int rows, const int *start)
{
    CHECK_TB(tb); CHECK_PTR(table); CHECK_PTR(start);
    if (rows < tb->N) return fail(TINY_BATCH_EINVAL, "trajectory table has %d rows, need at least N=%d", rows, tb->N);
    for (int b = 0; b < tb->batch; b++)
        if (start[b] < 0 || start[b] + tb->N > rows)
            return fail(TINY_BATCH_EINVAL, "window start[%d]=%d out of range for %d rows, N=%d", b, start[b], rows, tb->N);
    TRY(set_device(tb));
    // table on the device in both forms: [rows][4 gq][NXC] (streaming kernel) and [rows][rw] (row / wave kernels)
    std::vector<float> tt((size_t)rows * 4 * tb->NXC, 0.f), tr((size_t)rows * tb->rw, 0.f);
    for (int r = 0; r < rows; r++)
        for (int row = 0; row < tb->nx; row++)
        {
            const float v = table[(size_t)r * tb->nx + row];
            tt[((size_t)r * 4 + (row & 3)) * tb->NXC + (row >> 2)] = v;
            if (row < tb->rw) tr[(size_t)r * tb->rw + row] = v;
        }
    if (tb->table_rows != rows)
    {
        (void)guarded_free(tb->tab_tile); (void)guarded_free(tb->tab_row); (void)guarded_free(tb->tab_row_h);
        tb->tab_tile = tb->tab_row = tb->tab_row_h = nullptr;
    }
    TRY(upload_vec(tb, &tb->tab_tile, tt));
    TRY(upload_vec(tb, &tb->tab_row, tr));
    {
        std::vector<_Float16> th(tr.size());
        for (size_t e = 0; e < tr.size(); e++) th[e] = (_Float16)tr[e];
        std::vector<float> packed(tr.size() / 2); // rows * rw halves
        std::memcpy(packed.data(), th.data(), packed.size() * sizeof(float));
        TRY(upload_vec(tb, &tb->tab_row_h, packed));
    }
    HIP_TRY(hipMemcpyAsync(tb->xref_start, start, (size_t)tb->batch * sizeof(int), hipMemcpyHostToDevice, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    tb->table_rows = rows;
    tb->xref_mode = 1;
    tb->tile_map_dirty = true;
    invalidate_graph(tb);
    return 0;
}

int tiny_batch_set_xmin(TinyBatch *tb, const float *s, int shared) { return set_bound(tb, s, shared, 0); }
int tiny_batch_set_xmax(TinyBatch *tb, const float *s, int shared) { return set_bound(tb, s, shared, 1); }
int tiny_batch_set_umin(TinyBatch *tb, const float *s, int shared) { return set_bound(tb, s, shared, 2); }
int tiny_batch_set_umax(TinyBatch *tb, const float *s, int shared) { return set_bound(tb, s, shared, 3); }

int tiny_batch_reset_dual_variables(TinyBatch *tb)
{
    CHECK_TB(tb);
    tb->duals_zero_pending = true; // folded into the next solve's first iteration; flushed by any other reader
    return 0;
}

int tiny_batch_solve_async(TinyBatch *tb)
{
    CHECK_TB(tb);
    KernelPlan pl;
    TRY(prepare_solve(tb, kLoneSolve, &pl));
    return enqueue_solve(tb, pl, tb->timing, nullptr);
}

int tiny_batch_wait(TinyBatch *tb, int *n_unsolved)
{
    CHECK_TB(tb);
    TRY(set_device(tb));
    int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, tb->n_unsolved, sizeof(int), hipMemcpyDeviceToHost, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    if (n_unsolved) *n_unsolved = n;
    return 0;
}

int tiny_batch_solve(TinyBatch *tb)
{
    TRY(tiny_batch_solve_async(tb));
    int n = 0;
    TRY(tiny_batch_wait(tb, &n));
    return n > 0 ? 1 : 0;
}

// Mixed problem classes in one call (BASELINE.json configs[4]): every handle is one class (nx, nu, N, storage); all
// solves are enqueued before any is waited for, each on its handle's stream, so they overlap on the device.
int tiny_batch_group_solve(TinyBatch **tbs, int n, int *n_unsolved)
{
    CHECK_PTR(tbs);
    if (n < 1) return fail(TINY_BATCH_EINVAL, "tiny_batch_group_solve: need at least one handle");
    for (int i = 0; i < n; i++)
    {
        CHECK_TB(tbs[i]);
        for (int j = 0; j < i; j++)
            if (tbs[j] == tbs[i]) return fail(TINY_BATCH_EINVAL, "tiny_batch_group_solve: handle %d appears twice", i);
    }
    for (int i = 0; i < n; i++)
    {
        TinyBatch *tb = tbs[i];
        TRY(leave_null_stream(tb)); // the null stream would serialise the group
        TRY(tiny_batch_solve_async(tb));
    }
    int total = 0;
    for (int i = 0; i < n; i++)
    {
        int u = 0;
        TRY(tiny_batch_wait(tbs[i], &u));
        total += u;
    }
    if (n_unsolved) *n_unsolved = total;
    return total > 0 ? 1 : 0;
}

// Multi-device epilogue: handles that each own a block of the instance index (one handle per GPU, one
// stream per handle) deliver u.col(0) of all their instances into ONE device buffer — handle order = block order.  Each
// handle unpacks its first input column into a buffer of its own device and, where that is not the destination device, the
// block travels device-to-device (hipMemcpyPeerAsync: xGMI between the GPUs of a node, no host staging), all copies in flight
// together, one wait per handle at the end.  No collective: the path has none (the batch shards with no exchange step).
int tiny_batch_group_gather_u0(TinyBatch **tbs, int n, int dst_device, float *d_dst)
{
    CHECK_PTR(tbs); CHECK_PTR(d_dst);
    if (n < 1) return fail(TINY_BATCH_EINVAL, "tiny_batch_group_gather_u0: need at least one handle");
    for (int i = 0; i < n; i++)
    {
        CHECK_TB(tbs[i]);
        if (tbs[i]->nu != tbs[0]->nu) return fail(TINY_BATCH_EINVAL, "tiny_batch_group_gather_u0: handle %d has nu=%d, handle 0 nu=%d", i, tbs[i]->nu, tbs[0]->nu);
    }
    size_t off = 0;
    for (int i = 0; i < n; i++)
    {
        TinyBatch *tb = tbs[i];
        const size_t cnt = (size_t)tb->batch * tb->nu;
        TRY(set_device(tb));
        if (tb->device == dst_device)
            TRY(launch_unpack(tb, work_ptr(tb, TINY_ARR_U), d_dst + off, tb->layout, 1, tb->batch, 0, 1)); // straight into its block
        else
        {
            if (!tb->u0_stage) TRY(dev_alloc_zero(&tb->u0_stage, cnt));
            TRY(launch_unpack(tb, work_ptr(tb, TINY_ARR_U), tb->u0_stage, tb->layout, 1, tb->batch, 0, 1));
            HIP_TRY(hipMemcpyPeerAsync(d_dst + off, dst_device, tb->u0_stage, tb->device, cnt * sizeof(float), tb->stream));
        }
        off += cnt;
    }
    for (int i = 0; i < n; i++)
    {
        TRY(set_device(tbs[i]));
        HIP_TRY(hipStreamSynchronize(tbs[i]->stream));
    }
    return 0;
}

// the same into host memory: gathered on the device of handle 0, then ONE device-to-host copy
int tiny_batch_group_get_u0(TinyBatch **tbs, int n, float *u0_host)
{
    CHECK_PTR(tbs); CHECK_PTR(u0_host);
    if (n < 1) return fail(TINY_BATCH_EINVAL, "tiny_batch_group_get_u0: need at least one handle");
    size_t total = 0;
    for (int i = 0; i < n; i++) { CHECK_TB(tbs[i]); total += (size_t)tbs[i]->batch * tbs[i]->nu; }
    TRY(set_device(tbs[0]));
    float *d = nullptr;
    HIP_TRY(guarded_malloc((void **)&d, total * sizeof(float)));
    int rc = tiny_batch_group_gather_u0(tbs, n, tbs[0]->device, d);
    if (rc == 0)
    {
        (void)hipSetDevice(tbs[0]->device);
        hipError_t e = hipMemcpy(u0_host, d, total * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(TINY_BATCH_EHIP, "tiny_batch_group_get_u0: %s", hipGetErrorString(e));
    }
    (void)hipSetDevice(tbs[0]->device);
    (void)guarded_free(d);
    return rc;
}

int tiny_batch_forward_pass(TinyBatch *tb) { CHECK_TB(tb); return run_step(tb, STEP_FORWARD_PASS, nullptr, nullptr); }
int tiny_batch_update_slack(TinyBatch *tb) { CHECK_TB(tb); return run_step(tb, STEP_UPDATE_SLACK, nullptr, nullptr); }
int tiny_batch_update_dual(TinyBatch *tb) { CHECK_TB(tb); return run_step(tb, STEP_UPDATE_DUAL, nullptr, nullptr); }
int tiny_batch_update_linear_cost(TinyBatch *tb) { CHECK_TB(tb); return run_step(tb, STEP_UPDATE_LINEAR_COST, nullptr, nullptr); }
int tiny_batch_backward_pass_grad(TinyBatch *tb) { CHECK_TB(tb); return run_step(tb, STEP_BACKWARD_PASS_GRAD, nullptr, nullptr); }
int tiny_batch_termination_condition(TinyBatch *tb, int *converged)
{
    CHECK_TB(tb);
    int n_true = 0;
    TRY(run_step(tb, STEP_TERMINATION_CONDITION, converged, &n_true));
    return n_true;
}

int tiny_batch_get_x(TinyBatch *tb, float *x) { return tiny_batch_get_array(tb, TINY_ARR_X, x); }
int tiny_batch_get_u(TinyBatch *tb, float *u) { return tiny_batch_get_array(tb, TINY_ARR_U, u); }

int tiny_batch_get_status(TinyBatch *tb, int *iter, int *status, float *residuals)
{
    CHECK_TB(tb);
    TRY(set_device(tb));
    TRY(flush_pending(tb));
    if (iter) HIP_TRY(hipMemcpyAsync(iter, tb->iter, (size_t)tb->batch * sizeof(int), hipMemcpyDeviceToHost, tb->stream));
    if (status) HIP_TRY(hipMemcpyAsync(status, tb->status, (size_t)tb->batch * sizeof(int), hipMemcpyDeviceToHost, tb->stream));
    if (residuals) HIP_TRY(hipMemcpyAsync(residuals, tb->res, (size_t)tb->batch * 4 * sizeof(float), hipMemcpyDeviceToHost, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    return 0;
}

int tiny_batch_set_status(TinyBatch *tb, const int *iter, const int *status, const float *residuals)
{
    CHECK_TB(tb);
    TRY(set_device(tb));
    TRY(flush_pending(tb));
    if (iter) { HIP_TRY(hipMemcpyAsync(tb->iter, iter, (size_t)tb->batch * sizeof(int), hipMemcpyHostToDevice, tb->stream)); tb->iter_history = false; }
    if (status) HIP_TRY(hipMemcpyAsync(tb->status, status, (size_t)tb->batch * sizeof(int), hipMemcpyHostToDevice, tb->stream));
    if (residuals) HIP_TRY(hipMemcpyAsync(tb->res, residuals, (size_t)tb->batch * 4 * sizeof(float), hipMemcpyHostToDevice, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    return 0;
}

int tiny_batch_set_array(TinyBatch *tb, int id, const float *src)
{
    CHECK_TB(tb); CHECK_PTR(src);
    if (id < 0 || id >= TINY_ARR_COUNT) return fail(TINY_BATCH_EINVAL, "bad array id %d", id);
    TRY(set_device(tb));
    TRY(flush_pending(tb));
    TRY(upload_work(tb, src, id, 0, is_xfam(id) ? tb->N : tb->N - 1));
    if (id == TINY_ARR_X) // keep the closed-loop state buffer coherent with x.col(0)
        TRY(launch_unpack(tb, work_ptr(tb, TINY_ARR_X), tb->x0buf, tb->layout, 0, tb->batch, 0, 1));
    return 0;
}

int tiny_batch_get_array(TinyBatch *tb, int id, float *dst)
{
    CHECK_TB(tb); CHECK_PTR(dst);
    if (id < 0 || id >= TINY_ARR_COUNT) return fail(TINY_BATCH_EINVAL, "bad array id %d", id);
    TRY(set_device(tb));
    TRY(flush_pending(tb));
    return download_work(tb, id, dst, 0, is_xfam(id) ? tb->N : tb->N - 1);
}

int tiny_batch_reset_workspace(TinyBatch *tb)
{
    CHECK_TB(tb);
    TRY(set_device(tb));
    // Everything is zeroed lazily: the next solve reads d,v,z,y,g (and p) as zero in its first iteration and overwrites
    // the rest, any other reader triggers the zero fill (flush_pending); x.col(0) is zeroed before the next solve unless
    // a set_x0 overwrites it first (flush_x0_zero).
    tb->x0_zero_pending = true;
    tb->cold_pending = true;
    tb->duals_zero_pending = false;
    tb->iter_history = false;
    return 0;
}

// Device-pointer forms of set_array / get_array / set_xref: same host-layout arrays ([B][N][nx] / [B][N-1][nu], fp32),
// but resident in device memory on the handle's device; converted to/from the private layout by one kernel on the
// handle's stream, no host round trip and no synchronisation.
int tiny_batch_set_array_device(TinyBatch *tb, int id, const float *d_src)
{
    CHECK_TB(tb); CHECK_PTR(d_src);
    if (id < 0 || id >= TINY_ARR_COUNT) return fail(TINY_BATCH_EINVAL, "bad array id %d", id);
    TRY(set_device(tb));
    TRY(flush_pending(tb));
    const int fam = is_xfam(id) ? 0 : 1;
    TRY(launch_pack(tb, d_src, work_ptr(tb, id), tb->layout, fam, tb->batch, false, 0, fam ? tb->N - 1 : tb->N));
    if (id == TINY_ARR_X) TRY(launch_unpack(tb, work_ptr(tb, TINY_ARR_X), tb->x0buf, tb->layout, 0, tb->batch, 0, 1));
    return 0;
}

int tiny_batch_get_array_device(TinyBatch *tb, int id, float *d_dst)
{
    CHECK_TB(tb); CHECK_PTR(d_dst);
    if (id < 0 || id >= TINY_ARR_COUNT) return fail(TINY_BATCH_EINVAL, "bad array id %d", id);
    TRY(set_device(tb));
    TRY(flush_pending(tb));
    const int fam = is_xfam(id) ? 0 : 1;
    return launch_unpack(tb, work_ptr(tb, id), d_dst, tb->layout, fam, tb->batch, 0, fam ? tb->N - 1 : tb->N);
}

int tiny_batch_set_xref_device(TinyBatch *tb, const float *d_xref, int shared)
{
    CHECK_TB(tb); CHECK_PTR(d_xref);
    TRY(set_device(tb));
    TRY(store_input(tb, tb->in_xref, d_xref, shared != 0, tb->N, tb->nx, hipMemcpyDeviceToDevice));
    tb->xref_mode = 0;
    return 0;
}

int tiny_batch_get_u0_device(TinyBatch *tb, float *d_u0)
{
    CHECK_TB(tb); CHECK_PTR(d_u0);
    TRY(set_device(tb));
    return launch_unpack(tb, work_ptr(tb, TINY_ARR_U), d_u0, tb->layout, 1, tb->batch, 0, 1);
}

namespace // closed loop: tiny_batch_mpc_step_* (solve + plant step, one MPC step per call) and tiny_batch_mpc_run_* (`steps` of them back to back)
{
// what the step and the run calls ask alike.  who: the public call, what: "mpc_step" / "mpc_run", for the messages (no handle has nx > 64: tiny_batch_create)
int check_loop_args(const TinyBatch *tb, const char *who, const char *what, int window_advance)
{
    if (window_advance < 0) return fail(TINY_BATCH_EINVAL, "%s: window_advance must be >= 0 (got %d): the window gather clamps at the last table row only", who, window_advance);
    if (tb->nx > 64) return fail(TINY_BATCH_EUNSUPPORTED, "%s supports nx <= 64", what);
    return 0;
}

int mpc_step_sim(TinyBatch *tb, const char *who, int window_advance, const float *d_w)
{
    TRY(check_loop_args(tb, who, "mpc_step", window_advance));
    tb->duals_zero_pending = true; // x.col(0) already holds x0 (set_x0 / previous plant step); reset duals, solve, then simulate forward
    TRY(tiny_batch_solve_async(tb));
    return enqueue_plant_step(tb, window_advance, d_w, nullptr);
}

// Loop::OnChip: ONE launch runs all the steps, the state never leaves registers / LDS between solves; the host adds what the last step leaves to it
int run_on_chip(TinyBatch *tb, const KernelPlan &pl, const RunArgs &run)
{
    const int last = run.steps - 1;
    TRY(enqueue_solve(tb, pl, false, &run));
    if (run.d_u0_traj) TRY(launch_unpack(tb, work_ptr(tb, TINY_ARR_U), run.u0_at(tb, last), tb->layout, 1, tb->batch, 0, 1));
    HIP_TRY(run.log_row(tb, last)); // the last row of the logs is the host's too: iter[] / status[] as the kernel's live-out left them
    return enqueue_plant_step(tb, run.window_advance, run.w_at(tb, last), run.x_at(tb, last)); // ... and so is the last plant step: the same plant, its own rows
}

// Loop::Replay, and a run of one step: the launch sequence (dispatch order or counter reset, solve kernel, u.col(0), log rows, plant kernel) x steps is captured
// ONCE into a hipGraph and replayed, which removes the per-launch overhead that dominates small batches with short warm-started solves
int run_replayed(TinyBatch *tb, const KernelPlan &pl, const RunArgs &run)
{
    TRY(leave_null_stream(tb)); // stream capture is not allowed on the null stream
    const std::string sig = graph_signature(tb, pl, run);
    if (!tb->graph_exec || tb->graph_sig != sig)
    {
        if (tb->graph_exec) { (void)hipGraphExecDestroy(tb->graph_exec); tb->graph_exec = nullptr; }
        hipGraph_t graph = nullptr;
        HIP_TRY(hipStreamBeginCapture(tb->stream, hipStreamCaptureModeThreadLocal));
        int rc = 0;
        for (int k = 0; k < run.steps && rc == 0; k++)
        {
            tb->duals_zero_pending = true;
            rc = enqueue_solve(tb, pl, false, nullptr);
            if (rc == 0 && run.d_u0_traj) rc = launch_unpack(tb, work_ptr(tb, TINY_ARR_U), run.u0_at(tb, k), tb->layout, 1, tb->batch, 0, 1);
            if (rc == 0 && run.log_row(tb, k) != hipSuccess) rc = fail(TINY_BATCH_EHIP, "%s: the copy of a log row failed", run.who);
            if (rc == 0) rc = enqueue_plant_step(tb, run.window_advance, run.w_at(tb, k), run.x_at(tb, k));
        }
        hipError_t ec = hipStreamEndCapture(tb->stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        HIP_TRY(ec);
        hipError_t ei = hipGraphInstantiate(&tb->graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        HIP_TRY(ei);
        tb->graph_sig = sig;
        tb->graph_captures++;
    }
    HIP_TRY(hipGraphLaunch(tb->graph_exec, tb->stream));
    tb->duals_zero_pending = tb->cold_pending = false; // (a replay enqueues no solve of its own to clear them)
    return 0;
}

// the run calls, all of them: the argument checks, what may allocate or synchronise, then the loop the plan names.  The two loops give identical results
int mpc_run_sim(TinyBatch *tb, RunArgs run)
{
    if (run.steps < 1) return fail(TINY_BATCH_EINVAL, "%s: steps must be >= 1", run.who);
    TRY(check_loop_args(tb, run.who, "mpc_run", run.window_advance));
    if (budget_min(tb) <= 0) return fail(TINY_BATCH_EINVAL, tb->ps ? "%s needs max_iter > 0 for every instance" : "%s needs max_iter > 0", run.who);
    TRY(set_device(tb));
    if (tb->xref_mode == 1 && run.window_advance) tb->tile_map_dirty = true; // either loop slides xref_start[] (the on-chip one writes it back)
    run.from_reset = tb->cold_pending; // (flush_pending materialises the zeros and clears the flag: the run's first solve is the cold one all the same)
    TRY(flush_pending(tb)); // every solve of the run starts from "duals reset, workspace warm"
    tb->duals_zero_pending = true;
    const bool sim = tb->plant_mode != 0 || run.d_w != nullptr || run.d_x_traj != nullptr, logs = run.d_iter_log != nullptr || run.d_status_log != nullptr;
    KernelPlan pl;
    TRY(prepare_solve(tb, Call{run.steps > 1 ? Call::Run : Call::Solve, sim, logs}, &pl));
    TRY(pl.loop == Loop::OnChip ? run_on_chip(tb, pl, run) : run_replayed(tb, pl, run));
    tb->ev_valid = false; // no event brackets a run
    return 0;
}

// host-array variant of tiny_batch_mpc_run_log_async (any of the five may be NULL): the device buffers live on the HANDLE's device for the call
int mpc_run_log_host(TinyBatch *tb, const char *who, int steps, int window_advance, const float *w, float *u0_traj, float *x_traj, int *iter_log, int *status_log)
{
    if (!tb) return fail(TINY_BATCH_EINVAL, "%s: NULL TinyBatch handle", who);
    if (steps < 1) return fail(TINY_BATCH_EINVAL, "%s: steps must be >= 1", who);
    TRY(set_device(tb));
    // device copies kept on the handle and re-allocated only when their size changes: on the replayed paths the captured graph bakes their addresses
    // in (they are in its signature), and a loop of equal calls must replay one graph.  (The two logs are ints in float-sized words.)
    const size_t nxf = (size_t)steps * tb->batch * tb->nx, nuf = (size_t)steps * tb->batch * tb->nu, nlf = (size_t)steps * tb->batch;
    const void *host[5] = {w, u0_traj, x_traj, iter_log, status_log};
    const size_t nf[5] = {nxf, nuf, nxf, nlf, nlf};
    float *dev[5] = {};
    for (int k = 0; k < 5; k++)
        if (host[k])
        {
            if (tb->sim_stage[k] && tb->sim_stage_n[k] != nf[k]) HIP_TRY(hipStreamSynchronize(tb->stream)); // a run still using the old buffer may be in flight
            TRY(sized_buffer(&tb->sim_stage[k], &tb->sim_stage_n[k], nf[k]));
            dev[k] = tb->sim_stage[k];
        }
    if (w) HIP_TRY(hipMemcpy(dev[0], w, nxf * sizeof(float), hipMemcpyHostToDevice));
    TRY(mpc_run_sim(tb, RunArgs{who, steps, window_advance, dev[0], dev[1], dev[2], (int *)dev[3], (int *)dev[4]}));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    if (u0_traj) HIP_TRY(hipMemcpy(u0_traj, dev[1], nuf * sizeof(float), hipMemcpyDeviceToHost));
    if (x_traj) HIP_TRY(hipMemcpy(x_traj, dev[2], nxf * sizeof(float), hipMemcpyDeviceToHost));
    if (iter_log) HIP_TRY(hipMemcpy(iter_log, dev[3], nlf * sizeof(int), hipMemcpyDeviceToHost));
    if (status_log) HIP_TRY(hipMemcpy(status_log, dev[4], nlf * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}
} // namespace

int tiny_batch_mpc_step_sim_async(TinyBatch *tb, int window_advance, const float *d_w) { CHECK_TB(tb); return mpc_step_sim(tb, "tiny_batch_mpc_step_sim_async", window_advance, d_w); }
int tiny_batch_mpc_step_async(TinyBatch *tb, int window_advance) { CHECK_TB(tb); return mpc_step_sim(tb, "tiny_batch_mpc_step_async", window_advance, nullptr); }

// `steps` closed-loop MPC steps back to back against the plant of tiny_batch_set_plant (none set: the model's own dynamics): RunArgs has the arguments.  Whether
// the steps run inside one launch or as a replayed launch sequence is the plan's to say (KernelPlan::loop): the results are the same
int tiny_batch_mpc_run_sim_async(TinyBatch *tb, int steps, int window_advance, const float *d_w, float *d_u0_traj, float *d_x_traj)
{
    CHECK_TB(tb);
    return mpc_run_sim(tb, RunArgs{"tiny_batch_mpc_run_sim_async", steps, window_advance, d_w, d_u0_traj, d_x_traj, nullptr, nullptr});
}

// ... and the per-step solver log: what a step-by-step loop reads with tiny_batch_get_status after step k.  A log does not make a run simulated: kernel and
// results are those of the same call without it
int tiny_batch_mpc_run_log_async(TinyBatch *tb, int steps, int window_advance, const float *d_w, float *d_u0_traj, float *d_x_traj, int *d_iter_log, int *d_status_log)
{
    CHECK_TB(tb);
    return mpc_run_sim(tb, RunArgs{"tiny_batch_mpc_run_log_async", steps, window_advance, d_w, d_u0_traj, d_x_traj, d_iter_log, d_status_log});
}

int tiny_batch_mpc_run_traj_async(TinyBatch *tb, int steps, int window_advance, float *d_u0_traj)
{
    CHECK_TB(tb);
    return mpc_run_sim(tb, RunArgs{"tiny_batch_mpc_run_async", steps, window_advance, nullptr, d_u0_traj, nullptr, nullptr, nullptr});
}

int tiny_batch_mpc_run_async(TinyBatch *tb, int steps, int window_advance) { return tiny_batch_mpc_run_traj_async(tb, steps, window_advance, nullptr); }

// host-copy variant: the trajectory buffer is allocated on the HANDLE's device (whatever device is current for the calling
// thread), the run is waited for and u.col(0) of every step lands in host memory
int tiny_batch_mpc_run_traj(TinyBatch *tb, int steps, int window_advance, float *u0_traj_host)
{
    CHECK_TB(tb); CHECK_PTR(u0_traj_host);
    if (steps < 1) return fail(TINY_BATCH_EINVAL, "tiny_batch_mpc_run_traj: steps must be >= 1");
    TRY(set_device(tb));
    const size_t n = (size_t)steps * tb->batch * tb->nu;
    float *d = nullptr;
    HIP_TRY(guarded_malloc((void **)&d, n * sizeof(float)));
    int rc = tiny_batch_mpc_run_traj_async(tb, steps, window_advance, d);
    if (rc == 0)
    {
        hipError_t e = hipStreamSynchronize(tb->stream);
        if (e == hipSuccess) e = hipMemcpy(u0_traj_host, d, n * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(TINY_BATCH_EHIP, "tiny_batch_mpc_run_traj: %s", hipGetErrorString(e));
    }
    (void)guarded_free(d);
    return rc;
}

int tiny_batch_mpc_run_log(TinyBatch *tb, int steps, int window_advance, const float *w, float *u0_traj, float *x_traj, int *iter_log, int *status_log)
{
    return mpc_run_log_host(tb, "tiny_batch_mpc_run_log", steps, window_advance, w, u0_traj, x_traj, iter_log, status_log);
}
int tiny_batch_mpc_run_sim(TinyBatch *tb, int steps, int window_advance, const float *w, float *u0_traj, float *x_traj)
{
    return mpc_run_log_host(tb, "tiny_batch_mpc_run_sim", steps, window_advance, w, u0_traj, x_traj, nullptr, nullptr);
}

int tiny_batch_get_x0(TinyBatch *tb, float *x0)
{
    CHECK_TB(tb); CHECK_PTR(x0);
    TRY(set_device(tb));
    TRY(flush_x0_zero(tb));
    HIP_TRY(hipMemcpyAsync(x0, tb->x0buf, (size_t)tb->batch * tb->nx * sizeof(float), hipMemcpyDeviceToHost, tb->stream));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    return 0;
}

int tiny_batch_enable_timing(TinyBatch *tb, int on)
{
    CHECK_TB(tb);
    tb->timing = on != 0;
    tb->ev_valid = false;
    return 0;
}

int tiny_batch_last_solve_ms(TinyBatch *tb, float *ms)
{
    CHECK_TB(tb); CHECK_PTR(ms);
    if (!tb->ev_valid) return fail(TINY_BATCH_ENOTREADY, "no timed solve recorded (call tiny_batch_enable_timing first)");
    TRY(set_device(tb));
    HIP_TRY(hipEventSynchronize(tb->ev1));
    HIP_TRY(hipEventElapsedTime(ms, tb->ev0, tb->ev1));
    return 0;
}

const char *tiny_batch_kernel_name(TinyBatch *tb)
{
    if (!tb) return "";
    // per-instance tables of the class admm_tile16_pi.hip serves: whether they change along the horizon (one resident row per instance, or rings)
    // is found when the derived tables are built, and the automatic choice depends on it — build them now, as the next solve would
    // ... and so is whether the bounds table holds a zero that hands an exact solve over from the matrix-core kernels (zero_ties_hand_over)
    if (!tb->h16 && tb->derived_dirty[LAYOUT_ROW] &&
        ((tb->tile16_ok && tile16_per_instance(tb)) || ((tb->tile16_ok || tb->tile48_ok) && (tb->variant == VAR_AUTO || tb->variant == VAR_ROW_EXACT))))
    {
        const std::string keep = g_err;
        KernelPlan pl;
        (void)prepare_solve(tb, kLoneSolve, &pl); // (not ready yet: the name is then the one the present knowledge gives)
        g_err = keep;
    }
    return plan_name(tb, kLoneSolve);
}

int tiny_batch_debug_graph_captures(TinyBatch *tb)
{
    CHECK_TB(tb);
    return tb->graph_captures; // how often tiny_batch_mpc_run_* had to capture its hipGraph (a replay does not count)
}

int tiny_batch_debug_guards(int on)
{
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guards_on = on != 0; // applies to allocations made from now on (handles created earlier keep what they have)
    return 0;
}

long long tiny_batch_debug_check(void)
{
    std::lock_guard<std::mutex> lk(g_guard_mu);
    if (g_guarded.empty()) return 0;
    unsigned long long *bad = nullptr, host = 0;
    if (hipMalloc((void **)&bad, sizeof *bad) != hipSuccess || hipMemset(bad, 0, sizeof *bad) != hipSuccess) return fail(TINY_BATCH_EHIP, "tiny_batch_debug_check: allocation failed");
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipFree(bad); return fail(TINY_BATCH_EHIP, "tiny_batch_debug_check: a kernel faulted: %s", hipGetErrorString(hipGetLastError())); }
    hipError_t e = hipSuccess;
    for (const auto &kv : g_guarded)
    {
        char *u = (char *)kv.first;
        if (e == hipSuccess) e = launch_guard_count((const unsigned *)(u - kGuard * sizeof(float)), kGuard, bad, nullptr);
        if (e == hipSuccess) e = launch_guard_count((const unsigned *)(u + kv.second), kGuard, bad, nullptr);
    }
    if (e == hipSuccess) e = hipMemcpy(&host, bad, sizeof host, hipMemcpyDeviceToHost);
    (void)hipFree(bad);
    if (e != hipSuccess) return fail(TINY_BATCH_EHIP, "tiny_batch_debug_check: %s", hipGetErrorString(e));
    return (long long)host;
}

int tiny_batch_debug_poke(TinyBatch *tb, int which)
{
    CHECK_TB(tb);
    TRY(set_device(tb));
    // test hook of the guard zones: deliberately writes ONE word just outside a work array of this handle (which = 0: in front, 1: behind)
    float *arr = tb->layout == LAYOUT_ROW ? tb->pair[0] : tb->arr[0];
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        auto it = g_guarded.find(arr);
        if (it == g_guarded.end()) return fail(TINY_BATCH_ENOTREADY, "tiny_batch_debug_poke: the handle was not created under tiny_batch_debug_guards(1)");
        bytes = it->second;
    }
    const float v = 1.0f;
    HIP_TRY(hipMemcpy(which ? (char *)arr + bytes : (char *)arr - sizeof(float), &v, sizeof v, hipMemcpyHostToDevice));
    return 0;
}

int tiny_batch_arithmetic(TinyBatch *tb)
{
    CHECK_TB(tb);
    KernelPlan pl;
    TRY(resolve_plan(tb, kLoneSolve, &pl));
    return pl.exact ? TINY_BATCH_ARITH_EXACT : TINY_BATCH_ARITH_FMA;
}

// the kernel a closed-loop run of several steps (tiny_batch_mpc_run_async) launches: it can differ from the kernel of a lone solve (the automatic
// choice keeps the 16-lane kernel's on-chip MPC loop where a lone solve of the same batch goes to the matrix-core kernel)
const char *tiny_batch_closed_loop_kernel_name(TinyBatch *tb)
{
    if (!tb) return "";
    return plan_name(tb, Call{Call::Run, tb->plant_mode != 0}); // (a run that passes d_w or d_x_traj without a plant is simulated too: only the call knows)
}

int tiny_batch_set_row_kernel(TinyBatch *tb, int family)
{
    CHECK_TB(tb);
    if (family < 0 || family > 8)
        return fail(TINY_BATCH_EINVAL, "row kernel must be 0 (auto), 1 (rowlane), 2 (rowloop), 3 (rowstream), 4 (quadlane), 5 (tile16), 6 (wavestream), 7 (waveres) or 8 (tile48)");
    std::optional<Kernel> forced; // the kernel with that number, if the class has an instantiation of it
    for (const KernelTraits &t : kKernelTraits)
        if (family && t.row_kernel_number == family && tb->*t.has) forced = (Kernel)(&t - kKernelTraits);
    if (family && !forced)
        return fail(TINY_BATCH_EUNSUPPORTED, "row kernel %d has no instantiation for nx=%d nu=%d N=%d", family, tb->nx, tb->nu, tb->N);
    tb->row_family_forced = forced;
    invalidate_graph(tb);
    return 0;
}

// bits = 16: the duals stay fp32 wherever the kernels implement that (round 3: with 16-bit duals a quarter of a cartpole batch and
// 8 % of a quadrotor batch stall above the tolerances; 16-bit duals remain available through tiny_batch_set_storage_ex(tb, 16, 16)
// and are what the kernels that stream their state implement)
int tiny_batch_set_storage(TinyBatch *tb, int bits)
{
    CHECK_TB(tb);
    const bool d32 = bits == 16 && (tb->row_dims_ok || tb->quad_ok);
    TRY(tiny_batch_set_storage_ex(tb, bits, d32 ? 32 : bits));
    tb->dual32_pref = d32;     // a preference: every solve / step call settles the width on the kernel it resolves to (settle_dual_width)
    tb->dual32_forced = false;
    return 0;
}

int tiny_batch_set_storage_ex(TinyBatch *tb, int bits, int dual_bits)
{
    CHECK_TB(tb);
    if (bits != 16 && bits != 32) return fail(TINY_BATCH_EINVAL, "storage must be 32 (fp32, default) or 16 (IEEE binary16)");
    if (dual_bits != bits && !(bits == 16 && dual_bits == 32)) return fail(TINY_BATCH_EINVAL, "dual storage must equal the storage, or be 32 with 16-bit storage");
    const bool want = bits == 16, want_d32 = want && dual_bits == 32;
    if (want_d32 && !(tb->row_dims_ok || tb->quad_ok))
        return fail(TINY_BATCH_EUNSUPPORTED, "fp16 storage with fp32 duals needs a register-resident kernel instantiation (nx=%d nu=%d N=%d has none)", tb->nx, tb->nu, tb->N);
    if (want && !(tb->row_dims_ok || tb->rowmath_ok) )
        return fail(TINY_BATCH_EUNSUPPORTED, "fp16 storage is implemented by the row kernels only (nx=%d nu=%d has none)", tb->nx, tb->nu);
    if (want && tb->variant == VAR_STREAM) return fail(TINY_BATCH_EUNSUPPORTED, "fp16 storage cannot be combined with the streaming kernel");
    tb->dual32_pref = false;      // (a refused call leaves the handle as it was)
    tb->dual32_forced = want_d32;
    if (want == tb->h16 && want_d32 == tb->dual32) return 0;
    TRY(set_device(tb));
    HIP_TRY(hipStreamSynchronize(tb->stream));
    invalidate_graph(tb);
    // the workspace restarts from zero in the new precision (like tiny_batch_create), inputs are re-derived
    free_layout(tb, LAYOUT_TILE);
    free_layout(tb, LAYOUT_ROW);
    tb->h16 = want;
    tb->dual32 = want_d32;
    tb->layout = (want || tb->row_dims_ok || tb->wave_ok || !tb->tile_dims_ok) ? LAYOUT_ROW : LAYOUT_TILE;
    TRY(alloc_layout(tb, tb->layout));
    HIP_TRY(hipMemsetAsync(tb->res, 0, (size_t)tb->batch * 4 * sizeof(float), tb->stream));
    HIP_TRY(hipMemsetAsync(tb->status, 0, (size_t)tb->batch * sizeof(int), tb->stream));
    HIP_TRY(hipMemsetAsync(tb->iter, 0, (size_t)tb->batch * sizeof(int), tb->stream));
    tb->iter_history = false;
    HIP_TRY(hipMemsetAsync(tb->x0buf, 0, (size_t)tb->batch * tb->nx * sizeof(float), tb->stream));
    tb->cold_pending = tb->duals_zero_pending = tb->x0_zero_pending = false;
    tb->derived_dirty[0] = tb->derived_dirty[1] = true;
    return 0;
}

int tiny_batch_select_kernel(TinyBatch *tb, int variant)
{
    CHECK_TB(tb);
    if (variant < VAR_AUTO || variant > VAR_GENERIC)
        return fail(TINY_BATCH_EINVAL, "variant must be 0 (auto), 1 (streaming, fma), 2 (row / wave kernels, exact), 3 (row / wave kernels, fma) or 4 (run-time dimensions, exact)");
    const int old = tb->variant;
    tb->variant = variant;
    KernelPlan pl;
    if (int rc = resolve_plan(tb, kLoneSolve, &pl)) { tb->variant = old; return rc; }
    invalidate_graph(tb);
    TRY(set_device(tb));
    TRY(ensure_layout(tb, traits(pl.kernel).layout));
    return 0;
}

} // extern "C"
