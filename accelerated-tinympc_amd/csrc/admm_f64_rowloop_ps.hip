// admm_f64_rowloop_ps.hip — the on-chip closed-loop instantiations of admm_f64_rows_kernel with per-instance settings (Mpc64, Settings64: the SET
// blocks of admm_f64_rows.hip) and their launcher, as a translation unit of their own.
#define TINY_F64PS_UNIT 2
#include "admm_f64_rows.hip"
