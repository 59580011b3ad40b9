// admm_f64_rowsim_pm.hip — the closed-loop instantiations of admm_f64_rows_kernel with per-instance models (Mpc64, Sim64, Models64: the PM blocks
// of admm_f64_rows.hip) and their launcher, as a translation unit of their own.
#define TINY_F64PM_UNIT 2
#include "admm_f64_rows.hip"
