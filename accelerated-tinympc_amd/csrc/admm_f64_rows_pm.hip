// admm_f64_rows_pm.hip — the one-solve instantiations of admm_f64_rows_kernel with per-instance models (tiny_batch64_set_models: the PM blocks of
// admm_f64_rows.hip) and their launcher, as a translation unit of their own.
#define TINY_F64PM_UNIT 1
#include "admm_f64_rows.hip"
