// admm_f64_rows_ps.hip — the one-solve instantiations of admm_f64_rows_kernel with per-instance settings (tiny_batch64_set_instance_settings: the SET
// blocks of admm_f64_rows.hip) and their launcher, as a translation unit of their own.
#define TINY_F64PS_UNIT 1
#include "admm_f64_rows.hip"
