// admm_f64_rowsim.hip — the SIM instantiations of admm_f64_rows_kernel (the on-chip closed loop against a separate plant, with a disturbance and
// the state trajectory: see the SIM blocks of admm_f64_rows.hip) and their launcher, as a translation unit of their own.
#define TINY_F64SIM_UNIT 1
#include "admm_f64_rows.hip"
