// admm_rowlane_ps.hip — the per-instance-settings instantiations of the register-resident 16-lane kernel (tiny_batch_set_instance_settings): the PS
// instantiations of rowlane_body and their launcher, a translation unit of its own so that the kernels of admm_rowlane.hip keep their code.
#define TINY_ROWLANE_PS_UNIT
#include "admm_rowlane.hip"
