// admm_rowsim.hip — the SIM instantiations of the 16-lane kernel's body (the on-chip closed loop against a separate plant, with a disturbance and the
// state trajectory: see the SIM block of admm_rowlane.hip) and their launcher, as a translation unit of their own.
#define TINY_ROWSIM_UNIT 1
#include "admm_rowlane.hip"
