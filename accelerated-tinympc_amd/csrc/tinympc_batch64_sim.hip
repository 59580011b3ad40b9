// tinympc_batch64_sim.hip — the fp64 library's closed loop against a separate plant (tiny_batch64_set_plant, tiny_batch64_mpc_run_sim): the SIM
// instantiations of the sixteen-lane kernel (see the SIM block of tinympc_batch64.hip), the simulated plant kernel and their launchers, as a
// translation unit of their own.
#define TINY_F64SIM_UNIT 1
#include "tinympc_batch64.hip"
