// admm_wave_pm.hip — the per-instance-model instantiations of the streaming wave kernel's body (see the PM block of admm_wave.hip) and their launcher,
// as a translation unit of their own.
#define TINY_WAVE_PM_UNIT 1
#include "admm_wave.hip"
