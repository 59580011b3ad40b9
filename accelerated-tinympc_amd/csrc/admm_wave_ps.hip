// admm_wave_ps.hip — the per-instance-settings instantiations of the streaming wave kernel's body (see the PS block of admm_wave.hip) and their launcher,
// as a translation unit of their own.
#define TINY_WAVE_PS_UNIT 1
#include "admm_wave.hip"
