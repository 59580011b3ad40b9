// admm_waveres_ps.hip — the per-instance-settings instantiations of the state-on-chip wave kernel's body (see the PS block of admm_waveres.hip) and their
// launcher, as a translation unit of their own.
#define TINY_WAVERES_PS_UNIT 1
#include "admm_waveres.hip"
