// admm_waveres_pm.hip — the per-instance-model instantiations of the state-on-chip wave kernel's body (see the PM block of admm_waveres.hip), their
// launcher and models_pack_wave_kernel, which packs the gain tables of both wave kernels, as a translation unit of their own.
#define TINY_WAVERES_PM_UNIT 1
#include "admm_waveres.hip"
