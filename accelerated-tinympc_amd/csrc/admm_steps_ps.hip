// admm_steps_ps.hip — the per-instance-settings forms of the streaming row kernel and of the step kernel, whose termination_condition reads an instance's
// record (tiny_batch_set_instance_settings): the two kernel bodies of admm_steps.hip compiled with the settings view on SP.rec[inst], and their launchers;
// a translation unit of its own so that the kernels of admm_steps.hip keep their code.
#define TINY_STEPS_PS_UNIT
#include "admm_steps.hip"
