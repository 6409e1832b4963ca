"""The cases of the wide SAC1 learner's tests (tests/test_gpu_sac1_wide.py on the GPU, tests/test_sac1_wide_cpu.py for the oracles'
side of the bars): tests/_state_parity.Case rows, `fused` unset — the GPU test asserts ddrl_sac1_is_wide itself."""
from _state_parity import HYPER_H, HYPER_I, HYPER_J, Case

CASES = [
    Case("sac1-wide-walker", "sac1", 24, 4, (400, 300), 256),                             # float4 loads; steps 13 / 16
    Case("sac1-wide-12-1", "sac1", 12, 1, (36, 8), 37, **HYPER_H),                        # first shape outside the narrow envelope; element loads; ragged; one action
    Case("sac1-wide-27-4", "sac1", 27, 4, (72, 44), 37, **HYPER_I),                       # D1 = 32 fills the block; the action columns straddle a float4
    Case("sac1-wide-28-3", "sac1", 28, 3, (512, 512), 1, **HYPER_J),                      # D1 = 32; float4 observations, element-loaded action; widest hidden; one row
    Case("sac1-wide-16-4-b512", "sac1", 16, 4, (300, 300), 512),                          # the last batch the wgrad tile holds
    Case("sac1-wide-8-2", "sac1", 8, 2, (64, 48), 37),                                    # the short step-count instantiations
]
PATH_CASE = Case("sac1-wide-paths-27-4", "sac1", 27, 4, (72, 44), 37, **HYPER_I)
