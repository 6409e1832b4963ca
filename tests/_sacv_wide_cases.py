"""The cases of the wide SAC-v learner's tests (tests/test_gpu_sacv_wide.py on the GPU, tests/test_sacv_wide_cpu.py for the oracles'
side of the bars): tests/_state_parity.Case rows mirroring tests/_sac1_wide_cases.py, `fused` unset — the GPU test asserts
ddrl_sac1_is_wide itself."""
from _state_parity import HYPER_H, HYPER_I, HYPER_J, Case

CASES = [
    Case("sacv-wide-walker", "sacv", 24, 4, (400, 300), 256),                             # float4 loads; V runs 13 steps beside the Q jobs' 16
    Case("sacv-wide-12-1", "sacv", 12, 1, (36, 8), 37, **HYPER_H),                        # first shape outside the narrow envelope; element loads; ragged; one action
    Case("sacv-wide-27-4", "sacv", 27, 4, (72, 44), 37, **HYPER_I),                       # D1 = 32 fills the block; the action columns straddle a float4
    Case("sacv-wide-28-3", "sacv", 28, 3, (512, 512), 1, **HYPER_J),                      # D1 = 32; widest hidden; one row
    Case("sacv-wide-16-4-b512", "sacv", 16, 4, (300, 300), 512),                          # the last batch the wgrad tile holds
    Case("sacv-wide-8-2", "sacv", 8, 2, (64, 48), 37, **HYPER_H),                         # the short step counts; the shape and bars of sacv-direct-b37-h64x48
]
PATH_CASE = Case("sacv-wide-paths-27-4", "sacv", 27, 4, (72, 44), 37, **HYPER_I)
