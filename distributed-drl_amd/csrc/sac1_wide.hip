// The kernels of a WIDE learner — SAC1 (ddrl_sac1_create_wide, include/ddrl_sac1_wide.h) or SAC-v (ddrl_sacv_create_wide,
// include/ddrl_sacv_wide.h); obs_dim + act_dim <= 31: the bipedal walker's 24 / 4 — and their launch functions, called by sac1.hip's launch state for a handle on its third kernel path:
//   * k_dfwd_wide<0 / 1> (sac1_wide.h): the two forward launches over the wide layer-1 block layout;
//   * k_dg (sac1_direct.h) compiled HERE with DDRL_W1_INDEX = w1wide_index: the three backward launches with their existing job kinds —
//     the layer-1 wgrad tile (DG_WGRAD_W1Y: 32 input columns, bias row included, x 32 hidden units, the batch contracted in 8-deep groups
//     over the four waves, Adam and polyak in the epilogue) then addresses gradient, m, v, main and target in the mode-3 blocks, and the
//     dQ/da partials read the action rows of q1's mode-3 block.  sac1.hip's own k_dg is compiled from the same text with the default;
//   * k_pack_wide (wide_pack.h): external order <-> the mode-3 learner layout, through the handle's segment table.
// This translation unit is compiled without the packed float32 VALU forms (Makefile), device library included.
// The job tables cross the boundary as untyped pointers: their types have internal linkage in each translation unit and are laid out
// from the same headers by the same compiler.
#include "gemm_core.h"
#include "policy_row.h"

namespace {
#include "wide_pack.h"
#define DDRL_W1_INDEX w1wide_index
#include "sac1_direct.h"
#include "sac1_wide.h"
}  // namespace

void ddrl_sac1_wide_launch_fwd(int phase, const void *head, const void *args, void *stream) {
    const DFHead &d = *static_cast<const DFHead *>(head);
    const DFArgs &F = *static_cast<const DFArgs *>(args);
    if (phase == 0) launch_dfwd_wide<0>(d, F, static_cast<hipStream_t>(stream));
    else launch_dfwd_wide<1>(d, F, static_cast<hipStream_t>(stream));
}

void ddrl_sac1_wide_launch_dg(const void *jobs, void *stream, int kid) {
    launch_dg(*static_cast<const DGJobs *>(jobs), static_cast<hipStream_t>(stream), kid);
}

// to_internal 1: dense flat vector -> the wide layout (dst, and dst2 when given: main and target at set_weights);  0: the reverse
void ddrl_sac1_wide_pack(const void *segs_d, int nsegs, const float *src, float *dst, float *dst2, int to_internal, void *stream) {
    const Seg *segs = static_cast<const Seg *>(segs_d);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(64, (unsigned)nsegs);
    if (!to_internal) { k_pack_wide<0><<<grid, 256, 0, s>>>(segs, src, dst, nullptr, 0, nullptr); return; }
    k_pack_wide<1><<<grid, 256, 0, s>>>(segs, src, dst, nullptr, 0, nullptr);
    if (dst2) k_pack_wide<1><<<grid, 256, 0, s>>>(segs, src, dst2, nullptr, 0, nullptr);
}
