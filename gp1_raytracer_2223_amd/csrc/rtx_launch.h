// rtx_launch.h — the launches of rtx_render_kernel (rtx_hip.hip) as plain host functions: each picks
// the instantiation from run-time facts and queues it on `s`; the caller checks hipGetLastError.
// A combination no frame takes (one without an instantiation) aborts.  Internal to librtx_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include "rtx_kernels.h"

namespace rtxh {

// PHASE `phase` (0..6) of a frame in its specialised variant (index into kSpecVariants, -1: the
// generic kernel), with the cull variant when the scene has cull records and the SS one for a
// supersampled frame.
void launch_render_phase(int phase, int variant, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                         const rtxd::FrameArgs& F);
// The one-launch frames without a specialised variant: the counting kernels (plain, with the cull,
// deep, deep with HBM stacks) and the deep-stack frames (deep, deep with HBM stacks).
void launch_render_one(bool count, bool deep, bool hstk, bool cull, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                       const rtxd::FrameArgs& F);
// The hit pass (PHASE 7): the generic kernel with every stack, or with the exact cull.
void launch_hit_pass(bool deep, bool hstk, bool cull, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                     const rtxd::FrameArgs& F);
// Deferred shading (PHASE 8): the frame's specialised variant (-1: generic) with the cull variant when
// the scene has cull records, or the generic kernel with the deep stacks (which walk without the cull).
void launch_deferred(int variant, bool deep, bool hstk, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                     const rtxd::FrameArgs& F);
// The shadow pass (PHASE 9): the instantiation launch_deferred would take, variant for variant.
void launch_shadows(int variant, bool deep, bool hstk, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                    const rtxd::FrameArgs& F);
// Relighting (rtx_relight_kernel): grid.x workgroups of kRelightThreads, one wave per 64-pixel row piece.
void launch_relight(dim3 grid, hipStream_t s, const rtxd::DevScene& d, const rtxd::RelightArgs& A);
// The resolved relight (rtx_relight_resolve_kernel<ss_log2>, ss_log2 = 1..3): the same workgroups, one wave per
// 64-sample piece of an OUTPUT row's sample rows; A describes the sample frame, its rows and stripes output rows.
void launch_relight_resolve(uint32_t ss_log2, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                            const rtxd::RelightArgs& A);
// A ray query (rtx_query_kernel): closest hit or occlusion (`any`) with the default stack, the deep
// one, or the deep one in HBM; grid.x = the launch's waves, ceil(Q.n / 64) / kWavesPerBlock.
void launch_query(bool any, bool deep, bool hstk, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                  const rtxd::QueryArgs& Q);
// Shaded rays (rtx_shade_kernel): the same three stacks and grid.
void launch_shade(bool deep, bool hstk, dim3 grid, hipStream_t s, const rtxd::DevScene& d, const rtxd::ShadeArgs& Q);
// Adaptive refinement (rtx_adaptive_kernel): the same three stacks; grid.x * kWavesPerBlock persistent
// waves stride over the listed pixels, whose number the kernel reads from the device.
void launch_adaptive(bool deep, bool hstk, dim3 grid, hipStream_t s, const rtxd::DevScene& d,
                     const rtxd::AdaptiveArgs& A);

}  // namespace rtxh
