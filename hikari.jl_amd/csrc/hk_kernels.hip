// hk_kernels.hip — the device code of the library for gfx950 (wave64): ONE translation unit (DESIGN.md §4 describes the pass).
// The headers are slices of it, not modules: each uses what stands above it, and the order of the kernels in the code object is the
// order of this list.  Keep the order; a new kernel goes into the header of its stage.  This file holds no code of its own:
//     hk_device.h, hk_edit_host.h, hk_bvh_decide.h, hk_sky.h, hk_light_bounds.h    not slices: the device library, and the arithmetic shared with the host
//     hk_wave_queues.h    lane_id, WaveQ, segment tickets and loops, streaming loads / stores, record loaders, HK_DBG*
//     hk_camera_stage.h    k_sobol_table, k_segment_lists, k_sobol_lo_table, k_camera                                      [K1]
//     hk_traverse.h        LDS cache fills, k_trace, the per-lane ray state machine, k_trace_lean                          [K3]
//     hk_track.h           k_track, k_track_flat, k_track_pool, k_scatter, k_detect_camera_medium                         [K4-K6]
//     hk_shade.h           k_escaped, k_light_select, k_light_select_pool, k_shade                               [K7, K2,K8,K9,K11]
//     hk_shadow.h          shadow_contribute*, k_shadow, trace_shadow_body                                                 [K10]
//     hk_small_pass.h      k_small_pass: all stages of a small pass in one launch
//     hk_shadow_walk.h     k_shadow_walk, k_walk_pool, k_walk_cast, k_walk_track                                           [K10]
//     hk_film_kernels.h    the film fold and k_film                                                                        [K12]
//     hk_display.h         the display chain                                                                               [K13]
//     hk_edit_kernels.h    k_slot_of_prim, k_tri_geo, k_xform_tris, k_refit_level, k_set_tris, k_light_refit_*, k_bvh_cost: the scene edits
//     hk_build_kernels.h   k_build_*: the device BVH build
//     hk_table_kernels.h   k_envmap_*, k_majorant_*, k_nvdb_bricks
//     hk_nvdb_build.h      a NanoVDB tree from a dense field
//     hk_sky_kernels.h     k_sky_texels: a Hosek-Wilkie sky baked into an environment map
//     hk_launch_impl.h     the launch layer (hk_launch.h), which names every kernel
//     hk_test_kernels.h    the parity tests' entry points
#include <hip/hip_runtime.h>
#include <type_traits>
#include <cstdlib>
#include <cstdio>

#include "hikari_mi355x.h"
#include "hk_device.h"
#include "hk_edit_host.h"
#include "hk_bvh_decide.h"
#include "hk_sky.h"
#include "hk_light_bounds.h"

using namespace hkd;

namespace {
#include "hk_wave_queues.h"
}  // namespace
#include "hk_camera_stage.h"
#include "hk_traverse.h"
#include "hk_track.h"
#include "hk_shade.h"
#include "hk_shadow.h"
#include "hk_small_pass.h"
#include "hk_shadow_walk.h"
#include "hk_film_kernels.h"
#include "hk_display.h"
#include "hk_edit_kernels.h"
#include "hk_build_kernels.h"
#include "hk_table_kernels.h"
#include "hk_nvdb_build.h"
#include "hk_sky_kernels.h"
#include "hk_launch_impl.h"
#include "hk_test_kernels.h"
