// hk_launch.h — the launch layer: which kernel instantiation runs for a scene, a pass and a knob table.  Defined in hk_launch_impl.h and
// hk_test_kernels.h (both part of the hk_kernels.hip translation unit), called from the host files (hk_render.cpp, hk_film.cpp, hk_scene_edit.cpp, hk_test_api.cpp).  This is the only declaration of it.
#pragma once
#include "hikari_mi355x.h"
#include "hk_types.h"

namespace hk {

// A LEAN scene: no medium and no pass-through surface (alpha-tested or medium-transition triangle).  Its rays run through k_trace_lean /
// k_shadow / k_small_pass, and its path state is laid out for them (slim shadow records, 32-bit meta words: ensure_state) — the kernels
// and the layout must agree, or MIS weights are read from the wrong words.  Every site asks this one predicate.
inline bool lean_scene(const DScene& sc) { return sc.all_opaque != 0 && sc.n_media == 0; }
// HK_WALK_SPLIT=1: the grey medium's shadow walk runs as k_walk_cast / k_walk_track rounds instead of ONE k_shadow_walk<.., GREY>
// (measured on the BOMEX stand-in: cast rounds 0.085 s + tracking rounds 0.45 s against 0.51 s unsplit — off by default).  The path
// state of such a pass carries hand-over queues (ensure_state).
inline int walk_split_mode() { return knob_int("HK_WALK_SPLIT", 0); }

bool grey_compact_ok(const DScene& sc);
bool preselect_lights(const DScene& sc, const DPathState& st);
bool small_pass_fusable(const DScene& sc, uint32_t kinds_mask);

// ---- the stages of a pass ----
void launch_camera(hipStream_t s, int n_cu, const DPathState& st, const DFrame& fr, const DTables& T, const DFilter& flt, const DCamera& cam, const DSobol& sob, int initial_medium);
void launch_trace(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, int depth, DStats* stats);
void launch_shadow(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, int depth, DStats* stats);
void launch_escaped(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, int depth);
void launch_medium(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DSobol& sob, int depth, DStats* stats);
void launch_detect_camera_medium(hipStream_t s, const DPathState& st, const DScene& sc, float x, float y, float z, DStats* stats);
void launch_light_select(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DSobol& sob, int depth, uint32_t kinds_mask, DStats* stats);
void launch_shade(hipStream_t s, int n_cu, int kind, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DSobol& sob, int depth, int first_kind, DStats* stats);
// the whole pass of a small call in one launch; -> false when this scene / pass is not its case (the caller launches the stages).
// dry: only say whether it would be launched; film_mode: 0 the caller launches k_film, 1 / 2: float / double accumulators, added inside
bool launch_small_pass(hipStream_t s, int n_cu, const DPathState& st, const DScene& sc, const DTables& T, const DFrame& fr, const DFilter& flt, const DCamera& cam, const DSobol& sob, int max_depth,
                       uint32_t kinds_mask, DStats* stats, bool dry, void* accum, int film_mode);
void launch_segment_lists(hipStream_t s, const DPathState& st, int n, const int* depths, const int* queues);
void launch_film(hipStream_t s, const DPathState& st, const DFrame& fr, const DTables& T, void* accum, bool f64);

// ---- sampler tables, image passes, scene edits ----
void launch_sobol_table(hipStream_t s, const DSobol& sob, const DFrame& fr, uint2* table, int rows);
void launch_sobol_lo_table(hipStream_t s, const DSobol& sob, const DFrame& fr, uint16_t* table, int rows, int base, int stride, int count);
// the display chain (hk_display.h), one launcher per stage over the pixel layout (PlanarPixels / PackedPixels, hk_types.h)
template <class Layout> void launch_finalize(hipStream_t s, const void* accum, bool f64, Layout out, int w, int h);
template <class Layout> void launch_aux(hipStream_t s, const DScene& sc, const DCamera& cam, int h, int w, float miss_depth, float* albedo, Layout out);
template <class Layout> void launch_variance(hipStream_t s, Layout src, float* variance, int h, int w);
template <class Layout> void launch_postprocess(hipStream_t s, const hk_postprocess_params& P, Layout src, float* out, int h, int w);
// one a-trous pass src -> dst; packed: out != nullptr makes it the LAST pass, which writes the 3-float frame `out` (pp != nullptr: postprocessed)
void launch_atrous(hipStream_t s, const hk_denoise_params& P, int step, PlanarPixels src, const float* variance, PlanarPixels dst, int h, int w);
void launch_atrous(hipStream_t s, const hk_denoise_params& P, int step, PackedPixels src, const float* variance, PackedPixels dst, float* out, const hk_postprocess_params* pp, int h, int w);
void launch_slot_of_prim(hipStream_t s, const float4* leaf, int n, int* slot_of_prim);
// the geometry table of a whole scene (DScene::tri_geo: the float offset of its rows behind `pos`; shade: the packed records hold them instead)
void launch_tri_geo(hipStream_t s, float* pos, int n, int tri_geo, float* shade);
void launch_xform_tris(hipStream_t s, const DXform& X, int first, int n, const float* bp, const float* bn, const float* bt, const int* slot_of_prim, float* pos, float* nrm, float* tan, float* shade,
                       float4* geo, float4* leaf);
void launch_refit_level(hipStream_t s, int begin, int end, DNode* nodes, DQNode* qnodes, const DQGrid& grid, const float4* leaf, const float* pos);
// hk_scene_set_vertices: one pass over the uploaded range (base copies, transform, every copy of the geometry, leaf slots)
void launch_set_tris(hipStream_t s, const DSetTris& A);
// hk_scene_refit_lights: the edited records and leaves into place (one lane per edited light), then the stamped inner entries of one
// depth of the light BVH (`entries`: that depth's slice of the scene's list), called deepest depth first
void launch_light_refit_leaves(hipStream_t s, const DLightRefit& A);
void launch_light_refit_level(hipStream_t s, const int* entries, int count, const DLightRefit& A);
// hk_scene_bvh_cost: partial[b] = the cost terms of nodes [256 b, 256 b + 256) (bvh_cost_blocks(n) of them)
inline int bvh_cost_blocks(int n_nodes) { return (n_nodes + 255) / 256; }
void launch_bvh_cost(hipStream_t s, const DNode* nodes, int n, double* partial);
// hk_scene_rebuild_bvh: the topology of a new tree over B.pos into B.nodes / B.qnodes / B.order / B.ctl (boxes: launch_refit_level
// afterwards), then the leaf records of that order
void launch_bvh_build(hipStream_t s, const DBuild& B);
void launch_bvh_build_leaves(hipStream_t s, const DBuildLeaves& A);
void launch_envmap_tables(hipStream_t s, const DEnvMap& e, DEnvMap* record);
// hk_scene_update_envmap_sky: the res x res texels of a Hosek-Wilkie sky into `data` (launch_envmap_tables follows)
void launch_sky_texels(hipStream_t s, const hk_sky_params& sky, int res, float4* data);
// hk_scene_update_medium: majorant grid + zero-cell mask of a Grid / RGB grid / NanoVDB medium, and the NanoVDB halo bricks, from the data `m` points to
void launch_majorant_grid(hipStream_t s, const DMedium& m);
void launch_majorant_nanovdb(hipStream_t s, const DMedium& m, const DIndexBox& index_bbox);
void launch_nvdb_bricks(hipStream_t s, const DMedium& m, size_t n_blocks);
// hk_scene_update_medium_dense (hk_nvdb_build.h): the flags, node numbering and counts of the tree of a dense field into D.lev / D.ctl;
// then, once the host has read D.ctl and sized the tree, the tree's bytes and its block table
void launch_dense_count(hipStream_t s, const DDense& D);
void launch_dense_emit(hipStream_t s, const DDense& D, const uint32_t count[3], size_t n_bytes);

// ---- sub-kernel entry points of the parity tests (hk_test_kernels.h) ----
void launch_test_trace(hipStream_t s, const DScene& sc, int n, const float* o, const float* d, const float* tmax, float* t, int* prim, float* uv);
// hk_test_tri_geo: out[t] = the geometry table's row of triangle t (recompute 0) or tri_geo_of of its world positions (1)
void launch_test_tri_geo(hipStream_t s, const DScene& sc, int recompute, float4* out);
void launch_test_trace_lean(hipStream_t s, int n_cu, const DScene& sc, int anyhit, int n, const float* o, const float* d, const float* tmax, float* t, int* prim, float* uv);
void launch_test_sobol(hipStream_t s, const DTables& T, const DSobol& sob, int n, const int* px, const int* py, const int* si, const int* dim, float* o1, float* o2);
void launch_test_camera(hipStream_t s, const DTables& T, const DFilter& flt, const DCamera& cam, const DSobol& sob, int height, int n, const int* px, const int* py, const int* si, float* out);
void launch_test_uplift(hipStream_t s, const DTables& T, int mode, int n, const float* rgb, const float* lam, float* out);
void launch_test_light_bvh(hipStream_t s, const DScene& sc, int n, const float* p, const float* nn, const float* u, int* out_light, float* out_pmf, const int* query, float* out_qpmf);
void launch_test_light(hipStream_t s, const DScene& sc, const DTables& T, int mode, int light_idx, int n, const float* p3, const float* in3, const float* lambda, float* out);
void launch_test_bsdf(hipStream_t s, const DScene& sc, const DTables& T, int mode, int mat_idx, int regularize, int n, const float* wo, const float* wi, const float* ns, const float* lambda,
                      const float* u, const float* uc, float* out);
void launch_test_mix(hipStream_t s, const DScene& sc, int mat_idx, int n, const float* p3, const float* wo3, const float* uv2, int* out);
void launch_test_medium(hipStream_t s, const DScene& sc, const DTables& T, int mode, int medium_idx, int n, const float* a3, const float* b3, const float* tmax, const float* lambda, float* out);
int test_majorant_stride();

}  // namespace hk
