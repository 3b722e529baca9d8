/*
 * hikari_mi355x.h — C ABI of the MI355X-native VolPath hot path.
 *
 * This is the drop-in boundary for ONE path of JuliaGraphics/Hikari.jl: the per-ray inner loop
 * of the `VolPath` integrator.  The reference has no FFI for it: callers invoke
 *
 *     integrator(scene, film, camera)          src/integrators/volpath/volpath.jl:655-670
 *     render!(integrator, scene, film, camera) src/integrators/volpath/volpath.jl:445-636
 *     clear!(integrator)                       src/integrators/volpath/volpath.jl:108-113
 *     close(integrator)                        src/Hikari.jl:47
 *
 * A Julia shim (julia/HikariMI355X.jl) subtypes `Hikari.Integrator`, flattens
 * `Scene`/`Film`/`Camera` into the POD records below and `ccall`s these entry points.
 *
 * Conventions
 *  - every entry point returns int32 status: 0 = ok, <0 = error; hk_last_error() gives the text.
 *  - no exceptions cross the boundary; one hk_ctx is used from one thread at a time.
 *  - host input buffers are borrowed for the duration of the call and copied to the device.
 *  - indices inside records are 0-based unless the field name says `_1based`; -1 means "none".
 *  - arrays described as "Julia layout" are column-major exactly as the Julia arrays they replace.
 *  - all floating point is IEEE binary32 unless stated.
 */
#ifndef HIKARI_MI355X_H
#define HIKARI_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HK_OK 0
#define HK_ERR_INVALID -1
#define HK_ERR_DEVICE -2
#define HK_ERR_UNSUPPORTED -3
#define HK_UNSET -100 /* hk_ctx_get_option: the knob has no value (distinct from every error code) */

/* ---------------------------------------------------------------------------------------------
 * Textures (reference: textures/texture-ref.jl:151-186 bilinear fetch with the (1-v, u) flip).
 * data = Julia Matrix [height, width] of `channels` floats per texel (column-major: texel (iy,ix)
 * at ((iy + height*ix) * channels)).  channels is 1 (Float32 texture) or 4 (RGBSpectrum r,g,b,a).
 * ------------------------------------------------------------------------------------------- */
typedef struct hk_texture {
    int32_t width, height, channels;
    int32_t kind; /* 0: 2-D image (above).  1: VertexColorTexture (textures/basic.jl:42-46; texture-ref.jl:230-235):
                     data = face_colors[3, n_faces] (Julia layout: the 3 colours of a face are adjacent), height = 3,
                     width = n_faces; looked up with the hit's face index and barycentrics, not with uv */
    const float* data;
} hk_texture;

/* A material parameter that is either a constant or a texture reference (texture-ref.jl:50-84). */
typedef struct hk_tex_rgba {
    float c[4];  /* constant r,g,b,alpha (RGBSpectrum is 4 floats, spectrum.jl:38-43) */
    int32_t tex; /* -1 => constant `c`; otherwise index into hk_scene_desc.textures */
} hk_tex_rgba;

typedef struct hk_tex_f32 {
    float v;
    int32_t tex;
} hk_tex_f32;

/* ---------------------------------------------------------------------------------------------
 * Materials (Appendix A of SURVEY.md; uber-material.jl:180-215,378-384; coated-*.jl;
 * thin-dielectric.jl:45-47; diffuse-transmission.jl:39-43; mix-material.jl).
 * One tagged record; which slots a kind reads is listed next to the kind.
 * ------------------------------------------------------------------------------------------- */
enum {
    HK_MAT_MATTE = 0,            /* rgb[0]=Kd, f[0]=sigma */
    HK_MAT_MIRROR = 1,           /* rgb[0]=Kr */
    HK_MAT_GLASS = 2,            /* rgb[0]=Kr, rgb[1]=Kt, f[0]=index (roughness ignored, Q12) */
    HK_MAT_CONDUCTOR = 3,        /* rgb[0]=eta, rgb[1]=k (or spectrum[0/1]), f[0]=roughness, flags&REMAP */
    HK_MAT_COATED_DIFFUSE = 4,   /* rgb[0]=reflectance, rgb[1]=albedo, f[0]=u_rough, f[1]=v_rough,
                                    f[2]=thickness, f[3]=eta, f[4]=g, i[0]=max_depth, i[1]=n_samples */
    HK_MAT_THIN_DIELECTRIC = 5,  /* f[0]=eta */
    HK_MAT_DIFFUSE_TRANSMISSION = 6, /* rgb[0]=reflectance, rgb[1]=transmittance, f[0]=scale */
    HK_MAT_COATED_DIFFUSE_TRANSMISSION = 7, /* rgb[0]=reflectance, rgb[1]=transmittance, rgb[2]=albedo,
                                    f[0..4] as coated diffuse, i[0], i[1] */
    HK_MAT_COATED_CONDUCTOR = 8, /* rgb[0]=conductor eta, rgb[1]=conductor k, rgb[2]=reflectance,
                                    rgb[3]=albedo, f[0]=iface u_rough, f[1]=iface v_rough, f[2]=iface eta,
                                    f[3]=cond u_rough, f[4]=cond v_rough, f[5]=thickness, f[6]=g,
                                    i[0]=max_depth, i[1]=n_samples, flags&USE_ETA_K */
    HK_MAT_MIX = 9,              /* f[0]=amount, i[0]=material1, i[1]=material2 (indices into materials), mix_key */
    HK_MAT_FALLBACK = 10         /* any other Material (e.g. a bare Emissive): gray 0.5 Lambertian, Q24 */
};
#define HK_MATF_REMAP_ROUGHNESS 1
#define HK_MATF_USE_ETA_K 2

typedef struct hk_material {
    int32_t kind;
    int32_t flags;
    hk_tex_rgba rgb[4];
    hk_tex_f32 f[8];
    int32_t i[4];
    int32_t spectrum[2];  /* piecewise-linear spectrum ids for eta / k, -1 => use rgb slot */
    /* Mix only: the SetKeys of the two sub-materials as the reference hashes them
       (mix-material.jl:96-127): {type_idx1, vec_idx1, type_idx2, vec_idx2}. */
    uint32_t mix_key[4];
} hk_material;

/* PiecewiseLinearSpectrum (spectral/piecewise-linear.jl; metal-spectra.jl): n (lambda, value) knots. */
typedef struct hk_pl_spectrum {
    int32_t n;
    int32_t _pad;
    const float* lambdas;
    const float* values;
} hk_pl_spectrum;

/* MediumInterfaceIdx (materials/medium-interface.jl:76-80). */
typedef struct hk_medium_interface {
    int32_t material; /* index into materials */
    int32_t inside;   /* index into media, -1 = vacuum */
    int32_t outside;
} hk_medium_interface;

/* TriangleMeta (scene.jl:11-15). */
typedef struct hk_tri_meta {
    uint32_t medium_interface_idx; /* 0-based index into media_interfaces */
    uint32_t primitive_index;      /* face index within its mesh, as the reference stores it (1-based) */
    uint32_t arealight_flat_idx_1based; /* flat index into lights, 0 = no area light */
} hk_tri_meta;

/* ---------------------------------------------------------------------------------------------
 * Lights (src/lights; flat order = the reference's flat light index, light-sampler.jl:289-329).
 * ------------------------------------------------------------------------------------------- */
enum {
    HK_LIGHT_POINT = 0,
    HK_LIGHT_SPOT = 1,
    HK_LIGHT_DIRECTIONAL = 2,
    HK_LIGHT_SUN = 3,
    HK_LIGHT_AMBIENT = 4,
    HK_LIGHT_ENVIRONMENT = 5,
    HK_LIGHT_DIFFUSE_AREA = 6
};
enum {
    HK_SPEC_RGB = 0,       /* RGBSpectrum: uplifted at run time with uplift_rgb_illuminant */
    HK_SPEC_ILLUMINANT = 1 /* RGBIlluminantSpectrum{poly(c0,c1,c2), scale} (rgb2spec.jl:317-335) */
};

typedef struct hk_light {
    int32_t kind;
    int32_t spectrum_kind;
    float i_rgb[4];       /* RGBSpectrum i / scale (environment) */
    float poly[3];        /* RGBIlluminantSpectrum coefficients */
    float illum_scale;    /* RGBIlluminantSpectrum.scale */
    float scale;          /* light.scale (Q4) */
    float position[3];    /* point, spot */
    float direction[3];   /* directional, sun: travel direction, normalised */
    float world_to_light[16]; /* spot, row-major 4x4 */
    float light_to_world[16];
    float cos_total_width, cos_falloff_start; /* spot */
    /* diffuse area (lights/diffuse-area.jl:25-33) */
    float v[9];
    float normal[3];
    float area;
    float uv[6];
    hk_tex_rgba Le;
    int32_t two_sided;
    int32_t envmap; /* environment: index into envmaps */
} hk_light;

/* EnvironmentMap + Distribution2D (textures/environment_map.jl:9-45; sampler/sampling.jl:179-262). */
typedef struct hk_envmap {
    int32_t width, height;    /* data is Julia Matrix{RGBSpectrum}[height,width], 4 floats per texel */
    const float* data;
    float rotation[9];        /* 3x3 row-major */
    int32_t nu, nv;
    const float* conditional_func;     /* [nu, nv]   Julia layout */
    const float* conditional_cdf;      /* [nu+1, nv] */
    const float* conditional_func_int; /* [nv] */
    const float* marginal_func;        /* [nv] */
    const float* marginal_cdf;         /* [nv+1] */
    float marginal_func_int;
    int32_t _pad;
} hk_envmap;

/* ---------------------------------------------------------------------------------------------
 * Media (volpath/media.jl, nanovdb.jl) — records are defined now so the ABI is stable.
 * ------------------------------------------------------------------------------------------- */
enum { HK_MEDIUM_HOMOGENEOUS = 0, HK_MEDIUM_GRID = 1, HK_MEDIUM_RGB_GRID = 2, HK_MEDIUM_NANOVDB = 3 };

typedef struct hk_medium {
    int32_t kind;
    float sigma_a[4], sigma_s[4], Le[4]; /* RGBSpectrum */
    float g;
    float sigma_scale, Le_scale;
    /* grid media */
    float bounds_min[3], bounds_max[3];
    float render_to_medium[16], medium_to_render[16]; /* row-major */
    int32_t res[3];
    const float* density;      /* Grid: [nx,ny,nz] Julia layout (x fastest) */
    const float* sigma_a_grid; /* RGBGrid: rgba [nx,ny,nz] or NULL */
    const float* sigma_s_grid;
    const float* Le_grid;
    int32_t majorant_res[3];
    const float* majorant;     /* [rx*ry*rz], index x + rx*(y + ry*z) */
    float max_density;
    /* NanoVDB */
    const uint8_t* nvdb_bytes;
    int64_t nvdb_size;
    int64_t root_offset_1based, upper_offset_1based, lower_offset_1based, leaf_offset_1based;
    int32_t upper_count, lower_count, leaf_count, root_table_size;
    float inv_mat[9], vec[3];
    int32_t index_bbox_min[3], index_bbox_max[3];
} hk_medium;

/* ---------------------------------------------------------------------------------------------
 * Scene: flat triangle soup (world space) + records.  Triangle t has vertices
 * positions[9t..9t+8]; normals/uvs/tangents follow the same [T][3][k] layout, NULL = absent
 * (NaN normals/tangents per triangle also mean absent: intersection.jl:136-139,93).
 * Absent uvs default to (0,0),(1,0),(1,1).
 * ------------------------------------------------------------------------------------------- */
typedef struct hk_scene_desc {
    int32_t n_triangles;
    int32_t n_materials;
    int32_t n_textures;
    int32_t n_media_interfaces;
    int32_t n_lights;
    int32_t n_envmaps;
    int32_t n_media;
    int32_t n_spectra;
    const float* positions;
    const float* normals;
    const float* uvs;
    const float* tangents;
    const hk_tri_meta* meta;
    const hk_material* materials;
    const hk_texture* textures;
    const hk_medium_interface* media_interfaces;
    const hk_light* lights;
    const hk_envmap* envmaps;
    const hk_medium* media;
    const hk_pl_spectrum* spectra;
} hk_scene_desc;

/* Data tables the reference embeds in its sources; the caller hands them over once per context.
 * sobol: SobolMatrices32 (sampler/sobol_matrices.jl, 1024 x 52 uint32; only dims 0,1 are read)
 * cie:   CIE_X, CIE_Y, CIE_Z 1-nm tables 360..830 (spectral/color.jl:53-345)
 * rgb2spec: RGBToSpectrumTable (spectral/rgb2spec.jl:71-75): coeffs[3,res,res,res,3] Julia layout. */
typedef struct hk_tables {
    const uint32_t* sobol_matrices;
    int32_t sobol_count; /* number of uint32 (>= 104) */
    int32_t rgb2spec_res;
    const float* cie_x;
    const float* cie_y;
    const float* cie_z; /* 471 floats each */
    const float* rgb2spec_scale;
    const float* rgb2spec_coeffs;
} hk_tables;

/* VolPath parameters (volpath.jl:29-101) + pixel filter (filter.jl:574-604). */
enum { HK_FILTER_BOX = 1, HK_FILTER_TRIANGLE = 2, HK_FILTER_GAUSSIAN = 3, HK_FILTER_MITCHELL = 4, HK_FILTER_LANCZOS = 5 };
enum { HK_COHERENCE_NONE = 0, HK_COHERENCE_SORTED = 1, HK_COHERENCE_PER_TYPE = 2 };

typedef struct hk_integrator_params {
    int32_t max_depth;              /* default 8 */
    int32_t samples_per_pixel;      /* default 64 */
    int32_t russian_roulette_depth; /* carried, unused by the kernels (Q7) */
    int32_t regularize;             /* default 1 */
    int32_t material_coherence;     /* result-neutral knob; the HIP path always sorts by material kind */
    float max_component_value;      /* default 10 */
    int32_t filter_type;            /* default HK_FILTER_GAUSSIAN */
    float filter_radius[2];         /* default 1.5, 1.5 */
    float filter_param1;            /* sigma (Gaussian, default 0.5) | B (Mitchell) | tau (Lanczos) */
    float filter_param2;            /* C (Mitchell) */
    int32_t accumulate_f64;         /* accumulation_eltype == Float64 */
    uint32_t sampler_seed;          /* reference fixes 0 (volpath.jl:480) */
    int32_t samples_per_pass;       /* HIP-only tuning: samples in flight per wavefront pass (0 = auto) */
} hk_integrator_params;

/* One record covers PerspectiveCamera (camera/perspective.jl:41-128) and MatrixCamera
 * (camera/matrix.jl:13-58, lens_radius = 0).  Matrices are row-major 4x4. */
typedef struct hk_camera {
    float raster_to_camera[16];
    float camera_to_world[16];
    float lens_radius, focal_distance;
    float shutter_open, shutter_close;
    float dx_camera[3], dy_camera[3];
} hk_camera;

typedef struct hk_stats {
    uint64_t rays_closest;     /* closest-hit casts from camera/indirect segments (K3) */
    uint64_t rays_shadow;      /* closest-hit casts from shadow segments (K10) */
    uint64_t bvh_nodes_visited;
    uint64_t tris_tested;
    uint64_t hits_accepted;
    uint64_t path_vertices;    /* surface shading events */
    uint64_t medium_collisions;
    uint64_t light_bvh_nodes;
    double seconds_trace;      /* HIP-event time spent in the closest-hit traversal kernel (k_trace) */
    double seconds_total;      /* HIP-event span from the first hk_render after hk_stats_reset to the last */
    uint64_t trace_launches;
    /* per-kernel-class breakdown (filled when hk_stats_enable_counters flags are set) */
    uint64_t trace_nodes, trace_tris;    /* k_trace only (needs flag bit 0) */
    uint64_t shadow_nodes, shadow_tris;  /* k_shadow only */
    uint64_t shadow_launches, shade_launches;
    double seconds_shadow, seconds_shade, seconds_other; /* HIP-event sums (flag bit 1) */
    /* ALGORITHMIC bytes of the three hot kernel classes, SURVEY 8(d): per cast 32 (ray in) + 64 per BVH node visited + 36 per
       triangle tested + 96 per accepted hit (closest-hit only) + 16 (hit out); per path vertex 2*104 (state read + written) + 64
       (material record) + 96 (light record) + 60 per light-BVH node.  The node / triangle terms need counter flag bit 0. */
    uint64_t bytes_algorithmic_trace, bytes_algorithmic_shadow, bytes_algorithmic_shade;
    double seconds_media;      /* HIP-event sum of the delta-tracking kernels (k_track + k_scatter); not part of seconds_other */
    /* media class (84 B per collision through a NanoVDB tree / 36 B on a dense grid, 4 B per majorant cell entered).
       medium_collisions above = track_collisions + shadow_collisions. */
    uint64_t track_collisions, shadow_collisions;   /* tentative collisions of delta tracking (K4) / of the shadow rays' ratio tracking (K10) */
    uint64_t track_dda_steps, shadow_dda_steps;     /* majorant cells entered by K4 / by K10 */
    uint64_t scatter_vertices;                      /* real scattering events handed to K5 + K6 */
    uint64_t media_launches;                        /* k_track + k_scatter launches */
    /* collisions x 84|36 + 4 x DDA steps of K4, + (2 x 104 state + 96 light record) per scattering vertex of K5 + K6;
       bytes_algorithmic_shadow likewise includes the shadow walk's collisions and DDA steps */
    uint64_t bytes_algorithmic_media;
    /* the part of seconds_shade spent choosing the next-event light in a kernel of its own (scenes with a deep light BVH: k_light_select*),
       and its launches (not part of shade_launches) */
    double seconds_select;
    uint64_t select_launches;
    /* passes rendered as ONE launch (k_small_pass: camera rays and every bounce of a small pass of a closed all-matte scene; the film
       kernel follows).  Their stages are not counted in *_launches. */
    uint64_t fused_passes;
    /* passes that kept the camera records of the pass before them on the same path state and did not launch k_camera (the view
       cache: one-pass frames of an unchanged view; HK_VIEW_CACHE=0 turns it off) */
    uint64_t view_cache_hits;
} hk_stats;

typedef struct hk_ctx hk_ctx;
typedef struct hk_scene hk_scene;
typedef struct hk_film hk_film;
typedef struct hk_integrator hk_integrator;

/* Context: one per GPU.  `stream` is a hipStream_t (0 = default stream); it lets the host harness
 * run the path on a stream it owns (torch.cuda.Stream().cuda_stream). */
int32_t hk_ctx_create(int32_t device_id, void* stream, hk_ctx** out);
int32_t hk_ctx_destroy(hk_ctx* ctx);
const char* hk_last_error(void);
int32_t hk_ctx_set_tables(hk_ctx* ctx, const hk_tables* tables);
/* Tuning knobs (the HK_* table of INTEGRATION.md).  The library reads the environment ONCE, in hk_ctx_create — never on a render
 * path — and keeps the values in the context; hk_ctx_set_option changes one afterwards (value NULL: back to the built-in default).
 * Calls that were only noted (see hk_render) are rendered first, under the options they were made with.  Unknown names are
 * HK_ERR_INVALID.  hk_ctx_get_option: length of the value (copied to `out`, NUL-terminated, at most out_bytes); HK_UNSET — not an error:
 * the built-in default applies, `out` becomes the empty string — when the knob has no value.
 * There is no reference counterpart: Hikari's knobs are keyword arguments of VolPath(...) (volpath.jl:55-106), carried here by
 * hk_integrator_params. */
int32_t hk_ctx_set_option(hk_ctx* ctx, const char* name, const char* value);
int32_t hk_ctx_get_option(hk_ctx* ctx, const char* name, char* out, int32_t out_bytes);
/* Gives the path-state slabs this process keeps cached for `ctx`'s device back to the driver (a destroyed integrator's path
 * state — up to HK_STATE_CACHE_GB = 128 in total — is otherwise kept for the next one: allocating 84 GB takes seconds). */
int32_t hk_trim_cache(hk_ctx* ctx);

/* Scene: copies the description, builds the BVH + light BVH on the host, uploads. */
int32_t hk_scene_create(hk_ctx* ctx, const hk_scene_desc* desc, hk_scene** out);
int32_t hk_scene_destroy(hk_scene* scene);

/* ---------------------------------------------------------------------------------------------
 * Editing a scene in place (update_transform!, src/surface_interaction.jl:413-423; update_material!, src/scene.jl:104-112).
 * Every call first renders the noted calls (see hk_render: they were made against the scene as it was), then enqueue their work on
 * ctx's stream behind everything already enqueued, and return without waiting for the device.  Films are not cleared.  A refused
 * call (HK_ERR_INVALID, hk_last_error says why) leaves the scene untouched.
 *
 * hk_scene_set_transform: the world positions, normals and tangents of triangles [first_tri, first_tri + n_tris) become m34 (3x4
 * row-major affine) applied to the values those triangles had at hk_scene_create or were given by the last hk_scene_set_vertices
 * ("base"); the BVH keeps its topology and its boxes are refit on the device (traversal slows as the boxes of a tree built for the old
 * geometry grow and overlap: the quantity to watch is cost_now / cost_created of hk_scene_bvh_cost).  Area lights and the light BVH stay
 * as created (they are built from the un-transformed mesh, Q18).  Binary32 without contraction, in this order:
 *   points    p'[k] = ((m[k][0]*x + m[k][1]*y) + m[k][2]*z) + m[k][3]
 *   normals   A = m[:, 0..2]; C[i][j] = A[i+1][j+1]*A[i+2][j+2] - A[i+1][j+2]*A[i+2][j+1] (indices mod 3) and
 *             det = (A[0][0]*C[0][0] + A[0][1]*C[0][1]) + A[0][2]*C[0][2] in double; N[i][j] = (float)(C[i][j] / det);
 *             n'[k] = (N[k][0]*nx + N[k][1]*ny) + N[k][2]*nz, then n' / sqrt((n'x*n'x + n'y*n'y) + n'z*n'z) (division and square root
 *             correctly rounded); a normal with a NaN component (none given) is kept as it is
 *   tangents  as normals with A in place of N
 *   identity  an m34 that is exactly [I | 0] copies the base values back (the scene as created, bit for bit)
 * Refused: a null pointer, a scene without triangles, n_tris < 1 or a range outside the scene, a non-finite or singular m34.
 *
 * hk_scene_set_vertices: the arrays given become the new BASE geometry of triangles [first_tri, first_tri + n_tris): positions and, where
 * given, normals and tangents (9 floats per triangle each) and uvs (6 per triangle).  A NULL normals / tangents / uvs keeps that
 * attribute's base values for the range.  Transforms are kept: each triangle of the range is put under the transform in force on it
 * (the last hk_scene_set_transform that covered it, the identity otherwise — a range may straddle several), by the arithmetic above,
 * an identity as a copy; uvs are not transformed.  The triangle count, the BVH topology, materials and which triangles emit do not
 * change; the boxes are refit as for hk_scene_set_transform, and area lights and the light BVH stay as they are (Q18).  The arrays are
 * borrowed for the call (copied through pinned memory owned by the scene) and cross to the device once; one kernel rewrites every copy
 * of the geometry.  A range larger than any before grows a device buffer, which waits for earlier edits of the scene — the one wait.
 * Refused: a null scene or positions, a scene without triangles, n_tris < 1 or a range outside the scene, a non-finite position,
 * normals / tangents / uvs for a scene created without that array (which arrays exist selects code paths and cannot change).
 *
 * hk_scene_update_materials: material records [first, first + n) of hk_scene_desc::materials are replaced by materials[0 .. n-1]
 * (upload through pinned memory owned by the scene).  Refused: a null pointer, n < 1 or a range outside the scene, and a record that
 * changes its kind, a Mix's children (i[0], i[1], mix_key), its opacity class (Matte with an alpha texture or alpha < 1) or names a
 * texture / spectrum index that is out of range.  ONE change of kind is accepted: a record may become a MixMaterial whose children are
 * materials of the scene, and a MixMaterial may become a material of a kind that a non-Mix record of the scene had at hk_scene_create
 * (either way the scene shades only kinds it was created for; whether it holds a Mix selects the closest-hit kernel of the next call).
 *
 * hk_scene_update_lights: light records [first, first + n) of hk_scene_desc::lights are replaced by lights[0 .. n-1].  Everything but
 * `kind` may change (spectrum, scale, position, direction, the spot matrices and cosines; v, normal, area, uv, Le, two_sided of an area
 * light).  The light BVH is REBUILT on the host from the scene's whole light array, by the builder hk_scene_create uses, and uploaded
 * with the baked records: the pmf of the light sampler depends on the tree's shape, and the scene after the call is, bit for bit, the
 * scene hk_scene_create builds from the edited description.  A light whose power becomes 0 leaves the tree, one whose power becomes
 * positive enters it.  The triangles of an area light are not moved by this call (nor is a light moved by hk_scene_set_transform).
 * Refused: a null pointer, n < 1 or a range outside the scene, a record whose kind differs from the one it replaces, an environment
 * light whose `envmap` or an area light whose `Le.tex` is out of range.
 *
 * hk_scene_update_envmap: environment map `idx` of hk_scene_desc::envmaps gets new texels (`data`: width x height texels in the layout
 * of hk_envmap::data, the sizes unchanged), a new `rotation` (3x3 row-major), or both; either pointer may be NULL, not both.  A rotation
 * alone rewrites the nine floats of the device record.  With texels the Distribution2D tables are rebuilt ON THE DEVICE from them
 * (sampler/sampling.jl:179-262 over to_Y of the texels, textures/environment_map.jl:24-45), binary32 without contraction, division
 * correctly rounded, every sum sequential in index order:
 *   func[v][u]    = (0.212671f*r + 0.715160f*g) + 0.072169f*b                    of texel (v, u)
 *   row v         c[0] = 0, c[u+1] = c[u] + func[v][u] / (float)nu;  func_int[v] = c[nu];
 *                 cdf[v][u] = func_int[v] == 0 ? (float)u / (float)nu : c[u] / func_int[v]          (u = 1 .. nu; cdf[v][0] = 0)
 *   marginal      the same over func_int[0 .. nv-1] with nv in place of nu; its integral is marginal_func_int
 * Refused: a null scene, both pointers NULL, idx out of range, a non-finite rotation entry, texels for a map whose tables are not of
 * the texels' resolution (nu != width or nv != height).
 *
 * hk_scene_update_medium: medium `idx` of hk_scene_desc::media is replaced by *medium.  What may change: sigma_a, sigma_s, Le, g of every
 * kind (baked as hk_scene_create bakes them); of a Grid / RGB grid medium the voxel data (density, or sigma_a_grid / sigma_s_grid /
 * Le_grid), sigma_scale, Le_scale, bounds_* and the two transforms; of a NanoVDB medium the tree — of any size: nvdb_bytes, nvdb_size, the
 * offsets and counts, inv_mat, vec, index_bbox_* — and bounds_*.  `majorant` and `max_density` are NOT read (NULL / 0 will do): the
 * majorant grid, its zero-cell mask and the NanoVDB halo bricks are built ON THE DEVICE from the data, and are bit for bit what
 * hk_scene_create is handed by a caller that follows the reference, or builds itself:
 *   Grid        cell i of r along an axis of n voxels covers the 1-based voxels max(1, floor(i*n/r) + 1) .. min(n, ceil((i+1)*n/r))
 *               (exact integer arithmetic; media.jl:1459-1493); value = max(0, the largest density in the box)
 *   RGB grid    the same boxes; value = sigma_scale * (ma + ms) in binary32, ma / ms = max(0, the largest R, G or B of sigma_a_grid /
 *               sigma_s_grid in the box), 1 for a grid that is absent (media.jl:1122-1183)
 *   NanoVDB     per axis k the corners bounds_min[k] + (bounds_max[k] - bounds_min[k]) * i / r and ... * (i + 1) / r in binary32
 *               (product, quotient, sum), both through p -> inv_mat * (p - vec) with every row summed left to right; the inclusive integer
 *               range [floor(min - 1), ceil(max + 1)] clipped to index_bbox_*; value = max(0, the voxels of the range), a voxel outside
 *               every leaf reading its tile's or the root's background value (nanovdb.jl:1174-1235)
 *   mask        bit c set <=> value of cell c is exactly 0;  bricks: every block of the host-built block table with the first plane of
 *               its +x / +y / +z neighbours, when they fit HK_NVDB_DENSE_MB (as at creation)
 * Only the voxel grids, or the tree bytes and the block table, cross to the device, through pinned memory owned by the scene; the data is
 * borrowed for the call.  Grid data and majorant are overwritten in place.  The NanoVDB tree, block table and brick buffers are reused
 * while the new tree fits them; when one has to GROW, the call waits for the context's stream before the old buffer is released (the
 * one case in which an edit waits for the device).
 * Refused: a null pointer, idx out of range, a different kind, a different res (grid kinds) or majorant_res, an RGB grid that appears or
 * disappears, what hk_scene_create refuses of a medium record (an RGB grid medium without its grids, a NanoVDB tree with a non-background
 * root tile, too large for the block table, or with data on the table's margin), a leaf outside nvdb_size, non-finite g, bounds,
 * transforms, scales, inv_mat or vec, and an edit after which the scene's media classes would differ from those it was created with:
 * a grey medium (flat sigma_a and sigma_s) turning coloured or the reverse, bricks that no longer fit HK_NVDB_DENSE_MB or fit it for
 * the first time in a scene whose only medium is grey.  The classes select kernels and size the integrator's path state.  Every refusal
 * of this call is HK_ERR_INVALID. */
int32_t hk_scene_set_transform(hk_scene* scene, int32_t first_tri, int32_t n_tris, const float* m34);
int32_t hk_scene_set_vertices(hk_scene* scene, int32_t first_tri, int32_t n_tris, const float* positions /* 9 per triangle */,
                              const float* normals /* 9 per triangle or NULL */, const float* tangents /* 9 per triangle or NULL */,
                              const float* uvs /* 6 per triangle or NULL */);
int32_t hk_scene_update_materials(hk_scene* scene, int32_t first, int32_t n, const hk_material* materials);
int32_t hk_scene_update_lights(hk_scene* scene, int32_t first, int32_t n, const hk_light* lights);
int32_t hk_scene_update_envmap(hk_scene* scene, int32_t idx, const float* data, const float* rotation);
int32_t hk_scene_update_medium(hk_scene* scene, int32_t idx, const hk_medium* medium);

/* hk_scene_refit_lights: new records for a SET of lights, and the light BVH REFIT on the device instead of rebuilt on the host — what
 * hk_scene_set_transform is to the geometry, with hk_scene_update_lights as the rebuild.  index[0 .. n-1] are distinct 0-based indices
 * into hk_scene_desc::lights in any order, lights[j] replaces light index[j].  The topology of the tree stays: bit trails, node
 * count, the two light counts and the infinite list are unchanged.  Leaves: the bounds of an edited light are the builder's own,
 * computed on the host, so a refit leaf is bit for bit the leaf a fresh scene has for that light.  Inner nodes: every node on a path
 * from an edited leaf to the root becomes the union of its two children (box, phi = the binary32 sum, cos_e = the min, two_sided = the
 * or, the cone by the reference's DirectionCone union with two statements added: the rotation axis is made perpendicular to the first
 * child's axis again, because a kept topology pairs lights of nearly opposite axes, for which the cross product is rounding noise, and
 * the cosine of the union's angle is stepped one to two ulps towards -1, so that the cone errs to the outside), deepest first, and the
 * record the sampler walks is derived from it; every other node keeps its bits.  The union's asin / acos / sin / cos are binary32 routines of the library (csrc/hk_light_bounds.h: + - * / sqrt
 * only, the same bits on the device and on the host), NOT libm's: with those and the two statements above, the cone of a refit inner
 * node differs from a built one in its last places, also where no record changed.  Light sampling and its MIS pdf read the same tree, so a refit scene renders the same expected
 * image with another pmf — it is NOT bit for bit the scene hk_scene_create builds from the edited description, and a tree refit
 * after large moves selects lights less well than a rebuilt one.  hk_scene_update_lights (any record, also an unchanged one)
 * rebuilds from the current records and gives the fresh scene again.
 * Ordering as for every edit: noted calls render first, the work is enqueued on the context's stream, the call does not wait.  The
 * upload, through pinned memory of the scene, is proportional to the edit: n baked records and one 64-byte leaf per edited light of
 * the tree.  A scene's FIRST refit (and the first after a rebuild) also uploads the tree as built, its parent links and level lists.
 * After a refit hk_scene_light_bvh_copy reads the tree back from the device and waits for it.
 * Refused, each HK_ERR_INVALID with the scene untouched: a null pointer, n < 1 or n above the light count, an index out of range or
 * given twice, what hk_scene_update_lights refuses of a record (another kind, envmap or Le.tex out of range), a non-finite position
 * (point, spot), vertex, normal or area (area light) or bounds, and a light whose membership in the tree would change — bounded lights
 * (point, spot, area) of positive power are in the tree, infinite kinds and lights of zero power are not; an edit that moves a light
 * into or out of the tree goes through hk_scene_update_lights, and the error text says so. */
int32_t hk_scene_refit_lights(hk_scene* scene, int32_t n, const int32_t* index, const hk_light* lights);

/* hk_scene_update_medium_dense: NanoVDB medium `idx` becomes the tree of a dense density field, and the tree is built ON THE DEVICE.
 * Of *medium the call reads kind, sigma_a, sigma_s, Le, g, bounds_min, bounds_max and majorant_res (which must be unchanged) — and, like
 * hk_scene_update_medium, the two transforms; every NanoVDB field (nvdb_bytes, nvdb_size, offsets, counts, inv_mat, vec, index_bbox_*),
 * majorant and max_density are ignored.  The map is derived on the host in binary32, as the reference's dense builder derives it
 * (nanovdb.jl:602-858):
 *   d[k] = (bounds_max[k] - bounds_min[k]) / (float)res[k];   inv_mat = diag(1.0f / d[k]);   vec[k] = bounds_min[k] + d[k] / 2.0f
 * THE CONTRACT: after the call the scene holds, bit for bit, what it holds after hk_scene_update_medium with the tree that builder makes
 * of the same field (background 0): the tree bytes [root header and tiles | upper | lower | leaf nodes], every byte that is not written
 * being 0; offsets, counts and index bounding box of the record; the block table, its extent and background; majorant grid, zero-cell
 * mask and halo bricks.  The rules the bytes follow:
 *   leaf          an 8^3 block (blocks that stick out of res are padded with 0) with any voxel != 0.0f; -0.0f is background.  Its value
 *                 mask has bit (lx << 6) | (ly << 3) | lz for every voxel != 0.0f; min and max are those of the 512 values, -0.0f
 *                 ordered below +0.0f
 *   order         leaves, lower nodes (16^3 blocks) and upper nodes (32^3 lower nodes) are numbered in lexicographic (x, y, z) order of
 *                 their origins, z fastest; a child offset is relative to its parent, a root tile's to the root (key, child, state 1,
 *                 value 0)
 *   bounding box  the integer minimum of the leaf origins, and their maximum + 8; all 0 without a leaf (a tree of 64 bytes)
 * The field is read in place when it is on the device; a host field crosses once, through the scene's pinned memory, and nothing else
 * does: the block table is built on the device too.  The call accepts and refuses what hk_scene_update_medium would for that tree, with
 * the same status (the media classes against HK_NVDB_DENSE_MB, more than 2^27 blocks in the table, 4 GiB of tree), and also: a null
 * argument or field, a medium that is not NanoVDB, a res below 1 or a field of more than 2^27 blocks, an unknown layout, a non-finite
 * voxel (found on the device, for both kinds of source).  A refused call leaves the scene as it was.
 * The call WAITS FOR THE DEVICE ONCE, for one record: the node counts, the leaves' bounds and the non-finite flag, which size the tree and
 * the table and decide the class check.  Buffers are reused while the new tree fits and grow as in hk_scene_update_medium.  Like every
 * edit it renders the noted calls first and does not clear films. */
enum { HK_DENSE_X_FASTEST = 0,   /* Julia [nx,ny,nz], the layout of hk_medium::density */
       HK_DENSE_Z_FASTEST = 1 }; /* C [nx][ny][nz], a numpy / torch array as it is      */
typedef struct hk_dense_field {
    const float* data;
    int32_t res[3];      /* nx, ny, nz >= 1; may differ from the last update's */
    int32_t layout;
    int32_t on_device;   /* 0: host memory, borrowed for the call, staged through the scene's pinned memory.
                            1: memory of ctx's device, already visible to ctx's stream (the caller has ordered its
                               producer before the call); read by the build kernels, not kept after they ran */
} hk_dense_field;
int32_t hk_scene_update_medium_dense(hk_scene* scene, int32_t idx, const hk_medium* medium, const hk_dense_field* field);

/* hk_scene_update_envmap_sky: the texels of environment map `idx` become a Hosek-Wilkie sky (lights/sun_sky.jl:87-190, 319-434), evaluated
 * ON THE DEVICE from the record below, one thread per texel; the Distribution2D tables are then rebuilt from them exactly as
 * hk_scene_update_envmap rebuilds them.  Only the record crosses to the device (1224 bytes against 16 * res^2 of texels).  The caller
 * cooks the coefficients for its turbidity, albedo and solar elevation (hosek_cook_config / hosek_cook_radiance, a few hundred flops):
 * the library holds no dataset.  Like hk_scene_update_envmap with texels, the call renders the noted calls first, joins the lanes and
 * enqueues on the context's stream; it does not wait for the device, clears no film and leaves `rotation` alone.
 * Texel (v_idx, u_idx) (0-based; hk_envmap::data[v_idx + height * u_idx]) of a map of res x res.  binary32 where marked f32, binary64
 * elsewhere, nothing contracted, division and square root correctly rounded:
 *   direction  f32: c(k) = ((float)(k + 1) - 0.5f) / (float)res;  w = equal_area_square_to_sphere(c(u_idx), c(v_idx))
 *              (textures/environment_map.jl:131-160); cos and sin of phi are taken in double and rounded to binary32
 *   ground     ground_enabled != 0 and w.z <= 0 (+0 included): the texel is (ground_rgb, 1)
 *   angles     f32: cosg = clamp((w.x*d.x + w.y*d.y) + w.z*d.z, -1, 1), d = sun_dir;  theta = acos(clamp(w.z, 0, 1)) and
 *              gamma = acos(cosg) are binary32 values (acos taken in double and rounded), widened to double;
 *              cg = cos(gamma), ct = max(cos(theta), 0)
 *   band b     c = config[b]:  F[b] = (1 + c0*exp(c1 / (ct + 0.01))) * (c2 + c3*exp(c4*gamma) + c5*cg*cg
 *                                     + c6*(1 + cg*cg) / (1 + c8*c8 - 2*c8*cg)^1.5 + c7*sqrt(ct)),    x^1.5 taken as x * sqrt(x)
 *   lambda_k   = 320 + k*400/12 (k = 0 .. 12), x = (lambda_k - 320) / 40, low = floor(x), t = x - low:
 *              L[k] = F[low]*radiance[low] when t < 1e-6, otherwise
 *              L[k] = (1 - t)*(F[low]*radiance[low]) + (low + 1 < 11 ? t*F[low+1]*radiance[low+1] : 0)
 *   colour     XYZ[c] = sum over k ascending of L[k] * xyz_weight[c][k], rounded once to binary32; then in f32, left to right,
 *              r =  3.2404542f*X - 1.5371385f*Y - 0.4985314f*Z,  g = -0.9692660f*X + 1.8760108f*Y + 0.0415560f*Z,
 *              b =  0.0556434f*X - 0.2040259f*Y + 1.0572252f*Z;  texel = (max(0, r), max(0, g), max(0, b), 1)
 * A bake of the same record on another libm (NumPy on the host) differs in the last places: tests/golden/sky_bake_bounds.json records by
 * how much.  Refused, each with HK_ERR_INVALID and a message, nothing changed: a null scene or null params, idx out of range, a map that
 * is not square, a map whose tables are not of its texels' resolution, a non-finite entry anywhere in the record, a sun_dir whose squared
 * length is outside 1 +- 1e-3, reserved != 0.
 * hk_scene_envmap_copy reads back what the device holds of map `idx`: the sizes, the texels (4 floats per texel, layout of
 * hk_envmap::data) and the Distribution2D tables in the layouts of the hk_envmap record with nu = width and nv = height
 * (marginal_func_int: one float).  Any output pointer may be NULL.  It waits for the device.  Refused: a null scene, idx out of range,
 * a table pointer for a map whose tables are not of its texels' resolution (the caller sizes its buffers from width and height; the
 * sizes, the texels and marginal_func_int of such a map can still be read). */
typedef struct hk_sky_params {
    float   sun_dir[3];          /* unit vector TO the sun in the map's own frame (before `rotation`), z up */
    int32_t ground_enabled;
    float   ground_rgb[3];       /* the texel of every direction with z <= 0 when ground_enabled */
    int32_t reserved;            /* 0 */
    double  config[11][9];       /* cooked Hosek-Wilkie coefficients per band (hosek_cook_config) */
    double  radiance[11];        /* cooked band radiances (hosek_cook_radiance) */
    double  xyz_weight[3][13];   /* spectrum -> XYZ weights of the 13 wavelengths, / CIE_Y_INTEGRAL */
} hk_sky_params;
int32_t hk_scene_update_envmap_sky(hk_scene* scene, int32_t idx, const hk_sky_params* sky);
int32_t hk_scene_envmap_copy(hk_scene* scene, int32_t idx, int32_t* width, int32_t* height, float* texels /* 4 per texel in the layout of hk_envmap::data */,
                             float* conditional_func, float* conditional_cdf, float* marginal_func, float* marginal_cdf, float* marginal_func_int);

int32_t hk_integrator_create(hk_ctx* ctx, const hk_integrator_params* params, hk_integrator** out);
int32_t hk_integrator_destroy(hk_integrator* integ);

/* Film accumulators [pixel_rgb 3N | pixel_weight_sum N] (volpath-state.jl:122-131).  If
 * `external_accum` is non-NULL it is a device pointer to 4*N floats (or doubles when the integrator
 * accumulates in f64) owned by the caller — e.g. a torch tensor that torch.distributed reduces. */
int32_t hk_film_create(hk_ctx* ctx, int32_t width, int32_t height, int32_t f64, void* external_accum, hk_film** out);
int32_t hk_film_destroy(hk_film* film);
int32_t hk_film_clear(hk_film* film); /* clear!(vp), volpath.jl:108-113 */

/* Render samples first_sample_idx .. first_sample_idx+n_samples-1 (1-based like
 * film.iteration_index, volpath.jl:488-489) with stride `sample_stride` (1 on a single GPU; G when
 * G GPUs shard by sample index) on top of the current accumulators.
 *
 * ORDERING CONTRACT.  The call returns before the samples are rendered.
 *   - A call of more than 8 M paths (HK_PIPELINE_MAX_PATHS_M), a call on a context that was created on a CALLER'S stream, and a call
 *     into a film with EXTERNAL accumulators — or one whose accumulators hk_film_accum_device_ptr has handed out — are enqueued on ctx's stream before the call returns: whatever the caller orders behind
 *     that stream (events, a collective on the accumulators, torch.cuda.synchronize()) sees the samples.
 *   - A SMALL call (a one-sample `render!`, volpath.jl:445-450) on a context with the default stream and a library-owned film may only
 *     be NOTED: calls that continue each other (same scene / integrator / film / camera / pixel range / stride, sample indices
 *     following on) are rendered as ONE pass — bit-identical film, a seventh of the time — when the note reaches HK_BATCH_PATHS_M
 *     (64 M paths), when a call comes that does not continue it, or when anything looks: hk_flush, hk_sync, every hk_film_* / hk_stats_* /
 *     hk_*_destroy / hk_ctx_set_option /
 *     hk_scene_set_transform / hk_scene_set_vertices / hk_scene_update_materials / hk_scene_update_lights / hk_scene_update_envmap / hk_scene_update_medium / hk_scene_update_medium_dense / hk_scene_update_envmap_sky entry point.  hk_flush enqueues the noted calls without waiting for them.
 *     HK_BATCH_PATHS_M=0 (hk_ctx_set_option) turns the noting off.
 * Argument errors are reported by the call itself; a device error of a deferred pass by the call that flushes it — also by the
 * destroy entry points, which still destroy their object. */
int32_t hk_render(hk_ctx* ctx, hk_scene* scene, hk_integrator* integ, hk_film* film, const hk_camera* cam,
                  int32_t first_sample_idx, int32_t n_samples, int32_t sample_stride);

/* The same, restricted to the pixels [x0, x1) x [y0, y1) (0-based, py counted like the film rows of hk_film_read_rgb): the
 * pixel-tile sharding mode of SURVEY 8(e).  Paths are independent (volpath.jl:538-612 reads no other pixel) and ZSobol is a
 * pure function of (px, py, sample_idx, dim), so a pixel gets bit-identical accumulators whichever range it is rendered in;
 * pixels outside the range are left untouched, so the sum-reduce of zero-initialised films gathers disjoint tiles. */
int32_t hk_render_tile(hk_ctx* ctx, hk_scene* scene, hk_integrator* integ, hk_film* film, const hk_camera* cam,
                       int32_t first_sample_idx, int32_t n_samples, int32_t sample_stride, int32_t x0, int32_t y0, int32_t x1, int32_t y1);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU: units = (pixel, sample_idx) paths, no communication between paths; each device renders its share
 * (sample indices g+1, g+1+G, ... through `sample_stride`, or a pixel tile through hk_render_tile) of the same replicated scene,
 * and ONE exchange finishes the frame: ncclReduce(sum) of [pixel_rgb 3N | pixel_weight_sum N] (volpath.jl:364-373,
 * volpath-state.jl:122-131) onto the root over xGMI.  RCCL is loaded on first use.
 *   one process, several GPUs (the Julia shim's `devices = 0:7`): hk_ctx per device, hk_comm_create over them, hk_render on
 *     each, hk_film_reduce(comm, films, n, root), hk_film_read_rgb on films[root];
 *   one process per GPU (torchrun-style): rank 0 calls hk_comm_unique_id and hands the 128 bytes to the others (any side
 *     channel), every rank hk_comm_create_rank, then hk_film_reduce(comm, &film, 1, root).
 * The reduce is enqueued on each context's stream, after the renders already enqueued there, in place.
 * ------------------------------------------------------------------------------------------- */
typedef struct hk_comm hk_comm;
int32_t hk_comm_create(hk_ctx* const* ctxs, int32_t n, hk_comm** out);
int32_t hk_comm_unique_id(uint8_t* id_out128);
int32_t hk_comm_create_rank(hk_ctx* ctx, const uint8_t* id128, int32_t rank, int32_t world, hk_comm** out);
int32_t hk_comm_destroy(hk_comm* comm);
int32_t hk_film_reduce(hk_comm* comm, hk_film* const* films, int32_t n_films, int32_t root);

/* K13 finalize (volpath.jl:384-417): writes rgb/weight as Julia Matrix{RGB{Float32}}[height,width]
 * (`out_hw3` = 3 floats per pixel, column-major over (py,px)) into host memory; synchronises. */
int32_t hk_film_read_rgb(hk_ctx* ctx, hk_film* film, float* out_hw3);
/* The same frame without stopping the GPU for the copy — what an interactive viewer wants between two render! calls
 * (volpath.jl:617-633 writes the frame after EVERY sample):
 *   hk_film_read_rgb_async   enqueues K13 + the copy of the frame into PINNED host memory owned by the film (two buffers, used in
 *                            turn) behind everything rendered so far, and returns at once — the next hk_render may follow;
 *   hk_film_read_wait        waits for the LAST hk_film_read_rgb_async of the film only (not for renders enqueued after it), then
 *                            copies the frame to out_hw3 (may be NULL) and / or returns the pinned buffer itself in *frame (may be
 *                            NULL; valid until the second-next hk_film_read_rgb_async of this film).
 * hk_film_read_rgb itself goes through the same pinned buffers and a memcpy.  A viewer that reads every frame into ONE buffer can
 * spare the memcpy: hk_film_pin_host registers that buffer (3 * width * height floats) with the driver (hipHostRegister) and
 * hk_film_read_rgb copies straight into it whenever it is the destination; the caller keeps the buffer alive until hk_film_unpin_host
 * or hk_film_destroy.  The library never registers caller memory on its own (it cannot know when such a buffer is freed), unless
 * HK_READBACK_PIN=1 asks for round 5's behaviour: the same destination twice in a row is registered. */
int32_t hk_film_read_rgb_async(hk_ctx* ctx, hk_film* film);
int32_t hk_film_read_wait(hk_ctx* ctx, hk_film* film, float* out_hw3, const float** frame);
int32_t hk_film_pin_host(hk_film* film, float* host_hw3);
int32_t hk_film_unpin_host(hk_film* film);
/* raw accumulators (host copy): 4*N floats (or doubles). */
int32_t hk_film_read_accum(hk_ctx* ctx, hk_film* film, void* out);
/* the accumulators on the device.  Noted calls are enqueued first, and because the caller may KEEP the pointer (a reduce, an event of
 * its own behind ctx's stream), every later hk_render into this film is enqueued before it returns — as for external accumulators. */
void* hk_film_accum_device_ptr(hk_film* film);

/* hk_flush: every render call made so far is enqueued on ctx's stream (noted small calls are rendered now); does not wait.
 * hk_sync: hk_flush + waits until the stream is idle. */
int32_t hk_flush(hk_ctx* ctx);
int32_t hk_sync(hk_ctx* ctx);
int32_t hk_stats_get(hk_ctx* ctx, hk_stats* out);
int32_t hk_stats_reset(hk_ctx* ctx);
/* flags bit 0: count BVH nodes/triangles per cast during the next renders (adds two counters per lane; keep
 * off while timing); bit 1: bracket every kernel launch with HIP events on ctx's stream. */
int32_t hk_stats_enable_counters(hk_ctx* ctx, int32_t flags);

/* ---- sub-kernel entry points (parity tests drive these through the same ABI) ---- */
/* closest-hit of n rays (host arrays): t (inf = miss), prim (index into scene triangles, -1 = miss), bary u,v */
int32_t hk_trace_closest(hk_ctx* ctx, hk_scene* scene, int32_t n, const float* o3, const float* d3, const float* tmax,
                         float* out_t, int32_t* out_prim, float* out_uv2);
/* ZSobol draws on the device: for i<n: out[i] = sample_1d / sample_2d(px[i],py[i],sample_idx[i],dim[i]) */
int32_t hk_test_sobol(hk_ctx* ctx, int32_t width, int32_t height, int32_t spp, uint32_t seed, int32_t n,
                      const int32_t* px, const int32_t* py, const int32_t* sample_idx, const int32_t* dim,
                      float* out_1d, float* out_2d);
/* camera-sample stage (K1) for n (px,py,sample): lambda[4],pdf[4],filter weight, ray o,d  => 15 floats each */
int32_t hk_test_camera(hk_ctx* ctx, hk_integrator* integ, const hk_camera* cam, int32_t width, int32_t height, int32_t n,
                       const int32_t* px, const int32_t* py, const int32_t* sample_idx, float* out15);
/* uplift: mode 0 bounded, 1 unbounded, 2 illuminant; rgb[3n], lambda[4n] -> out[4n] */
int32_t hk_test_uplift(hk_ctx* ctx, int32_t mode, int32_t n, const float* rgb, const float* lambda, float* out);
/* light-BVH: sample (light_idx_1based, pmf) and pmf of a given light for n shading points */
int32_t hk_test_light_bvh(hk_ctx* ctx, hk_scene* scene, int32_t n, const float* p3, const float* n3, const float* u,
                          int32_t* out_light, float* out_pmf, const int32_t* query_light, float* out_query_pmf);
/* the host twin of hk_scene_refit_lights, no device involved: the tree built from lights[0 .. n_lights-1], then n_calls refits in turn
   (call k takes the next call_n[k] entries of index / records).  Out: the tree as hk_scene_light_bvh_copy hands it out, and the table
   the sampler walks (16 words per entry, 2 n_lights entries, device order).  HK_ERR_INVALID for an edit the entry point refuses. */
int32_t hk_test_light_refit_host(const hk_light* lights, int32_t n_lights, int32_t n_calls, const int32_t* call_n, const int32_t* index,
                                 const hk_light* records, int32_t* n_nodes, float* nodes_out, uint32_t* bit_trails, uint32_t* table_out);
/* that table as the device holds it now: 16 words per entry, 2 max(n_lights, 1) entries (waits for the context's stream) */
int32_t hk_test_light_table_copy(hk_scene* scene, uint32_t* table_out);
/* ---------------------------------------------------------------------------------------------
 * postprocess!(film; exposure, tonemap, gamma, white_point, sensor, background)  (src/postprocess.jl:293-357).
 * Non-destructive: reads the film's current rgb/weight, writes tonemapped RGB to `dst` (host, Julia [h,w] RGB{Float32}
 * layout like hk_film_read_rgb).  Parameters are the kernel arguments of postprocess_kernel! (:185-250): the host side
 * resolves symbols / sensor / white-balance matrix (compute_white_balance_matrix, spectral/color.jl:522-547).
 * depth: optional host float[h*w] (film.depth, Julia [h,w]); with mask_escaped != 0 pixels are blended towards `bg` by the
 * fraction of +Inf depths in their 3x3 neighbourhood.
 * ------------------------------------------------------------------------------------------- */
enum { HK_TONEMAP_NONE = 0, HK_TONEMAP_REINHARD = 1, HK_TONEMAP_REINHARD_EXT = 2, HK_TONEMAP_ACES = 3, HK_TONEMAP_UNCHARTED2 = 4, HK_TONEMAP_FILMIC = 5 };
typedef struct hk_postprocess_params {
    float exposure;
    int32_t tonemap;
    float inv_gamma;
    int32_t apply_gamma;
    float white_point;
    float imaging_ratio; /* sensor.exposure_time * sensor.iso / 100 */
    int32_t apply_wb;
    float wb[9];         /* row-major 3x3 Bradford matrix */
    int32_t mask_escaped;
    float bg[3];
} hk_postprocess_params;
int32_t hk_film_postprocess(hk_ctx* ctx, hk_film* film, const hk_postprocess_params* params, const float* depth, float* dst_rgb);
/* the same kernel on a caller-supplied framebuffer (host, Julia [h,w] RGB layout) */
int32_t hk_postprocess(hk_ctx* ctx, const hk_postprocess_params* params, int32_t width, int32_t height, const float* src_rgb,
                       const float* depth, float* dst_rgb);

/* ---------------------------------------------------------------------------------------------
 * denoise!(film; config) (src/denoise.jl:301-376): edge-avoiding a-trous wavelet filter.  compute_variance_kernel! (:236-286,
 * 3x3 luminance variance, in-bounds neighbours only) when use_variance, then `iterations` passes of atrous_denoise_kernel!
 * (:136-229; 5x5 B-spline taps at spacing 2^(i-1), clamped to the edge, weights = spatial * colour * normal * depth) ping-ponging
 * between the framebuffer and a scratch buffer.  All buffers are host arrays in Julia [h,w] layout (rgb / normal 3 floats per
 * pixel, depth 1).  dst_rgb receives film.postprocess.  The reference's even passes write INTO film.framebuffer, so after
 * denoise! with iterations >= 2 the framebuffer holds the output of the last even pass: src_after (optional) receives it.
 * ------------------------------------------------------------------------------------------- */
typedef struct hk_denoise_params {
    int32_t iterations;   /* DenoiseConfig defaults (denoise.jl:41-47): 5 */
    float sigma_color;    /* 4 */
    float sigma_normal;   /* 128 */
    float sigma_depth;    /* 1 */
    int32_t use_variance; /* true */
} hk_denoise_params;
int32_t hk_denoise(hk_ctx* ctx, const hk_denoise_params* params, int32_t width, int32_t height, const float* src_rgb, const float* normal,
                   const float* depth, float* dst_rgb, float* src_after);

/* fill_aux_buffers!(film, scene, camera; has_infinite_lights) (src/film.jl:410-483): one primary ray through every pixel
 * centre; albedo = (0.8,0.8,0.8) on a hit else 0, normal = geometric normal of the hit triangle (Raycore's si.core.n is not
 * available here: normalize((v1-v0) x (v2-v0)), un-flipped) else 0, depth = |hit - ray.o|, else +Inf (or 1e30 when the scene
 * has infinite lights).  Outputs are host arrays in Julia [h,w] layout: albedo/normal 3 floats per pixel, depth 1. */
int32_t hk_film_fill_aux(hk_ctx* ctx, hk_scene* scene, const hk_camera* cam, int32_t width, int32_t height, int32_t has_infinite_lights,
                         float* albedo, float* normal, float* depth);

/* ---------------------------------------------------------------------------------------------
 * The display chain on the device: what a viewer shows after every render! is the denoised, tone-mapped frame, and in the reference
 * fill_aux_buffers!, denoise! and postprocess! all work on the film's own device arrays.  These entry points do the same; like every
 * other film call they render the noted small calls first and work on ctx's stream.
 *
 * update_aux: fill_aux_buffers! kept on the device — the first-hit guides go into buffers the FILM owns (allocated on first use,
 *   reused afterwards).  Enqueued on ctx's stream, no wait.  Valid until the next call or the film's destruction; after a scene
 *   transform or a camera change the caller calls it again.
 * read_aux: host copies of what update_aux computed (any pointer may be NULL); Julia [h,w] layout as the fill_aux entry point above; synchronises.
 * present: K13 finalize -> [variance -> `iterations` a-trous passes] -> [postprocess] entirely on the device, then ONE copy of the
 *   result (Julia [h,w] RGB{Float32}) to the host.  dn == NULL: no denoise.  pp == NULL: linear output.  Non-destructive: the
 *   accumulators and the aux buffers are only read.  The arithmetic is that of the host chain (read_rgb -> denoise -> postprocess)
 *   bit for bit; with neither dn nor pp the frame is the one of the plain read.  The synchronous form synchronises; the _async form
 *   goes through the film's two pinned staging buffers exactly like the asynchronous read, and the same wait call collects it.
 *   Every scratch buffer belongs to the film and is sized once: a steady-state present allocates nothing.
 * HK_ERR_INVALID (nothing enqueued): a null ctx / film, a film of another context, out_hw3 == NULL in the synchronous form, dn != NULL
 *   or pp->mask_escaped != 0 on a film that never had update_aux, dn->iterations outside 0..30, an unknown tonemap, read_aux before
 *   update_aux.
 * ------------------------------------------------------------------------------------------- */
int32_t hk_film_update_aux(hk_ctx* ctx, hk_film* film, hk_scene* scene, const hk_camera* cam, int32_t has_infinite_lights);
int32_t hk_film_read_aux(hk_ctx* ctx, hk_film* film, float* albedo, float* normal, float* depth);
int32_t hk_film_present(hk_ctx* ctx, hk_film* film, const hk_denoise_params* dn, const hk_postprocess_params* pp, float* out_hw3);
int32_t hk_film_present_async(hk_ctx* ctx, hk_film* film, const hk_denoise_params* dn, const hk_postprocess_params* pp);

/* point-wise BSDFs of a scene's material `mat_idx` (material-dispatch.jl:23-53; spectral-eval.jl) at uv=(0,0):
   mode 0 = sample_bsdf_spectral(wo, ns, lambda, u, uc, regularize) -> out[10n] = wi3, f4, pdf, is_specular, eta_scale
   mode 1 = evaluate_bsdf_spectral(wo, wi, ns, lambda)              -> out[10n] = f4, pdf, 0...
   wo/wi/ns: 3n floats, lambda: 4n, u: 2n, uc: n. */
int32_t hk_test_bsdf(hk_ctx* ctx, hk_scene* scene, int32_t mode, int32_t mat_idx, int32_t regularize, int32_t n, const float* wo,
                     const float* wi, const float* ns, const float* lambda, const float* u, const float* uc, float* out);
/* point-wise lights (physical-wavefront/lights.jl:39-297, 408-467):
   mode 0 = sample_light_spectral(light_idx_1based, p, lambda, u = in3.xy) -> out[12n] = wi3, pdf, Li4, p_light3, is_delta
   mode 1 = escaped ray along in3 -> out[12n] = Le4 summed over every light, environment pdf, 0... */
int32_t hk_test_light(hk_ctx* ctx, hk_scene* scene, int32_t mode, int32_t light_idx_1based, int32_t n, const float* p3,
                      const float* in3, const float* lambda, float* out);

/* resolve_mix_material (mix-material.jl:96-127, 222-238) for n hit points (p, wo, uv): out_mat = the material index a
   MixMaterial `mat_idx` resolves to (nested mixes followed, textured amount looked up nearest-texel, Q28) */
int32_t hk_test_mix(hk_ctx* ctx, hk_scene* scene, int32_t mat_idx, int32_t n, const float* p3, const float* wo3, const float* uv2,
                    int32_t* out_mat);
/* point-wise media (volpath/media.jl, nanovdb.jl), medium `medium_idx` (0-based), lambda: 4n:
   mode 0 = sample_point at p = a3 (media.jl:1327-1370, 1527-1575; nanovdb.jl:400-469) -> out[13n] = sigma_a4, sigma_s4, Le4, g
   mode 1 = majorant iterator along ray (o = a3, d = b3, t_max) (media.jl:229-340, 625-729; nanovdb.jl:509-554)
            -> out[49n] = number of segments (<= 256), then (t_min, t_max, sigma_maj[lambda 1]) of the first 16 segments
   mode 2 = mode 1 walked the way the tracking kernels do — cells whose majorant is exactly 0 are fast-forwarded without fetching
            the grid — -> out[49n] = number of segments INCLUDING the skipped ones, then the first 16 segments that were not skipped */
int32_t hk_test_medium(hk_ctx* ctx, hk_scene* scene, int32_t mode, int32_t medium_idx, int32_t n, const float* a3, const float* b3,
                       const float* tmax, const float* lambda, float* out);
/* hk_trace_closest through the traversal of the surfaces-only render path (k_trace_lean / k_shadow: while-while rounds with
   per-lane refill and the 16- or 32-entry LDS stack the scene's BVH depth selects).  anyhit != 0: the shadow kernel's
   first-accepted-hit mode, out_prim >= 0 <=> occluded (t / uv then belong to the hit that stopped the ray). */
int32_t hk_test_trace_lean(hk_ctx* ctx, hk_scene* scene, int32_t anyhit, int32_t n, const float* o3, const float* d3, const float* tmax,
                           float* out_t, int32_t* out_prim, float* out_uv2);

/* introspection used by tests/bench */
int32_t hk_scene_bvh_info(hk_scene* scene, int32_t* n_nodes, int32_t* n_leaf_tris, int32_t* max_depth);
/* (after hk_scene_refit_lights: the refit tree, read back from the device — the call waits for the context's stream) */
int32_t hk_scene_light_bvh_copy(hk_scene* scene, int32_t* n_nodes, float* nodes_out /* 16 floats per node */,
                                uint32_t* bit_trails /* n_lights */);
/* The cost of the scene's BVH as the device holds it (cost_now) and as hk_scene_create built it (cost_created): the sum over the inner
   nodes and both children of A(child box) * w / A(root), A = 2(dx*dy + dx*dz + dy*dz) of the float boxes in double (an empty box: 0),
   w = 1 for an inner child and the triangle count for a leaf child, the root box the union of the root node's two child boxes.  Refits
   (hk_scene_set_transform, hk_scene_set_vertices) keep the topology, so cost_now / cost_created says how much more box area a ray meets
   than in a tree built for the geometry: the quantity to watch when deciding to create the scene anew.  cost_now is reduced on the
   device without atomics (the same tree gives the same bits) and waits for the context's stream; either pointer may be NULL.  Both are 0
   for a scene without inner nodes. */
int32_t hk_scene_bvh_cost(hk_scene* scene, double* cost_now, double* cost_created);
/* The float nodes as the device holds them: n_nodes inner nodes, breadth-first, node 0 the root; boxes = the two child boxes of every
   node (lo0[3] hi0[3] lo1[3] hi1[3]), refs = the two child references (>= 0: an inner node; < 0: ~ref = first leaf slot << 3 | count - 1).
   Waits for the context's stream.  Either array may be NULL. */
int32_t hk_scene_bvh_copy(hk_scene* scene, int32_t* n_nodes, float* boxes /* 12 per node: lo0 hi0 lo1 hi1 */, int32_t* refs /* 2 per node */);
/* The triangle index of every leaf slot, in the order of the leaf records (the slots the leaf references of hk_scene_bvh_copy count):
   *n = the number of slots (the scene's triangle count), prims (NULL: only *n) = n indices.  Waits for the context's stream. */
int32_t hk_scene_bvh_leaves(hk_scene* scene, int32_t* n, int32_t* prims);
/* Rebuilds the triangle BVH on the device from the world positions the device holds (under every hk_scene_set_transform and
   hk_scene_set_vertices in force): the tree hk_scene_create would build from those positions now — the same binned-SAH decision per
   node (one function for both builders), leaf size and bin count of the context's HK_BVH_LEAF / HK_BVH_BINS as of this call — so node
   count, depth, every child reference, the set of triangles of every leaf and every box are the fresh scene's.  (Exception: a node
   that takes the builder's median fallback — all centroids coincide, or the depth budget of 30 levels refuses the SAH split — is cut at
   count / 2 in both builders, but the device keeps the segment's order where the host selects by centroid: other triangles may land
   on either side, and the subtree below a node the depth budget cut may differ.)  The order of the triangles INSIDE a leaf is the device builder's.  Hits, and therefore
   films, do not depend on the tree.
   Like every edit the call renders the noted calls first, joins the lanes and enqueues on the context's stream; unlike the others it
   WAITS FOR THE DEVICE ONCE, for the node count, the depth and the level table of the new tree.  Geometry, transforms, materials,
   lights, media, films and the view cache stay as they are; cost_created of hk_scene_bvh_cost becomes the cost of the tree just built
   (the new baseline of the drift), and cost_now equals it.  The depth may cross 16 in either direction: the traversal kernels are chosen
   per render call from the depth the scene has then.  A scene whose root is a leaf (no inner node) is left as it is: HK_OK.
   HK_BVH_BUILD_SMALL (context option, default 1024): nodes of at most that many triangles are binned by one block in LDS, larger ones
   by many blocks through integer atomics; the tree does not depend on it.
   The tree is built into new buffers that replace the old ones at the end: a failing call leaves the scene as it was. */
int32_t hk_scene_rebuild_bvh(hk_scene* scene);

/* The majorant grid (n_cells floats, index x + rx*(y + ry*z)) and the zero-cell mask ((n_cells + 31) / 32 words, bit c of the mask = cell c)
   of medium `idx` as the device holds them; waits for the context's stream.  Either array may be NULL; n_cells = 0 for a homogeneous medium. */
int32_t hk_scene_medium_copy(hk_scene* scene, int32_t idx, int32_t* n_cells, float* majorant, uint32_t* zero_mask);
/* The tree of NanoVDB medium `idx` as the device holds it, whichever call put it there: *record_out (NULL: not wanted) = the record with
   its offsets, counts, inv_mat, vec and index bounding box, every pointer NULL; *n_bytes = the size of the tree; table_dims / table_min
   (3 each, or NULL) = extent and origin of the block table in blocks.  Call once for the sizes, then with `bytes` (*n_bytes of them)
   and / or `table` (2 words per block: leaf offset and value bits, block (bx, by, bz) at bz + dims[2]*(by + dims[1]*bx)); either may be
   NULL.  A call that copies waits for the context's stream. */
int32_t hk_scene_medium_tree_copy(hk_scene* scene, int32_t idx, hk_medium* record_out, int64_t* n_bytes, uint8_t* bytes, int32_t* table_dims, int32_t* table_min, uint32_t* table);
/* The halo bricks of NanoVDB medium `idx` as the device holds them: dims[3] = the block table's extent (all 0 when the medium has no
   bricks), out (NULL: only the extent) = dims[0]*dims[1]*dims[2] bricks of 729 floats, block (bx, by, bz) at bz + dims[2]*(by + dims[1]*bx). */
int32_t hk_test_medium_bricks(hk_scene* scene, int32_t idx, int32_t* dims, float* out);
/* The sizes the shading queue of material kind `kind` (HK_MAT_*) had at bounce `depth` in the integrator's last pass, one per wave
   segment of the path state: *n_segments = the number of segments, counts (NULL: only *n_segments) = that many entry counts — what
   one wave of k_shade walked in 64-entry chunks.  flagged (NULL: not wanted; needs counts): per segment, how many of those entries carry
   the emissive flag — read from the queue itself, which every bounce overwrites, so `depth` must be the bounce traced last (a pass of
   max_depth 1: depth 0).  kind -1: the rays of the generation at `depth` (hits and escaped together), kind -2: those of them that escaped
   (both without `flagged`).  Staged passes only (a pass rendered in one fused launch leaves no counts); waits for the context's stream. */
int32_t hk_test_queue_counts(hk_integrator* integrator, int32_t depth, int32_t kind, int32_t* n_segments, int32_t* counts, int32_t* flagged);
/* The per-triangle geometry table of the scene, (n.x, n.y, n.z, area) per triangle in original triangle order — what the shading
   kernels read in place of the three vertex positions (context option HK_TRI_GEO=0: they compute it from the positions at every
   vertex, the same bits).  *n_tris = the scene's triangle count; out4 (NULL: only the count) = 4 floats per triangle: recompute 0 the
   rows as the device holds them (from the packed shading records where the scene has them), recompute 1 the rows a kernel computes
   now from the world positions the device holds, by the function that fills the table.  *has_table (NULL: not wanted) = 0 for a scene
   without one (no triangles): recompute 0 is then an error.  Waits for the context's stream. */
int32_t hk_test_tri_geo(hk_scene* scene, int32_t recompute, int32_t* n_tris, int32_t* has_table, float* out4);

#ifdef __cplusplus
}
#endif
#endif /* HIKARI_MI355X_H */
