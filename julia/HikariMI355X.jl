# HikariMI355X.jl — the reference-side binding a Hikari.jl maintainer adds (INTEGRATION.md): a `Hikari.Integrator` subtype that
# flattens `Scene` / `Film` / `Camera` into the POD records of include/hikari_mi355x.h and `ccall`s libhikari_mi355x.so.
#
# STATUS: written against the reference sources under /root/reference (file:line cited at each step) and against the C header;
# it has NOT been executed — the build image has no Julia toolchain and Raycore.jl (the un-vendored BVH dependency, branch
# `sd/multitype-vec`, Project.toml:33-34) is absent.  What is checked here instead: tests/test_julia_shim.py parses the `struct Hk*`
# declarations below and compares every field offset and size with the C header (through the ctypes mirror, itself checked
# against `sizeof` from gcc), and checks that every `ccall` names an exported symbol with the right argument count.
# Raycore internals this file touches, all of them through names Hikari's own sources use:
#   accel.instances[i].transform / .inv_transform        src/surface_interaction.jl:418-423
#   accel.blas_array                                      src/scene.jl:196-197
#   blas.primitives (Raycore.BVH)                         src/scene.jl:201
#   Raycore.vertices / normals / uvs / tangents, triangle.metadata::TriangleMeta   src/surface_interaction.jl:331-353, src/scene.jl:11-15
#   Raycore.get_static(multitypeset), Raycore.deref(static, ::TextureRef), SetKey.type_idx / .vec_idx, Raycore.is_valid
# The ONE unknown is the name of the field that links a TLAS instance to its BLAS: `instance_blas` resolves it at run time from a
# short list and fails with an explicit message otherwise.
module HikariMI355X

using Hikari
import Hikari: Integrator, render!, clear!
using Raycore
using LinearAlgebra: normalize, transpose

const LIB = get(ENV, "HIKARI_MI355X_LIB", "libhikari_mi355x")
const Vec3f = Hikari.Vec3f

check(st::Int32, what) = st == 0 || error("$what failed ($st): " * unsafe_string(ccall((:hk_last_error, LIB), Cstring, ())))

# ---- POD mirrors of include/hikari_mi355x.h (field order and types must match; tests/test_julia_shim.py checks the layout) ----
struct HkTexture
    width::Int32; height::Int32; channels::Int32; kind::Int32
    data::Ptr{Float32}
end
struct HkTexRgba
    c::NTuple{4,Float32}; tex::Int32
end
struct HkTexF32
    v::Float32; tex::Int32
end
struct HkMaterial
    kind::Int32; flags::Int32
    rgb::NTuple{4,HkTexRgba}
    f::NTuple{8,HkTexF32}
    i::NTuple{4,Int32}
    spectrum::NTuple{2,Int32}
    mix_key::NTuple{4,UInt32}
end
struct HkPlSpectrum
    n::Int32; _pad::Int32
    lambdas::Ptr{Float32}; values::Ptr{Float32}
end
struct HkMediumInterface
    material::Int32; inside::Int32; outside::Int32
end
struct HkTriMeta
    medium_interface_idx::UInt32; primitive_index::UInt32; arealight_flat_idx_1based::UInt32
end
struct HkLight
    kind::Int32; spectrum_kind::Int32
    i_rgb::NTuple{4,Float32}
    poly::NTuple{3,Float32}
    illum_scale::Float32
    scale::Float32
    position::NTuple{3,Float32}
    direction::NTuple{3,Float32}
    world_to_light::NTuple{16,Float32}
    light_to_world::NTuple{16,Float32}
    cos_total_width::Float32; cos_falloff_start::Float32
    v::NTuple{9,Float32}
    normal::NTuple{3,Float32}
    area::Float32
    uv::NTuple{6,Float32}
    Le::HkTexRgba
    two_sided::Int32
    envmap::Int32
end
struct HkEnvmap
    width::Int32; height::Int32
    data::Ptr{Float32}
    rotation::NTuple{9,Float32}
    nu::Int32; nv::Int32
    conditional_func::Ptr{Float32}; conditional_cdf::Ptr{Float32}; conditional_func_int::Ptr{Float32}
    marginal_func::Ptr{Float32}; marginal_cdf::Ptr{Float32}
    marginal_func_int::Float32
    _pad::Int32
end
struct HkMedium
    kind::Int32
    sigma_a::NTuple{4,Float32}; sigma_s::NTuple{4,Float32}; Le::NTuple{4,Float32}
    g::Float32
    sigma_scale::Float32; Le_scale::Float32
    bounds_min::NTuple{3,Float32}; bounds_max::NTuple{3,Float32}
    render_to_medium::NTuple{16,Float32}; medium_to_render::NTuple{16,Float32}
    res::NTuple{3,Int32}
    density::Ptr{Float32}
    sigma_a_grid::Ptr{Float32}; sigma_s_grid::Ptr{Float32}; Le_grid::Ptr{Float32}
    majorant_res::NTuple{3,Int32}
    majorant::Ptr{Float32}
    max_density::Float32
    nvdb_bytes::Ptr{UInt8}
    nvdb_size::Int64
    root_offset_1based::Int64; upper_offset_1based::Int64; lower_offset_1based::Int64; leaf_offset_1based::Int64
    upper_count::Int32; lower_count::Int32; leaf_count::Int32; root_table_size::Int32
    inv_mat::NTuple{9,Float32}; vec::NTuple{3,Float32}
    index_bbox_min::NTuple{3,Int32}; index_bbox_max::NTuple{3,Int32}
end
struct HkSceneDesc
    n_triangles::Int32; n_materials::Int32; n_textures::Int32; n_media_interfaces::Int32
    n_lights::Int32; n_envmaps::Int32; n_media::Int32; n_spectra::Int32
    positions::Ptr{Float32}; normals::Ptr{Float32}; uvs::Ptr{Float32}; tangents::Ptr{Float32}
    meta::Ptr{HkTriMeta}
    materials::Ptr{HkMaterial}
    textures::Ptr{HkTexture}
    media_interfaces::Ptr{HkMediumInterface}
    lights::Ptr{HkLight}
    envmaps::Ptr{HkEnvmap}
    media::Ptr{HkMedium}
    spectra::Ptr{HkPlSpectrum}
end
struct HkTables
    sobol_matrices::Ptr{UInt32}; sobol_count::Int32; rgb2spec_res::Int32
    cie_x::Ptr{Float32}; cie_y::Ptr{Float32}; cie_z::Ptr{Float32}
    rgb2spec_scale::Ptr{Float32}; rgb2spec_coeffs::Ptr{Float32}
end
struct HkIntegratorParams
    max_depth::Int32; samples_per_pixel::Int32; russian_roulette_depth::Int32; regularize::Int32
    material_coherence::Int32; max_component_value::Float32; filter_type::Int32
    filter_radius::NTuple{2,Float32}; filter_param1::Float32; filter_param2::Float32
    accumulate_f64::Int32; sampler_seed::UInt32; samples_per_pass::Int32
end
struct HkCamera
    raster_to_camera::NTuple{16,Float32}; camera_to_world::NTuple{16,Float32}
    lens_radius::Float32; focal_distance::Float32; shutter_open::Float32; shutter_close::Float32
    dx_camera::NTuple{3,Float32}; dy_camera::NTuple{3,Float32}
end
struct HkPostprocessParams
    exposure::Float32; tonemap::Int32; inv_gamma::Float32; apply_gamma::Int32; white_point::Float32
    imaging_ratio::Float32; apply_wb::Int32; wb::NTuple{9,Float32}; mask_escaped::Int32; bg::NTuple{3,Float32}
end
struct HkDenoiseParams
    iterations::Int32; sigma_color::Float32; sigma_normal::Float32; sigma_depth::Float32; use_variance::Int32
end

# enum values of the header
const HK_MAT_MATTE, HK_MAT_MIRROR, HK_MAT_GLASS, HK_MAT_CONDUCTOR, HK_MAT_COATED_DIFFUSE, HK_MAT_THIN_DIELECTRIC = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4), Int32(5)
const HK_MAT_DIFFUSE_TRANSMISSION, HK_MAT_COATED_DIFFUSE_TRANSMISSION, HK_MAT_COATED_CONDUCTOR, HK_MAT_MIX, HK_MAT_FALLBACK = Int32(6), Int32(7), Int32(8), Int32(9), Int32(10)
const HK_MATF_REMAP_ROUGHNESS, HK_MATF_USE_ETA_K = Int32(1), Int32(2)
const HK_LIGHT_POINT, HK_LIGHT_SPOT, HK_LIGHT_DIRECTIONAL, HK_LIGHT_SUN, HK_LIGHT_AMBIENT, HK_LIGHT_ENVIRONMENT, HK_LIGHT_DIFFUSE_AREA = Int32(0), Int32(1), Int32(2), Int32(3), Int32(4), Int32(5), Int32(6)
const HK_SPEC_RGB, HK_SPEC_ILLUMINANT = Int32(0), Int32(1)
const HK_MEDIUM_HOMOGENEOUS, HK_MEDIUM_GRID, HK_MEDIUM_RGB_GRID, HK_MEDIUM_NANOVDB = Int32(0), Int32(1), Int32(2), Int32(3)

# ---------------------------------------------------------------------------------------------------------------------------
mutable struct DeviceState
    device::Int
    ctx::Ptr{Cvoid}; integ::Ptr{Cvoid}; film::Ptr{Cvoid}; scene::Ptr{Cvoid}
end

mutable struct MI355XVolPath <: Integrator
    params::HkIntegratorParams
    samples_per_pixel::Int32
    devs::Vector{DeviceState}
    comm::Ptr{Cvoid}
    scene_id::UInt
    film_size::Tuple{Int,Int}
    display::Symbol            # what `render!` does with film.framebuffer after its sample: :every, :pipelined, :manual (see MI355XVolPath)
    display_every::Int         # ... and every how many calls
    calls_since_display::Int
    read_pending::Bool         # an hk_film_read_rgb_async nobody has waited for yet
    pinned_fb::Any             # the framebuffer registered with hk_film_pin_host (held here so that it outlives the registration), or nothing
end

rowmajor(m) = ntuple(i -> Float32(m[(i - 1) ÷ 4 + 1, (i - 1) % 4 + 1]), 16)
rowmajor3(m) = ntuple(i -> Float32(m[(i - 1) ÷ 3 + 1, (i - 1) % 3 + 1]), 9)
tup3(v) = (Float32(v[1]), Float32(v[2]), Float32(v[3]))
rgba(s::Hikari.RGBSpectrum) = (s.c[1], s.c[2], s.c[3], s.c[4])

"""
    MI355XVolPath(; max_depth=8, samples=64, russian_roulette_depth=3, regularize=true, material_coherence=:none,
                  max_component_value=10f0, filter=GaussianFilter(), accumulation_eltype=Float32, devices=0:0)

Same keywords and defaults as `Hikari.VolPath` (volpath.jl:75-101) plus `devices`: the GPUs of this node that share a frame
(sample-index sharding + one RCCL reduce of the film inside the library, SURVEY 8e), and how `render!` — ONE sample per call, what
RayMakie's interactive loop drives (volpath.jl:445-450) — keeps `film.framebuffer` (host memory here; a device array in the reference):

  * `display = :every` (default), `display_every = k`: the frame is read back after every k-th call (`hk_film_read_rgb`: K13 + a copy into
    `film.framebuffer`, which the shim registers with `hk_film_pin_host` and keeps alive).  With k = 1 `film.framebuffer` is current after every call,
    exactly like the reference; calls that are not followed by a read-back are only NOTED by the library and rendered as one pass with the
    next read-back (bit-identical film, up to 7x less time per sample) — k = 4 … 16 is what a viewer at 60 Hz wants.
  * `display = :pipelined`: after call i `film.framebuffer` holds the frame of call i − 1; the copy of frame i is in flight while call
    i + 1 renders (`hk_film_read_rgb_async` / `hk_film_read_wait`), so the GPU never waits for the host.  `sync_display!(vp, film)` brings
    the last frame in.
  * `display = :manual`: `render!` never reads back; call `sync_display!(vp, film)` when a frame is wanted (an offline loop).
The functor `vp(scene, film, camera)` always returns with the finished frame in place.
"""
function MI355XVolPath(; max_depth::Int = 8, samples::Int = 64, russian_roulette_depth::Int = 3, regularize::Bool = true,
                       material_coherence::Symbol = :none, max_component_value::Real = 10f0,
                       filter = Hikari.GaussianFilter(), accumulation_eltype::DataType = Float32,
                       devices = 0:0, display::Symbol = :every, display_every::Int = 1)
    @assert display in (:every, :pipelined, :manual) && display_every >= 1
    @assert material_coherence in (:none, :sorted, :per_type)          # volpath.jl:85
    @assert accumulation_eltype in (Float32, Float64)                 # volpath.jl:86
    fp = Hikari.GPUFilterParams(filter)                                # filter.jl:574-604
    p = HkIntegratorParams(max_depth, samples, russian_roulette_depth, regularize, findfirst(==(material_coherence), (:none, :sorted, :per_type)) - 1,
                           Float32(max_component_value), fp.filter_type, (fp.radius[1], fp.radius[2]), fp.param1, fp.param2,
                           accumulation_eltype === Float64, UInt32(0), 0)
    devs = [DeviceState(Int(d), C_NULL, C_NULL, C_NULL, C_NULL) for d in devices]
    MI355XVolPath(p, samples, devs, C_NULL, UInt(0), (0, 0), display, display_every, 0, false, nothing)
end

function ensure_ctx!(vp::MI355XVolPath)
    vp.devs[1].ctx != C_NULL && return
    tab = Hikari.get_srgb_table()
    sob, cx, cy, cz = Hikari.SobolMatrices32, Hikari.CIE_X, Hikari.CIE_Y, Hikari.CIE_Z
    scale, coeffs = Vector{Float32}(tab.scale), Array{Float32}(tab.coeffs)
    for d in vp.devs
        r = Ref{Ptr{Cvoid}}()
        check(ccall((:hk_ctx_create, LIB), Int32, (Int32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), d.device, C_NULL, r), "hk_ctx_create")
        d.ctx = r[]
        GC.@preserve sob cx cy cz scale coeffs begin
            t = HkTables(pointer(sob), length(sob), tab.res, pointer(cx), pointer(cy), pointer(cz), pointer(scale), pointer(coeffs))
            check(ccall((:hk_ctx_set_tables, LIB), Int32, (Ptr{Cvoid}, Ref{HkTables}), d.ctx, t), "hk_ctx_set_tables")
        end
        ri = Ref{Ptr{Cvoid}}()
        check(ccall((:hk_integrator_create, LIB), Int32, (Ptr{Cvoid}, Ref{HkIntegratorParams}, Ref{Ptr{Cvoid}}), d.ctx, vp.params, ri), "hk_integrator_create")
        d.integ = ri[]
    end
    if length(vp.devs) > 1
        ctxs = [d.ctx for d in vp.devs]
        rc = Ref{Ptr{Cvoid}}()
        GC.@preserve ctxs check(ccall((:hk_comm_create, LIB), Int32, (Ptr{Ptr{Cvoid}}, Int32, Ref{Ptr{Cvoid}}), pointer(ctxs), length(ctxs), rc), "hk_comm_create")
        vp.comm = rc[]
    end
    nothing
end

# ---------------------------------------------------------------------------------------------------------------------------
# Scene flattening: Hikari.Scene -> hk_scene_desc (the record-by-record twin of hikari.jl_amd/scene.py::Scene.sync)
# ---------------------------------------------------------------------------------------------------------------------------
"The BLAS (Raycore.BVH over the instance's triangles) of a TLAS instance; the linking field is resolved from the names Raycore has used."
function instance_blas(accel, inst)
    for f in (:blas_index, :blas_idx, :blas_id, :geometry_index, :geometry_id, :blas)
        hasproperty(inst, f) || continue
        v = getproperty(inst, f)
        return v isa Integer ? accel.blas_array[v] : v
    end
    error("HikariMI355X: cannot find the BLAS of a TLAS instance (fields: $(propertynames(inst))); adapt `instance_blas` to this Raycore version")
end

"Transformation applied to a point: divide by w unless w == 1 (Raycore `Transformation(p::Point3f)`)."
function xform_point(m, p)
    x = m[1, 1] * p[1] + m[1, 2] * p[2] + m[1, 3] * p[3] + m[1, 4]
    y = m[2, 1] * p[1] + m[2, 2] * p[2] + m[2, 3] * p[3] + m[2, 4]
    z = m[3, 1] * p[1] + m[3, 2] * p[2] + m[3, 3] * p[3] + m[3, 4]
    w = m[4, 1] * p[1] + m[4, 2] * p[2] + m[4, 3] * p[3] + m[4, 4]
    w == 1f0 ? (Float32(x), Float32(y), Float32(z)) : (Float32(x / w), Float32(y / w), Float32(z / w))
end
"Normals go through the inverse transpose and are re-normalised (surface_interaction.jl:425-436); NaN (= absent) stays NaN."
function xform_normal(inv_m, n)
    any(isnan, n) && return (NaN32, NaN32, NaN32)
    v = Vec3f(inv_m[1, 1] * n[1] + inv_m[2, 1] * n[2] + inv_m[3, 1] * n[3],
              inv_m[1, 2] * n[1] + inv_m[2, 2] * n[2] + inv_m[3, 2] * n[3],
              inv_m[1, 3] * n[1] + inv_m[2, 3] * n[2] + inv_m[3, 3] * n[3])
    tup3(normalize(v))
end
function xform_dir(m, d)
    any(isnan, d) && return (NaN32, NaN32, NaN32)
    tup3(normalize(Vec3f(m[1, 1] * d[1] + m[1, 2] * d[2] + m[1, 3] * d[3], m[2, 1] * d[1] + m[2, 2] * d[2] + m[2, 3] * d[3], m[3, 1] * d[1] + m[3, 2] * d[2] + m[3, 3] * d[3])))
end

"Builder state: arrays handed to the library are collected in `keep` so that one GC.@preserve covers the hk_scene_create call."
mutable struct Flattener
    static_mats                     # StaticMultiTypeSet the TextureRefs being resolved point into (materials, then lights)
    textures::Vector{HkTexture}
    tex_ids::Dict{UInt,Int32}
    spectra::Vector{HkPlSpectrum}
    envmaps::Vector{HkEnvmap}
    keep::Vector{Any}
end

function texture_index!(fl::Flattener, data::AbstractArray, kind::Int32 = Int32(0))
    get!(fl.tex_ids, objectid(data)) do
        T = eltype(data)
        arr, ch = if T === Float32
            (Array{Float32}(data), Int32(1))
        elseif T === Hikari.RGBSpectrum
            (Array{Hikari.RGBSpectrum}(data), Int32(4))                # 4 floats per texel (spectrum.jl:38-43)
        else                                                           # RGB{Float32} and friends: promote to RGBSpectrum
            (map(c -> Hikari.RGBSpectrum(Float32(c.r), Float32(c.g), Float32(c.b), 1f0), data), Int32(4))
        end
        push!(fl.keep, arr)
        h, w = size(arr, 1), size(arr, 2)                              # Julia [height, width] column-major == the ABI's texture layout
        push!(fl.textures, HkTexture(w, h, ch, kind, Ptr{Float32}(pointer(arr))))
        Int32(length(fl.textures) - 1)
    end
end

"A material parameter: constant or texture (texture-ref.jl:50-84).  Returns (constant, texture index or -1)."
function resolve_tex(fl::Flattener, x)
    x isa Raycore.TextureRef && (x = Raycore.deref(fl.static_mats, x))
    x isa Hikari.Texture && (x = x.isconst ? x.constval : x.data)
    if x isa Hikari.VertexColorTexture                               # textures/basic.jl:42-46, texture-ref.jl:230-235
        fc = x.face_colors
        fc isa Raycore.TextureRef && (fc = Raycore.deref(fl.static_mats, fc))
        return (nothing, texture_index!(fl, fc, Int32(1)))
    end
    x isa AbstractArray && ndims(x) == 0 && (x = x[])
    x isa AbstractArray && return (nothing, texture_index!(fl, x))
    return (x, Int32(-1))
end
function tex_rgba(fl::Flattener, x)
    c, t = resolve_tex(fl, x)
    c === nothing && return HkTexRgba((0f0, 0f0, 0f0, 1f0), t)
    c isa Hikari.RGBSpectrum && return HkTexRgba(rgba(c), Int32(-1))
    c isa Real && return HkTexRgba((Float32(c), Float32(c), Float32(c), 1f0), Int32(-1))
    return HkTexRgba((Float32(c.r), Float32(c.g), Float32(c.b), 1f0), Int32(-1))      # RGB{Float32}
end
function tex_f32(fl::Flattener, x)
    c, t = resolve_tex(fl, x)
    c === nothing ? HkTexF32(0f0, t) : HkTexF32(Float32(c), Int32(-1))
end
const NO_RGBA = HkTexRgba((0f0, 0f0, 0f0, 1f0), Int32(-1))
const NO_F32 = HkTexF32(0f0, Int32(-1))
pad4(xs...) = ntuple(i -> i <= length(xs) ? xs[i] : NO_RGBA, 4)
pad8(xs...) = ntuple(i -> i <= length(xs) ? xs[i] : NO_F32, 8)
f32c(v) = HkTexF32(Float32(v), Int32(-1))

function spectrum_index!(fl::Flattener, s::Hikari.PiecewiseLinearSpectrum)
    lam, val = collect(Float32, s.lambdas), collect(Float32, s.values)
    push!(fl.keep, lam, val)
    push!(fl.spectra, HkPlSpectrum(length(lam), 0, pointer(lam), pointer(val)))
    Int32(length(fl.spectra) - 1)
end
"eta / k of the conductors: measured spectrum or colour (uber-material.jl:378-384)"
function ior_slot(fl::Flattener, x)
    x isa Hikari.PiecewiseLinearSpectrum ? (NO_RGBA, spectrum_index!(fl, x)) : (tex_rgba(fl, x), Int32(-1))
end

"One hk_material per scene material (Appendix A of SURVEY.md).  `flat` maps a SetKey to the flat 0-based material index."
function material_record(fl::Flattener, m, flat)
    z4, nosp, nokey = (Int32(0), Int32(0), Int32(0), Int32(0)), (Int32(-1), Int32(-1)), (UInt32(0), UInt32(0), UInt32(0), UInt32(0))
    remap(x) = x.remap_roughness ? HK_MATF_REMAP_ROUGHNESS : Int32(0)
    if m isa Hikari.MatteMaterial
        return HkMaterial(HK_MAT_MATTE, 0, pad4(tex_rgba(fl, m.Kd)), pad8(tex_f32(fl, m.σ)), z4, nosp, nokey)
    elseif m isa Hikari.MirrorMaterial
        return HkMaterial(HK_MAT_MIRROR, 0, pad4(tex_rgba(fl, m.Kr)), pad8(), z4, nosp, nokey)
    elseif m isa Hikari.GlassMaterial
        return HkMaterial(HK_MAT_GLASS, remap(m), pad4(tex_rgba(fl, m.Kr), tex_rgba(fl, m.Kt)), pad8(tex_f32(fl, m.index)), z4, nosp, nokey)
    elseif m isa Hikari.ConductorMaterial
        (e, se), (k, sk) = ior_slot(fl, m.eta), ior_slot(fl, m.k)
        return HkMaterial(HK_MAT_CONDUCTOR, remap(m), pad4(e, k), pad8(tex_f32(fl, m.roughness)), z4, (se, sk), nokey)
    elseif m isa Hikari.CoatedDiffuseMaterial
        return HkMaterial(HK_MAT_COATED_DIFFUSE, remap(m), pad4(tex_rgba(fl, m.reflectance), tex_rgba(fl, m.albedo)),
                          pad8(tex_f32(fl, m.u_roughness), tex_f32(fl, m.v_roughness), tex_f32(fl, m.thickness), f32c(m.eta), tex_f32(fl, m.g)),
                          (m.max_depth, m.n_samples, Int32(0), Int32(0)), nosp, nokey)
    elseif m isa Hikari.ThinDielectricMaterial
        return HkMaterial(HK_MAT_THIN_DIELECTRIC, 0, pad4(), pad8(f32c(m.eta)), z4, nosp, nokey)
    elseif m isa Hikari.DiffuseTransmissionMaterial
        return HkMaterial(HK_MAT_DIFFUSE_TRANSMISSION, 0, pad4(tex_rgba(fl, m.reflectance), tex_rgba(fl, m.transmittance)), pad8(f32c(m.scale)), z4, nosp, nokey)
    elseif m isa Hikari.CoatedDiffuseTransmissionMaterial
        return HkMaterial(HK_MAT_COATED_DIFFUSE_TRANSMISSION, remap(m), pad4(tex_rgba(fl, m.reflectance), tex_rgba(fl, m.transmittance), tex_rgba(fl, m.albedo)),
                          pad8(tex_f32(fl, m.u_roughness), tex_f32(fl, m.v_roughness), tex_f32(fl, m.thickness), f32c(m.eta), tex_f32(fl, m.g)),
                          (m.max_depth, m.n_samples, Int32(0), Int32(0)), nosp, nokey)
    elseif m isa Hikari.CoatedConductorMaterial
        (e, se), (k, sk) = ior_slot(fl, m.conductor_eta), ior_slot(fl, m.conductor_k)
        flags = remap(m) | (m.use_eta_k ? HK_MATF_USE_ETA_K : Int32(0))
        return HkMaterial(HK_MAT_COATED_CONDUCTOR, flags, pad4(e, k, tex_rgba(fl, m.reflectance), tex_rgba(fl, m.albedo)),
                          pad8(tex_f32(fl, m.interface_u_roughness), tex_f32(fl, m.interface_v_roughness), f32c(m.interface_eta),
                               tex_f32(fl, m.conductor_u_roughness), tex_f32(fl, m.conductor_v_roughness), tex_f32(fl, m.thickness), tex_f32(fl, m.g)),
                          (m.max_depth, m.n_samples, Int32(0), Int32(0)), (se, sk), nokey)
    elseif m isa Hikari.MixMaterial                                    # mix-material.jl: children by SetKey, hashed with their keys (:96-127)
        k1, k2 = m.material1_idx, m.material2_idx
        return HkMaterial(HK_MAT_MIX, 0, pad4(), pad8(tex_f32(fl, m.amount)), (flat(k1), flat(k2), Int32(0), Int32(0)), nosp,
                          (UInt32(k1.type_idx), UInt32(k1.vec_idx), UInt32(k2.type_idx), UInt32(k2.vec_idx)))
    end
    # any other Material (a bare Emissive, ...): no BSDF method => the gray 0.5 Lambertian fallback (quirk Q24)
    return HkMaterial(HK_MAT_FALLBACK, 0, pad4(), pad8(), z4, nosp, nokey)
end

"Light spectrum: RGBSpectrum (uplifted at run time) or a baked RGBIlluminantSpectrum (rgb2spec.jl:317-335)"
function spectrum_fields(i)
    if i isa Hikari.RGBIlluminantSpectrum
        return (HK_SPEC_ILLUMINANT, (0f0, 0f0, 0f0, 1f0), (i.poly.c0, i.poly.c1, i.poly.c2), i.scale)
    end
    return (HK_SPEC_RGB, rgba(i), (0f0, 0f0, 0f0), 0f0)
end
const Z3, Z6, Z9, Z16 = (0f0, 0f0, 0f0), ntuple(_ -> 0f0, 6), ntuple(_ -> 0f0, 9), ntuple(_ -> 0f0, 16)

function envmap_index!(fl::Flattener, em)
    D = em.distribution                                                # sampler/sampling.jl:179-262, stored verbatim
    data = Array{Hikari.RGBSpectrum}(em.data)                          # Matrix{RGBSpectrum}[h, w]
    cf, cc = Array{Float32}(D.conditional_func), Array{Float32}(D.conditional_cdf)
    cfi, mf, mc = Vector{Float32}(D.conditional_func_int), Vector{Float32}(D.marginal_func), Vector{Float32}(D.marginal_cdf)
    push!(fl.keep, data, cf, cc, cfi, mf, mc)
    h, w = size(data)
    push!(fl.envmaps, HkEnvmap(w, h, Ptr{Float32}(pointer(data)), rowmajor3(em.rotation), D.nu, D.nv, pointer(cf), pointer(cc), pointer(cfi), pointer(mf), pointer(mc),
                               D.marginal_func_int, 0))
    Int32(length(fl.envmaps) - 1)
end

function light_record(fl::Flattener, l)
    if l isa Hikari.DiffuseAreaLight                                   # lights/diffuse-area.jl:25-33, one per emissive face (scene-mesh.jl:98-131)
        v = l.vertices
        return HkLight(HK_LIGHT_DIFFUSE_AREA, HK_SPEC_RGB, (0f0, 0f0, 0f0, 1f0), Z3, 0f0, l.scale, Z3, Z3, Z16, Z16, 0f0, 0f0,
                       (v[1][1], v[1][2], v[1][3], v[2][1], v[2][2], v[2][3], v[3][1], v[3][2], v[3][3]), tup3(l.normal), l.area,
                       (l.uv[1][1], l.uv[1][2], l.uv[2][1], l.uv[2][2], l.uv[3][1], l.uv[3][2]), tex_rgba(fl, l.Le), l.two_sided, Int32(-1))
    elseif l isa Hikari.EnvironmentLight                               # lights/environment.jl:5-19: scale::RGBSpectrum rides in i_rgb
        return HkLight(HK_LIGHT_ENVIRONMENT, HK_SPEC_RGB, rgba(l.scale), Z3, 0f0, 1f0, Z3, Z3, Z16, Z16, 0f0, 0f0, Z9, Z3, 0f0, Z6, NO_RGBA, 0, envmap_index!(fl, l.env_map))
    end
    sk, irgb, poly, isc = spectrum_fields(l.i)
    if l isa Hikari.PointLight
        return HkLight(HK_LIGHT_POINT, sk, irgb, poly, isc, l.scale, tup3(l.position), Z3, Z16, Z16, 0f0, 0f0, Z9, Z3, 0f0, Z6, NO_RGBA, 0, Int32(-1))
    elseif l isa Hikari.SpotLight
        return HkLight(HK_LIGHT_SPOT, sk, irgb, poly, isc, l.scale, tup3(l.position), Z3, rowmajor(l.world_to_light.m), rowmajor(l.light_to_world.m),
                       l.cos_total_width, l.cos_falloff_start, Z9, Z3, 0f0, Z6, NO_RGBA, 0, Int32(-1))
    elseif l isa Hikari.SunLight
        return HkLight(HK_LIGHT_SUN, sk, irgb, poly, isc, l.scale, Z3, tup3(l.direction), Z16, Z16, 0f0, 0f0, Z9, Z3, 0f0, Z6, NO_RGBA, 0, Int32(-1))
    elseif l isa Hikari.DirectionalLight
        return HkLight(HK_LIGHT_DIRECTIONAL, sk, irgb, poly, isc, l.scale, Z3, tup3(l.direction), Z16, Z16, 0f0, 0f0, Z9, Z3, 0f0, Z6, NO_RGBA, 0, Int32(-1))
    elseif l isa Hikari.AmbientLight
        return HkLight(HK_LIGHT_AMBIENT, sk, irgb, poly, isc, l.scale, Z3, Z3, Z16, Z16, 0f0, 0f0, Z9, Z3, 0f0, Z6, NO_RGBA, 0, Int32(-1))
    end
    error("HikariMI355X: light type $(typeof(l)) is not part of the VolPath path")
end

i3(v) = (Int32(v[1]), Int32(v[2]), Int32(v[3]))
const I3Z = (Int32(0), Int32(0), Int32(0))
function grid_ptr!(fl::Flattener, g)
    g === nothing && return Ptr{Float32}(C_NULL)
    arr = Array(g)
    push!(fl.keep, arr)
    Ptr{Float32}(pointer(arr))
end
function medium_record(fl::Flattener, m)
    nul, nul8 = Ptr{Float32}(C_NULL), Ptr{UInt8}(C_NULL)
    z4 = (0f0, 0f0, 0f0, 1f0)
    if m isa Hikari.HomogeneousMedium                                  # volpath/media.jl:762-776
        return HkMedium(HK_MEDIUM_HOMOGENEOUS, rgba(m.σ_a), rgba(m.σ_s), rgba(m.Le), m.g, 1f0, 1f0, Z3, Z3, Z16, Z16, I3Z, nul, nul, nul, nul, I3Z, nul, 0f0,
                        nul8, 0, 0, 0, 0, 0, 0, 0, 0, 0, Z9, Z3, I3Z, I3Z)
    elseif m isa Hikari.GridMedium                                     # :873-935; density [nx,ny,nz] x fastest; majorant x + rx*(y + ry*z)
        mg = m.majorant_grid
        return HkMedium(HK_MEDIUM_GRID, rgba(m.σ_a), rgba(m.σ_s), z4, m.g, 1f0, 1f0, tup3(m.bounds.p_min), tup3(m.bounds.p_max), rowmajor(m.render_to_medium),
                        rowmajor(m.medium_to_render), i3(m.density_res), grid_ptr!(fl, m.density), nul, nul, nul, i3(mg.res), grid_ptr!(fl, mg.voxels), m.max_density,
                        nul8, 0, 0, 0, 0, 0, 0, 0, 0, 0, Z9, Z3, I3Z, I3Z)
    elseif m isa Hikari.RGBGridMedium                                  # :1002-1113; RGBSpectrum voxels = 4 floats each
        mg = m.majorant_grid
        return HkMedium(HK_MEDIUM_RGB_GRID, z4, z4, z4, m.g, m.sigma_scale, m.Le_scale, tup3(m.bounds.p_min), tup3(m.bounds.p_max), rowmajor(m.render_to_medium),
                        rowmajor(m.medium_to_render), i3(m.grid_res), nul, grid_ptr!(fl, m.σ_a_grid), grid_ptr!(fl, m.σ_s_grid), grid_ptr!(fl, m.Le_grid), i3(mg.res),
                        grid_ptr!(fl, mg.voxels), 0f0, nul8, 0, 0, 0, 0, 0, 0, 0, 0, 0, Z9, Z3, I3Z, I3Z)
    elseif m isa Hikari.NanoVDBMedium                                  # nanovdb.jl:153-191: the raw grid bytes and the reference's 1-based offsets
        mg = m.majorant_grid
        buf = Vector{UInt8}(m.buffer)
        push!(fl.keep, buf)
        return HkMedium(HK_MEDIUM_NANOVDB, rgba(m.σ_a), rgba(m.σ_s), z4, m.g, 1f0, 1f0, tup3(m.bounds.p_min), tup3(m.bounds.p_max), Z16, Z16, I3Z, nul, nul, nul, nul,
                        i3(mg.res), grid_ptr!(fl, mg.voxels), m.max_density, pointer(buf), length(buf), m.root_offset, m.upper_offset, m.lower_offset, m.leaf_offset,
                        m.upper_count, m.lower_count, m.leaf_count, m.root_table_size, m.inv_mat, m.vec, m.index_bbox_min, m.index_bbox_max)
    end
    error("HikariMI355X: medium type $(typeof(m)) is not part of the VolPath path")
end

"""
    flatten_scene(ctx, scene) -> hk_scene

World-space triangle soup + TriangleMeta from the TLAS, materials / media by MultiTypeSet slot, lights in the flat order of
`flat_to_light_index` (lights/light-sampler.jl:289-329), medium interfaces; then `hk_scene_create` (BVH + light BVH are built by
the library).  Arrays are borrowed for the call only.
"""
function flatten_scene(ctx::Ptr{Cvoid}, scene)
    fl = Flattener(Raycore.get_static(scene.materials), HkTexture[], Dict{UInt,Int32}(), HkPlSpectrum[], HkEnvmap[], Any[])
    # ---- materials / media: flat index = position in slot order; SetKey -> flat index ----
    mat_base, n = Int32[], Int32(0)
    for vec in scene.materials
        push!(mat_base, n); n += Int32(length(vec))
    end
    flat_mat(k) = Raycore.is_valid(k) ? mat_base[k.type_idx] + Int32(k.vec_idx) - Int32(1) : Int32(-1)
    materials = HkMaterial[]
    for vec in scene.materials, m in vec
        push!(materials, material_record(fl, m, flat_mat))
    end
    med_base, n = Int32[], Int32(0)
    for vec in scene.media
        push!(med_base, n); n += Int32(length(vec))
    end
    flat_med(k) = Raycore.is_valid(k) ? med_base[k.type_idx] + Int32(k.vec_idx) - Int32(1) : Int32(-1)
    media = HkMedium[]
    for vec in scene.media, m in vec
        push!(media, medium_record(fl, m))
    end
    mis = [HkMediumInterface(flat_mat(mi.material), flat_med(mi.inside), flat_med(mi.outside)) for mi in scene.media_interfaces]
    # ---- lights: type slots in order == the flat light index the TriangleMeta and the light sampler use ----
    lights = HkLight[]
    fl.static_mats = Raycore.get_static(scene.lights)                  # a textured DiffuseAreaLight.Le refers to the LIGHTS set's textures
    for vec in scene.lights, l in vec
        push!(lights, light_record(fl, l))
    end
    # ---- geometry: every TLAS instance's triangles, transformed to world space ----
    pos, nrm, uvs, tan, meta = Float32[], Float32[], Float32[], Float32[], HkTriMeta[]
    accel = scene.accel
    for inst in accel.instances
        blas = instance_blas(accel, inst)
        m, im = inst.transform, inst.inv_transform
        for tri in blas.primitives
            vs, ns, ts, uv = Raycore.vertices(tri), Raycore.normals(tri), Raycore.tangents(tri), Raycore.uvs(tri)
            for k in 1:3
                append!(pos, xform_point(m, vs[k]))
                append!(nrm, xform_normal(im, ns[k]))
                append!(tan, xform_dir(m, ts[k]))
                push!(uvs, Float32(uv[k][1]), Float32(uv[k][2]))
            end
            tm = tri.metadata::Hikari.TriangleMeta                     # scene.jl:11-15: interface index is 1-based on the Julia side
            push!(meta, HkTriMeta(tm.medium_interface_idx - UInt32(1), tm.primitive_index, tm.arealight_flat_idx))
        end
    end
    textures, spectra, envmaps = fl.textures, fl.spectra, fl.envmaps
    out = Ref{Ptr{Cvoid}}()
    keep = fl.keep
    GC.@preserve keep pos nrm uvs tan meta materials textures mis lights envmaps media spectra begin
        p(a) = isempty(a) ? Ptr{eltype(a)}(C_NULL) : pointer(a)
        desc = HkSceneDesc(length(meta), length(materials), length(textures), length(mis), length(lights), length(envmaps), length(media), length(spectra),
                           p(pos), p(nrm), p(uvs), p(tan), p(meta), p(materials), p(textures), p(mis), p(lights), p(envmaps), p(media), p(spectra))
        check(ccall((:hk_scene_create, LIB), Int32, (Ptr{Cvoid}, Ref{HkSceneDesc}, Ref{Ptr{Cvoid}}), ctx, desc, out), "hk_scene_create")
    end
    out[]
end

# ---------------------------------------------------------------------------------------------------------------------------
# Cameras: one record covers PerspectiveCamera (camera/perspective.jl:41-128) and MatrixCamera (camera/matrix.jl:13-115, no lens)
# ---------------------------------------------------------------------------------------------------------------------------
function camera_record(cam::Hikari.PerspectiveCamera)
    HkCamera(rowmajor(cam.core.raster_to_camera.m), rowmajor(cam.core.core.camera_to_world.m), cam.core.lens_radius, cam.core.focal_distance,
             cam.core.core.shutter_open, cam.core.core.shutter_close, tup3(cam.dx_camera), tup3(cam.dy_camera))
end
function camera_record(cam::Hikari.MatrixCamera)
    HkCamera(rowmajor(cam.raster_to_camera.m), rowmajor(cam.core.camera_to_world.m), 0f0, 1f6, cam.core.shutter_open, cam.core.shutter_close,
             tup3(cam.dx_camera), tup3(cam.dy_camera))
end

# ---------------------------------------------------------------------------------------------------------------------------
# render! / functor / clear! / close  (volpath.jl:445-670, 108-113; Hikari.jl:47)
# ---------------------------------------------------------------------------------------------------------------------------
function render_samples!(vp::MI355XVolPath, scene, film::Hikari.Film, camera, n::Int; display::Symbol = :every)
    ensure_ctx!(vp)
    h, w = size(film.framebuffer)
    G = length(vp.devs)
    if vp.devs[1].film == C_NULL || vp.film_size != (w, h)
        vp.pinned_fb = nothing                              # (hk_film_destroy unregisters)
        for d in vp.devs
            d.film != C_NULL && ccall((:hk_film_destroy, LIB), Int32, (Ptr{Cvoid},), d.film)
            r = Ref{Ptr{Cvoid}}()
            check(ccall((:hk_film_create, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), d.ctx, w, h, vp.params.accumulate_f64, C_NULL, r), "hk_film_create")
            d.film = r[]
            check(ccall((:hk_film_clear, LIB), Int32, (Ptr{Cvoid},), d.film), "hk_film_clear")
        end
        vp.film_size = (w, h)
    end
    if vp.devs[1].scene == C_NULL || vp.scene_id != objectid(scene)
        for d in vp.devs
            d.scene != C_NULL && ccall((:hk_scene_destroy, LIB), Int32, (Ptr{Cvoid},), d.scene)
            d.scene = flatten_scene(d.ctx, scene)                       # the scene is replicated on every device (SURVEY 8e)
        end
        vp.scene_id = objectid(scene)
    end
    first = film.iteration_index[] + Int32(1)
    cam = camera_record(camera)
    # sample-index sharding: device g renders first+g, first+g+G, ... ; every hk_render only enqueues work on its context's stream
    for (g, d) in enumerate(vp.devs)
        cnt = n >= g ? cld(n - (g - 1), G) : 0
        cnt == 0 && continue
        check(ccall((:hk_render, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{HkCamera}, Int32, Int32, Int32),
                    d.ctx, d.scene, d.integ, d.film, cam, first + Int32(g - 1), cnt, G), "hk_render")
    end
    film.iteration_index[] = first + Int32(n - 1)
    root = vp.devs[1]
    if G > 1
        # The film of a multi-device frame is the SUM of the per-device accumulators.  hk_film_reduce adds them on the root IN PLACE,
        # so the other devices restart from zero afterwards (their samples now live in the root's accumulators).
        films = [d.film for d in vp.devs]
        GC.@preserve films check(ccall((:hk_film_reduce, LIB), Int32, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Int32, Int32), vp.comm, pointer(films), G, 0), "hk_film_reduce")
        for d in vp.devs[2:end]
            check(ccall((:hk_sync, LIB), Int32, (Ptr{Cvoid},), d.ctx), "hk_sync")
            check(ccall((:hk_film_clear, LIB), Int32, (Ptr{Cvoid},), d.film), "hk_film_clear")
        end
    end
    fb = film.framebuffer                               # Matrix{RGB{Float32}}[h, w]: exactly hk_film_read_rgb's layout
    if display === :every
        vp.read_pending = false
        if vp.pinned_fb !== fb          # the viewer's one framebuffer: the frame is copied straight into it (a refusal only costs the memcpy)
            ok = GC.@preserve fb ccall((:hk_film_pin_host, LIB), Int32, (Ptr{Cvoid}, Ptr{Float32}), root.film, Ptr{Float32}(pointer(fb)))
            vp.pinned_fb = ok == 0 ? fb : nothing
        end
        GC.@preserve fb check(ccall((:hk_film_read_rgb, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}), root.ctx, root.film, Ptr{Float32}(pointer(fb))), "hk_film_read_rgb")
    elseif display === :pipelined
        # this call's samples go to the GPU now; the frame of the PREVIOUS call is collected while they render; then this call's copy is enqueued
        check(ccall((:hk_flush, LIB), Int32, (Ptr{Cvoid},), root.ctx), "hk_flush")
        if vp.read_pending
            GC.@preserve fb check(ccall((:hk_film_read_wait, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Ptr{Float32}}), root.ctx, root.film, Ptr{Float32}(pointer(fb)), C_NULL), "hk_film_read_wait")
        end
        check(ccall((:hk_film_read_rgb_async, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), root.ctx, root.film), "hk_film_read_rgb_async")
        vp.read_pending = true
    end                                                 # :skip — the call is only noted (hk_render's ordering contract); the next read-back renders it
    nothing
end

"film.framebuffer <- the frame of everything rendered so far (after `display = :pipelined` / `:manual` loops, or between displayed calls)"
function sync_display!(vp::MI355XVolPath, film::Hikari.Film)
    root = vp.devs[1]
    (root.ctx == C_NULL || root.film == C_NULL) && return nothing
    fb = film.framebuffer
    vp.read_pending = false
    vp.calls_since_display = 0
    GC.@preserve fb check(ccall((:hk_film_read_rgb, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}), root.ctx, root.film, Ptr{Float32}(pointer(fb))), "hk_film_read_rgb")
    nothing
end

function Hikari.render!(vp::MI355XVolPath, scene::Hikari.AbstractScene, film::Hikari.Film, camera::Hikari.Camera)
    vp.calls_since_display += 1
    due = vp.display !== :manual && vp.calls_since_display >= vp.display_every
    due && (vp.calls_since_display = 0)
    # multi-device frames reduce (and look) in every call: batching is a one-device matter
    render_samples!(vp, scene, film, camera, 1; display = !due && length(vp.devs) == 1 ? :skip : (vp.display === :pipelined && due ? :pipelined : :every))
end

function Hikari.clear!(vp::MI355XVolPath)
    for d in vp.devs
        d.film != C_NULL && check(ccall((:hk_film_clear, LIB), Int32, (Ptr{Cvoid},), d.film), "hk_film_clear")
    end
end

function (vp::MI355XVolPath)(scene::Hikari.AbstractScene, film::Hikari.Film, camera::Hikari.Camera)
    film.iteration_index[] = Int32(0)
    Hikari.clear!(vp)
    vp.calls_since_display = 0
    render_samples!(vp, scene, film, camera, Int(vp.samples_per_pixel))
    copyto!(film.postprocess, film.framebuffer)          # the functor returns film.postprocess (volpath.jl:669): linear HDR until postprocess! runs
    return film.postprocess
end

function Base.close(vp::MI355XVolPath)
    vp.read_pending = false
    vp.devs[1].film != C_NULL && vp.pinned_fb !== nothing && ccall((:hk_film_unpin_host, LIB), Int32, (Ptr{Cvoid},), vp.devs[1].film)
    vp.pinned_fb = nothing
    vp.comm != C_NULL && ccall((:hk_comm_destroy, LIB), Int32, (Ptr{Cvoid},), vp.comm)
    vp.comm = C_NULL
    for d in vp.devs
        d.film != C_NULL && ccall((:hk_film_destroy, LIB), Int32, (Ptr{Cvoid},), d.film)
        d.integ != C_NULL && ccall((:hk_integrator_destroy, LIB), Int32, (Ptr{Cvoid},), d.integ)
        d.scene != C_NULL && ccall((:hk_scene_destroy, LIB), Int32, (Ptr{Cvoid},), d.scene)
        d.ctx != C_NULL && ccall((:hk_ctx_destroy, LIB), Int32, (Ptr{Cvoid},), d.ctx)
        d.film = d.integ = d.scene = d.ctx = C_NULL
    end
    nothing
end

# ---------------------------------------------------------------------------------------------------------------------------
# Lights, environment maps and media in place (hk_scene_update_lights / hk_scene_update_envmap / hk_scene_update_medium): the scene on the device is edited, not rebuilt
# ---------------------------------------------------------------------------------------------------------------------------
"""
    update_light!(vp, flat_index, light; envmap_index = 0, tree = :rebuild)

Replaces light `flat_index` (0-based, in the `flat_to_light_index` order `flatten_scene` uploads) of the scene `vp` holds on its devices
by `light`, which must be of the same type.  `tree = :rebuild`: the library rebuilds the light BVH on the host (the scene a fresh upload
would give, bit for bit).  `tree = :refit`: the tree keeps its topology and is refit on the device (`refit_lights!`).  Films are not
cleared.  An `EnvironmentLight` keeps pointing at map `envmap_index` of the scene; a textured `Le` cannot be introduced by an update.
"""
function update_light!(vp::MI355XVolPath, flat_index::Integer, light; envmap_index::Integer = 0, tree::Symbol = :rebuild)
    tree in (:rebuild, :refit) || error("HikariMI355X: update_light!: tree must be :rebuild or :refit")
    if tree === :refit
        return refit_lights!(vp, [flat_index], [light]; envmap_index = envmap_index)
    end
    rec = edited_light_record(light, envmap_index)
    for d in vp.devs
        d.scene == C_NULL && continue
        check(ccall((:hk_scene_update_lights, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{HkLight}), d.scene, Int32(flat_index), Int32(1), rec), "hk_scene_update_lights")
    end
    nothing
end

# the record of a light that replaces one of the scene: no texture may come with it
function edited_light_record(light, envmap_index::Integer)
    fl = Flattener(nothing, HkTexture[], Dict{UInt,Int32}(), HkPlSpectrum[], HkEnvmap[], Any[])
    rec = if light isa Hikari.EnvironmentLight
        HkLight(HK_LIGHT_ENVIRONMENT, HK_SPEC_RGB, rgba(light.scale), Z3, 0f0, 1f0, Z3, Z3, Z16, Z16, 0f0, 0f0, Z9, Z3, 0f0, Z6, NO_RGBA, 0, Int32(envmap_index))
    else
        light_record(fl, light)
    end
    isempty(fl.textures) || error("HikariMI355X: update_light! cannot add a texture to the scene")
    rec
end

"""
    refit_lights!(vp, flat_indices, lights; envmap_index = 0)

New records for a set of lights (distinct 0-based flat indices, any order) in ONE `hk_scene_refit_lights` call per device: the light BVH
keeps its topology and is refit on the device — the nodes above the edited leaves are recomputed, everything else keeps its bits.  The
expected image is that of a rebuilt tree, the pmf is not; a light may not enter or leave the tree (a power going to or from zero): the
library refuses such an edit and `update_light!` with `tree = :rebuild` takes it.
"""
function refit_lights!(vp::MI355XVolPath, flat_indices, lights; envmap_index::Integer = 0)
    length(flat_indices) == length(lights) || error("HikariMI355X: refit_lights!: as many lights as indices")
    idx = Int32[Int32(i) for i in flat_indices]
    recs = HkLight[edited_light_record(l, envmap_index) for l in lights]
    isempty(idx) && return nothing
    for d in vp.devs
        d.scene == C_NULL && continue
        check(ccall((:hk_scene_refit_lights, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{HkLight}), d.scene, Int32(length(idx)), idx, recs), "hk_scene_refit_lights")
    end
    nothing
end

"""
    update_envmap!(vp, index; data = nothing, rotation = nothing)

New texels (`Matrix{RGBSpectrum}` of the map's size) and / or a new rotation (`Mat3f`) for environment map `index` (0-based) of the
scene on the devices; with texels the library builds the `Distribution2D` tables on the device.
"""
function update_envmap!(vp::MI355XVolPath, index::Integer; data = nothing, rotation = nothing)
    texels = data === nothing ? nothing : Array{Hikari.RGBSpectrum}(data)
    rot = rotation === nothing ? nothing : collect(rowmajor3(rotation))
    GC.@preserve texels rot begin
        pd = texels === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(texels))
        pr = rot === nothing ? Ptr{Float32}(C_NULL) : pointer(rot)
        for d in vp.devs
            d.scene == C_NULL && continue
            check(ccall((:hk_scene_update_envmap, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}), d.scene, Int32(index), pd, pr), "hk_scene_update_envmap")
        end
    end
    nothing
end

"""
    update_medium!(vp, index, medium)

Medium `index` (0-based, in the order `flatten_scene` uploads `scene.media`) of the scene on the devices becomes `medium`, an object of the
same type, voxel resolution and majorant resolution: a new density field, new coefficients, new bounds, a new NanoVDB tree of any size.
The library builds the majorant grid (and the NanoVDB bricks) on the device from the data; the `majorant_grid` of `medium` is not read.
"""
function update_medium!(vp::MI355XVolPath, index::Integer, medium)
    fl = Flattener(nothing, HkTexture[], Dict{UInt,Int32}(), HkPlSpectrum[], HkEnvmap[], Any[])
    rec = medium_record(fl, medium)
    GC.@preserve fl begin
        for d in vp.devs
            d.scene == C_NULL && continue
            check(ccall((:hk_scene_update_medium, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{HkMedium}), d.scene, Int32(index), rec), "hk_scene_update_medium")
        end
    end
    nothing
end

# hk_dense_field of the header (no Hk prefix: the mirrors named Hk* are those of the scene description)
struct DenseFieldRecord
    data::Ptr{Float32}
    res::NTuple{3,Int32}
    layout::Int32
    on_device::Int32
end
const HK_DENSE_X_FASTEST, HK_DENSE_Z_FASTEST = Int32(0), Int32(1)

"""
    update_medium_dense!(vp, index, data; bounds, sigma_a, sigma_s, g = 0f0)

NanoVDB medium `index` (0-based) of the scene on the devices becomes the tree of the dense field `data` (`Array{Float32,3}`, `[nx, ny, nz]`,
handed over as it is: `HK_DENSE_X_FASTEST`), placed in `bounds`.  The library builds the tree, its block table, the majorant grid and
the bricks on the device — what `update_medium!` with `NanoVDBMedium(data; bounds, ...)` leaves there, without the host tree build.
The majorant resolution cannot change in place: it is read from the record the device scene keeps.
"""
function update_medium_dense!(vp::MI355XVolPath, index::Integer, data::AbstractArray{<:Real,3}; bounds, sigma_a, sigma_s, g = 0f0)
    field = Array{Float32,3}(data)
    nul, nul8 = Ptr{Float32}(C_NULL), Ptr{UInt8}(C_NULL)
    record(mres) = HkMedium(HK_MEDIUM_NANOVDB, rgba(sigma_a), rgba(sigma_s), (0f0, 0f0, 0f0, 1f0), Float32(g), 1f0, 1f0, tup3(bounds.p_min), tup3(bounds.p_max), Z16, Z16, I3Z, nul, nul, nul, nul,
                            mres, nul, 0f0, nul8, 0, 0, 0, 0, 0, 0, 0, 0, 0, Z9, Z3, I3Z, I3Z)
    GC.@preserve field begin
        dense = DenseFieldRecord(pointer(field), i3(size(field)), HK_DENSE_X_FASTEST, Int32(0))
        for d in vp.devs
            d.scene == C_NULL && continue
            kept, n = Ref(record(I3Z)), Ref{Int64}(0)               # the medium as the device scene holds it: its majorant_res
            check(ccall((:hk_scene_medium_tree_copy, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{HkMedium}, Ref{Int64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt32}), d.scene, Int32(index), kept, n,
                        Ptr{UInt8}(C_NULL), Ptr{Int32}(C_NULL), Ptr{Int32}(C_NULL), Ptr{UInt32}(C_NULL)), "hk_scene_medium_tree_copy")
            check(ccall((:hk_scene_update_medium_dense, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{HkMedium}, Ref{DenseFieldRecord}), d.scene, Int32(index), record(kept[].majorant_res), dense),
                  "hk_scene_update_medium_dense")
        end
    end
    nothing
end

"""
    medium_tree(vp, index) -> (bytes, table, table_dims, table_min)

The NanoVDB tree of medium `index` as the first device holds it (whichever update put it there) and its block table
(`2 x dims[3] x dims[2] x dims[1]` words: leaf offset and value bits per block, z fastest).
"""
function medium_tree(vp::MI355XVolPath, index::Integer)
    d = first(vp.devs)
    n = Ref{Int64}(0)
    dims, tmin = zeros(Int32, 3), zeros(Int32, 3)
    check(ccall((:hk_scene_medium_tree_copy, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ref{Int64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt32}), d.scene, Int32(index), C_NULL, n,
                Ptr{UInt8}(C_NULL), dims, tmin, Ptr{UInt32}(C_NULL)), "hk_scene_medium_tree_copy")
    bytes = zeros(UInt8, n[])
    table = zeros(UInt32, 2, dims[3], dims[2], dims[1])
    check(ccall((:hk_scene_medium_tree_copy, LIB), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ref{Int64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{UInt32}), d.scene, Int32(index), C_NULL, n,
                bytes, dims, tmin, table), "hk_scene_medium_tree_copy")
    bytes, table, dims, tmin
end

# hk_sky_params of the header (C arrays are row-major: config[b][j] is entry 9b + j + 1, xyz_weight[c][k] entry 13c + k + 1)
struct SkyParamsRecord
    sun_dir::NTuple{3,Float32}
    ground_enabled::Int32
    ground_rgb::NTuple{3,Float32}
    reserved::Int32
    config::NTuple{99,Float64}
    radiance::NTuple{11,Float64}
    xyz_weight::NTuple{39,Float64}
end

"""
    update_sky!(vp, index; direction, turbidity = 2.5f0, ground_albedo = Hikari.RGBSpectrum(0.3f0), ground_enabled = true)

The texels of environment map `index` (0-based) of the scene on the devices become the Hosek-Wilkie sky `Hikari.sunsky_to_envlight` bakes
for the same arguments (`direction` points TO the sun), evaluated on the device: only the cooked coefficients of `Hikari.HosekState`, the
sun direction, the ground texel and the spectrum -> XYZ weights cross (1224 bytes), and the library builds the `Distribution2D` tables
from the texels it wrote.  The map must be square; its rotation stays.  The device's texels agree with the host bake within the bound
recorded in tests/golden/sky_bake_bounds.json, not to the bit.
"""
function update_sky!(vp::MI355XVolPath, index::Integer; direction, turbidity = 2.5f0, ground_albedo = Hikari.RGBSpectrum(0.3f0), ground_enabled::Bool = true)
    dir = Hikari.normalize(Hikari.Vec3f(direction...))
    state = Hikari.HosekState(Float64(Float32(turbidity)), 0.5, Float64(asin(clamp(dir[3], 0f0, 1f0))))
    lambdas = [320.0 + i * (720.0 - 320.0) / 12 for i in 0:12]
    unit(k) = [j == k ? 1.0 : 0.0 for j in 1:13]
    weights = [Hikari._spectrum_to_xyz(lambdas, unit(k)) for k in 1:13]          # linear in the values: the weight of each wavelength
    ground = ground_albedo * 0.3f0
    rec = SkyParamsRecord(tup3(dir), Int32(ground_enabled), (ground.c[1], ground.c[2], ground.c[3]), Int32(0),
                          ntuple(i -> state.configs[(i - 1) ÷ 9 + 1][(i - 1) % 9 + 1], 99), state.radiances,
                          ntuple(i -> weights[(i - 1) % 13 + 1][(i - 1) ÷ 13 + 1], 39))
    for d in vp.devs
        d.scene == C_NULL && continue
        check(ccall((:hk_scene_update_envmap_sky, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{SkyParamsRecord}), d.scene, Int32(index), rec), "hk_scene_update_envmap_sky")
    end
    nothing
end

"""
    envmap_copy(vp, index) -> (texels, conditional_func, conditional_cdf, marginal_func, marginal_cdf, marginal_func_int)

Environment map `index` as the first device holds it (whichever update put it there): the texels as a `4 x height x width` `Float32`
array (r, g, b, a of `data[y, x]`) and the `Distribution2D` tables in the reference's layouts.  Waits for the device.
"""
function envmap_copy(vp::MI355XVolPath, index::Integer)
    d = first(vp.devs)
    w, h = Ref{Int32}(0), Ref{Int32}(0)
    nul = Ptr{Float32}(C_NULL)
    check(ccall((:hk_scene_envmap_copy, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), d.scene,
                Int32(index), w, h, nul, nul, nul, nul, nul, nul), "hk_scene_envmap_copy")
    nu, nv = Int(w[]), Int(h[])                                                   # the library refuses the table pointers below unless nu == width and nv == height
    texels = zeros(Float32, 4, nv, nu)
    cf, cc, mf, mc, mfi = zeros(Float32, nu, nv), zeros(Float32, nu + 1, nv), zeros(Float32, nv), zeros(Float32, nv + 1), zeros(Float32, 1)
    check(ccall((:hk_scene_envmap_copy, LIB), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}, Ref{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), d.scene,
                Int32(index), w, h, texels, cf, cc, mf, mc, mfi), "hk_scene_envmap_copy")
    texels, cf, cc, mf, mc, mfi[1]
end

"""
    set_vertices!(vp, first_tri, positions; normals = nothing, uvs = nothing)

New base geometry for triangles `first_tri` (0-based, in the order `flatten_scene` uploads them) onwards of the scene on the devices:
`positions` is a `3 x 3 x n` `Float32` array (coordinate, vertex, triangle — 9 floats per triangle in memory), `normals` likewise and `uvs`
`2 x 3 x n`, or `nothing` to keep what the triangles have.  The transform of the range is kept and the BVH is refit on the device; the
triangle count cannot change.  `bvh_cost` says when the refit tree has become slow.
"""
function set_vertices!(vp::MI355XVolPath, first_tri::Integer, positions; normals = nothing, uvs = nothing)
    P = Array{Float32}(positions)
    N = normals === nothing ? nothing : Array{Float32}(normals)
    U = uvs === nothing ? nothing : Array{Float32}(uvs)
    length(P) % 9 == 0 || error("HikariMI355X: set_vertices! takes 9 floats per triangle")
    n = length(P) ÷ 9
    (N === nothing || length(N) == 9n) && (U === nothing || length(U) == 6n) || error("HikariMI355X: set_vertices!: normals / uvs do not match the positions")
    GC.@preserve P N U begin
        pn = N === nothing ? Ptr{Float32}(C_NULL) : pointer(N)
        pu = U === nothing ? Ptr{Float32}(C_NULL) : pointer(U)
        for d in vp.devs
            d.scene == C_NULL && continue
            check(ccall((:hk_scene_set_vertices, LIB), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), d.scene, Int32(first_tri), Int32(n),
                        pointer(P), pn, Ptr{Float32}(C_NULL), pu), "hk_scene_set_vertices")
        end
    end
    nothing
end

"""
    bvh_cost(vp) -> (now, created)

The cost of the scene's BVH on the first device as it stands after refits, and as it was built; `now / created` is the quantity to watch
when deciding whether to flatten and create the scene anew.
"""
function bvh_cost(vp::MI355XVolPath)
    now = Ref{Float64}(0.0)
    created = Ref{Float64}(0.0)
    for d in vp.devs
        d.scene == C_NULL && continue
        check(ccall((:hk_scene_bvh_cost, LIB), Int32, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), d.scene, now, created), "hk_scene_bvh_cost")
        break
    end
    (now[], created[])
end

"""
    rebuild_bvh!(vp)

Rebuilds the triangle BVH of every device scene from the world positions the device holds (under every `set_transform!` /
`set_vertices!` in force): the tree a freshly created scene would get.  Everything else of the scene stays; `bvh_cost` afterwards
reports the new tree as its baseline.  The one edit that waits for the device (once, for the size of the new tree).
"""
function rebuild_bvh!(vp::MI355XVolPath)
    for d in vp.devs
        d.scene == C_NULL && continue
        check(ccall((:hk_scene_rebuild_bvh, LIB), Int32, (Ptr{Cvoid},), d.scene), "hk_scene_rebuild_bvh")
    end
    nothing
end

"""
    bvh_leaves(vp) -> Vector{Int32}

The 0-based triangle index of every leaf slot of the scene's BVH on the first device, in the order of the leaf records.
"""
function bvh_leaves(vp::MI355XVolPath)
    prims = Int32[]
    for d in vp.devs
        d.scene == C_NULL && continue
        n = Ref{Int32}(0)
        check(ccall((:hk_scene_bvh_leaves, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}), d.scene, n, Ptr{Int32}(C_NULL)), "hk_scene_bvh_leaves")
        prims = Vector{Int32}(undef, n[])
        GC.@preserve prims begin
            check(ccall((:hk_scene_bvh_leaves, LIB), Int32, (Ptr{Cvoid}, Ref{Int32}, Ptr{Int32}), d.scene, n, pointer(prims)), "hk_scene_bvh_leaves")
        end
        break
    end
    prims
end

# ---------------------------------------------------------------------------------------------------------------------------
# postprocess! / denoise! / fill_aux_buffers! forwards (postprocess.jl:293-357, denoise.jl:301-376, film.jl:410-483)
# ---------------------------------------------------------------------------------------------------------------------------
const TONEMAPS = Dict(nothing => Int32(0), :none => Int32(0), :reinhard => Int32(1), :reinhard_extended => Int32(2), :aces => Int32(3), :uncharted2 => Int32(4), :filmic => Int32(5))

"""
    postprocess!(vp, film; exposure=1f0, tonemap=:aces, gamma=2.2f0, white_point=4f0, sensor=nothing, background=nothing)

The keyword set of `Hikari.postprocess!`; symbols / `FilmSensor` / the Bradford matrix are resolved here into the kernel arguments
of `postprocess_kernel!` (postprocess.jl:185-250) and `hk_postprocess` runs it on `film.framebuffer` into `film.postprocess`.
"""
function postprocess!(vp::MI355XVolPath, film::Hikari.Film; exposure::Real = 1f0, tonemap = :aces, gamma = 2.2f0, white_point::Real = 4f0,
                      sensor = nothing, background = nothing)
    ensure_ctx!(vp)
    h, w = size(film.framebuffer)
    ratio, apply_wb, wb = 1f0, Int32(0), ntuple(i -> i in (1, 5, 9) ? 1f0 : 0f0, 9)
    if sensor !== nothing
        ratio = Float32(sensor.exposure_time * sensor.iso / 100f0)
        if sensor.white_balance > 0
            apply_wb, wb = Int32(1), rowmajor3(Hikari.compute_white_balance_matrix(Float32(sensor.white_balance)))   # spectral/color.jl:522-547
        end
    end
    mask, bg = background === nothing ? (Int32(0), Z3) : (Int32(1), (Float32(background.r), Float32(background.g), Float32(background.b)))
    P = HkPostprocessParams(Float32(exposure), TONEMAPS[tonemap], gamma === nothing ? 1f0 : 1f0 / Float32(gamma), gamma === nothing ? 0 : 1, Float32(white_point),
                            ratio, apply_wb, wb, mask, bg)
    src, dst, depth = film.framebuffer, film.postprocess, film.depth
    GC.@preserve src dst depth check(ccall((:hk_postprocess, LIB), Int32, (Ptr{Cvoid}, Ref{HkPostprocessParams}, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                           vp.devs[1].ctx, P, w, h, Ptr{Float32}(pointer(src)), mask == 1 ? pointer(depth) : Ptr{Float32}(C_NULL), Ptr{Float32}(pointer(dst))),
                                     "hk_postprocess")
    film.postprocess
end

"denoise!(film; config) (denoise.jl:301-376): à-trous passes guided by film.normal / film.depth; even passes write into film.framebuffer like the reference."
function denoise!(vp::MI355XVolPath, film::Hikari.Film; config = Hikari.DenoiseConfig())
    ensure_ctx!(vp)
    h, w = size(film.framebuffer)
    P = HkDenoiseParams(config.iterations, config.sigma_color, config.sigma_normal, config.sigma_depth, config.use_variance)
    src, nrm, dep, dst = film.framebuffer, film.normal, film.depth, film.postprocess
    GC.@preserve src nrm dep dst check(ccall((:hk_denoise, LIB), Int32,
                                             (Ptr{Cvoid}, Ref{HkDenoiseParams}, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                             vp.devs[1].ctx, P, w, h, Ptr{Float32}(pointer(src)), Ptr{Float32}(pointer(nrm)), pointer(dep), Ptr{Float32}(pointer(dst)),
                                             Ptr{Float32}(pointer(src))), "hk_denoise")
    film.postprocess
end

"fill_aux_buffers!(film, scene, camera; has_infinite_lights) (film.jl:410-483): first-hit albedo / normal / depth per pixel centre."
function fill_aux_buffers!(vp::MI355XVolPath, film::Hikari.Film, scene, camera; has_infinite_lights::Bool = false)
    ensure_ctx!(vp)
    d = vp.devs[1]
    if d.scene == C_NULL || vp.scene_id != objectid(scene)
        d.scene != C_NULL && ccall((:hk_scene_destroy, LIB), Int32, (Ptr{Cvoid},), d.scene)
        d.scene = flatten_scene(d.ctx, scene)
        vp.scene_id = length(vp.devs) == 1 ? objectid(scene) : UInt(0)
    end
    h, w = size(film.framebuffer)
    cam = camera_record(camera)
    alb, nrm, dep = film.albedo, film.normal, film.depth
    GC.@preserve alb nrm dep check(ccall((:hk_film_fill_aux, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{HkCamera}, Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                         d.ctx, d.scene, cam, w, h, has_infinite_lights, Ptr{Float32}(pointer(alb)), Ptr{Float32}(pointer(nrm)), pointer(dep)), "hk_film_fill_aux")
    nothing
end

"the kernel arguments of `postprocess_kernel!` for the keyword set of `Hikari.postprocess!` (what `postprocess!` above builds inline), for `present!`"
function postprocess_record(; exposure::Real = 1f0, tonemap = :aces, gamma = 2.2f0, white_point::Real = 4f0, sensor = nothing, background = nothing)
    ratio, apply_wb, wb = 1f0, Int32(0), ntuple(i -> i in (1, 5, 9) ? 1f0 : 0f0, 9)
    if sensor !== nothing
        ratio = Float32(sensor.exposure_time * sensor.iso / 100f0)
        if sensor.white_balance > 0
            apply_wb, wb = Int32(1), rowmajor3(Hikari.compute_white_balance_matrix(Float32(sensor.white_balance)))   # spectral/color.jl:522-547
        end
    end
    mask, bg = background === nothing ? (Int32(0), Z3) : (Int32(1), (Float32(background.r), Float32(background.g), Float32(background.b)))
    HkPostprocessParams(Float32(exposure), TONEMAPS[tonemap], gamma === nothing ? 1f0 : 1f0 / Float32(gamma), gamma === nothing ? 0 : 1, Float32(white_point),
                        ratio, apply_wb, wb, mask, bg)
end

"""
    update_aux!(vp, film, scene, camera; has_infinite_lights=false)

`fill_aux_buffers!` kept on the device: the guides of `present!` go into buffers the library's film owns (`hk_film_update_aux`).
Call it after the first `render!` (the film exists from then on) and again after a scene transform or a camera change.
`host_copy = true` also fills `film.albedo` / `film.normal` / `film.depth`.
"""
function update_aux!(vp::MI355XVolPath, film::Hikari.Film, scene, camera; has_infinite_lights::Bool = false, host_copy::Bool = false)
    ensure_ctx!(vp)
    d = vp.devs[1]
    d.film == C_NULL && error("update_aux!: render! into this film first")
    if d.scene == C_NULL || vp.scene_id != objectid(scene)
        d.scene != C_NULL && ccall((:hk_scene_destroy, LIB), Int32, (Ptr{Cvoid},), d.scene)
        d.scene = flatten_scene(d.ctx, scene)
        vp.scene_id = length(vp.devs) == 1 ? objectid(scene) : UInt(0)
    end
    cam = camera_record(camera)
    check(ccall((:hk_film_update_aux, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{HkCamera}, Int32), d.ctx, d.film, d.scene, cam, has_infinite_lights), "hk_film_update_aux")
    if host_copy
        alb, nrm, dep = film.albedo, film.normal, film.depth
        GC.@preserve alb nrm dep check(ccall((:hk_film_read_aux, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                             d.ctx, d.film, Ptr{Float32}(pointer(alb)), Ptr{Float32}(pointer(nrm)), pointer(dep)), "hk_film_read_aux")
    end
    nothing
end

"""
    present!(vp, film; denoise=nothing, pipelined=false, kwargs...)

The frame a viewer shows: K13 -> [denoise] -> [postprocess] on the device and one copy into `film.postprocess` (`hk_film_present`).
`denoise`: `nothing`, `true` (`Hikari.DenoiseConfig()`) or a `DenoiseConfig` — needs `update_aux!` first.  `kwargs` are those of
`postprocess!`; none = linear output.  `pipelined = true` enqueues this frame and delivers the one of the previous pipelined call.
"""
function present!(vp::MI355XVolPath, film::Hikari.Film; denoise = nothing, pipelined::Bool = false, kwargs...)
    d = vp.devs[1]
    (d.ctx == C_NULL || d.film == C_NULL) && error("present!: render! into this film first")
    config = denoise === true ? Hikari.DenoiseConfig() : (denoise === false ? nothing : denoise)
    dn = config === nothing ? Ptr{HkDenoiseParams}(C_NULL) :
         Ref(HkDenoiseParams(config.iterations, config.sigma_color, config.sigma_normal, config.sigma_depth, config.use_variance))
    pp = isempty(kwargs) ? Ptr{HkPostprocessParams}(C_NULL) : Ref(postprocess_record(; kwargs...))
    dst = film.postprocess
    if pipelined
        check(ccall((:hk_flush, LIB), Int32, (Ptr{Cvoid},), d.ctx), "hk_flush")
        if vp.read_pending
            GC.@preserve dst check(ccall((:hk_film_read_wait, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Ptr{Float32}}), d.ctx, d.film, Ptr{Float32}(pointer(dst)), C_NULL), "hk_film_read_wait")
        end
        check(ccall((:hk_film_present_async, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{HkDenoiseParams}, Ptr{HkPostprocessParams}), d.ctx, d.film, dn, pp), "hk_film_present_async")
        vp.read_pending = true
    else
        vp.read_pending = false
        GC.@preserve dst check(ccall((:hk_film_present, LIB), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{HkDenoiseParams}, Ptr{HkPostprocessParams}, Ptr{Float32}),
                                     d.ctx, d.film, dn, pp, Ptr{Float32}(pointer(dst))), "hk_film_present")
    end
    film.postprocess
end

end # module
