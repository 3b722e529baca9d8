"""The host side of k_trace_lean's flush choice (CPU): DScene::has_mix is hk::materials_have_kind and DScene::single_kind is
hk::single_material_kind (hk_edit_host.h) over the scene's material records, asked by hk_scene_create and again after every
hk_scene_update_materials.  A stand-alone program, built with the sanitizers, walks the records through create, an edit to a
MixMaterial and the edit back."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hikari.jl_amd", "csrc")

PROGRAM = r"""
#include "hikari_mi355x.h"
#include "hk_edit_host.h"
#include <cstdio>
#include <vector>
static unsigned mask_of(const std::vector<hk_material>& m) {   // hk_scene::kinds_mask as hk_scene_create computes it
    unsigned k = 0;
    for (const auto& r : m)
        if (r.kind != HK_MAT_MIX) k |= 1u << r.kind;
    return k;
}
static void report(const std::vector<hk_material>& m, unsigned created_mask) {
    const int mix = hk::materials_have_kind(m.data(), m.size(), HK_MAT_MIX);
    std::printf("%d %d\n", mix, hk::single_material_kind(created_mask, mix, 16));
}
int main() {
    std::vector<hk_material> m(3);
    for (auto& r : m) r = hk_material{};
    m[0].kind = m[1].kind = m[2].kind = HK_MAT_MATTE;
    const unsigned created = mask_of(m);
    report(m, created);                       // created: one kind
    hk_material mix = hk_material{};
    mix.kind = HK_MAT_MIX, mix.i[0] = 0, mix.i[1] = 1;
    const hk_material old = m[2];
    m[2] = mix;
    report(m, created);                       // edited to a Mix
    m[2] = old;
    report(m, created);                       // and back
    m[1].kind = HK_MAT_MIRROR;
    report(m, mask_of(m));                    // a scene of two kinds
    std::printf("%d %d %d\n", hk::materials_have_kind(m.data(), 0, HK_MAT_MIX), hk::single_material_kind(0u, 0, 16), hk::single_material_kind(1u << 20, 0, 16));
    return 0;
}
"""


def test_flush_flags_follow_the_records(tmp_path):
    src = tmp_path / "flags.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "flags"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    from hikari_jl_amd import _abi as A
    matte = str(A.HK_MAT_MATTE)
    assert out[:5] == ["0 " + matte, "1 -1", "0 " + matte, "0 -1", "0 -1 -1"]
