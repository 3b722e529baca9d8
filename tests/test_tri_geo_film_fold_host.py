"""The host side of the geometry table and of k_film's grouped fold (CPU).  The header declares hk_test_tri_geo and the ctypes table
has its prototype; HK_TRI_GEO and HK_FILM_FOLD are on the list of record, read where the launches are chosen, and documented; the
table's place behind the positions (hk::tri_geo_word, hk::positions_floats) and the fold's choice per launch (hk::film_fold_launch)
are plain C++ (hk_edit_host.h): a stand-alone program, built with the sanitizers, prints their tables."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hikari.jl_amd", "csrc")

PROGRAM = r"""
#include "hk_edit_host.h"
#include <cstdio>
int main() {
    // no triangles; 1, 3, 4, 5 triangles without packed records: the first multiple of 4 floats at or behind 9 T; packed: the word is 1
    const int T[] = {0, 1, 3, 4, 5, 3782, 32767};
    for (int t : T) std::printf("%d %d %zu %zu\n", hk::tri_geo_word(t, false), hk::tri_geo_word(t, true), hk::positions_floats(t, hk::tri_geo_word(t, false), false),
                                hk::positions_floats(t, hk::tri_geo_word(t, true), true));
    // the last triangle count whose offset an int holds, and the first that gets no table (its positions alone are allocated)
    std::printf("%d %d %zu\n", hk::tri_geo_word(238609293, false), hk::tri_geo_word(238609294, false), hk::positions_floats(238609294, 0, false));
    // knob, samples per pass
    const int S[] = {1, 32, 48, 63, 64, 65, 96, 128, 192, 256};
    for (int s : S) std::printf("%d%d ", hk::film_fold_launch(true, s), hk::film_fold_launch(false, s));
    std::printf("\n");
    return 0;
}
"""


def test_table_placement_and_fold_choice(tmp_path):
    src = tmp_path / "geo.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "geo"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = []
    for t in (0, 1, 3, 4, 5, 3782, 32767):
        off = (9 * t + 3) // 4 * 4
        assert off % 4 == 0 and 9 * t <= off < 9 * t + 4
        want.append("%d %d %d %d" % (off if t else 0, 1 if t else 0, off + 4 * t if t else 0, 9 * t))
    assert out[:7] == want
    last = (2 ** 31 - 1 - 3) // 9      # 9 T + 3 <= 2^31 - 1
    assert last == 238609293
    assert out[7] == "%d 0 %d" % ((9 * last + 3) // 4 * 4, 9 * (last + 1))
    assert out[8].split() == ["00", "00", "00", "00", "10", "00", "00", "10", "10", "10"]


def test_header_stubs_and_knobs(hk):
    hdr = open(os.path.join(ROOT, "include", "hikari_mi355x.h")).read()
    assert re.search(r"int32_t hk_test_tri_geo\(hk_scene\* scene, int32_t recompute, int32_t\* n_tris, int32_t\* has_table, float\* out4\);", hdr)
    assert "hk_test_tri_geo" in hk._abi.EXPORTED_SYMBOLS
    lib_py = open(os.path.join(ROOT, "hikari.jl_amd", "_lib.py")).read()
    assert re.search(r'"hk_test_tri_geo": \(\[vp, i32, PI, PI, PF\], i32\)', lib_py)
    ctx = open(os.path.join(CSRC, "hk_ctx.cpp")).read()
    listed = re.search(r"KNOB_NAMES\[\]\s*=\s*\{(.*?)\};", ctx, re.S).group(1)
    launch = re.sub(r"//.*", "", open(os.path.join(CSRC, "hk_launch_impl.h")).read())
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("HK_TRI_GEO", "HK_FILM_FOLD"):
        assert '"%s"' % name in listed
        assert name in doc
    # read per launch: launch_shade picks the lean kernel's GEO instantiation, launch_film asks film_fold_launch
    assert re.search(r'static bool tri_geo_on\(const DScene& sc\) \{ return sc\.tri_geo != 0 && knob_on\("HK_TRI_GEO"\); \}', launch)
    assert re.search(r"with_bool\(tri_geo_on\(sc\), \[&\]\(auto GEO\)", launch)
    assert re.search(r'film_fold_launch\(knob_on\("HK_FILM_FOLD"\), fr\.samples_in_pass\)', launch)
    # the struct kept its size: the word was padding (the argument layout of every kernel is the parent's)
    types = open(os.path.join(CSRC, "hk_types.h")).read()
    assert "pad_nodes" not in types and re.search(r"int n_nodes;[^\n]*\n(\s*//[^\n]*\n)*\s*int tri_geo;\s*\n\s*const float\* positions;", types)
