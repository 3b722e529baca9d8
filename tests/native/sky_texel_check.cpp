// sky_texel_check — hk_sky.h on the host, alone: every texel of a sky record read from a file, written as the device would hold them.
// Built by tests/test_sky_edit_host.py with g++ -ffp-contract=off, plain and under -fsanitize=address,undefined; no GPU, no Python.
//   sky_texel_check IN OUT      IN: int32 res, int32 0, then one hk_sky_params;  OUT: res * res texels of 4 floats, (v, u) at [v + res * u]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hk_sky.h"

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s params.bin texels.bin\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) {
        std::perror(argv[1]);
        return 2;
    }
    int32_t head[2] = {0, 0};
    SkyConsts S;
    const bool ok = std::fread(head, sizeof head, 1, in) == 1 && std::fread(&S, sizeof S, 1, in) == 1;
    std::fclose(in);
    const int res = head[0];
    if (!ok || res < 1 || res > 4096) {
        std::fprintf(stderr, "%s: not a parameter file\n", argv[1]);
        return 2;
    }
    std::vector<float> out((size_t)res * res * 4);
    for (int u = 0; u < res; ++u)
        for (int v = 0; v < res; ++v) {
            const SkyTexel t = hk_sky_texel(S, v, u, res);
            float* o = &out[4 * ((size_t)v + (size_t)res * u)];
            o[0] = t.r, o[1] = t.g, o[2] = t.b, o[3] = t.a;
        }
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) {
        std::perror(argv[2]);
        return 2;
    }
    std::fclose(f);
    std::printf("{\"res\": %d, \"bytes_in\": %zu}\n", res, sizeof S);
    return 0;
}
