// Host-only check of hikari.jl_amd/csrc/hk_edit_host.h: the parts of hk_scene_set_vertices and hk_scene_bvh_cost that run without a device
// (built by tests/test_vertex_edits_host.py with g++, once more with -fsanitize=address,undefined).
//  * stage_positions + merge_block_boxes, driven the way hk_scene_set_vertices drives them: a "scene" keeps its positions and one box
//    per `block` triangles; a random sequence of ranges — inside one block, across block boundaries, whole scene, last partial block —
//    gets new positions.  After every edit each box CONTAINS the true bounds of its block, a block the range covered whole HAS them
//    exactly, blocks outside the range are untouched, and the staged copy equals the input.  A range with a non-finite position is
//    refused before anything is folded in.
//  * tree_cost against a long double evaluation of the header's formula over random trees, with empty child boxes, leaf counts 1 .. 8,
//    a one-node tree and no tree.
// usage: vertex_edit_check <sequences> <seed>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "hk_edit_host.h"

static unsigned rng_state;
static unsigned urand() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}
static float frand() { return (float)urand() * (1.0f / 16777216.0f); }
#define CHECK(c)                                                                           \
    if (!(c)) {                                                                            \
        std::printf("FAILED %s (line %d, sequence %d, edit %d)\n", #c, __LINE__, seq, edit); \
        return 1;                                                                          \
    }

static void true_box(const std::vector<float>& pos, int begin, int end, float bb[6]) {
    for (int k = 0; k < 3; ++k) bb[k] = INFINITY, bb[3 + k] = -INFINITY;
    for (int t = begin; t < end; ++t)
        for (int v = 0; v < 9; ++v) {
            const float x = pos[9 * (size_t)t + v];
            bb[v % 3] = std::min(bb[v % 3], x);
            bb[3 + v % 3] = std::max(bb[3 + v % 3], x);
        }
}

static long double area_ref(const float* lo, const float* hi) {
    for (int k = 0; k < 3; ++k)
        if (!(lo[k] <= hi[k])) return 0.0L;
    const long double dx = (long double)hi[0] - lo[0], dy = (long double)hi[1] - lo[1], dz = (long double)hi[2] - lo[2];
    return 2.0L * (dx * dy + dx * dz + dy * dz);
}

int main(int argc, char** argv) {
    const int sequences = argc > 1 ? std::atoi(argv[1]) : 200;
    rng_state = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u;
    long edits_done = 0, refused = 0, trees = 0;
    static const int blocks[4] = {1, 7, 64, 1024};
    for (int seq = 0; seq < sequences; ++seq) {
        int edit = -1;
        const int block = blocks[urand() % 4];
        const int T = seq < 4 ? seq + 1 : 1 + (int)(urand() % (5 * block + 3));
        const int nb = (T + block - 1) / block;
        std::vector<float> pos(9 * (size_t)T);
        for (float& x : pos) x = 4.0f * frand() - 2.0f;
        std::vector<float> box(6 * (size_t)nb);   // as hk_scene_create notes them
        for (int b = 0; b < nb; ++b) true_box(pos, b * block, std::min(T, (b + 1) * block), &box[6 * (size_t)b]);
        const int n_edits = 1 + (int)(urand() % 8);
        for (edit = 0; edit < n_edits; ++edit) {
            int first = (int)(urand() % T), n = 1 + (int)(urand() % (T - first));
            const int mode = (int)(urand() % 5);   // 0: any range, 1: the whole scene, 2: one triangle, 3: from a block boundary, 4: to the end
            if (mode == 1) first = 0, n = T;
            if (mode == 2) n = 1;
            if (mode == 3) first = first / block * block, n = std::min(n, T - first);
            if (mode == 4) n = T - first;
            const float scale = (urand() & 3) == 0 ? 40.0f : 1.0f;   // some edits leave the old bounds, some shrink inside them
            std::vector<float> in(9 * (size_t)n), staged(9 * (size_t)n), fresh;
            for (float& x : in) x = scale * (frand() - 0.5f);
            const bool poison = (urand() & 7) == 0;
            if (poison) in[urand() % in.size()] = (urand() & 1) ? std::numeric_limits<float>::quiet_NaN() : -INFINITY;
            const std::vector<float> before = box;
            const bool ok = hk::stage_positions(in.data(), first, n, staged.data(), block, fresh);
            CHECK(ok == !poison);
            if (!ok) {   // refused: the caller returns before merge_block_boxes
                CHECK(box == before);
                ++refused;
                continue;
            }
            CHECK(staged == in);
            CHECK(fresh.size() == 6 * (size_t)((first + n - 1) / block - first / block + 1));
            hk::merge_block_boxes(box, T, first, n, block, fresh);
            for (size_t i = 0; i < in.size(); ++i) pos[9 * (size_t)first + i] = in[i];
            for (int b = 0; b < nb; ++b) {
                const int begin = b * block, end = std::min(T, begin + block);
                float tb[6];
                true_box(pos, begin, end, tb);
                const float* bb = &box[6 * (size_t)b];
                const bool touched = first < end && first + n > begin, whole = first <= begin && first + n >= end;
                for (int k = 0; k < 3; ++k) {
                    CHECK(bb[k] <= tb[k] && bb[3 + k] >= tb[3 + k]);
                    if (whole) CHECK(bb[k] == tb[k] && bb[3 + k] == tb[3 + k]);
                    if (!touched) CHECK(bb[k] == before[6 * (size_t)b + k] && bb[3 + k] == before[6 * (size_t)b + 3 + k]);
                }
            }
            ++edits_done;
        }
        {   // no boxes kept (a scene without quantised nodes): block 0 copies and checks only, merge does nothing
            std::vector<float> in(9, 1.0f), staged(9), fresh(3, 5.0f), none;
            CHECK(hk::stage_positions(in.data(), 0, 1, staged.data(), 0, fresh) && fresh.empty() && staged == in);
            hk::merge_block_boxes(none, T, 0, 1, block, fresh);
            CHECK(none.empty());
        }
        // ---- tree cost ----
        const size_t nn = seq < 3 ? (size_t)seq : 1 + urand() % 300;
        std::vector<float> boxes(12 * nn);
        std::vector<int> refs(2 * nn);
        for (size_t i = 0; i < nn; ++i)
            for (int c = 0; c < 2; ++c) {
                float* b = &boxes[12 * i + 6 * c];
                for (int k = 0; k < 3; ++k) {
                    b[k] = 10.0f * frand() - 5.0f;
                    b[3 + k] = b[k] + ((urand() & 15) == 0 ? 0.0f : 3.0f * frand());
                }
                if ((urand() & 15) == 0)   // an empty box
                    for (int k = 0; k < 3; ++k) b[k] = INFINITY, b[3 + k] = -INFINITY;
                const bool leaf = (urand() & 1) != 0 || nn == 1;
                refs[2 * i + c] = leaf ? ~(int)(((urand() % 1000) << 3) | (urand() & 7)) : (int)(urand() % nn);
            }
        const double got = hk::tree_cost(boxes.data(), refs.data(), nn);
        long double sum = 0.0L, root = 0.0L;
        for (size_t i = 0; i < nn; ++i) {
            for (int c = 0; c < 2; ++c) {
                const int r = refs[2 * i + c];
                sum += area_ref(&boxes[12 * i + 6 * c], &boxes[12 * i + 6 * c + 3]) * (r >= 0 ? 1.0L : (long double)(((~r) & 7) + 1));
            }
            if (i == 0) {
                float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (int c = 0; c < 2; ++c) {
                    const float* b = &boxes[6 * c];
                    if (!(b[0] <= b[3] && b[1] <= b[4] && b[2] <= b[5])) continue;
                    for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], b[k]), hi[k] = std::max(hi[k], b[3 + k]);
                }
                root = area_ref(lo, hi);
            }
        }
        const long double want = root > 0.0L ? sum / root : 0.0L;
        CHECK(std::isfinite(got) && got >= 0.0);
        CHECK(std::fabs((long double)got - want) <= 1e-12L * (want > 1.0L ? want : 1.0L));
        if (nn == 0) CHECK(got == 0.0);
        ++trees;
    }
    std::printf("ok sequences %d edits %ld refused %ld trees %ld\n", sequences, edits_done, refused, trees);
    return 0;
}
