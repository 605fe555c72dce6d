// TEST-ONLY stand-alone program: the placement rule of asyncflow_amd/csrc/af_cells.hpp (afc::layout_cells: cell_off and pre from
// the members' bounds; afc::window_of and afc::destination: where element j of a member's segment goes) as g++ compiles it, built
// with -fsanitize=address,undefined by tests/test_sharded_cells_hostcheck.py.  Bounds, groups and the rule's arrays live in heap
// blocks of exactly their size, so an index one past any of them is a sanitizer report.
//
// stdin:  cases of  `n G W`  (W >= 1) then n group ids (4294967295: in no cell) and n (W + 1) bounds, all decimal u32.
// stdout: per case one line  `error total`  (afc::LayoutError as a number; the latencies in all cells), then -- without an error --
//         one line per member: the destination of every element of its segment in order (an empty line for none).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../asyncflow_amd/csrc/af_cells.hpp"

int main() {
    uint32_t n, G, W;
    while (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &n, &G, &W) == 3) {
        std::vector<uint32_t> group(n);
        for (uint32_t s = 0; s < n; ++s)
            if (std::scanf("%" SCNu32, &group[s]) != 1) return 2;
        uint32_t* bounds = new uint32_t[(size_t)n * (W + 1u)];
        for (size_t i = 0; i < (size_t)n * (W + 1u); ++i)
            if (std::scanf("%" SCNu32, &bounds[i]) != 1) return 2;
        std::vector<uint64_t> cell_off;
        std::vector<uint32_t> pre;
        const afc::LayoutResult lr = afc::layout_cells(bounds, group, n, G, W, true, cell_off, pre);
        const size_t C = (size_t)G * W;
        std::printf("%d %" PRIu64 "\n", (int)lr.error, lr.error == afc::LayoutError::kNone ? cell_off[C] : (uint64_t)0);
        if (lr.error == afc::LayoutError::kNone) {
            // exact-size copies: the rule reads W + 1 bounds, W entries of pre and W offsets of the member's group, nothing else
            for (uint32_t s = 0; s < n; ++s) {
                if (group[s] != afc::kSkip) {
                    uint32_t* bs = new uint32_t[W + 1u];
                    uint32_t* ps = new uint32_t[W];
                    uint64_t* og = new uint64_t[W];
                    std::memcpy(bs, bounds + (size_t)s * (W + 1u), (W + 1u) * sizeof(uint32_t));
                    std::memcpy(ps, pre.data() + (size_t)s * W, W * sizeof(uint32_t));
                    std::memcpy(og, cell_off.data() + (size_t)group[s] * W, W * sizeof(uint64_t));
                    const uint32_t len = bs[W] - bs[0];
                    for (uint32_t j = 0; j < len; ++j) std::printf(j ? " %" PRIu64 : "%" PRIu64, afc::destination(bs, ps, og, W, j));
                    delete[] bs;
                    delete[] ps;
                    delete[] og;
                }
                std::printf("\n");
            }
        }
        delete[] bounds;
    }
    return 0;
}
