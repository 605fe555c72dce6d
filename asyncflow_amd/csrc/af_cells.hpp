// Cells across devices: the (group, window) cells of af_windowed.hpp / af_quantiles.hpp built from latencies that were EXPORTED
// per scenario (af_engine_export_cells, on the device that holds the scenario's rqs_clock) instead of from clock rows
// (af_engine_import_cells, on the device that reduces).  An exported scenario s is one contiguous SEGMENT of the imported
// array: its latencies inside the windows, window after window, a window's in row order; bounds[s][0 .. W] (the r_s[k] of
// af_windowed.hpp, or the c_s[k] of af_arrival.hpp) give the windows' lengths, begin[s] its first element.  The sample of cell
// c = g * W + w is, as everywhere, the concatenation in ascending member index over the members of g of the members' window w:
//   element j of scenario s (0 <= j < bounds[s][W] - bounds[s][0]) lies in the window w with
//       bounds[s][w] - bounds[s][0] <= j < bounds[s][w + 1] - bounds[s][0]
//   and goes to  cell_off[g W + w] + pre[s][w] + (j - (bounds[s][w] - bounds[s][0]))
// with pre[s][w] the latencies of that cell that earlier members bring: the compacted array of the unsharded call, element for
// element, whatever device a member ran on and wherever its segment lies.  The whole run (no windows) is W = 1: a segmented copy.
//   (host)   layout_cells: cell_off and pre from the bounds -- the ONE implementation, layout_window_cells of engine.hip calls it
//   merge    one workgroup per member streams its segment: 16-byte loads where the address allows (segments start at any 8-byte
//            offset: an odd head and an odd tail element go alone), the element's window by binary search over the member's bounds
//            (in LDS up to kLdsWindows windows, as af_win_compact), 8-byte stores.  Plain vector loads and stores, no atomics.
// The placement rule is plain C++ (g++ compiles this header: tests/hostcheck/cells_main.cpp); the kernel is HIP only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AFC_HD __host__ __device__ __forceinline__
#else
#define AFC_HD inline
#endif

namespace afc {

constexpr uint32_t kSkip = 0xFFFFFFFFu;       // AF_POOL_SKIP
constexpr uint32_t kLdsWindows = 4096;        // windows whose bounds and destinations the merge keeps in LDS (48 KB)
constexpr uint64_t kCellMax = 0xFFFFFFFFull;  // a cell holds at most this many latencies

// what layout_cells found wrong: nothing; a member's bounds decrease at window w; window w of group g holds 2^32 or more
enum class LayoutError { kNone, kOrder, kCellTooLarge };
struct LayoutResult {
    LayoutError error = LayoutError::kNone;
    uint32_t scenario = 0, group = 0, window = 0;
};

// The cells of n members with bounds [n][W + 1] in G groups (group: [n] or empty = all in group 0; kSkip: in no cell):
// cell_off [G W + 1] the cells' first latencies, pre [n][W].  check_order: decreasing bounds are an error (rows by finish time).
inline LayoutResult layout_cells(const uint32_t* bounds, const std::vector<uint32_t>& group, uint32_t n, uint32_t G, uint32_t W, bool check_order,
                                 std::vector<uint64_t>& cell_off, std::vector<uint32_t>& pre) {
    const size_t C = (size_t)G * W;
    cell_off.assign(C + 1u, 0u);   // (first the sizes, at [c + 1])
    pre.resize((size_t)n * W);
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t g = group.empty() ? 0u : group[s];
        if (g == kSkip) continue;
        const uint32_t* r = bounds + (size_t)s * (W + 1u);
        uint64_t* sz = cell_off.data() + 1u + (size_t)g * W;
        uint32_t* ps = pre.data() + (size_t)s * W;
        for (uint32_t w = 0; w < W; ++w) {
            if (check_order && r[w + 1u] < r[w]) return LayoutResult{LayoutError::kOrder, s, g, w};
            if (sz[w] > kCellMax) return LayoutResult{LayoutError::kCellTooLarge, s, g, w};
            ps[w] = (uint32_t)sz[w];
            sz[w] += r[w + 1u] - r[w];
        }
    }
    for (size_t c = 0; c < C; ++c) {
        if (cell_off[c + 1u] > kCellMax) return LayoutResult{LayoutError::kCellTooLarge, 0u, (uint32_t)(c / W), (uint32_t)(c % W)};
        cell_off[c + 1u] += cell_off[c];
    }
    return LayoutResult{};
}

// the window of row i of a member with bounds bs[0 .. W]: bs[w] <= i < bs[w + 1] (the caller has bs[0] <= i < bs[W])
AFC_HD uint32_t window_of(const uint32_t* bs, uint32_t n_win, uint32_t i) {
    uint32_t lo = 0u, hi = n_win - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bs[mid + 1u] <= i) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// where element j of a member's segment goes: bs its bounds [W + 1], pre_s its row of pre [W], off_g the offsets of its group's cells [W]
AFC_HD uint64_t destination(const uint32_t* bs, const uint32_t* pre_s, const uint64_t* off_g, uint32_t n_win, uint32_t j) {
    const uint32_t i = bs[0] + j;
    const uint32_t w = window_of(bs, n_win, i);
    return off_g[w] + pre_s[w] + (uint64_t)(i - bs[w]);
}

#if defined(__HIPCC__)

constexpr int kThreads = 256;

struct MergeArgs {
    const double* src;          // the imported latencies: the shards' exports, one after the other
    const uint64_t* begin;      // [n] first element of member s in src
    const uint32_t* bounds;     // [n][W + 1]
    const uint32_t* pre;        // [n][W]
    const uint64_t* cell_off;   // [G W + 1]
    const uint32_t* group;      // [n] or null (all in group 0)
    uint32_t n_win;             // W >= 1
    double* lat;                // the merged cells
};

// the segment of member blockIdx.x to its cells
template <bool kLds>
__global__ __launch_bounds__(kThreads) void af_cells_merge(MergeArgs a) {
    extern __shared__ __attribute__((aligned(8))) unsigned char dyn[];   // kLds: [W] u64 destinations - first row, then [W + 1] bounds
    const uint32_t s = blockIdx.x;
    const uint32_t g = a.group ? a.group[s] : 0u;
    if (g == kSkip) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t W = a.n_win;
    const uint32_t* gb = a.bounds + (size_t)s * (W + 1u);
    const uint32_t* gpre = a.pre + (size_t)s * W;
    const uint64_t* goff = a.cell_off + (size_t)g * W;
    uint64_t* ldst = reinterpret_cast<uint64_t*>(dyn);
    uint32_t* lb = reinterpret_cast<uint32_t*>(dyn + (size_t)(kLds ? W : 0u) * 8u);
    if (kLds) {
        for (uint32_t k = tid; k <= W; k += kThreads) lb[k] = gb[k];
        for (uint32_t w = tid; w < W; w += kThreads) ldst[w] = goff[w] + gpre[w] - gb[w];   // (+ the row's index: its place)
        __syncthreads();
    }
    const uint32_t* bs = kLds ? lb : gb;
    const uint32_t r0 = bs[0], len = bs[W] - r0;
    if (len == 0u) return;
    const double* src = a.src + a.begin[s];
    const auto place = [&](uint32_t j, double x) {
        const uint32_t i = r0 + j;
        const uint32_t w = window_of(bs, W, i);
        const uint64_t d = kLds ? ldst[w] + i : goff[w] + gpre[w] + (uint64_t)(i - gb[w]);
        a.lat[d] = x;
    };
    const uint32_t head = (uint32_t)((reinterpret_cast<uintptr_t>(src) >> 3) & 1u);   // (len >= 1) an element before the first 16-byte boundary
    const uint32_t n_pair = (len - head) >> 1, tail = (len - head) & 1u;
    if (tid == 0u && head) place(0u, src[0]);
    if (tid == 1u && tail) place(len - 1u, src[len - 1u]);
    const double2* src2 = reinterpret_cast<const double2*>(src + head);
    constexpr uint32_t kU = 4;
    for (uint32_t p0 = tid; p0 < n_pair; p0 += kU * kThreads) {
        double2 c[kU];
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) c[u] = p0 + u * kThreads < n_pair ? src2[p0 + u * kThreads] : double2{};
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) {
            const uint32_t p = p0 + u * kThreads;
            if (p < n_pair) {
                place(head + 2u * p, c[u].x);
                place(head + 2u * p + 1u, c[u].y);
            }
        }
    }
}

#endif  // __HIPCC__

}  // namespace afc
