// tile_owner.h -- the fixed-tile expansion of per-row lengths that k_explode.hip and k_listexpr.hip share.
//
// Rows with lengths L_r (0 for a null row) own m = sum L_r virtual (row, position) slots, numbered in (row,
// position) order; an exclusive scan of the lengths gives every row's first slot.  The rows with L_r > 0 are
// compacted (their starts then ascend strictly), and the work runs over fixed tiles of kExplodeTile slots: a
// tile's first row comes from a binary search of the compacted starts (one thread per tile), the rows that begin
// inside the tile mark their head slot in LDS, and a max scan of the marks gives every slot its row.  A tile
// reads at most kExplodeTile compacted rows whatever the lengths are, so its work does not depend on the length
// distribution.  (The owner-from-a-max-scan pattern of k_varlen.hip k_vl4_wedges.)
#pragma once

#include "capsmi_impl.h"

namespace capsmi {

// The slots of n rows with lengths len (flag[r] = len[r] > 0), planned on the device (tile_plan, k_explode.hip;
// synchronises).  m == 0, or m above the caller's `max_slots` (>= 0): nothing but m and starts is set, and nothing
// sized by m has been allocated -- the caller refuses the count.
struct TilePlan {
    int64_t m = 0, k = 0, ntiles = 0;
    Buf starts;                  // n + 1: the exclusive scan of the lengths
    Buf nzb, csb, tk;            // compacted rows, their starts (when k < n), first compacted row per tile
    const int64_t* cs = nullptr; // first slot of compacted row c (k of them)
    const int64_t* nz = nullptr; // its row (null: c itself)
};
TilePlan tile_plan(capsmi_session* s, const int64_t* len, const uint8_t* flag, int64_t n, const char* timer,
                   int64_t max_slots = -1);
// fills tp.tk (queued; part of the consumer's timed launch)
void tile_heads(capsmi_session* s, const TilePlan& tp);
// len[r] = elements of row r's list (0 for a null row), flag[r] = len > 0
void list_lengths(capsmi_session* s, const int64_t* word, const uint8_t* valid, int64_t n, const int64_t* off, int64_t* len,
                  uint8_t* flag);

namespace tiles {

constexpr int kExB = 256;                   // threads per block
constexpr int kExI = kExplodeTile / kExB;   // slots per thread
static_assert(kExplodeTile % kExB == 0 && kExplodeTile <= 65536, "tile slots are uint16 marks, kExI per thread");

inline unsigned grid_for(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// blocks of a tile kernel: every tile its block up to a few resident blocks per CU, then block-stride
inline unsigned tile_grid(const capsmi_session* s, int64_t ntiles) {
    const int64_t cap = (int64_t)s->num_cus * 8;
    return (unsigned)(ntiles < 1 ? 1 : (ntiles > cap ? cap : ntiles));
}

// max over the threads before this one of one value per thread (kExB threads)
__device__ __forceinline__ uint32_t max_before(uint32_t v, uint32_t* wtot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x = max(x, y);
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    const uint32_t xp = __shfl_up(x, 1, 64);  // every lane active
    uint32_t pre = lane > 0 ? xp : 0u;
    for (int q = 0; q < wave; ++q) pre = max(pre, wtot[q]);
    __syncthreads();  // wtot is reused by the next tile
    return pre;
}

struct TileLds {
    int64_t sbase[kExplodeTile];  // base_of(row) minus the slot (tile-relative) of the tile's c-th row's position 0
    int64_t srow[kExplodeTile];   // its row
    uint16_t own[kExplodeTile];   // slot -> its row (tile-local c)
    uint32_t wtot[kExB / 64];
};

// Fills L for the tile of nt slots that starts at slot j0 and whose first compacted row is c0: afterwards slot i
// (< nt) belongs to the tile-local row c = L.own[i], which is row L.srow[c], and is position L.sbase[c] + i -
// base_of(row) of it (so with base_of = the row's first store element, L.sbase[c] + i is the slot's element).
// Every thread of the block calls it (block-uniform arguments); ends with a barrier.
template <class F>
__device__ __forceinline__ void tile_owners(TileLds& L, const int64_t* __restrict__ cs, const int64_t* __restrict__ nz,
                                            int64_t k, int64_t c0, int64_t j0, int nt, F base_of) {
    const int t = threadIdx.x;
    for (int i = t; i < kExplodeTile; i += kExB) L.own[i] = 0;
    __syncthreads();
    for (int i = t; i < kExplodeTile && c0 + i < k; i += kExB) {
        const int64_t w = cs[c0 + i];
        if (i > 0 && w >= j0 + nt) break;  // past the tile (starts ascend)
        const int64_t r = nz ? nz[c0 + i] : c0 + i;
        L.sbase[i] = base_of(r) - (w - j0);
        L.srow[i] = r;
        if (i > 0) L.own[w - j0] = (uint16_t)i;  // w > j0: row c0 is the last one starting at or before j0
    }
    __syncthreads();
    // fill forward: own[s] = max(own[0..s]) (the heads ascend with c); thread t holds slots kExI*t ..
    uint32_t v[kExI];
    uint32_t mx = 0;
#pragma unroll
    for (int j = 0; j < kExI; ++j) {
        mx = max(mx, (uint32_t)L.own[t * kExI + j]);
        v[j] = mx;
    }
    const uint32_t pre = max_before(mx, L.wtot);
#pragma unroll
    for (int j = 0; j < kExI; ++j) L.own[t * kExI + j] = (uint16_t)max(v[j], pre);
    __syncthreads();
}

}  // namespace tiles
}  // namespace capsmi
