// k_masklist.hip -- lists built from per-row masks over a fixed set of names (capsmi_with_mask_list_column):
//   labels(n) (SparkSQLExprMapper.scala:192-201, CAPSFunctions.scala:73-81 get_node_labels) ... CAPSMI_MASK_TRUE
//   keys(n)   (SparkSQLExprMapper.scala:203-208, CAPSFunctions.scala:83-91 get_property_keys) . CAPSMI_MASK_NOT_NULL
// The reference runs a UDF per row over array(flag or property columns); here a row is one 64-bit word.
//
// k_mask_len: one lane per row, the columns in the outer loop (every column's loads coalesce): bit i of the
// row's mask is set when column i passes -- non-null and TRUE, or non-null -- and the row's length is the mask's
// popcount.  The scan of the lengths (tile_plan) is the new store's offsets.
// k_mask_fill: over the fixed tiles of tile_owner.h, as k_listexpr.hip range_lists: slot p of row r holds
// codes[select(mask[r], p)], select = the index of the p-th set bit, found by six popcount halvings.  The codes
// (at most 64 words) sit in LDS.  One row of 64 names among a million empty rows costs what a million one-name
// rows cost.
#include "tile_owner.h"

namespace capsmi {

namespace {

using namespace tiles;

// the columns of a mask, by value in the kernel arguments (64 x two pointers = 1 KiB), as k_expr.hip's ColPtrs
struct MaskCols {
    const int64_t* data[kMaskListCols];   // CAPSMI_MASK_TRUE: the flag words (unused under CAPSMI_MASK_NOT_NULL)
    const uint8_t* valid[kMaskListCols];  // null: the column holds no nulls
};

// mask[r] bit i = column i passes in row r; len[r] = popcount; flag[r] = len > 0
template <int MODE>
__global__ void k_mask_len(MaskCols cp, int ncols, int64_t n, int64_t* __restrict__ mask, int64_t* __restrict__ len,
                           uint8_t* __restrict__ flag) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        uint64_t m = 0;
        for (int c = 0; c < ncols; ++c) {  // wave-uniform: the pointers are scalar loads
            const uint8_t* v = cp.valid[c];
            bool pass = v == nullptr || v[r] != 0;
            if (MODE == CAPSMI_MASK_TRUE) pass = pass & (cp.data[c][r] != 0);  // a word under a null row is masked
            m |= (uint64_t)pass << c;
        }
        const int l = __popcll(m);
        mask[r] = (int64_t)m;
        len[r] = l;
        flag[r] = l > 0 ? 1 : 0;
    }
}

// index of the p-th (0-based) set bit of m; p < popcount(m)
__device__ __forceinline__ int select_bit(uint64_t m, uint32_t p) {
    int pos = 0;
    uint32_t c = __popc((uint32_t)m);
    bool up = p >= c;
    uint32_t x = up ? (uint32_t)(m >> 32) : (uint32_t)m;
    p -= up ? c : 0;
    pos += up ? 32 : 0;
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        c = __popc(x & ((1u << w) - 1u));
        up = p >= c;
        x = up ? x >> w : x;
        p -= up ? c : 0;
        pos += up ? w : 0;
    }
    return pos;
}

__global__ void __launch_bounds__(kExB) k_mask_fill(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                   const int64_t* __restrict__ tk, int64_t m,
                                                   const int64_t* __restrict__ mask, const int64_t* __restrict__ codes,
                                                   int ncodes, int64_t* __restrict__ vals) {
    __shared__ TileLds L;
    __shared__ int64_t scodes[kMaskListCols];
    const int t = threadIdx.x;
    if (t < kMaskListCols) scodes[t] = t < ncodes ? codes[t] : 0;  // the first tile_owners barrier publishes them
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [](int64_t) { return (int64_t)0; });  // sbase + i = position
#pragma unroll
        for (int j = 0; j < kExI; ++j) {
            const int i = t + j * kExB;
            if (i < nt) {
                const int c = L.own[i];
                const uint32_t p = (uint32_t)(L.sbase[c] + i);
                vals[j0 + i] = scodes[select_bit((uint64_t)mask[L.srow[c]], p)];
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

}  // namespace

std::shared_ptr<ListStore> mask_lists(capsmi_session* s, int32_t mode, const std::vector<const int64_t*>& data,
                                      const std::vector<const uint8_t*>& valid, const std::vector<int64_t>& codes,
                                      int64_t n) {
    hipStream_t st = s->stream;
    const int ncols = (int)codes.size();
    REQUIRE(ncols <= kMaskListCols && data.size() == codes.size() && valid.size() == codes.size(), CAPSMI_ERR_INTERNAL,
            "mask list: column count");
    auto L = std::make_shared<ListStore>();
    L->elem = CAPSMI_STR;
    L->nlists = n;
    if (n == 0) {  // no rows: one offset, no element
        L->offsets = dev_alloc(sizeof(int64_t), s);
        fill_i64(P<int64_t>(L->offsets), 0, 1, st);
        L->values = dev_alloc(sizeof(int64_t), s);
        return L;
    }
    MaskCols cp;
    int nullable = 0;
    for (int c = 0; c < kMaskListCols; ++c) {
        cp.data[c] = c < ncols ? data[c] : nullptr;
        cp.valid[c] = c < ncols ? valid[c] : nullptr;
        nullable += cp.valid[c] != nullptr;
    }
    Buf mask = dev_alloc(sizeof(int64_t) * n, s), len = dev_alloc(sizeof(int64_t) * n, s), flag = dev_alloc(n, s);
    {
        // algorithmic bytes: a flag word per column and a validity byte per nullable column read (validity bytes
        // alone under NOT_NULL); mask, length and flag written
        const double in_b = mode == CAPSMI_MASK_TRUE ? 8.0 * ncols + nullable : (double)nullable;
        KernelTimer kt(s, "mask_list_len", (in_b + 17.0) * (double)n);
        auto kern = mode == CAPSMI_MASK_TRUE ? k_mask_len<CAPSMI_MASK_TRUE> : k_mask_len<CAPSMI_MASK_NOT_NULL>;
        hipLaunchKernelGGL(kern, dim3(grid_for(n)), dim3(256), 0, st, cp, ncols, n, P<int64_t>(mask), P<int64_t>(len),
                           P<uint8_t>(flag));
        HIP_CHECK(hipGetLastError());
    }
    // the names' codes: queued before the scan, whose read-back completes the copy while `codes` is alive
    Buf dcodes = dev_alloc(sizeof(int64_t) * (ncols > 0 ? ncols : 1), s);
    if (ncols > 0)
        HIP_CHECK(hipMemcpyAsync(P<void>(dcodes), codes.data(), sizeof(int64_t) * ncols, hipMemcpyHostToDevice, st));
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    // as range_lists: the scan's total is read, and refused, before anything sized by it is allocated
    const int64_t max_slots = (int64_t)(total_b / 8);
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), n, "mask_list_starts", max_slots);
    REQUIRE(tp.m <= max_slots, CAPSMI_ERR_UNSUPPORTED,
            "mask list: " + std::to_string((long long)tp.m) + " elements exceed what the session can allocate (" +
                std::to_string((unsigned long long)total_b) + " bytes of device memory)");
    L->offsets = tp.starts;
    L->nvalues = tp.m;
    L->values = dev_alloc(sizeof(int64_t) * (tp.m > 0 ? tp.m : 1), s);
    if (tp.m > 0) {  // m == 0: nothing to write, no launch (the plan holds nothing but m and the starts)
        // algorithmic bytes: n starts and n masks read, M element words written
        KernelTimer kt(s, "mask_list", 8.0 * (2.0 * (double)n + (double)tp.m));
        tile_heads(s, tp);
        hipLaunchKernelGGL(k_mask_fill, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k,
                           P<int64_t>(tp.tk), tp.m, P<int64_t>(mask), P<int64_t>(dcodes), ncols, P<int64_t>(L->values));
        HIP_CHECK(hipGetLastError());
    }
    return L;
}

}  // namespace capsmi
