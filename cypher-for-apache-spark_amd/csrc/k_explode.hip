// k_explode.hip -- UNWIND: functions.explode of a list column or of a literal list
// (okapi-relational/.../impl/planning/RelationalPlanner.scala:94-96 lowers logical.Unwind(list, item, in) to
// in.add(Explode(list) as item); spark-cypher/.../impl/SparkSQLExprMapper.scala:237-241 maps Explode to
// functions.explode: one output row per element, none for a null or an empty list).
//
// Column form.  Row i's list is store list word[i] (any index, repeated after a join, shifted after a union of
// stores); its length L_i is 0 for a null row.  An exclusive scan of the lengths gives every row's first output
// row, the scan's last entry the output size m.  The rows with L_i > 0 are compacted (their starts then ascend
// strictly), and the expansion runs over fixed tiles of kExplodeTile OUTPUT rows: a tile's first source row
// comes from a binary search of the compacted starts (one thread per tile, a kernel of its own), the source
// rows that begin inside the tile mark their head slot in LDS, a max scan of the marks gives every slot its
// source row, and each slot writes its element and its source-row index.  A tile reads at most kExplodeTile
// compacted rows whatever the lengths are, so one list of a million elements among a million empty rows costs
// what a million one-element lists cost: O(n) for lengths, scan and compaction, O(m) for the expansion,
// O(tiles log n) for the searches.  (The owner-from-a-max-scan pattern of k_varlen.hip k_vl4_wedges.)
//
// Constant form (explode(array(lit...)), SparkSQLExprMapper.scala:86-89, 111-112): output row j repeats input
// row j / count with item values[j % count].
#include "tile_owner.h"

namespace capsmi {

namespace {

using namespace tiles;

// len[r] = elements of row r's list (0 for a null row), flag[r] = len > 0
__global__ void k_explode_len(const int64_t* __restrict__ word, const uint8_t* __restrict__ valid, int64_t n,
                              const int64_t* __restrict__ off, int64_t* __restrict__ len, uint8_t* __restrict__ flag) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t l = 0;
        if (valid == nullptr || valid[r]) {
            const int64_t w = word[r];
            l = off[w + 1] - off[w];
        }
        len[r] = l;
        flag[r] = l > 0 ? 1 : 0;
    }
}

// tk[i] = the last compacted row whose first output row is <= i * kExplodeTile (cs ascends strictly, cs[0] = 0)
__global__ void k_explode_heads(const int64_t* __restrict__ cs, int64_t k, int64_t ntiles, int64_t* __restrict__ tk) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ntiles; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j0 = i * kExplodeTile;
        int64_t lo = 0, hi = k;  // the first row whose start is > j0
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cs[mid] <= j0) lo = mid + 1; else hi = mid;
        }
        tk[i] = lo - 1;
    }
}

// cs: first output row of compacted row c (k of them); nz: its input row (null: c itself); word / off / vals:
// the input rows' list indices and the store
__global__ void __launch_bounds__(kExB) k_explode(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                 const int64_t* __restrict__ tk, int64_t m,
                                                 const int64_t* __restrict__ word, const int64_t* __restrict__ off,
                                                 const int64_t* __restrict__ vals, int64_t* __restrict__ item,
                                                 int64_t* __restrict__ src) {
    __shared__ TileLds L;
    const int t = threadIdx.x;
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        // slot s of a row holds store element sbase + s
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [&](int64_t r) { return off[word[r]]; });
#pragma unroll
        for (int j = 0; j < kExI; ++j) {
            const int i = t + j * kExB;
            if (i < nt) {
                const int c = L.own[i];
                item[j0 + i] = vals[L.sbase[c] + i];
                src[j0 + i] = L.srow[c];
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

__global__ void k_explode_values(int64_t total, int64_t count, const int64_t* __restrict__ vals,
                                 const uint8_t* __restrict__ vvalid, int64_t* __restrict__ item,
                                 uint8_t* __restrict__ item_valid, int64_t* __restrict__ src) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = j / count, e = j - r * count;
        src[j] = r;
        item[j] = vals[e];
        if (item_valid) item_valid[j] = vvalid[e];
    }
}

}  // namespace

void list_lengths(capsmi_session* s, const int64_t* word, const uint8_t* valid, int64_t n, const int64_t* off, int64_t* len,
                  uint8_t* flag) {
    hipLaunchKernelGGL(k_explode_len, dim3(grid_for(n)), dim3(256), 0, s->stream, word, valid, n, off, len, flag);
    HIP_CHECK(hipGetLastError());
}

TilePlan tile_plan(capsmi_session* s, const int64_t* len, const uint8_t* flag, int64_t n, const char* timer,
                   int64_t max_slots) {
    TilePlan tp;
    tp.starts = dev_alloc(sizeof(int64_t) * (n + 1), s);
    {
        KernelTimer kt(s, timer);
        exclusive_scan_i64(len, P<int64_t>(tp.starts), n, s);
    }
    tp.m = read_scalar(s, P<int64_t>(tp.starts) + n);
    if (tp.m == 0 || (max_slots >= 0 && tp.m > max_slots)) return tp;
    // the rows that contribute, in order; when every row does, the starts are already the compacted ones
    tp.cs = P<int64_t>(tp.starts);
    {
        KernelTimer kt(s, timer);
        tp.k = flags_to_indices(s, flag, n, tp.nzb);
        if (tp.k < n) {
            tp.csb = dev_alloc(sizeof(int64_t) * tp.k, s);
            gather_col(P<int64_t>(tp.starts), nullptr, P<int64_t>(tp.nzb), tp.k, P<int64_t>(tp.csb), nullptr, s->stream);
            tp.cs = P<int64_t>(tp.csb);
            tp.nz = P<int64_t>(tp.nzb);
        }
    }
    tp.ntiles = (tp.m + kExplodeTile - 1) / kExplodeTile;
    tp.tk = dev_alloc(sizeof(int64_t) * tp.ntiles, s);
    return tp;
}

// the tile heads of a plan (part of the consumer's timed launch)
void tile_heads(capsmi_session* s, const TilePlan& tp) {
    hipLaunchKernelGGL(k_explode_heads, dim3(grid_for(tp.ntiles)), dim3(256), 0, s->stream, tp.cs, tp.k, tp.ntiles,
                       P<int64_t>(tp.tk));
    HIP_CHECK(hipGetLastError());
}

int64_t explode_lists(capsmi_session* s, const int64_t* word, const uint8_t* valid, int64_t n, const ListStore& L,
                      Buf& item, Buf& src) {
    hipStream_t st = s->stream;
    item = src = nullptr;
    if (n == 0) return 0;
    Buf len = dev_alloc(sizeof(int64_t) * n, s), flag = dev_alloc(n, s);
    {
        KernelTimer kt(s, "explode_starts");
        list_lengths(s, word, valid, n, P<int64_t>(L.offsets), P<int64_t>(len), P<uint8_t>(flag));
    }
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), n, "explode_starts");
    const int64_t m = tp.m;
    if (m == 0) return 0;
    item = dev_alloc(sizeof(int64_t) * m, s);
    src = dev_alloc(sizeof(int64_t) * m, s);
    {
        // algorithmic bytes: n starts and n row words read, m values read, m items and m source rows written
        KernelTimer kt(s, "explode", 8.0 * (2.0 * (double)n + 3.0 * (double)m));
        tile_heads(s, tp);
        hipLaunchKernelGGL(k_explode, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k, P<int64_t>(tp.tk), m,
                           word, P<int64_t>(L.offsets), P<int64_t>(L.values), P<int64_t>(item), P<int64_t>(src));
        HIP_CHECK(hipGetLastError());
    }
    return m;
}

void explode_values(capsmi_session* s, int64_t n, int64_t count, const int64_t* vals, const uint8_t* vvalid, int64_t* item,
                    uint8_t* item_valid, int64_t* src) {
    const int64_t total = n * count;
    if (total <= 0) return;
    // m values read (from `count` words that stay in cache), m items and m source rows written
    KernelTimer kt(s, "explode_values", 8.0 * 2.0 * (double)total + 8.0 * (double)count);
    const int64_t cap = (int64_t)s->num_cus * 32, g = (total + 255) / 256;
    hipLaunchKernelGGL(k_explode_values, dim3((unsigned)(g > cap ? cap : g)), dim3(256), 0, s->stream, total, count, vals,
                       vvalid, item, item_valid, src);
    HIP_CHECK(hipGetLastError());
}

}  // namespace capsmi
