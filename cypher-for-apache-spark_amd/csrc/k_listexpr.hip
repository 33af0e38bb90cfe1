// k_listexpr.hip -- the list expressions whose work is proportional to the elements, not to the rows:
//   x IN list-column (SparkSQLExprMapper.scala:138-145, array_contains) ........ list_contains
//   range(from, to, step) (SparkSQLExprMapper.scala:243-245, CAPSFunctions.scala:50 rangeUdf) .. range_lists
// (size() and list[i] are two offset reads and one value read per row: they live in the interpreter, k_expr.hip.)
//
// Both run over the fixed tiles of tile_owner.h, as k_explode.hip does: a scan of the per-row lengths (0 for a
// null row; taken through the row's list word, so rows that repeat a list index after a join, or index a shifted
// union store, work), then tiles of kExplodeTile virtual (row, position) slots whose owners come from a max scan
// of head marks in LDS.  One list of a million elements among a million empty rows costs what a million
// one-element lists cost.
//
// list_contains: every slot compares its element with its row's probe word; a match stores 1 into hit[row] -- a
// plain byte store: every writer writes the same value, so no atomic is needed.  A row-wise finish composes the
// three-valued result: NULL when the probe or the list is NULL or the element type cannot be compared with the
// probe's, TRUE on a hit, else FALSE (stores hold no element nulls).  Equality is the interpreter's `=` (k_expr.hip
// cmp3): Long against Double as doubles, NaN equal to NaN.
//
// range_lists: lengths without signed overflow (to - from as an unsigned difference), a step-0 flag, the scan --
// which is the new store's offsets -- and a tiled fill: slot p of row r holds from + p * step, never past `to`.
#include "tile_owner.h"

namespace capsmi {

namespace {

using namespace tiles;

enum { kCmpWord = 0, kCmpF64 = 1 };  // equality of the raw words; of both sides as doubles

__device__ __forceinline__ double word_f64(int64_t w, bool is_f64) { return is_f64 ? __longlong_as_double(w) : (double)w; }

template <int MODE>
__global__ void __launch_bounds__(kExB) k_list_contains(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz,
                                                       int64_t k, const int64_t* __restrict__ tk, int64_t m,
                                                       const int64_t* __restrict__ word, const int64_t* __restrict__ off,
                                                       const int64_t* __restrict__ vals, const int64_t* __restrict__ probe,
                                                       const uint8_t* __restrict__ pvalid, bool probe_f64, bool elem_f64,
                                                       uint8_t* __restrict__ hit) {
    __shared__ TileLds L;
    const int t = threadIdx.x;
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [&](int64_t r) { return off[word[r]]; });
#pragma unroll
        for (int j = 0; j < kExI; ++j) {
            const int i = t + j * kExB;
            if (i < nt) {
                const int c = L.own[i];
                const int64_t r = L.srow[c];
                if (pvalid == nullptr || pvalid[r]) {
                    const int64_t e = vals[L.sbase[c] + i], x = probe[r];
                    bool eq;
                    if (MODE == kCmpWord) {
                        eq = e == x;
                    } else {
                        const double a = word_f64(x, probe_f64), b = word_f64(e, elem_f64);
                        eq = a == b || (a != a && b != b);
                    }
                    if (eq) hit[r] = 1;
                }
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

__global__ void k_contains_finish(const uint8_t* __restrict__ hit, const uint8_t* __restrict__ pvalid,
                                  const uint8_t* __restrict__ lvalid, bool comparable, int64_t n, int64_t* __restrict__ out,
                                  uint8_t* __restrict__ out_valid) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const bool ok = comparable && (pvalid == nullptr || pvalid[r]) && (lvalid == nullptr || lvalid[r]);
        out[r] = ok && hit[r] ? 1 : 0;
        out_valid[r] = ok ? 1 : 0;
    }
}

// the largest length a row may report: the sum over n rows stays below 2^62
__host__ __device__ inline uint64_t range_row_cap(int64_t n) {
    const uint64_t c = (uint64_t(1) << 62) / (uint64_t)(n > 0 ? n : 1);
    return c < (uint64_t(1) << 40) ? c : (uint64_t(1) << 40);
}

// len[r] = elements of from, from + step, .. up to `to` (0 for a null row, saturated at cap), flag, row validity;
// err[0] = 1 when some row's step is 0, err[1] = 1 when some row's length was saturated
__global__ void k_range_len(const int64_t* __restrict__ from, const uint8_t* __restrict__ fv, const int64_t* __restrict__ to,
                            const uint8_t* __restrict__ tv, const int64_t* __restrict__ step,
                            const uint8_t* __restrict__ sv, int64_t n, uint64_t cap, int64_t* __restrict__ len,
                            uint8_t* __restrict__ flag, uint8_t* __restrict__ valid, int64_t* __restrict__ err) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const bool ok = (fv == nullptr || fv[r]) && (tv == nullptr || tv[r]) && (sv == nullptr || sv[r]);
        uint64_t l = 0;
        if (ok) {
            const int64_t a = from[r], b = to[r], st = step ? step[r] : 1;
            if (st == 0) {
                err[0] = 1;
            } else if (st > 0 ? a <= b : a >= b) {
                // |to - from| < 2^64 and |step| <= 2^63 as unsigned words
                const uint64_t d = st > 0 ? (uint64_t)b - (uint64_t)a : (uint64_t)a - (uint64_t)b;
                const uint64_t us = st > 0 ? (uint64_t)st : 0ULL - (uint64_t)st;
                const uint64_t q = d / us;
                if (q >= cap) {
                    l = cap;
                    err[1] = 1;
                } else {
                    l = q + 1;
                }
            }
        }
        len[r] = (int64_t)l;
        flag[r] = l > 0 ? 1 : 0;
        valid[r] = ok ? 1 : 0;
    }
}

// slot p of row r = from[r] + p * step[r]: p < len[r], so the element lies between from and to and the wrapping
// unsigned arithmetic is exact
__global__ void __launch_bounds__(kExB) k_range_fill(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                    const int64_t* __restrict__ tk, int64_t m,
                                                    const int64_t* __restrict__ from, const int64_t* __restrict__ step,
                                                    int64_t* __restrict__ vals) {
    __shared__ TileLds L;
    const int t = threadIdx.x;
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
                const int64_t r = L.srow[c];
                const uint64_t p = (uint64_t)(L.sbase[c] + i), st = step ? (uint64_t)step[r] : 1ULL;
                vals[j0 + i] = (int64_t)((uint64_t)from[r] + p * st);
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

}  // namespace

void list_contains(capsmi_session* s, const int64_t* probe, const uint8_t* pvalid, int32_t ptype, const int64_t* word,
                   const uint8_t* lvalid, const ListStore& L, int64_t n, int64_t* out, uint8_t* out_valid) {
    if (n == 0) return;
    hipStream_t st = s->stream;
    const int32_t et = L.elem;
    const bool num = (ptype == CAPSMI_I64 || ptype == CAPSMI_F64) && (et == CAPSMI_I64 || et == CAPSMI_F64);
    const bool comparable = num || ptype == et;
    Buf hit = dev_alloc(n, s);
    fill_u8(P<uint8_t>(hit), 0, n, st);
    if (comparable) {
        Buf len = dev_alloc(sizeof(int64_t) * n, s), flag = dev_alloc(n, s);
        {
            KernelTimer kt(s, "list_contains_starts");
            list_lengths(s, word, lvalid, n, P<int64_t>(L.offsets), P<int64_t>(len), P<uint8_t>(flag));
        }
        const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), n, "list_contains_starts");
        if (tp.m > 0) {
            // algorithmic bytes: n starts, n row words and n probe words read, M element words read (the hit
            // bytes and the 9 n bytes of the finish are not counted)
            KernelTimer kt(s, "list_contains", 8.0 * (3.0 * (double)n + (double)tp.m));
            tile_heads(s, tp);
            const bool words = !num || (ptype == CAPSMI_I64 && et == CAPSMI_I64);
            auto kern = words ? k_list_contains<kCmpWord> : k_list_contains<kCmpF64>;
            hipLaunchKernelGGL(kern, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k, P<int64_t>(tp.tk),
                               tp.m, word, P<int64_t>(L.offsets), P<int64_t>(L.values), probe, pvalid, ptype == CAPSMI_F64,
                               et == CAPSMI_F64, P<uint8_t>(hit));
            HIP_CHECK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_contains_finish, dim3(grid_for(n)), dim3(256), 0, st, P<uint8_t>(hit), pvalid, lvalid, comparable, n,
                       out, out_valid);
    HIP_CHECK(hipGetLastError());
}

std::shared_ptr<ListStore> range_lists(capsmi_session* s, const int64_t* from, const uint8_t* fv, const int64_t* to,
                                       const uint8_t* tv, const int64_t* step, const uint8_t* sv, int64_t n, Buf& valid) {
    hipStream_t st = s->stream;
    auto L = std::make_shared<ListStore>();
    L->elem = CAPSMI_I64;
    L->nlists = n;
    valid = dev_alloc(n > 0 ? n : 1, s);
    if (n == 0) {  // no rows: one offset, no element
        L->offsets = dev_alloc(sizeof(int64_t), s);
        fill_i64(P<int64_t>(L->offsets), 0, 1, st);
        L->values = dev_alloc(sizeof(int64_t), s);
        return L;
    }
    Buf len = dev_alloc(sizeof(int64_t) * n, s), flag = dev_alloc(n, s);
    Buf err = dev_alloc(sizeof(int64_t) * 2, s);
    fill_i64(P<int64_t>(err), 0, 2, st);
    {
        KernelTimer kt(s, "list_range_starts");
        hipLaunchKernelGGL(k_range_len, dim3(grid_for(n)), dim3(256), 0, st, from, fv, to, tv, step, sv, n, range_row_cap(n),
                           P<int64_t>(len), P<uint8_t>(flag), P<uint8_t>(valid), P<int64_t>(err));
        HIP_CHECK(hipGetLastError());
    }
    REQUIRE(read_scalar(s, P<int64_t>(err)) == 0, CAPSMI_ERR_ILLEGAL_ARGUMENT, "range: step 0");
    const bool saturated = read_scalar(s, P<int64_t>(err) + 1) != 0;
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    // the scan's total is read, and refused below, before anything sized by it is allocated (a saturated row
    // refuses whatever the total is)
    const int64_t max_slots = saturated ? 0 : (int64_t)(total_b / 8);
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), n, "list_range_starts", max_slots);
    // more words than the device has: refused here, before anything is allocated (a count the device could hold
    // but the pool cannot give right now is the allocator's CAPSMI_ERR_OUT_OF_MEMORY)
    REQUIRE(!saturated && tp.m <= max_slots, CAPSMI_ERR_UNSUPPORTED,
            "range: " + std::to_string((long long)tp.m) + (saturated ? " or more" : "") +
                " elements exceed what the session can allocate (" + std::to_string((unsigned long long)total_b) +
                " bytes of device memory)");
    L->offsets = tp.starts;
    L->nvalues = tp.m;
    L->values = dev_alloc(sizeof(int64_t) * (tp.m > 0 ? tp.m : 1), s);
    if (tp.m > 0) {
        // algorithmic bytes: n starts, n from and n step words read, M element words written
        KernelTimer kt(s, "list_range", 8.0 * (3.0 * (double)n + (double)tp.m));
        tile_heads(s, tp);
        hipLaunchKernelGGL(k_range_fill, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k,
                           P<int64_t>(tp.tk), tp.m, from, step, P<int64_t>(L->values));
        HIP_CHECK(hipGetLastError());
    }
    return L;
}

}  // namespace capsmi
