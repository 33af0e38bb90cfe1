// k_strconv.hip -- size(), toInteger(), toFloat() and toBoolean() of dictionary-coded strings
// (SparkSQLExprMapper.scala:124-127 functions.length, :231 and :229 casts of a String, :235 ToBoolean; the rules
// are stated per opcode in include/capsmi.h, the parsing code is str_conv.h).
//
// A String value is a code; the bytes live in the session's string store.  As in k_strmatch.hip a conversion runs
// in three steps:
//   1. index (k_str_index, shared): the operand's rows -> store indices, -1 for a null row.
//   2. convert, one value word and one validity byte per "row":
//      toInteger / toFloat / toBoolean (k_str_conv): one thread per row parses its string, front to back.  The
//      slow path of toFloat keeps strconv::kDecDigits decimal digits per thread in private memory; only the
//      lanes that take it touch them (DESIGN.md has the figures and why this is not an LDS slab).
//      size (k_str_size): a count of bytes, so it is load-balanced: row r owns one slot per byte of its string,
//      the slots run over the fixed tiles of tile_owner.h, a thread counts the lead bytes among its kExI
//      neighbouring slots and adds a run's count to its owner's LDS counter, and the tile adds every owner's
//      count to the row's sum with one ordinary 64-bit atomic add (only a tile's first and last owner are
//      shared with another tile).  One megabyte-long string costs what the same bytes in short strings cost.
//   3. lookup (k_str_conv_lookup), on the dictionary side only: step 2 ran once per store entry (entry e is
//      "row" e) and the rows gather val[idx[r]] and ok[idx[r]].  On the rows side step 2 writes the result column
//      itself.
// Which side: the store when the table has at least as many rows as the store has entries; CAPSMI_STR_MATCH =
// rows | dict forces one.
#include <string>
#include <vector>

#include "str_conv.h"
#include "tile_owner.h"

namespace capsmi {

namespace {

using namespace tiles;

// idx null: the rows are the store's entries
__device__ __forceinline__ int64_t entry_of(const int64_t* __restrict__ idx, int64_t r) { return idx ? idx[r] : r; }

template <int OP>
__global__ void __launch_bounds__(256) k_str_conv(const int64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                  const int64_t* __restrict__ idx, int64_t n, int64_t* __restrict__ val,
                                                  uint8_t* __restrict__ ok) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = entry_of(idx, r);
        int64_t v = 0;
        bool good = false;
        if (e >= 0) {
            const int64_t b = off[e], len = off[e + 1] - b;
            const uint8_t* p = bytes + b;
            if constexpr (OP == CAPSMI_X_STR_TO_INTEGER) {
                good = strconv::to_integer(p, len, &v);
            } else if constexpr (OP == CAPSMI_X_STR_TO_FLOAT) {
                uint64_t u = 0;
                good = strconv::to_float(p, len, &u);
                v = (int64_t)u;
            } else {
                const int t = strconv::to_boolean(p, len);
                good = t >= 0;
                v = t > 0 ? 1 : 0;
            }
        }
        val[r] = good ? v : 0;
        ok[r] = good ? 1 : 0;
    }
}

// size: len[r] = bytes of row r's string (0 for a null row), flag[r] = len > 0; valid[r] (when given) = not null
__global__ void k_str_bytes(const int64_t* __restrict__ off, const int64_t* __restrict__ idx, int64_t n,
                            int64_t* __restrict__ len, uint8_t* __restrict__ flag, uint8_t* __restrict__ valid) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = entry_of(idx, r);
        const int64_t l = e >= 0 ? off[e + 1] - off[e] : 0;
        len[r] = l;
        flag[r] = l > 0 ? 1 : 0;
        if (valid) valid[r] = e >= 0 ? 1 : 0;
    }
}

// slot i of a tile is byte L.sbase[c] + i of the byte array; sum[row] += the slot's lead bytes
__global__ void __launch_bounds__(kExB) k_str_size(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                  const int64_t* __restrict__ tk, int64_t m,
                                                  const int64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                  const int64_t* __restrict__ idx, int64_t* __restrict__ sum) {
    __shared__ TileLds L;
    __shared__ uint32_t cnt[kExplodeTile];
    const int t = threadIdx.x;
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        for (int i = t; i < kExplodeTile; i += kExB) cnt[i] = 0;
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [&](int64_t r) { return off[entry_of(idx, r)]; });
        // thread t holds slots kExI * t ..: a run of one owner is counted in a register
        int cur = -1;
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < kExI; ++j) {
            const int i = t * kExI + j;
            if (i < nt) {
                const int c = L.own[i];
                if (c != cur) {
                    if (run) atomicAdd(&cnt[cur], run);
                    cur = c;
                    run = 0;
                }
                run += strconv::is_lead_byte(bytes[L.sbase[c] + i]) ? 1u : 0u;
            }
        }
        if (run) atomicAdd(&cnt[cur], run);
        __syncthreads();
        const int last = L.own[nt - 1];
        for (int c = t; c <= last; c += kExB)
            if (cnt[c]) atomicAdd((unsigned long long*)(sum + L.srow[c]), (unsigned long long)cnt[c]);
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

// the dictionary side's gather: out / out_valid[r] = val / ok[idx[r]] (ok null: every entry has a value)
__global__ void k_str_conv_lookup(const int64_t* __restrict__ val, const uint8_t* __restrict__ ok,
                                  const int64_t* __restrict__ idx, int64_t n, int64_t* __restrict__ out,
                                  uint8_t* __restrict__ out_valid) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = idx[r];
        const bool good = e >= 0 && (ok == nullptr || ok[e]);
        out[r] = good ? val[e] : 0;
        out_valid[r] = good ? 1 : 0;
    }
}

const char* kNoStore = "string function: no string store is registered (capsmi_session_set_strings)";

// val / ok[i] for i < n "rows" whose strings are at idx (null: the store's entries); valid: see k_str_bytes
void conv_pass(capsmi_session* s, int32_t op, const StrStore& S, const int64_t* idx, int64_t n, int64_t* val, uint8_t* ok,
               uint8_t* valid) {
    hipStream_t st = s->stream;
    const int64_t* off = P<int64_t>(S.offsets);
    const uint8_t* bytes = P<uint8_t>(S.bytes);
    // algorithmic bytes of str_conv: per row two offsets (16 B) and, on the rows side, its index word (8 B) read
    // and 9 B written (size: 8 B, its validity byte is written with the lengths); the strings' bytes once each on
    // the dictionary side and for size (the slots); on the rows side of the parsers they depend on the data and
    // are not counted
    const double base = (idx ? 24.0 : 16.0) * (double)n;
    if (op != CAPSMI_X_STR_SIZE) {
        KernelTimer kt(s, "str_conv", base + 9.0 * (double)n + (idx ? 0.0 : (double)S.hoffsets[S.n]));
        auto kern = op == CAPSMI_X_STR_TO_INTEGER ? k_str_conv<CAPSMI_X_STR_TO_INTEGER>
                                                  : (op == CAPSMI_X_STR_TO_FLOAT ? k_str_conv<CAPSMI_X_STR_TO_FLOAT>
                                                                                 : k_str_conv<CAPSMI_X_TO_BOOLEAN>);
        hipLaunchKernelGGL(kern, dim3(grid_for(n)), dim3(256), 0, st, off, bytes, idx, n, val, ok);
        HIP_CHECK(hipGetLastError());
        return;
    }
    Buf len = dev_alloc(sizeof(int64_t) * n, s), flag = dev_alloc(n, s);
    {
        KernelTimer kt(s, "str_conv_starts");
        hipLaunchKernelGGL(k_str_bytes, dim3(grid_for(n)), dim3(256), 0, st, off, idx, n, P<int64_t>(len), P<uint8_t>(flag),
                           valid);
        HIP_CHECK(hipGetLastError());
        fill_i64(val, 0, n, st);
    }
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), n, "str_conv_starts");
    if (tp.m == 0) return;
    KernelTimer kt(s, "str_conv", base + 8.0 * (double)n + (double)tp.m);
    tile_heads(s, tp);
    hipLaunchKernelGGL(k_str_size, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k, P<int64_t>(tp.tk), tp.m,
                       off, bytes, idx, val);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

bool str_conv_fold(capsmi_session* s, int32_t op, int64_t code, int64_t* value) {
    const std::shared_ptr<const StrStore> S = s->strings;
    REQUIRE(S, CAPSMI_ERR_ILLEGAL_ARGUMENT, kNoStore);
    const int64_t i = str_const_index(*S, code);
    const int64_t b = S->hoffsets[i], len = S->hoffsets[i + 1] - b;
    std::vector<uint8_t> str((size_t)len + 1);
    if (len > 0) {
        HIP_CHECK(hipMemcpyAsync(str.data(), P<uint8_t>(S->bytes) + b, len, hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    }
    *value = 0;
    switch (op) {
        case CAPSMI_X_STR_SIZE: *value = strconv::count_code_points(str.data(), len); return true;
        case CAPSMI_X_STR_TO_INTEGER: return strconv::to_integer(str.data(), len, value);
        case CAPSMI_X_STR_TO_FLOAT: {
            uint64_t u = 0;
            const bool good = strconv::to_float(str.data(), len, &u);
            *value = good ? (int64_t)u : 0;
            return good;
        }
        default: {
            const int t = strconv::to_boolean(str.data(), len);
            *value = t > 0 ? 1 : 0;
            return t >= 0;
        }
    }
}

void str_conv(capsmi_session* s, int32_t op, const StrOperand& o, int64_t n, int64_t* out, uint8_t* out_valid) {
    if (n == 0) return;
    REQUIRE(!o.is_const, CAPSMI_ERR_INTERNAL, "string function: a constant is folded on the host");
    const std::shared_ptr<const StrStore> S = s->strings;  // the store registered now, kept while the passes run
    REQUIRE(S, CAPSMI_ERR_ILLEGAL_ARGUMENT, kNoStore);
    hipStream_t st = s->stream;
    Buf err = dev_alloc(sizeof(int64_t), s), idx = dev_alloc(sizeof(int64_t) * n, s);
    fill_i64(P<int64_t>(err), 0, 1, st);
    str_index_rows(s, *S, o, n, P<int64_t>(idx), P<int64_t>(err));
    str_index_check(s, P<int64_t>(err));
    const bool dict = s->cfg.str_match == 2 || (s->cfg.str_match == 0 && n >= S->n);
    if (!dict) {
        conv_pass(s, op, *S, P<int64_t>(idx), n, out, out_valid, out_valid);
        return;
    }
    const bool size = op == CAPSMI_X_STR_SIZE;
    Buf val = dev_alloc(sizeof(int64_t) * S->n, s), ok = size ? Buf() : dev_alloc(S->n, s);
    conv_pass(s, op, *S, nullptr, S->n, P<int64_t>(val), P<uint8_t>(ok), nullptr);
    // algorithmic bytes of the lookup: the index word, a value word and a validity byte read, 9 B written per row
    KernelTimer kt(s, "str_conv_lookup", (size ? 25.0 : 26.0) * (double)n);
    hipLaunchKernelGGL(k_str_conv_lookup, dim3(grid_for(n)), dim3(256), 0, st, P<int64_t>(val), P<uint8_t>(ok), P<int64_t>(idx),
                       n, out, out_valid);
    HIP_CHECK(hipGetLastError());
}

}  // namespace capsmi
