// k_strmatch.hip -- STARTS WITH, ENDS WITH and CONTAINS over dictionary-coded strings
// (SparkSQLExprMapper.scala:152-157, Column.startsWith / endsWith / contains; Spark's UTF8String matches bytes).
//
// A String value is a code; the bytes live in the session's string store (capsmi_session_set_strings): sorted
// codes, offsets and one byte array.  A match runs in three steps:
//   1. index (k_str_index): one thread per row finds its operand's code in the sorted codes by binary search and
//      writes the entry's index, -1 for a null row; a code that is absent raises a flag (an ordinary store, read
//      back after the pass) and gets -1 too, so nothing below reads outside the store.  A constant operand is
//      resolved on the host.
//   2. match, into one hit byte per "row":
//      STARTS / ENDS WITH (k_str_affix): one thread per row compares plen bytes at 0 or at hlen - plen.
//      CONTAINS: row r owns max(0, hlen - plen + 1) candidate slots, one per start position (none for a null row
//      or an empty pattern, which k_str_slots answers at once).  The slots run over the fixed tiles of
//      tile_owner.h, so one string of a megabyte among a million short ones costs what the same bytes in uniform
//      strings cost; neighbouring slots read neighbouring bytes.  A slot that matches stores 1 into hit[row] --
//      a plain byte store, every writer writes the same value (the convention of k_list_contains).
//   3. finish (k_str_finish): NULL when an operand is NULL, else the hit byte.
// A constant pattern is staged in LDS once per block (up to kPatLds bytes; a longer one is read like a row's).
// Dictionary side: with a constant pattern and a column haystack, step 2 can run over the store's entries instead of
// over the rows (entry e is "row" e), and step 3 gathers hit[idx[r]] (timer str_match_lookup).
#include <algorithm>
#include <string>

#include "tile_owner.h"

namespace capsmi {

namespace {

using namespace tiles;

constexpr int kPatLds = 256;
constexpr int64_t kRowIsEntry = -2;

// where a row's string is: idx[r] (a store index, -1 for a null row), or for every row the constant cst (a store
// index), or the row's own number (kRowIsEntry: the rows are the store's entries)
struct StrSide {
    const int64_t* idx;
    int64_t cst;
};

__device__ __forceinline__ int64_t entry_of(const StrSide& o, int64_t r) {
    return o.idx ? o.idx[r] : (o.cst == kRowIsEntry ? r : o.cst);
}

__global__ void k_str_index(const int64_t* __restrict__ codes, int64_t ns, const int64_t* __restrict__ word,
                            const uint8_t* __restrict__ valid, int64_t n, int64_t* __restrict__ idx,
                            int64_t* __restrict__ err) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t i = -1;
        if (valid == nullptr || valid[r]) {
            const int64_t c = word[r];
            int64_t lo = 0, hi = ns;  // the first entry whose code is >= c
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (codes[mid] < c) lo = mid + 1;
                else hi = mid;
            }
            if (lo < ns && codes[lo] == c) i = lo;
            else err[0] = 1;
        }
        idx[r] = i;
    }
}

// the constant pattern's bytes into LDS (cplen < 0: there is none); every thread of the block calls it
__device__ __forceinline__ void stage_pattern(uint8_t* sp, const uint8_t* __restrict__ cpat, int cplen) {
    for (int i = threadIdx.x; i < cplen; i += blockDim.x) sp[i] = cpat[i];
    __syncthreads();
}

// whether the plen bytes at a equal the pattern: the staged one (cplen >= 0), else the bytes at b
__device__ __forceinline__ bool same_bytes(const uint8_t* __restrict__ a, const uint8_t* sp, int cplen,
                                           const uint8_t* __restrict__ b, int64_t plen) {
    int64_t q = 0;
    if (cplen >= 0) {
        while (q < plen && a[q] == sp[q]) ++q;
    } else {
        while (q < plen && a[q] == b[q]) ++q;
    }
    return q == plen;
}

template <bool ENDS>
__global__ void __launch_bounds__(256) k_str_affix(const int64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                   StrSide H, StrSide Pt, const uint8_t* __restrict__ cpat, int cplen,
                                                   int64_t n, uint8_t* __restrict__ hit) {
    __shared__ uint8_t sp[kPatLds];
    stage_pattern(sp, cpat, cplen);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t hi = entry_of(H, r), pi = entry_of(Pt, r);
        bool res = false;
        if (hi >= 0 && pi >= 0) {
            const int64_t hb = off[hi], hlen = off[hi + 1] - hb;
            int64_t pb = 0, plen = cplen;
            if (cplen < 0) {
                pb = off[pi];
                plen = off[pi + 1] - pb;
            }
            if (plen <= hlen) res = same_bytes(bytes + hb + (ENDS ? hlen - plen : 0), sp, cplen, bytes + pb, plen);
        }
        hit[r] = res ? 1 : 0;
    }
}

// CONTAINS: len[r] = candidate slots of row r, flag[r] = len > 0; hit[r] = 1 at once for an empty pattern
__global__ void k_str_slots(const int64_t* __restrict__ off, StrSide H, StrSide Pt, int64_t n, int64_t* __restrict__ len,
                            uint8_t* __restrict__ flag, uint8_t* __restrict__ hit) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t hi = entry_of(H, r), pi = entry_of(Pt, r);
        int64_t l = 0;
        bool h = false;
        if (hi >= 0 && pi >= 0) {
            const int64_t hlen = off[hi + 1] - off[hi], plen = off[pi + 1] - off[pi];
            if (plen == 0) h = true;
            else if (plen <= hlen) l = hlen - plen + 1;
        }
        len[r] = l;
        flag[r] = l > 0 ? 1 : 0;
        hit[r] = h ? 1 : 0;
    }
}

// slot i of a tile: start position L.sbase[c] + i of the byte array (base_of = the haystack's first byte); the
// slot's last byte lies inside its haystack because the row owns hlen - plen + 1 slots
__global__ void __launch_bounds__(kExB) k_str_contains(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz,
                                                      int64_t k, const int64_t* __restrict__ tk, int64_t m,
                                                      const int64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                      StrSide H, StrSide Pt, const uint8_t* __restrict__ cpat, int cplen,
                                                      uint8_t* __restrict__ hit) {
    __shared__ TileLds L;
    __shared__ uint8_t sp[kPatLds];
    stage_pattern(sp, cpat, cplen);
    const int t = threadIdx.x;
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [&](int64_t r) { return off[entry_of(H, r)]; });
#pragma unroll
        for (int j = 0; j < kExI; ++j) {
            const int i = t + j * kExB;
            if (i < nt) {
                const int c = L.own[i];
                const int64_t r = L.srow[c];
                int64_t pb = 0, plen = cplen;
                if (cplen < 0) {
                    const int64_t pi = entry_of(Pt, r);
                    pb = off[pi];
                    plen = off[pi + 1] - pb;
                }
                if (same_bytes(bytes + L.sbase[c] + i, sp, cplen, bytes + pb, plen)) hit[r] = 1;
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

// out / out_valid[r]: NULL when an operand is NULL, else hit[r], or hit[the haystack's entry] with `gather`
__global__ void k_str_finish(const uint8_t* __restrict__ hit, StrSide H, StrSide Pt, bool gather, int64_t n,
                             int64_t* __restrict__ out, uint8_t* __restrict__ out_valid) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t hi = entry_of(H, r), pi = entry_of(Pt, r);
        const bool ok = hi >= 0 && pi >= 0;
        out[r] = ok && hit[gather ? hi : r] ? 1 : 0;
        out_valid[r] = ok ? 1 : 0;
    }
}

const char* kNoStore = "string match: no string store is registered (capsmi_session_set_strings)";

// hit[i] for i < n "rows" whose strings are at H and Pt; columns: the index arrays among them
void match_pass(capsmi_session* s, int32_t op, const StrStore& S, const StrSide& H, const StrSide& Pt, int64_t n,
                uint8_t* hit) {
    hipStream_t st = s->stream;
    const int64_t* off = P<int64_t>(S.offsets);
    const uint8_t* bytes = P<uint8_t>(S.bytes);
    const uint8_t* cpat = nullptr;
    int cplen = -1;
    double pat_bytes = 0;
    if (!Pt.idx && Pt.cst >= 0) {
        const int64_t pb = S.hoffsets[Pt.cst], plen = S.hoffsets[Pt.cst + 1] - pb;
        pat_bytes = (double)plen;
        if (plen <= kPatLds) {
            cpat = bytes + pb;
            cplen = (int)plen;
        }
    }
    // algorithmic bytes of str_match: an 8-byte index word per row and column operand, two offsets (16 B) per row
    // and operand that is not constant, a constant pattern's bytes once, and for CONTAINS one byte per candidate
    // slot (each start position is read at least once; the plen - 1 bytes behind a row's last slot, a column
    // pattern's bytes and what STARTS / ENDS WITH compare depend on the data and are not counted)
    const int ncol = (H.idx ? 1 : 0) + (Pt.idx ? 1 : 0);
    const int nvar = (H.idx || H.cst == kRowIsEntry ? 1 : 0) + (Pt.idx ? 1 : 0);
    const double base = (8.0 * ncol + 16.0 * nvar) * (double)n + pat_bytes;
    if (op != CAPSMI_X_CONTAINS) {
        KernelTimer kt(s, "str_match", base);
        auto kern = op == CAPSMI_X_ENDS_WITH ? k_str_affix<true> : k_str_affix<false>;
        hipLaunchKernelGGL(kern, dim3(grid_for(n)), dim3(256), 0, st, off, bytes, H, Pt, cpat, cplen, n, hit);
        HIP_CHECK(hipGetLastError());
        return;
    }
    Buf len = dev_alloc(sizeof(int64_t) * n, s), flag = dev_alloc(n, s);
    {
        KernelTimer kt(s, "str_match_starts");
        hipLaunchKernelGGL(k_str_slots, dim3(grid_for(n)), dim3(256), 0, st, off, H, Pt, n, P<int64_t>(len), P<uint8_t>(flag),
                           hit);
        HIP_CHECK(hipGetLastError());
    }
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), n, "str_match_starts");
    if (tp.m == 0) return;
    KernelTimer kt(s, "str_match", base + (double)tp.m);
    tile_heads(s, tp);
    hipLaunchKernelGGL(k_str_contains, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k, P<int64_t>(tp.tk),
                       tp.m, off, bytes, H, Pt, cpat, cplen, hit);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

int64_t str_const_index(const StrStore& S, int64_t code) {
    const auto it = std::lower_bound(S.hcodes.begin(), S.hcodes.end(), code);
    REQUIRE(it != S.hcodes.end() && *it == code, CAPSMI_ERR_ILLEGAL_ARGUMENT,
            "string match: the code " + std::to_string((long long)code) +
                " of a constant operand is not registered in the session's string store (capsmi_session_set_strings)");
    return it - S.hcodes.begin();
}

void str_index_rows(capsmi_session* s, const StrStore& S, const StrOperand& o, int64_t n, int64_t* idx, int64_t* err) {
    // algorithmic bytes: the row's word (and validity byte) read, its index written, the codes it searches
    KernelTimer kt(s, "str_index", (16.0 + (o.valid ? 1.0 : 0.0)) * (double)n + 8.0 * (double)S.n);
    hipLaunchKernelGGL(k_str_index, dim3(grid_for(n)), dim3(256), 0, s->stream, P<int64_t>(S.codes), S.n, o.data, o.valid, n,
                       idx, err);
    HIP_CHECK(hipGetLastError());
}

void str_index_check(capsmi_session* s, const int64_t* err) {
    REQUIRE(read_scalar(s, err) == 0, CAPSMI_ERR_ILLEGAL_ARGUMENT,
            "string match: a String value's code is not registered in the session's string store "
            "(capsmi_session_set_strings)");
}

bool str_match_fold(capsmi_session* s, int32_t op, int64_t hcode, int64_t pcode) {
    const std::shared_ptr<const StrStore> S = s->strings;
    REQUIRE(S, CAPSMI_ERR_ILLEGAL_ARGUMENT, kNoStore);
    std::string str[2];
    const int64_t code[2] = {hcode, pcode};
    for (int q = 0; q < 2; ++q) {
        const int64_t i = str_const_index(*S, code[q]);
        const int64_t b = S->hoffsets[i], len = S->hoffsets[i + 1] - b;
        str[q].resize(len);
        if (len > 0)
            HIP_CHECK(hipMemcpyAsync(&str[q][0], P<uint8_t>(S->bytes) + b, len, hipMemcpyDeviceToHost, s->stream));
    }
    HIP_CHECK(hipStreamSynchronize(s->stream));
    const std::string &h = str[0], &p = str[1];
    if (p.size() > h.size()) return false;
    if (op == CAPSMI_X_STARTS_WITH) return h.compare(0, p.size(), p) == 0;
    if (op == CAPSMI_X_ENDS_WITH) return h.compare(h.size() - p.size(), p.size(), p) == 0;
    return h.find(p) != std::string::npos;
}

void str_match(capsmi_session* s, int32_t op, const StrOperand& h, const StrOperand& p, int64_t n, int64_t* out,
               uint8_t* out_valid) {
    if (n == 0) return;
    REQUIRE(!(h.is_const && p.is_const), CAPSMI_ERR_INTERNAL, "string match: two constants are folded on the host");
    const std::shared_ptr<const StrStore> S = s->strings;  // the store registered now, kept while the pass runs
    REQUIRE(S, CAPSMI_ERR_ILLEGAL_ARGUMENT, kNoStore);
    hipStream_t st = s->stream;
    StrSide side[2];
    Buf idx[2], err;
    const StrOperand* opd[2] = {&h, &p};
    for (int q = 0; q < 2; ++q) {
        if (opd[q]->is_const) {
            side[q] = StrSide{nullptr, str_const_index(*S, opd[q]->code)};
            continue;
        }
        if (!err) {
            err = dev_alloc(sizeof(int64_t), s);
            fill_i64(P<int64_t>(err), 0, 1, st);
        }
        idx[q] = dev_alloc(sizeof(int64_t) * n, s);
        str_index_rows(s, *S, *opd[q], n, P<int64_t>(idx[q]), P<int64_t>(err));
        side[q] = StrSide{P<int64_t>(idx[q]), 0};
    }
    if (err) str_index_check(s, P<int64_t>(err));
    // the dictionary side: a constant pattern is matched once per store entry and the rows look their entry up
    const bool can_dict = p.is_const && !h.is_const;
    const bool dict = can_dict && (s->cfg.str_match == 2 || (s->cfg.str_match == 0 && n >= S->n));
    const int64_t rows = dict ? S->n : n;
    Buf hit = dev_alloc(rows, s);
    match_pass(s, op, *S, dict ? StrSide{nullptr, kRowIsEntry} : side[0], side[1], rows, P<uint8_t>(hit));
    // algorithmic bytes of the lookup: the index word and a hit byte read, 9 B written per row
    KernelTimer kt(s, dict ? "str_match_lookup" : "str_match_finish", dict ? 18.0 * (double)n : 0.0);
    hipLaunchKernelGGL(k_str_finish, dim3(grid_for(n)), dim3(256), 0, st, P<uint8_t>(hit), side[0], side[1], dict, n, out,
                       out_valid);
    HIP_CHECK(hipGetLastError());
}

}  // namespace capsmi
