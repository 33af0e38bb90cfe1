// k_strmake.hip -- toString() and string concatenation: strings made on the device
// (SparkSQLExprMapper.scala:233 ToString, cast(StringType); :160-181 Add over a String and a String or Number,
// functions.concat; the rules are stated per opcode in include/capsmi.h, the formatting code is str_make.h).
//
// A String value is a code of a dictionary the caller owns, so a produced string has no code until the caller
// gives it one (the session's string sink).  The host call per string costs far more than a hash pass, and a
// produced string is a function of its operand tuple, so the tuples are deduplicated before anything is formatted:
//   1. distinct tuples (hash_build / hash_group_ids over the operand columns; a row with a NULL operand is skipped
//      and comes out NULL): gid_of_row and one representative row per group.  A STR operand went through the
//      shared k_str_index first, which also finds a code that is not registered.
//   2. lengths (k_make_lengths), one thread per group: the digit count of a Long, 4 or 5 for a Boolean, the offset
//      difference of a String, a constant's length; both parts summed.
//   3. write (k_make_write): an exclusive scan of the lengths lays the output bytes out, and they are written over
//      the fixed tiles of tile_owner.h -- group g owns one slot per byte of its string, a slot knows its group and
//      its position and copies a store byte, a constant's byte, or emits a digit, the sign or a letter of true /
//      false.  One string of a megabyte among short ones costs what the same bytes in uniform strings cost.
//   4. sink: offsets and bytes go to the host, the sink returns one code per group.
//   5. store merge (k_store_merge): the entries whose codes the registered store does not hold are merged into a
//      new store.  Codes and the copy's plan are built on the host; the bytes make no round trip: the merged
//      entries are the rows of one more tile-balanced copy whose sources are the old store's byte array and the
//      buffer of step 3.  Nothing new: nothing is done.
//   6. gather (k_make_gather): row r takes codes[gid[r]].
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "str_make.h"
#include "tile_owner.h"

namespace capsmi {

namespace {

using namespace tiles;

enum { kSideStr = 0, kSideLong = 1, kSideBool = 2, kSideConst = 3 };

// one operand as the kernels see it
struct MakeSide {
    int kind;
    const int64_t* word;  // per row -- a String: its store index (never -1 in a representative row); else the value
    const uint8_t* cst;   // a constant's bytes
    int64_t clen;
};

__device__ __forceinline__ int64_t side_length(const MakeSide& o, const int64_t* __restrict__ off, int64_t r) {
    switch (o.kind) {
        case kSideStr: {
            const int64_t e = o.word[r];
            return off[e + 1] - off[e];
        }
        case kSideLong: return strmake::long_length(o.word[r]);
        case kSideBool: return strmake::bool_length(o.word[r] != 0);
        default: return o.clen;
    }
}

// byte q of the operand's `len` bytes in row r
__device__ __forceinline__ uint8_t side_byte(const MakeSide& o, const int64_t* __restrict__ off,
                                             const uint8_t* __restrict__ bytes, int64_t r, int64_t len, int64_t q) {
    switch (o.kind) {
        case kSideStr: return bytes[off[o.word[r]] + q];
        case kSideLong: return strmake::long_byte(o.word[r], (int)len, (int)q);
        case kSideBool: return strmake::bool_byte(o.word[r] != 0, (int)q);
        default: return o.cst[q];
    }
}

// len[g] = bytes of group g's string, la[g] = those of its first operand, flag[g] = len > 0
__global__ void k_make_lengths(MakeSide A, MakeSide B, int nops, const int64_t* __restrict__ rep, int64_t ng,
                               const int64_t* __restrict__ off, int64_t* __restrict__ len, int64_t* __restrict__ la,
                               uint8_t* __restrict__ flag) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = rep[g];
        const int64_t a = side_length(A, off, r), b = nops > 1 ? side_length(B, off, r) : 0;
        len[g] = a + b;
        la[g] = a;
        flag[g] = a + b > 0 ? 1 : 0;
    }
}

// slot i of a tile is output byte j0 + i: byte L.sbase[c] + i of its group's string
__global__ void __launch_bounds__(kExB) k_make_write(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz,
                                                    int64_t k, const int64_t* __restrict__ tk, int64_t m, MakeSide A,
                                                    MakeSide B, const int64_t* __restrict__ rep,
                                                    const int64_t* __restrict__ len, const int64_t* __restrict__ la,
                                                    const int64_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                    uint8_t* __restrict__ out) {
    __shared__ TileLds L;
    const int t = threadIdx.x;
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [](int64_t) { return (int64_t)0; });
#pragma unroll
        for (int j = 0; j < kExI; ++j) {
            const int i = t + j * kExB;
            if (i < nt) {
                const int c = L.own[i];
                const int64_t g = L.srow[c], p = L.sbase[c] + i;
                const int64_t r = rep[g], a = la[g];
                out[j0 + i] = p < a ? side_byte(A, off, bytes, r, a, p) : side_byte(B, off, bytes, r, len[g] - a, p - a);
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

// The merged store's bytes: entry e's bytes start at src[e] of the old store's byte array followed by the new
// buffer (one address space: a < nold is an old byte, else new byte a - nold).  Slot i of a tile is byte j0 + i.
__global__ void __launch_bounds__(kExB) k_store_merge(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz,
                                                     int64_t k, const int64_t* __restrict__ tk, int64_t m,
                                                     const int64_t* __restrict__ src, const uint8_t* __restrict__ oldb,
                                                     int64_t nold, const uint8_t* __restrict__ newb,
                                                     uint8_t* __restrict__ out) {
    __shared__ TileLds L;
    const int t = threadIdx.x;
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [&](int64_t e) { return src[e]; });
#pragma unroll
        for (int j = 0; j < kExI; ++j) {
            const int i = t + j * kExB;
            if (i < nt) {
                const int64_t a = L.sbase[L.own[i]] + i;
                out[j0 + i] = a < nold ? oldb[a] : newb[a - nold];
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
}

__global__ void k_make_gather(const int64_t* __restrict__ gid, const int64_t* __restrict__ codes, int64_t n,
                              int64_t* __restrict__ out, uint8_t* __restrict__ out_valid) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = gid[r];
        out[r] = g >= 0 ? codes[g] : 0;
        out_valid[r] = g >= 0 ? 1 : 0;
    }
}

const char* kNoStore = "string concatenation: no string store is registered (capsmi_session_set_strings)";

Buf upload(capsmi_session* s, const void* host, size_t bytes) {
    Buf b = dev_alloc(bytes > 0 ? bytes : 1, s);
    if (bytes > 0) HIP_CHECK(hipMemcpyAsync(P<void>(b), host, bytes, hipMemcpyHostToDevice, s->stream));
    return b;
}

// Steps 4 and 5 for n made strings -- string i is hb[ho[i] .. ho[i + 1]) on the host and the same bytes of `newb` on
// the device: the sink's codes into codes[n], what it may not do refused, the new entries merged into the store.
// The session's store is replaced last, so every refusal leaves it as it was.
void intern_and_merge(capsmi_session* s, int64_t n, const int64_t* ho, const char* hb, const uint8_t* newb, int64_t* codes) {
    REQUIRE(s->sink, CAPSMI_ERR_ILLEGAL_ARGUMENT,
            "toString() / string concatenation: no string sink is registered (capsmi_session_set_string_sink)");
    REQUIRE(s->sink(s->sink_ctx, n, ho, hb, codes) == 0, CAPSMI_ERR_ILLEGAL_ARGUMENT,
            "the string sink failed (it returned a non-zero status)");
    auto same = [&](int64_t i, const char* p, int64_t len) {
        return ho[i + 1] - ho[i] == len && (len == 0 || memcmp(hb + ho[i], p, (size_t)len) == 0);
    };
    // The made strings in code order: one string per code (equal codes are neighbours), and for a code the store
    // holds, the store's bytes.  The codes ascend, so the search of the store's codes goes on where it stopped.
    const std::shared_ptr<const StrStore> S = s->strings;
    std::vector<int64_t> order(n);
    for (int64_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return codes[x] != codes[y] ? codes[x] < codes[y] : x < y; });
    std::vector<std::pair<int64_t, int64_t>> fresh;  // (code, made string) of the codes the store lacks, ascending
    size_t at = 0;  // the store's first code that is not below the last one looked up
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = order[k];
        if (k > 0 && codes[order[k - 1]] == codes[i]) {
            const int64_t j = order[k - 1];
            REQUIRE(same(i, hb + ho[j], ho[j + 1] - ho[j]), CAPSMI_ERR_ILLEGAL_ARGUMENT,
                    "the string sink gave two different strings the code " + std::to_string((long long)codes[i]));
            continue;
        }
        if (S) at = std::lower_bound(S->hcodes.begin() + at, S->hcodes.end(), codes[i]) - S->hcodes.begin();
        if (S && at < S->hcodes.size() && S->hcodes[at] == codes[i]) {
            REQUIRE(same(i, S->hbytes.data() + S->hoffsets[at], S->hoffsets[at + 1] - S->hoffsets[at]), CAPSMI_ERR_ILLEGAL_ARGUMENT,
                    "the string sink returned the code " + std::to_string((long long)codes[i]) +
                        ", which the string store holds for other bytes");
        } else {
            fresh.emplace_back(codes[i], i);
        }
    }
    if (fresh.empty()) return;  // the repeated query: nothing to merge
    // the merged entries in code order: codes, lengths, and where the bytes come from
    const int64_t nold = S ? S->n : 0, oldbytes = S ? S->hoffsets[nold] : 0;
    const int64_t nn = nold + (int64_t)fresh.size();
    auto st = std::make_shared<StrStore>();
    st->n = nn;
    st->hcodes.reserve(nn);
    st->hoffsets.reserve(nn + 1);
    st->hoffsets.push_back(0);
    std::vector<int64_t> src(nn), len(nn);
    std::vector<uint8_t> flag(nn);
    int64_t fresh_bytes = 0;
    for (int64_t a = 0, b = 0; a < nold || b < (int64_t)fresh.size();) {
        const bool take_old = b == (int64_t)fresh.size() || (a < nold && S->hcodes[a] < fresh[b].first);
        const int64_t e = (int64_t)st->hcodes.size();
        if (take_old) {
            src[e] = S->hoffsets[a];
            len[e] = S->hoffsets[a + 1] - S->hoffsets[a];
            st->hcodes.push_back(S->hcodes[a]);
            st->hbytes.append(S->hbytes, (size_t)src[e], (size_t)len[e]);
            ++a;
        } else {
            const int64_t i = fresh[b].second;
            src[e] = oldbytes + ho[i];
            len[e] = ho[i + 1] - ho[i];
            fresh_bytes += len[e];
            st->hcodes.push_back(fresh[b].first);
            st->hbytes.append(hb + ho[i], (size_t)len[e]);
            ++b;
        }
        flag[e] = len[e] > 0 ? 1 : 0;
        st->hoffsets.push_back(st->hoffsets.back() + len[e]);
    }
    hipStream_t stream = s->stream;
    st->codes = upload(s, st->hcodes.data(), sizeof(int64_t) * nn);
    Buf dsrc = upload(s, src.data(), sizeof(int64_t) * nn), dlen = upload(s, len.data(), sizeof(int64_t) * nn),
        dflag = upload(s, flag.data(), nn);
    // the plan's scan of the lengths is the new store's offsets array
    const TilePlan tp = tile_plan(s, P<int64_t>(dlen), P<uint8_t>(dflag), nn, "str_store_merge_starts");
    REQUIRE(tp.m == st->hoffsets[nn], CAPSMI_ERR_INTERNAL, "string store merge: the device's byte count differs from the host's");
    st->offsets = tp.starts;
    st->bytes = dev_alloc(tp.m > 0 ? tp.m : 1, s);
    if (tp.m > 0) {
        // algorithmic bytes: the old store's bytes and the new entries' bytes, each read and written once
        KernelTimer kt(s, "str_store_merge", 2.0 * ((double)oldbytes + (double)fresh_bytes));
        tile_heads(s, tp);
        hipLaunchKernelGGL(k_store_merge, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, stream, tp.cs, tp.nz, tp.k,
                           P<int64_t>(tp.tk), tp.m, P<int64_t>(dsrc), S ? P<uint8_t>(S->bytes) : nullptr, oldbytes, newb,
                           P<uint8_t>(st->bytes));
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(stream));  // the host arrays above are free again
    s->strings = std::move(st);
}

}  // namespace

std::string str_const_bytes(capsmi_session* s, int64_t code) {
    const std::shared_ptr<const StrStore> S = s->strings;
    REQUIRE(S, CAPSMI_ERR_ILLEGAL_ARGUMENT, kNoStore);
    const int64_t i = str_const_index(*S, code);
    return S->hbytes.substr((size_t)S->hoffsets[i], (size_t)(S->hoffsets[i + 1] - S->hoffsets[i]));
}

int64_t str_make_fold(capsmi_session* s, const std::string& bytes) {
    const int64_t ho[2] = {0, (int64_t)bytes.size()};
    Buf newb = upload(s, bytes.data(), bytes.size());
    int64_t code = 0;
    intern_and_merge(s, 1, ho, bytes.data(), P<uint8_t>(newb), &code);
    HIP_CHECK(hipStreamSynchronize(s->stream));  // `bytes` was the source of a queued copy
    return code;
}

void str_make(capsmi_session* s, int nops, const MakeOperand* o, int64_t n, int64_t* out, uint8_t* out_valid) {
    if (n == 0) return;
    REQUIRE(nops == 1 || nops == 2, CAPSMI_ERR_INTERNAL, "string make: one or two operands");
    hipStream_t st = s->stream;
    std::shared_ptr<const StrStore> S = s->strings;  // the store registered now, kept while the passes run
    MakeSide side[2] = {{kSideConst, nullptr, nullptr, 0}, {kSideConst, nullptr, nullptr, 0}};
    Buf idx[2], cst[2], err;
    KeyCols keys;
    keys.n = 0;
    int nstr = 0, nlong = 0;
    for (int q = 0; q < nops; ++q)  // before anything is queued
        REQUIRE(S || o[q].is_const || o[q].type != CAPSMI_STR, CAPSMI_ERR_ILLEGAL_ARGUMENT, kNoStore);
    for (int q = 0; q < nops; ++q) {
        if (o[q].is_const) {
            cst[q] = upload(s, o[q].bytes.data(), o[q].bytes.size());
            side[q] = MakeSide{kSideConst, nullptr, P<uint8_t>(cst[q]), (int64_t)o[q].bytes.size()};
            continue;
        }
        keys.data[keys.n] = o[q].data;
        keys.valid[keys.n] = o[q].valid;
        ++keys.n;
        if (o[q].type != CAPSMI_STR) {
            side[q] = MakeSide{o[q].type == CAPSMI_BOOL ? kSideBool : kSideLong, o[q].data, nullptr, 0};
            ++nlong;
            continue;
        }
        if (!err) {
            err = dev_alloc(sizeof(int64_t), s);
            fill_i64(P<int64_t>(err), 0, 1, st);
        }
        idx[q] = dev_alloc(sizeof(int64_t) * n, s);
        StrOperand so;
        so.data = o[q].data;
        so.valid = o[q].valid;
        str_index_rows(s, *S, so, n, P<int64_t>(idx[q]), P<int64_t>(err));
        side[q] = MakeSide{kSideStr, P<int64_t>(idx[q]), nullptr, 0};
        ++nstr;
    }
    REQUIRE(keys.n > 0, CAPSMI_ERR_INTERNAL, "string make: constants are folded on the host");
    if (err) str_index_check(s, P<int64_t>(err));
    // 1. the distinct operand tuples
    HashTable ht;
    Buf slot_of_row, gid, rep;
    hash_build(s, keys, n, true, ht, slot_of_row);
    const int64_t ng = hash_group_ids(s, ht, slot_of_row, n, gid, rep);
    if (ng == 0) {  // every row has a NULL operand: nothing to make
        fill_i64(out, 0, n, st);
        fill_u8(out_valid, 0, n, st);
        return;
    }
    // 2. lengths
    const int64_t* off = S ? P<int64_t>(S->offsets) : nullptr;
    const uint8_t* bytes = S ? P<uint8_t>(S->bytes) : nullptr;
    Buf len = dev_alloc(sizeof(int64_t) * ng, s), la = dev_alloc(sizeof(int64_t) * ng, s), flag = dev_alloc(ng, s);
    {
        KernelTimer kt(s, "str_make_lengths");
        hipLaunchKernelGGL(k_make_lengths, dim3(grid_for(ng)), dim3(256), 0, st, side[0], side[1], nops, P<int64_t>(rep), ng, off,
                           P<int64_t>(len), P<int64_t>(la), P<uint8_t>(flag));
        HIP_CHECK(hipGetLastError());
    }
    // 3. write
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), ng, "str_make_starts");
    Buf outb = dev_alloc(tp.m > 0 ? tp.m : 1, s);
    if (tp.m > 0) {
        // algorithmic bytes: the output bytes written once, two offsets per STR operand and group, 8 B per Long
        // (or Boolean) operand and group
        KernelTimer kt(s, "str_make", (double)tp.m + (16.0 * nstr + 8.0 * nlong) * (double)ng);
        tile_heads(s, tp);
        hipLaunchKernelGGL(k_make_write, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k, P<int64_t>(tp.tk),
                           tp.m, side[0], side[1], P<int64_t>(rep), P<int64_t>(len), P<int64_t>(la), off, bytes,
                           P<uint8_t>(outb));
        HIP_CHECK(hipGetLastError());
    }
    // 4. and 5. the sink and the merge
    std::vector<int64_t> ho(ng + 1), codes(ng);
    std::vector<char> hb(tp.m > 0 ? tp.m : 1);
    HIP_CHECK(hipMemcpyAsync(ho.data(), P<int64_t>(tp.starts), sizeof(int64_t) * (ng + 1), hipMemcpyDeviceToHost, st));
    if (tp.m > 0) HIP_CHECK(hipMemcpyAsync(hb.data(), P<uint8_t>(outb), tp.m, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    intern_and_merge(s, ng, ho.data(), hb.data(), P<uint8_t>(outb), codes.data());
    // 6. gather
    Buf dcodes = upload(s, codes.data(), sizeof(int64_t) * ng);
    {
        KernelTimer kt(s, "str_make_gather", 17.0 * (double)n);
        hipLaunchKernelGGL(k_make_gather, dim3(grid_for(n)), dim3(256), 0, st, P<int64_t>(gid), P<int64_t>(dcodes), n, out, out_valid);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(st));  // `codes` was the source of a queued copy
}

}  // namespace capsmi
