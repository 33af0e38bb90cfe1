// tri_walk.h -- what the tile walks over a single-device TriGraph's base arrays (off, tg, ov, sl, orig) share:
// the transitive triangle (k_tri_trans.hip) and the undirected one (k_tri_und.hip).  Both run a self-term pass,
// a pair-term pass over the oriented edges and a walk over tiles of slots (edge, position in the walked list)
// that finds every simple triangle {u, v, w} once at its edge u -> v; they differ in the weights only, which
// the walk takes as a functor called on a hit.
#pragma once

#include "capsmi_impl.h"
#include "tile_owner.h"
#include "tri_code.h"

namespace capsmi {
namespace tri {

// the privatised window of k_tri_grouped.hip (measured there), with its build-time override
#ifndef CAPSMI_TRI_BY_NODE_WIN
#define CAPSMI_TRI_BY_NODE_WIN 64
#endif
constexpr int kByNodeWin = CAPSMI_TRI_BY_NODE_WIN;
static_assert(kByNodeWin >= 1 && kByNodeWin <= 3072, "the window and the tile's owner arrays share 64 KiB of LDS");

typedef unsigned long long u64;

__device__ __forceinline__ void node_add(u64* win, u64* __restrict__ cnt, uint32_t id, u64 x) {
    if (id < (uint32_t)kByNodeWin) atomicAdd(&win[id], x);
    else atomicAdd(&cnt[id], x);
}

__device__ __forceinline__ void win_flush(const u64* win, u64* __restrict__ cnt, int64_t n) {
    for (int i = threadIdx.x; i < kByNodeWin && i < n; i += blockDim.x)
        if (win[i]) atomicAdd(&cnt[i], win[i]);
}

// the workgroup's sum of x, added to *out by one atomic (every thread calls it; tot: one LDS word, zeroed here)
__device__ __forceinline__ void block_add(u64 x, u64* tot, u64* __restrict__ out) {
    if (threadIdx.x == 0) *tot = 0;
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicAdd(tot, x);
    __syncthreads();
    if (threadIdx.x == 0 && *tot) atomicAdd(out, *tot);
}

inline unsigned egrid(const capsmi_session* s, int64_t n) {
    const int64_t g = (n + 255) / 256, cap = (int64_t)s->num_cus * 16;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// Slot i of a tile_owners tile whose rows are oriented edges e = u -> v with min(od(v), p) slots each (p = e's
// position in out(u)): the slot walks entry j of the shorter of out(v) and out(u)[0, p) and binary-searches the
// other.  Sets c (the slot's tile-local row), u and v; where the entry closes u -> v -> w, calls
// hit(w, puv, pvw, puw) with the three payloads (f << 32 | b of u -> v, v -> w, u -> w).
template <class Hit>
__device__ __forceinline__ void tile_slot(const tiles::TileLds& L, int i, const int64_t* __restrict__ off,
                                          const uint32_t* __restrict__ tg, TgCode tc, const int64_t* __restrict__ ov,
                                          const uint32_t* __restrict__ eu, int& c, uint32_t& u, uint32_t& v, Hit hit) {
    c = L.own[i];
    const int64_t e = L.srow[c], j = L.sbase[c] + i;
    u = eu[e];
    const uint32_t wuv = tg[e];
    v = tid(wuv, tc);
    const int64_t uo = off[u], vo = off[v], odv = off[v + 1] - vo, p = e - uo;
    // walk the shorter of out(v) and out(u)[0, p), search the other
    const bool wlk = odv <= p;
    const int64_t at = (wlk ? vo : uo) + j;
    const uint32_t xw = tg[at], x = tid(xw, tc);
    int64_t a = wlk ? uo : vo;
    const int64_t end = wlk ? e : vo + odv;
    int64_t b = end;
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (tid(tg[mid], tc) < x) a = mid + 1; else b = mid;
    }
    if (a < end) {
        const uint32_t yw = tg[a];
        if (tid(yw, tc) == x) {  // w = x closes u -> v -> w
            const uint64_t puv = tpay(wuv, tc, ov, e);
            const uint64_t pvw = wlk ? tpay(xw, tc, ov, at) : tpay(yw, tc, ov, a);
            const uint64_t puw = wlk ? tpay(yw, tc, ov, a) : tpay(xw, tc, ov, at);
            hit(x, puv, pvw, puw);
        }
    }
}

// per oriented edge e = u -> v at position p of out(u): its source (off is searched: the base arrays keep no
// source column), and its slots, min(od(v), p)  (as k_tbn_edges)
static __global__ void k_ttr_edges(const int64_t* __restrict__ off, const uint32_t* __restrict__ tg, TgCode tc, int64_t n,
                                   int64_t ne, uint32_t* __restrict__ eu, int64_t* __restrict__ len,
                                   uint8_t* __restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t a = 0, b = n + 1;  // the first entry of off[0, n] above e (off[n] = ne is)
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (off[mid] <= e) a = mid + 1; else b = mid;
        }
        const int64_t u = a - 1;
        const uint32_t v = tid(tg[e], tc);
        const int64_t l = min(off[v + 1] - off[v], e - off[u]);
        eu[e] = (uint32_t)u;
        len[e] = l;
        flag[e] = l > 0 ? 1 : 0;
    }
}

static __global__ void k_ttr_flags(const u64* __restrict__ cnt, int64_t n, uint8_t* __restrict__ f) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        f[r] = cnt[r] != 0 ? 1 : 0;
}

// rows (relative id, count) of the nodes with a non-zero counter, in no particular order; returns their number
inline int64_t node_rows(capsmi_session* s, const TriGraph& g, const u64* cp, const char* timer, Buf& ids, Buf& counts) {
    hipStream_t st = s->stream;
    const int64_t n = g.n;
    KernelTimer kt(s, timer);
    Buf f = dev_alloc(n > 0 ? n : 1, s), idx;
    hipLaunchKernelGGL(k_ttr_flags, dim3(egrid(s, n)), dim3(256), 0, st, cp, n, P<uint8_t>(f));
    HIP_CHECK(hipGetLastError());
    const int64_t rows = flags_to_indices(s, P<uint8_t>(f), n, idx);
    ids = dev_alloc(sizeof(int64_t) * (rows > 0 ? rows : 1), s);
    counts = dev_alloc(sizeof(int64_t) * (rows > 0 ? rows : 1), s);
    gather_col(P<int64_t>(g.orig), nullptr, P<int64_t>(idx), rows, P<int64_t>(ids), nullptr, st);
    gather_col(reinterpret_cast<const int64_t*>(cp), nullptr, P<int64_t>(idx), rows, P<int64_t>(counts), nullptr, st);
    return rows;
}

}  // namespace tri
}  // namespace capsmi
