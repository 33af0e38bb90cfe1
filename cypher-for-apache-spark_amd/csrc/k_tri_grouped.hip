// k_tri_grouped.hip -- the cyclic triangle grouped by its start (route "triangle_grouped").
//
//   MATCH (a)-[r1]->(b)-[r2]->(c)-[r3]->(a) WHERE n_ok(a), n_ok(b), n_ok(c) RETURN id(a), count(*)
//
// With m(x,y) the multiplicity of x->y (x != y), s(x) the self-loops at x and W(u,v,w) = tri_weight, the
// bindings that start at x are (DESIGN.md "grouped triangle"; restated in tests/tri_grouped_ref.py)
//   count(x) = sum over simple triangles {u,v,w} containing x of W(u,v,w)
//            + sum over y != x of m(x,y) m(y,x) (2 s(x) + s(y))
//            + s(x) (s(x)-1) (s(x)-2)
// and the same numbers group the pattern by b or by c (rotation).  A walk over a single-device TriGraph's base
// arrays (off, tg, ov, sl, orig) fills one 64-bit counter per degree-order id:
//   self terms   one pass over the vertices (which also brings sl into degree-order ids);
//   pair terms   one pass over the oriented edges: each undirected pair is one oriented edge with both
//                multiplicities;
//   triangles    every simple triangle {u,v,w}, u -> v -> w in the orientation (w < v < u as degree-order ids),
//                is found once, at its edge u -> v (position p of out(u)): w is common to out(v) and to
//                out(u)[0, p).  The edge owns min(od(v), p) slots: it walks the shorter of the two lists, one
//                entry per slot, and binary-searches the other (both are sorted by id).  The slots of all edges
//                are cut into fixed tiles of kExplodeTile (tile_owner.h), so a workgroup's work does not depend
//                on the degree distribution and a hub's wedges spread over as many tiles as they fill.
// A hit adds its weight to all three corners.  The slots of one edge are consecutive lanes, so the adds to u
// and v are summed per (wave, edge) first.  The adds to w -- the highest-degree corner, i.e. the lowest ids --
// and every other add to an id below kByNodeWin go to a per-workgroup LDS window of 64-bit counters that is
// flushed once at the kernel's end; the rest are 64-bit global atomics on counters that few slots share.
#include <algorithm>

#include "capsmi_impl.h"
#include "tile_owner.h"
#include "tri_code.h"

namespace capsmi {
namespace tri {
namespace {

using namespace tiles;

// The privatised window: the counters of degree-order ids [0, kByNodeWin).  Measured at C4:
// 64 ids 1136 ms, 512 ids 1258 ms, 2048 ids 1251 ms -- the window's 8 B per id come out of the LDS that the tile's
// 36 KiB of owner arrays leave, and at 64 ids four workgroups fit a CU where 512 and more leave three.  (At scale
// 20 the order turns: 62 ms with 64 ids against 30 ms with 2048.)  Mirrored in
// tests/tri_grouped_ref.py.  (CAPSMI_TRI_BY_NODE_WIN: the build-time override those measurements used.)
#ifndef CAPSMI_TRI_BY_NODE_WIN
#define CAPSMI_TRI_BY_NODE_WIN 64
#endif
constexpr int kByNodeWin = CAPSMI_TRI_BY_NODE_WIN;
static_assert(kByNodeWin >= 1 && kByNodeWin <= 3072, "the window and the tile's owner arrays share 64 KiB of LDS");

__device__ __forceinline__ void node_add(unsigned long long* win, unsigned long long* __restrict__ cnt, uint32_t id,
                                         unsigned long long x) {
    if (id < (uint32_t)kByNodeWin) atomicAdd(&win[id], x);
    else atomicAdd(&cnt[id], x);
}

__device__ __forceinline__ void win_flush(const unsigned long long* win, unsigned long long* __restrict__ cnt, int64_t n) {
    for (int i = threadIdx.x; i < kByNodeWin && i < n; i += blockDim.x)
        if (win[i]) atomicAdd(&cnt[i], win[i]);
}

inline unsigned egrid(const capsmi_session* s, int64_t n) {
    const int64_t g = (n + 255) / 256, cap = (int64_t)s->num_cus * 16;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

// self terms (every counter is written: no memset), and the self-loop counts in degree-order ids (the sorted
// build keeps sl by relative id: rel != 0)
__global__ void k_tbn_self(const uint32_t* __restrict__ sl, const int64_t* __restrict__ orig, int rel, int64_t n,
                           uint32_t* __restrict__ sd, unsigned long long* __restrict__ cnt) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t x = sl[rel ? orig[r] : r];
        sd[r] = (uint32_t)x;
        cnt[r] = x >= 3 ? x * (x - 1) * (x - 2) : 0;
    }
}

// per oriented edge e = u -> v at position p of out(u): its source (off is searched: the base arrays keep no
// source column), and its slots, min(od(v), p)
__global__ void k_tbn_edges(const int64_t* __restrict__ off, const uint32_t* __restrict__ tg, TgCode tc, int64_t n,
                            int64_t ne, uint32_t* __restrict__ eu, int64_t* __restrict__ len, uint8_t* __restrict__ flag) {
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

// pair terms: the pair {u, v} with f = m(u,v), b = m(v,u) both present gives f b (2 s(x) + s(y)) to x = u, v
__global__ void __launch_bounds__(256) k_tbn_pairs(const uint32_t* __restrict__ tg, TgCode tc,
                                                   const int64_t* __restrict__ ov, const uint32_t* __restrict__ eu,
                                                   const uint32_t* __restrict__ sd, int64_t n, int64_t ne,
                                                   unsigned long long* __restrict__ cnt) {
    __shared__ unsigned long long win[kByNodeWin];
    for (int i = threadIdx.x; i < kByNodeWin; i += blockDim.x) win[i] = 0;
    __syncthreads();
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t word = tg[e];
        const uint64_t pay = tpay(word, tc, ov, e);
        const uint64_t f = pay >> 32, b = pay & 0xffffffffULL;
        if (f == 0 || b == 0) continue;  // one direction only: no term, no gathers
        const uint32_t u = eu[e], v = tid(word, tc);
        const uint64_t su = sd[u], sv = sd[v];
        if ((su | sv) == 0) continue;
        node_add(win, cnt, u, f * b * (2 * su + sv));
        node_add(win, cnt, v, f * b * (2 * sv + su));
    }
    __syncthreads();
    win_flush(win, cnt, n);
}

// the triangles: tiles of slots (edge, position in the walked list); see the file comment
__global__ void __launch_bounds__(kExB) k_tbn_walk(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                  const int64_t* __restrict__ tk, int64_t m,
                                                  const int64_t* __restrict__ off, const uint32_t* __restrict__ tg,
                                                  TgCode tc, const int64_t* __restrict__ ov,
                                                  const uint32_t* __restrict__ eu, int64_t n,
                                                  unsigned long long* __restrict__ cnt) {
    __shared__ TileLds L;
    __shared__ unsigned long long win[kByNodeWin];
    const int t = threadIdx.x, lane = t & 63;
    for (int i = t; i < kByNodeWin; i += kExB) win[i] = 0;
    __syncthreads();
    const int64_t ntiles = (m + kExplodeTile - 1) / kExplodeTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // block-uniform
        const int64_t j0 = tile * kExplodeTile;
        const int nt = (int)min((int64_t)kExplodeTile, m - j0);
        tile_owners(L, cs, nz, k, tk[tile], j0, nt, [](int64_t) { return (int64_t)0; });  // sbase + i = position
#pragma unroll 1
        for (int q = 0; q < kExI; ++q) {  // wave-uniform: every lane takes part in the shuffles below
            const int i = t + q * kExB;
            int c = -1;
            uint32_t u = 0, v = 0;
            unsigned long long wt = 0;
            if (i < nt) {
                c = L.own[i];
                const int64_t e = L.srow[c], j = L.sbase[c] + i;
                u = eu[e];
                const uint32_t wuv = tg[e];
                v = tid(wuv, tc);
                const int64_t uo = off[u], vo = off[v], odv = off[v + 1] - vo, p = e - uo;
                // walk the shorter of out(v) and out(u)[0, p), search the other
                const bool wv = odv <= p;
                const int64_t at = (wv ? vo : uo) + j;
                const uint32_t xw = tg[at], x = tid(xw, tc);
                int64_t a = wv ? uo : vo;
                const int64_t end = wv ? e : vo + odv;
                int64_t b = end;
                while (a < b) {
                    const int64_t mid = (a + b) >> 1;
                    if (tid(tg[mid], tc) < x) a = mid + 1; else b = mid;
                }
                if (a < end) {
                    const uint32_t yw = tg[a];
                    if (tid(yw, tc) == x) {  // w = x closes u -> v -> w
                        const uint64_t puv = tpay(wuv, tc, ov, e);
                        const uint64_t pvw = wv ? tpay(xw, tc, ov, at) : tpay(yw, tc, ov, a);
                        const uint64_t puw = wv ? tpay(yw, tc, ov, a) : tpay(xw, tc, ov, at);
                        wt = tri_weight(puv, pvw, puw);
                        if (wt) node_add(win, cnt, x, wt);
                    }
                }
            }
            if (__ballot(wt != 0) == 0) continue;  // wave-uniform
            // the lanes of one edge are contiguous: their sum at the edge's first lane, one add each to u and v
            unsigned long long sum = wt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long y = __shfl_down(sum, o, 64);
                const int cy = __shfl_down(c, o, 64);
                if (lane + o < 64 && cy == c) sum += y;
            }
            const int cp = __shfl_up(c, 1, 64);
            if ((lane == 0 || cp != c) && sum) {
                node_add(win, cnt, u, sum);
                node_add(win, cnt, v, sum);
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
    __syncthreads();
    win_flush(win, cnt, n);
}

__global__ void k_tbn_flags(const unsigned long long* __restrict__ cnt, int64_t n, uint8_t* __restrict__ f) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        f[r] = cnt[r] != 0 ? 1 : 0;
}

}  // namespace
}  // namespace tri

// rows (relative id, count) of the nodes with a non-zero count, in no particular order; returns their number
int64_t tri_count_by_node(capsmi_session* s, const TriGraph& g, Buf& ids, Buf& counts) {
    using namespace tri;
    REQUIRE(!g.dist, CAPSMI_ERR_UNSUPPORTED, "triangle counts per node: not over a distributed trigraph");
    hipStream_t st = s->stream;
    const int64_t n = g.n, ne = g.ne;
    const TgCode tc{(uint32_t)g.ib, (uint32_t)g.cb};
    Buf cnt = dev_alloc(sizeof(unsigned long long) * n, s);
    unsigned long long* cp = P<unsigned long long>(cnt);
    {
        Buf sd = dev_alloc(sizeof(uint32_t) * n, s);
        Buf eu, len, flag;
        {
            KernelTimer kt(s, "tri_by_node_terms");
            hipLaunchKernelGGL(k_tbn_self, dim3(egrid(s, n)), dim3(256), 0, st, P<uint32_t>(g.sl), P<int64_t>(g.orig),
                               g.sl_relative ? 1 : 0, n, P<uint32_t>(sd), cp);
            if (ne > 0) {
                eu = dev_alloc(sizeof(uint32_t) * ne, s);
                len = dev_alloc(sizeof(int64_t) * ne, s);
                flag = dev_alloc(ne, s);
                hipLaunchKernelGGL(k_tbn_edges, dim3(egrid(s, ne)), dim3(256), 0, st, P<int64_t>(g.off), P<uint32_t>(g.tg),
                                   tc, n, ne, P<uint32_t>(eu), P<int64_t>(len), P<uint8_t>(flag));
                hipLaunchKernelGGL(k_tbn_pairs, dim3(std::min(egrid(s, ne), (unsigned)(4 * s->num_cus))), dim3(256), 0, st,
                                   P<uint32_t>(g.tg), tc, P<int64_t>(g.ov), P<uint32_t>(eu), P<uint32_t>(sd), n, ne, cp);
            }
            HIP_CHECK(hipGetLastError());
        }
        if (ne > 0) {
            const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), ne, "tri_by_node_plan");
            len.reset();
            flag.reset();
            if (tp.m > 0) {
                KernelTimer kt(s, "triangles_by_node");
                tile_heads(s, tp);
                hipLaunchKernelGGL(k_tbn_walk, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k,
                                   P<int64_t>(tp.tk), tp.m, P<int64_t>(g.off), P<uint32_t>(g.tg), tc, P<int64_t>(g.ov),
                                   P<uint32_t>(eu), n, cp);
                HIP_CHECK(hipGetLastError());
            }
        }
    }
    KernelTimer kt(s, "tri_by_node_rows");
    Buf f = dev_alloc(n, s), idx;
    hipLaunchKernelGGL(k_tbn_flags, dim3(egrid(s, n)), dim3(256), 0, st, cp, n, P<uint8_t>(f));
    HIP_CHECK(hipGetLastError());
    const int64_t rows = flags_to_indices(s, P<uint8_t>(f), n, idx);
    ids = dev_alloc(sizeof(int64_t) * (rows > 0 ? rows : 1), s);
    counts = dev_alloc(sizeof(int64_t) * (rows > 0 ? rows : 1), s);
    gather_col(P<int64_t>(g.orig), nullptr, P<int64_t>(idx), rows, P<int64_t>(ids), nullptr, st);
    gather_col(reinterpret_cast<const int64_t*>(cp), nullptr, P<int64_t>(idx), rows, P<int64_t>(counts), nullptr, st);
    return rows;
}

}  // namespace capsmi
