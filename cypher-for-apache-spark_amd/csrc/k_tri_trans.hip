// k_tri_trans.hip -- the transitive ("feed-forward") triangle (routes "triangle_transitive" and
// "triangle_transitive_grouped").
//
//   MATCH (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a) WHERE n_ok(a), n_ok(b), n_ok(c) RETURN count(*)
//   ... RETURN id(a), count(*)      (or id(b), or id(c))
//
// r1, r2, r3 are pairwise distinct; a, b, c may coincide.  With m(x,y) the multiplicity of x->y (x != y), s(x)
// the self-loops at x and M(y,z) = m(y,z) + m(z,y), the bindings are (DESIGN.md "transitive triangle"; restated
// in tests/tri_trans_ref.py)
//   three distinct nodes   m(a,b) m(b,c) m(a,c).  Node x of the simple triangle {x,y,z} receives
//                            as source a   m(x,y) m(x,z) M(y,z)
//                            as sink c     m(y,x) m(z,x) M(y,z)
//                            as middle b   m(y,x) m(x,z) m(y,z) + m(z,x) m(x,y) m(z,y)
//   a = b = x, c = y       s(x) m(x,y) (m(x,y)-1)      (r1 is a loop)
//   b = c = y, a = x       m(x,y) (m(x,y)-1) s(y)      (r2 is a loop)
//   a = c = x, b = y       m(x,y) m(y,x) s(x)          (r3 is a loop)
//   a = b = c = x          s(x) (s(x)-1) (s(x)-2)
// Unlike the cycle the pattern is not symmetric under rotation: the three positions are three roles, each with
// its own per-node count (a count grouped by a role credits every term to the node in that role), and a pair
// with relationships in one direction only has pair terms (m (m-1)).  The passes are those of k_tri_grouped.hip
// over a single-device TriGraph's base arrays (off, tg, ov, sl, orig) -- a self-term pass, a pair-term pass over
// the oriented edges (each undirected pair is one oriented edge with both multiplicities) and the tile walk that
// finds every simple triangle {u,v,w} once at its edge u -> v -- with the weights above.  A triangle's payload
// halves are keyed to the orientation (u -> v, v -> w, u -> w in degree order), not to the pattern's direction:
// role_weight takes the six multiplicities around one corner and is called once per corner.
//   ROLE 0..2 (per node)   one 64-bit counter per degree-order id.  u and v get different weights, so the
//                          slots of one edge pre-sum two values per (wave, edge); the adds to w and to every id
//                          below kByNodeWin go to the workgroup's LDS window.
//   ROLE 3 (count(*))      no per-node counters: every lane sums its slots' six-assignment totals, a workgroup
//                          reduces them, and one 64-bit atomic per workgroup and pass reaches the result word.
#include <algorithm>

#include "capsmi_impl.h"
#include "tri_walk.h"

namespace capsmi {
namespace tri {
namespace {

using namespace tiles;

constexpr int kTotal = 3;  // ROLE of the ungrouped form (after CAPSMI_TRI_ROLE_SOURCE / _MIDDLE / _SINK)

// (the window, node_add / win_flush / block_add, the edge pass and the slot search: tri_walk.h)

// What corner x of the simple triangle {x, y, z} receives in ROLE, from the six multiplicities around it.
template <int ROLE>
__device__ __forceinline__ u64 role_weight(uint64_t xy, uint64_t yx, uint64_t xz, uint64_t zx, uint64_t yz, uint64_t zy) {
    if (ROLE == CAPSMI_TRI_ROLE_SOURCE) return xy * xz * (yz + zy);
    if (ROLE == CAPSMI_TRI_ROLE_SINK) return yx * zx * (yz + zy);
    return yx * xz * yz + zx * xy * zy;  // the middle: y -> x -> z closed by y -> z, and z -> x -> y by z -> y
}

// The pair {x, y}'s terms read from x -> y (m = m(x,y), r = m(y,x)): what x and y receive in ROLE.
//   t1 = s(x) m (m-1)   a = b = x, c = y      t2 = m (m-1) s(y)   a = x, b = c = y      t3 = m r s(x)   a = c = x, b = y
template <int ROLE>
__device__ __forceinline__ void pair_terms(uint64_t m, uint64_t r, uint64_t sx, uint64_t sy, u64& tox, u64& toy) {
    const u64 mm = m ? m * (m - 1) : 0, t1 = sx * mm, t2 = mm * sy, t3 = m * r * sx;
    if (ROLE == CAPSMI_TRI_ROLE_SOURCE) { tox += t1 + t2 + t3; }
    else if (ROLE == CAPSMI_TRI_ROLE_MIDDLE) { tox += t1; toy += t2 + t3; }
    else if (ROLE == CAPSMI_TRI_ROLE_SINK) { tox += t3; toy += t1 + t2; }
    else { tox += t1 + t2 + t3; }
}

// self terms, and the self-loop counts in degree-order ids (the sorted build keeps sl by relative id: rel != 0).
// Per node every counter is written (no memset); the count adds to its (zeroed) result word.
template <int ROLE>
__global__ void __launch_bounds__(256) k_ttr_self(const uint32_t* __restrict__ sl, const int64_t* __restrict__ orig,
                                                  int rel, int64_t n, uint32_t* __restrict__ sd, u64* __restrict__ cnt) {
    __shared__ u64 tot;
    u64 acc = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t x = sl[rel ? orig[r] : r];
        sd[r] = (uint32_t)x;
        const u64 t = x >= 3 ? x * (x - 1) * (x - 2) : 0;
        if (ROLE == kTotal) acc += t;
        else cnt[r] = t;
    }
    if (ROLE == kTotal) block_add(acc, &tot, cnt);
}

// pair terms: one oriented edge u -> v per undirected pair, f = m(u,v), b = m(v,u); a pair with one direction
// only has terms too (m (m-1)), so only pairs without a looped end are passed over
template <int ROLE>
__global__ void __launch_bounds__(256) k_ttr_pairs(const uint32_t* __restrict__ tg, TgCode tc,
                                                   const int64_t* __restrict__ ov, const uint32_t* __restrict__ eu,
                                                   const uint32_t* __restrict__ sd, int64_t n, int64_t ne,
                                                   u64* __restrict__ cnt) {
    __shared__ u64 win[ROLE == kTotal ? 1 : kByNodeWin];
    if (ROLE != kTotal) {
        for (int i = threadIdx.x; i < kByNodeWin; i += blockDim.x) win[i] = 0;
        __syncthreads();
    }
    u64 acc = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t word = tg[e];
        const uint32_t u = eu[e], v = tid(word, tc);
        const uint64_t su = sd[u], sv = sd[v];
        if ((su | sv) == 0) continue;  // no loop at either end: no term, no payload read
        const uint64_t pay = tpay(word, tc, ov, e);
        const uint64_t f = pay >> 32, b = pay & 0xffffffffULL;
        u64 tu = 0, tv = 0;
        pair_terms<ROLE>(f, b, su, sv, tu, tv);
        pair_terms<ROLE>(b, f, sv, su, tv, tu);
        if (ROLE == kTotal) {
            acc += tu + tv;
        } else {
            if (tu) node_add(win, cnt, u, tu);
            if (tv) node_add(win, cnt, v, tv);
        }
    }
    if (ROLE == kTotal) {
        block_add(acc, win, cnt);
    } else {
        __syncthreads();
        win_flush(win, cnt, n);
    }
}

// the triangles: tiles of slots (edge, position in the walked list), as k_tbn_walk; see the file comment
template <int ROLE>
__global__ void __launch_bounds__(kExB) k_ttr_walk(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                  const int64_t* __restrict__ tk, int64_t m,
                                                  const int64_t* __restrict__ off, const uint32_t* __restrict__ tg,
                                                  TgCode tc, const int64_t* __restrict__ ov,
                                                  const uint32_t* __restrict__ eu, int64_t n, u64* __restrict__ cnt) {
    __shared__ TileLds L;
    __shared__ u64 win[ROLE == kTotal ? 1 : kByNodeWin];
    const int t = threadIdx.x, lane = t & 63;
    if (ROLE != kTotal) {
        for (int i = t; i < kByNodeWin; i += kExB) win[i] = 0;
        __syncthreads();
    }
    u64 acc = 0;  // ROLE == kTotal: this lane's triangles
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
            u64 wu = 0, wv = 0;
            if (i < nt) {
                // the slot search of tri_walk.h; on a hit x = w closes u -> v -> w
                tile_slot(L, i, off, tg, tc, ov, eu, c, u, v, [&](uint32_t x, uint64_t puv, uint64_t pvw, uint64_t puw) {
                    const uint64_t uv = puv >> 32, vu = puv & 0xffffffffULL;
                    const uint64_t vw = pvw >> 32, wv_ = pvw & 0xffffffffULL;
                    const uint64_t uw = puw >> 32, wu_ = puw & 0xffffffffULL;
                    if (ROLE == kTotal) {  // the six assignments: every corner as the source
                        acc += role_weight<CAPSMI_TRI_ROLE_SOURCE>(uv, vu, uw, wu_, vw, wv_) +
                               role_weight<CAPSMI_TRI_ROLE_SOURCE>(vu, uv, vw, wv_, uw, wu_) +
                               role_weight<CAPSMI_TRI_ROLE_SOURCE>(wu_, uw, wv_, vw, uv, vu);
                    } else {
                        constexpr int R = ROLE == kTotal ? 0 : ROLE;
                        wu = role_weight<R>(uv, vu, uw, wu_, vw, wv_);  // corner u, others v, w
                        wv = role_weight<R>(vu, uv, vw, wv_, uw, wu_);  // corner v, others u, w
                        const u64 ww = role_weight<R>(wu_, uw, wv_, vw, uv, vu);  // corner w, others u, v
                        if (ww) node_add(win, cnt, x, ww);
                    }
                });
            }
            if (ROLE == kTotal) continue;
            if (__ballot((wu | wv) != 0) == 0) continue;  // wave-uniform
            // the lanes of one edge are contiguous: their sums at the edge's first lane, one add each to u and v
            u64 su = wu, sv = wv;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 yu = __shfl_down(su, o, 64), yv = __shfl_down(sv, o, 64);
                const int cy = __shfl_down(c, o, 64);
                if (lane + o < 64 && cy == c) {
                    su += yu;
                    sv += yv;
                }
            }
            const int cp = __shfl_up(c, 1, 64);
            if (lane == 0 || cp != c) {
                if (su) node_add(win, cnt, u, su);
                if (sv) node_add(win, cnt, v, sv);
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
    if (ROLE == kTotal) {
        block_add(acc, win, cnt);
    } else {
        __syncthreads();
        win_flush(win, cnt, n);
    }
}

struct Timers {
    const char *terms, *plan, *walk;
};

// fills cp: ROLE 0..2 one counter per degree-order id, kTotal the (zeroed) result word
template <int ROLE>
void run(capsmi_session* s, const TriGraph& g, u64* cp, const Timers& tm) {
    hipStream_t st = s->stream;
    const int64_t n = g.n, ne = g.ne;
    const TgCode tc{(uint32_t)g.ib, (uint32_t)g.cb};
    Buf sd = dev_alloc(sizeof(uint32_t) * (n > 0 ? n : 1), s);
    Buf eu, len, flag;
    {
        KernelTimer kt(s, tm.terms);
        hipLaunchKernelGGL(k_ttr_self<ROLE>, dim3(egrid(s, n)), dim3(256), 0, st, P<uint32_t>(g.sl), P<int64_t>(g.orig),
                           g.sl_relative ? 1 : 0, n, P<uint32_t>(sd), cp);
        if (ne > 0) {
            eu = dev_alloc(sizeof(uint32_t) * ne, s);
            len = dev_alloc(sizeof(int64_t) * ne, s);
            flag = dev_alloc(ne, s);
            hipLaunchKernelGGL(k_ttr_edges, dim3(egrid(s, ne)), dim3(256), 0, st, P<int64_t>(g.off), P<uint32_t>(g.tg), tc,
                               n, ne, P<uint32_t>(eu), P<int64_t>(len), P<uint8_t>(flag));
            hipLaunchKernelGGL(k_ttr_pairs<ROLE>, dim3(std::min(egrid(s, ne), (unsigned)(4 * s->num_cus))), dim3(256), 0,
                               st, P<uint32_t>(g.tg), tc, P<int64_t>(g.ov), P<uint32_t>(eu), P<uint32_t>(sd), n, ne, cp);
        }
        HIP_CHECK(hipGetLastError());
    }
    if (ne <= 0) return;
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), ne, tm.plan);
    len.reset();
    flag.reset();
    if (tp.m <= 0) return;
    KernelTimer kt(s, tm.walk);
    tile_heads(s, tp);
    hipLaunchKernelGGL(k_ttr_walk<ROLE>, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k,
                       P<int64_t>(tp.tk), tp.m, P<int64_t>(g.off), P<uint32_t>(g.tg), tc, P<int64_t>(g.ov), P<uint32_t>(eu), n,
                       cp);
    HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace tri

// count(*) of the transitive triangle over a single-device trigraph
uint64_t tri_trans_count(capsmi_session* s, const TriGraph& g) {
    using namespace tri;
    REQUIRE(!g.dist, CAPSMI_ERR_UNSUPPORTED, "transitive triangle count: not over a distributed trigraph");
    Buf tot = dev_alloc(sizeof(u64), s);
    HIP_CHECK(hipMemsetAsync(P<void>(tot), 0, sizeof(u64), s->stream));
    run<kTotal>(s, g, P<u64>(tot), Timers{"tri_trans_terms", "tri_trans_plan", "triangles_transitive"});
    u64 h = 0;
    HIP_CHECK(hipMemcpyAsync(&h, P<void>(tot), sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    return h;
}

// rows (relative id, count) of the nodes with a non-zero count in `role`, in no particular order; returns their
// number
int64_t tri_trans_count_by_node(capsmi_session* s, const TriGraph& g, int role, Buf& ids, Buf& counts) {
    using namespace tri;
    REQUIRE(!g.dist, CAPSMI_ERR_UNSUPPORTED, "transitive triangle counts per node: not over a distributed trigraph");
    REQUIRE(role >= CAPSMI_TRI_ROLE_SOURCE && role <= CAPSMI_TRI_ROLE_SINK, CAPSMI_ERR_ILLEGAL_ARGUMENT, "role");
    const int64_t n = g.n;
    Buf cnt = dev_alloc(sizeof(u64) * (n > 0 ? n : 1), s);
    u64* cp = P<u64>(cnt);
    const Timers tm{"tri_trans_by_node_terms", "tri_trans_by_node_plan", "triangles_transitive_by_node"};
    if (role == CAPSMI_TRI_ROLE_SOURCE) run<CAPSMI_TRI_ROLE_SOURCE>(s, g, cp, tm);
    else if (role == CAPSMI_TRI_ROLE_MIDDLE) run<CAPSMI_TRI_ROLE_MIDDLE>(s, g, cp, tm);
    else run<CAPSMI_TRI_ROLE_SINK>(s, g, cp, tm);
    return node_rows(s, g, cp, "tri_trans_by_node_rows", ids, counts);
}

}  // namespace capsmi
