// k_tri_und.hip -- the undirected triangle (routes "triangle_undirected" and "triangle_undirected_grouped").
//
//   MATCH (a)-[r1]-(b)-[r2]-(c)-[r3]-(a) WHERE n_ok(a), n_ok(b), n_ok(c) RETURN count(*)
//   ... RETURN id(a), count(*)      (or id(b), or id(c))
//
// as RelationalPlanner emits it: the two Expands bind a self-loop once (their incoming branch runs over the
// relationships with start <> end), the closing ExpandInto is a union of two joins without that filter and binds
// a self-loop twice.  r1, r2, r3 are pairwise distinct; a, b, c may coincide.  With m(x,y) the multiplicity of
// x->y (x != y), s(x) the self-loops at x, U(x,y) = m(x,y) + m(y,x) and Q(x,y) = U(x,y) (U(x,y) - 1), the bindings
// are (DESIGN.md "undirected triangle"; restated in tests/tri_und_ref.py)
//   three distinct nodes   U(a,b) U(b,c) U(c,a) per ordered triple: a simple triangle {x,y,z} gives 6 U U U in
//                          all, and 2 U U U to each corner at each position
//   a = b = x, c = y       s(x) Q(x,y)                  (r1 is a loop)
//   b = c = y, a = x       Q(x,y) s(y)                  (r2 is a loop)
//   a = c = x, b = y       2 s(x) Q(x,y)                (r3 is a loop, bound twice)
//   a = b = c = x          2 s(x) (s(x)-1) (s(x)-2)
// The closing hop makes the positions two classes: the ends of the ExpandInto (a and c: the same rows) and the
// middle b.  Per node
//   end(x)    = T(x) + sum_y [3 s(x) + s(y)] Q(x,y) + 2 s (s-1) (s-2)
//   middle(x) = T(x) + sum_y [2 s(x) + 2 s(y)] Q(x,y) + 2 s (s-1) (s-2),     T(x) = sum_{y,z} U(x,y) U(y,z) U(z,x)
// and both sum to the count.  The passes are those of k_tri_trans.hip over a single-device TriGraph's base arrays
// (tri_walk.h): a self-term pass, a pair-term pass over the oriented edges (one per undirected pair, both
// multiplicities in its payload) and the tile walk that finds every simple triangle {u,v,w} once at u -> v.
//   CLS 0, 1 (per node)    one 64-bit counter per degree-order id.  A hit adds the same 2 U U U to u, v and w:
//                          the slots of one edge pre-sum one value per (wave, edge); the adds to w and to every
//                          id below kByNodeWin go to the workgroup's LDS window.
//   CLS 2 (count(*))       no per-node counters: per-lane sums, one 64-bit atomic per workgroup and pass.
// count(*) has a second form (config CAPSMI_TRI_UND_COUNT=hash): the weight is symmetric in the three pairs, so
// the LDS-hash list walks of k_tri.hip over the combined out-lists (tri_und_hash_walk) give sum U U U over the
// simple triangles; the count is 6 times that plus the term passes here.
#include <algorithm>

#include "capsmi_impl.h"
#include "tri_walk.h"

namespace capsmi {
namespace tri {
namespace {

using namespace tiles;

constexpr int kTotal = 2;  // CLS of the ungrouped form (after CAPSMI_TRI_UND_END / _MIDDLE)

__device__ __forceinline__ uint64_t und(uint64_t pay) { return (pay >> 32) + (pay & 0xffffffffULL); }

// self terms, and the self-loop counts in degree-order ids (the sorted build keeps sl by relative id: rel != 0).
// Per node every counter is written (no memset); the count adds to its (zeroed) result word.
template <int CLS>
__global__ void __launch_bounds__(256) k_tun_self(const uint32_t* __restrict__ sl, const int64_t* __restrict__ orig,
                                                  int rel, int64_t n, uint32_t* __restrict__ sd, u64* __restrict__ cnt) {
    __shared__ u64 tot;
    u64 acc = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t x = sl[rel ? orig[r] : r];
        sd[r] = (uint32_t)x;
        const u64 t = x >= 3 ? 2 * x * (x - 1) * (x - 2) : 0;
        if (CLS == kTotal) acc += t;
        else cnt[r] = t;
    }
    if (CLS == kTotal) block_add(acc, &tot, cnt);
}

// the source of every oriented edge (the pair pass of the hash form, which plans no tiles)
__global__ void k_tun_sources(const int64_t* __restrict__ off, int64_t n, int64_t ne, uint32_t* __restrict__ eu) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t a = 0, b = n + 1;  // the first entry of off[0, n] above e (off[n] = ne is)
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (off[mid] <= e) a = mid + 1; else b = mid;
        }
        eu[e] = (uint32_t)(a - 1);
    }
}

// pair terms: one oriented edge u -> v per undirected pair; Q = U (U - 1) with U = m(u,v) + m(v,u).  Only a pair
// with a looped end has a term, and only its payload is read.
//   end:    u gets (3 s(u) + s(v)) Q, v gets (3 s(v) + s(u)) Q      middle: both get 2 (s(u) + s(v)) Q
template <int CLS>
__global__ void __launch_bounds__(256) k_tun_pairs(const uint32_t* __restrict__ tg, TgCode tc,
                                                   const int64_t* __restrict__ ov, const uint32_t* __restrict__ eu,
                                                   const uint32_t* __restrict__ sd, int64_t n, int64_t ne,
                                                   u64* __restrict__ cnt) {
    __shared__ u64 win[CLS == kTotal ? 1 : kByNodeWin];
    if (CLS != kTotal) {
        for (int i = threadIdx.x; i < kByNodeWin; i += blockDim.x) win[i] = 0;
        __syncthreads();
    }
    u64 acc = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t word = tg[e];
        const uint32_t u = eu[e], v = tid(word, tc);
        const uint64_t su = sd[u], sv = sd[v];
        if ((su | sv) == 0) continue;  // no loop at either end: no term, no payload read
        const uint64_t U = und(tpay(word, tc, ov, e));
        const u64 q = U * (U - 1);  // U >= 1: the edge exists
        if (CLS == kTotal) {
            acc += 4 * (su + sv) * q;
        } else {
            const u64 tu = CLS == CAPSMI_TRI_UND_END ? (3 * su + sv) * q : 2 * (su + sv) * q;
            const u64 tv = CLS == CAPSMI_TRI_UND_END ? (3 * sv + su) * q : tu;
            if (tu) node_add(win, cnt, u, tu);
            if (tv) node_add(win, cnt, v, tv);
        }
    }
    if (CLS == kTotal) {
        block_add(acc, win, cnt);
    } else {
        __syncthreads();
        win_flush(win, cnt, n);
    }
}

// the triangles: tiles of slots (edge, position in the walked list), as k_ttr_walk.  Both classes take the same
// walk (T(x) does not depend on the position); CLS only tells the per-node form from the count.
template <int CLS>
__global__ void __launch_bounds__(kExB) k_tun_walk(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                  const int64_t* __restrict__ tk, int64_t m,
                                                  const int64_t* __restrict__ off, const uint32_t* __restrict__ tg,
                                                  TgCode tc, const int64_t* __restrict__ ov,
                                                  const uint32_t* __restrict__ eu, int64_t n, u64* __restrict__ cnt) {
    __shared__ TileLds L;
    __shared__ u64 win[CLS == kTotal ? 1 : kByNodeWin];
    const int t = threadIdx.x, lane = t & 63;
    if (CLS != kTotal) {
        for (int i = t; i < kByNodeWin; i += kExB) win[i] = 0;
        __syncthreads();
    }
    u64 acc = 0;  // CLS == kTotal: this lane's triangles, U U U each
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
            u64 w2 = 0;  // 2 U U U of this slot's triangle
            if (i < nt) {
                tile_slot(L, i, off, tg, tc, ov, eu, c, u, v, [&](uint32_t x, uint64_t puv, uint64_t pvw, uint64_t puw) {
                    const u64 uuu = und(puv) * und(pvw) * und(puw);
                    if (CLS == kTotal) {
                        acc += uuu;
                    } else {
                        w2 = 2 * uuu;
                        node_add(win, cnt, x, w2);
                    }
                });
            }
            if (CLS == kTotal) continue;
            if (__ballot(w2 != 0) == 0) continue;  // wave-uniform
            // the lanes of one edge are contiguous: their sum at the edge's first lane, one add each to u and v
            u64 su = w2;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 yu = __shfl_down(su, o, 64);
                const int cy = __shfl_down(c, o, 64);
                if (lane + o < 64 && cy == c) su += yu;
            }
            const int cp = __shfl_up(c, 1, 64);
            if ((lane == 0 || cp != c) && su) {
                node_add(win, cnt, u, su);
                node_add(win, cnt, v, su);
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
    if (CLS == kTotal) {
        block_add(6 * acc, win, cnt);
    } else {
        __syncthreads();
        win_flush(win, cnt, n);
    }
}

struct Timers {
    const char *terms, *plan, *walk;
};

// fills cp: CLS 0, 1 one counter per degree-order id, kTotal the (zeroed) result word.  walk = false: the term
// passes only (the hash form of the count)
template <int CLS>
void run(capsmi_session* s, const TriGraph& g, u64* cp, const Timers& tm, bool walk) {
    hipStream_t st = s->stream;
    const int64_t n = g.n, ne = g.ne;
    const TgCode tc{(uint32_t)g.ib, (uint32_t)g.cb};
    // the self pass and the walk give both classes the same terms: one per-node instantiation serves them
    constexpr int kSame = CLS == kTotal ? kTotal : CAPSMI_TRI_UND_END;
    Buf sd = dev_alloc(sizeof(uint32_t) * (n > 0 ? n : 1), s);
    Buf eu, len, flag;
    {
        KernelTimer kt(s, tm.terms);
        hipLaunchKernelGGL(k_tun_self<kSame>, dim3(egrid(s, n)), dim3(256), 0, st, P<uint32_t>(g.sl), P<int64_t>(g.orig),
                           g.sl_relative ? 1 : 0, n, P<uint32_t>(sd), cp);
        if (ne > 0) {
            eu = dev_alloc(sizeof(uint32_t) * ne, s);
            if (walk) {
                len = dev_alloc(sizeof(int64_t) * ne, s);
                flag = dev_alloc(ne, s);
                hipLaunchKernelGGL(k_ttr_edges, dim3(egrid(s, ne)), dim3(256), 0, st, P<int64_t>(g.off), P<uint32_t>(g.tg),
                                   tc, n, ne, P<uint32_t>(eu), P<int64_t>(len), P<uint8_t>(flag));
            } else {
                hipLaunchKernelGGL(k_tun_sources, dim3(egrid(s, ne)), dim3(256), 0, st, P<int64_t>(g.off), n, ne,
                                   P<uint32_t>(eu));
            }
            hipLaunchKernelGGL(k_tun_pairs<CLS>, dim3(std::min(egrid(s, ne), (unsigned)(4 * s->num_cus))), dim3(256), 0,
                               st, P<uint32_t>(g.tg), tc, P<int64_t>(g.ov), P<uint32_t>(eu), P<uint32_t>(sd), n, ne, cp);
        }
        HIP_CHECK(hipGetLastError());
    }
    if (ne <= 0 || !walk) return;
    const TilePlan tp = tile_plan(s, P<int64_t>(len), P<uint8_t>(flag), ne, tm.plan);
    len.reset();
    flag.reset();
    if (tp.m <= 0) return;
    KernelTimer kt(s, tm.walk);
    tile_heads(s, tp);
    hipLaunchKernelGGL(k_tun_walk<kSame>, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k,
                       P<int64_t>(tp.tk), tp.m, P<int64_t>(g.off), P<uint32_t>(g.tg), tc, P<int64_t>(g.ov), P<uint32_t>(eu), n,
                       cp);
    HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace tri

// count(*) of the undirected triangle over a single-device trigraph (config CAPSMI_TRI_UND_COUNT: the form)
uint64_t tri_und_count(capsmi_session* s, const TriGraph& g) {
    using namespace tri;
    REQUIRE(!g.dist, CAPSMI_ERR_UNSUPPORTED, "undirected triangle count: not over a distributed trigraph");
    const bool hash = s->cfg.tri_und_hash;
    Buf tot = dev_alloc(2 * sizeof(u64), s);  // [0] the terms (and the search walk's triangles), [1] the hash walks' sum
    HIP_CHECK(hipMemsetAsync(P<void>(tot), 0, 2 * sizeof(u64), s->stream));
    run<kTotal>(s, g, P<u64>(tot), Timers{"tri_und_terms", "tri_und_plan", "triangles_undirected_walk"}, !hash);
    if (hash && g.ne > 0) tri_und_hash_walk(s, g, P<u64>(tot) + 1);
    u64 h[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(h, P<void>(tot), 2 * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    return h[0] + 6 * h[1];
}

// rows (relative id, count) of the nodes with a non-zero count at a position of class `position`, in no
// particular order; returns their number
int64_t tri_und_count_by_node(capsmi_session* s, const TriGraph& g, int position, Buf& ids, Buf& counts) {
    using namespace tri;
    REQUIRE(!g.dist, CAPSMI_ERR_UNSUPPORTED, "undirected triangle counts per node: not over a distributed trigraph");
    REQUIRE(position == CAPSMI_TRI_UND_END || position == CAPSMI_TRI_UND_MIDDLE, CAPSMI_ERR_ILLEGAL_ARGUMENT, "position");
    const int64_t n = g.n;
    Buf cnt = dev_alloc(sizeof(u64) * (n > 0 ? n : 1), s);
    u64* cp = P<u64>(cnt);
    const Timers tm{"tri_und_by_node_terms", "tri_und_by_node_plan", "triangles_undirected_by_node"};
    if (position == CAPSMI_TRI_UND_END) run<CAPSMI_TRI_UND_END>(s, g, cp, tm, true);
    else run<CAPSMI_TRI_UND_MIDDLE>(s, g, cp, tm, true);
    return node_rows(s, g, cp, "tri_und_by_node_rows", ids, counts);
}

}  // namespace capsmi
