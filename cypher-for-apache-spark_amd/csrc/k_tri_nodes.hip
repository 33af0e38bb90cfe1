// k_tri_nodes.hip -- the tile walks over a single-device TriGraph's base arrays (off, tg, ov, sl, orig): the
// closed triangle over one relationship set with pairwise distinct relationships r1, r2, r3, where a, b, c may
// coincide, in three shapes:
//   cycle        (a)-[r1]->(b)-[r2]->(c)-[r3]->(a)   RETURN id(a), count(*)               "triangle_grouped"
//   transitive   (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a)   RETURN count(*) | id(a|b|c), count(*)
//                                                    "triangle_transitive", "triangle_transitive_grouped"
//   undirected   (a)-[r1]-(b)-[r2]-(c)-[r3]-(a)      RETURN count(*) | id(a|b|c), count(*)
//                                                    "triangle_undirected", "triangle_undirected_grouped"
// (the cycle's count(*) is tri_count in k_tri.hip).  With m(x,y) the multiplicity of x->y (x != y), s(x) the
// self-loops at x, M(y,z) = U(y,z) = m(y,z) + m(z,y) and Q(x,y) = U(x,y) (U(x,y) - 1), node x receives
// (DESIGN.md "grouped triangle", "transitive triangle", "undirected triangle"; restated in tests/tri_*_ref.py)
//   cycle        from a simple triangle {u,v,w} containing x: tri_weight(u,v,w); from a pair {x,y}:
//                m(x,y) m(y,x) (2 s(x) + s(y)); from itself: s (s-1) (s-2).  The same numbers group the pattern by
//                b or by c (rotation).
//   transitive   the positions are three roles, each with its own per-node count.  From a simple triangle {x,y,z}
//                  as source a   m(x,y) m(x,z) M(y,z)
//                  as sink c     m(y,x) m(z,x) M(y,z)
//                  as middle b   m(y,x) m(x,z) m(y,z) + m(z,x) m(x,y) m(z,y)
//                from a pair, credited to the node in the role (a pair with relationships in one direction only
//                has such terms too)
//                  a = b = x, c = y   s(x) m(x,y) (m(x,y)-1)      (r1 is a loop)
//                  b = c = y, a = x   m(x,y) (m(x,y)-1) s(y)      (r2 is a loop)
//                  a = c = x, b = y   m(x,y) m(y,x) s(x)          (r3 is a loop)
//                and a = b = c = x: s (s-1) (s-2).
//   undirected   as RelationalPlanner emits it: the two Expands bind a self-loop once (their incoming branch runs
//                over the relationships with start <> end), the closing ExpandInto is a union of two joins without
//                that filter and binds a self-loop twice.  That makes the positions two classes, the ends of the
//                ExpandInto (a and c: the same rows) and the middle b:
//                  end(x)    = T(x) + sum_y [3 s(x) + s(y)] Q(x,y) + 2 s (s-1) (s-2)
//                  middle(x) = T(x) + sum_y [2 s(x) + 2 s(y)] Q(x,y) + 2 s (s-1) (s-2)
//                with T(x) = sum_{y,z} U(x,y) U(y,z) U(z,x): 2 U U U from every simple triangle containing x.
// A count(*) is the sum of one role's (class's) per-node counts.  Every shape fills its counters in three passes:
//   self terms   one pass over the vertices (which also brings sl into degree-order ids);
//   pair terms   one pass over the oriented edges: each undirected pair is one oriented edge with both
//                multiplicities;
//   triangles    every simple triangle {u,v,w}, u -> v -> w in the orientation (w < v < u as degree-order ids),
//                is found once, at its edge u -> v (position p of out(u)): w is common to out(v) and to
//                out(u)[0, p).  The edge owns min(od(v), p) slots: it walks the shorter of the two lists, one
//                entry per slot, and binary-searches the other (both are sorted by id).  The slots of all edges
//                are cut into fixed tiles of kExplodeTile (tile_owner.h), so a workgroup's work does not depend
//                on the degree distribution and a hub's wedges spread over as many tiles as they fill.
// The shapes differ in the weights only: each is a policy W (Cycle, Transitive, Undirected below).  A triangle's
// payload halves are keyed to the orientation (u -> v, v -> w, u -> w in degree order), not to the pattern.
//   per node     one 64-bit counter per degree-order id.  A hit adds a weight to each corner.  The slots of one
//                edge are consecutive lanes, so the adds to u and v are summed per (wave, edge) first.  The adds to
//                w -- the highest-degree corner, i.e. the lowest ids -- and every other add to an id below
//                kByNodeWin go to a per-workgroup LDS window of 64-bit counters that is flushed once at the
//                kernel's end; the rest are 64-bit global atomics on counters that few slots share.
//   count(*)     no per-node counters: every lane sums what its slots' corners receive, a workgroup reduces the
//                sums, and one 64-bit atomic per workgroup and pass reaches the result word.
// The undirected count(*) has a second form (config CAPSMI_TRI_UND_COUNT=hash): its weight is symmetric in the
// three pairs, so the LDS-hash list walks of k_tri.hip over the combined out-lists (tri_und_hash_walk) give
// sum U U U over the simple triangles; the count is 6 times that plus the term passes here.
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

// A shape's weights W:
//   kTotal    count(*): one (zeroed) result word takes the sum of what the nodes would receive; else one counter
//             per degree-order id
//   kOneWay   a pair with relationships in one direction only can have pair terms
//   kSameUV   a hit gives u and v the same weight: the (wave, edge) pre-sum carries one value, not two
//   Walk      the policy whose self and walk kernels serve this one (the same terms: one instantiation)
//   self(s)   the self term of a node with s loops
//   pair(f, b, su, sv, tu, tv)   adds the terms of the pair {u, v}, f = m(u,v), b = m(v,u), to tu and tv
//   hit(puv, pvw, puw, wu, wv, ww)   what the simple triangle's corners receive, from its three payloads
//             (f << 32 | b of u -> v, v -> w, u -> w)
struct Cycle {
    static constexpr bool kTotal = false, kOneWay = false, kSameUV = true;
    typedef Cycle Walk;
    static __device__ __forceinline__ u64 self(uint64_t s) { return s >= 3 ? s * (s - 1) * (s - 2) : 0; }
    // both directions present: f b (2 s(x) + s(y)) to x = u, v
    static __device__ __forceinline__ void pair(uint64_t f, uint64_t b, uint64_t su, uint64_t sv, u64& tu, u64& tv) {
        tu += f * b * (2 * su + sv);
        tv += f * b * (2 * sv + su);
    }
    static __device__ __forceinline__ void hit(uint64_t puv, uint64_t pvw, uint64_t puw, u64& wu, u64& wv, u64& ww) {
        wu = wv = ww = tri_weight(puv, pvw, puw);
    }
};

// ROLE: CAPSMI_TRI_ROLE_SOURCE / _MIDDLE / _SINK
template <int ROLE, bool TOTAL>
struct Transitive {
    static constexpr bool kTotal = TOTAL, kOneWay = true, kSameUV = false;
    typedef Transitive Walk;
    static __device__ __forceinline__ u64 self(uint64_t s) { return Cycle::self(s); }
    // What corner x of the simple triangle {x, y, z} receives in ROLE, from the six multiplicities around it.
    static __device__ __forceinline__ u64 role_weight(uint64_t xy, uint64_t yx, uint64_t xz, uint64_t zx, uint64_t yz,
                                                      uint64_t zy) {
        if (ROLE == CAPSMI_TRI_ROLE_SOURCE) return xy * xz * (yz + zy);
        if (ROLE == CAPSMI_TRI_ROLE_SINK) return yx * zx * (yz + zy);
        return yx * xz * yz + zx * xy * zy;  // the middle: y -> x -> z closed by y -> z, and z -> x -> y by z -> y
    }
    // The pair {x, y}'s terms read from x -> y (m = m(x,y), r = m(y,x)): what x and y receive in ROLE.
    //   t1 = s(x) m (m-1)   a = b = x, c = y      t2 = m (m-1) s(y)   a = x, b = c = y      t3 = m r s(x)   a = c = x, b = y
    static __device__ __forceinline__ void pair_terms(uint64_t m, uint64_t r, uint64_t sx, uint64_t sy, u64& tox, u64& toy) {
        const u64 mm = m ? m * (m - 1) : 0, t1 = sx * mm, t2 = mm * sy, t3 = m * r * sx;
        if (ROLE == CAPSMI_TRI_ROLE_SOURCE) { tox += t1 + t2 + t3; }
        else if (ROLE == CAPSMI_TRI_ROLE_MIDDLE) { tox += t1; toy += t2 + t3; }
        else { tox += t3; toy += t1 + t2; }
    }
    static __device__ __forceinline__ void pair(uint64_t f, uint64_t b, uint64_t su, uint64_t sv, u64& tu, u64& tv) {
        pair_terms(f, b, su, sv, tu, tv);
        pair_terms(b, f, sv, su, tv, tu);
    }
    static __device__ __forceinline__ void hit(uint64_t puv, uint64_t pvw, uint64_t puw, u64& wu, u64& wv, u64& ww) {
        const uint64_t uv = puv >> 32, vu = puv & 0xffffffffULL;
        const uint64_t vw = pvw >> 32, wv_ = pvw & 0xffffffffULL;
        const uint64_t uw = puw >> 32, wu_ = puw & 0xffffffffULL;
        wu = role_weight(uv, vu, uw, wu_, vw, wv_);  // corner u, others v, w
        wv = role_weight(vu, uv, vw, wv_, uw, wu_);  // corner v, others u, w
        ww = role_weight(wu_, uw, wv_, vw, uv, vu);  // corner w, others u, v
    }
};

// CLS: CAPSMI_TRI_UND_END / _MIDDLE.  The classes differ in the pair terms only.
template <int CLS, bool TOTAL>
struct Undirected {
    static constexpr bool kTotal = TOTAL, kOneWay = true, kSameUV = true;
    typedef Undirected<CAPSMI_TRI_UND_END, TOTAL> Walk;
    static __device__ __forceinline__ uint64_t und(uint64_t pay) { return (pay >> 32) + (pay & 0xffffffffULL); }
    static __device__ __forceinline__ u64 self(uint64_t s) { return 2 * Cycle::self(s); }
    // Q = U (U - 1), U >= 1 (the edge exists)
    //   end:    u gets (3 s(u) + s(v)) Q, v gets (3 s(v) + s(u)) Q      middle: both get 2 (s(u) + s(v)) Q
    static __device__ __forceinline__ void pair(uint64_t f, uint64_t b, uint64_t su, uint64_t sv, u64& tu, u64& tv) {
        const u64 U = f + b, q = U * (U - 1);
        tu += CLS == CAPSMI_TRI_UND_END ? (3 * su + sv) * q : 2 * (su + sv) * q;
        tv += CLS == CAPSMI_TRI_UND_END ? (3 * sv + su) * q : 2 * (su + sv) * q;
    }
    static __device__ __forceinline__ void hit(uint64_t puv, uint64_t pvw, uint64_t puw, u64& wu, u64& wv, u64& ww) {
        wu = wv = ww = 2 * (und(puv) * und(pvw) * und(puw));
    }
};

// self terms, and the self-loop counts in degree-order ids (the sorted build keeps sl by relative id: rel != 0).
// Per node every counter is written (no memset); the count adds to its (zeroed) result word.
template <class W>
__global__ void __launch_bounds__(256) k_tri_self(const uint32_t* __restrict__ sl, const int64_t* __restrict__ orig,
                                                  int rel, int64_t n, uint32_t* __restrict__ sd, u64* __restrict__ cnt) {
    __shared__ u64 tot;
    u64 acc = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t x = sl[rel ? orig[r] : r];
        sd[r] = (uint32_t)x;
        if (W::kTotal) acc += W::self(x);
        else cnt[r] = W::self(x);
    }
    if (W::kTotal) block_add(acc, &tot, cnt);
}

// the source of oriented edge e: off is searched (the base arrays keep no source column)
__device__ __forceinline__ int64_t edge_source(const int64_t* __restrict__ off, int64_t n, int64_t e) {
    int64_t a = 0, b = n + 1;  // the first entry of off[0, n] above e (off[n] = ne is)
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if (off[mid] <= e) a = mid + 1; else b = mid;
    }
    return a - 1;
}

// per oriented edge e = u -> v at position p of out(u): its source, and its slots, min(od(v), p)
__global__ void k_tri_edges(const int64_t* __restrict__ off, const uint32_t* __restrict__ tg, TgCode tc, int64_t n,
                            int64_t ne, uint32_t* __restrict__ eu, int64_t* __restrict__ len, uint8_t* __restrict__ flag) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = edge_source(off, n, e);
        const uint32_t v = tid(tg[e], tc);
        const int64_t l = min(off[v + 1] - off[v], e - off[u]);
        eu[e] = (uint32_t)u;
        len[e] = l;
        flag[e] = l > 0 ? 1 : 0;
    }
}

// the source of every oriented edge (the pair pass of the undirected count's hash form, which plans no tiles)
__global__ void k_tun_sources(const int64_t* __restrict__ off, int64_t n, int64_t ne, uint32_t* __restrict__ eu) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x)
        eu[e] = (uint32_t)edge_source(off, n, e);
}

// pair terms: one oriented edge u -> v per undirected pair, f = m(u,v), b = m(v,u).  Only a pair with a looped
// end has a term.  Where one direction alone has none either (!kOneWay), such pairs are passed over on the coded
// word, before the gathers; else the pairs without a looped end are, before the payload read.
template <class W>
__global__ void __launch_bounds__(256) k_tri_pairs(const uint32_t* __restrict__ tg, TgCode tc,
                                                   const int64_t* __restrict__ ov, const uint32_t* __restrict__ eu,
                                                   const uint32_t* __restrict__ sd, int64_t n, int64_t ne,
                                                   u64* __restrict__ cnt) {
    __shared__ u64 win[W::kTotal ? 1 : kByNodeWin];
    if (!W::kTotal) {
        for (int i = threadIdx.x; i < kByNodeWin; i += blockDim.x) win[i] = 0;
        __syncthreads();
    }
    u64 acc = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t word = tg[e];
        uint64_t pay = 0;
        if (!W::kOneWay) {
            pay = tpay(word, tc, ov, e);
            if ((pay >> 32) == 0 || (pay & 0xffffffffULL) == 0) continue;  // one direction only: no term, no gathers
        }
        const uint32_t u = eu[e], v = tid(word, tc);
        const uint64_t su = sd[u], sv = sd[v];
        if ((su | sv) == 0) continue;  // no loop at either end: no term, no payload read
        if (W::kOneWay) pay = tpay(word, tc, ov, e);
        u64 tu = 0, tv = 0;
        W::pair(pay >> 32, pay & 0xffffffffULL, su, sv, tu, tv);
        if (W::kTotal) {
            acc += tu + tv;
        } else {  // (both directions and a looped end: neither term is zero)
            if (!W::kOneWay || tu) node_add(win, cnt, u, tu);
            if (!W::kOneWay || tv) node_add(win, cnt, v, tv);
        }
    }
    if (W::kTotal) {
        block_add(acc, win, cnt);
    } else {
        __syncthreads();
        win_flush(win, cnt, n);
    }
}

// Slot i of a tile_owners tile whose rows are oriented edges e = u -> v with min(od(v), p) slots each (p = e's
// position in out(u)): the slot walks entry j of the shorter of out(v) and out(u)[0, p) and binary-searches the
// other.  Sets c (the slot's tile-local row), u and v; where the entry closes u -> v -> w, calls
// hit(w, puv, pvw, puw) with the three payloads (f << 32 | b of u -> v, v -> w, u -> w).
template <class Hit>
__device__ __forceinline__ void tile_slot(const TileLds& L, int i, const int64_t* __restrict__ off,
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

// the triangles: tiles of slots (edge, position in the walked list); see the file comment
template <class W>
__global__ void __launch_bounds__(kExB) k_tri_walk(const int64_t* __restrict__ cs, const int64_t* __restrict__ nz, int64_t k,
                                                  const int64_t* __restrict__ tk, int64_t m,
                                                  const int64_t* __restrict__ off, const uint32_t* __restrict__ tg,
                                                  TgCode tc, const int64_t* __restrict__ ov,
                                                  const uint32_t* __restrict__ eu, int64_t n, u64* __restrict__ cnt) {
    __shared__ TileLds L;
    __shared__ u64 win[W::kTotal ? 1 : kByNodeWin];
    const int t = threadIdx.x, lane = t & 63;
    if (!W::kTotal) {
        for (int i = t; i < kByNodeWin; i += kExB) win[i] = 0;
        __syncthreads();
    }
    u64 acc = 0;  // kTotal: this lane's triangles
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
                tile_slot(L, i, off, tg, tc, ov, eu, c, u, v, [&](uint32_t x, uint64_t puv, uint64_t pvw, uint64_t puw) {
                    u64 ww;
                    W::hit(puv, pvw, puw, wu, wv, ww);
                    if (W::kTotal) acc += wu + wv + ww;
                    else if (ww) node_add(win, cnt, x, ww);
                });
            }
            if (W::kTotal) continue;
            if (__ballot((W::kSameUV ? wu : wu | wv) != 0) == 0) continue;  // wave-uniform
            // the lanes of one edge are contiguous: their sums at the edge's first lane, one add each to u and v
            u64 su = wu, sv = wv;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 yu = __shfl_down(su, o, 64), yv = W::kSameUV ? 0 : __shfl_down(sv, o, 64);
                const int cy = __shfl_down(c, o, 64);
                if (lane + o < 64 && cy == c) {
                    su += yu;
                    sv += yv;
                }
            }
            const u64 tv = W::kSameUV ? su : sv;
            const int cp = __shfl_up(c, 1, 64);
            if (lane == 0 || cp != c) {
                if (su) node_add(win, cnt, u, su);
                if (tv) node_add(win, cnt, v, tv);
            }
        }
        __syncthreads();  // the next tile rewrites the LDS arrays
    }
    if (W::kTotal) {
        block_add(acc, win, cnt);
    } else {
        __syncthreads();
        win_flush(win, cnt, n);
    }
}

__global__ void k_tri_flags(const u64* __restrict__ cnt, int64_t n, uint8_t* __restrict__ f) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
        f[r] = cnt[r] != 0 ? 1 : 0;
}

struct Timers {
    const char *terms, *plan, *walk, *rows;
};

// fills cp: one counter per degree-order id, or (W::kTotal) the zeroed result word.  walk = false: the term
// passes only (the hash form of the undirected count)
template <class W>
void run(capsmi_session* s, const TriGraph& g, u64* cp, const Timers& tm, bool walk) {
    hipStream_t st = s->stream;
    const int64_t n = g.n, ne = g.ne;
    const TgCode tc{(uint32_t)g.ib, (uint32_t)g.cb};
    Buf sd = dev_alloc(sizeof(uint32_t) * (n > 0 ? n : 1), s);
    Buf eu, len, flag;
    {
        KernelTimer kt(s, tm.terms);
        hipLaunchKernelGGL(k_tri_self<typename W::Walk>, dim3(egrid(s, n)), dim3(256), 0, st, P<uint32_t>(g.sl),
                           P<int64_t>(g.orig), g.sl_relative ? 1 : 0, n, P<uint32_t>(sd), cp);
        if (ne > 0) {
            eu = dev_alloc(sizeof(uint32_t) * ne, s);
            if (walk) {
                len = dev_alloc(sizeof(int64_t) * ne, s);
                flag = dev_alloc(ne, s);
                hipLaunchKernelGGL(k_tri_edges, dim3(egrid(s, ne)), dim3(256), 0, st, P<int64_t>(g.off), P<uint32_t>(g.tg),
                                   tc, n, ne, P<uint32_t>(eu), P<int64_t>(len), P<uint8_t>(flag));
            } else {
                hipLaunchKernelGGL(k_tun_sources, dim3(egrid(s, ne)), dim3(256), 0, st, P<int64_t>(g.off), n, ne,
                                   P<uint32_t>(eu));
            }
            hipLaunchKernelGGL(k_tri_pairs<W>, dim3(std::min(egrid(s, ne), (unsigned)(4 * s->num_cus))), dim3(256), 0, st,
                               P<uint32_t>(g.tg), tc, P<int64_t>(g.ov), P<uint32_t>(eu), P<uint32_t>(sd), n, ne, cp);
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
    hipLaunchKernelGGL(k_tri_walk<typename W::Walk>, dim3(tile_grid(s, tp.ntiles)), dim3(kExB), 0, st, tp.cs, tp.nz, tp.k,
                       P<int64_t>(tp.tk), tp.m, P<int64_t>(g.off), P<uint32_t>(g.tg), tc, P<int64_t>(g.ov), P<uint32_t>(eu), n,
                       cp);
    HIP_CHECK(hipGetLastError());
}

// indexed by TriShape
const char* const kShapeName[] = {"triangle", "transitive triangle", "undirected triangle"};
const Timers kCountTimers[] = {{},
                               {"tri_trans_terms", "tri_trans_plan", "triangles_transitive", nullptr},
                               {"tri_und_terms", "tri_und_plan", "triangles_undirected_walk", nullptr}};
const Timers kByNodeTimers[] = {
    {"tri_by_node_terms", "tri_by_node_plan", "triangles_by_node", "tri_by_node_rows"},
    {"tri_trans_by_node_terms", "tri_trans_by_node_plan", "triangles_transitive_by_node", "tri_trans_by_node_rows"},
    {"tri_und_by_node_terms", "tri_und_by_node_plan", "triangles_undirected_by_node", "tri_und_by_node_rows"}};

}  // namespace
}  // namespace tri

// count(*) of the transitive or the undirected triangle (the latter in the form config CAPSMI_TRI_UND_COUNT selects)
uint64_t tri_shape_count(capsmi_session* s, const TriGraph& g, TriShape shape) {
    using namespace tri;
    REQUIRE(shape != TriShape::cycle, CAPSMI_ERR_INTERNAL, "the cyclic triangle's count is tri_count");
    const int si = (int)shape;
    REQUIRE(!g.dist, CAPSMI_ERR_UNSUPPORTED, std::string(kShapeName[si]) + " count: not over a distributed trigraph");
    const bool hash = shape == TriShape::undirected && s->cfg.tri_und_hash;
    Buf tot = dev_alloc(2 * sizeof(u64), s);  // [0] the terms (and the search walk's triangles), [1] the hash walks' sum
    HIP_CHECK(hipMemsetAsync(P<void>(tot), 0, 2 * sizeof(u64), s->stream));
    if (shape == TriShape::transitive) run<Transitive<CAPSMI_TRI_ROLE_SOURCE, true>>(s, g, P<u64>(tot), kCountTimers[si], true);
    else run<Undirected<CAPSMI_TRI_UND_MIDDLE, true>>(s, g, P<u64>(tot), kCountTimers[si], !hash);
    if (hash && g.ne > 0) tri_und_hash_walk(s, g, P<u64>(tot) + 1);
    u64 h[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(h, P<void>(tot), 2 * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    return h[0] + 6 * h[1];
}

// rows (relative id, count) of the nodes with a non-zero count, in no particular order; returns their number
int64_t tri_shape_count_by_node(capsmi_session* s, const TriGraph& g, TriShape shape, int cls, Buf& ids, Buf& counts) {
    using namespace tri;
    const int si = (int)shape;
    REQUIRE(!g.dist, CAPSMI_ERR_UNSUPPORTED,
            std::string(kShapeName[si]) + " counts per node: not over a distributed trigraph");
    hipStream_t st = s->stream;
    const int64_t n = g.n;
    const Timers& tm = kByNodeTimers[si];
    Buf cnt = dev_alloc(sizeof(u64) * (n > 0 ? n : 1), s);
    u64* cp = P<u64>(cnt);
    if (shape == TriShape::cycle) {
        run<Cycle>(s, g, cp, tm, true);
    } else if (shape == TriShape::transitive) {
        REQUIRE(cls >= CAPSMI_TRI_ROLE_SOURCE && cls <= CAPSMI_TRI_ROLE_SINK, CAPSMI_ERR_ILLEGAL_ARGUMENT, "role");
        if (cls == CAPSMI_TRI_ROLE_SOURCE) run<Transitive<CAPSMI_TRI_ROLE_SOURCE, false>>(s, g, cp, tm, true);
        else if (cls == CAPSMI_TRI_ROLE_MIDDLE) run<Transitive<CAPSMI_TRI_ROLE_MIDDLE, false>>(s, g, cp, tm, true);
        else run<Transitive<CAPSMI_TRI_ROLE_SINK, false>>(s, g, cp, tm, true);
    } else {
        REQUIRE(cls == CAPSMI_TRI_UND_END || cls == CAPSMI_TRI_UND_MIDDLE, CAPSMI_ERR_ILLEGAL_ARGUMENT, "position");
        if (cls == CAPSMI_TRI_UND_END) run<Undirected<CAPSMI_TRI_UND_END, false>>(s, g, cp, tm, true);
        else run<Undirected<CAPSMI_TRI_UND_MIDDLE, false>>(s, g, cp, tm, true);
    }
    KernelTimer kt(s, tm.rows);
    Buf f = dev_alloc(n > 0 ? n : 1, s), idx;
    hipLaunchKernelGGL(k_tri_flags, dim3(egrid(s, n)), dim3(256), 0, st, cp, n, P<uint8_t>(f));
    HIP_CHECK(hipGetLastError());
    const int64_t rows = flags_to_indices(s, P<uint8_t>(f), n, idx);
    ids = dev_alloc(sizeof(int64_t) * (rows > 0 ? rows : 1), s);
    counts = dev_alloc(sizeof(int64_t) * (rows > 0 ? rows : 1), s);
    gather_col(P<int64_t>(g.orig), nullptr, P<int64_t>(idx), rows, P<int64_t>(ids), nullptr, st);
    gather_col(reinterpret_cast<const int64_t*>(cp), nullptr, P<int64_t>(idx), rows, P<int64_t>(counts), nullptr, st);
    return rows;
}

}  // namespace capsmi
