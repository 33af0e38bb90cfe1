// tri_code.h -- the coded oriented targets of a TriGraph and a triangle's weight, shared by the triangle
// count (k_tri.hip) and its per-node form (k_tri_nodes.hip).
#pragma once

#include "capsmi_impl.h"

namespace capsmi {
namespace tri {

struct TgCode {
    uint32_t ib, cb;  // id bits, code bits per direction (0: every payload is an exception)
    __host__ __device__ uint32_t idmask() const { return ib >= 32 ? ~0u : (1u << ib) - 1u; }
    __host__ __device__ uint32_t cmask() const { return (1u << cb) - 1u; }
};

// Oriented targets carry their edge's multiplicities (`TgCode`): word = to | f << ib | b << (ib + cb),
// f = m(from, to), b = m(to, from), cb bits each; a field at its all-ones value (cmask) marks an
// exception whose exact payload is read from ov.  The wedge walks then resolve a hit from the two words
// alone (a hit used to cost two dependent 8-byte payload loads: 47 of the 116 ms at C4, measured by a
// run with the loads removed).  With 2^24 ids, cb = 4: < 1 % of the hits need an exact payload (R-MAT
// s = 20 / 22, hits whose edges carry a multiplicity >= 15).

__device__ __forceinline__ uint32_t tid(uint32_t word, TgCode c) { return word & c.idmask(); }

// payload (f << 32 | b) of a coded word, or the exact one at ov[pos] for an exception
__device__ __forceinline__ uint64_t tpay(uint32_t word, TgCode c, const int64_t* __restrict__ ov, int64_t pos) {
    if (c.cb == 0) return (uint64_t)ov[pos];
    const uint32_t f = (word >> c.ib) & c.cmask(), b = (word >> (c.ib + c.cb)) & c.cmask();
    if (f == c.cmask() || b == c.cmask()) return (uint64_t)ov[pos];
    return (uint64_t)f << 32 | b;
}

__device__ __forceinline__ unsigned long long tri_weight(uint64_t puv, uint64_t pvw, uint64_t puw) {
    const uint64_t m_uv = puv >> 32, m_vu = puv & 0xffffffffULL;
    const uint64_t m_vw = pvw >> 32, m_wv = pvw & 0xffffffffULL;
    const uint64_t m_uw = puw >> 32, m_wu = puw & 0xffffffffULL;
    return m_uv * m_vw * m_wu + m_uw * m_wv * m_vu;
}

// The weight of a hit as a template parameter of the combined list walks (k_tri_small, k_tri_big_items):
// the directed cycle's, and the undirected triangle's U(u,v) U(v,w) U(u,w) with U = f + b of a payload
// (k_tri_nodes.hip).  The latter is symmetric in the three pairs, the order of the arguments does not matter.
struct CycleWeight {
    static __device__ __forceinline__ unsigned long long of(uint64_t puv, uint64_t pvw, uint64_t puw) {
        return tri_weight(puv, pvw, puw);
    }
};
struct UndirectedWeight {
    static __device__ __forceinline__ unsigned long long of(uint64_t puv, uint64_t pvw, uint64_t puw) {
        return ((puv >> 32) + (puv & 0xffffffffULL)) * ((pvw >> 32) + (pvw & 0xffffffffULL)) *
               ((puw >> 32) + (puw & 0xffffffffULL));
    }
};

}  // namespace tri
}  // namespace capsmi
