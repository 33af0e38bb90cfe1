// k_reach.hip -- count(DISTINCT b) and collect(DISTINCT b) over a bounded var-length expand: k-hop reach by
// bit-parallel BFS, and the reach lists read off its bit matrix (the last section).
//
//   MATCH (a)-[r*lower..upper]->(b) WHERE a_ok(a) AND b_ok(b) RETURN id(a), count(DISTINCT b)   (grouped)
//   MATCH (a)-[r*lower..upper]->(b) WHERE a_ok(a) AND b_ok(b) RETURN count(DISTINCT b)          (global)
//   lower in {0, 1}, upper >= 1 (a level budget: a frontier dies after at most n levels)
//
// Lemma: for lower <= 1, b ends a relationship-distinct path of length in [1, k] from a iff b
// ends a walk of length in [1, k] from a -- cut the stretch between two uses of a repeated relationship; the
// walk stays a walk from a to b, gets shorter and keeps one relationship.  So the distinct ends are plain
// bounded reachability, with none of the uniqueness corrections of the count(*) closed form (k_varlen.hip).
// lower = 0 adds the zero-length path, whose b is a copy of a without b's node scan (k_final's rule): a
// counts once whatever b_ok(a) says, and once only when a cycle also returns to it.
//
// Levels: R_0 = {}, F_0 = {a}; N_i = heads of the relationships whose tail is in F_(i-1), F_i = N_i \ R_(i-1),
// R_i = R_(i-1) | N_i.  Only new nodes are expanded; an empty frontier ends the walk.
//
// Global form: one BFS from all of a_ok over three n-bit maps (reached, frontier, next).
// Grouped form: multi-source BFS, 64 * NW sources per batch (NW 64-bit words per node, node-major), the
// batches walking the set bits of a_ok in id order.  The relationships are bucketed once per query by
// TARGET slice (the chunked partition of k_part.hip); the block that owns a slice segment ORs
// front[source] into its slice's `next` words in LDS, and a block that holds all of a slice's chunks finishes
// the slice from LDS (new = next & ~seen, plain stores of seen and front, per-source counts by ballot).
// Slices shared by several blocks, and slices no relationship enters, are finished by k_rg_fix.
#include "part_common.h"

namespace capsmi {
namespace reach {

using u64 = unsigned long long;
using part::ChunkWalk;

constexpr int kBlock = 1024;
constexpr int kLdsWords = 16384;  // 128 KiB of `next` words per block: 16384 / NW ids per slice
constexpr int kMaxWords = 8;
constexpr int kListTile = 256;  // nodes per extraction tile of the reach lists (a multiple of 64)

inline int grid(const capsmi_session* s, int64_t n) {
    int64_t g = (n + 255) / 256;
    const int64_t cap = (int64_t)s->num_cus * 16;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

__device__ __forceinline__ bool bit_of(const uint32_t* w, int full, uint64_t x) {
    return full || ((w[x >> 5] >> (x & 31)) & 1u);
}

__global__ void k_zero3(u64* a, u64* b, u64* c, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        a[i] = 0;
        b[i] = 0;
        c[i] = 0;
    }
}

// ---- global form ------------------------------------------------------------------------------------------
// F = a_ok over the nw words of the window (bits past n clear), R = N = 0
__global__ void k_rc_init(const uint32_t* __restrict__ aw, int a_full, int64_t n, int64_t nw, uint32_t* __restrict__ F,
                          uint32_t* __restrict__ R, uint32_t* __restrict__ N) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t left = n - 32 * i;
        const uint32_t in = left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u);
        F[i] = (a_full ? 0xFFFFFFFFu : aw[i]) & in;
        R[i] = 0;
        N[i] = 0;
    }
}

// one level: the head's bit in N for every relationship whose tail is in F; heads already reached, or already
// marked this level, cost a load and no atomic
template <typename IdT>
__global__ void k_rc_level(const IdT* __restrict__ src, const IdT* __restrict__ dst, int64_t m, int64_t lo, uint64_t n,
                           const uint32_t* __restrict__ F, const uint32_t* __restrict__ R, uint32_t* __restrict__ N) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t u = part::rel_id(src[e], lo), v = part::rel_id(dst[e], lo);
        if (u >= n || v >= n) continue;
        if (!((F[u >> 5] >> (u & 31)) & 1u)) continue;
        const uint32_t bit = 1u << (v & 31);
        if ((R[v >> 5] | N[v >> 5]) & bit) continue;
        atomicOr(&N[v >> 5], bit);
    }
}

// per node word: new = N & ~R, R |= new, F = new, N = 0; tot[0] += new bits in b_ok, tot[1] += new bits
// (one add per block each: the host compares tot[1] with the level before to see an empty frontier)
__global__ void k_rc_final(int64_t nw, uint32_t* __restrict__ N, uint32_t* __restrict__ R, uint32_t* __restrict__ F,
                           const uint32_t* __restrict__ bw, int b_full, u64* __restrict__ tot) {
    __shared__ unsigned int cb, cn;
    if (threadIdx.x == 0) cb = cn = 0;
    __syncthreads();
    unsigned int mb = 0, mn = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t nx = N[i], r = R[i], nv = nx & ~r;
        if (nx) N[i] = 0;
        if (nv) R[i] = r | nv;
        F[i] = nv;
        mn += __popc(nv);
        mb += __popc(b_full ? nv : nv & bw[i]);
    }
    if (mb) atomicAdd(&cb, mb);
    if (mn) atomicAdd(&cn, mn);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (cb) atomicAdd(&tot[0], (u64)cb);
        if (cn) atomicAdd(&tot[1], (u64)cn);
    }
}

// lower = 0: the a_ok nodes that the reached b_ok set does not hold already
__global__ void k_rc_zero(int64_t n, int64_t nw, const uint32_t* __restrict__ R, const uint32_t* __restrict__ aw,
                          int a_full, const uint32_t* __restrict__ bw, int b_full, u64* __restrict__ tot) {
    __shared__ unsigned int cb;
    if (threadIdx.x == 0) cb = 0;
    __syncthreads();
    unsigned int mb = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t left = n - 32 * i;
        const uint32_t in = left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u);
        const uint32_t a = (a_full ? 0xFFFFFFFFu : aw[i]) & in;
        mb += __popc(a & ~(R[i] & (b_full ? 0xFFFFFFFFu : bw[i])));
    }
    if (mb) atomicAdd(&cb, mb);
    __syncthreads();
    if (threadIdx.x == 0 && cb) atomicAdd(&tot[0], (u64)cb);
}

// ---- grouped form -----------------------------------------------------------------------------------------
__global__ void k_rg_flags(const uint32_t* __restrict__ aw, int a_full, int64_t n, uint8_t* __restrict__ f) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        f[i] = bit_of(aw, a_full, (uint64_t)i) ? 1 : 0;
}

// source j of the batch (node idx[j], relative) starts with its own bit in the frontier (distinct nodes: plain stores)
__global__ void k_rg_init(const int64_t* __restrict__ idx, int bw, int nwords, u64* __restrict__ front) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < bw) front[idx[j] * nwords + (j >> 6)] = 1ULL << (j & 63);
}

// OR of a 64-bit value over the wave, the same in every lane
__device__ __forceinline__ u64 wave_or(u64 x) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x |= __shfl_xor(x, o, 64);
    return x;
}

// The lanes of a wave hold 64 nodes' new bits of word w (0 for nodes outside b_ok): per set source bit j, the
// number of lanes that hold it goes into the block's LDS counter of source 64 w + j.  All 64 lanes call.
__device__ __forceinline__ void count_sources(u64 cm, int w, uint32_t* cl) {
    u64 m = wave_or(cm);
    m = ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) |
        (u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
    const int lane = threadIdx.x & 63;
    while (m) {  // wave-uniform
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        const unsigned int c = (unsigned int)__popcll(__ballot((cm >> j) & 1ULL));
        if (lane == 0) atomicAdd(&cl[w * 64 + j], c);
    }
}

// one add per (block, source) and one per block for the "anything new" word
__device__ __forceinline__ void flush_counts(const uint32_t* cl, int nwords, const uint32_t& anynew, u64* cnts, u64* tot) {
    __syncthreads();
    for (int t = threadIdx.x; t < nwords * 64; t += blockDim.x)
        if (cl[t]) atomicAdd(&cnts[t], (u64)cl[t]);
    if (threadIdx.x == 0 && anynew) atomicAdd(tot, 1ULL);
}

// One level over the target partition (pair = (source, target), bucket = slice of the target).  Slices are
// 2^tbits ids, those of the query's width W (kLdsWords / W); a last batch narrower than W (NW < W) uses the
// first NW * 2^tbits words of the block's LDS.
template <int NW>
__global__ void __launch_bounds__(kBlock) k_rg_level(ChunkWalk cw, int tbits, int64_t n, const u64* __restrict__ fin,
                                                     u64* __restrict__ seen, u64* __restrict__ fout,
                                                     const uint32_t* __restrict__ bw, int b_full,
                                                     u64* __restrict__ cnts, u64* __restrict__ tot) {
    extern __shared__ u64 rg_next[];  // kLdsWords
    __shared__ uint32_t cl[NW * 64];
    __shared__ uint32_t anynew;
    const int kIds = 1 << tbits;  // >= 2048: a multiple of kBlock
    for (int i = threadIdx.x; i < kIds * NW; i += kBlock) rg_next[i] = 0;
    for (int i = threadIdx.x; i < NW * 64; i += kBlock) cl[i] = 0;
    if (threadIdx.x == 0) anynew = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    part::walk_chunks_n<kBlock>(
        cw,
        [&](const uint2 (&pr)[part::kWalkItems], uint32_t valid, int) {
            constexpr int G = NW >= 8 ? 2 : (NW == 4 ? 4 : 8);  // items whose front words are gathered together
#pragma unroll
            for (int k0 = 0; k0 < part::kWalkItems; k0 += G) {
                u64 f[G][NW];
#pragma unroll
                for (int k = 0; k < G; ++k)
#pragma unroll
                    for (int w = 0; w < NW; ++w) f[k][w] = fin[(size_t)pr[k0 + k].x * NW + w];  // zero pairs read node 0
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    if (!((valid >> (k0 + k)) & 1u)) continue;
                    const uint32_t t = pr[k0 + k].y & (uint32_t)(kIds - 1);
#pragma unroll
                    for (int w = 0; w < NW; ++w)
                        if (f[k][w]) atomicOr(&rg_next[t * NW + w], f[k][w]);
                }
            }
        },
        [&](int j) {
            const bool own = part::owns_slice(cw, j);  // block-uniform
            const int64_t base = (int64_t)j * kIds;
            u64 any = 0;
            for (int i = threadIdx.x; i < kIds; i += kBlock) {  // wave-uniform trips
                const int64_t x = base + i;
                const bool in = x < n;
                const bool bk = in && bit_of(bw, b_full, (uint64_t)x);
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const u64 nx = rg_next[i * NW + w];
                    rg_next[i * NW + w] = 0;
                    if (own) {
                        u64 nv = 0;
                        if (in) {
                            const u64 sn = seen[(size_t)x * NW + w];
                            nv = nx & ~sn;
                            if (nv) seen[(size_t)x * NW + w] = sn | nv;
                            fout[(size_t)x * NW + w] = nv;
                        }
                        any |= nv;
                        count_sources(bk ? nv : 0ULL, w, cl);
                    } else if (nx && in) {
                        atomicOr(&fout[(size_t)x * NW + w], nx);  // k_rg_fix finishes the shared slices
                    }
                }
            }
            if (__any(any != 0) && lane == 0) anynew = 1;
        });
    flush_counts(cl, NW, anynew, cnts, tot);
}

// whether one block of the level kernel's grid holds all of slice j's chunks (part::owns_slice, seen from outside)
__device__ __forceinline__ bool slice_owned(const int64_t* jst, int nt, int64_t blocks, int j) {
    const int64_t c0 = jst[j], c1 = jst[j + 1];
    if (c1 <= c0) return false;  // no relationship enters the slice: no block visits it
    const part::SegSplit S(jst, nt, blocks);
    const int64_t w = c0 / S.per;
    return c1 <= min(w * S.per + S.per, S.nch);
}

// The nodes of the slices that no single block finished (shared by several blocks, or never visited; jst == null:
// every node, the flat form): fout holds their `next` words.  new = next & ~seen, seen |= new, fout = new, and the
// old front is cleared, since no owner overwrites it when it becomes the next level's fout.
template <int NW>
__global__ void __launch_bounds__(256) k_rg_fix(const int64_t* __restrict__ jst, int nt, int64_t blocks, int tbits,
                                                int64_t n,
                                                u64* __restrict__ fin, u64* __restrict__ seen, u64* __restrict__ fout,
                                                const uint32_t* __restrict__ bw, int b_full, u64* __restrict__ cnts,
                                                u64* __restrict__ tot) {
    __shared__ uint32_t cl[NW * 64];
    __shared__ uint32_t anynew;
    for (int i = threadIdx.x; i < NW * 64; i += blockDim.x) cl[i] = 0;
    if (threadIdx.x == 0) anynew = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    u64 any = 0;
    // a wave takes 64 consecutive nodes, all of one slice (slices are multiples of 64 ids): wave-uniform trips
    for (int64_t x0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~(int64_t)63; x0 < n;
         x0 += (int64_t)gridDim.x * blockDim.x) {
        if (jst && slice_owned(jst, nt, blocks, (int)(x0 >> tbits))) continue;
        const int64_t x = x0 + lane;
        const bool in = x < n;
        const bool bk = in && bit_of(bw, b_full, (uint64_t)x);
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            u64 nv = 0;
            if (in) {
                const size_t q = (size_t)x * NW + w;
                const u64 nx = fout[q], sn = seen[q];
                nv = nx & ~sn;
                if (nv) seen[q] = sn | nv;
                if (nx != nv) fout[q] = nv;
                if (fin[q]) fin[q] = 0;
            }
            any |= nv;
            count_sources(bk ? nv : 0ULL, w, cl);
        }
    }
    if (__any(any != 0) && lane == 0) anynew = 1;
    flush_counts(cl, NW, anynew, cnts, tot);
}

// The flat form of a level (domains beyond the sliced path, or CAPSMI_REACH=flat): one global OR per
// relationship and word that brings something new; k_rg_fix (jst == null) finishes every node.
template <int NW, typename IdT>
__global__ void k_rg_level_flat(const IdT* __restrict__ src, const IdT* __restrict__ dst, int64_t m, int64_t lo,
                                uint64_t n, const u64* __restrict__ fin, const u64* __restrict__ seen,
                                u64* __restrict__ fout) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t u = part::rel_id(src[e], lo), v = part::rel_id(dst[e], lo);
        if (u >= n || v >= n) continue;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            u64 f = fin[u * NW + w];
            if (!f) continue;
            f &= ~seen[v * NW + w];
            if (f) atomicOr(&fout[v * NW + w], f);
        }
    }
}

// lower = 0: source j counts itself unless its own bit is in seen[a] and b_ok(a) (then a level counted it)
__global__ void k_rg_zero(const int64_t* __restrict__ idx, int bw, int nwords, const u64* __restrict__ seen,
                          const uint32_t* __restrict__ bwd, int b_full, u64* __restrict__ cnts) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= bw) return;
    const int64_t a = idx[j];
    const bool self = (seen[a * nwords + (j >> 6)] >> (j & 63)) & 1ULL;
    if (!(self && bit_of(bwd, b_full, (uint64_t)a))) cnts[j] += 1;
}

__global__ void k_rg_rowflags(const u64* __restrict__ cnts, int64_t A, uint8_t* __restrict__ f) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < A; i += (int64_t)gridDim.x * blockDim.x)
        f[i] = cnts[i] ? 1 : 0;
}

__global__ void k_rg_rows(const int64_t* __restrict__ sel, int64_t rows, const int64_t* __restrict__ idx, int64_t lo,
                          const u64* __restrict__ cnts, int64_t* __restrict__ ids, int64_t* __restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = sel[r];
        ids[r] = lo + idx[j];
        out[r] = (int64_t)cnts[j];
    }
}

// The early-exit read-back (one 8-byte copy and a stream wait per level) is skipped while it cannot pay: an
// empty frontier saves the levels still to run, and a read-back costs about what one level costs at the
// sizes where levels are cheap.  So no level is checked while at most kNoCheckLevels levels remain after it,
// and a query with upper <= kNoCheckLevels + 1 never waits.
constexpr int kNoCheckLevels = 2;
inline bool check_after(int level, int upper) { return upper - level > kNoCheckLevels; }

template <int NW>
void run_level(capsmi_session* s, bool sliced, int tbits, const ChunkWalk& cw, const ChunkPart& cp, const int64_t* const* srcs,
               const int64_t* const* dsts, const int64_t* ms, int nt, const NarrowRel* nar, int64_t lo, int64_t n,
               int64_t mtot, u64* fin, u64* seen, u64* fout, const uint32_t* bw, int b_full, u64* cnts, u64* tot) {
    hipStream_t st = s->stream;
    const double state = 3.0 * (double)n * NW * 8;
    if (sliced) {
        {
            KernelTimer kt(s, "reach_level", (double)mtot * (8 + NW * 8) + state);
            hipLaunchKernelGGL(k_rg_level<NW>, dim3((unsigned)cp.g2), dim3(kBlock), sizeof(u64) * kLdsWords, st, cw, tbits,
                               n, fin, seen, fout, bw, b_full, cnts, tot);
        }
        KernelTimer kt(s, "reach_final");
        hipLaunchKernelGGL(k_rg_fix<NW>, dim3(grid(s, n)), dim3(256), 0, st, cp.jst, cw.nt, cp.g2, tbits, n, fin, seen, fout,
                           bw, b_full, cnts, tot);
    } else {
        {
            double rel_bytes = 0;
            for (int i = 0; i < nt; ++i)
                if (ms[i] > 0) rel_bytes += (double)ms[i] * (nar && nar[i].s ? 8 : 16);
            KernelTimer kt(s, "reach_level", rel_bytes + (double)mtot * NW * 8);
            for (int i = 0; i < nt; ++i) {
                if (ms[i] <= 0) continue;
                if (nar && nar[i].s)
                    hipLaunchKernelGGL((k_rg_level_flat<NW, uint32_t>), dim3(grid(s, ms[i])), dim3(256), 0, st, nar[i].s,
                                       nar[i].d, ms[i], lo - nar[i].base, (uint64_t)n, fin, seen, fout);
                else
                    hipLaunchKernelGGL((k_rg_level_flat<NW, int64_t>), dim3(grid(s, ms[i])), dim3(256), 0, st, srcs[i],
                                       dsts[i], ms[i], lo, (uint64_t)n, fin, seen, fout);
            }
        }
        KernelTimer kt(s, "reach_final", state);
        hipLaunchKernelGGL(k_rg_fix<NW>, dim3(grid(s, n)), dim3(256), 0, st, (const int64_t*)nullptr, 0, (int64_t)0, 0,
                           n, fin, seen, fout, bw, b_full, cnts, tot);
    }
}

inline int tbits_of(int nwords) { return nwords == 1 ? 14 : nwords == 2 ? 13 : nwords == 4 ? 12 : 11; }

// the largest domain the sliced path takes at `nwords` words: the partition's slice count, and k_varlen's 2^24
inline int64_t sliced_max(int nwords) {
    return std::min<int64_t>(int64_t(1) << 24, (int64_t)part::kMaxTSlices << tbits_of(nwords));
}

}  // namespace reach

namespace reach {
// The BFS of the global form from all of a_ok (n > 0): maps holds the three bitmaps F, R, N of nw words each, R the
// nodes reached in 1..upper relationships; tot[0] counts those of them in b_ok.
void reach_global(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms, int nt,
                  const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int upper, const NarrowRel* nar, Buf& maps,
                  Buf& tot) {
    hipStream_t st = s->stream;
    const int64_t n = b_ok->hi - b_ok->lo, lo = b_ok->lo;
    const int64_t nw = (n + 31) / 32;
    const uint32_t* aw = P<uint32_t>(a_ok->words);
    const uint32_t* bw = P<uint32_t>(b_ok->words);
    const int a_full = a_ok->full ? 1 : 0, b_full = b_ok->full ? 1 : 0;
    maps = dev_alloc(sizeof(uint32_t) * 3 * (size_t)nw, s);
    tot = dev_alloc(2 * sizeof(u64), s);
    uint32_t *F = P<uint32_t>(maps), *R = F + nw, *N = R + nw;
    HIP_CHECK(hipMemsetAsync(P<void>(tot), 0, 2 * sizeof(u64), st));
    hipLaunchKernelGGL(k_rc_init, dim3(grid(s, nw)), dim3(256), 0, st, aw, a_full, n, nw, F, R, N);
    double rel_bytes = 0;
    for (int i = 0; i < nt; ++i)
        if (ms[i] > 0) rel_bytes += (double)ms[i] * (nar && nar[i].s ? 8 : 16);
    int64_t before = 0;
    for (int level = 1; level <= upper; ++level) {
        {
            KernelTimer kt(s, "reach_count_level", rel_bytes);
            for (int i = 0; i < nt; ++i) {
                if (ms[i] <= 0) continue;
                if (nar && nar[i].s)
                    hipLaunchKernelGGL(k_rc_level<uint32_t>, dim3(grid(s, ms[i])), dim3(256), 0, st, nar[i].s, nar[i].d,
                                       ms[i], lo - nar[i].base, (uint64_t)n, F, R, N);
                else
                    hipLaunchKernelGGL(k_rc_level<int64_t>, dim3(grid(s, ms[i])), dim3(256), 0, st, srcs[i], dsts[i],
                                       ms[i], lo, (uint64_t)n, F, R, N);
            }
        }
        {
            KernelTimer kt(s, "reach_count_final", 4.0 * 5 * (double)nw);
            hipLaunchKernelGGL(k_rc_final, dim3(grid(s, nw)), dim3(256), 0, st, nw, N, R, F, bw, b_full, P<u64>(tot));
        }
        if (check_after(level, upper)) {
            const int64_t now = read_scalar(s, P<int64_t>(tot) + 1);
            if (now == before) break;  // nothing new: the frontier is empty
            before = now;
        }
    }
    HIP_CHECK(hipGetLastError());
}
}  // namespace reach

// |U_a D(a)|: one BFS from all of a_ok
int64_t var_length_reach_count(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts,
                               const int64_t* ms, int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower,
                               int upper, const NarrowRel* nar) {
    using namespace reach;
    const int64_t n = b_ok->hi - b_ok->lo;
    if (n <= 0) return 0;
    const int64_t nw = (n + 31) / 32;
    Buf maps, tot;
    reach_global(s, srcs, dsts, ms, nt, a_ok, b_ok, upper, nar, maps, tot);
    if (lower == 0)
        hipLaunchKernelGGL(k_rc_zero, dim3(grid(s, nw)), dim3(256), 0, s->stream, n, nw, P<uint32_t>(maps) + nw,
                           P<uint32_t>(a_ok->words), a_ok->full ? 1 : 0, P<uint32_t>(b_ok->words), b_ok->full ? 1 : 0,
                           P<u64>(tot));
    HIP_CHECK(hipGetLastError());
    return read_scalar(s, P<int64_t>(tot));
}

namespace reach {

// a finished batch of the grouped walk, handed to the caller while its bit matrix is live: the levels and the
// zero-length rule have run, so cnts[base .. base + bwid) are final
struct Batch {
    int64_t base;        // the batch's first source: an index into the source list and the counts
    int bwid, nwords;    // sources of the batch, words per node
    const int64_t* idx;  // the batch's sources (relative ids, ascending)
    u64* seen;           // seen[v * nwords + w]: bit j = source 64 w + j reaches v in 1..upper relationships
    u64 *fa, *fb;        // the two frontier buffers, n * nwords words each, free from here on
};

// The front that the grouped count and the grouped collect share: the source list, the width, the target partition
// and the batch loop.  `after(batch)` runs once per batch, after its levels and k_rg_zero.  Returns the number of
// sources A; idx holds them, cnts their |D(a)| (plus padding).
template <class After>
int64_t reach_batches(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms, int nt,
                      const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper, const NarrowRel* nar,
                      Buf& idx, Buf& cnts, After&& after) {
    hipStream_t st = s->stream;
    const int64_t n = b_ok->hi - b_ok->lo, lo = b_ok->lo;
    const uint32_t* aw = P<uint32_t>(a_ok->words);
    const uint32_t* bw = P<uint32_t>(b_ok->words);
    const int a_full = a_ok->full ? 1 : 0, b_full = b_ok->full ? 1 : 0;
    // the sources in id order (relative ids): the one read-back before the levels
    int64_t A = 0;
    if (n > 0) {
        Buf fl = dev_alloc((size_t)n, s);
        hipLaunchKernelGGL(k_rg_flags, dim3(grid(s, n)), dim3(256), 0, st, aw, a_full, n, P<uint8_t>(fl));
        A = flags_to_indices(s, P<uint8_t>(fl), n, idx);
    }
    if (A == 0) return 0;
    int64_t mtot = 0;
    for (int i = 0; i < nt; ++i) mtot += ms[i] > 0 ? ms[i] : 0;
    // words per node: the knob, or auto: the narrowest width that takes all sources in one
    // batch, up to kMaxWords, halved while the state (3 n W words) exceeds a quarter of the free memory or the
    // domain is beyond the sliced path at that width
    const int64_t need_words = (A + 63) / 64;
    int W = s->cfg.reach_words;
    const bool autow = W == 0;
    if (autow) W = kMaxWords;
    while (W > 1 && W / 2 >= need_words) W /= 2;  // never wider than the sources
    if (autow) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        while (W > 1 && (3.0 * (double)n * W * 8 > (double)free_b / 4 || (n > sliced_max(W) && n <= sliced_max(1)))) W /= 2;
    }
    const bool sliced = !s->cfg.reach_flat && mtot > 0 && n <= sliced_max(W);
    ChunkPart cp;
    ChunkWalk cw{};
    if (sliced) {
        part::Layout L{};
        L.lo = lo;
        L.hi = b_ok->hi;
        L.tbits = tbits_of(W);
        L.nt = (int)((n + (int64_t(1) << L.tbits) - 1) >> L.tbits);
        L.ns = 1;
        L.sbits = 31;
        L.ncells = L.nt;
        {
            KernelTimer kt(s, "reach_part");
            chunk_partition(s, srcs, dsts, ms, nt, false, L, s->num_cus, cp, false, false, nar);
        }
        cw = ChunkWalk{P<uint2>(cp.pool), P<unsigned long long>(cp.meta), cp.order, cp.jst, cp.segbase, cp.ja, L.nt};
        const size_t lds = sizeof(u64) * kLdsWords;
        lds_attr(reinterpret_cast<const void*>(k_rg_level<1>), lds);
        lds_attr(reinterpret_cast<const void*>(k_rg_level<2>), lds);
        lds_attr(reinterpret_cast<const void*>(k_rg_level<4>), lds);
        lds_attr(reinterpret_cast<const void*>(k_rg_level<8>), lds);
    }
    const size_t words = (size_t)n * W;
    Buf state = dev_alloc(sizeof(u64) * 3 * words, s), tot = dev_alloc(sizeof(u64), s);
    cnts = dev_alloc(sizeof(u64) * (size_t)(A + 64 * kMaxWords), s);
    HIP_CHECK(hipMemsetAsync(P<void>(cnts), 0, sizeof(u64) * (size_t)(A + 64 * kMaxWords), st));
    HIP_CHECK(hipMemsetAsync(P<void>(tot), 0, sizeof(u64), st));
    u64 *seen = P<u64>(state), *fa = seen + words, *fb = fa + words;
    int64_t before = 0;
    for (int64_t base = 0; base < A; base += 64 * (int64_t)W) {
        // no batch wider than the sources left: the last one takes the narrowest width that holds them (the
        // slices stay those of W; a narrower batch uses part of the block's LDS)
        const int bwid = (int)std::min<int64_t>(64 * (int64_t)W, A - base);
        int NWb = 1;
        while (NWb * 64 < bwid) NWb *= 2;
        const int64_t bwords = n * NWb;
        hipLaunchKernelGGL(k_zero3, dim3(grid(s, bwords)), dim3(256), 0, st, seen, fa, fb, bwords);
        const int64_t* bidx = P<int64_t>(idx) + base;
        u64* bcnt = P<u64>(cnts) + base;
        hipLaunchKernelGGL(k_rg_init, dim3((bwid + 255) / 256), dim3(256), 0, st, bidx, bwid, NWb, fa);
        u64 *fin = fa, *fout = fb;
        for (int level = 1; level <= upper; ++level) {
            switch (NWb) {
                case 1: run_level<1>(s, sliced, tbits_of(W), cw, cp, srcs, dsts, ms, nt, nar, lo, n, mtot, fin, seen, fout, bw, b_full, bcnt, P<u64>(tot)); break;
                case 2: run_level<2>(s, sliced, tbits_of(W), cw, cp, srcs, dsts, ms, nt, nar, lo, n, mtot, fin, seen, fout, bw, b_full, bcnt, P<u64>(tot)); break;
                case 4: run_level<4>(s, sliced, tbits_of(W), cw, cp, srcs, dsts, ms, nt, nar, lo, n, mtot, fin, seen, fout, bw, b_full, bcnt, P<u64>(tot)); break;
                default: run_level<8>(s, sliced, tbits_of(W), cw, cp, srcs, dsts, ms, nt, nar, lo, n, mtot, fin, seen, fout, bw, b_full, bcnt, P<u64>(tot)); break;
            }
            std::swap(fin, fout);
            if (check_after(level, upper)) {
                const int64_t now = read_scalar(s, P<int64_t>(tot));
                if (now == before) break;  // no block saw a new bit: every frontier of the batch is empty
                before = now;
            }
        }
        if (lower == 0)
            hipLaunchKernelGGL(k_rg_zero, dim3((bwid + 255) / 256), dim3(256), 0, st, bidx, bwid, NWb, seen, bw, b_full, bcnt);
        after(Batch{base, bwid, NWb, bidx, seen, fa, fb});
    }
    HIP_CHECK(hipGetLastError());
    return A;
}

// the rows of the sources with a non-empty D(a): their ids and counts, and (sel) their indices into the source list
int64_t reach_rows_out(capsmi_session* s, const Buf& idx, const Buf& cnts, int64_t A, int64_t lo, Buf& out_ids,
                       Buf& out_cnt, Buf& sel) {
    hipStream_t st = s->stream;
    if (A == 0) {
        out_ids = dev_alloc(8, s);
        out_cnt = dev_alloc(8, s);
        return 0;
    }
    Buf rf = dev_alloc((size_t)A, s);
    hipLaunchKernelGGL(k_rg_rowflags, dim3(grid(s, A)), dim3(256), 0, st, P<u64>(cnts), A, P<uint8_t>(rf));
    const int64_t rows = flags_to_indices(s, P<uint8_t>(rf), A, sel);  // the read-back of the row count
    out_ids = dev_alloc(sizeof(int64_t) * (size_t)(rows > 0 ? rows : 1), s);
    out_cnt = dev_alloc(sizeof(int64_t) * (size_t)(rows > 0 ? rows : 1), s);
    if (rows > 0)
        hipLaunchKernelGGL(k_rg_rows, dim3(grid(s, rows)), dim3(256), 0, st, P<int64_t>(sel), rows, P<int64_t>(idx), lo,
                           P<u64>(cnts), P<int64_t>(out_ids), P<int64_t>(out_cnt));
    HIP_CHECK(hipGetLastError());
    return rows;
}

}  // namespace reach

// rows (a, |D(a)|) of the a_ok nodes with a non-empty D(a); returns the row count
int64_t var_length_reach_rows(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                              int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper,
                              Buf& out_ids, Buf& out_cnt, const NarrowRel* nar) {
    using namespace reach;
    Buf idx, cnts, sel;
    const int64_t A = reach_batches(s, srcs, dsts, ms, nt, a_ok, b_ok, lower, upper, nar, idx, cnts, [](const Batch&) {});
    return reach_rows_out(s, idx, cnts, A, b_ok->lo, out_ids, out_cnt, sel);
}

// ---- collect(DISTINCT b): the reach lists ------------------------------------------------------------------
// D(a) as one strictly ascending id list per source, read off a batch's bit matrix while it is live.  The hit
// matrix hit(v, j) = (bit j of seen[v] and b_ok(v)) or (lower = 0 and v = idx[j]) is written word-major
// (hit[w * n + v]) into a free frontier buffer, so the 64 lanes of a wave read 64 consecutive nodes' words of
// one source word w.  A wave owns a unit: the tile of kListTile consecutive nodes, for one word w, and steps
// through it 64 nodes at a time.  Per set bit j of the wave's OR of its 64 words, the ballot of bit j is the set
// of lanes (nodes) that source 64 w + j reaches: its popcount is the source's count in this step (pass 1), and
// the popcount below a lane is the lane's rank (pass 2).  Lane j keeps the running count of source 64 w + j in a
// register (read by readlane with the wave-uniform j), so the walk needs neither LDS nor atomics, and the element
// order falls out of it: tiles, steps and lanes all ascend in the node id.  Pass 1 leaves one count per (unit,
// lane); a column scan over the tiles turns them into each tile's base per source and each source's length; pass
// 2 repeats the walk from offset + base.  Lengths, offsets and positions all come from the same walk over the
// same words, so a store cannot leave its list.
namespace reach {

constexpr int kListBlock = 256;  // 4 waves, one unit each at a time

__global__ void k_rl_hit(int64_t n, int nwords, const u64* __restrict__ seen, const uint32_t* __restrict__ bw, int b_full,
                         u64* __restrict__ hit) {
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
        const bool bk = bit_of(bw, b_full, (uint64_t)v);
        for (int w = 0; w < nwords; ++w) hit[(size_t)w * n + v] = bk ? seen[(size_t)v * nwords + w] : 0ULL;
    }
}

// lower = 0: source j holds itself (the batch's sources are distinct nodes: one thread per word touched)
__global__ void k_rl_self(const int64_t* __restrict__ idx, int bw, int64_t n, u64* __restrict__ hit) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < bw) hit[(size_t)(j >> 6) * n + idx[j]] |= 1ULL << (j & 63);
}

// Remapped ids (a compacted graph: dense id d holds the original id orig[d], and orig is not monotonic).  The lists
// must ascend in the original ids, and no list element is ever sorted: position p of the hit matrix is taken from
// the node of rank p, by_rank[p], so the walk's ascending positions are ascending original ids and pass 2 stores
// sorted_orig[p].  seen is node-major, so a node's NW words are one stretch of NW * 8 bytes (a 64-byte line at
// NW = 8): a lane reads it whole, at random, and the stores stay coalesced as in k_rl_hit.
template <int NW>
__global__ void k_rl_hit_rank(int64_t n, const u64* __restrict__ seen, const int64_t* __restrict__ by_rank,
                              const uint32_t* __restrict__ bw, int b_full, u64* __restrict__ hit) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t d = (uint64_t)by_rank[p];  // a permutation of [0, n): the payload of the order's sort
        const bool bk = bit_of(bw, b_full, d);
        u64 x[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) x[w] = seen[(size_t)d * NW + w];
#pragma unroll
        for (int w = 0; w < NW; ++w) hit[(size_t)w * n + p] = bk ? x[w] : 0ULL;
    }
}

// lower = 0, remapped: source j's own bit goes to the position of its original id, found by bisection of sorted_orig
// (at most 64 * NW sources per batch, log2 n steps each: no inverse of by_rank is kept).  The sources are distinct
// nodes, so their positions differ: one thread per word touched.
__global__ void k_rl_self_rank(const int64_t* __restrict__ idx, int bw, int64_t n, const int64_t* __restrict__ orig,
                               const int64_t* __restrict__ sorted, u64* __restrict__ hit) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= bw) return;
    const int64_t key = orig[idx[j]];
    int64_t a = 0, b = n;  // the first position whose id is >= key
    while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (sorted[mid] < key) a = mid + 1;
        else b = mid;
    }
    if (a < n && sorted[a] == key) hit[(size_t)(j >> 6) * n + a] |= 1ULL << (j & 63);
}

__device__ __forceinline__ int64_t readlane64(int64_t x, int j) {  // j wave-uniform
    const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, j);
    const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)((u64)x >> 32), j);
    return (int64_t)(((u64)h << 32) | l);
}

// WRITE = false (pass 1): tcol[unit * 64 + j] = nodes of the unit's tile that source 64 w + j holds.
// WRITE = true (pass 2): tcol holds the tile bases; node lo + v goes to vals[offs[source] + base + rank].
// MAP (pass 2 over a rank-ordered hit matrix): position v stands for the original id sorted[v], stored in its place.
template <bool WRITE, bool MAP = false>
__global__ void __launch_bounds__(kListBlock) k_rl_walk(int64_t n, int64_t ntiles, int nwords, int bwid,
                                                        const u64* __restrict__ hit, uint32_t* __restrict__ tcol,
                                                        const int64_t* __restrict__ offs, int64_t lo,
                                                        int64_t* __restrict__ vals,
                                                        const int64_t* __restrict__ sorted = nullptr) {
    const int lane = threadIdx.x & 63;
    const int64_t units = ntiles * nwords;
    for (int64_t u = (int64_t)blockIdx.x * (kListBlock / 64) + (threadIdx.x >> 6); u < units;
         u += (int64_t)gridDim.x * (kListBlock / 64)) {  // wave-uniform
        const int64_t tile = u / nwords;
        const int w = (int)(u - tile * nwords);
        // lane j: pass 1, the running count of source 64 w + j; pass 2, where its next element goes
        int64_t pos = 0;
        if (WRITE) pos = (w * 64 + lane < bwid ? offs[w * 64 + lane] : 0) + (int64_t)tcol[u * 64 + lane];
        const u64* hw = hit + (size_t)w * n;
        for (int step = 0; step < kListTile / 64; ++step) {
            const int64_t v = tile * kListTile + step * 64 + lane;
            const u64 x = v < n ? hw[v] : 0ULL;
            if (!__any(x != 0)) continue;
            int64_t val = lo + v;
            if (MAP) val = x ? sorted[v] : 0;  // x != 0 only below n
            u64 m = wave_or(x);
            m = ((u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) |
                (u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
            while (m) {  // wave-uniform
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                const bool on = (x >> j) & 1ULL;
                const u64 bal = __ballot(on);
                if (WRITE) {
                    const int64_t p = readlane64(pos, j);
                    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
                    if (on) vals[p + below] = val;
                }
                if (lane == j) pos += __popcll(bal);
            }
        }
        if (!WRITE) tcol[u * 64 + lane] = (uint32_t)pos;
    }
}

// per source column t of the batch: tcol[tile][t] becomes the count of the tiles before, lens[t] the total
__global__ void k_rl_colscan(int64_t ntiles, int ncols, int bwid, uint32_t* __restrict__ tcol, int64_t* __restrict__ lens) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncols) return;
    uint32_t acc = 0;
    for (int64_t i = 0; i < ntiles; ++i) {
        const uint32_t c = tcol[i * ncols + t];
        tcol[i * ncols + t] = acc;
        acc += c;
    }
    if (t < bwid) lens[t] = (int64_t)acc;
}

// global form: word i of the answer = R & b_ok, with a_ok for lower = 0; cnt[i] its bits
__global__ void k_rc_listwords(int64_t n, int64_t nw, const uint32_t* __restrict__ R, const uint32_t* __restrict__ aw,
                               int a_full, const uint32_t* __restrict__ bw, int b_full, int lower, uint32_t* __restrict__ out,
                               int64_t* __restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t left = n - 32 * i;
        const uint32_t in = left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u);
        uint32_t x = R[i] & (b_full ? 0xFFFFFFFFu : bw[i]);
        if (lower == 0) x |= a_full ? 0xFFFFFFFFu : aw[i];
        x &= in;
        out[i] = x;
        cnt[i] = __popc(x);
    }
}

// MAP: the words are in rank order (k_rc_rank) and bit p stands for the original id sorted[p]
template <bool MAP>
__global__ void k_rc_listwrite(int64_t nw, const uint32_t* __restrict__ words, const int64_t* __restrict__ offs, int64_t lo,
                               int64_t* __restrict__ vals, const int64_t* __restrict__ sorted) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nw; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t x = words[i];
        int64_t o = offs[i];
        while (x) {
            const int64_t p = 32 * i + (__ffs((int)x) - 1);
            vals[o++] = MAP ? sorted[p] : lo + p;
            x &= x - 1;
        }
    }
}

// global form, remapped ids: the answer's bitmap from dense order into rank order, bit p of the output = bit
// by_rank[p] of the input.  A wave takes 64 consecutive positions: one ballot, and lane 0 stores the 64-bit word
// (two of the 32-bit words that the count, scan and write passes walk) and lanes 0 and 1 its halves' bit counts.
// out has 2 * ceil(n / 64) 32-bit words; cnt has nw = ceil(n / 32), so the last odd half has no count to store.
__global__ void __launch_bounds__(256) k_rc_rank(int64_t n, int64_t nw, const uint32_t* __restrict__ words,
                                                 const int64_t* __restrict__ by_rank, u64* __restrict__ out,
                                                 int64_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t nw64 = (n + 63) >> 6;
    for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < nw64;
         i += ((int64_t)gridDim.x * blockDim.x) >> 6) {  // wave-uniform
        const int64_t p = i * 64 + lane;
        bool on = false;
        if (p < n) {
            const uint64_t d = (uint64_t)by_rank[p];
            on = (words[d >> 5] >> (d & 31)) & 1u;
        }
        const u64 bal = __ballot(on);
        if (lane == 0) out[i] = bal;
        if (lane < 2 && 2 * i + lane < nw) cnt[2 * i + lane] = __popc((uint32_t)(bal >> (32 * lane)));
    }
}

// sorted keys (the order-preserving image of the ids) back to ids
__global__ void k_ro_unkey(int64_t n, uint64_t* __restrict__ key) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        key[i] ^= 0x8000000000000000ULL;
}

__global__ void k_ro_dup(int64_t n, const uint64_t* __restrict__ key, int64_t* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (key[i] == key[i - 1]) *flag = 1;  // every writer stores the same word
}

// CAPSMI_REACH_LIST_LIMIT in elements; auto: what fits the device's memory at the 16 B per element of the peak (the
// batches' buffers and the joined store side by side)
inline int64_t list_limit(capsmi_session* s) {
    if (s->cfg.reach_list_limit > 0) return s->cfg.reach_list_limit;
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    return (int64_t)(total_b / 16);
}

inline void check_list_limit(int64_t elems, int64_t limit) {
    REQUIRE(elems <= limit, CAPSMI_ERR_UNSUPPORTED,
            "var-length collect(DISTINCT b): the lists reach " + std::to_string(elems) +
                " elements, above CAPSMI_REACH_LIST_LIMIT = " + std::to_string(limit));
}

}  // namespace reach

// rows (a, |D(a)|, D(a)) of the a_ok nodes with a non-empty D(a): list k of the store is D of source k (empty lists
// included, which no row names), out_sel the rows' list indices
int64_t var_length_reach_lists(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                               int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper,
                               Buf& out_ids, Buf& out_cnt, Buf& out_sel, std::shared_ptr<ListStore>& lists,
                               const NarrowRel* nar, const int64_t* orig, const IdOrder* ord) {
    using namespace reach;
    hipStream_t st = s->stream;
    const int64_t n = b_ok->hi - b_ok->lo, lo = b_ok->lo;
    REQUIRE(n < (int64_t(1) << 32), CAPSMI_ERR_UNSUPPORTED, "var-length collect(DISTINCT b): at most 2^32 - 1 ids");
    REQUIRE(!ord || (orig && ord->n == n), CAPSMI_ERR_INTERNAL, "var-length collect(DISTINCT b): the id order is not the domain's");
    const int64_t* by_rank = ord ? P<int64_t>(ord->by_rank) : nullptr;
    const int64_t* sorted = ord ? P<int64_t>(ord->sorted_orig) : nullptr;
    const int64_t limit = list_limit(s);
    const uint32_t* bw = P<uint32_t>(b_ok->words);
    const int b_full = b_ok->full ? 1 : 0;
    const int64_t ntiles = (n + kListTile - 1) / kListTile;
    Buf tcol = dev_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(ntiles, 1) * 64 * kMaxWords, s);
    Buf boffs = dev_alloc(sizeof(int64_t) * (64 * kMaxWords + 1), s);
    Buf lens;  // int64 per source, sized once the sources are known
    std::vector<std::pair<Buf, int64_t>> parts;  // a values buffer per batch
    int64_t total = 0;
    Buf idx, cnts;
    const int64_t A = reach_batches(s, srcs, dsts, ms, nt, a_ok, b_ok, lower, upper, nar, idx, cnts, [&](const Batch& b) {
        if (!lens) lens = dev_alloc(sizeof(int64_t) * (size_t)n, s);  // at most n sources
        const int64_t units = ntiles * b.nwords;
        const int wgrid = (int)std::min<int64_t>((units + kListBlock / 64 - 1) / (kListBlock / 64), (int64_t)s->num_cus * 32);
        const double hit_bytes = (double)n * b.nwords * 8, col_bytes = (double)units * 64 * 4;
        int64_t* blen = P<int64_t>(lens) + b.base;
        if (ord) {  // the hit matrix in rank order: n ranks and n * W words read (by node lines), n * W words written
            {
                KernelTimer kt(s, "reach_list_gather", 2.0 * hit_bytes + 8.0 * (double)n);
                const dim3 g(grid(s, n)), t(256);
                switch (b.nwords) {
                    case 1: hipLaunchKernelGGL(k_rl_hit_rank<1>, g, t, 0, st, n, b.seen, by_rank, bw, b_full, b.fa); break;
                    case 2: hipLaunchKernelGGL(k_rl_hit_rank<2>, g, t, 0, st, n, b.seen, by_rank, bw, b_full, b.fa); break;
                    case 4: hipLaunchKernelGGL(k_rl_hit_rank<4>, g, t, 0, st, n, b.seen, by_rank, bw, b_full, b.fa); break;
                    default: hipLaunchKernelGGL(k_rl_hit_rank<8>, g, t, 0, st, n, b.seen, by_rank, bw, b_full, b.fa); break;
                }
            }
            if (lower == 0) {
                KernelTimer kt(s, "reach_list_starts");
                hipLaunchKernelGGL(k_rl_self_rank, dim3((b.bwid + 255) / 256), dim3(256), 0, st, b.idx, b.bwid, n, orig,
                                   sorted, b.fa);
            }
        } else {
            KernelTimer kt(s, "reach_list_starts");
            hipLaunchKernelGGL(k_rl_hit, dim3(grid(s, n)), dim3(256), 0, st, n, b.nwords, b.seen, bw, b_full, b.fa);
            if (lower == 0)
                hipLaunchKernelGGL(k_rl_self, dim3((b.bwid + 255) / 256), dim3(256), 0, st, b.idx, b.bwid, n, b.fa);
        }
        {
            KernelTimer kt(s, "reach_list_count", hit_bytes + col_bytes);
            hipLaunchKernelGGL(k_rl_walk<false>, dim3(wgrid), dim3(kListBlock), 0, st, n, ntiles, b.nwords, b.bwid, b.fa,
                               P<uint32_t>(tcol), (const int64_t*)nullptr, lo, (int64_t*)nullptr, (const int64_t*)nullptr);
        }
        {
            KernelTimer kt(s, "reach_list_starts");
            hipLaunchKernelGGL(k_rl_colscan, dim3(b.nwords), dim3(64), 0, st, ntiles, b.nwords * 64, b.bwid,
                               P<uint32_t>(tcol), blen);
            exclusive_scan_i64(blen, P<int64_t>(boffs), b.bwid, s);
        }
        HIP_CHECK(hipGetLastError());
        const int64_t elems = read_scalar(s, P<int64_t>(boffs) + b.bwid);  // the batch's total: 8 bytes back
        check_list_limit(total + elems, limit);                            // before the batch is written
        Buf vals = dev_alloc(sizeof(int64_t) * (size_t)(elems > 0 ? elems : 1), s);
        if (elems > 0) {
            KernelTimer kt(s, "reach_list_write", 8.0 * (double)elems + hit_bytes + col_bytes + (ord ? 8.0 * (double)n : 0));
            if (ord)
                hipLaunchKernelGGL((k_rl_walk<true, true>), dim3(wgrid), dim3(kListBlock), 0, st, n, ntiles, b.nwords, b.bwid,
                                   b.fa, P<uint32_t>(tcol), P<int64_t>(boffs), lo, P<int64_t>(vals), sorted);
            else
                hipLaunchKernelGGL(k_rl_walk<true>, dim3(wgrid), dim3(kListBlock), 0, st, n, ntiles, b.nwords, b.bwid, b.fa,
                                   P<uint32_t>(tcol), P<int64_t>(boffs), lo, P<int64_t>(vals), (const int64_t*)nullptr);
        }
        parts.emplace_back(vals, elems);
        total += elems;
    });
    int64_t rows = 0;
    if (ord) {  // the sources' dense indices, then their original ids
        Buf dense_ids;
        rows = reach_rows_out(s, idx, cnts, A, 0, dense_ids, out_cnt, out_sel);
        out_ids = dev_alloc(sizeof(int64_t) * (size_t)(rows > 0 ? rows : 1), s);
        if (rows > 0) gather_col(orig, nullptr, P<int64_t>(dense_ids), rows, P<int64_t>(out_ids), nullptr, st);
    } else {
        rows = reach_rows_out(s, idx, cnts, A, lo, out_ids, out_cnt, out_sel);
    }
    if (!out_sel) out_sel = dev_alloc(8, s);
    auto L = std::make_shared<ListStore>();
    L->elem = CAPSMI_I64;
    L->nlists = A;
    L->nvalues = total;
    L->offsets = dev_alloc(sizeof(int64_t) * (size_t)(A + 1), s);
    if (A > 0) {
        KernelTimer kt(s, "reach_list_starts");
        exclusive_scan_i64(P<int64_t>(lens), P<int64_t>(L->offsets), A, s);
    } else {
        HIP_CHECK(hipMemsetAsync(P<void>(L->offsets), 0, sizeof(int64_t), st));
    }
    if (parts.size() == 1) {
        L->values = parts[0].first;  // one batch: its buffer is the store
    } else {
        L->values = dev_alloc(sizeof(int64_t) * (size_t)(total > 0 ? total : 1), s);
        int64_t at = 0;
        for (auto& p : parts) {  // batch order is source order: the joined values follow the offsets
            if (p.second)
                HIP_CHECK(hipMemcpyAsync(P<int64_t>(L->values) + at, P<int64_t>(p.first), sizeof(int64_t) * (size_t)p.second,
                                         hipMemcpyDeviceToDevice, st));
            at += p.second;
        }
    }
    lists = L;
    return rows;
}

// the ascending ids of U_a D(a) (returns their number)
int64_t var_length_reach_list(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                              int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper,
                              Buf& out_vals, const NarrowRel* nar, const IdOrder* ord) {
    using namespace reach;
    hipStream_t st = s->stream;
    const int64_t n = b_ok->hi - b_ok->lo, lo = b_ok->lo;
    if (n <= 0) {
        out_vals = dev_alloc(8, s);
        return 0;
    }
    const int64_t limit = list_limit(s);
    const int64_t nw = (n + 31) / 32;
    Buf maps, tot;
    reach_global(s, srcs, dsts, ms, nt, a_ok, b_ok, upper, nar, maps, tot);
    REQUIRE(!ord || ord->n == n, CAPSMI_ERR_INTERNAL, "var-length collect(DISTINCT b): the id order is not the domain's");
    uint32_t *F = P<uint32_t>(maps), *R = F + nw;  // F is free after the levels: it takes the answer's words
    Buf cnt = dev_alloc(sizeof(int64_t) * (size_t)nw, s), offs = dev_alloc(sizeof(int64_t) * (size_t)(nw + 1), s);
    int64_t elems = 0;
    Buf ranked;  // remapped ids: the answer's words in rank order
    {
        KernelTimer kt(s, "reach_list_starts");
        hipLaunchKernelGGL(k_rc_listwords, dim3(grid(s, nw)), dim3(256), 0, st, n, nw, R, P<uint32_t>(a_ok->words),
                           a_ok->full ? 1 : 0, P<uint32_t>(b_ok->words), b_ok->full ? 1 : 0, lower, F, P<int64_t>(cnt));
        if (!ord) exclusive_scan_i64(P<int64_t>(cnt), P<int64_t>(offs), nw, s);
    }
    if (ord) {
        const int64_t nw64 = (n + 63) / 64;
        ranked = dev_alloc(sizeof(u64) * (size_t)nw64, s);
        {
            KernelTimer kt(s, "reach_list_gather", 8.0 * (double)n + 4.0 * (double)nw + 8.0 * (double)nw64 + 8.0 * (double)nw);
            hipLaunchKernelGGL(k_rc_rank, dim3(grid(s, n)), dim3(256), 0, st, n, nw, F, P<int64_t>(ord->by_rank),
                               P<u64>(ranked), P<int64_t>(cnt));
        }
        KernelTimer kt(s, "reach_list_starts");
        exclusive_scan_i64(P<int64_t>(cnt), P<int64_t>(offs), nw, s);
    }
    HIP_CHECK(hipGetLastError());
    elems = read_scalar(s, P<int64_t>(offs) + nw);
    check_list_limit(elems, limit);
    out_vals = dev_alloc(sizeof(int64_t) * (size_t)(elems > 0 ? elems : 1), s);
    if (elems > 0) {
        KernelTimer kt(s, "reach_list_write", 8.0 * (double)elems + 12.0 * (double)nw);
        if (ord)
            hipLaunchKernelGGL(k_rc_listwrite<true>, dim3(grid(s, nw)), dim3(256), 0, st, nw, P<uint32_t>(ranked),
                               P<int64_t>(offs), lo, P<int64_t>(out_vals), P<int64_t>(ord->sorted_orig));
        else
            hipLaunchKernelGGL(k_rc_listwrite<false>, dim3(grid(s, nw)), dim3(256), 0, st, nw, F, P<int64_t>(offs), lo,
                               P<int64_t>(out_vals), (const int64_t*)nullptr);
    }
    HIP_CHECK(hipGetLastError());
    return elems;
}

// The signed order of n original ids: ORDER BY's key image of a Long (the sign bit flipped) under the 64-bit radix
// sort, the dense index as the payload.
std::shared_ptr<const IdOrder> id_order_build(capsmi_session* s, const int64_t* orig, int64_t n, bool* dup) {
    using namespace reach;
    hipStream_t st = s->stream;
    auto o = std::make_shared<IdOrder>();
    o->n = n;
    o->sorted_orig = dev_alloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1), s);
    o->by_rank = dev_alloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1), s);
    if (dup) *dup = false;
    if (n <= 0) return o;
    uint64_t* key = P<uint64_t>(o->sorted_orig);
    Buf flag;
    {
        KernelTimer kt(s, "reach_list_order", 16.0 * (double)n);
        iota_i64(P<int64_t>(o->by_rank), 0, n, st);
        order_keys(s, orig, nullptr, CAPSMI_I64, false, false, P<int64_t>(o->by_rank), n, key);
        radix_sort_pairs(s, key, P<int64_t>(o->by_rank), n, 0, 64);
        if (dup) {
            flag = dev_alloc(sizeof(int64_t), s);
            HIP_CHECK(hipMemsetAsync(P<void>(flag), 0, sizeof(int64_t), st));
            hipLaunchKernelGGL(k_ro_dup, dim3(grid(s, n)), dim3(256), 0, st, n, key, P<int64_t>(flag));
        }
        hipLaunchKernelGGL(k_ro_unkey, dim3(grid(s, n)), dim3(256), 0, st, n, key);
    }
    HIP_CHECK(hipGetLastError());
    if (dup) *dup = read_scalar(s, P<int64_t>(flag)) != 0;
    return o;
}

}  // namespace capsmi
