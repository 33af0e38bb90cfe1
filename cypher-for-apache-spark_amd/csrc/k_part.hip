// k_part.hip -- 2-D radix-partitioned relationship layout and LDS-resident 2-hop kernels.
//
// The 2-hop count(DISTINCT c) touches two id-indexed bitmaps per relationship: the frontier of
// the middle node (indexed by source) and the mark of the end node (indexed by target).  Over
// 2^26 ids each is 8 MiB, twice an XCD's L2, so in ingest order both are random cache traffic
// (the streaming kernels in k_graph.hip run at ~1/8 of HBM bandwidth for that reason).
//
// Layout: relationships are grouped into cells (target slice j, source slice i), j-major.  A
// target slice is 2^19 ids, whose bitmap (64 KiB) a workgroup keeps in LDS while it streams the
// slice's cells, so marks are LDS atomics; a source slice is 2^19 ids too when the domain allows
// (<= 128 x 128 cells), so a workgroup also pulls the frontier slice (64 KiB, from L2/MALL) into
// LDS before a large cell and every frontier test is an LDS read.  Target-side node filters
// (b_ok / c_ok) commute with the OR over relationships and are applied word-wise when a target
// slice is flushed, so the per-relationship work is one 8-byte load and two LDS accesses.
//
// Build: pass 0 counts cells (LDS histogram), pass 1 scatters (source, target) int64 pairs into
// target slices as packed uint32 pairs, pass 2 scatters each target slice into its source cells.
// Both scatters stage an 8192-relationship tile in LDS grouped by bucket, so the HBM writes are
// runs of whole cache lines rather than 8-byte scatters.  A cold 2-hop with a full a_ok over at most
// 2^26 ids stops after pass 1 and runs both hops over the pass-1 pool (k_pool_hop1 / k_pool_hop2);
// pass 2 is then the second stage of the build (relpart_cells), run only when something reads the cells.
#include <map>
#include <mutex>
#include "part_common.h"
#include "presence_rule.h"

namespace capsmi {

namespace part {
// Cache policies measured at C3 (round 6, alternating libraries on one box; default policy everywhere else):
// non-temporal pass-1 loads 5.23 -> 5.50 ms, non-temporal pass-1 stores 5.23 -> 5.28, non-temporal pass-2 chunk
// loads 3.56 -> 3.60 (hop 2 1.49 -> 1.61), non-temporal pass-2 layout stores 3.56 -> 3.69 with hop 2 1.49 -> 1.36
// (the step unchanged).  The hops' pair loads stay non-temporal.

// ---- pass 1: int64 (source, target) -> packed pairs in per-workgroup chunks of one target slice ------
//
// No counting pass: every workgroup keeps one open chunk (kCh pairs) per target slice and appends
// its tiles' runs to it; a full chunk is retired and the next one taken from the workgroup's own
// range of the pool (a block with T tiles fills at most T chunks and leaves at most one open per
// slice, so T + nt chunks suffice and no global atomic sits in the tile loop).  Chunk metadata
// records (slice, fill); fill 0 = unused.  With HIST each open chunk also counts its pairs per source
// slice (16-bit LDS counters, nt x ns of them = one per 2-D cell), written out as the chunk's cell
// histogram when it is retired; pass 2 derives exact output offsets from those.  Callers whose
// consumers walk the pool (the cold 2-hop's pool hops, C5's partitions) run HIST = false, and a pool
// that comes to need the rows after all gets them from k_chunk_hist.  The next tile's loads are
// issued before this tile is regrouped and written.



__host__ __device__ constexpr size_t scatter1_lds(int nb, int ns, bool hist, int block = kP1Block, int tile = kP1Tile) {
    return sizeof(uint2) * tile +
           sizeof(uint32_t) * ((hist ? (size_t)nb * hist_words(ns) : 0) + 7 * (size_t)nb + block / 64 + 4);
}

// chunks per pass-1 block: tiles of the busiest block + one open chunk per slice
__host__ __device__ inline int64_t chunks_per_block(int64_t m, int64_t grid, int nt, int64_t tile = kP1Tile) {
    return ((m + tile - 1) / tile + grid - 1) / grid + nt;
}

__device__ __forceinline__ void hist_add(uint32_t* H, int hw, int b, uint32_t i) {
    atomicAdd(&H[b * hw + (int)(i >> 1)], 1u << ((i & 1u) * 16u));
}

// HIST = false: no cell counts (no H, no chist rows); k_chunk_hist makes the rows when something asks for them
// IdT: int64_t columns, or uint32_t for their narrow copies (then L is the window shifted by the copies' base)
template <int B, int IT, int MINW, bool NTS, bool HIST, typename IdT = int64_t>  // MINW: waves per SIMD to fit
__global__ void __launch_bounds__(B, MINW) k_scatter_c(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                       int64_t m, Layout L, int swap, int64_t chunk0, size_t trash,
                                                       uint2* __restrict__ pool, unsigned long long* __restrict__ cmeta,
                                                       uint32_t* __restrict__ chist) {
    constexpr int T = B * IT;
    static_assert(T <= kCh, "a pass-1 run must span at most two chunks");
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const int nb = L.nt, hw = hist_words(L.ns);
    uint2* stage = reinterpret_cast<uint2*>(smem);
    uint32_t* H = reinterpret_cast<uint32_t*>(stage + T);  // nb rows of hw words: open chunks' cell counts
    uint32_t* cnt = H + (HIST ? (size_t)nb * hw : 0);  // this tile's run length per slice
    uint32_t* loc = cnt + nb;             // run start in the stage
    uint32_t* ph = loc + nb;              // open chunk per slice (kNone: none yet) ...
    uint32_t* fl = ph + nb;               // ... and its fill, both as of the start of the tile
    uint32_t* p1 = fl + nb;               // chunk opened by this tile's run (kNone: the run fits)
    uint32_t* opened = p1 + nb;           // slices that opened a chunk in this tile
    uint32_t* wtot = opened + nb;
    uint32_t* misc = wtot + B / 64;  // [0] chunks opened this tile, [1] next free chunk
    if (HIST)
        for (int i = threadIdx.x; i < nb * hw; i += B) H[i] = 0;
    for (int i = threadIdx.x; i < nb; i += B) {
        ph[i] = kNone;
        fl[i] = 0;
    }
    if (threadIdx.x == 0) {
        misc[0] = 0;
        misc[1] = (uint32_t)(chunk0 + (int64_t)blockIdx.x * chunks_per_block(m, gridDim.x, nb, T));
    }
    const uint64_t range = (uint64_t)(L.hi - L.lo);
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int64_t stride = (int64_t)gridDim.x * T;
    IdT sr[IT], tr[IT];
    int64_t t0 = (int64_t)blockIdx.x * T;
    if (t0 < m) load_tile<B>(src, dst, t0, m, vec, sr, tr);
    for (; t0 < m; t0 += stride) {  // block-uniform
        for (int i = threadIdx.x; i < nb; i += B) cnt[i] = 0;
        __syncthreads();
        uint2 pr[IT];
        uint32_t rk[IT];
        uint32_t valid = 0;
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int64_t e = t0 + tile_item_off<B, IdT>(u);
            const uint64_t s = rel_id(sr[u], L.lo), t = rel_id(tr[u], L.lo);
            const bool ok = e < m && s < range && t < range;
            pr[u] = swap ? make_uint2((uint32_t)t, (uint32_t)s) : make_uint2((uint32_t)s, (uint32_t)t);
            valid |= (ok ? 1u : 0u) << u;
            rk[u] = 0;
        }
        if (t0 + stride < m) load_tile<B>(src, dst, t0 + stride, m, vec, sr, tr);  // prefetch
#pragma unroll
        for (int u = 0; u < IT; ++u)
            if ((valid >> u) & 1u) rk[u] = atomicAdd(&cnt[pr[u].y >> L.tbits], 1u);
        __syncthreads();
        const uint32_t total = block_exclusive_scan<B>(cnt, loc, nb, wtot);
        const uint32_t nf = misc[1];
        for (int i = threadIdx.x; i < nb; i += B) {  // a run that does not fit opens a chunk
            const uint32_t c = cnt[i];
            uint32_t np = kNone;
            if (c && (ph[i] == kNone || fl[i] + c > (uint32_t)kCh)) {
                const uint32_t k = atomicAdd(&misc[0], 1u);
                np = nf + k;
                opened[k] = (uint32_t)i;
            }
            p1[i] = np;
        }
#pragma unroll
        for (int u = 0; u < IT; ++u)
            if ((valid >> u) & 1u) stage[loc[pr[u].y >> L.tbits] + rk[u]] = pr[u];
        __syncthreads();
        // run item r of slice b: r < room -> open chunk ph[b] at fl[b] + r, else the opened chunk p1[b]
#pragma unroll
        for (int k = 0; k < IT; ++k) {  // unconditional stores (idx >= total -> trash chunk)
            const uint32_t idx = (uint32_t)(k * B + (int)threadIdx.x);
            const uint2 p = stage[idx];
            const int b = min((int)(p.y >> L.tbits), nb - 1);  // stale stage entries past `total`
            const uint32_t r = idx - loc[b], o = ph[b], room = o == kNone ? 0u : (uint32_t)kCh - fl[b];
            const bool first = r < room;
            if (HIST && idx < total && first) hist_add(H, hw, b, p.x >> L.sbits);
            const size_t at = idx >= total ? trash + threadIdx.x
                            : first       ? (size_t)o * kCh + fl[b] + r
                                          : (size_t)p1[b] * kCh + (r - room);
            if (NTS)
                __builtin_nontemporal_store(*reinterpret_cast<const unsigned long long*>(&p),
                                            reinterpret_cast<unsigned long long*>(pool + at));
            else
                pool[at] = p;
        }
        const uint32_t nop = misc[0];
        if (HIST && nop) {  // block-uniform: retire the filled chunks (histogram row out), count the runs' tails
            __syncthreads();
            for (uint32_t x = threadIdx.x; x < nop * (uint32_t)hw; x += B) {
                const int b = (int)opened[x / hw], w = (int)(x % hw);
                if (ph[b] != kNone) {
                    chist[(size_t)ph[b] * hw + w] = H[b * hw + w];
                    H[b * hw + w] = 0;
                }
            }
            __syncthreads();
            for (uint32_t k = 0; k < nop; ++k) {
                const int b = (int)opened[k];
                const uint32_t room = ph[b] == kNone ? 0u : (uint32_t)kCh - fl[b];
                for (uint32_t r = room + threadIdx.x; r < cnt[b]; r += B)
                    hist_add(H, hw, b, stage[loc[b] + r].x >> L.sbits);
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += B) {  // advance the open chunks
            const uint32_t c = cnt[i];
            if (!c) continue;
            if (p1[i] == kNone) {
                fl[i] += c;
            } else {
                if (ph[i] != kNone) cmeta[ph[i]] = chunk_meta(i, (uint32_t)kCh);
                fl[i] = ph[i] == kNone ? c : fl[i] + c - (uint32_t)kCh;
                ph[i] = p1[i];
            }
        }
        if (threadIdx.x == 0) {
            misc[1] += misc[0];
            misc[0] = 0;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += B)
        if (ph[i] != kNone) cmeta[ph[i]] = chunk_meta(i, fl[i]);
    if (HIST)
        for (int x = threadIdx.x; x < nb * hw; x += B) {
            const uint32_t p = ph[x / hw];
            if (p != kNone) chist[(size_t)p * hw + x % hw] = H[x];
        }
}

// ---- pass 1, whole-line variant (used when its LDS fits: <= 128 target slices at 2^19 ids) -------
// The chunk bookkeeping of a tile (scan of the run lengths, chunks opened) and the deferred part of
// the previous tile (retiring the chunks it filled, the histogram counts of its runs' tails,
// advancing the open chunks) run in wave 0 between the ranking and the regroup; run lengths are
// double-buffered by tile parity, so a tile takes three barriers.

// orders one wave's LDS accesses (wave 0 runs the bookkeeping alone)
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// This lane's index for wave 0's bookkeeping (p1l_settle, p1l_plan), opaque to the optimiser.  From a plain
// `threadIdx.x & 63` the per-lane constants of the bookkeeping loops (slice ranges, LDS addresses) are hoisted out
// of the tile loop, where the prefetched tile and the tile being ranked leave them no registers: they were
// spilled (36 B of scratch per lane), and every reload inside wave 0's section waited on vmcnt, in order, behind
// the next tile's loads, with 15 waves at the barrier.  Recomputed per tile they cost a few VALU instructions,
// the kernel has no scratch and wave 0's section waits for no vector memory.
__device__ __forceinline__ int p1l_lane() {
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    return lane;
}

// Pass 1 writing whole 128-byte lines only.  A slice's run is appended behind the items its open
// chunk still holds back (fewer than kLine, kept in LDS): the combined sequence is staged, every
// complete line of it is stored, and the tail is held back again.  A line is then written once,
// by one wave, instead of in two pieces by two tiles, which the L2 may write back separately.
// The chunk contents and histograms equal k_scatter_c's up to the order within a chunk.
// With SPLIT the chunk is the split pool's two word arrays (part_common.h) and a whole line is 32 pairs in each.
constexpr int kLine = 16;       // pairs per 128-byte line
constexpr int kLineSplit = 32;  // words per 128-byte line of the split pool's arrays
__host__ __device__ constexpr int p1_line(bool split) { return split ? kLineSplit : kLine; }
constexpr int kStageGroup = 4;  // staged pairs per lane and step of the split pool's store loop (two 16-byte stores)
__host__ __device__ constexpr int p1_pad(bool split) { return split ? kStageGroup : 0; }

template <int LN>
__device__ __forceinline__ uint32_t held(uint32_t o, uint32_t f) { return o == kNone ? 0u : (f & (LN - 1)); }

// wave 0: retire the chunks the previous tile filled, add its runs' tails to the opened chunks'
// histogram rows (HIST), advance the open chunks and clear the previous run lengths `cp`
template <bool HIST, int LN>
__device__ __forceinline__ void p1l_settle(const Layout& L, int hw, const uint2* stage, uint32_t* H, uint32_t* cp,
                                           const uint32_t* loc, uint32_t* ph, uint32_t* fl, const uint32_t* p1,
                                           const uint32_t* opened, uint32_t* misc, unsigned long long* cmeta,
                                           uint32_t* chist) {
    const int nb = L.nt, lane = p1l_lane();
    const uint32_t nop = misc[0];
    if (HIST) {
        for (uint32_t x = lane; x < nop * (uint32_t)hw; x += 64) {
            const int b = (int)opened[x / hw], w = (int)(x % hw);
            if (ph[b] != kNone) {
                chist[(size_t)ph[b] * hw + w] = H[b * hw + w];
                H[b * hw + w] = 0;
            }
        }
        wave_lds_order();
        for (uint32_t k = 0; k < nop; ++k) {  // items past the old chunk's room belong to the opened one
            const int b = (int)opened[k];
            const uint32_t h = held<LN>(ph[b], fl[b]);
            const uint32_t room = ph[b] == kNone ? 0u : (uint32_t)kCh - (fl[b] - h);
            for (uint32_t r = room + lane; r < h + cp[b]; r += 64) hist_add(H, hw, b, stage[loc[b] + r].x >> L.sbits);
        }
        wave_lds_order();
    }
    for (int i = lane; i < nb; i += 64) {
        const uint32_t c = cp[i];
        if (!c) continue;
        if (p1[i] == kNone) {
            fl[i] += c;
        } else {
            if (ph[i] != kNone) cmeta[ph[i]] = chunk_meta(i, (uint32_t)kCh);
            fl[i] = ph[i] == kNone ? c : fl[i] + c - (uint32_t)kCh;
            ph[i] = p1[i];
        }
        cp[i] = 0;
    }
    if (lane == 0) {
        misc[1] += nop;
        misc[0] = 0;
    }
    wave_lds_order();
}

// What the regroup and the store loop need per slice, worked out once per tile by wave 0 instead of per item
// from loc / ph / fl / cn / p1.  Staged item r of slice b (r = index - loc) goes to logical position w + r of
// the open chunk (w = its written prefix) while r < room, else to position r - room of the opened chunk;
// positions below the landing chunk's last complete line (cut) are stored, the rest held back.
//   x: loc | room << 16        y: w / LN | cut(open) / LN << 10 | cut(opened) / LN << 20
//   z: the open chunk          w: the chunk this tile's run opens
template <int LN>
__device__ __forceinline__ uint4 p1l_pack(uint32_t loc, uint32_t c, uint32_t o, uint32_t f, uint32_t np) {
    const uint32_t h = held<LN>(o, f), w = f - h, room = o == kNone ? 0u : (uint32_t)kCh - w;
    const uint32_t cut0 = min(w + h + c, (uint32_t)kCh) / LN, cut1 = h + c > room ? (h + c - room) / LN : 0u;
    return make_uint4(loc | room << 16, w / LN | cut0 << 10 | cut1 << 20, o, np);
}
static_assert(kCh / kLine < 1024 && kCh / kLineSplit < 1024 && kCh < 65536, "p1l_pack fields");

// wave 0: run starts `loc` of this tile (exclusive scan over each slice's staged sequence = held
// items + run), where each run itself starts (base = loc + held), the chunks its runs open (p1, opened,
// misc[0]), the store loop's per-slice words (Q) and the staged total (misc[2]).  G is the store loop's group:
// every slice's staged length is rounded up to a multiple of it, so each loc is one and misc[2] is the padded
// total (kStageGroup for the split pool, whose store loop takes four staged pairs per lane; 1 otherwise).
template <int LN, int G>
__device__ __forceinline__ void p1l_plan(int nb, const uint32_t* cn, uint32_t* loc, const uint32_t* ph,
                                         const uint32_t* fl, uint32_t* p1, uint32_t* opened, uint32_t* misc,
                                         uint32_t* base, uint4* Q) {
    const int lane = p1l_lane();
    const int per = (nb + 63) / 64, b0 = lane * per, b1 = min(b0 + per, nb);
    uint32_t sum = 0, need = 0;
    for (int i = b0; i < b1; ++i) {
        const uint32_t c = cn[i];
        sum += (c + held<LN>(ph[i], fl[i]) + (G - 1)) & ~(uint32_t)(G - 1);
        need += (c && (ph[i] == kNone || fl[i] + c > (uint32_t)kCh)) ? 1u : 0u;
    }
    const uint32_t is = wave_incl_scan(sum), in = wave_incl_scan(need);
    uint32_t pre = is - sum, k = in - need;
    const uint32_t nf = misc[1];
    for (int i = b0; i < b1; ++i) {
        const uint32_t c = cn[i], o = ph[i], f = fl[i];
        loc[i] = pre;
        base[i] = pre + held<LN>(o, f);
        uint32_t np = kNone;
        if (c && (o == kNone || f + c > (uint32_t)kCh)) {
            np = nf + k;
            opened[k++] = (uint32_t)i;
        }
        p1[i] = np;
        Q[i] = p1l_pack<LN>(pre, c, o, f, np);
        pre += (c + held<LN>(o, f) + (G - 1)) & ~(uint32_t)(G - 1);
    }
    if (lane == 63) {
        misc[0] = in;
        misc[2] = is;
    }
    wave_lds_order();
}

// (the split pool's stage has kStageGroup more entries per slice: each staged length is padded to a multiple of it;
// a whole group and not kStageGroup - 1, so that `hold` and `Q` stay 16-byte aligned for every nb)
__host__ __device__ constexpr size_t scatter1l_lds(int nb, int ns, bool hist, int block, int tile, bool split = false) {
    return sizeof(uint2) * ((size_t)tile + (size_t)nb * (2 * p1_line(split) + p1_pad(split))) +
           sizeof(uint32_t) * ((hist ? (size_t)nb * hist_words(ns) : 0) + 12 * (size_t)nb + block / 64 + 4);
}

// IdT as in k_scatter_c: the narrow form holds the prefetched tile (sr, tr) in 2 * IT registers, not 4 * IT.
template <int B, int IT, int MINW, bool HIST, bool SPLIT = false, bool NTL = false, bool NTS = false,
          typename IdT = int64_t>
__global__ void __launch_bounds__(B, MINW) k_scatter_l(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                      int64_t m, Layout L, int swap, int64_t chunk0, size_t trash,
                                                      uint2* __restrict__ pool, unsigned long long* __restrict__ cmeta,
                                                      uint32_t* __restrict__ chist) {
    constexpr int T = B * IT;
    constexpr int kLine = p1_line(SPLIT);  // the instantiation's line, in pairs
    constexpr int kG = SPLIT ? kStageGroup : 1;  // staged pairs per lane and step of the store loop
    static_assert(kG == 1 || (kLine % kG == 0 && kG * sizeof(uint2) == 32), "a group is two 16-byte words of a line");
    static_assert(T <= kCh && kCh % kLine == 0, "a pass-1 run must span at most two chunks");
    static_assert(!(SPLIT && HIST), "the split pool is built without the cell counts");
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const int nb = L.nt, hw = hist_words(L.ns);
    // the pair (x, y) at position pos of chunk q
    auto put = [&](uint32_t q, uint32_t pos, uint2 p) {
        if (SPLIT) {
            uint32_t* tw = reinterpret_cast<uint32_t*>(pool + (size_t)q * kCh);
            tw[pos] = p.y | (p.x == p.y ? kLoopBit : 0u);
            tw[kCh + pos] = p.x;
        } else if (NTS) {
            __builtin_nontemporal_store(*reinterpret_cast<const unsigned long long*>(&p),
                                        reinterpret_cast<unsigned long long*>(pool + (size_t)q * kCh + pos));
        } else {
            pool[(size_t)q * kCh + pos] = p;
        }
    };
    // T + nb * (kLine + p1_pad): runs behind their held items, each slice's length padded to a multiple of kG
    uint2* stage = reinterpret_cast<uint2*>(smem);
    uint2* hold = stage + T + (size_t)nb * (kLine + p1_pad(SPLIT));  // nb x kLine held items
    uint4* Q = reinterpret_cast<uint4*>(hold + (size_t)nb * kLine);  // p1l_pack, 16-byte aligned
    uint32_t* H = reinterpret_cast<uint32_t*>(Q + nb);
    uint32_t* cnt = H + (HIST ? (size_t)nb * hw : 0);
    uint32_t* base = cnt + 2 * nb;
    uint32_t* loc = base + nb;
    uint32_t* ph = loc + nb;
    uint32_t* fl = ph + nb;  // logical fill of the open chunk (held items included)
    uint32_t* p1 = fl + nb;
    uint32_t* opened = p1 + nb;
    uint32_t* misc = opened + nb;
    if (HIST)
        for (int i = threadIdx.x; i < nb * hw; i += B) H[i] = 0;
    for (int i = threadIdx.x; i < nb; i += B) {
        cnt[i] = 0;
        cnt[nb + i] = 0;
        ph[i] = kNone;
        fl[i] = 0;
    }
    if (threadIdx.x == 0) {
        misc[0] = 0;
        misc[1] = (uint32_t)(chunk0 + (int64_t)blockIdx.x * chunks_per_block(m, gridDim.x, nb, T));
    }
    __syncthreads();
    const uint64_t range = (uint64_t)(L.hi - L.lo);
    const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15) == 0;
    const int64_t stride = (int64_t)gridDim.x * T;
    IdT sr[IT], tr[IT];
    int64_t t0 = (int64_t)blockIdx.x * T;
    if (t0 < m) load_tile<B, NTL>(src, dst, t0, m, vec, sr, tr);
    int par = 0;
    bool pending = false;
    for (; t0 < m; t0 += stride, par ^= 1) {
        uint32_t* cn = cnt + par * nb;
        uint2 pr[IT];
        uint32_t rk[IT];
        uint32_t valid = 0;
#pragma unroll
        for (int u = 0; u < IT; ++u) {
            const int64_t e = t0 + tile_item_off<B, IdT>(u);
            const uint64_t s = rel_id(sr[u], L.lo), t = rel_id(tr[u], L.lo);
            const bool ok = e < m && s < range && t < range;
            pr[u] = swap ? make_uint2((uint32_t)t, (uint32_t)s) : make_uint2((uint32_t)s, (uint32_t)t);
            valid |= (ok ? 1u : 0u) << u;
            rk[u] = 0;
        }
        if (t0 + stride < m) load_tile<B, NTL>(src, dst, t0 + stride, m, vec, sr, tr);  // prefetch
#pragma unroll
        for (int u = 0; u < IT; ++u)
            if ((valid >> u) & 1u) rk[u] = atomicAdd(&cn[pr[u].y >> L.tbits], 1u);
        __syncthreads();
        if (threadIdx.x < 64) {
            if (pending)
                p1l_settle<HIST, kLine>(L, hw, stage, H, cnt + (par ^ 1) * nb, loc, ph, fl, p1, opened, misc, cmeta, chist);
            p1l_plan<kLine, kG>(nb, cn, loc, ph, fl, p1, opened, misc, base, Q);
        }
        __syncthreads();
        pending = true;
        const uint32_t total = misc[2];
        for (int x = threadIdx.x; x < nb * kLine; x += B) {  // held items first
            const int b = x / kLine, k = x % kLine;
            if ((uint32_t)k < base[b] - loc[b]) stage[loc[b] + k] = hold[x];
        }
#pragma unroll
        for (int u = 0; u < IT; ++u)
            if ((valid >> u) & 1u) stage[base[pr[u].y >> L.tbits] + rk[u]] = pr[u];
        __syncthreads();
        // The split pool: a lane takes kG = 4 staged pairs (two 16-byte LDS reads), one Q[b] and one decode for the
        // group, and stores the four target words and the four source words with one 16-byte store each (the same
        // bytes as one pair per lane, in a quarter of the store instructions and of the decodes).  A group needs
        // no per-item decision: every loc is a multiple of 4 (p1l_plan pads each slice's staged length), so r and
        // pos are; w, room, both cuts and kCh are multiples of 32.  The group therefore lies wholly in the open
        // chunk or wholly in the opened one, and wholly below the cut or wholly at or above it.  Padding is the
        // last 1..3 entries of a slice's sequence whose length is no multiple of 4: that group's first pair is
        // real (so b is the slice's), the sequence's end is then no multiple of 32, the cut lies below the group
        // and the group is held; its padding lands in hold slots past the held count, which nobody reads
        // (pos - cut <= 28, inside the slice's line of hold).
        if (SPLIT) {
            typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));  // one LDS / global access each
            const v4u32* stage4 = reinterpret_cast<const v4u32*>(stage);
            for (uint32_t idx = kG * threadIdx.x; idx < total; idx += kG * B) {
                // the pairs (a.x, a.y) (a.z, a.w) (c.x, c.y) (c.z, c.w)
                const v4u32 a = stage4[idx / 2], c = stage4[idx / 2 + 1];
                const int b = min((int)(a.y >> L.tbits), nb - 1);
                const uint4 q = Q[b];
                const uint32_t r = idx - (q.x & 0xFFFFu), room = q.x >> 16, w = (q.y & 1023u) * kLine;
                const bool first = r < room;
                const uint32_t pos = first ? w + r : r - room;
                const uint32_t cut = ((first ? q.y >> 10 : q.y >> 20) & 1023u) * kLine;
                if (pos < cut) {
                    uint32_t* tw = reinterpret_cast<uint32_t*>(pool + (size_t)(first ? q.z : q.w) * kCh) + pos;
                    const v4u32 t = {a.y | (a.x == a.y ? kLoopBit : 0u), a.w | (a.z == a.w ? kLoopBit : 0u),
                                     c.y | (c.x == c.y ? kLoopBit : 0u), c.w | (c.z == c.w ? kLoopBit : 0u)};
                    const v4u32 s = {a.x, a.z, c.x, c.z};
                    *reinterpret_cast<v4u32*>(tw) = t;
                    *reinterpret_cast<v4u32*>(tw + kCh) = s;
                } else {
                    v4u32* h = reinterpret_cast<v4u32*>(hold + b * kLine + (pos - cut));
                    h[0] = a;
                    h[1] = c;
                }
            }
        }
        // staged item r of slice b lands as p1l_pack lays out; one 16-byte LDS read per item
        for (uint32_t idx = threadIdx.x; !SPLIT && idx < (uint32_t)(T + nb * kLine); idx += B) {
            const uint2 p = stage[idx];
            const int b = min((int)(p.y >> L.tbits), nb - 1);
            const uint4 q = Q[b];
            const uint32_t r = idx - (q.x & 0xFFFFu), room = q.x >> 16, w = (q.y & 1023u) * kLine;
            const bool first = r < room;
            if (HIST && idx < total && first && r >= base[b] - loc[b]) hist_add(H, hw, b, p.x >> L.sbits);
            const uint32_t pos = first ? w + r : r - room;
            const uint32_t cut = ((first ? q.y >> 10 : q.y >> 20) & 1023u) * kLine;
            if (idx >= total) {
                break;  // idx only grows
            } else if (pos < cut) {
                put(first ? q.z : q.w, pos, p);
            } else {
                hold[b * kLine + (pos - cut)] = p;
            }
        }
    }
    __syncthreads();
    if (pending && threadIdx.x < 64)
        p1l_settle<HIST, kLine>(L, hw, stage, H, cnt + (par ^ 1) * nb, loc, ph, fl, p1, opened, misc, cmeta, chist);
    __syncthreads();
    for (int x = threadIdx.x; x < nb * kLine; x += B) {  // held tails
        const int b = x / kLine, k = x % kLine;
        const uint32_t h = held<kLine>(ph[b], fl[b]);
        if ((uint32_t)k < h) put(ph[b], fl[b] - h + k, hold[x]);
    }
    for (int i = threadIdx.x; i < nb; i += B)
        if (ph[i] != kNone) cmeta[ph[i]] = chunk_meta(i, fl[i]);
    if (HIST)
        for (int x = threadIdx.x; x < nb * hw; x += B) {
            const uint32_t p = ph[x / hw];
            if (p != kNone) chist[(size_t)p * hw + x % hw] = H[x];
        }
}

// The cell-count rows of a pool whose pass 1 ran without them (HIST = false): one wave per used chunk counts
// the chunk's pairs per source slice (16-bit LDS counters) and writes the row pass 1 would have written.
constexpr int kHistBlock = 256;

__global__ void __launch_bounds__(kHistBlock) k_chunk_hist(const uint2* __restrict__ pool,
                                                           const unsigned long long* __restrict__ cmeta,
                                                           int64_t nchunks, int ns, int sbits, int split,
                                                           uint32_t* __restrict__ chist) {
    constexpr int W = kHistBlock / 64;
    __shared__ uint32_t rows[W][64];  // hist_words(ns) <= 64
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hw = hist_words(ns);
    uint32_t* h = rows[wave];
    for (int64_t q = (int64_t)blockIdx.x * W + wave; q < nchunks; q += (int64_t)gridDim.x * W) {  // wave-uniform
        const uint32_t fill = (uint32_t)(cmeta[q] >> 32);
        if (!fill) continue;
        h[lane] = 0;
        wave_lds_order();
        const uint2* __restrict__ c = pool + (size_t)q * kCh;
        const uint32_t* __restrict__ cs = split_s(pool, (size_t)q);  // the split pool's source words
        for (uint32_t i0 = 0; i0 < fill; i0 += 256) {  // four loads in flight per lane
            uint32_t x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = min(i0 + (uint32_t)(k * 64 + lane), fill - 1);
                x[k] = split ? cs[i] : c[i].x;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + (uint32_t)(k * 64 + lane) < fill) hist_add(h, hw, 0, x[k] >> sbits);
        }
        wave_lds_order();
        if (lane < hw) chist[(size_t)q * hw + lane] = h[lane];
        wave_lds_order();
    }
}

// used chunks (fill > 0) grouped by target slice (order within a slice is arbitrary).  Each block
// takes kChunkPer chunks and aggregates per slice in LDS, so a slice counter sees one global atomic
// per block instead of one per chunk (≈10^5 chunks on ≈10^2 counters at C3).
constexpr int kChunkBlock = 1024, kChunkPer = 8192;

__global__ void __launch_bounds__(kChunkBlock) k_chunk_count(const unsigned long long* __restrict__ cmeta,
                                                             int64_t nchunks, int nt, int64_t* __restrict__ jcnt) {
    extern __shared__ uint32_t h[];  // nt
    for (int i = threadIdx.x; i < nt; i += kChunkBlock) h[i] = 0;
    __syncthreads();
    const int64_t q0 = (int64_t)blockIdx.x * kChunkPer, q1 = min(q0 + kChunkPer, nchunks);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kChunkBlock)
        if (cmeta[q] >> 32) atomicAdd(&h[(uint32_t)cmeta[q]], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += kChunkBlock)
        if (h[i]) atomicAdd(reinterpret_cast<unsigned long long*>(&jcnt[i]), (unsigned long long)h[i]);
}

__global__ void __launch_bounds__(kChunkBlock) k_chunk_place(const unsigned long long* __restrict__ cmeta,
                                                             int64_t nchunks, int nt,
                                                             unsigned long long* __restrict__ jcur,
                                                             uint32_t* __restrict__ order) {
    extern __shared__ uint32_t h[];  // nt counts, then nt bases (low 32 bits of the global cursor)
    uint32_t* base = h + nt;
    for (int i = threadIdx.x; i < nt; i += kChunkBlock) h[i] = 0;
    __syncthreads();
    const int64_t q0 = (int64_t)blockIdx.x * kChunkPer, q1 = min(q0 + kChunkPer, nchunks);
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kChunkBlock)
        if (cmeta[q] >> 32) atomicAdd(&h[(uint32_t)cmeta[q]], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < nt; i += kChunkBlock) {
        base[i] = h[i] ? (uint32_t)atomicAdd(&jcur[i], (unsigned long long)h[i]) : 0u;  // order has < 2^32 entries
        h[i] = 0;
    }
    __syncthreads();
    for (int64_t q = q0 + threadIdx.x; q < q1; q += kChunkBlock)
        if (cmeta[q] >> 32) {
            const uint32_t j = (uint32_t)cmeta[q];
            order[base[j] + atomicAdd(&h[j], 1u)] = (uint32_t)q;
        }
}

// block exclusive scan of a[0, n) in place (1024 lanes, each a run of consecutive entries); returns the total
__device__ uint32_t block_scan_inplace(uint32_t* a, int n, uint32_t* wtot) {
    constexpr int B = kChunkBlock;
    const int per = (n + B - 1) / B, b0 = (int)threadIdx.x * per, b1 = min(b0 + per, n);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t sum = 0;
    for (int i = b0; i < b1; ++i) sum += a[i];
    uint32_t x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t v = lane < B / 64 ? wtot[lane] : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(v, o, 64);
            if (lane >= o) v += y;
        }
        if (lane < B / 64) wtot[lane] = v;
    }
    __syncthreads();
    uint32_t pre = x - sum + (wave > 0 ? wtot[wave - 1] : 0u);
    for (int i = b0; i < b1; ++i) {
        const uint32_t c = a[i];
        a[i] = pre;
        pre += c;
    }
    const uint32_t total = wtot[B / 64 - 1];
    __syncthreads();
    return total;
}

// chunk_order in ONE launch for small pools (a rank's shard, C5's partitions): one workgroup counts the used
// chunks per slice, scans them (jst), places the chunks (order), and splits them into the g2 consumer blocks'
// segments (kseg -> segbase, ja) -- instead of a fill, two count / place launches, a copy and two scans
// (≈28 µs of launches and gaps per partition at a C5 shard of 2^22 relationships)
constexpr int64_t kOrder1Max = 32768;  // chunks; and nt <= kMaxTSlices, g2 <= 4096 (one workgroup over C3's 160K chunks: +0.13 ms)

__global__ void __launch_bounds__(kChunkBlock) k_chunk_order1(const unsigned long long* __restrict__ cmeta,
                                                              int64_t nchunks, int nt, int64_t g2,
                                                              int64_t* __restrict__ jst_out,
                                                              uint32_t* __restrict__ order,
                                                              int64_t* __restrict__ segbase, int* __restrict__ ja) {
    __shared__ uint32_t h[kMaxTSlices + 1];  // counts -> starts
    __shared__ uint32_t cur[kMaxTSlices];
    __shared__ uint32_t ks[4096 + 1];        // segments per consumer block -> their first index
    __shared__ uint32_t wtot[kChunkBlock / 64];
    for (int i = threadIdx.x; i <= nt; i += kChunkBlock) h[i] = 0;
    __syncthreads();
    for (int64_t q = threadIdx.x; q < nchunks; q += kChunkBlock)
        if (cmeta[q] >> 32) atomicAdd(&h[(uint32_t)cmeta[q]], 1u);
    __syncthreads();
    const uint32_t used = block_scan_inplace(h, nt, wtot);
    if (threadIdx.x == 0) h[nt] = used;
    __syncthreads();
    for (int i = threadIdx.x; i <= nt; i += kChunkBlock) {
        jst_out[i] = (int64_t)h[i];
        if (i < nt) cur[i] = h[i];
    }
    __syncthreads();
    for (int64_t q = threadIdx.x; q < nchunks; q += kChunkBlock)
        if (cmeta[q] >> 32) order[atomicAdd(&cur[(uint32_t)cmeta[q]], 1u)] = (uint32_t)q;
    // the consumers' split (k_seg_count / SegSplit): block w takes chunks [w per, (w + 1) per) of `order`
    const int64_t per = max((int64_t)1, ((int64_t)used + g2 - 1) / g2);
    for (int64_t w = threadIdx.x; w < g2; w += kChunkBlock) {
        const int64_t q0 = w * per, q1 = min(q0 + per, (int64_t)used);
        uint32_t k = 0;
        int a = 0;
        if (q0 < q1) {
            int lo = 0, hi = nt;  // last j with start <= q0, and with start <= q1 - 1
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)h[mid] <= q0) lo = mid; else hi = mid;
            }
            a = lo;
            hi = nt;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if ((int64_t)h[mid] <= q1 - 1) lo = mid; else hi = mid;
            }
            k = (uint32_t)(lo - a + 1);
        }
        ks[w] = k;
        ja[w] = a;
    }
    __syncthreads();
    const uint32_t nseg = block_scan_inplace(ks, (int)g2, wtot);
    for (int64_t w = threadIdx.x; w < g2; w += kChunkBlock) segbase[w] = (int64_t)ks[w];
    if (threadIdx.x == 0) segbase[g2] = (int64_t)nseg;
}

// segments per block, ja(w)
__global__ void k_seg_count(const int64_t* __restrict__ jst, int nt, int64_t blocks, int64_t* __restrict__ kseg,
                            int* __restrict__ ja) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= blocks) return;
    const SegSplit S(jst, nt, blocks);
    const int64_t q0 = w * S.per, q1 = min(q0 + S.per, S.nch);
    if (q0 >= q1) {
        kseg[w] = 0;
        ja[w] = 0;
        return;
    }
    const int a = slice_of(jst, nt, q0), b = slice_of(jst, nt, q1 - 1);
    kseg[w] = b - a + 1;
    ja[w] = a;
}

// psum[g][i] = pairs of segment g in source slice i (sum of its chunks' histogram rows)
__global__ void __launch_bounds__(1024) k_seg_sum(const uint32_t* __restrict__ chist, const uint32_t* __restrict__ order,
                                                 const int64_t* __restrict__ jst, int nt, int64_t blocks,
                                                 const int64_t* __restrict__ segbase, const int* __restrict__ ja,
                                                 int ns, uint32_t* __restrict__ psum) {
    __shared__ uint32_t acc[1024];
    const int64_t g = blockIdx.x;
    if (g >= segbase[blocks]) return;  // grid sized by an upper bound
    const SegSplit S(jst, nt, blocks);
    const int64_t w = block_of_seg(segbase, blocks, g);
    const Seg sg = seg_of(jst, nt, S, ja, w, g - segbase[w]);
    const int hw = hist_words(ns), rows = 1024 / hw;  // hw <= 64
    const int r = threadIdx.x / hw, x = threadIdx.x % hw;
    uint32_t lo = 0, hi = 0;
    if (r < rows) {
        int64_t q = sg.q0 + r;
        for (; q + 3 * rows < sg.q1; q += 4 * rows) {  // four rows' loads in flight per lane
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = chist[(size_t)order[q + k * rows] * hw + x];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo += v[k] & 0xFFFFu;
                hi += v[k] >> 16;
            }
        }
        for (; q < sg.q1; q += rows) {
            const uint32_t v = chist[(size_t)order[q] * hw + x];
            lo += v & 0xFFFFu;
            hi += v >> 16;
        }
    }
    for (int half = 0; half < 2; ++half) {
        acc[threadIdx.x] = half ? hi : lo;
        __syncthreads();
        if (threadIdx.x < hw && 2 * (int)threadIdx.x + half < ns) {
            uint32_t s = 0;
            for (int k = 0; k < rows; ++k) s += acc[k * hw + threadIdx.x];
            psum[(size_t)g * ns + 2 * threadIdx.x + half] = s;
        }
        __syncthreads();
    }
}

// per cell (j, i): exclusive running sum over slice j's segments (in place) and the cell total
__global__ void k_seg_prefix(uint32_t* __restrict__ psum, const int64_t* __restrict__ jst, int64_t blocks,
                             const int64_t* __restrict__ segbase, const int* __restrict__ ja, Layout L,
                             int64_t* __restrict__ tot) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= L.ncells) return;
    const int j = c / L.ns, i = c % L.ns;
    const SegSplit S(jst, L.nt, blocks);
    int64_t run = 0;
    if (jst[j + 1] > jst[j])
        for (int64_t w = jst[j] / S.per; w <= (jst[j + 1] - 1) / S.per; ++w) {
            const size_t at = (size_t)(segbase[w] + (j - ja[w])) * L.ns + i;
            const uint32_t v = psum[at];
            psum[at] = (uint32_t)run;
            run += v;
        }
    tot[c] = run;
}

// OR the block's target slice j into the global words, masked by the target-side node filter
__device__ __forceinline__ void flush_slice(const uint32_t* tl, uint32_t* g, int j, int64_t gwords, BitV mask) {
    const int64_t w0 = (int64_t)j * kSliceWords;
    for (int i = threadIdx.x; i < kSliceWords; i += kBlock) {
        const int64_t gw = w0 + i;
        if (gw >= gwords) break;
        uint32_t v = tl[i];
        if (v && !mask.full) v &= mask.w[gw];
        if (v) atomicOr(&g[gw], v);
    }
}

// hop-1 outputs when it runs inside pass 2 (a_ok covers the whole domain, so no source test)
struct Hop1Out {
    BitV tmask;  // b_ok
    uint32_t* M;
    uint32_t* S1;
    uint32_t* S2;
    int64_t gwords;
};

// The 2-hop layout's pair store.  Packed (L.packed): the cell-relative key
// k = (s mod 2^sbits) << tbits | (t mod 2^tbits), at most 40 bits, split into its low word w[pos]
// and high byte b[pos] -- 5 bytes per relationship instead of 8; the cell gives the slices back.
struct PairOut {
    uint2* p;     // unpacked
    uint32_t* w;  // packed: low words
    uint8_t* b;   // packed: high bytes
};

__device__ __forceinline__ uint64_t cell_key(const Layout& L, uint2 v) {
    return (uint64_t)(v.x & ((1u << L.sbits) - 1u)) << L.tbits | (v.y & ((1u << L.tbits) - 1u));
}

// pair of a cell-relative key in cell (j, i)
__device__ __forceinline__ uint2 key_pair(const Layout& L, uint32_t sbase, uint32_t tbase, uint32_t w, uint32_t b) {
    const uint64_t k = (uint64_t)b << 32 | w;
    return make_uint2(sbase + (uint32_t)(k >> L.tbits), tbase + (w & ((1u << L.tbits) - 1u)));
}

// ---- pass 2: block w's segments (chunks of one target slice each) -> the slices' source cells -----
// Output offsets are exact and precomputed, so the reservation per tile is an LDS cursor bump and the
// layout is deterministic.  The next chunk is loaded (buffer loads clipped at its fill) while this
// one is regrouped.  With HOP1 the block also runs hop 1 on the pairs it moves: M(t) for s != t
// marked in an LDS copy of the current slice (flushed through b_ok when it changes), self-loops
// -> S1 / S2.
// output line in items: 128 bytes of pairs, or of the packed low words
__host__ __device__ constexpr int s2_line(bool pk) { return pk ? 32 : kLine; }

// LDS bytes of the per-cell held items (packed: low word + high byte each)
__host__ __device__ constexpr size_t s2_hold_bytes(int nb, bool pk) {
    return pk ? (((size_t)nb * s2_line(true) * 5 + 15) & ~(size_t)15) : sizeof(uint2) * (size_t)nb * kLine;
}

template <bool HOP1, bool PK, bool SP = false>  // PK: without HOP1 (LDS); SP: the pool is split (part_common.h)
__global__ void __launch_bounds__(kSBlock) k_scatter_s2(const void* __restrict__ pool_,
                                                        const unsigned long long* __restrict__ cmeta,
                                                        const uint32_t* __restrict__ order,
                                                        const int64_t* __restrict__ jst,
                                                        const int64_t* __restrict__ segbase,
                                                        const int* __restrict__ ja, const uint32_t* __restrict__ prel,
                                                        const int64_t* __restrict__ coff, Layout L,
                                                        PairOut out, int64_t trash, Hop1Out h1) {
    constexpr int LN = s2_line(PK);
    extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
    const int nb = L.ns;
    const int64_t w = blockIdx.x, blocks = gridDim.x;
    uint2* stage = reinterpret_cast<uint2*>(smem);
    // per source cell: the items of its unfinished output line, slot = index mod LN
    unsigned char* hbase = reinterpret_cast<unsigned char*>(stage + kTile);
    uint2* hold = reinterpret_cast<uint2*>(hbase);
    uint32_t* holdw = reinterpret_cast<uint32_t*>(hbase);
    uint8_t* holdb = hbase + sizeof(uint32_t) * (size_t)nb * LN;
    uint32_t* cur = reinterpret_cast<uint32_t*>(hbase + s2_hold_bytes(nb, PK));  // next output index per cell (< 2^32)
    uint32_t* cnt = cur + nb;
    uint32_t* loc = cnt + nb;
    uint32_t* hc = loc + nb;  // items held per cell (all in the line of cur)
    uint32_t* wtot = hc + nb;
    uint32_t* tl = wtot + kSBlock / 64;  // HOP1: target slice marks
    const SegSplit S(jst, L.nt, blocks);
    for (int i = threadIdx.x; i < nb; i += kSBlock) hc[i] = 0;
    auto put = [&](uint32_t pos, uint2 v) {
        if (PK) {
            const uint64_t k = cell_key(L, v);
            out.w[pos] = (uint32_t)k;
            out.b[pos] = (uint8_t)(k >> 32);
        } else {
            out.p[pos] = v;
        }
    };
    auto hold_put = [&](int slot, uint2 v) {
        if (PK) {
            const uint64_t k = cell_key(L, v);
            holdw[slot] = (uint32_t)k;
            holdb[slot] = (uint8_t)(k >> 32);
        } else {
            hold[slot] = v;
        }
    };
    auto hold_out = [&](uint32_t pos, int slot) {
        if (PK) {
            out.w[pos] = holdw[slot];
            out.b[pos] = holdb[slot];
        } else {
            out.p[pos] = hold[slot];
        }
    };
    auto flush_held = [&]() {  // the segment's unfinished lines (shared with a neighbouring segment)
        for (int x = threadIdx.x; x < nb * LN; x += kSBlock) {
            const int b = x / LN, k = x % LN;
            if ((uint32_t)k < hc[b]) {
                const uint32_t pos = cur[b] - hc[b] + (uint32_t)k;
                hold_out(pos, b * LN + (int)(pos & (LN - 1)));
            }
        }
    };
    const uint2* pool = static_cast<const uint2*>(pool_);
    auto load_chunk = [&](int64_t q, uint2 (&pr)[kItems]) -> uint32_t {
        const uint32_t phys = order[q];
        const uint32_t fill = (uint32_t)(cmeta[phys] >> 32);
        if (SP) {  // the same two pairs per load step, from the two word arrays
            const int bytes = (int)(fill * sizeof(uint32_t));
            const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint32_t*>(split_t(pool, phys)), (short)0, bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint32_t*>(split_s(pool, phys)), (short)0, bytes, 0x00020000);
#pragma unroll
            for (int k = 0; k < kItems / 2; ++k) {
                const uint32_t at = (uint32_t)(k * kSBlock + (int)threadIdx.x) * 8u;
                const auto t = __builtin_amdgcn_raw_buffer_load_b64(rt, at, 0, 0);
                const auto x = __builtin_amdgcn_raw_buffer_load_b64(rx, at, 0, 0);
                pr[2 * k] = make_uint2(x[0], t[0] & ~kLoopBit);
                pr[2 * k + 1] = make_uint2(x[1], t[1] & ~kLoopBit);
            }
            return fill;
        }
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint2*>(pool + (size_t)phys * kCh), (short)0, (int)(fill * sizeof(uint2)), 0x00020000);
#pragma unroll
        for (int k = 0; k < kItems / 2; ++k) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (uint32_t)(k * kSBlock + (int)threadIdx.x) * 16u, 0, 0);
            pr[2 * k] = make_uint2(v[0], v[1]);
            pr[2 * k + 1] = make_uint2(v[2], v[3]);
        }
        return fill;
    };
    const int64_t qb = w * S.per, qe = min(qb + S.per, S.nch);
    uint2 nx[kItems];
    uint32_t nfill = qb < qe ? load_chunk(qb, nx) : 0u;
    int64_t g = segbase[w] - 1, seg_end = qb;  // current segment and the end of its chunk range
    int cur_j = -1;
    uint32_t tbase = 0;
    // One flat loop over the block's chunks, so the only vector-memory operations between a
    // chunk's prefetch and its use are the kItems stores of the tile before (unconditional, so the
    // compiler can wait for the loads alone); segment changes are the rare branch.
    for (int64_t q = qb; q < qe; ++q) {  // block-uniform
        if (q == seg_end) {
            __syncthreads();
            flush_held();
            __syncthreads();
            for (int i = threadIdx.x; i < nb; i += kSBlock) hc[i] = 0;
            Seg sg;
            do {
                ++g;
                sg = seg_of(jst, L.nt, S, ja, w, g - segbase[w]);
            } while (sg.q0 >= sg.q1);  // skip empty slices
            seg_end = sg.q1;
            if (HOP1 && sg.j != cur_j) {
                if (cur_j >= 0) {
                    __syncthreads();
                    flush_slice(tl, h1.M, cur_j, h1.gwords, h1.tmask);
                }
                __syncthreads();
                for (int k = threadIdx.x; k < kSliceWords; k += kSBlock) tl[k] = 0;
            }
            cur_j = sg.j;
            tbase = (uint32_t)sg.j << kSliceBits;
            __syncthreads();
            for (int i = threadIdx.x; i < nb; i += kSBlock)
                cur[i] = (uint32_t)(coff[(size_t)sg.j * nb + i] + prel[(size_t)g * nb + i]);
        }
        uint2 pr[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k) pr[k] = nx[k];
        const uint32_t fill = nfill;
        if (q + 1 < qe) nfill = load_chunk(q + 1, nx);  // prefetch (may be the next segment's)
        for (int i = threadIdx.x; i < nb; i += kSBlock) cnt[i] = 0;
        __syncthreads();
        uint32_t rk[kItems];
        uint32_t valid = 0;
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            valid |= ((uint32_t)item_off<kSBlock>(k) < fill ? 1u : 0u) << k;
            rk[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < kItems; ++k)
            if ((valid >> k) & 1u) {
                rk[k] = atomicAdd(&cnt[pr[k].x >> L.sbits], 1u);
                if (HOP1) {
                    const uint32_t s = pr[k].x, t = pr[k].y;
                    if (s != t) {
                        lds_set(tl, t - tbase);
                    } else if (h1.tmask.full || gbit(h1.tmask.w, t)) {  // rare: self-loops
                        const uint32_t bit = 1u << (t & 31);
                        const uint32_t old = atomicOr(&h1.S1[t >> 5], bit);
                        if (old & bit) atomicOr(&h1.S2[t >> 5], bit);
                    }
                }
            }
        __syncthreads();
        const uint32_t total = small_exclusive_scan<kSBlock>(cnt, loc, nb, wtot);
        // Whole output lines: a cell's run is stored up to the last line boundary it reaches, the
        // rest held in LDS; held items go out when their line completes, together with the run
        // items that complete it (so a line is written within one tile, not in pieces by two).
        for (int x = threadIdx.x; x < nb * LN; x += kSBlock) {
            const int b = x / LN, k = x % LN;
            if ((uint32_t)k < hc[b]) {
                const uint32_t c = cur[b], pos = c - hc[b] + (uint32_t)k;
                if (((c + cnt[b]) & ~(uint32_t)(LN - 1)) > (c & ~(uint32_t)(LN - 1)))
                    hold_out(pos, b * LN + (int)(pos & (LN - 1)));
            }
        }
#pragma unroll
        for (int k = 0; k < kItems; ++k)
            if ((valid >> k) & 1u) stage[loc[pr[k].x >> L.sbits] + rk[k]] = pr[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const uint32_t idx = (uint32_t)(k * kSBlock + (int)threadIdx.x);
            const uint2 v = stage[idx];
            const int b = min((int)(v.x >> L.sbits), nb - 1);  // stale stage entries past `total`
            const uint32_t pos = cur[b] + idx - loc[b];
            const uint32_t cut = (cur[b] + cnt[b]) & ~(uint32_t)(LN - 1);
            if (idx >= total)
                put((uint32_t)trash + threadIdx.x, v);
            else if (pos < cut)
                put(pos, v);
            else
                hold_put(b * LN + (int)(pos & (LN - 1)), v);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < nb; i += kSBlock) {
            const uint32_t c = cur[i], n = cnt[i];
            const uint32_t cut = (c + n) & ~(uint32_t)(LN - 1);
            hc[i] = cut > (c & ~(uint32_t)(LN - 1)) ? c + n - cut : hc[i] + n;
            cur[i] = c + n;
        }
    }
    __syncthreads();
    flush_held();
    if (HOP1 && cur_j >= 0) flush_slice(tl, h1.M, cur_j, h1.gwords, h1.tmask);
}

// One hop over the 2-D layout.  Block b streams relationships [b*per, (b+1)*per) of the
// j-major cell order, per = max(ceil(kept / blocks), min_per); kept = coff[ncells] is read on the
// device, so building the layout needs no host round trip.
//   HOP1: M(t) |= a_ok(s) for s != t; self-loops (a_ok(s) and b_ok(t)) -> S1, second one -> S2.
//         Target filter b_ok at flush.
//   HOP2: C(t) |= X1(s) for s != t, X2(s) for s == t.  Target filter c_ok at flush.
// `sb` is the per-relationship source bitmap (a_ok or X1); `tmask` the target filter.
// this lane's kN packed items of the cell walk starting at the 4-aligned index b: item u is
// b + 4 * ((u >> 2) * B + lane) + (u & 3), one 16-byte low-word load and one 4-byte high-byte load
// per four items (streamed once: non-temporal)

template <int B, int N>
__device__ __forceinline__ void load_packed(const uint32_t* __restrict__ w, const uint8_t* __restrict__ hb, int64_t b,
                                            uint32_t (&lw)[N], uint32_t (&hw)[N / 4]) {
    typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
    const v4u32* __restrict__ v = reinterpret_cast<const v4u32*>(w + b);
    const uint32_t* __restrict__ h = reinterpret_cast<const uint32_t*>(hb + b);
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        const v4u32 x = __builtin_nontemporal_load(v + k * B + (int)threadIdx.x);
        lw[4 * k] = x.x;
        lw[4 * k + 1] = x.y;
        lw[4 * k + 2] = x.z;
        lw[4 * k + 3] = x.w;
        hw[k] = __builtin_nontemporal_load(h + k * B + (int)threadIdx.x);
    }
}

template <bool HOP1, bool SRC_FULL, bool PK>
__global__ void __launch_bounds__(kBlock) k_hop_2d(PairOut pairs, const int64_t* __restrict__ coff,
                                                   int64_t min_per, Layout L, BitV sb,
                                                   const uint32_t* __restrict__ X2, BitV tmask,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ S1,
                                                   uint32_t* __restrict__ S2, int64_t gwords) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* tl = lds;                // target slice marks
    uint32_t* sl = lds + kSliceWords;  // source slice frontier (when pulled)
    const int64_t kept = coff[L.ncells];
    int64_t per = (kept + gridDim.x - 1) / gridDim.x;
    if (per < min_per) per = min_per;
    int64_t e0 = (int64_t)blockIdx.x * per;
    const int64_t e1 = min(e0 + per, kept);
    if (e0 >= e1) return;  // block-uniform
    int c = 0;
    {  // last cell with coff[c] <= e0
        int lo = 0, hi = L.ncells;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (coff[mid] <= e0) lo = mid; else hi = mid;
        }
        c = lo;
    }
    int cur_j = -1;
    const bool can_pull = !SRC_FULL && L.sbits == kSliceBits;
    // The source slice a cell pulls is loaded into registers while the cell before it streams (this lane's
    // kSliceWords / kBlock words, 16-byte loads issued ahead of the cell's pair loads), so the pull no longer
    // waits for its own load latency behind a barrier; `nxt_i` = the slice held (-1: none).
    static_assert(kSliceWords % (4 * kBlock) == 0, "pull prefetch: whole 16-byte words per lane");
    constexpr int kPw = kSliceWords / (4 * kBlock);
    uint4 nsl[kPw];
    int nxt_i = -1;
    auto prefetch_slice = [&](int i2) {
        const uint4* src4 = reinterpret_cast<const uint4*>(sb.w + (int64_t)i2 * kSliceWords);
        const int64_t lim4 = (gwords - (int64_t)i2 * kSliceWords) / 4;  // whole uint4 words inside the bitmap
#pragma unroll
        for (int k = 0; k < kPw; ++k) {
            const int64_t x = (int64_t)k * kBlock + threadIdx.x;
            nsl[k] = x < lim4 ? src4[x] : make_uint4(0u, 0u, 0u, 0u);
        }
        nxt_i = i2;
    };
    while (e0 < e1) {
        while (coff[c + 1] <= e0) ++c;
        const int j = c / L.ns, i = c % L.ns;
        const int64_t ce = min(e1, coff[c + 1]);
        if (j != cur_j) {
            if (cur_j >= 0) {
                __syncthreads();
                flush_slice(tl, out, cur_j, gwords, tmask);
            }
            __syncthreads();
            for (int k = threadIdx.x; k < kSliceWords; k += kBlock) tl[k] = 0;
            cur_j = j;
        }
        const bool pull = can_pull && ce - e0 >= kLoadMin;
        if (pull) {
            const int64_t w0 = (int64_t)i * kSliceWords;
            if (nxt_i == i && (gwords - w0) % 4 == 0) {
                uint4* sl4 = reinterpret_cast<uint4*>(sl);
#pragma unroll
                for (int k = 0; k < kPw; ++k) sl4[k * kBlock + threadIdx.x] = nsl[k];
            } else {
                for (int k = threadIdx.x; k < kSliceWords; k += kBlock) sl[k] = w0 + k < gwords ? sb.w[w0 + k] : 0u;
            }
            nxt_i = -1;
        }
        if (can_pull && ce == coff[c + 1] && ce < e1 && ((uintptr_t)sb.w & 15) == 0) {  // the next cell, if it pulls
            const int c2 = c + 1;
            if (min(e1, coff[c2 + 1]) - ce >= kLoadMin) prefetch_slice(c2 % L.ns);
        }
        __syncthreads();
        const uint32_t tbase = (uint32_t)j << L.tbits, sbase = (uint32_t)i << L.sbits;  // pull: sbits = kSliceBits
        auto visit = [&](const uint2 pr) {
            const uint32_t s = pr.x, t = pr.y;
            if (s != t) {
                const bool ok = SRC_FULL || (pull ? gbit(sl, s - sbase) : gbit(sb.w, s));
                if (ok) lds_set(tl, t - tbase);
            } else if (HOP1) {  // rare: self-loops
                if ((SRC_FULL || gbit(sb.w, s)) && (tmask.full || gbit(tmask.w, t))) {
                    const uint32_t bit = 1u << (t & 31);
                    const uint32_t old = atomicOr(&S1[t >> 5], bit);
                    if (old & bit) atomicOr(&S2[t >> 5], bit);
                }
            } else {
                if (gbit(X2, s)) lds_set(tl, t - tbase);
            }
        };
        if (PK) {  // 5 bytes per item: twice the items per step for the same loads in flight
            constexpr int U = 2 * kUnroll;
            for (int64_t cb = e0 & ~int64_t(3); cb < ce; cb += (int64_t)kBlock * U) {  // block-uniform
                uint32_t lw[U], hw[U / 4];
                load_packed<kBlock, U>(pairs.w, pairs.b, cb, lw, hw);
                const int lo = (int)max(e0 - cb, (int64_t)0), hi = (int)min(ce - cb, (int64_t)kBlock * U);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int e = item_off4<kBlock>(u);
                    if (e >= lo && e < hi) visit(key_pair(L, sbase, tbase, lw[u], (hw[u >> 2] >> (8 * (u & 3))) & 0xFFu));
                }
            }
        } else {
            for (int64_t cb = e0 & ~int64_t(1); cb < ce; cb += (int64_t)kBlock * kUnroll) {  // block-uniform, even
                uint2 p[kUnroll];
                load_pairs<kBlock, kUnroll>(pairs.p, cb, p);
                const int lo = (int)max(e0 - cb, (int64_t)0), hi = (int)min(ce - cb, (int64_t)kBlock * kUnroll);
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int e = item_off<kBlock>(u);
                    if (e >= lo && e < hi) visit(p[u]);
                }
            }
        }
        e0 = ce;
        ++c;
        __syncthreads();  // the next cell may overwrite sl / flush tl
    }
    __syncthreads();
    flush_slice(tl, out, cur_j, gwords, tmask);
}

// ---- both hops over the pass-1 pool (no pass 2) -------------------------------------------------------
// The pool is grouped by target slice, so a block keeps the slice's target bitmap in LDS while it walks its
// share of the slice's chunks (part::walk_chunks_n); several blocks may share a slice, so the flush ORs.
constexpr int kPoolBlock = 1024;
// Hop 2's exchange (k_pool_hop2<true, XW>): windows of 256 words a wave takes per chunk it enters.  1 = the block
// covers its slice every 64 chunks, about 8 times per 4-Mi share.
constexpr int kPoolXchgWindows = 1;

// move the LDS slice j out through `mask` and clear it.  SKIP: a word whose bits the global word already holds
// (another block's, or this block's own exchange) costs a plain load instead of an atomic; a stale load lacks
// bits and never has one too many (a set bit of an OR is final), so it costs the atomic and nothing else.
template <bool SKIP = false>
__device__ __forceinline__ void pool_flush(uint32_t* tl, uint32_t* g, int j, int64_t gwords, BitV mask) {
    const int64_t w0 = (int64_t)j * kSliceWords;
    for (int i = threadIdx.x; i < kSliceWords; i += kPoolBlock) {
        uint32_t v = tl[i];
        tl[i] = 0;
        const int64_t gw = w0 + i;
        if (!v || gw >= gwords) continue;
        if (!mask.full) v &= mask.w[gw];
        if (SKIP && v) v &= ~g[gw];
        if (v) atomicOr(&g[gw], v);
    }
}

// Hop 1 for a full a_ok: M(t) for s != t in LDS, flushed through b_ok; self-loops -> S1 / S2 as in
// k_scatter_s2<true>.  It uses the target and whether the pair is a loop, nothing else of the source: over a
// split pool (SPLIT) it walks the T arrays alone, 4 bytes per relationship.
template <bool SPLIT>
__global__ void __launch_bounds__(kPoolBlock) k_pool_hop1(ChunkWalk cw, BitV tmask, uint32_t* __restrict__ M,
                                                          uint32_t* __restrict__ S1, uint32_t* __restrict__ S2,
                                                          int64_t gwords) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tl[];
    for (int k = threadIdx.x; k < kSliceWords; k += kPoolBlock) tl[k] = 0;
    __syncthreads();
    auto mark = [&](uint32_t t, bool loop, uint32_t tbase) {
        if (!loop) {
            lds_set(tl, t - tbase);
        } else if (tmask.full || gbit(tmask.w, t)) {  // rare: self-loops
            const uint32_t bit = 1u << (t & 31);
            const uint32_t old = atomicOr(&S1[t >> 5], bit);
            if (old & bit) atomicOr(&S2[t >> 5], bit);
        }
    };
    auto flush = [&](int j) { pool_flush(tl, M, j, gwords, tmask); };
    if (SPLIT) {
        walk_chunks_t<kPoolBlock>(
            cw,
            [&](const uint32_t (&tw)[kWalkWords], uint32_t valid, int j) {
                const uint32_t tbase = (uint32_t)j << kSliceBits;
#pragma unroll
                for (int k = 0; k < kWalkWords; ++k)
                    if ((valid >> k) & 1u) mark(tw[k] & ~kLoopBit, (tw[k] & kLoopBit) != 0, tbase);
            },
            flush);
    } else {
        walk_chunks_n<kPoolBlock>(
            cw,
            [&](const uint2 (&pr)[kWalkItems], uint32_t valid, int j) {
                const uint32_t tbase = (uint32_t)j << kSliceBits;
#pragma unroll
                for (int k = 0; k < kWalkItems; ++k)
                    if ((valid >> k) & 1u) mark(pr[k].y, pr[k].x == pr[k].y, tbase);
            },
            flush);
    }
}

// Hop 1 for a full a_ok from the tables' presence words (PresenceWords, capsmi_impl.h): what k_pool_hop1 derives
// from the pool -- M(t) = some relationship s -> t with s != t, S1 / S2 = one / two self-loops at t over all the
// tables -- is a fact about the tables, kept since their registration.  One thread per word of the domain: the
// tables' words are shifted to the domain (presence_word), masked with b_ok and ORed into M, S1, S2.  A second
// loop at an id is one table's loop2 bit or the loop1 bits of two list entries (a table listed twice counts twice).
constexpr int kPresenceMax = 8;  // tables per launch (more: hop 1 walks the pool)
struct PresenceIn {
    const uint32_t* m[kPresenceMax];
    const uint32_t* l1[kPresenceMax];
    const uint32_t* l2[kPresenceMax];
    int64_t nwords[kPresenceMax];
    int64_t shift[kPresenceMax];  // the table's window low end - the domain's (>= 0: presence_usable)
    int n;
};
__global__ void __launch_bounds__(256) k_presence_hop1(PresenceIn in, BitV tmask, uint32_t* __restrict__ M,
                                                       uint32_t* __restrict__ S1, uint32_t* __restrict__ S2,
                                                       int64_t gwords) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= gwords) return;
    uint32_t m = 0, l1 = 0, l2 = 0;
#pragma unroll
    for (int i = 0; i < kPresenceMax; ++i) {  // unrolled: the argument arrays are read at constant offsets
        if (i >= in.n) break;
        m |= presence_word(in.m[i], in.nwords[i], in.shift[i], w);
        const uint32_t a = presence_word(in.l1[i], in.nwords[i], in.shift[i], w);
        l2 |= presence_word(in.l2[i], in.nwords[i], in.shift[i], w) | (l1 & a);
        l1 |= a;
    }
    if (!tmask.full) {
        const uint32_t b = tmask.w[w];
        m &= b;
        l1 &= b;
        l2 &= b;
    }
    if (m) M[w] |= m;
    if (l1) S1[w] |= l1;
    if (l2) S2[w] |= l2;
}

// Hop 2: C(t) |= X1(s) for s != t, X2(s) for s == t, with the C slice in LDS.  A pair whose target bit is
// already set needs no X read (the result is an OR, so skipping is exact in any order); targets outside c_ok
// are preset so their pairs skip too, and the flush masks them off again.  A lane tests its step's targets
// first, then issues the X1 gathers of the unset ones together (buffer loads: a lane that needs none gives an
// offset past the bitmap, which reads as zero without a memory request) and only then sets bits.
// Over a split pool the steps run as a software pipeline (part::walk_chunks_st_pipe): the target test of step
// i + 1 and the T loads of step i + 2 are issued while step i waits for its gathers, and a lane loads the
// source words of four pairs only if one of them needs its source (about two thirds of the 128-byte source
// lines at C3).  A target tested in step i + 1 may be set a moment later by step i - 1 or i: that costs one
// gather too many and never a wrong bit, since C is an OR.  Four waves per SIMD is what one block per CU uses,
// so the split instantiation may take 128 VGPRs for its three steps in flight.
//
// XW > 0 (split pool only, CAPSMI_HOP2_EXCHANGE): the blocks that walk one slice exchange their C bits through
// the global C while they walk.  A block starts a share with an empty LDS slice and would gather once for every
// distinct target of the share, also for the ones another block has long resolved; at C3 about 37 of the 256
// blocks walk slice 0.  A set bit of the global C is final and true, so a block may OR global words into its
// LDS slice and publish its own new bits at any moment, with no barrier and no ordering: a stale read costs a
// gather and never a wrong bit.  The walker hands a wave XW windows of 256 words per chunk it enters
// (part::walk_chunks_st_pipe); per word the lane ORs the global word into LDS and publishes what LDS holds
// beyond it.  The loads carry sc1 (what an agent-scope relaxed atomic load compiles to), so a word is not
// served for the rest of the kernel from a line the XCD's L2 took before other XCDs' atomics.  LDS also holds
// bits that are no results (the preset ~c_ok): everything that leaves, leaves through cmask.  A visit also
// starts from the global words (begin), and its flush skips the words that are already out.
template <bool SPLIT, int XW = 0>
__global__ void __launch_bounds__(kPoolBlock, SPLIT ? 4 : 8)
    k_pool_hop2(ChunkWalk cw, const uint32_t* __restrict__ X1, const uint32_t* __restrict__ X2, BitV cmask,
                uint32_t* __restrict__ C, int64_t gwords) {
    static_assert(SPLIT || XW == 0, "the exchange rides on the pipelined walk of the split pool");
    extern __shared__ __attribute__((aligned(16))) uint32_t tl[];
    for (int k = threadIdx.x; k < kSliceWords; k += kPoolBlock) tl[k] = 0;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint32_t*>(X1), (short)0, (int)(gwords * (int64_t)sizeof(uint32_t)), 0x00020000);
    // a lane's step: pair k is source(k) -> the target whose in-slice offset is off(k), a loop if loop(k)
    auto step = [&](auto source, auto off, auto loop, uint32_t valid) {
        uint32_t need = 0;
#pragma unroll
        for (int k = 0; k < kWalkItems; ++k) {
            const uint32_t r = off(k);
            if (((valid >> k) & 1u) && !((tl[r >> 5] >> (r & 31)) & 1u)) need |= 1u << k;
        }
        uint32_t xw[kWalkItems];
#pragma unroll
        for (int k = 0; k < kWalkItems; ++k) {
            const bool ld = ((need >> k) & 1u) && !loop(k);
            xw[k] = __builtin_amdgcn_raw_buffer_load_b32(xr, ld ? (source(k) >> 5) * 4u : 0xFFFFFFF0u, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < kWalkItems; ++k) {
            if (!((need >> k) & 1u)) continue;
            const uint32_t s = source(k);
            const bool ok = !loop(k) ? ((xw[k] >> (s & 31)) & 1u) != 0 : gbit(X2, s);  // self-loops: rare
            if (ok) lds_set(tl, off(k));
        }
    };
    auto flush = [&](int j) { pool_flush<(XW > 0)>(tl, C, j, gwords, cmask); };
    auto begin = [&](int j) {
        if constexpr (XW > 0) {  // the preset, and what is out already: free and exact, for a block that comes late
            const int64_t w0 = (int64_t)j * kSliceWords;
            for (int i = threadIdx.x; i < kSliceWords; i += kPoolBlock) {
                const int64_t gw = w0 + i;
                uint32_t v = cmask.full ? 0u : 0xFFFFFFFFu;
                if (gw < gwords) v = (cmask.full ? 0u : ~cmask.w[gw]) | C[gw];
                tl[i] = v;
            }
            return;
        }
        if (cmask.full) return;
        const int64_t w0 = (int64_t)j * kSliceWords;
        for (int i = threadIdx.x; i < kSliceWords; i += kPoolBlock)
            tl[i] = w0 + i < gwords ? ~cmask.w[w0 + i] : 0xFFFFFFFFu;
    };
    // The exchange: the lane's four words of the window in flight (xg), of c_ok too where it is partial (xm), and
    // the window they belong to.  Buffer loads, so the words past the bitmap's end in the last slice read as zero.
    typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));
    [[maybe_unused]] v4u32 xg = {0u, 0u, 0u, 0u}, xm = {0u, 0u, 0u, 0u};
    [[maybe_unused]] uint32_t xcur = 0;
    auto xword = [&]() { return xcur * (uint32_t)kXchgWords + 4u * (threadIdx.x & 63u); };  // in the slice
    auto xissue = [&](uint32_t win, int j) {
        const __amdgpu_buffer_rsrc_t cr = __builtin_amdgcn_make_buffer_rsrc(
            C, (short)0, (int)(gwords * (int64_t)sizeof(uint32_t)), 0x00020000);
        xcur = win;
        const uint32_t off = ((uint32_t)j * (uint32_t)kSliceWords + xword()) * 4u;
        xg = __builtin_amdgcn_raw_buffer_load_b128(cr, off, 0, 16);  // sc1: not from the L1, nor a stale L2 line
        if (!cmask.full) {
            const __amdgpu_buffer_rsrc_t mr = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<uint32_t*>(cmask.w), (short)0, (int)(gwords * (int64_t)sizeof(uint32_t)), 0x00020000);
            xm = __builtin_amdgcn_raw_buffer_load_b128(mr, off, 0, 0);
        }
    };
    auto xconsume = [&](int j) {
        const uint32_t w = xword();
        const int64_t gw = (int64_t)j * kSliceWords + w;
        const v4u32 l = *reinterpret_cast<const v4u32*>(&tl[w]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t in = xg[e] & ~l[e];
            if (in) atomicOr(&tl[w + e], in);
            uint32_t out = l[e] & ~xg[e];  // may hold preset bits: out through c_ok only
            if (!cmask.full) out &= xm[e];
            if (out && gw + e < gwords) atomicOr(&C[gw + e], out);
        }
    };
    if (SPLIT) {
        constexpr uint32_t kOff = (1u << kSliceBits) - 1u;  // (T word - slice base) & kOff drops the loop bit too
        walk_chunks_st_pipe<kPoolBlock, XW>(
            cw,
            [&](const uint32_t (&tw)[kWalkItems], uint32_t valid, int j) {
                const uint32_t tbase = (uint32_t)j << kSliceBits;
                uint32_t cbits[kWalkItems], need = 0;  // all eight LDS reads before any is used
#pragma unroll
                for (int k = 0; k < kWalkItems; ++k) cbits[k] = tl[((tw[k] - tbase) & kOff) >> 5];
#pragma unroll
                for (int k = 0; k < kWalkItems; ++k) need |= (~(cbits[k] >> (tw[k] & 31)) & 1u) << k;
                return need & valid;
            },
            [&](const uint32_t (&sw)[kWalkItems], const uint32_t (&tw)[kWalkItems], uint32_t need,
                uint32_t (&xw)[kWalkItems]) {
#pragma unroll
                for (int k = 0; k < kWalkItems; ++k) {
                    const bool ld = ((need >> k) & 1u) && !(tw[k] & kLoopBit);
                    xw[k] = __builtin_amdgcn_raw_buffer_load_b32(xr, ld ? (sw[k] >> 5) * 4u : 0xFFFFFFF0u, 0, 0);
                }
            },
            [&](const uint32_t (&sw)[kWalkItems], const uint32_t (&tw)[kWalkItems], const uint32_t (&xw)[kWalkItems],
                uint32_t need, int j) {
                const uint32_t tbase = (uint32_t)j << kSliceBits;
                uint32_t loops = 0;
#pragma unroll
                for (int k = 0; k < kWalkItems; ++k) {
                    if (!((need >> k) & 1u)) continue;
                    if (tw[k] & kLoopBit)
                        loops |= 1u << k;
                    else if ((xw[k] >> (sw[k] & 31)) & 1u)
                        lds_set(tl, (tw[k] - tbase) & kOff);
                }
                // self-loops: rare.  A wave-uniform branch, so that the X2 read and its wait stay off the common path
                if (__builtin_amdgcn_ballot_w64(loops != 0) != 0) {
#pragma unroll
                    for (int k = 0; k < kWalkItems; ++k)
                        if (((loops >> k) & 1u) && gbit(X2, sw[k])) lds_set(tl, (tw[k] - tbase) & kOff);
                }
            },
            flush, begin, xissue, xconsume);
    } else {
        walk_chunks_n<kPoolBlock>(
            cw,
            [&](const uint2 (&pr)[kWalkItems], uint32_t valid, int j) {
                const uint32_t tbase = (uint32_t)j << kSliceBits;
                step([&](int k) { return pr[k].x; },
                     [&](int k) { return (pr[k].y - tbase) & ((1u << kSliceBits) - 1u); },
                     [&](int k) { return pr[k].x == pr[k].y; }, valid);
            },
            flush, begin);
    }
}

}  // namespace part

// ================================ host side =====================================================
static part::Layout make_layout(int64_t lo, int64_t hi, bool allow_packed) {
    part::Layout L;
    L.lo = lo;
    L.hi = hi;
    const uint64_t range = (uint64_t)(hi - lo);
    const uint64_t slice = uint64_t(1) << part::kSliceBits;
    L.nt = (int)((range + slice - 1) / slice);
    if (L.nt < 1) L.nt = 1;
    // source slices: 2^19 ids while nt * ns fits the cell histogram, coarser beyond that
    const uint64_t ns_max = (uint64_t)(part::kMaxCells / L.nt);
    L.sbits = part::kSliceBits;
    while (((range + (uint64_t(1) << L.sbits) - 1) >> L.sbits) > ns_max) ++L.sbits;
    L.ns = (int)((range + (uint64_t(1) << L.sbits) - 1) >> L.sbits);
    if (L.ns < 1) L.ns = 1;
    L.ncells = L.nt * L.ns;
    L.tbits = part::kSliceBits;
    L.packed = allow_packed && L.sbits + L.tbits <= 40;  // 5-byte cell keys
    return L;
}

static part::PairOut pair_out(const RelPart& rp) {
    part::PairOut o{};
    if (rp.L.packed) {
        o.w = P<uint32_t>(rp.pairs);
        o.b = reinterpret_cast<uint8_t*>(o.w + rp.cap);
    } else {
        o.p = P<uint2>(rp.pairs);
    }
    return o;
}

void lds_attr(const void* kernel, size_t bytes) {
    // set once per (device, kernel) and raised only when a launch needs more: the attribute call
    // costs host time on every query otherwise
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    const auto key = std::make_pair(dev, kernel);
    std::lock_guard<std::mutex> g(mu);
    auto it = done.find(key);
    if (it != done.end() && it->second >= bytes) return;
    HIP_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[key] = bytes;
}

template <typename K>
static void allow_lds(K kernel, size_t bytes) {
    lds_attr(reinterpret_cast<const void*>(kernel), bytes);
}

void chunk_partition(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                     int nt, bool swap, const part::Layout& L, int64_t g2_want, ChunkPart& cp, bool want_hist,
                     bool want_split, const NarrowRel* nar) {
    using namespace part;
    hipStream_t st = s->stream;
    cp.L = L;
    // the whole-line variant where its LDS fits with the cell counts (the choice does not follow want_hist:
    // the pool of a layout is the same whoever asks for it)
    const bool lines = scatter1l_lds(L.nt, L.ns, true, kP1Block, kP1Tile) <= (size_t)160 * 1024;
    // the split pool: the whole-line pass 1 without cell counts, where its 32-pair holds fit too; else pairs
    const bool split = want_split && lines && !want_hist &&
                       scatter1l_lds(L.nt, L.ns, false, kP1Block, kP1Tile, true) <= (size_t)160 * 1024;
    if (split)
        REQUIRE((uint64_t)(L.hi - L.lo) <= (uint64_t(1) << 30), CAPSMI_ERR_UNSUPPORTED,
                "the split pool keeps a flag in bit 31 of its target words: at most 2^30 ids");
    cp.split = split;
    // pass 1 grid: one 1024-lane block per CU, fewer for small inputs so the open chunks
    // (blocks x slices) stay within a few times the filled ones
    std::vector<int> g1(nt, 0);
    std::vector<int64_t> c0(nt, 0);
    int64_t pool_chunks = 0, mtot = 0;
    for (int i = 0; i < nt; ++i) {
        if (ms[i] <= 0) continue;
        const int64_t full = (ms[i] + kCh - 1) / kCh;
        // tiles per block: 8 for large inputs; small ones (a rank's 1/8 shard of C5: 2^22 relationships) take
        // 2, so the pass spreads over the CUs instead of 64 blocks walking 8 tiles each (124 us for 2^22
        // relationships at 64 blocks, round-5 kernel trace, profiles/r05_c5_small_trace_stats.csv)
        const int64_t tmin = ms[i] <= (int64_t(1) << 24) ? 2 : 8;
        int64_t g = std::min<int64_t>((int64_t)s->num_cus * (kSBlock / kP1Block),
                                      (ms[i] + tmin * (int64_t)kP1Tile - 1) / (tmin * (int64_t)kP1Tile));
        // (at most ~32 open chunks per filled one -- 64 for small inputs, whose pools are small anyway: a 1/8
        // shard of C5's 2^25 relationships got 32 blocks at the earlier bound of 8, and its three
        // partitions took 1.33 ms against 0.29 ms for the whole table's two)
        g = std::min<int64_t>(g, std::max<int64_t>(1, (tmin == 2 ? 64 : 32) * full / L.nt));
        g1[i] = (int)std::max<int64_t>(1, g);
        c0[i] = pool_chunks;
        pool_chunks += (int64_t)g1[i] * chunks_per_block(ms[i], g1[i], L.nt);
        mtot += ms[i];
    }
    REQUIRE(pool_chunks < (int64_t)INT32_MAX && mtot + 2 * kPad < (int64_t)UINT32_MAX, CAPSMI_ERR_UNSUPPORTED,
            "relationship table too large for the layout");
    const int64_t npool = pool_chunks > 0 ? pool_chunks : 1;
    const int hw = hist_words(L.ns);
    cp.pool = dev_alloc(sizeof(uint2) * kCh * (size_t)(npool + 1), s);  // + a trash chunk
    cp.meta = dev_alloc(sizeof(unsigned long long) * npool, s);
    cp.has_hist = want_hist;
    if (want_hist) cp.chist = dev_alloc(sizeof(uint32_t) * hw * (size_t)npool, s);
    // (clearing each block's metadata range inside pass 1 instead measured 5.25 -> 5.39 ms at C3: the fill stays)
    HIP_CHECK(hipMemsetAsync(P<void>(cp.meta), 0, sizeof(unsigned long long) * npool, st));
    const size_t lds1 = lines ? scatter1l_lds(L.nt, L.ns, want_hist, kP1Block, kP1Tile, split) : scatter1_lds(L.nt, L.ns, want_hist);
    auto k1 = split ? k_scatter_l<kP1Block, kItems, 4, false, true>
              : lines ? (want_hist ? k_scatter_l<kP1Block, kItems, 4, true> : k_scatter_l<kP1Block, kItems, 4, false>)
                    : (want_hist ? k_scatter_c<kP1Block, kItems, 4, kP1NT, true>
                                 : k_scatter_c<kP1Block, kItems, 4, kP1NT, false>);
    // the same instantiation over a table's 32-bit endpoint copies (NarrowRel), chosen per table
    using u32 = uint32_t;
    auto k1n = split ? k_scatter_l<kP1Block, kItems, 4, false, true, false, false, u32>
               : lines ? (want_hist ? k_scatter_l<kP1Block, kItems, 4, true, false, false, false, u32>
                                    : k_scatter_l<kP1Block, kItems, 4, false, false, false, false, u32>)
                     : (want_hist ? k_scatter_c<kP1Block, kItems, 4, kP1NT, true, u32>
                                  : k_scatter_c<kP1Block, kItems, 4, kP1NT, false, u32>);
    bool any_wide = false, any_narrow = false;
    for (int i = 0; i < nt; ++i)
        if (ms[i] > 0) (nar && nar[i].s ? any_narrow : any_wide) = true;
    if (any_wide || !any_narrow) allow_lds(k1, lds1);
    if (any_narrow) allow_lds(k1n, lds1);
    for (int i = 0; i < nt; ++i) {
        if (ms[i] <= 0) continue;
        uint2* pool = P<uint2>(cp.pool);
        unsigned long long* meta = P<unsigned long long>(cp.meta);
        uint32_t* chist = want_hist ? P<uint32_t>(cp.chist) : nullptr;
        if (nar && nar[i].s) {
            // a word w stands for the id base + w: the kernel sees the window shifted by -base (part::rel_id), so
            // rows outside it on either side fail the range test exactly as their int64 words do.  Unsigned: the
            // shift may wrap, hi - lo does not change.  Declared bytes: 8 read + 8 written per relationship
            // (the caller's own figure is the int64 columns').
            Layout Ln = L;
            Ln.lo = (int64_t)((uint64_t)L.lo - (uint64_t)nar[i].base);
            Ln.hi = (int64_t)((uint64_t)L.hi - (uint64_t)nar[i].base);
            KernelTimer kt(s, "part_scatter1", 16.0 * (double)ms[i]);
            hipLaunchKernelGGL(k1n, dim3(g1[i]), dim3(kP1Block), lds1, st, nar[i].s, nar[i].d, ms[i], Ln, swap ? 1 : 0,
                               c0[i], (size_t)npool * kCh, pool, meta, chist);
            s->routes["pass1_narrow"] += 1;
            continue;
        }
        KernelTimer kt(s, "part_scatter1");
        hipLaunchKernelGGL(k1, dim3(g1[i]), dim3(kP1Block), lds1, st, srcs[i], dsts[i], ms[i], L, swap ? 1 : 0, c0[i],
                           (size_t)npool * kCh, pool, meta, chist);
    }
    HIP_CHECK(hipGetLastError());
    cp.mtot = mtot;
    if (split) s->routes["pool_split"] += 1;
    chunk_order(s, L.nt, pool_chunks, g2_want, cp);
}

// used chunks (cp.meta: slice, fill) ordered by target slice and the block-balanced segment split
// of a consumer grid of g2 blocks; no host round trip
void chunk_order(capsmi_session* s, int nt, int64_t pool_chunks, int64_t g2_want, ChunkPart& cp) {
    using namespace part;
    hipStream_t st = s->stream;
    Layout L = cp.L;
    L.nt = nt;
    const int64_t npool = pool_chunks > 0 ? pool_chunks : 1;
    const int64_t g2 = std::max<int64_t>(1, std::min<int64_t>(g2_want, npool));
    cp.jbuf = dev_alloc(sizeof(int64_t) * (3 * (size_t)L.nt + 2 * (size_t)g2 + 3) + sizeof(uint32_t) * npool +
                             sizeof(int) * g2, s);
    int64_t* jcnt = P<int64_t>(cp.jbuf);
    int64_t* jst = jcnt + L.nt;        // nt + 1
    int64_t* jcur = jst + L.nt + 1;    // nt
    int64_t* kseg = jcur + L.nt;       // g2
    int64_t* segbase = kseg + g2;      // g2 + 1
    uint32_t* order = reinterpret_cast<uint32_t*>(segbase + g2 + 2);
    int* ja = reinterpret_cast<int*>(order + npool);
    if (npool <= kOrder1Max && L.nt <= kMaxTSlices && g2 <= 4096) {  // small pools: one launch
        hipLaunchKernelGGL(k_chunk_order1, dim3(1), dim3(kChunkBlock), 0, st, P<unsigned long long>(cp.meta),
                           pool_chunks, L.nt, g2, jst, order, segbase, ja);
        HIP_CHECK(hipGetLastError());
        cp.pool_chunks = pool_chunks;
        cp.npool = npool;
        cp.g2 = g2;
        cp.jst = jst;
        cp.segbase = segbase;
        cp.ja = ja;
        cp.order = order;
        return;
    }
    HIP_CHECK(hipMemsetAsync(jcnt, 0, sizeof(int64_t) * L.nt, st));
    const unsigned cg = (unsigned)((npool + kChunkPer - 1) / kChunkPer);
    hipLaunchKernelGGL(k_chunk_count, dim3(cg), dim3(kChunkBlock), sizeof(uint32_t) * L.nt, st,
                       P<unsigned long long>(cp.meta), pool_chunks, L.nt, jcnt);
    exclusive_scan_i64(jcnt, jst, L.nt, s);
    HIP_CHECK(hipMemcpyAsync(jcur, jst, sizeof(int64_t) * L.nt, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_chunk_place, dim3(cg), dim3(kChunkBlock), sizeof(uint32_t) * 2 * L.nt, st,
                       P<unsigned long long>(cp.meta), pool_chunks, L.nt,
                       reinterpret_cast<unsigned long long*>(jcur), order);
    hipLaunchKernelGGL(k_seg_count, dim3((unsigned)((g2 + 255) / 256)), dim3(256), 0, st, jst, L.nt, g2, kseg, ja);
    exclusive_scan_i64(kseg, segbase, g2, s);
    HIP_CHECK(hipGetLastError());
    cp.pool_chunks = pool_chunks;
    cp.npool = npool;
    cp.g2 = g2;
    cp.jst = jst;
    cp.segbase = segbase;
    cp.ja = ja;
    cp.order = order;
}

static part::ChunkWalk chunk_walk(const ChunkPart& cp) {
    return part::ChunkWalk{P<uint2>(cp.pool), P<unsigned long long>(cp.meta), cp.order, cp.jst, cp.segbase, cp.ja, cp.L.nt};
}

// Grid of the pool hops: one 1024-lane block per CU (64 KiB of LDS), fewer for small tables so that a
// block's share stays at 16 chunks or more.  Two blocks per CU, measured at C3 (plain bench, libraries alternating
// on one box, six runs each, profiles/r15_c3_ab.json): 7.445 ms per step against 7.247 ms for one, and 7.380 ms
// for the parent without the exchange.  Round 7 measured the same loss (8.89 / 8.99 against 8.70 / 8.67 ms) and
// put it down to the first encounters, of which a slice cut into twice the shares has more.  With hop 2's
// exchange (k_pool_hop2<true, XW>) a share no longer pays for the targets other shares have resolved, and two
// blocks per CU still lose 0.2 ms: so it is not the first encounters alone.  What is left, not told apart: a 64 KiB
// begin and flush per share and slice, twice the open ends, and hop 2's 128 VGPRs, which let one block run per
// CU, so the second half of the grid runs as a second round and not beside the first.  The X gathers' latency is
// hidden inside the one block: three steps per wave in flight (part::walk_chunks_st_pipe).
constexpr int kPoolBlocksPerCU = 1;
constexpr int64_t kPoolMinShare = 16 * (int64_t)part::kCh;  // pairs
static unsigned pool_grid(const capsmi_session* s, const ChunkPart& cp) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((int64_t)s->num_cus * kPoolBlocksPerCU, cp.mtot / kPoolMinShare));
}

// Where the pool hops run (CAPSMI_HOP2=auto): domains of at most 2^26 ids (2^19-id source slices, X = 8 MiB).
// Measured on tables of uniform in-degree d (profiles/r07_pool_sweep.json): there the pool's hops beat or tie
// pass 2 + k_hop_2d at every d from 32 down to 1, where no pair finds its target set and hop 2 reads X once per
// relationship (2^26 relationships: 0.80 against 0.82 ms after pass 1; d >= 4, 2^28 relationships: 1.36 against
// 1.52 ms).  Over 2^28 ids (X = 32 MiB) the pool's hop 2 lost at d = 1, 2 and 4 (4.38 / 3.35 / 3.09 ms against
// 3.03 ms for pass 2 + k_hop_2d), so larger domains keep the cells path.  A choice per build from a count of
// hop 1's first encounters (one X read each) was built and removed: below 2^26 ids it never chose the cells
// rightly, above it never the pool.
static bool pool_domain(const part::Layout& L) { return L.sbits == part::kSliceBits; }

static void cells_build(capsmi_session* s, RelPart& rp, const RelPartHop1* h1);

// hop 1 for a full a from the presence words rp.pres (one launch over the domain's words)
static void presence_hop1(capsmi_session* s, const RelPart& rp, const capsmi_bitmap* b, uint32_t* M, uint32_t* S1,
                          uint32_t* S2) {
    using namespace part;
    PresenceIn in{};
    in.n = (int)rp.pres.size();
    double bytes = 16.0 * (double)b->nwords;  // b_ok read, M, S1, S2 written
    for (int i = 0; i < in.n; ++i) {
        const PresenceRel& p = rp.pres[i];
        in.m[i] = p.m;
        in.l1[i] = p.l1;
        in.l2[i] = p.l2;
        in.nwords[i] = p.nwords;
        in.shift[i] = p.lo - rp.L.lo;
        bytes += 12.0 * (double)p.nwords;
    }
    KernelTimer kt(s, "hop1", bytes);
    hipLaunchKernelGGL(k_presence_hop1, dim3((unsigned)((b->nwords + 255) / 256)), dim3(256), 0, s->stream, in,
                       BitV{P<uint32_t>(b->words), b->full ? 1 : 0}, M, S1, S2, b->nwords);
    HIP_CHECK(hipGetLastError());
    s->routes["hop1_presence"] += 1;
}

void relpart_build(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms, int nt,
                   int64_t lo, int64_t hi, RelPart& rp, const RelPartHop1* h1, bool unpacked, const NarrowRel* nar,
                   const PresenceRel* pres) {
    REQUIRE(hi > lo && (uint64_t)(hi - lo) <= (uint64_t(1) << 30), CAPSMI_ERR_UNSUPPORTED,
            "partitioned layout needs an id domain of at most 2^30 ids");
    // the presence words, if every table with rows offers some that the domain may read (presence_rule.h)
    rp.pres.clear();
    if (pres && s->cfg.presence) {
        bool all = true;
        for (int i = 0; i < nt && all; ++i) {
            if (ms[i] <= 0) continue;
            all = pres[i].m && presence_usable(pres[i].lo, pres[i].hi, lo, hi) && (int)rp.pres.size() < part::kPresenceMax;
            if (all) rp.pres.push_back(pres[i]);
        }
        if (!all) rp.pres.clear();
    }
    using namespace part;
    hipStream_t st = s->stream;
    rp.L = make_layout(lo, hi, s->cfg.pairs != 2);  // config CAPSMI_PAIRS=uint2: 8-byte pairs
    // Only a layout kept for later queries (capsmi_relpart_build, the cache() route) is packed: pass 2
    // writing the packed form is slower (C3: 3.45 -> 3.9-4.45 ms unfused, 3.73 -> 4.14 ms with hop 1
    // fused) while each hop over it gains 0.2-0.4 ms (hop 1 1.30 -> 0.90, hop 2 1.57 -> 1.35 ms), so a
    // layout read by one query's two hops is left in 8-byte pairs
    if (h1 || unpacked) rp.L.packed = 0;
    const Layout& L = rp.L;
    REQUIRE(L.nt <= kMaxTSlices && L.ncells <= kMaxCells, CAPSMI_ERR_INTERNAL, "layout too large");
    if (h1)
        REQUIRE(h1->a->lo == lo && h1->a->hi == hi && h1->b->lo == lo && h1->b->hi == hi, CAPSMI_ERR_UNSUPPORTED,
                "partitioned 2-hop needs node scans over the layout's id domain");

    int64_t rows = 0;
    for (int i = 0; i < nt; ++i) rows += std::max<int64_t>(ms[i], 0);
    // a full a_ok: hop 1 needs no source test.  It then runs over the pool (k_pool_hop1) and the cells wait
    // until something needs them; with CAPSMI_HOP2=cells it rides on pass 2 as before.
    const bool full_a = h1 && h1->a->full;
    const bool pool_hop = full_a && rows > 0 && (s->cfg.hop2 == 1 || (s->cfg.hop2 == 0 && pool_domain(L)));
    const bool fuse = full_a && !pool_hop;
    ChunkPart& cp = rp.cp;
    // (measured and removed in round 6: a 6-byte pass-1 pool, u32 + u16 arrays per chunk -- pass 1 5.26 ->
    // 5.58 ms, pass 2 + hop 1 3.76 -> 4.45 ms at C3; both passes are bound by their LDS / VALU phases)
    // the pool hops read no cell counts: pass 1 leaves them out, and a later reader of the cells has
    // k_chunk_hist make them (cells_build)
    // and hop 1 reads no sources: the pool is split (CAPSMI_POOL), so it streams the target words alone
    chunk_partition(s, srcs, dsts, ms, nt, false, L, (int64_t)s->num_cus * (fuse ? 1 : 2), cp, !pool_hop,
                    pool_hop && s->cfg.pool_split, nar);
    rp.cells = false;
    rp.sel = -1;
    rp.kept = -1;  // known on the device (boff[ncells]); read only when asked (relpart_kept)
    rp.rows = cp.mtot;
    if (pool_hop && !rp.pres.empty()) {
        presence_hop1(s, rp, h1->b, h1->M, h1->S1, h1->S2);
        return;
    }
    if (pool_hop) {
        const size_t lds = sizeof(uint32_t) * kSliceWords;
        auto k = cp.split ? k_pool_hop1<true> : k_pool_hop1<false>;
        allow_lds(k, lds);
        // split: 4 B per pair and M written, declared since the caller's own figure is the pair format's
        KernelTimer kt(s, "hop1", cp.split ? 4.0 * (double)cp.mtot + 4.0 * (double)h1->b->nwords : 0.0);
        hipLaunchKernelGGL(k, dim3(pool_grid(s, cp)), dim3(kPoolBlock), lds, st, chunk_walk(cp),
                           BitV{P<uint32_t>(h1->b->words), h1->b->full ? 1 : 0}, h1->M, h1->S1, h1->S2, h1->b->nwords);
        HIP_CHECK(hipGetLastError());
        return;
    }
    cells_build(s, rp, fuse ? h1 : nullptr);
    if (h1 && !fuse) relpart_hop1(s, rp, h1->a, h1->b, h1->M, h1->S1, h1->S2);
}

void relpart_cells(capsmi_session* s, RelPart& rp) {
    if (!rp.cells) cells_build(s, rp, nullptr);
}

// stage 2: the kept pool -> cells (pass 2; with h1, hop 1 for a full a_ok fused into it); the pool is dropped
static void cells_build(capsmi_session* s, RelPart& rp, const RelPartHop1* h1) {
    using namespace part;
    hipStream_t st = s->stream;
    const Layout& L = rp.L;
    const bool fuse = h1 != nullptr;
    ChunkPart& cp = rp.cp;
    const int64_t g2 = cp.g2, mtot = cp.mtot;
    const int64_t maxg = g2 + L.nt;  // segments <= blocks + slices
    int64_t* jst = cp.jst;
    int64_t* segbase = cp.segbase;
    int* ja = cp.ja;
    uint32_t* order = cp.order;
    Buf& pool = cp.pool;
    Buf& meta = cp.meta;
    if (!cp.has_hist) {  // pass 1 ran without the cell counts: one more read of the pool
        cp.chist = dev_alloc(sizeof(uint32_t) * hist_words(L.ns) * (size_t)cp.npool, s);
        const unsigned hg = (unsigned)std::max<int64_t>(
            1, std::min<int64_t>((int64_t)s->num_cus * 8, (cp.pool_chunks + kHistBlock / 64 - 1) / (kHistBlock / 64)));
        KernelTimer kt(s, "part_chunk_hist");
        hipLaunchKernelGGL(k_chunk_hist, dim3(hg), dim3(kHistBlock), 0, st, P<uint2>(cp.pool),
                           P<unsigned long long>(cp.meta), cp.pool_chunks, L.ns, L.sbits, cp.split ? 1 : 0,
                           P<uint32_t>(cp.chist));
        HIP_CHECK(hipGetLastError());
        cp.has_hist = true;
        s->routes["chunk_hist"] += 1;
    }
    Buf& chist = cp.chist;
    Buf pbuf = dev_alloc(sizeof(uint32_t) * (size_t)maxg * L.ns, s);
    uint32_t* psum = P<uint32_t>(pbuf);
    Buf tot = dev_alloc(sizeof(int64_t) * L.ncells, s);
    hipLaunchKernelGGL(k_seg_sum, dim3((unsigned)maxg), dim3(1024), 0, st, P<uint32_t>(chist), order, jst, L.nt, g2,
                       segbase, ja, L.ns, psum);
    hipLaunchKernelGGL(k_seg_prefix, dim3((L.ncells + 255) / 256), dim3(256), 0, st, psum, jst, g2, segbase, ja, L,
                       P<int64_t>(tot));
    rp.boff = dev_alloc(sizeof(int64_t) * (L.ncells + 1), s);  // cell offsets
    exclusive_scan_i64(P<int64_t>(tot), P<int64_t>(rp.boff), L.ncells, s);
    HIP_CHECK(hipGetLastError());
    rp.cap = mtot + kPad;  // kept <= mtot; slack for the hops' whole-step loads and pass 2's trash stores
    rp.pairs = dev_alloc(L.packed ? 5 * (size_t)rp.cap : sizeof(uint2) * (size_t)rp.cap, s);

    Hop1Out ho{};
    if (fuse) ho = Hop1Out{BitV{P<uint32_t>(h1->b->words), h1->b->full ? 1 : 0}, h1->M, h1->S1, h1->S2, h1->b->nwords};
    const size_t lds2 = sizeof(uint2) * (size_t)kTile + s2_hold_bytes(L.ns, L.packed) +
                        sizeof(uint32_t) * (4 * L.ns + kSBlock / 64) + (fuse ? sizeof(uint32_t) * kSliceWords : 0);
    REQUIRE(lds2 <= (size_t)160 * 1024, CAPSMI_ERR_INTERNAL, "pass-2 LDS");
    REQUIRE(!cp.split || !(L.packed || fuse), CAPSMI_ERR_INTERNAL, "a split pool feeds the plain pass 2 only");
    auto k2 = cp.split ? k_scatter_s2<false, false, true>
              : L.packed ? k_scatter_s2<false, true> : fuse ? k_scatter_s2<true, false> : k_scatter_s2<false, false>;
    allow_lds(k2, lds2);
    {
        KernelTimer kt(s, fuse ? "part_scatter2_hop1" : "part_scatter2");
        hipLaunchKernelGGL(k2, dim3((unsigned)g2), dim3(kSBlock), lds2, st, P<void>(pool), P<unsigned long long>(meta),
                           order, jst, segbase, ja, psum, P<int64_t>(rp.boff), L, pair_out(rp), mtot, ho);
    }
    HIP_CHECK(hipGetLastError());
    rp.cells = true;
    rp.sel = 1;
    rp.cp = ChunkPart();  // the pool and its bookkeeping go back to the allocator (stream-ordered)
}

template <bool HOP1, bool SRC_FULL>
static void launch_hop(capsmi_session* s, const RelPart& rp, part::BitV sb, const uint32_t* X2, part::BitV tmask,
                       uint32_t* out, uint32_t* S1, uint32_t* S2, int64_t gwords) {
    const size_t lds = sizeof(uint32_t) * 2 * part::kSliceWords;
    auto k = rp.L.packed ? part::k_hop_2d<HOP1, SRC_FULL, true> : part::k_hop_2d<HOP1, SRC_FULL, false>;
    allow_lds(k, lds);
    // one 128 KiB-LDS block per CU at a time; a few rounds of blocks, equal relationship shares
    // (at least kBlock * kUnroll each; blocks past the end exit at once).  Grid sized from the upper
    // bound of the kept count (the table rows), the exact count is read by the kernel.
    const int64_t min_per = (int64_t)part::kBlock * part::kUnroll;
    int64_t blocks = (int64_t)s->num_cus * 4;
    const int64_t bound = rp.kept >= 0 ? rp.kept : rp.rows;
    blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, (bound + min_per - 1) / min_per));
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(part::kBlock), lds, s->stream, pair_out(rp),
                       P<int64_t>(rp.boff), min_per, rp.L, sb, X2, tmask, out, S1, S2, gwords);
    HIP_CHECK(hipGetLastError());
}

void relpart_hop1(capsmi_session* s, RelPart& rp, const capsmi_bitmap* a, const capsmi_bitmap* b, uint32_t* M,
                  uint32_t* S1, uint32_t* S2) {
    REQUIRE(a->lo == rp.L.lo && a->hi == rp.L.hi && b->lo == rp.L.lo && b->hi == rp.L.hi, CAPSMI_ERR_UNSUPPORTED,
            "partitioned 2-hop needs node scans over the layout's id domain");
    if (rp.rows == 0) return;
    relpart_cells(s, rp);
    const part::BitV av{P<uint32_t>(a->words), a->full ? 1 : 0}, bv{P<uint32_t>(b->words), b->full ? 1 : 0};
    if (a->full && !rp.pres.empty() && s->cfg.presence) return presence_hop1(s, rp, b, M, S1, S2);
    KernelTimer kt(s, "hop1");
    if (a->full)
        launch_hop<true, true>(s, rp, av, nullptr, bv, M, S1, S2, b->nwords);
    else
        launch_hop<true, false>(s, rp, av, nullptr, bv, M, S1, S2, b->nwords);
}

void relpart_hop2(capsmi_session* s, RelPart& rp, const capsmi_bitmap* c, const uint32_t* X1, const uint32_t* X2,
                  uint32_t* C) {
    REQUIRE(c->lo == rp.L.lo && c->hi == rp.L.hi, CAPSMI_ERR_UNSUPPORTED,
            "partitioned 2-hop needs node scans over the layout's id domain");
    if (rp.rows == 0) return;
    const part::BitV xv{X1, 0}, cv{P<uint32_t>(c->words), c->full ? 1 : 0};
    if (!rp.cells) {
        // a handle that ran hop 1 over its pool and has built no cells since: hop 2 walks the pool too
        if (rp.sel < 0) rp.sel = 0;
        if (rp.sel == 0) {
            using namespace part;
            const size_t lds = sizeof(uint32_t) * kSliceWords;
            const bool xchg = rp.cp.split && s->cfg.hop2_exchange;
            auto k = xchg ? k_pool_hop2<true, kPoolXchgWindows> : rp.cp.split ? k_pool_hop2<true> : k_pool_hop2<false>;
            allow_lds(k, lds);
            KernelTimer kt(s, "hop2");
            hipLaunchKernelGGL(k, dim3(pool_grid(s, rp.cp)), dim3(kPoolBlock), lds, s->stream, chunk_walk(rp.cp),
                               X1, X2, cv, C, c->nwords);
            HIP_CHECK(hipGetLastError());
            s->routes["hop2_pool"] += 1;
            if (xchg) s->routes["hop2_exchange"] += 1;
            return;
        }
        relpart_cells(s, rp);
    }
    s->routes["hop2_cells"] += 1;
    KernelTimer kt(s, "hop2");
    launch_hop<false, false>(s, rp, xv, X2, cv, C, nullptr, nullptr, c->nwords);
}

// ---- layout digest (test support): per cell, pair count and wrapping sum of a 64-bit mix ----------------
__device__ __forceinline__ uint64_t pair_mix(uint2 p) {
    uint64_t z = ((uint64_t)p.x << 32 | p.y) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256) k_cell_digest(part::PairOut pairs, const int64_t* __restrict__ boff,
                                                    part::Layout L, unsigned long long* __restrict__ sums,
                                                    unsigned long long* __restrict__ bad) {
    const int c = blockIdx.x;
    const uint32_t sbase = (uint32_t)(c % L.ns) << L.sbits, tbase = (uint32_t)(c / L.ns) << L.tbits;
    unsigned long long acc = 0, nb = 0;
    for (int64_t i = boff[c] + threadIdx.x; i < boff[c + 1]; i += 256) {
        // packed: the pair comes back through its cell, so a misplaced one shows as a wrong sum
        const uint2 p = L.packed ? part::key_pair(L, sbase, tbase, pairs.w[i], pairs.b[i]) : pairs.p[i];
        acc += pair_mix(p);
        if (part::cell_of(L, p.x, p.y) != c) ++nb;
    }
    atomicAdd(&sums[c], acc);
    if (nb) atomicAdd(bad, nb);
}

void relpart_digest(capsmi_session* s, RelPart& rp, int64_t* counts, uint64_t* sums, int64_t* misplaced) {
    relpart_cells(s, rp);
    hipStream_t st = s->stream;
    const int nc = rp.L.ncells;
    std::vector<int64_t> off(nc + 1, 0);
    Buf d = dev_alloc(sizeof(unsigned long long) * (nc + 1), s);
    HIP_CHECK(hipMemsetAsync(P<void>(d), 0, sizeof(unsigned long long) * (nc + 1), st));
    if (rp.rows > 0) {
        hipLaunchKernelGGL(k_cell_digest, dim3(nc), dim3(256), 0, st, pair_out(rp), P<int64_t>(rp.boff), rp.L,
                           P<unsigned long long>(d), P<unsigned long long>(d) + nc);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(off.data(), P<void>(rp.boff), sizeof(int64_t) * (nc + 1), hipMemcpyDeviceToHost, st));
    }
    std::vector<unsigned long long> h(nc + 1);
    HIP_CHECK(hipMemcpyAsync(h.data(), P<void>(d), sizeof(unsigned long long) * (nc + 1), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int c = 0; c < nc; ++c) {
        counts[c] = off[c + 1] - off[c];
        sums[c] = h[c];
    }
    *misplaced = (int64_t)h[nc];
}

int64_t relpart_kept(capsmi_session* s, RelPart& rp) {
    relpart_cells(s, rp);
    if (rp.kept < 0) rp.kept = rp.rows > 0 ? read_scalar(s, P<int64_t>(rp.boff) + rp.L.ncells) : 0;
    return rp.kept;
}

}  // namespace capsmi
