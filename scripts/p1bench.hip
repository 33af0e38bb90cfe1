// Pass-1 microbenchmark (not shipped): times k_scatter_c / k_scatter_l against a copy floor with the same
// access pattern (16-B loads of both int64 columns, packed 8-B pairs written linearly) on uniform
// random (source, target) ids over 2^26; the *_n rows are the same kernels and floors over the columns'
// 32-bit copies (8 B read + 8 B written per relationship); floor_split1_n / floor_split4_n write the split pool's
// two word arrays with 4-byte and with 16-byte stores.  Build: see scripts/p1bench.sh; run on the GPU box.
#include "../cypher-for-apache-spark_amd/csrc/k_part.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace capsmi;
using namespace capsmi::part;

#define CK(x)                                                                     \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

__global__ void k_gen(int64_t* __restrict__ a, int64_t* __restrict__ b, int64_t m, int bits) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        a[i] = (int64_t)(z & ((1ull << bits) - 1));
        b[i] = (int64_t)((z >> 32) & ((1ull << bits) - 1));
    }
}

// the endpoint columns' 32-bit copies, as registration makes them (base 0 here)
__global__ void k_narrow(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t m, uint32_t* __restrict__ oa,
                         uint32_t* __restrict__ ob) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        oa[i] = (uint32_t)a[i];
        ob[i] = (uint32_t)b[i];
    }
}

// copy floor: same loads as pass 1 (load_tile: 16-B loads of both columns, int64 or their 32-bit copies), pairs
// written linearly with 16-B stores -- 16 + 8 B per relationship, or 8 + 8 B over the copies
template <bool NTL, bool NTS, typename IdT = int64_t>
__global__ void __launch_bounds__(kP1Block) k_floor(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                   int64_t m, uint2* __restrict__ out) {
    IdT sr[kItems], tr[kItems];
    const int64_t stride = (int64_t)gridDim.x * kP1Tile;
    int64_t t0 = (int64_t)blockIdx.x * kP1Tile;
    if (t0 < m) load_tile<kP1Block, NTL>(src, dst, t0, m, true, sr, tr);
    for (; t0 < m; t0 += stride) {
        uint4 v[kItems / 2];
#pragma unroll
        for (int k = 0; k < kItems / 2; ++k)
            v[k] = make_uint4((uint32_t)sr[2 * k], (uint32_t)tr[2 * k], (uint32_t)sr[2 * k + 1], (uint32_t)tr[2 * k + 1]);
        if (t0 + stride < m) load_tile<kP1Block, NTL>(src, dst, t0 + stride, m, true, sr, tr);
#pragma unroll
        for (int k = 0; k < kItems / 2; ++k) {  // items 2k and 2k + 1 are neighbours in both item orders
            typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
            v4u32 w = {v[k].x, v[k].y, v[k].z, v[k].w};
            const int64_t at = t0 + tile_item_off<kP1Block, IdT>(2 * k);
            if (at + 1 >= m) continue;
            v4u32* q = reinterpret_cast<v4u32*>(out + at);
            if (NTS) __builtin_nontemporal_store(w, q); else *q = w;
        }
    }
}

// Store-shape floors of the split pool over k_floor's loads: the same 8 B read and 8 B written per relationship,
// the target words into one array and the source words into another (both linear).  G = 1: one 4-byte store per
// pair and array, a wave-instruction writing 256 contiguous bytes, as the split store loop issued them before it
// took groups; G = 4: one 16-byte store per four pairs and array, as it issues them now.  Their difference is
// what the store shape alone owns.
template <int G, typename IdT>
__global__ void __launch_bounds__(kP1Block) k_floor_split(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                         int64_t m, uint2* __restrict__ out) {
    static_assert(G == 1 || G == 4, "one word or one 16-byte store per array");
    typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));
    IdT sr[kItems], tr[kItems];
    uint32_t* tw = reinterpret_cast<uint32_t*>(out);
    uint32_t* sw = tw + ((m + 3) & ~int64_t(3));
    const int64_t stride = (int64_t)gridDim.x * kP1Tile;
    int64_t t0 = (int64_t)blockIdx.x * kP1Tile;
    if (t0 < m) load_tile<kP1Block, false>(src, dst, t0, m, true, sr, tr);
    for (; t0 < m; t0 += stride) {
        uint32_t x[kItems], y[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            x[k] = (uint32_t)sr[k];
            y[k] = (uint32_t)tr[k] | (sr[k] == tr[k] ? kLoopBit : 0u);
        }
        if (t0 + stride < m) load_tile<kP1Block, false>(src, dst, t0 + stride, m, true, sr, tr);
#pragma unroll
        for (int k = 0; k < kItems / G; ++k) {  // lane i takes positions G * (k * B + i) ... + G - 1 of the tile
            const int64_t at = t0 + (int64_t)G * (k * kP1Block + (int)threadIdx.x);
            if (at + G > m) continue;
            if (G == 1) {
                tw[at] = y[k];
                sw[at] = x[k];
            } else {
                const v4u32 t = {y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]};
                const v4u32 s = {x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]};
                *reinterpret_cast<v4u32*>(tw + at) = t;
                *reinterpret_cast<v4u32*>(sw + at) = s;
            }
        }
    }
}

// validation: every used chunk's pairs lie in its slice and match its histogram row; per-slice
// pair checksums (sum and xor of a mix of the pair) for comparison across kernels
__global__ void k_check(const uint2* __restrict__ pool, const unsigned long long* __restrict__ meta,
                        const uint32_t* __restrict__ chist, int64_t npool, Layout L,
                        unsigned long long* __restrict__ sums, unsigned long long* __restrict__ bad, int cs) {
    __shared__ uint32_t h[2048];
    const int64_t q = blockIdx.x;
    if (q >= npool) return;
    const uint32_t fill = (uint32_t)(meta[q] >> 32), j = (uint32_t)meta[q];
    if (!fill) return;
    for (int i = threadIdx.x; i < L.ns; i += blockDim.x) h[i] = 0;
    __syncthreads();
    unsigned long long sa = 0, sx = 0, nb = 0;
    for (uint32_t i = threadIdx.x; i < fill; i += blockDim.x) {
        const uint2 p = pool[(size_t)q * cs + i];
        if ((p.y >> L.tbits) != j) ++nb;
        atomicAdd(&h[p.x >> L.sbits], 1u);
        uint64_t z = ((uint64_t)p.x << 32 | p.y) * 0x9E3779B97F4A7C15ull;
        z ^= z >> 29;
        sa += z;
        sx ^= z;
    }
    __syncthreads();
    const int hw = hist_words(L.ns);
    for (int i = threadIdx.x; i < L.ns; i += blockDim.x) {
        const uint32_t v = (chist[(size_t)q * hw + (i >> 1)] >> ((i & 1) * 16)) & 0xFFFFu;
        if (v != h[i]) ++nb;
    }
    if (nb) atomicAdd(bad, nb);
    atomicAdd(&sums[2 * j], sa);
    atomicXor(&sums[2 * j + 1], sx);
}

int main(int argc, char** argv) {
    const int bits = 26;
    const int64_t m = argc > 1 ? atoll(argv[1]) : (int64_t(1) << 30);
    int dev_cus = 0;
    CK(hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, 0));
    int64_t *src, *dst;
    CK(hipMalloc(&src, 8 * m));
    CK(hipMalloc(&dst, 8 * m));
    hipLaunchKernelGGL(k_gen, dim3(4096), dim3(256), 0, 0, src, dst, m, bits);
    uint32_t *src32, *dst32;
    CK(hipMalloc(&src32, 4 * m));
    CK(hipMalloc(&dst32, 4 * m));
    hipLaunchKernelGGL(k_narrow, dim3(4096), dim3(256), 0, 0, src, dst, m, src32, dst32);
    Layout L;
    L.lo = 0;
    L.hi = int64_t(1) << bits;
    L.nt = 128;
    L.ns = 128;
    L.sbits = 19;
    L.tbits = 19;
    L.ncells = L.nt * L.ns;
    struct V {
        const char* name;
        const void* fn;
        int block, tile, gmul, floor;  // floor: 0 k_scatter_c, 1 copy floor, 2 k_scatter_l
        bool hist, split, narrow;  // narrow: over the 32-bit copies (8 B read + 8 B written per relationship)
    };
    // the library's instantiations (chunk_partition) and the copy floors
    const V vs[] = {
        {"sc_hist", (const void*)k_scatter_c<1024, 8, 4, false, true>, 1024, 8192, 1, 0, true, false},
        {"sl_hist", (const void*)k_scatter_l<1024, 8, 4, true>, 1024, 8192, 1, 2, true, false},
        {"sl_pairs", (const void*)k_scatter_l<1024, 8, 4, false>, 1024, 8192, 1, 2, false, false},
        {"sl_split", (const void*)k_scatter_l<1024, 8, 4, false, true>, 1024, 8192, 1, 2, false, true},
        {"floor", (const void*)k_floor<false, false>, 1024, 8192, 1, 1, false, false},
        {"floor_ntls", (const void*)k_floor<true, true>, 1024, 8192, 1, 1, false, false},
        {"sc_hist_n", (const void*)k_scatter_c<1024, 8, 4, false, true, uint32_t>, 1024, 8192, 1, 0, true, false, true},
        {"sl_hist_n", (const void*)k_scatter_l<1024, 8, 4, true, false, false, false, uint32_t>, 1024, 8192, 1, 2, true, false, true},
        {"sl_pairs_n", (const void*)k_scatter_l<1024, 8, 4, false, false, false, false, uint32_t>, 1024, 8192, 1, 2, false, false, true},
        {"sl_split_n", (const void*)k_scatter_l<1024, 8, 4, false, true, false, false, uint32_t>, 1024, 8192, 1, 2, false, true, true},
        {"floor_n", (const void*)k_floor<false, false, uint32_t>, 1024, 8192, 1, 1, false, false, true},
        {"floor_ntls_n", (const void*)k_floor<true, true, uint32_t>, 1024, 8192, 1, 1, false, false, true},
        {"floor_split1_n", (const void*)k_floor_split<1, uint32_t>, 1024, 8192, 1, 1, false, false, true},
        {"floor_split4_n", (const void*)k_floor_split<4, uint32_t>, 1024, 8192, 1, 1, false, false, true},
    };
    const int nv = sizeof(vs) / sizeof(vs[0]);
    int64_t npool = 1;
    for (int v = 0; v < nv; ++v) {
        const int64_t g = (int64_t)dev_cus * vs[v].gmul;
        const int64_t c = g * chunks_per_block(m, g, L.nt, vs[v].tile);
        npool = c > npool ? c : npool;
    }
    const int hw = hist_words(L.ns);
    uint2* pool;
    unsigned long long* meta;
    uint32_t* chist;
    CK(hipMalloc(&pool, sizeof(uint2) * (kCh + 1024) * (size_t)(npool + 1)));
    CK(hipMalloc(&meta, 8 * npool));
    CK(hipMalloc(&chist, 4 * hw * (size_t)npool));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    int64_t* dcount;
    CK(hipMalloc(&dcount, 8));
    for (int v = 0; v < nv; ++v) {
        const int64_t g = (int64_t)dev_cus * vs[v].gmul;
        const size_t lds = vs[v].floor == 1 ? 0 : vs[v].floor == 2 ? scatter1l_lds(L.nt, L.ns, vs[v].hist, vs[v].block, vs[v].tile, vs[v].split)
                                                                : scatter1_lds(L.nt, L.ns, vs[v].hist, vs[v].block, vs[v].tile);
        if (lds) CK(hipFuncSetAttribute(vs[v].fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const double bytes = (vs[v].narrow ? 16.0 : 24.0) * (double)m;
        const void* a0 = vs[v].narrow ? (const void*)src32 : (const void*)src;
        const void* a1 = vs[v].narrow ? (const void*)dst32 : (const void*)dst;
        float best = 1e30f, sum = 0;
        for (int r = 0; r < 6; ++r) {
            CK(hipMemsetAsync(meta, 0, 8 * npool, 0));
            CK(hipEventRecord(e0, 0));
            if (vs[v].floor == 1) {
                void* args[] = {&a0, &a1, (void*)&m, &pool};
                CK(hipLaunchKernel(vs[v].fn, dim3(g), dim3(vs[v].block), args, 0, 0));
            } else if (vs[v].floor == 2) {
                int swap = 0;
                int64_t c0 = 0;
                size_t trash = (size_t)npool * kCh;
                void* args[] = {&a0, &a1, (void*)&m, &L, &swap, &c0, &trash, &pool, &meta, &chist};
                CK(hipLaunchKernel(vs[v].fn, dim3(g), dim3(vs[v].block), args, lds, 0));
            } else {
                int swap = 0;
                int64_t c0 = 0;
                size_t trash = (size_t)npool * kCh;
                void* args[] = {&a0, &a1, (void*)&m, &L, &swap, &c0, &trash, &pool, &meta, &chist};
                CK(hipLaunchKernel(vs[v].fn, dim3(g), dim3(vs[v].block), args, lds, 0));
            }
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r) {
                best = ms < best ? ms : best;
                sum += ms;
            }
        }
        // check: total fill over chunk metadata == m; chunks consistent with their histograms
        unsigned long long tot = 0, nbad = 0, sig = 0;
        if (vs[v].floor != 1 && vs[v].hist) {  // k_check reads pairs and their histogram rows
            unsigned long long* d;
            CK(hipMalloc(&d, 8 * (2 * L.nt + 1)));
            CK(hipMemset(d, 0, 8 * (2 * L.nt + 1)));
            hipLaunchKernelGGL(k_check, dim3(npool), dim3(256), 0, 0, pool, meta, chist, npool, L, d, d + 2 * L.nt, kCh);
            std::vector<unsigned long long> hs(2 * L.nt + 1);
            CK(hipMemcpy(hs.data(), d, 8 * hs.size(), hipMemcpyDeviceToHost));
            nbad = hs[2 * L.nt];
            for (int j = 0; j < 2 * L.nt; ++j) sig = sig * 0x100000001B3ull + hs[j];
            CK(hipFree(d));
        }
        if (vs[v].floor != 1) {
            std::vector<unsigned long long> h(npool);
            CK(hipMemcpy(h.data(), meta, 8 * npool, hipMemcpyDeviceToHost));
            for (auto x : h) tot += x >> 32;
        }
        printf("%-14s best %.3f ms avg %.3f ms  %.0f GB/s  filled=%llu bad=%llu sig=%016llx\n", vs[v].name, best,
               sum / 5, bytes / (best * 1e6), tot, nbad, sig);
        fflush(stdout);
    }
    return 0;
}
