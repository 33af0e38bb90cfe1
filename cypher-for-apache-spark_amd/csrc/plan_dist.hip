// plan_dist.hip -- the fused routes' bodies over a distributed graph (capsmi_graph_distribute, k_dist.hip; g_dist.on):
// the scanned tables are this rank's shards and the steps exchange through the session's collective.
#include "plan_impl.h"

namespace capsmi {
namespace planning {

int64_t sum_over_ranks(capsmi_session* s, int64_t v) {
    Buf t = dev_alloc(sizeof(int64_t), s);
    fill_i64(P<int64_t>(t), v, 1, s->stream);
    collective(s, CAPSMI_COLL_ALL_REDUCE_SUM, P<int64_t>(t), P<int64_t>(t), 1, CAPSMI_I64);
    return read_scalar(s, P<int64_t>(t));
}

namespace {

unsigned small_grid(capsmi_session* s, int64_t n) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)s->num_cus * 8));
}

// the owned X1 / X2 slices side by side (one all-gather for both), and back into [X1 | X2] after it
__global__ void k_pack_x12(const uint32_t* __restrict__ mid, int64_t nw, int64_t S, int64_t r, uint32_t* __restrict__ send) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * S; i += (int64_t)gridDim.x * blockDim.x)
        send[i] = mid[(i < S ? 0 : nw) + r * S + (i < S ? i : i - S)];
}
__global__ void k_unpack_x12(const uint32_t* __restrict__ got, int64_t nw, int64_t S, uint32_t* __restrict__ full) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * nw; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = (i / S) >> 1, h = (i / S) & 1, k = i % S;  // got = [rank][X1 | X2][S]
        full[h * nw + q * S + k] = got[i];
    }
}

}  // namespace

// 2-hop count(DISTINCT end) over relationship shards BY_TARGET: hop 1 is complete for the
// middle ids this rank owns (their in-relationships are all here), one all-gather of the owned slices of
// the frontier (X1, X2) gives every rank the whole frontier, hop 2 marks the end ids this rank owns, and
// the owned popcounts add up in one all-reduce.  `cached`: the relationship layout kept by cache().
int64_t dist_two_hop_distinct(capsmi_session* s, const capsmi_relpart* cached, int32_t nt, capsmi_table* const* views,
                              const capsmi_bitmap* a, const capsmi_bitmap* b, const capsmi_bitmap* c) {
    const int64_t S = g_dist.slice_words, nw = b->nwords, r = g_dist.rank;
    REQUIRE(nw == S * g_dist.world, CAPSMI_ERR_INTERNAL, "distributed bitmap geometry");
    Buf mid = dev_alloc(sizeof(uint32_t) * 2 * nw, s), scratch = dev_alloc(sizeof(uint32_t) * nw, s);
    Buf full = dev_alloc(sizeof(uint32_t) * 2 * nw, s), dst = dev_alloc(sizeof(uint32_t) * nw, s);
    capsmi_relpart* rp = nullptr;
    if (cached) check(capsmi_two_hop_mark_mid_part(s, cached, a, b, P<uint32_t>(mid), P<uint32_t>(scratch)));
    else check(capsmi_relpart_build_mark_mid(s, nt, views, "s", "t", a, b, P<uint32_t>(mid), P<uint32_t>(scratch), &rp));
    std::unique_ptr<capsmi_relpart, capsmi_status (*)(capsmi_relpart*)> hold(rp, capsmi_relpart_release);
    {  // one all-gather of the owned (X1, X2) slice pairs instead of one per frontier
        Buf x12 = dev_alloc(sizeof(uint32_t) * (2 * S + 2 * nw), s);
        uint32_t *send = P<uint32_t>(x12), *got = send + 2 * S;
        hipLaunchKernelGGL(k_pack_x12, dim3(small_grid(s, 2 * S)), dim3(256), 0, s->stream, P<uint32_t>(mid), nw, S, r, send);
        HIP_CHECK(hipGetLastError());
        collective(s, CAPSMI_COLL_ALL_GATHER, send, got, 2 * S, CAPSMI_COLL_U32);
        hipLaunchKernelGGL(k_unpack_x12, dim3(small_grid(s, 2 * nw)), dim3(256), 0, s->stream, got, nw, S, P<uint32_t>(full));
        HIP_CHECK(hipGetLastError());
    }
    check(capsmi_two_hop_mark_dst_part(s, cached ? cached : rp, b, c, P<uint32_t>(full), P<uint32_t>(dst)));
    Buf cnt = dev_alloc(sizeof(int64_t), s);
    check(capsmi_words_popcount_device(s, P<uint32_t>(dst), r * S, (r + 1) * S, P<int64_t>(cnt)));
    collective(s, CAPSMI_COLL_ALL_REDUCE_SUM, P<int64_t>(cnt), P<int64_t>(cnt), 1, CAPSMI_I64);
    return read_scalar(s, P<int64_t>(cnt));
}

namespace {

// [X1 | X2] (2 x W x S words) -> rank-major send segments [q][X1 slice q | X2 slice q] (2 x S each)
__global__ void k_x12_by_owner(const uint32_t* __restrict__ mid, int64_t nw, int64_t S, int W, uint32_t* __restrict__ send) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * nw; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = i / (2 * S), h = (i / S) & 1, k = i % S;
        send[i] = mid[h * nw + q * S + k];
    }
}
// OR of the W received [X1 | X2] slice pairs (got = [source rank][2][S]) into this rank's slices of full
// [X1 | X2] (words outside them zero: hop 2 reads X only at the owned sources of this rank's relationships)
__global__ void k_x12_or(const uint32_t* __restrict__ got, int W, int64_t nw, int64_t S, int64_t r,
                         uint32_t* __restrict__ full) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * S; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t v = 0;
        for (int q = 0; q < W; ++q) v |= got[(int64_t)q * 2 * S + i];
        const int64_t h = i / S, k = i % S;
        full[h * nw + r * S + k] = v;
    }
}
// popcount of the OR of W received slices of S words (got = [source rank][S]) added into *cnt
__global__ void k_or_popcount(const uint32_t* __restrict__ got, int W, int64_t S, unsigned long long* __restrict__ cnt) {
    unsigned long long c = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < S; k += (int64_t)gridDim.x * blockDim.x) {
        uint32_t v = 0;
        for (int q = 0; q < W; ++q) v |= got[(int64_t)q * S + k];
        c += __popc(v);
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(cnt, c);
}

// The union of every rank's partial bitmap `words` (W x S words, rank-major slices) counted: one equal-count
// ALL_TO_ALL_V gives each rank every rank's copy of its owned slice, ORed and popcounted on the device, and
// one all-reduce adds the owned counts -- the reduce-scatter(OR) + popcount of SURVEY.md 8e (bitwise OR is
// not an RCCL reduction).  Returns the count (the step's one host read).
int64_t or_reduce_count(capsmi_session* s, const uint32_t* words) {
    const int64_t S = g_dist.slice_words;
    const int W = g_dist.world;
    Buf got = dev_alloc(sizeof(uint32_t) * (size_t)W * S, s), cnt = dev_alloc(sizeof(int64_t), s);
    std::vector<int64_t> c(W, S);
    collective_a2av(s, words, c.data(), P<void>(got), c.data(), CAPSMI_COLL_U32, S);
    HIP_CHECK(hipMemsetAsync(P<void>(cnt), 0, sizeof(int64_t), s->stream));
    hipLaunchKernelGGL(k_or_popcount, dim3(small_grid(s, S)), dim3(256), 0, s->stream, P<uint32_t>(got), W, S,
                       P<unsigned long long>(cnt));
    HIP_CHECK(hipGetLastError());
    collective(s, CAPSMI_COLL_ALL_REDUCE_SUM, P<int64_t>(cnt), P<int64_t>(cnt), 1, CAPSMI_I64);
    return read_scalar(s, P<int64_t>(cnt));
}

}  // namespace

// 2-hop count(DISTINCT end) over relationship shards BY_SOURCE (north_star's owner(source)):
// hop 1 over this rank's relationships (sources owned, middles anywhere) marks a partial frontier
// X1 = M | S1, X2 = M | S2 for every id -- S1 / S2 (self-loops) are complete on the owner, and M is an OR
// over the ranks; one ALL_TO_ALL_V of the slices + OR gives each rank the whole frontier of its owned
// middles, which are exactly the sources of its hop-2 relationships; hop 2 marks ends anywhere, and the
// OR-reduce + popcount of the end bitmap gives the answer (or_reduce_count).
int64_t dist_two_hop_distinct_src(capsmi_session* s, const capsmi_relpart* cached, int32_t nt, capsmi_table* const* views,
                                  const capsmi_bitmap* a, const capsmi_bitmap* b, const capsmi_bitmap* c) {
    const int64_t S = g_dist.slice_words, nw = b->nwords, r = g_dist.rank;
    const int W = g_dist.world;
    REQUIRE(nw == S * W, CAPSMI_ERR_INTERNAL, "distributed bitmap geometry");
    Buf mid = dev_alloc(sizeof(uint32_t) * 2 * nw, s), scratch = dev_alloc(sizeof(uint32_t) * nw, s);
    Buf full = dev_alloc(sizeof(uint32_t) * 2 * nw, s), dst = dev_alloc(sizeof(uint32_t) * nw, s);
    capsmi_relpart* rp = nullptr;
    if (cached) check(capsmi_two_hop_mark_mid_part(s, cached, a, b, P<uint32_t>(mid), P<uint32_t>(scratch)));
    else check(capsmi_relpart_build_mark_mid(s, nt, views, "s", "t", a, b, P<uint32_t>(mid), P<uint32_t>(scratch), &rp));
    std::unique_ptr<capsmi_relpart, capsmi_status (*)(capsmi_relpart*)> hold(rp, capsmi_relpart_release);
    {
        Buf x12 = dev_alloc(sizeof(uint32_t) * 4 * nw, s);
        uint32_t *send = P<uint32_t>(x12), *got = send + 2 * nw;
        hipLaunchKernelGGL(k_x12_by_owner, dim3(small_grid(s, 2 * nw)), dim3(256), 0, s->stream, P<uint32_t>(mid), nw, S,
                           W, send);
        HIP_CHECK(hipGetLastError());
        std::vector<int64_t> cnt(W, 2 * S);
        collective_a2av(s, send, cnt.data(), got, cnt.data(), CAPSMI_COLL_U32, 2 * S);
        HIP_CHECK(hipMemsetAsync(P<void>(full), 0, sizeof(uint32_t) * 2 * nw, s->stream));
        hipLaunchKernelGGL(k_x12_or, dim3(small_grid(s, 2 * S)), dim3(256), 0, s->stream, got, W, nw, S, r,
                           P<uint32_t>(full));
        HIP_CHECK(hipGetLastError());
    }
    check(capsmi_two_hop_mark_dst_part(s, cached ? cached : rp, b, c, P<uint32_t>(full), P<uint32_t>(dst)));
    return or_reduce_count(s, P<uint32_t>(dst));
}

// 2-hop count(*) over relationship shards BY_TARGET: each rank's relationships into its owned ids give
// their complete in-degrees inA; one all-gather of the owned slices gives every rank inA of every id; each
// rank sums inA(source) over its relationships (less its self-loops) and one all-reduce adds the parts
int64_t dist_two_hop_count(capsmi_session* s, int32_t nt, capsmi_table* const* views, const capsmi_bitmap* a,
                           const capsmi_bitmap* b, const capsmi_bitmap* c) {
    const int64_t S = g_dist.slice_words, n = b->hi - b->lo, r = g_dist.rank;
    const int64_t own_lo = r * 32 * S, own_hi = std::min(own_lo + 32 * S, n);
    Buf owned = dev_alloc(sizeof(uint32_t) * 32 * S, s), in_all = dev_alloc(sizeof(uint32_t) * 32 * S * g_dist.world, s);
    Buf cnt = dev_alloc(sizeof(int64_t), s);
    capsmi_count_shard* h = nullptr;
    check(capsmi_count_shard_begin(s, nt, views, "s", "t", a, b, c, own_lo, own_hi, P<uint32_t>(owned), &h));
    std::unique_ptr<capsmi_count_shard, capsmi_status (*)(capsmi_count_shard*)> hold(h, capsmi_count_shard_release);
    collective(s, CAPSMI_COLL_ALL_GATHER, P<uint32_t>(owned), P<uint32_t>(in_all), 32 * S, CAPSMI_COLL_U32);
    check(capsmi_count_shard_finish(h, P<uint32_t>(in_all), P<int64_t>(cnt)));
    collective(s, CAPSMI_COLL_ALL_REDUCE_SUM, P<int64_t>(cnt), P<int64_t>(cnt), 1, CAPSMI_I64);
    return read_scalar(s, P<int64_t>(cnt));
}

namespace {

// a copy of bitmap b restricted to this rank's owned ids (whole word slices [rank * S, (rank + 1) * S))
std::unique_ptr<capsmi_bitmap> owned_mask(capsmi_session* s, const capsmi_bitmap* b) {
    const int64_t S = g_dist.slice_words, r = g_dist.rank;
    REQUIRE(b->nwords == S * g_dist.world, CAPSMI_ERR_INTERNAL, "distributed bitmap geometry");
    auto m = std::make_unique<capsmi_bitmap>();
    m->sess = s;
    m->lo = b->lo;
    m->hi = b->hi;
    m->nwords = b->nwords;
    m->words = dev_alloc(sizeof(uint32_t) * (size_t)b->nwords, s);
    m->any_dup = b->any_dup;
    HIP_CHECK(hipMemsetAsync(P<void>(m->words), 0, sizeof(uint32_t) * (size_t)b->nwords, s->stream));
    HIP_CHECK(hipMemcpyAsync(P<uint32_t>(m->words) + r * S, P<uint32_t>(b->words) + r * S, sizeof(uint32_t) * S,
                             hipMemcpyDeviceToDevice, s->stream));
    return m;
}

}  // namespace

// count(*) over distributed shards without moving any per-id array.  A rank's shard and
// its complement (BY_SOURCE: the relationships from other ranks' sources into owned ids; BY_TARGET: those from
// owned sources into other ranks' ids; exchanged once at capsmi_graph_distribute) hold every relationship
// incident to an owned id exactly once, so for an owned middle b both inA(b) and outC(b) are complete here:
// count(*) = sum over the ranks of sum_{owned b} b_ok(b) inA(b) outC(b) - loops(b), one record-partition
// count over the union with b restricted to owned ids and one 8-byte all-reduce -- per-rank bytes received
// fall with N (the earlier BY_TARGET form all-gathered 4 B x every id's in-degree, 256 MiB at 2^26 ids).
// The walk's orientation picks which complement column is the source.
int64_t dist_two_hop_count_owned(capsmi_session* s, const Path& P, const RelViews& v0, const capsmi_bitmap* a,
                               const capsmi_bitmap* b, const capsmi_bitmap* c) {
    REQUIRE(!a->any_dup && !b->any_dup && !c->any_dup, CAPSMI_ERR_UNSUPPORTED,
            "closed-form count(*) needs each node id in one scanned row");
    const Hop& h = P.hops[0];
    const bool fwd = h.from_role == ROLE_SRC;
    RelCols rc(v0.t);  // + the complement
    for (const Member& m : P.inst[h.rel].m) {
        if (m.base->in_rows <= 0) continue;
        rc.srcs.push_back(fwd ? m.base->in_src.d() : m.base->in_dst.d());
        rc.dsts.push_back(fwd ? m.base->in_dst.d() : m.base->in_src.d());
        rc.ms.push_back(m.base->in_rows);
    }
    std::unique_ptr<capsmi_bitmap> bown = owned_mask(s, b);
    const int64_t x = two_hop_count_rec(s, rc.srcs.data(), rc.dsts.data(), rc.ms.data(), (int)rc.ms.size(), a, bown.get(), c);
    return sum_over_ranks(s, x);
}

// the cyclic triangle count over a distributed graph (any relationship mode): the distributed trigraph
// build (k_tri.hip tri_build: pairs exchanged to their lower end's owner, oriented ranges exchanged and
// all-gathered), this rank's work share of the centers, one all-reduce of the parts
int64_t dist_triangle_count(capsmi_session* s, const std::vector<capsmi_table*>& views, const capsmi_bitmap* n_ok) {
    const RelCols rc(views);
    TriDist dd;
    dd.rank = g_dist.rank;
    dd.world = g_dist.world;
    dd.span = 32 * g_dist.slice_words;
    TriGraph g;
    tri_build(s, rc.srcs.data(), rc.dsts.data(), rc.ms.data(), (int)rc.ms.size(), n_ok, g, &dd);
    const uint64_t part = tri_count(s, g, g_dist.rank, g_dist.world);
    return sum_over_ranks(s, (int64_t)part);
}

// The undirected 1- / 2-hop routes over BY_SOURCE shards.  A rank's relationships (sources owned) hold each
// relationship once over the ranks; with its in-relationships (targets owned, exchanged at registration)
// they are every relationship incident to an owned id.
//   1 hop: the arcs of the rank's own relationships: count(*) summed, distinct ends ORed over the ranks;
//   2 hops: the middle b restricted to owned ids, over every relationship incident to them, so inU(b),
//   outU(b), K(b) and x(b) are complete: count(*) summed, the distinct ends ORed (or_reduce_count).
void dist_undirected(capsmi_session* s, const Scan& R, const std::vector<const int64_t*>& srcs,
                     const std::vector<const int64_t*>& dsts, const std::vector<int64_t>& ms, int h,
                     const std::vector<capsmi_bitmap*>& pos, const std::vector<int>& kinds, std::vector<int64_t>& vals) {
    std::vector<const int64_t*> as = srcs, ad = dsts;  // + the in-relationships
    std::vector<int64_t> am = ms;
    for (const Member& m : R.m) {
        if (m.base->in_rows <= 0) continue;
        as.push_back(m.base->in_src.d());
        ad.push_back(m.base->in_dst.d());
        am.push_back(m.base->in_rows);
    }
    std::unique_ptr<capsmi_bitmap> bown;
    if (h == 2) bown = owned_mask(s, pos[1]);
    Buf marks = dev_alloc(sizeof(uint32_t) * (size_t)pos[0]->nwords, s);
    for (int k : kinds) {
        const int kind = k == A_COUNT ? 0 : (k == A_DISTINCT_END ? 1 : 2);
        int64_t x;
        if (h == 1) {
            x = undirected_count(s, srcs.data(), dsts.data(), ms.data(), (int)srcs.size(), 1, pos[0], pos[1], pos[1], kind,
                                 kind ? P<uint32_t>(marks) : nullptr);
        } else {
            x = undirected_count(s, as.data(), ad.data(), am.data(), (int)as.size(), 2, pos[0], bown.get(), pos[2], kind,
                                 kind ? P<uint32_t>(marks) : nullptr);
        }
        vals.push_back(kind ? or_reduce_count(s, P<uint32_t>(marks)) : sum_over_ranks(s, x));
    }
}

// The var-length grouped count over BY_SOURCE shards: this rank owns the
// start ids [rank * span, (rank + 1) * span) and holds their out-relationships (`views`) plus the
// relationships into its owned ids from other ranks (the bases' in-shards, exchanged at registration).
// begin (owned od, reverse multiplicities) -> all-reduce od -> mid (owned Y) -> all-reduce Y -> finish:
// the (relative dense id, count) rows of the owned start nodes.
void dist_var_length(capsmi_session* s, const std::vector<capsmi_table*>& views,
                     const std::vector<const capsmi_table*>& bases, const capsmi_bitmap* a, const capsmi_bitmap* b,
                     int lower, int upper, const std::string& id_name, const std::string& count_name,
                     capsmi_table** out) {
    const RelCols rc(views);
    std::vector<const int64_t*> isrcs, idsts;
    std::vector<int64_t> ims;
    for (const capsmi_table* t : bases) {
        if (t->in_rows <= 0) continue;
        isrcs.push_back(t->in_src.d());
        idsts.push_back(t->in_dst.d());
        ims.push_back(t->in_rows);
    }
    const int64_t n = b->hi - b->lo, span = 32 * g_dist.slice_words;
    const int64_t own_lo = std::min<int64_t>(g_dist.rank * span, n), own_hi = std::min<int64_t>(own_lo + span, n);
    Buf od = dev_alloc(sizeof(int64_t) * n, s), y = dev_alloc(sizeof(int64_t) * n, s);
    VarlenShard* v = varlen_shard_begin(s, rc.srcs.data(), rc.dsts.data(), rc.ms.data(), (int)rc.ms.size(), isrcs.data(),
                                        idsts.data(), ims.data(), (int)isrcs.size(), a, b, lower, upper, own_lo + b->lo,
                                        own_hi + b->lo, P<int64_t>(od));
    std::unique_ptr<VarlenShard, void (*)(VarlenShard*)> hold(v, varlen_shard_free);
    collective(s, CAPSMI_COLL_ALL_REDUCE_SUM, P<int64_t>(od), P<int64_t>(od), n, CAPSMI_I64);
    varlen_shard_mid(v, P<int64_t>(y));
    collective(s, CAPSMI_COLL_ALL_REDUCE_SUM, P<int64_t>(y), P<int64_t>(y), n, CAPSMI_I64);
    Buf ids, cnt;
    const int64_t rows = varlen_shard_finish(v, ids, cnt);
    auto* r = result_table(s, rows);
    Column ic, cc;
    ic.name = id_name;
    ic.type = CAPSMI_I64;
    ic.data = ids;
    cc.name = count_name;
    cc.type = CAPSMI_I64;
    cc.data = cnt;
    r->cols.push_back(std::move(ic));
    r->cols.push_back(std::move(cc));
    *out = r;
}

}  // namespace planning
}  // namespace capsmi
