// plan_routes.hip -- the fused routes: the pattern shapes (plan_match.hip) that one kernel family answers, each with the
// name capsmi_session_route_count counts it under.  try_fused_shapes tries them in the order of this table:
//   count(*) / count(DISTINCT end | start), no key, one branch (fused_counts):
//     Expand + node filters ........................................ "expand_count"
//     2 x Expand + uniqueness ...................................... "two_hop"
//     2 x Expand + ExpandInto closing a directed cycle, count(*) ... "triangle"
//     the same with mixed directions ............................... "triangle_transitive"
//   2 x Expand grouped by the start, count(*) / count(DISTINCT end)  "two_hop_grouped"
//   the closed triangle grouped by the id of a, b or c, count(*) ... "triangle_grouped"
//   the same with mixed directions: the counts of the key's role ... "triangle_transitive_grouped"
//   2 x undirected Expand + undirected ExpandInto, count(*) ........ "triangle_undirected"
//   the same grouped by the id of a, b or c ........................ "triangle_undirected_grouped"
//   var-length, lower 0 or 1: count / collect(DISTINCT end), grouped
//     by the start or alone (alone: two branches or more) .......... "var_length_distinct"
//   1 or 2 undirected Expands, no key, count(*) / count(DISTINCT) .. "undirected"
//   var-length 0 <= l <= u <= 4 grouped by the start, count(*) ..... "var_length"
//   without a grouping: Expand + node filters, projected ........... "expand"
// A plan in a pattern shape that none of them took is counted once per materialisation as "miss" (try_fused,
// materialize in plan.hip).  Node predicates become node-scan bitmaps; ids must be unique per scan and inside one
// window of at most 2^30 ids (or a compacted graph's dense ids, id_window), else the plan runs unfused.
#include "plan_impl.h"

namespace capsmi {
namespace planning {

namespace {

void route(capsmi_session* s, const char* name) { s->routes[name] += 1; }

bool any_no_loops(const Path& P) {  // an undirected branch: only fused_undirected takes it
    for (const Scan& sc : P.inst) if (sc.no_loops) return true;
    return false;
}

int bits_for_ids(int64_t n) {  // bits of the largest relative id (k_tri.hip bits_for)
    int b = 1;
    while (b < 63 && (int64_t(1) << b) < n) ++b;
    return b;
}

Column i64_column(capsmi_session* s, const std::vector<int64_t>& v) {
    Column c;
    c.type = CAPSMI_I64;
    c.data = dev_alloc(sizeof(int64_t) * (v.empty() ? 1 : v.size()), s);
    c.host = std::make_shared<const std::vector<int64_t>>(v);
    if (v.size() == 1) {  // one word: a fill kernel, so neither a copy nor a host sync
        fill_i64(P<int64_t>(c.data), v[0], 1, s->stream);
    } else if (!v.empty()) {
        HIP_CHECK(hipMemcpyAsync(P<void>(c.data), v.data(), sizeof(int64_t) * v.size(), hipMemcpyHostToDevice, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    }
    return c;
}

// the one row of a global aggregation: one Long column per aggregate, under its output name
capsmi_table* count_row(capsmi_session* s, const std::vector<AggSpec>& aggs, const std::vector<int64_t>& vals) {
    auto* r = result_table(s, 1);
    for (size_t i = 0; i < vals.size(); ++i) {
        Column c = i64_column(s, {vals[i]});
        c.name = aggs[i].output;
        r->cols.push_back(std::move(c));
    }
    return r;
}

// the position of P that the group's one key denotes, when the key is a non-null id or endpoint column; else -1
int key_position(const capsmi_table* in, const PlanNode& g, const Path& P) {
    const int gc = find_col(in, g.a[0]);
    if (gc < 0 || !id_like(P, P.cols[gc])) return -1;
    return position_of(P, P.cols[gc]);
}

// A branch of an undirected pattern whose first `nexpands` hops are its Expands: each is incoming exactly when its
// relationship scan is the start <> end instance (RelationalPlanner.scala:130-131).  Returns the orientation, bit i
// set for an incoming hop i, or -1 when a hop breaks the rule; the caller sees that every orientation occurs once.
int undirected_orientation(const Path& P, int nexpands) {
    int o = 0;
    for (int i = 0; i < nexpands; ++i) {
        const bool incoming = P.hops[i].from_role == ROLE_DST;
        if (P.inst[P.hops[i].rel].no_loops != incoming) return -1;
        o |= (incoming ? 1 : 0) << i;
    }
    return o;
}

// count(*) / count(DISTINCT end | start) of one branch: 1 hop, a 2-hop chain, or the closed triangle.
// Returns false when the shape or a precondition does not hold.
bool fused_counts(capsmi_session* s, const Path& P, const std::vector<int>& kinds, std::vector<int64_t>& vals) {
    Classified c;
    if (any_no_loops(P) || !classify(P, c)) return false;
    for (int x : P.pos_node) if (x < 0) return false;
    const size_t nh = P.hops.size();
    if (nh < 1 || nh > 3) return false;
    std::vector<Path> one{P};
    int64_t lo, hi;
    if (!id_window(one, &lo, &hi)) return false;
    BitmapSet bs;
    RelViews v0;
    rel_views(P, P.hops[0], v0);
    const int64_t nt = (int64_t)v0.t.size();
    if (nh == 1 && is_chain(P) && c.uniq.empty()) {
        for (int k : kinds) if (k != A_COUNT) return false;
        capsmi_bitmap* a = node_bitmap(s, P, c, P.pos_node[0], lo, hi, bs);
        capsmi_bitmap* b = node_bitmap(s, P, c, P.pos_node[1], lo, hi, bs);
        if (!a || !b) return false;
        int64_t total = 0;
        for (capsmi_table* t : v0.t) {
            const char* sc[1] = {"s"};
            capsmi_table* o = nullptr;
            check(capsmi_expand_filter(s, t, "s", "t", a, b, 1, sc, nullptr, &o));
            total += o->nrows;
            capsmi_table_release(o);
        }
        if (g_dist.on) total = sum_over_ranks(s, total);  // each rank counted its own relationships
        vals.assign(kinds.size(), total);
        route(s, "expand_count");
        return true;
    }
    if (nh == 2 && is_chain(P) && same_orientation(P)) {
        RelViews v1;
        rel_views(P, P.hops[1], v1);
        if (v1.sig != v0.sig || !all_pairs_unique(c, 2)) return false;
        if (g_dist.on)  // the distributed count(*) folds in-degrees of at most 2^26 ids (k_count.hip)
            for (int k : kinds)
                if (k == A_COUNT && hi - lo > (int64_t(1) << 26)) return false;
        capsmi_bitmap* a = node_bitmap(s, P, c, P.pos_node[0], lo, hi, bs);
        capsmi_bitmap* b = node_bitmap(s, P, c, P.pos_node[1], lo, hi, bs);
        capsmi_bitmap* cc = node_bitmap(s, P, c, P.pos_node[2], lo, hi, bs);
        if (!a || !b || !cc) return false;
        // Cache analogue: relationship tables marked cache() keep the partitioned layout of the walk
        const Scan& R = P.inst[P.hops[0].rel];
        bool keep = !R.m.empty();
        for (const Member& m : R.m) keep = keep && m.base->keep_layouts;
        // the reversed relationships (distinct start = distinct end of the reversed walk)
        RelViews rv;
        reversed_views(v0, rv);
        const bool by_tgt = g_dist.rel_mode == CAPSMI_RELS_BY_TARGET;
        for (int k : kinds) {
            int64_t x = 0;
            const bool rev = k == A_DISTINCT_START;
            capsmi_table* const* vw = rev ? rv.t.data() : v0.t.data();
            const capsmi_bitmap* A = rev ? cc : a;
            const capsmi_bitmap* C = rev ? a : cc;
            const capsmi_relpart* lay = nullptr;
            if (keep && k != A_COUNT) {
                const std::string key = v0.sig + (rev ? "<" : ">") + std::to_string(lo) + ":" + std::to_string(hi);
                auto& cache = R.m[0].base->layouts;
                auto it = cache.find(key);
                if (it == cache.end()) {
                    capsmi_relpart* rp = nullptr;
                    check(capsmi_relpart_build(s, (int32_t)nt, vw, "s", "t", lo, hi, &rp));
                    it = cache.emplace(key, std::shared_ptr<capsmi_relpart>(rp, [](capsmi_relpart* q) {
                                           capsmi_relpart_release(q);
                                       })).first;
                }
                lay = it->second.get();
            }
            if (g_dist.on && k == A_COUNT) {
                // the shard and its complement around the owned middles, no per-id exchange (dense ids: the
                // complement's); without dense ids the all-gather form (BY_TARGET forwards, BY_SOURCE reversed)
                x = g_dense ? dist_two_hop_count_owned(s, P, v0, a, b, cc)
                    : by_tgt ? dist_two_hop_count(s, (int32_t)nt, v0.t.data(), a, b, cc)
                             : dist_two_hop_count(s, (int32_t)nt, rv.t.data(), cc, b, a);
            } else if (g_dist.on) {
                // the walk's relationships arrive by their end's owner (BY_TARGET forwards, BY_SOURCE reversed):
                // the all-gather form; by their start's owner: the OR-reduce form
                const bool end_owned = by_tgt != rev;
                x = end_owned ? dist_two_hop_distinct(s, lay, lay ? 0 : (int32_t)nt, lay ? nullptr : vw, A, b, C)
                              : dist_two_hop_distinct_src(s, lay, lay ? 0 : (int32_t)nt, lay ? nullptr : vw, A, b, C);
            } else if (k == A_COUNT) {
                check(capsmi_two_hop_count(s, (int32_t)nt, v0.t.data(), "s", "t", a, b, cc, &x));
            } else if (lay) {
                check(capsmi_two_hop_count_distinct_part(s, lay, A, b, C, &x));
            } else {
                check(capsmi_two_hop_count_distinct(s, (int32_t)nt, vw, "s", "t", A, b, C, &x));
            }
            vals.push_back(x);
        }
        route(s, "two_hop");
        return true;
    }
    int tri_role[3];
    if (const int shape = closed_triangle(P, tri_role)) {
        // P0 - P1 - P2 - P0 (the closing hop is the ExpandInto), every hop read along its relationships
        if (!all_pairs_unique(c, 3)) return false;
        for (int k : kinds) if (k != A_COUNT) return false;
        RelViews d0;
        capsmi_bitmap* a = one_set_one_filter(s, &P, &c, 1, lo, hi, bs, d0);
        if (!a) return false;
        // the distributed build codes oriented targets in 24 bits: larger domains take the generic plan
        if (g_dist.on && (bits_for_ids(hi - lo) + 7) / 8 * 8 > 24) return false;
        int64_t x = 0;
        if (shape == TRI_TRANSITIVE) {
            if (g_dist.on) return false;  // single device
            check(capsmi_triangle_count_transitive(s, (int32_t)nt, d0.t.data(), "s", "t", a, &x));
            vals.assign(kinds.size(), x);
            route(s, "triangle_transitive");
            return true;
        }
        if (g_dist.on) x = dist_triangle_count(s, d0.t, a);
        else check(capsmi_triangle_count(s, (int32_t)nt, d0.t.data(), "s", "t", a, &x));
        vals.assign(kinds.size(), x);
        route(s, "triangle");
        return true;
    }
    return false;
}

// Undirected Expand chains of 1 or 2 hops (RelationalPlanner.scala:126-136): 2^hops branches, one per
// orientation of the hops, the incoming hops over relationships with start <> end, the same node scans at
// every position, pairwise uniqueness of the relationships; count(*) / count(DISTINCT end | start).
bool fused_undirected(capsmi_session* s, const capsmi_table* in, const PlanNode& g, const std::vector<Path>& B,
                      std::vector<int64_t>& vals) {
    const size_t h = B[0].hops.size();
    if (h < 1 || h > 2 || B.size() != (size_t(1) << h)) return false;
    std::set<int> orients;
    std::vector<Classified> cls(B.size());
    std::vector<int> kinds;
    for (size_t bi = 0; bi < B.size(); ++bi) {
        const Path& P = B[bi];
        if (P.hops.size() != h || !is_chain(P)) return false;
        for (int x : P.pos_node) if (x < 0) return false;
        const int o = undirected_orientation(P, (int)h);
        if (o < 0) return false;
        orients.insert(o);
        if (!classify(P, cls[bi])) return false;
        if (h == 2 ? !all_pairs_unique(cls[bi], 2) : !cls[bi].uniq.empty()) return false;
        std::vector<int> k;
        if (!agg_kinds(in, g, P, 0, (int)h, k)) return false;
        if (bi == 0) kinds = k;
        else if (k != kinds) return false;
    }
    if (orients.size() != B.size()) return false;
    int64_t lo, hi;
    if (!id_window(B, &lo, &hi)) return false;
    // distributed: BY_SOURCE shards, whose in-relationships complete every owned id's incident set
    if (g_dist.on && g_dist.rel_mode != CAPSMI_RELS_BY_SOURCE) return false;
    // one relationship set for every hop of every branch, read as (start, end)
    auto plain_views = [&](const Path& P, const Hop& hp, RelViews& v) {
        Hop fwd = hp;
        fwd.from_role = ROLE_SRC;
        fwd.to_role = ROLE_DST;
        rel_views(P, fwd, v);
    };
    RelViews v0;
    plain_views(B[0], B[0].hops[0], v0);
    for (const Path& P : B)
        for (const Hop& hp : P.hops) {
            RelViews v;
            plain_views(P, hp, v);
            if (v.sig != v0.sig) return false;
        }
    // one node scan per position, identical in every branch
    BitmapSet bs;
    std::vector<capsmi_bitmap*> pos(h + 1, nullptr);
    for (size_t q = 0; q <= h; ++q) {
        std::string k0;
        pos[q] = node_bitmap(s, B[0], cls[0], B[0].pos_node[q], lo, hi, bs, &k0);
        if (!pos[q]) return false;
        for (size_t bi = 1; bi < B.size(); ++bi) {
            std::string kq;
            if (!node_bitmap(s, B[bi], cls[bi], B[bi].pos_node[q], lo, hi, bs, &kq) || kq != k0) return false;
        }
    }
    const RelCols rc(v0.t);
    if (g_dist.on) {
        dist_undirected(s, B[0].inst[B[0].hops[0].rel], rc.srcs, rc.dsts, rc.ms, (int)h, pos, kinds, vals);
        route(s, "undirected");
        return true;
    }
    for (int k : kinds) {
        const int kind = k == A_COUNT ? 0 : (k == A_DISTINCT_END ? 1 : 2);
        vals.push_back(undirected_count(s, rc.srcs.data(), rc.dsts.data(), rc.ms.data(), (int)rc.ms.size(), (int)h, pos[0],
                                        pos[1], h == 2 ? pos[2] : pos[1], kind));
    }
    route(s, "undirected");
    return true;
}

// n ids of the route's dense domain (g_dense) as the graph's Long ids: in[0, n) into out.  The scrambled form (a
// distributed graph) is undone in place, so there out may be in; the compacted form gathers, so there it may not.
void dense_to_long(capsmi_session* s, const int64_t* in, int64_t n, int64_t* out) {
    if (g_dense->scrambled) {
        if (n && in != out) HIP_CHECK(hipMemcpyAsync(out, in, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, s->stream));
        unscramble_ids(s, *g_dense, out, n);
    } else {
        gather_col(P<int64_t>(g_dense->orig), nullptr, in, n, out, nullptr, s->stream);
    }
}

// the start ids of a route's rows back to the graph's Long ids, in place (relative ids in [0, n) of the route's
// window: without a dense domain the window's lo is added)
void ids_to_long(capsmi_session* s, int64_t lo, int64_t* v, int64_t n) {
    if (n <= 0) return;
    if (!g_dense) {
        add_i64(v, lo, n, s->stream);
    } else if (g_dense->scrambled) {
        dense_to_long(s, v, n, v);
    } else {
        Buf ids = dev_alloc(sizeof(int64_t) * n, s);
        dense_to_long(s, v, n, P<int64_t>(ids));
        HIP_CHECK(hipMemcpyAsync(v, P<void>(ids), sizeof(int64_t) * n, hipMemcpyDeviceToDevice, s->stream));
    }
}

// The same for the start-id column (column 0) of a var-length entry point's rows.  Those ids are absolute already,
// so only a dense domain is undone; the ids land in a block of their own, and what described the old one (row
// offset, host copy, 32-bit copy) goes.
void start_ids_to_long(capsmi_session* s, capsmi_table* r) {
    if (!g_dense) return;
    Column& c = r->cols[0];
    Buf ids = dev_alloc(sizeof(int64_t) * (r->nrows > 0 ? r->nrows : 1), s);
    dense_to_long(s, c.d(), r->nrows, P<int64_t>(ids));
    c.data = ids;
    c.offset = 0;
    c.host.reset();
    c.narrow.reset();
}

// C3's grouped form: the 2-hop chain grouped by its start node, count(*) / count(DISTINCT end)
bool fused_grouped_two_hop(capsmi_session* s, const capsmi_table* in, const PlanNode& g, const std::vector<Path>& B,
                           capsmi_table** out) {
    if (B.size() != 1 || g.a.size() != 1 || g.aggs.empty()) return false;
    const Path& P = B[0];
    if (any_no_loops(P) || P.hops.size() != 2 || !is_chain(P) || !same_orientation(P)) return false;
    for (int x : P.pos_node) if (x < 0) return false;
    if (key_position(in, g, P) != 0) return false;
    std::vector<int> kinds;
    if (!agg_kinds(in, g, P, 0, 2, kinds)) return false;
    for (int k : kinds) if (k == A_DISTINCT_START) return false;
    Classified c;
    if (!classify(P, c) || !all_pairs_unique(c, 2)) return false;
    RelViews v0, v1;
    rel_views(P, P.hops[0], v0);
    rel_views(P, P.hops[1], v1);
    if (v0.sig != v1.sig) return false;
    std::vector<Path> one{P};
    int64_t lo, hi;
    if (!id_window(one, &lo, &hi)) return false;
    if (g_dist.on && g_dist.rel_mode != CAPSMI_RELS_BY_SOURCE) return false;  // the rows of owned starts
    BitmapSet bs;
    capsmi_bitmap* a = node_bitmap(s, P, c, P.pos_node[0], lo, hi, bs);
    capsmi_bitmap* b = node_bitmap(s, P, c, P.pos_node[1], lo, hi, bs);
    capsmi_bitmap* cc = node_bitmap(s, P, c, P.pos_node[2], lo, hi, bs);
    if (!a || !b || !cc) return false;
    const RelCols rc(v0.t);
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    auto* r = result_table(s, 0);
    std::unique_ptr<capsmi_table> guard(r);
    int64_t rows = -1;
    for (size_t i = 0; i < kinds.size(); ++i) {
        Buf ids, vals;
        int64_t nrow = 0;
        GroupedDist gd;
        gd.rank = g_dist.rank;
        gd.world = g_dist.world;
        gd.span = 32 * g_dist.slice_words;
        if (!grouped_two_hop(s, rc.srcs.data(), rc.dsts.data(), rc.ms.data(), (int)rc.ms.size(), a, b, cc, kinds[i] != A_COUNT,
                             (int64_t)(free_b / 2), ids, vals, &nrow, g_dist.on ? &gd : nullptr))
            return false;  // the keys would not fit: the generic plan (and its size guard) decides
        REQUIRE(rows < 0 || rows == nrow, CAPSMI_ERR_INTERNAL, "grouped 2-hop: aggregates disagree on the groups");
        if (i == 0) {
            rows = nrow;
            ids_to_long(s, lo, ::capsmi::P<int64_t>(ids), nrow);
            Column k;
            k.type = CAPSMI_I64;
            k.data = ids;
            r->cols.push_back(std::move(k));
        }
        Column v;
        v.type = CAPSMI_I64;
        v.data = vals;
        r->cols.push_back(std::move(v));
    }
    r->nrows = rows;
    r->partitioned = g_dist.on && g_dist.world > 1;  // the rows of this rank's owned start nodes
    *out = guard.release();
    route(s, "two_hop_grouped");
    return true;
}

// The grouped triangle routes' tail: the trigraph of the views, its per-node rows (relative ids back to the graph's
// Long ids) and the result table: the key and one count column per aggregate (every aggregate is the same count).
capsmi_table* tri_grouped_rows(capsmi_session* s, const RelViews& v, const capsmi_bitmap* n_ok, TriShape shape, int cls,
                               int64_t lo, size_t naggs) {
    const RelCols rc(v.t);
    Buf ids, cnt;
    int64_t rows = 0;
    {
        TriGraph tg;
        tri_build(s, rc.srcs.data(), rc.dsts.data(), rc.ms.data(), (int)rc.ms.size(), n_ok, tg);
        rows = tri_shape_count_by_node(s, tg, shape, cls, ids, cnt);
    }
    ids_to_long(s, lo, ::capsmi::P<int64_t>(ids), rows);
    std::unique_ptr<capsmi_table> r(result_table(s, rows));
    Column k;
    k.type = CAPSMI_I64;
    k.data = ids;
    r->cols.push_back(k);
    k.data = cnt;
    r->cols.insert(r->cols.end(), naggs, k);
    return r.release();
}

// C4's grouped form: the closed triangle grouped by one of its nodes, count(*).  The preconditions of the
// triangle in fused_counts (three hops closing on position 0, one relationship set, pairwise-unique
// relationships, one node filter for all three positions) make the pattern symmetric under rotation, so the
// counts grouped by position 1 or 2 are the counts grouped by position 0 (k_tri_nodes.hip).  Single device.
// The same closed path with mixed directions is the transitive triangle (closed_triangle): the key's position
// has a role -- source, middle or sink -- and the rows are that role's counts (k_tri_nodes.hip,
// "triangle_transitive_grouped").
bool fused_grouped_triangle(capsmi_session* s, const capsmi_table* in, const PlanNode& g, const std::vector<Path>& B,
                            capsmi_table** out) {
    if (B.size() != 1 || g.a.size() != 1 || g.aggs.empty()) return false;
    const Path& P = B[0];
    Classified c;
    if (any_no_loops(P) || !classify(P, c)) return false;
    for (int x : P.pos_node) if (x < 0) return false;
    int role[3];
    const int shape = closed_triangle(P, role);
    if (shape == TRI_NONE) return false;
    const int gp = key_position(in, g, P);
    if (gp < 0 || gp > 2) return false;
    std::vector<int> kinds;
    if (!agg_kinds(in, g, P, 0, 0, kinds)) return false;
    for (int k : kinds) if (k != A_COUNT) return false;
    std::vector<Path> one{P};
    int64_t lo, hi;
    if (!id_window(one, &lo, &hi) || g_dist.on) return false;  // (sets the id domain the views below read)
    if (!all_pairs_unique(c, 3)) return false;
    BitmapSet bs;
    RelViews v0;
    capsmi_bitmap* a = one_set_one_filter(s, &P, &c, 1, lo, hi, bs, v0);
    if (!a) return false;
    if (shape == TRI_CYCLE) {
        *out = tri_grouped_rows(s, v0, a, TriShape::cycle, 0, lo, kinds.size());
        route(s, "triangle_grouped");
    } else {
        *out = tri_grouped_rows(s, v0, a, TriShape::transitive, role[gp], lo, kinds.size());
        route(s, "triangle_transitive_grouped");
    }
    return true;
}

// The undirected triangle (a)-[r1]-(b)-[r2]-(c)-[r3]-(a) (RelationalPlanner.scala:126-136 and :150-153): eight
// branches, one per orientation of the three hops.  Every branch is the closed path of closed_triangle; hops 0 and
// 1 (the Expands) are incoming exactly when their relationship scan is the start <> end instance, the closing
// ExpandInto's scan never is (it binds a self-loop in both of its joins); one relationship set read as (start,
// end) by every hop of every branch, pairwise-unique relationships, one node filter for all positions and
// branches, count(*) aggregates only.  Without keys: the count ("triangle_undirected"); with one key, the id of
// the same position p in every branch: the rows of p's class -- the ends of the ExpandInto (p = 0, 2) or the
// middle (p = 1) -- ("triangle_undirected_grouped", k_tri_nodes.hip).  Single device.
bool fused_undirected_triangle(capsmi_session* s, const capsmi_table* in, const PlanNode& g, const std::vector<Path>& B,
                               capsmi_table** out) {
    if (B.size() != 8 || g.a.size() > 1 || g.aggs.empty()) return false;
    std::set<int> orients;
    std::vector<Classified> cls(B.size());
    std::vector<int> kinds;
    int gp = -1;
    for (size_t bi = 0; bi < B.size(); ++bi) {
        const Path& P = B[bi];
        int role[3];
        if (closed_triangle(P, role) == TRI_NONE) return false;
        for (int x : P.pos_node) if (x < 0) return false;
        const int o = undirected_orientation(P, 2);
        if (o < 0 || P.inst[P.hops[2].rel].no_loops) return false;
        orients.insert(o | (P.hops[2].from == 0 ? 1 : 0) << 2);
        if (!classify(P, cls[bi]) || !all_pairs_unique(cls[bi], 3)) return false;
        std::vector<int> k;
        if (!agg_kinds(in, g, P, 0, 0, k)) return false;
        for (int x : k) if (x != A_COUNT) return false;
        if (bi == 0) kinds = k;
        if (!g.a.empty()) {
            const int p = key_position(in, g, P);
            if (p < 0 || p > 2 || (bi > 0 && p != gp)) return false;
            gp = p;
        }
    }
    if (orients.size() != B.size()) return false;
    int64_t lo, hi;
    if (!id_window(B, &lo, &hi) || g_dist.on) return false;
    // one relationship set for every hop of every branch, read as (start, end), and one node filter for all three
    // positions of every branch
    BitmapSet bs;
    RelViews v0;
    capsmi_bitmap* a = one_set_one_filter(s, B.data(), cls.data(), B.size(), lo, hi, bs, v0);
    if (!a) return false;
    const int nt = (int)v0.t.size();
    if (nt <= 0) return false;
    if (g.a.empty()) {
        int64_t x = 0;
        check(capsmi_triangle_count_undirected(s, (int32_t)nt, v0.t.data(), "s", "t", a, &x));
        *out = count_row(s, g.aggs, std::vector<int64_t>(kinds.size(), x));
        route(s, "triangle_undirected");
        return true;
    }
    *out = tri_grouped_rows(s, v0, a, TriShape::undirected, gp == 1 ? CAPSMI_TRI_UND_MIDDLE : CAPSMI_TRI_UND_END, lo,
                            kinds.size());
    route(s, "triangle_undirected_grouped");
    return true;
}

// What the two var-length routes ask of the branches of a bounded var-length expand (VarLengthExpandPlanner.scala:
// 46-310), and what they get: one branch per length, each a chain of hops in one orientation over one relationship
// set with pairwise-unique relationships, node-scanned at its two ends only and with predicates only there; the
// zero-length branch (lower = 0) is copyEntity(source -> target) of the start scan (:146-153, :190-210), one row per
// scanned start node whatever the target's labels.  Every branch of a hop or more shares one start scan, which is
// the zero-length branch's, and one end scan.
struct VarLength {
    BitmapSet bs;
    capsmi_bitmap *a = nullptr, *b = nullptr;  // the start and the end scan (kept by bs)
    RelViews views;                            // the relationship set, read along the hops
    std::vector<const capsmi_table*> bases;    // the tables behind `views` (their in-shards)
    int l = 0, u = 0;                          // the lengths: every one of l .. u
};

// `branch_ok(P, k)`: the caller's own checks of a branch of k hops -- where its key and aggregated columns sit, what
// its session can walk.  It runs with the other pure checks, before the branch's node scans: those launch kernels
// (distributed: collectives too), so whatever can decline a plan without them comes first.  The window [lo, hi) is
// id_window(B)'s, called by the route so that its own launch-free checks of the domain precede the scans as well.
bool match_var_length(capsmi_session* s, const std::vector<Path>& B, int64_t lo, int64_t hi,
                      const std::function<bool(const Path&, int)>& branch_ok, VarLength& m) {
    std::set<int> lens;
    std::string akey, bkey, rsig;
    std::string zero_key;  // the zero-length branch's start scan
    bool first = true;
    for (const Path& P : B) {
        if (any_no_loops(P)) return false;
        const int k = (int)P.hops.size();
        if (lens.count(k) || P.pos_node.empty() || P.pos_node[0] < 0) return false;
        lens.insert(k);
        if (k > 0) {
            if (!is_chain(P) || !same_orientation(P) || P.pos_node[k] < 0) return false;
            for (int q = 1; q < k; ++q) if (P.pos_node[q] >= 0) return false;  // hops are not node-scanned
        }
        if (!branch_ok(P, k)) return false;
        Classified c;
        if (!classify(P, c) || !all_pairs_unique(c, k)) return false;
        for (size_t q = 0; q < P.inst.size(); ++q)
            if (!c.pred[q].empty() && (int)q != P.pos_node[0] && (int)q != P.pos_node[k]) return false;
        if (k == 0) {
            if (!node_bitmap(s, P, c, P.pos_node[0], lo, hi, m.bs, &zero_key)) return false;
            continue;
        }
        std::string ka, kb;
        capsmi_bitmap* a = node_bitmap(s, P, c, P.pos_node[0], lo, hi, m.bs, &ka);
        capsmi_bitmap* b = node_bitmap(s, P, c, P.pos_node[k], lo, hi, m.bs, &kb);
        if (!a || !b) return false;
        for (int h = 0; h < k; ++h) {
            RelViews v;
            rel_views(P, P.hops[h], v);
            if (first && h == 0) {
                rsig = v.sig;
                m.views.t.swap(v.t);
                for (const Member& mb : P.inst[P.hops[h].rel].m) m.bases.push_back(mb.base);
            } else if (v.sig != rsig) {
                return false;
            }
        }
        if (first) { akey = ka; bkey = kb; m.a = a; m.b = b; first = false; }
        else if (ka != akey || kb != bkey) return false;
    }
    if (first || (lens.count(0) && zero_key != akey)) return false;  // a path of >= 1 hop; one start scan
    m.l = *lens.begin();
    m.u = *lens.rbegin();
    return m.u - m.l + 1 == (int)lens.size();
}

// group by the start node, count(*), over the branches of a bounded var-length expand
bool fused_var_length(capsmi_session* s, const capsmi_table* in, const PlanNode& g, const std::vector<Path>& B,
                      capsmi_table** out) {
    if (g.a.size() != 1 || g.aggs.size() != 1) return false;
    const AggSpec& ag = g.aggs[0];
    int64_t lo, hi;
    if (!id_window(B, &lo, &hi)) return false;
    // the sharded count needs every owned source's out-relationships (BY_SOURCE shards); decided before any
    // node scan, whose gathers would otherwise run for nothing
    if (g_dist.on && g_dist.rel_mode != CAPSMI_RELS_BY_SOURCE) return false;
    VarLength m;
    const auto branch_ok = [&](const Path& P, int k) {
        if (key_position(in, g, P) != 0) return false;
        if (k == 0) return ag.kind == CAPSMI_AGG_COUNT_STAR;  // the zero-length branch: count(*) only
        if (ag.kind == CAPSMI_AGG_COUNT) {
            const int c = find_col(in, ag.input);
            if (ag.distinct || c < 0 || !id_like(P, P.cols[c])) return false;
        } else if (ag.kind != CAPSMI_AGG_COUNT_STAR) {
            return false;
        }
        for (const Hop& h : P.hops)
            if (g_dist.on && h.from_role != ROLE_SRC) return false;  // outgoing over BY_SOURCE shards
        return true;
    };
    if (!match_var_length(s, B, lo, hi, branch_ok, m)) return false;
    // upper 4 on one device (var_length4, ids below 2^24 - 1); the sharded form stops at 3
    if (m.u > (g_dist.on ? 3 : 4)) return false;
    if (m.u == 4 && hi - lo >= (int64_t(1) << 24) - 1) return false;
    if (g_dist.on) dist_var_length(s, m.views.t, m.bases, m.a, m.b, m.l, m.u, g.a[0], ag.output, out);
    else
        check(capsmi_var_length_count(s, (int32_t)m.views.t.size(), m.views.t.data(), "s", "t", m.a, m.b, m.l, m.u,
                                      g.a[0].c_str(), ag.output.c_str(), out));
    start_ids_to_long(s, *out);
    (*out)->partitioned = g_dist.on && g_dist.world > 1;  // the rows of this rank's owned start nodes
    route(s, "var_length");
    return true;
}

// count(DISTINCT end node) and / or collect(DISTINCT end node), at most one of each, over the branches of a bounded
// var-length expand, grouped by the start node (g.a = the start's id-like column) or alone (g.a empty): k-hop reach
// (k_reach.hip).  Lengths lower..upper contiguous with lower in {0, 1} and any upper.
bool fused_var_length_distinct(capsmi_session* s, const capsmi_table* in, const PlanNode& g, const std::vector<Path>& B,
                               capsmi_table** out) {
    if (g.a.size() > 1 || g.aggs.empty() || g.aggs.size() > 2 || g_dist.on) return false;  // single device: the operator path answers
    const bool grouped = !g.a.empty();
    const AggSpec *cag = nullptr, *lag = nullptr;  // the count, the collect
    std::vector<int> ics;
    for (const AggSpec& ag : g.aggs) {
        if (!ag.distinct) return false;
        if (ag.kind == CAPSMI_AGG_COUNT && !cag) cag = &ag;
        else if (ag.kind == CAPSMI_AGG_COLLECT && !lag) lag = &ag;
        else return false;
        ics.push_back(find_col(in, ag.input));
        if (ics.back() < 0) return false;
    }
    int64_t lo, hi;
    if (!id_window(B, &lo, &hi)) return false;
    // The lists ascend in the ids the walk runs on.  A compacted graph's dense ids are hash group numbers
    // (graph_compact: orig[] is not monotonic), so the extraction walks the domain in the order of the original ids
    // (DenseIds::order, built at the first collect and kept; k_reach.hip "Remapped ids") and stores those.  The
    // scrambled form of a distributed graph has no orig table: collect there stays on the operator path, which sorts
    // the original ids (distributed sessions were declined above).
    if (lag && g_dense && g_dense->scrambled) return false;
    std::shared_ptr<const IdOrder> ord;
    const int64_t* orig = nullptr;
    if (lag && g_dense) {
        if (hi - lo != g_dense->n) return false;
        std::lock_guard<std::mutex> lk(g_dense->order_mu);
        if (!g_dense->order) g_dense->order = id_order_build(s, P<int64_t>(g_dense->orig), g_dense->n);
        ord = g_dense->order;
        orig = P<int64_t>(g_dense->orig);
    }
    VarLength m;
    const auto branch_ok = [&](const Path& P, int k) {
        if (grouped && key_position(in, g, P) != 0) return false;
        for (int ic : ics)  // the end node's id; in the zero-length branch the copied start column
            if (position_of(P, P.cols[ic]) != k || !id_like(P, P.cols[ic])) return false;
        return true;
    };
    if (!match_var_length(s, B, lo, hi, branch_ok, m)) return false;
    if (m.l > 1) return false;  // lower >= 2: the join plan
    if (m.a->any_dup || m.b->any_dup) return false;
    const int32_t nt = (int32_t)m.views.t.size();
    capsmi_table* const* vt = m.views.t.data();
    if (!grouped && lag) {  // one row: the union's list, and its length as the count
        capsmi_table* lt = nullptr;
        var_length_reach_list_table(s, nt, vt, "s", "t", m.a, m.b, m.l, m.u, lag->output.c_str(), ord.get(), &lt);
        std::unique_ptr<capsmi_table, void (*)(capsmi_table*)> hold(lt, [](capsmi_table* t) { capsmi_table_release(t); });
        const Column& list = lt->cols[0];
        auto* r = cag ? count_row(s, {*cag}, {list.list->nvalues}) : result_table(s, 1);
        r->cols.insert(lag == &g.aggs[0] ? r->cols.begin() : r->cols.end(), list);
        *out = r;
    } else if (!grouped) {
        int64_t x = 0;
        check(capsmi_var_length_reach_count(s, nt, vt, "s", "t", m.a, m.b, m.l, m.u, &x));
        *out = count_row(s, {*cag}, {x});
    } else if (lag) {  // (id, list[, count]) in the order of the aggregates; on dense ids, original ids throughout
        var_length_collect_table(s, nt, vt, "s", "t", m.a, m.b, m.l, m.u, g.a[0].c_str(), lag->output.c_str(),
                                 cag ? cag->output.c_str() : nullptr, orig, ord.get(), out);
        if (cag && cag == &g.aggs[0]) std::swap((*out)->cols[1], (*out)->cols[2]);
    } else {
        check(capsmi_var_length_count_distinct(s, nt, vt, "s", "t", m.a, m.b, m.l, m.u, g.a[0].c_str(),
                                               cag->output.c_str(), out));
        start_ids_to_long(s, *out);
    }
    route(s, "var_length_distinct");
    return true;
}

// Expand + node filters projected on relationship / endpoint columns (C2)
bool fused_projection(capsmi_session* s, const capsmi_table* t, const std::vector<Path>& B, capsmi_table** out) {
    if (B.size() != 1) return false;
    const Path& P = B[0];
    if (P.hops.size() != 1 || !is_chain(P) || P.pos_node[0] < 0 || P.pos_node[1] < 0 || any_no_loops(P)) return false;
    Classified c;
    if (!classify(P, c) || !c.uniq.empty()) return false;
    const Hop& h = P.hops[0];
    const Scan& R = P.inst[h.rel];
    // output column -> (relationship scan column | endpoint role | constant)
    std::vector<int> rcol(P.cols.size(), -1), endp(P.cols.size(), ROLE_NONE);
    int ndata = 0;
    for (size_t i = 0; i < P.cols.size(); ++i) {
        const Role& r = P.cols[i];
        if (r.k == RK_CONST) continue;
        if (r.k == RK_REL && r.inst == h.rel) { rcol[i] = r.scol; ++ndata; continue; }
        const int pos = position_of(P, r);
        if (r.k == RK_NODE && pos == 0) { endp[i] = h.from_role; ++ndata; continue; }
        if (r.k == RK_NODE && pos == 1) { endp[i] = h.to_role; ++ndata; continue; }
        return false;  // node properties / labels: joined in the generic plan
    }
    if (ndata > 4) return false;
    std::vector<Path> one{P};
    int64_t lo, hi;
    if (!id_window(one, &lo, &hi)) return false;
    BitmapSet bs;
    capsmi_bitmap* a = node_bitmap(s, P, c, P.pos_node[0], lo, hi, bs);
    capsmi_bitmap* b = node_bitmap(s, P, c, P.pos_node[1], lo, hi, bs);
    if (!a || !b) return false;
    std::vector<capsmi_table*> parts;
    struct Release { std::vector<capsmi_table*>& v; ~Release() { for (auto* x : v) capsmi_table_release(x); } } rel{parts};
    for (const Member& m : R.m) {
        const EntityInfo& e = *m.base->entity;
        const int fc = h.from_role == ROLE_SRC ? e.src : e.dst, tc = h.to_role == ROLE_SRC ? e.src : e.dst;
        std::vector<const char*> ocols, onames;
        std::vector<std::string> tmpn;
        for (size_t i = 0; i < P.cols.size(); ++i) tmpn.push_back("c" + std::to_string(i));
        bool const_member = false;
        for (size_t i = 0; i < P.cols.size(); ++i) {
            int bc = -1;
            if (rcol[i] >= 0) bc = m.src[rcol[i]];
            else if (endp[i] != ROLE_NONE) bc = endp[i] == ROLE_SRC ? e.src : e.dst;
            else continue;
            if (bc < 0) { const_member = true; break; }  // a per-table constant in a relationship column
            ocols.push_back(m.base->cols[bc].name.c_str());
            onames.push_back(tmpn[i].c_str());
        }
        if (const_member) return false;
        const char* any[1] = {m.base->cols[fc].name.c_str()};
        const char* anyn[1] = {"c_"};
        capsmi_table* o = nullptr;
        // node tests on the (dense) endpoint columns, projections of the original columns
        capsmi_table* tab = g_dense ? dense_view(m.base) : m.base;
        const char* tf = g_dense ? (h.from_role == ROLE_SRC ? "__dense_src" : "__dense_dst") : m.base->cols[fc].name.c_str();
        const char* tt = g_dense ? (h.to_role == ROLE_SRC ? "__dense_src" : "__dense_dst") : m.base->cols[tc].name.c_str();
        capsmi_status st;
        if (ocols.empty()) st = capsmi_expand_filter(s, tab, tf, tt, a, b, 1, any, anyn, &o);
        else st = capsmi_expand_filter(s, tab, tf, tt, a, b, (int32_t)ocols.size(), ocols.data(), onames.data(), &o);
        if (g_dense) capsmi_table_release(tab);
        check(st);
        parts.push_back(o);
    }
    // assemble the output schema: data columns from the kernel, constants filled
    capsmi_table* acc = nullptr;
    for (capsmi_table* part : parts) {
        auto* r = result_table(s, part->nrows);
        for (size_t i = 0; i < P.cols.size(); ++i) {
            Column col;
            const int j = find_col(part, "c" + std::to_string(i));
            if (j >= 0) {
                col = part->cols[j];
            } else {
                const capsmi_expr& x = P.cols[i].cst;
                col.type = t->cols[i].type;
                col.data = dev_alloc(sizeof(int64_t) * (part->nrows > 0 ? part->nrows : 1), s);
                fill_i64(::capsmi::P<int64_t>(col.data), x.op == CAPSMI_X_LIT ? x.ival : 0, part->nrows, s->stream);
                if (x.op == CAPSMI_X_NULL || t->cols[i].nullable()) {
                    col.valid = dev_alloc(part->nrows > 0 ? part->nrows : 1, s);
                    fill_u8(::capsmi::P<uint8_t>(col.valid), x.op == CAPSMI_X_NULL ? 0 : 1, part->nrows, s->stream);
                }
            }
            col.name = t->cols[i].name;
            r->cols.push_back(col);
        }
        if (!acc) {
            acc = r;
        } else {
            capsmi_table* u = nullptr;
            const capsmi_status st = eager_union_all(acc, r, &u);
            capsmi_table_release(acc);
            capsmi_table_release(r);
            check(st);
            acc = u;
        }
    }
    acc->partitioned = g_dist.on;  // this rank's relationships' rows
    *out = acc;
    route(s, "expand");
    return true;
}

bool has_hop(const std::vector<Path>& B) {
    for (const Path& P : B) if (!P.hops.empty()) return true;
    return false;
}

}  // namespace

thread_local bool g_missed = false;  // a pattern shape went unrouted during the current materialisation

// a plan over entity tables in a pattern shape that no fused route took: counted once per
// materialisation as route "miss" (capsmi_session_route_count)
bool try_fused(capsmi_table* t, capsmi_table** out) {
    if (try_fused_shapes(t, out)) return true;
    const PlanNode& p = *t->plan;
    std::vector<Path> B;
    if (as_paths(p.kind == PlanNode::GROUP ? p.in[0] : t, B) && has_hop(B)) g_missed = true;
    return false;
}

bool try_fused_shapes(capsmi_table* t, capsmi_table** out) {
    capsmi_session* s = t->sess;
    if (!s->fused) return false;
    const PlanNode& p = *t->plan;
    if (p.kind == PlanNode::GROUP) {
        const capsmi_table* in = p.in[0];
        std::vector<Path> B;
        if (!as_paths(in, B) || B.empty()) return false;
        // The attempts in the order of the file's table, one order for plans with and without a key.  Order matters
        // only between routes that can both get past their launch-free checks on one plan, and the first-line guards
        // on B.size() and g.a.size() leave few such pairs: fused_counts wants no key and one branch, the two grouped
        // routes one key and one branch, fused_undirected two or four branches, fused_undirected_triangle eight,
        // fused_var_length one key.  fused_var_length_distinct takes any number of branches, but chains only, and
        // the branches of an undirected triangle are closed: each of the two declines the other's plans at the
        // first branch, before any node scan, and the one launch fused_var_length_distinct may make before its
        // branches, the id order of a compacted graph for a collect, is for a plan fused_undirected_triangle
        // declines at its aggregates (counts only), so it is made wherever the two stand.  Against
        // fused_undirected its place does show: the outgoing branch of an undirected chain is a chain to it, whose
        // ends it scans before the next branch's start <> end scan turns the plan down; it stays in front.  The
        // two var-length routes share their shape and differ in their aggregates.  Without a key a single branch,
        // the plain 1-hop count(DISTINCT b), is fused_counts's alone; fused_undirected does not look at a key, so
        // a plan with one does not get to it.
        const bool keyed = !p.a.empty();
        std::vector<int64_t> vals;  // of the routes that compute the aggregates' values, not their table
        if (!keyed && B.size() == 1) {
            std::vector<int> kinds;
            const int end = (int)B[0].pos_node.size() - 1;
            if (!agg_kinds(in, p, B[0], 0, B[0].hops.size() == 3 ? 0 : end, kinds)) return false;
            if (!fused_counts(s, B[0], kinds, vals)) return false;
        } else if (fused_grouped_two_hop(s, in, p, B, out) || fused_grouped_triangle(s, in, p, B, out) ||
                   fused_undirected_triangle(s, in, p, B, out) || fused_var_length_distinct(s, in, p, B, out)) {
            return true;
        } else if (keyed) {
            return fused_var_length(s, in, p, B, out);
        } else if (!fused_undirected(s, in, p, B, vals)) {
            return false;
        }
        *out = count_row(s, p.aggs, vals);
        return true;
    }
    std::vector<Path> B;
    if (!as_paths(t, B)) return false;
    return fused_projection(s, t, B, out);
}

}  // namespace planning
}  // namespace capsmi
