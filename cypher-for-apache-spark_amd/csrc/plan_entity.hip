// plan_entity.hip -- entity tables: registration (capsmi_node_table / capsmi_rel_table, attach_entity) with the
// 32-bit endpoint copies and the presence words made there, the session's routing setters and counters, the dense
// id compaction of a graph (capsmi_graph_compact) and capsmi_flatten_rel_types.
#include "plan_impl.h"
#include "narrow_rule.h"
#include "presence_rule.h"

namespace capsmi {

// The 32-bit copies of a registered relationship table's endpoint columns (Column::narrow; the rule:
// narrow_rule.h), base = the window's lo.  A storage encoding of the table, which no query shapes: made once, here,
// in one pass over both columns on the session's stream, and carried by every later view of the columns.
// Costs 8 B per relationship of device memory.  CAPSMI_NARROW=off: none.
static void narrow_endpoints(capsmi_table* t, const EntityInfo& e) {
    if (e.kind != 2 || !t->sess || !t->sess->cfg.narrow || t->lazy()) return;
    Column& sc = t->cols[e.src];
    Column& dc = t->cols[e.dst];
    if (sc.type != CAPSMI_I64 || dc.type != CAPSMI_I64 || sc.lazy_nullable || dc.lazy_nullable) return;
    if (!narrow_eligible(sc.valid != nullptr, dc.valid != nullptr, t->nrows, e.lo, e.hi)) return;
    capsmi_session* s = t->sess;
    HIP_CHECK(hipSetDevice(s->device));
    // each copy under its column's own row offset (a table registered behind a skip), so n32() applies it like d()
    try {
        sc.narrow = dev_alloc(sizeof(uint32_t) * (size_t)(sc.offset + t->nrows), s);
        dc.narrow = dev_alloc(sizeof(uint32_t) * (size_t)(dc.offset + t->nrows), s);
    } catch (const Error& x) {
        // the copies are optional: a table that leaves no room for them is registered without (every reader
        // then takes the int64 columns, and narrow_built does not count it)
        if (x.code != CAPSMI_ERR_OUT_OF_MEMORY) throw;
        sc.narrow.reset();
        dc.narrow.reset();
        return;
    }
    sc.narrow_of = sc.data.get();
    dc.narrow_of = dc.data.get();
    sc.narrow_base = dc.narrow_base = e.lo;
    narrow_pair_i64(s, sc.d(), dc.d(), t->nrows, e.lo, P<uint32_t>(sc.narrow) + sc.offset,
                    P<uint32_t>(dc.narrow) + dc.offset);
    s->routes["narrow_built"] += 1;
}

NarrowRel narrow_rel(const capsmi_session* s, const Column& sc, const Column& dc) {
    NarrowRel r;
    if (!s->cfg.narrow) return r;
    const uint32_t *a = sc.n32(), *b = dc.n32();
    if (a && b && sc.narrow_base == dc.narrow_base) {
        r.s = a;
        r.d = b;
        r.base = sc.narrow_base;
    }
    return r;
}

PresenceRel presence_rel(const capsmi_session* s, const Column& from, const Column& to, int64_t rows) {
    PresenceRel r;
    const std::shared_ptr<const PresenceWords>& w = to.presence;
    if (!s->cfg.presence || !w || rows != w->rows) return r;
    const DevBuf *f = from.data.get(), *t = to.data.get();
    const bool with = t == w->dst_of && f == w->src_of && to.offset == w->dst_off && from.offset == w->src_off;
    const bool against = t == w->src_of && f == w->dst_of && to.offset == w->src_off && from.offset == w->dst_off;
    if (!with && !against) return r;
    r.m = P<uint32_t>(with ? w->in : w->out);
    r.l1 = P<uint32_t>(w->loop1);
    r.l2 = P<uint32_t>(w->loop2);
    r.lo = w->lo;
    r.hi = w->hi;
    r.nwords = w->nwords;
    r.keep = w;
    return r;
}

// The presence words of a registered relationship table's endpoints (Column::presence; the rule: presence_rule.h).
// Like the 32-bit copies a fact about the immutable table, which no query shapes: made once, here, by the 2-hop's
// own build -- relpart_build with hop 1 over a full bitmap of the window leaves M = `in`, S1 = `loop1`, S2 =
// `loop2`, and the same with the columns swapped leaves `out` -- so whatever path that build takes, the words are
// what hop 1 would have computed.  Costs two builds at registration (transient: the pass-1 pool) and 4 bits per
// id of the window.  Two endpoint columns that already carry words valid for each other (a second registration
// of the same columns) reuse them.  CAPSMI_PRESENCE=off: none.
static void presence_endpoints(capsmi_table* t, const EntityInfo& e) {
    if (e.kind != 2 || !t->sess || !t->sess->cfg.presence || t->lazy()) return;
    Column& sc = t->cols[e.src];
    Column& dc = t->cols[e.dst];
    if (sc.type != CAPSMI_I64 || dc.type != CAPSMI_I64 || sc.lazy_nullable || dc.lazy_nullable) return;
    if (!presence_eligible(sc.valid != nullptr, dc.valid != nullptr, t->nrows, e.lo, e.hi)) return;
    if (sc.data.get() == dc.data.get()) return;  // one block on both sides: the sides could not be told apart
    capsmi_session* s = t->sess;
    if (presence_rel(s, sc, dc, t->nrows).m) {
        s->routes["presence_reused"] += 1;
        return;
    }
    HIP_CHECK(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    auto w = std::make_shared<PresenceWords>();
    w->lo = e.lo;
    w->hi = e.hi;
    w->nwords = (int64_t)(((uint64_t)e.hi - (uint64_t)e.lo + 31) / 32);
    w->src_of = sc.data.get();
    w->dst_of = dc.data.get();
    w->src_off = sc.offset;
    w->dst_off = dc.offset;
    w->rows = t->nrows;
    // the build is no routed query: its route counts and kernel timers stay out of the session's, which get one
    // `presence_build` timer and one `presence_built` count instead
    struct Quiet {
        capsmi_session* s;
        std::map<std::string, int64_t> routes;
        bool prof;
        ~Quiet() {
            s->routes = std::move(routes);
            s->prof = prof;
        }
    };
    try {
        const size_t bytes = sizeof(uint32_t) * (size_t)w->nwords;
        w->in = dev_alloc(bytes, s);
        w->out = dev_alloc(bytes, s);
        w->loop1 = dev_alloc(bytes, s);
        w->loop2 = dev_alloc(bytes, s);
        Buf spare = dev_alloc(2 * bytes, s);  // the swapped build's loop words: the same as the first's
        capsmi_bitmap all;
        all.sess = s;
        all.lo = e.lo;
        all.hi = e.hi;
        all.nwords = w->nwords;
        all.words = dev_alloc(bytes, s);
        all.set_bits = (int64_t)((uint64_t)e.hi - (uint64_t)e.lo);
        all.full = true;
        for (const Buf* b : {&w->in, &w->out, &w->loop1, &w->loop2}) HIP_CHECK(hipMemsetAsync(P<void>(*b), 0, bytes, st));
        HIP_CHECK(hipMemsetAsync(P<void>(spare), 0, 2 * bytes, st));
        HIP_CHECK(hipMemsetAsync(P<void>(all.words), 0xFF, bytes, st));
        KernelTimer kt(s, "presence_build");
        Quiet q{s, s->routes, s->prof};
        s->prof = false;
        const NarrowRel n = narrow_rel(s, sc, dc);
        for (int side = 0; side < 2; ++side) {
            const int64_t* from = side ? dc.d() : sc.d();
            const int64_t* to = side ? sc.d() : dc.d();
            NarrowRel ns = n;
            if (side) std::swap(ns.s, ns.d);
            const RelPartHop1 h1{&all, &all, P<uint32_t>(side ? w->out : w->in),
                                 side ? P<uint32_t>(spare) : P<uint32_t>(w->loop1),
                                 side ? P<uint32_t>(spare) + w->nwords : P<uint32_t>(w->loop2)};
            RelPart rp;  // the pool goes back to the allocator at the end of each round
            relpart_build(s, &from, &to, &t->nrows, 1, e.lo, e.hi, rp, &h1, false, &ns);
        }
    } catch (const Error& x) {
        // the words are optional, as the copies are: a table that leaves no room for the transient pool is
        // registered without (hop 1 then walks the pool, and presence_built does not count it)
        if (x.code != CAPSMI_ERR_OUT_OF_MEMORY) throw;
        return;
    }
    sc.presence = dc.presence = w;
    s->routes["presence_built"] += 1;
}

void attach_entity(capsmi_table* t, int kind, int64_t lo, int64_t hi, bool ids_exact, bool ids_unique) {
    auto e = std::make_shared<EntityInfo>();
    e->kind = kind;
    e->id = 0;
    if (kind == 2) {
        e->src = 1;
        e->dst = 2;
    }
    e->rows = t->nrows;
    e->lo = lo;
    e->hi = hi;
    e->ids_exact = ids_exact;
    e->ids_unique = ids_exact || ids_unique;
    t->entity = e;
    narrow_endpoints(t, *e);
    presence_endpoints(t, *e);
}

}  // namespace capsmi

using namespace capsmi;
using namespace capsmi::planning;

extern "C" {

capsmi_status capsmi_session_set_fused(capsmi_session* s, int32_t enabled) {
    P_BEGIN
    need(s, "session");
    s->fused = enabled != 0;
    P_END
}

capsmi_status capsmi_session_set_csv_partitioning(capsmi_session* s, int64_t default_parallelism,
                                                  int64_t max_partition_bytes, int64_t open_cost_bytes) {
    P_BEGIN
    need(s, "session");
    REQUIRE(default_parallelism >= 0 && max_partition_bytes > 0 && open_cost_bytes >= 0, CAPSMI_ERR_ILLEGAL_ARGUMENT,
            "csv partitioning: parallelism >= 0, max partition bytes > 0, open cost >= 0");
    s->csv_parallelism = default_parallelism;
    s->csv_max_partition_bytes = max_partition_bytes;
    s->csv_open_cost = open_cost_bytes;
    P_END
}

capsmi_status capsmi_session_set_unrouted_limit(capsmi_session* s, int64_t max_bytes) {
    P_BEGIN
    need(s, "session");
    REQUIRE(max_bytes >= 0, CAPSMI_ERR_ILLEGAL_ARGUMENT, "negative limit");
    s->unrouted_limit = max_bytes;
    P_END
}

capsmi_status capsmi_session_route_count(capsmi_session* s, const char* name, int64_t* count) {
    P_BEGIN
    need(s, "session");
    need(name, "name");
    need(count, "count");
    auto it = s->routes.find(name);
    *count = it == s->routes.end() ? 0 : it->second;
    P_END
}

// ---- entity tables ------------------------------------------------------------------------------
static void verify_key(const capsmi_table* t, const char* name, const char* what, int32_t type) {
    need(name, what);
    const int i = find_col(t, name);
    REQUIRE(i >= 0, CAPSMI_ERR_ILLEGAL_ARGUMENT,
            std::string("table with column key ") + name + " (EntityTable.verify: no such column)");
    const Column& c = t->cols[i];
    const char* tn = type == CAPSMI_I64 ? "CTInteger" : "CTBoolean";
    REQUIRE(c.type == type, CAPSMI_ERR_ILLEGAL_ARGUMENT,
            std::string(what) + " column `" + name + "` of type " + tn + " (incompatible column type)");
    REQUIRE(!c.nullable(), CAPSMI_ERR_ILLEGAL_ARGUMENT,
            std::string("non-nullable type for ") + what + " column `" + name + "` (nullable type)");
}

static capsmi_table* register_entity(capsmi_table* t, int kind, const std::vector<const char*>& keys,
                                     const std::vector<const char*>& flags) {
    // canonical order: keys ++ flags ++ properties sorted (EntityMapping.allSourceKeys, EntityMapping.scala:50)
    std::vector<std::string> want(keys.begin(), keys.end());
    want.insert(want.end(), flags.begin(), flags.end());
    std::set<std::string> fixed(want.begin(), want.end());
    REQUIRE(fixed.size() == want.size(), CAPSMI_ERR_ILLEGAL_ARGUMENT, "One-to-one mapping from entity elements to source keys");
    std::vector<std::string> props;
    for (auto& c : t->cols) if (!fixed.count(c.name)) props.push_back(c.name);
    std::sort(props.begin(), props.end());
    want.insert(want.end(), props.begin(), props.end());
    bool ok = want.size() == t->cols.size();
    for (size_t i = 0; ok && i < want.size(); ++i) ok = t->cols[i].name == want[i];
    if (!ok) {
        std::string exp, got;
        for (auto& w : want) exp += (exp.empty() ? "" : ", ") + w;
        for (auto& c : t->cols) got += (got.empty() ? "" : ", ") + c.name;
        throw Error(CAPSMI_ERR_ILLEGAL_ARGUMENT, "Columns: " + exp + " expected, got Columns: " + got +
                                                     " (use CAPS[Node|Relationship]Table#fromMapping to create a valid "
                                                     "EntityTable)");
    }
    materialize(t);
    auto e = std::make_shared<EntityInfo>();
    e->kind = kind;
    e->id = 0;
    if (kind == 2) {
        e->src = 1;
        e->dst = 2;
    }
    e->rows = t->nrows;
    if (t->nrows > 0) {
        capsmi_session* s = t->sess;
        HIP_CHECK(hipSetDevice(s->device));
        int64_t mm[2];
        if (kind == 1) {
            const int64_t* c[1] = {t->cols[0].d()};
            minmax_i64(s, c, 1, t->nrows, mm);
        } else {
            const int64_t* c[2] = {t->cols[1].d(), t->cols[2].d()};
            minmax_i64(s, c, 2, t->nrows, mm);
        }
        e->lo = mm[0];
        e->hi = mm[1] == INT64_MAX ? INT64_MAX : mm[1] + 1;
        if (kind == 1 && mm[1] != INT64_MAX && e->hi - e->lo <= (int64_t(1) << 31) && !t->cols[0].valid) {
            // one bitmap pass over [min, max]: whether an id repeats (a node scan of a table without
            // repeats then needs no count read back, capsmi_bitmap_add_scan), and whether the ids are
            // exactly that window (as many rows as ids in it, none repeated)
            capsmi_bitmap* b = nullptr;
            check(capsmi_bitmap_create(s, e->lo, e->hi, &b));
            const capsmi_status st = capsmi_bitmap_add_scan(b, t, t->cols[0].name.c_str(), 0, nullptr);
            e->ids_unique = st == CAPSMI_OK && !b->any_dup;
            e->ids_exact = e->ids_unique && b->set_bits == t->nrows && e->hi - e->lo == t->nrows;
            capsmi_bitmap_release(b);
            check(st);
        }
    }
    auto* o = new capsmi_table();
    o->sess = t->sess;
    o->nrows = t->nrows;
    o->cols = t->cols;
    o->entity = e;
    try {
        narrow_endpoints(o, *e);
        presence_endpoints(o, *e);
    } catch (...) {
        delete o;
        throw;
    }
    return o;
}

capsmi_status capsmi_node_table(capsmi_table* t, const char* id_col, int32_t nlabels, const char* const* label_cols,
                                capsmi_table** out) {
    return build(t, out, [&] {
        verify_key(t, id_col, "id key", CAPSMI_I64);
        std::vector<const char*> flags;
        for (int i = 0; i < nlabels; ++i) {
            verify_key(t, label_cols[i], "optional label", CAPSMI_BOOL);
            flags.push_back(label_cols[i]);
        }
        return register_entity(t, 1, {id_col}, flags);
    });
}

capsmi_status capsmi_rel_table(capsmi_table* t, const char* id_col, const char* src_col, const char* dst_col,
                               int32_t ntypes, const char* const* type_cols, capsmi_table** out) {
    return build(t, out, [&] {
        verify_key(t, id_col, "id key", CAPSMI_I64);
        verify_key(t, src_col, "start node", CAPSMI_I64);
        verify_key(t, dst_col, "end node", CAPSMI_I64);
        std::vector<const char*> flags;
        for (int i = 0; i < ntypes; ++i) {
            verify_key(t, type_cols[i], "relationship type", CAPSMI_BOOL);
            flags.push_back(type_cols[i]);
        }
        return register_entity(t, 2, {id_col, src_col, dst_col}, flags);
    });
}

}  // extern "C"

namespace capsmi {
namespace {

__global__ void k_dense_of(const int64_t* __restrict__ slot_of_probe, const int64_t* __restrict__ slot_row,
                           const int64_t* __restrict__ gid_of_row, int64_t n, int64_t* __restrict__ out,
                           uint8_t* __restrict__ miss) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t sl = slot_of_probe[i];
        out[i] = sl >= 0 ? gid_of_row[slot_row[sl]] : -1;
        miss[i] = sl < 0;
    }
}

__global__ void k_place_dense(const int64_t* __restrict__ idx, const int64_t* __restrict__ gid, int64_t n, int64_t base,
                              int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[idx[i]] = base + gid[i];
}

unsigned grid_of(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 65536)); }

KeyCols one_key(const int64_t* d) {
    KeyCols k;
    k.n = 1;
    for (int i = 0; i < kMaxKeys; ++i) { k.data[i] = nullptr; k.valid[i] = nullptr; }
    k.data[0] = d;
    return k;
}

}  // namespace

void graph_compact(capsmi_session* s, const std::vector<capsmi_table*>& nodes, const std::vector<capsmi_table*>& rels,
                   int64_t* n_out) {
    hipStream_t st = s->stream;
    int64_t nn = 0;
    for (auto* t : nodes) nn += t->nrows;
    // node ids of every node table, one key column
    Buf keys = dev_alloc(sizeof(int64_t) * (nn > 0 ? nn : 1), s);
    int64_t off = 0;
    for (auto* t : nodes) {
        if (t->nrows) HIP_CHECK(hipMemcpyAsync(::capsmi::P<int64_t>(keys) + off, t->cols[t->entity->id].d(),
                                               sizeof(int64_t) * t->nrows, hipMemcpyDeviceToDevice, st));
        off += t->nrows;
    }
    const KeyCols kc = one_key(::capsmi::P<int64_t>(keys));
    HashTable ht;
    Buf sor, gid, rep;
    hash_build(s, kc, nn, false, ht, sor);
    const int64_t ng = nn > 0 ? hash_group_ids(s, ht, sor, nn, gid, rep) : 0;
    // endpoints: probe the node ids; endpoints of no node table (dangling) are numbered after them
    struct Miss { Buf idx; int64_t n; Buf dense; };
    std::vector<Miss> miss;
    std::vector<std::pair<Buf, Buf>> rel_dense;
    for (auto* t : rels) {
        const int64_t m = t->nrows;
        Buf d[2];
        for (int k = 0; k < 2; ++k) {
            const Column& c = t->cols[k == 0 ? t->entity->src : t->entity->dst];
            d[k] = dev_alloc(sizeof(int64_t) * (m > 0 ? m : 1), s);
            if (m == 0) continue;
            Buf sop, fl = dev_alloc(m, s);
            hash_probe(s, one_key(c.d()), kc, m, ht, sop);
            hipLaunchKernelGGL(k_dense_of, dim3(grid_of(m)), dim3(256), 0, st, ::capsmi::P<int64_t>(sop),
                               ::capsmi::P<int64_t>(ht.slot_row), ::capsmi::P<int64_t>(gid), m,
                               ::capsmi::P<int64_t>(d[k]), ::capsmi::P<uint8_t>(fl));
            HIP_CHECK(hipGetLastError());
            Miss x;
            x.n = flags_to_indices(s, ::capsmi::P<uint8_t>(fl), m, x.idx);
            x.dense = d[k];
            if (x.n > 0) {
                // remember the missing keys next to their row indices
                Buf mk = dev_alloc(sizeof(int64_t) * x.n, s);
                gather_col(c.d(), nullptr, ::capsmi::P<int64_t>(x.idx), x.n, ::capsmi::P<int64_t>(mk), nullptr, st);
                miss.push_back(x);
                miss.push_back(Miss{mk, -1, Buf()});  // keys of the entry before
            }
        }
        rel_dense.push_back({d[0], d[1]});
    }
    int64_t nm = 0;
    for (size_t i = 0; i < miss.size(); i += 2) nm += miss[i].n;
    Buf mkeys = dev_alloc(sizeof(int64_t) * (nm > 0 ? nm : 1), s);
    off = 0;
    for (size_t i = 0; i < miss.size(); i += 2) {
        HIP_CHECK(hipMemcpyAsync(::capsmi::P<int64_t>(mkeys) + off, ::capsmi::P<int64_t>(miss[i + 1].idx),
                                 sizeof(int64_t) * miss[i].n, hipMemcpyDeviceToDevice, st));
        off += miss[i].n;
    }
    int64_t ng2 = 0;
    Buf gid2, rep2;
    if (nm > 0) {
        HashTable h2;
        Buf sor2;
        hash_build(s, one_key(::capsmi::P<int64_t>(mkeys)), nm, false, h2, sor2);
        ng2 = hash_group_ids(s, h2, sor2, nm, gid2, rep2);
        off = 0;
        for (size_t i = 0; i < miss.size(); i += 2) {
            hipLaunchKernelGGL(k_place_dense, dim3(grid_of(miss[i].n)), dim3(256), 0, st, ::capsmi::P<int64_t>(miss[i].idx),
                               ::capsmi::P<int64_t>(gid2) + off, miss[i].n, ng, ::capsmi::P<int64_t>(miss[i].dense));
            off += miss[i].n;
        }
        HIP_CHECK(hipGetLastError());
    }
    auto D = std::make_shared<DenseIds>();
    D->n = ng + ng2;
    D->orig = dev_alloc(sizeof(int64_t) * (D->n > 0 ? D->n : 1), s);
    if (ng) gather_col(::capsmi::P<int64_t>(keys), nullptr, ::capsmi::P<int64_t>(rep), ng, ::capsmi::P<int64_t>(D->orig),
                       nullptr, st);
    if (ng2) gather_col(::capsmi::P<int64_t>(mkeys), nullptr, ::capsmi::P<int64_t>(rep2), ng2,
                        ::capsmi::P<int64_t>(D->orig) + ng, nullptr, st);
    off = 0;
    for (auto* t : nodes) {
        t->dense = D;
        t->did = Column();
        t->did.type = CAPSMI_I64;
        t->did.data = gid;
        t->did.offset = off;
        off += t->nrows;
    }
    for (size_t i = 0; i < rels.size(); ++i) {
        auto* t = rels[i];
        t->dense = D;
        t->dsrc = Column();
        t->dsrc.type = CAPSMI_I64;
        t->dsrc.data = rel_dense[i].first;
        t->ddst = Column();
        t->ddst.type = CAPSMI_I64;
        t->ddst.data = rel_dense[i].second;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    *n_out = D->n;
}

}  // namespace capsmi

extern "C" {

capsmi_status capsmi_graph_compact(capsmi_session* s, int32_t nnodes, capsmi_table* const* nodes, int32_t nrels,
                                   capsmi_table* const* rels, int64_t* dense_ids) {
    P_BEGIN
    need(s, "session");
    REQUIRE(nnodes >= 0 && nrels >= 0 && (nnodes == 0 || nodes) && (nrels == 0 || rels), CAPSMI_ERR_ILLEGAL_ARGUMENT,
            "tables");
    HIP_CHECK(hipSetDevice(s->device));
    std::vector<capsmi_table*> nv, rv;
    for (int i = 0; i < nnodes; ++i) {
        need(nodes[i], "nodes[i]");
        REQUIRE(nodes[i]->entity && nodes[i]->entity->kind == 1 && nodes[i]->sess == s, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                "graph_compact: nodes[i] is not a node table of this session (capsmi_node_table)");
        nv.push_back(nodes[i]);
    }
    for (int i = 0; i < nrels; ++i) {
        need(rels[i], "rels[i]");
        REQUIRE(rels[i]->entity && rels[i]->entity->kind == 2 && rels[i]->sess == s, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                "graph_compact: rels[i] is not a relationship table of this session (capsmi_rel_table)");
        rv.push_back(rels[i]);
    }
    int64_t n = 0;
    graph_compact(s, nv, rv, &n);
    if (dense_ids) *dense_ids = n;
    P_END
}

capsmi_status capsmi_table_entity(const capsmi_table* t, int32_t* kind, int64_t* id_lo, int64_t* id_hi) {
    P_BEGIN
    need(t, "table");
    if (kind) *kind = t->entity ? t->entity->kind : 0;
    if (id_lo) *id_lo = t->entity ? t->entity->lo : 0;
    if (id_hi) *id_hi = t->entity ? t->entity->hi : 0;
    P_END
}

capsmi_status capsmi_flatten_rel_types(capsmi_table* t, const char* type_col, int32_t ntypes, const int64_t* type_codes,
                                       const char* const* out_cols, capsmi_table** out) {
    return build(t, out, [&] {
        const int tc = col_of(t, type_col);
        REQUIRE(t->cols[tc].type == CAPSMI_STR, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                std::string("relationship type column `") + type_col + "` of type CTString");
        REQUIRE(ntypes >= 0 && (ntypes == 0 || (type_codes && out_cols)), CAPSMI_ERR_ILLEGAL_ARGUMENT, "types");
        materialize(t);
        capsmi_session* s = t->sess;
        HIP_CHECK(hipSetDevice(s->device));
        auto* o = new capsmi_table();
        std::unique_ptr<capsmi_table> g(o);
        o->sess = s;
        o->nrows = t->nrows;
        for (size_t i = 0; i < t->cols.size(); ++i)
            if ((int)i != tc) o->cols.push_back(t->cols[i]);
        for (int k = 0; k < ntypes; ++k) {
            need(out_cols[k], "type column name");
            REQUIRE(find_col(o, out_cols[k]) < 0, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                    std::string("column '") + out_cols[k] + "' already exists");
            // coalesce(type = code, false): a non-nullable flag (setNonNullable, CAPSTable.scala:198-200)
            capsmi_expr prog[5] = {};
            prog[0].op = CAPSMI_X_COL;
            prog[0].arg = tc;
            prog[1].op = CAPSMI_X_LIT;
            prog[1].type = CAPSMI_STR;
            prog[1].ival = type_codes[k];
            prog[2].op = CAPSMI_X_EQ;
            prog[3].op = CAPSMI_X_LIT;
            prog[3].type = CAPSMI_BOOL;
            prog[3].ival = 0;
            prog[4].op = CAPSMI_X_COALESCE;
            prog[4].arg = 2;
            Column c;
            c.name = out_cols[k];
            c.data = dev_alloc(sizeof(int64_t) * (t->nrows > 0 ? t->nrows : 1), s);
            eval_expr(s, t, 5, prog, P<int64_t>(c.data), nullptr, &c.type);
            c.type = CAPSMI_BOOL;
            o->cols.push_back(std::move(c));
        }
        return g.release();
    });
}

}  // extern "C"
