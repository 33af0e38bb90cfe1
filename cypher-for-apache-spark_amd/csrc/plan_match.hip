// plan_match.hip -- the pattern recogniser: a lazy plan over registered entity tables read back as the MATCH it
// came from.  as_scan folds a sub-plan into a scan (a union of entity tables, each column a base column or a
// constant); as_paths folds the joins above scans into paths (positions joined by hops) with their filter
// conjuncts, one path per branch of a union; classify sorts the conjuncts into relationship uniqueness and node
// predicates; id_window picks the id domain the kernels run on; node_bitmap and rel_views turn a path's scans
// into the kernels' inputs.  The routes (plan_routes.hip) decide what the paths are.
#include "plan_impl.h"

namespace capsmi {
namespace planning {

// ================================ the recogniser ===========================================

namespace {

void scan_roles(Scan& sc, size_t ncols) {
    sc.role.assign(ncols, ROLE_NONE);
    for (size_t k = 0; k < ncols; ++k) {
        for (int r : {ROLE_ID, ROLE_SRC, ROLE_DST}) {
            bool all = !sc.m.empty();
            for (const Member& m : sc.m) {
                const EntityInfo& e = *m.base->entity;
                const int want = r == ROLE_ID ? e.id : (r == ROLE_SRC ? e.src : e.dst);
                if (want < 0 || m.src[k] != want) { all = false; break; }
            }
            if (all) { sc.role[k] = r; break; }
        }
    }
}

}  // namespace

bool as_scan(const capsmi_table* t, Scan& sc) {
    if (!t->lazy()) {
        if (!t->entity) return false;
        sc = Scan();
        sc.kind = t->entity->kind;
        Member m;
        m.base = const_cast<capsmi_table*>(t);
        for (size_t k = 0; k < t->cols.size(); ++k) m.src.push_back((int)k);
        m.cst.resize(t->cols.size());
        sc.m.push_back(std::move(m));
        scan_roles(sc, t->cols.size());
        return true;
    }
    const PlanNode& p = *t->plan;
    const capsmi_table* in = p.in.empty() ? nullptr : p.in[0];
    switch (p.kind) {
        case PlanNode::WITH_COLUMNS: {
            if (pinned(t) || !as_scan(in, sc)) return false;
            std::vector<std::string> names;
            for (auto& c : in->cols) names.push_back(c.name);
            const std::vector<Member> before = sc.m;  // expressions read the input columns
            for (size_t i = 0; i < p.a.size(); ++i) {
                if (p.progs[i].size() != 1) return false;
                const capsmi_expr& x = p.progs[i][0];
                if (x.op != CAPSMI_X_COL && x.op != CAPSMI_X_LIT && x.op != CAPSMI_X_NULL) return false;
                int j = -1;
                for (size_t q = 0; q < names.size(); ++q) if (names[q] == p.a[i]) j = (int)q;
                if (j < 0) {
                    j = (int)names.size();
                    names.push_back(p.a[i]);
                    for (Member& m : sc.m) { m.src.push_back(-1); m.cst.push_back(capsmi_expr{}); }
                }
                for (size_t q = 0; q < sc.m.size(); ++q) {
                    Member& m = sc.m[q];
                    if (x.op == CAPSMI_X_COL) {
                        m.src[j] = before[q].src[x.arg];
                        m.cst[j] = before[q].cst[x.arg];
                    } else {
                        m.src[j] = -1;
                        m.cst[j] = x;
                    }
                }
            }
            break;
        }
        case PlanNode::SELECT:
        case PlanNode::DROP:
        case PlanNode::RENAME: {
            if (!as_scan(in, sc)) return false;
            std::vector<int> pick;
            if (p.kind == PlanNode::SELECT) {
                for (auto& nm : p.a) pick.push_back(find_col(in, nm));
            } else if (p.kind == PlanNode::DROP) {
                std::set<std::string> d(p.a.begin(), p.a.end());
                for (size_t k = 0; k < in->cols.size(); ++k) if (!d.count(in->cols[k].name)) pick.push_back((int)k);
            } else {
                for (size_t k = 0; k < in->cols.size(); ++k) pick.push_back((int)k);
            }
            for (Member& m : sc.m) {
                Member o;
                o.base = m.base;
                for (int k : pick) { o.src.push_back(m.src[k]); o.cst.push_back(m.cst[k]); }
                m = std::move(o);
            }
            break;
        }
        case PlanNode::UNION: {
            Scan r;
            if (!as_scan(in, sc) || !as_scan(p.in[1], r) || sc.kind != r.kind || sc.no_loops || r.no_loops) return false;
            for (Member& m : r.m) sc.m.push_back(std::move(m));
            break;
        }
        case PlanNode::FILTER: {  // only NOT(start = end) / start <> end over a relationship scan
            if (!as_scan(in, sc) || sc.kind != 2 || sc.no_loops) return false;
            const auto& pr = p.progs[0];
            const bool neq = pr.size() == 3 && pr[2].op == CAPSMI_X_NEQ;
            const bool negated_eq = pr.size() == 4 && pr[2].op == CAPSMI_X_EQ && pr[3].op == CAPSMI_X_NOT;
            if (!(neq || negated_eq) || pr[0].op != CAPSMI_X_COL || pr[1].op != CAPSMI_X_COL) return false;
            const int r0 = sc.role[pr[0].arg], r1 = sc.role[pr[1].arg];
            if (!((r0 == ROLE_SRC && r1 == ROLE_DST) || (r0 == ROLE_DST && r1 == ROLE_SRC))) return false;
            sc.no_loops = true;
            return true;  // same columns, same roles
        }
        default: return false;
    }
    scan_roles(sc, t->cols.size());
    return true;
}

namespace {

// operands of a node of a validated program (the one table of expr_prog.h)
int arity(const capsmi_expr& x) {
    const int k = expr_pops(x);
    REQUIRE(k >= 0, CAPSMI_ERR_NOT_IMPLEMENTED, "unknown expression op " + std::to_string(x.op));
    return k;
}

bool parse_prog(const std::vector<capsmi_expr>& prog, const std::vector<Role>& cols, ENode& out) {
    std::vector<ENode> st;
    for (const capsmi_expr& x : prog) {
        const int k = arity(x);
        if (k < 0 || (int)st.size() < k) return false;
        ENode n;
        n.x = x;
        n.kids.assign(st.end() - k, st.end());
        st.resize(st.size() - k);
        if (x.op == CAPSMI_X_COL) {
            if (x.arg < 0 || x.arg >= (int)cols.size()) return false;
            n.role = cols[x.arg];
        }
        st.push_back(std::move(n));
    }
    if (st.size() != 1) return false;
    out = std::move(st[0]);
    return true;
}

void flatten_and(const ENode& n, std::vector<ENode>& out) {
    if (n.x.op == CAPSMI_X_AND) {
        for (const ENode& k : n.kids) flatten_and(k, out);
    } else {
        out.push_back(n);
    }
}

}  // namespace

// position a join column denotes: a node scan's id, or one end of a relationship hop
int position_of(const Path& P, const Role& r) {
    if (r.k == RK_NODE) {
        if (P.inst[r.inst].role[r.scol] != ROLE_ID) return -1;
        for (size_t p = 0; p < P.pos_node.size(); ++p)
            if (P.pos_node[p] == r.inst) return (int)p;
        return -1;
    }
    if (r.k == RK_REL) {
        const int role = P.inst[r.inst].role[r.scol];
        for (const Hop& h : P.hops) {
            if (h.rel != r.inst) continue;
            if (role == h.from_role) return h.from;
            if (role == h.to_role) return h.to;
        }
    }
    return -1;
}

namespace {

// one left path joined with scan R (JOIN node p over left input `in`): a node scan completes a position,
// a relationship scan adds a hop (Expand) or closes one (ExpandInto)
bool join_path(Path P, const capsmi_table* in, const PlanNode& p, const Scan& R, std::vector<Path>& out) {
    const int ri = (int)P.inst.size();
    std::vector<int> lk, rk;
    for (size_t i = 0; i < p.a.size(); ++i) {
        lk.push_back(find_col(in, p.a[i]));
        rk.push_back(find_col(p.in[1], p.b[i]));
        if (lk.back() < 0 || rk.back() < 0) return false;
    }
    P.inst.push_back(R);
    if (R.kind == 1) {
        if (lk.size() != 1 || R.role[rk[0]] != ROLE_ID) return false;
        const int pos = position_of(P, P.cols[lk[0]]);
        if (pos < 0 || P.pos_node[pos] >= 0) return false;
        P.pos_node[pos] = ri;
    } else {
        if (lk.size() == 1) {  // Expand: a new position
            const int pos = position_of(P, P.cols[lk[0]]);
            const int rr = R.role[rk[0]];
            if (pos < 0 || (rr != ROLE_SRC && rr != ROLE_DST)) return false;
            Hop h;
            h.rel = ri;
            h.from = pos;
            h.to = (int)P.pos_node.size();
            h.from_role = rr;
            h.to_role = rr == ROLE_SRC ? ROLE_DST : ROLE_SRC;
            P.pos_node.push_back(-1);
            P.hops.push_back(h);
        } else if (lk.size() == 2) {  // ExpandInto: both ends bound
            const int p1 = position_of(P, P.cols[lk[0]]), p2 = position_of(P, P.cols[lk[1]]);
            const int r1 = R.role[rk[0]], r2 = R.role[rk[1]];
            if (p1 < 0 || p2 < 0 || !((r1 == ROLE_SRC && r2 == ROLE_DST) || (r1 == ROLE_DST && r2 == ROLE_SRC)))
                return false;
            Hop h;
            h.rel = ri;
            h.from = r1 == ROLE_SRC ? p1 : p2;
            h.to = r1 == ROLE_SRC ? p2 : p1;
            P.hops.push_back(h);
        } else {
            return false;
        }
    }
    const capsmi_table* rt = p.in[1];
    for (size_t k = 0; k < rt->cols.size(); ++k) {
        Role r;
        r.k = R.kind == 1 ? RK_NODE : RK_REL;
        r.inst = ri;
        r.scol = (int)k;
        P.cols.push_back(r);
    }
    out.push_back(std::move(P));
    return true;
}

bool as_paths_node(const capsmi_table* t, std::vector<Path>& out) {
    const PlanNode& p = *t->plan;
    const capsmi_table* in = p.in[0];
    switch (p.kind) {
        case PlanNode::JOIN: {
            if (p.jt != CAPSMI_JOIN_INNER) return false;
            std::vector<Path> L;
            Scan R;
            if (!as_paths(in, L) || L.empty() || !as_scan(p.in[1], R)) return false;
            // a join over a union of branches is the union of the joins (the second hop of an
            // undirected Expand joins both branches of the first)
            for (Path& lp : L)
                if (!join_path(std::move(lp), in, p, R, out)) return false;
            return true;
        }
        case PlanNode::FILTER: {
            if (!as_paths(in, out)) return false;
            for (Path& P : out) {
                ENode e;
                if (!parse_prog(p.progs[0], P.cols, e)) return false;
                flatten_and(e, P.conj);
            }
            return true;
        }
        case PlanNode::WITH_COLUMNS: {
            if (pinned(t) || !as_paths(in, out)) return false;  // a row index is no column of a pattern
            for (Path& P : out) {
                std::vector<Role> cols = P.cols;
                std::vector<std::string> names;
                for (auto& c : in->cols) names.push_back(c.name);
                for (size_t i = 0; i < p.a.size(); ++i) {
                    Role r;
                    const auto& prog = p.progs[i];
                    if (prog.size() == 1 && prog[0].op == CAPSMI_X_COL) r = P.cols[prog[0].arg];
                    else if (prog.size() == 1 && (prog[0].op == CAPSMI_X_LIT || prog[0].op == CAPSMI_X_NULL)) {
                        r.k = RK_CONST;
                        r.cst = prog[0];
                    }
                    int j = -1;
                    for (size_t q = 0; q < names.size(); ++q) if (names[q] == p.a[i]) j = (int)q;
                    if (j < 0) { names.push_back(p.a[i]); cols.push_back(r); }
                    else cols[j] = r;
                }
                P.cols = std::move(cols);
            }
            return true;
        }
        case PlanNode::SELECT:
        case PlanNode::DROP:
        case PlanNode::RENAME: {
            if (!as_paths(in, out)) return false;
            std::vector<int> pick;
            if (p.kind == PlanNode::SELECT) {
                for (auto& nm : p.a) pick.push_back(find_col(in, nm));
            } else if (p.kind == PlanNode::DROP) {
                std::set<std::string> d(p.a.begin(), p.a.end());
                for (size_t k = 0; k < in->cols.size(); ++k) if (!d.count(in->cols[k].name)) pick.push_back((int)k);
            } else {
                for (size_t k = 0; k < in->cols.size(); ++k) pick.push_back((int)k);
            }
            for (Path& P : out) {
                std::vector<Role> c;
                for (int k : pick) c.push_back(P.cols[k]);
                P.cols = std::move(c);
            }
            return true;
        }
        case PlanNode::UNION: {
            std::vector<Path> r;
            if (!as_paths(in, out) || !as_paths(p.in[1], r)) return false;
            for (Path& x : r) out.push_back(std::move(x));
            return true;
        }
        default: return false;
    }
}

}  // namespace

bool as_paths(const capsmi_table* t, std::vector<Path>& out) {
    Scan sc;
    if (as_scan(t, sc)) {  // a node scan starts a pattern
        if (sc.kind != 1) return false;
        Path P;
        P.inst.push_back(sc);
        P.pos_node.push_back(0);
        for (size_t k = 0; k < t->cols.size(); ++k) {
            Role r;
            r.k = RK_NODE;
            r.inst = 0;
            r.scol = (int)k;
            P.cols.push_back(r);
        }
        out.push_back(std::move(P));
        return true;
    }
    if (!t->lazy()) return false;
    return as_paths_node(t, out);
}

namespace {

// ---- conjunct classification ----------------------------------------------------------------
int hop_of_rel_id(const Path& P, const ENode& n) {
    if (n.x.op != CAPSMI_X_COL || n.role.k != RK_REL) return -1;
    if (P.inst[n.role.inst].role[n.role.scol] != ROLE_ID) return -1;
    for (size_t h = 0; h < P.hops.size(); ++h)
        if (P.hops[h].rel == n.role.inst) return (int)h;
    return -1;
}

// NOT(r_i = r_j) / r_i <> r_j over two hops' relationship ids
bool uniqueness(const Path& P, const ENode& c, int* i, int* j) {
    const ENode* eq = nullptr;
    if (c.x.op == CAPSMI_X_NOT && c.kids[0].x.op == CAPSMI_X_EQ) eq = &c.kids[0];
    else if (c.x.op == CAPSMI_X_NEQ) eq = &c;
    if (!eq) return false;
    *i = hop_of_rel_id(P, eq->kids[0]);
    *j = hop_of_rel_id(P, eq->kids[1]);
    return *i >= 0 && *j >= 0 && *i != *j;
}

// leaves of a node predicate: one node instance's columns and constants; returns the instance or -1
bool node_leaves(const ENode& n, int* inst) {
    if (n.x.op == CAPSMI_X_COL) {
        if (n.role.k == RK_CONST) return true;
        if (n.role.k != RK_NODE) return false;
        if (*inst >= 0 && *inst != n.role.inst) return false;
        *inst = n.role.inst;
        return true;
    }
    for (const ENode& k : n.kids)
        if (!node_leaves(k, inst)) return false;
    return true;
}

// postfix program of a node predicate over one member's base table
void emit_pred(const ENode& n, const Member& m, std::vector<capsmi_expr>& out) {
    for (const ENode& k : n.kids) emit_pred(k, m, out);
    if (n.x.op == CAPSMI_X_COL) {
        if (n.role.k == RK_CONST) {
            out.push_back(n.role.cst);
        } else if (m.src[n.role.scol] >= 0) {
            capsmi_expr x{};
            x.op = CAPSMI_X_COL;
            x.arg = m.src[n.role.scol];
            out.push_back(x);
        } else {
            out.push_back(m.cst[n.role.scol]);
        }
    } else {
        out.push_back(n.x);
    }
}

}  // namespace

bool classify(const Path& P, Classified& c) {
    c.pred.assign(P.inst.size(), {});
    for (const ENode& e : P.conj) {
        int i, j;
        if (uniqueness(P, e, &i, &j)) {
            c.uniq.insert({std::min(i, j), std::max(i, j)});
            continue;
        }
        int inst = -1;
        if (!node_leaves(e, &inst)) return false;
        if (inst < 0) {  // constant conjunct: only TRUE is harmless
            if (e.x.op == CAPSMI_X_LIT && e.x.type == CAPSMI_BOOL && e.x.ival != 0) continue;
            return false;
        }
        c.pred[inst].push_back(&e);
    }
    return true;
}

// The id domain the fused kernels run on: the Long ids' window when it holds at most 2^30 ids,
// else the dense ids of a compacted graph (capsmi_graph_compact) shared by every scanned table.
thread_local const DenseIds* g_dense = nullptr;  // domain of the route being planned (one at a time)

thread_local DistView g_dist;

namespace {

// every scanned table a shard of one distributed graph (then g_dense / g_dist are set), none, or a mix (false)
bool dist_window(const std::vector<Path>& B, bool* any, int64_t* lo, int64_t* hi) {
    const DenseIds* d = nullptr;
    const Shard* sh = nullptr;
    const capsmi_session* sess = nullptr;
    bool all = true;
    int rel_mode = -1;
    *any = false;
    for (const Path& P : B)
        for (const Scan& sc : P.inst) {
            int node_mode = -1;
            for (const Member& m : sc.m) {
                const capsmi_table* t = m.base;
                if (!t->shard) { all = false; continue; }
                *any = true;
                sess = t->sess;
                const DenseIds* e = t->dense.get();  // one domain: equal scramble (tables distributed apart)
                if (d && (e->n != d->n || e->kbits != d->kbits || e->lo != d->lo || e->mul != d->mul)) return false;
                d = e;
                sh = t->shard.get();
                if (sh->kind == 2) {
                    if (rel_mode >= 0 && rel_mode != sh->mode) return false;
                    rel_mode = sh->mode;
                } else {  // one node scan: all members replicated or all owned
                    if (node_mode >= 0 && node_mode != sh->mode) return false;
                    node_mode = sh->mode;
                }
            }
        }
    if (!*any) return true;
    if (!all || !d || d->n > (int64_t(1) << 30)) return false;
    g_dense = d;
    *lo = 0;
    *hi = d->n;
    // world 1 with a collective: the distributed routes over the one shard (their exchanges run through
    // the collective, e.g. RCCL at world size 1)
    if (sh->world > 1 || (sess && sess->coll != nullptr)) {
        g_dist.on = true;
        g_dist.rank = sh->rank;
        g_dist.world = sh->world;
        g_dist.slice_words = sh->slice_words;
        g_dist.rel_mode = rel_mode;
    }
    return true;
}

}  // namespace

bool id_window(const std::vector<Path>& B, int64_t* lo, int64_t* hi) {
    g_dist = DistView();
    g_dense = nullptr;
    bool any_shard = false;
    if (!dist_window(B, &any_shard, lo, hi)) return false;
    if (any_shard) return true;
    int64_t l = INT64_MAX, h = INT64_MIN;
    const DenseIds* d = nullptr;
    bool all_dense = true;
    for (const Path& P : B)
        for (const Scan& sc : P.inst)
            for (const Member& m : sc.m) {
                if (!m.base->dense || (d && m.base->dense.get() != d)) all_dense = false;
                else d = m.base->dense.get();
                if (m.base->entity->rows == 0) continue;
                l = std::min(l, m.base->entity->lo);
                h = std::max(h, m.base->entity->hi);
            }
    if (l < h && (uint64_t)(h - l) <= (uint64_t(1) << 30)) {
        *lo = l;
        *hi = h;
        return true;
    }
    if (all_dense && d && !d->scrambled && d->n > 0 && (uint64_t)d->n <= (uint64_t(1) << 30)) {
        g_dense = d;
        *lo = 0;
        *hi = d->n;
        return true;
    }
    return false;
}

// a zero-copy view of a base table with its dense key columns appended (dense domain only)
capsmi_table* dense_view(const capsmi_table* base) {
    auto* x = new capsmi_table();
    x->sess = base->sess;
    x->nrows = base->nrows;
    x->cols = base->cols;
    Column a = base->did, b = base->dsrc, c = base->ddst;
    a.name = "__dense_id";
    b.name = "__dense_src";
    c.name = "__dense_dst";
    if (base->entity->kind == 1) x->cols.push_back(a);
    else { x->cols.push_back(b); x->cols.push_back(c); }
    return x;
}

namespace {

// ---- bitmaps of node scans (+ predicates) ------------------------------------------------------

std::string member_prog_key(const capsmi_table* base, const std::vector<capsmi_expr>& prog) {
    std::string k(reinterpret_cast<const char*>(&base), sizeof(base));
    k.append(reinterpret_cast<const char*>(prog.data()), prog.size() * sizeof(capsmi_expr));
    return k + "|";
}

// A node scan over OWNED shards (multi-GPU): every rank set the bits of the ids it owns, which lie in
// its slice of the words; one all-gather of the slices completes the bitmap on every rank, and one SUM
// all-reduce gives its set-bit count and whether any rank saw a duplicate row (an id's rows are all on
// its owner, so duplicates are rank-local).
void gather_owned_bitmap(capsmi_session* s, capsmi_bitmap* b) {
    const int64_t S = g_dist.slice_words;
    REQUIRE(b->nwords == S * g_dist.world, CAPSMI_ERR_INTERNAL, "distributed bitmap geometry");
    // a scan that left its count unknown (capsmi_bitmap_add_scan): this rank's bits, before the gather
    if (b->set_bits < 0) b->set_bits = words_popcount(s, P<uint32_t>(b->words), 0, b->nwords);
    Buf full = dev_alloc(sizeof(uint32_t) * (size_t)b->nwords, s);
    collective(s, CAPSMI_COLL_ALL_GATHER, P<uint32_t>(b->words) + (int64_t)g_dist.rank * S, P<uint32_t>(full), S,
               CAPSMI_COLL_U32);
    b->words = full;
    Buf st = dev_alloc(2 * sizeof(int64_t), s);
    fill_i64(P<int64_t>(st), b->set_bits, 1, s->stream);
    fill_i64(P<int64_t>(st) + 1, b->any_dup ? 1 : 0, 1, s->stream);
    collective(s, CAPSMI_COLL_ALL_REDUCE_SUM, P<int64_t>(st), P<int64_t>(st), 2, CAPSMI_I64);
    int64_t h[2];
    HIP_CHECK(hipMemcpyAsync(h, P<void>(st), sizeof(h), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    b->set_bits = h[0];
    b->any_dup = h[1] > 0;
    b->full = b->set_bits == b->hi - b->lo;
}

}  // namespace

// bitmap of node instance `inst` with its predicate conjuncts over [lo, hi); identical scans share one.
// Returns null when an id occurs in two scanned rows (CAPS would bind it twice, ScanGraph.scala:72-76).
capsmi_bitmap* node_bitmap(capsmi_session* s, const Path& P, const Classified& c, int inst, int64_t lo, int64_t hi,
                           BitmapSet& bs, std::string* key_out) {
    const Scan& sc = P.inst[inst];
    std::vector<std::vector<capsmi_expr>> progs;
    std::string key;
    for (const Member& m : sc.m) {
        std::vector<capsmi_expr> prog;
        for (const ENode* e : c.pred[inst]) emit_pred(*e, m, prog);
        if (c.pred[inst].size() > 1) {
            capsmi_expr a{};
            a.op = CAPSMI_X_AND;
            a.arg = (int32_t)c.pred[inst].size();
            prog.push_back(a);
        }
        key += member_prog_key(m.base, prog);
        progs.push_back(std::move(prog));
    }
    if (key_out) *key_out = key;
    for (auto& x : bs.made)
        if (x.first == key) return x.second;
    capsmi_bitmap* b = nullptr;
    check(capsmi_bitmap_create(s, lo, hi, &b));
    bs.made.push_back({key, b});
    if (g_dist.on && g_dense && sc.m.size() == 1 && progs[0].empty() && sc.m[0].base->shard &&
        sc.m[0].base->shard->covers && lo == 0 && hi == g_dense->n) {
        // a node table covering the whole domain (over the ranks' shards, checked at registration): every
        // bit set, no row read, no exchange
        bitmap_set_range(b, 0, hi);
        b->rows_added = b->set_bits = hi;
        b->full = true;
        return b;
    }
    for (size_t i = 0; i < sc.m.size(); ++i) {
        const Member& m = sc.m[i];
        const capsmi_expr* pr = progs[i].empty() ? nullptr : progs[i].data();
        if (g_dense) {  // predicate columns keep their indices: the dense id is appended
            capsmi_table* v = dense_view(m.base);
            const capsmi_status st = capsmi_bitmap_add_scan(b, v, "__dense_id", (int32_t)progs[i].size(), pr);
            capsmi_table_release(v);
            check(st);
        } else {
            check(capsmi_bitmap_add_scan(b, m.base, m.base->cols[m.base->entity->id].name.c_str(),
                                         (int32_t)progs[i].size(), pr));
        }
    }
    bool owned = false;
    for (const Member& m : sc.m) owned = owned || (m.base->shard && m.base->shard->mode == CAPSMI_NODES_OWNED);
    if (g_dist.on && owned) gather_owned_bitmap(s, b);
    return b->any_dup ? nullptr : b;
}

void rel_views(const Path& P, const Hop& h, RelViews& v) {
    std::vector<std::string> sig;
    for (const Member& m : P.inst[h.rel].m) {
        const EntityInfo& e = *m.base->entity;
        const int fc = h.from_role == ROLE_SRC ? e.src : e.dst, tc = h.to_role == ROLE_SRC ? e.src : e.dst;
        auto* x = new capsmi_table();
        x->sess = m.base->sess;
        x->nrows = m.base->nrows;
        Column a = m.base->cols[fc], b = m.base->cols[tc];
        if (g_dense) {
            a = h.from_role == ROLE_SRC ? m.base->dsrc : m.base->ddst;
            b = h.to_role == ROLE_SRC ? m.base->dsrc : m.base->ddst;
        }
        a.name = "s";
        b.name = "t";
        x->cols = {a, b};
        v.t.push_back(x);
        std::string k(reinterpret_cast<const char*>(&m.base), sizeof(m.base));
        k += char(fc);
        k += char(tc);
        k += g_dense ? 'D' : 'L';
        sig.push_back(k);
    }
    std::sort(sig.begin(), sig.end());
    for (auto& k : sig) v.sig += k;
}

// the same relationship views read backwards: (s, t) <- (t, s), zero-copy
void reversed_views(const RelViews& v, RelViews& r) {
    for (capsmi_table* x : v.t) {
        auto* y = new capsmi_table();
        y->sess = x->sess;
        y->nrows = x->nrows;
        Column a = x->cols[1], b = x->cols[0];
        a.name = "s";
        b.name = "t";
        y->cols = {a, b};
        r.t.push_back(y);
    }
    r.sig = v.sig + "~";
}

bool id_like(const Path& P, const Role& r) {  // a non-null id / endpoint column
    if (r.k == RK_NODE) return P.inst[r.inst].role[r.scol] == ROLE_ID;
    if (r.k == RK_REL) return P.inst[r.inst].role[r.scol] != ROLE_NONE;
    return false;
}

capsmi_table* result_table(capsmi_session* s, int64_t rows) {
    auto* r = new capsmi_table();
    r->sess = s;
    r->nrows = rows;
    return r;
}

// ---- the shapes ---------------------------------------------------------------------------------

// count-like aggregates of a group over one branch
bool agg_kinds(const capsmi_table* in, const PlanNode& g, const Path& P, int start, int end, std::vector<int>& kinds) {
    for (const AggSpec& a : g.aggs) {
        if (a.kind == CAPSMI_AGG_COUNT_STAR) { kinds.push_back(A_COUNT); continue; }
        if (a.kind != CAPSMI_AGG_COUNT) return false;
        const int c = find_col(in, a.input);
        if (c < 0) return false;
        const Role& r = P.cols[c];
        if (!a.distinct) {
            if (!id_like(P, r)) return false;
            kinds.push_back(A_COUNT);
            continue;
        }
        const int pos = position_of(P, r);
        if (pos >= 0 && pos == end && end != start) kinds.push_back(A_DISTINCT_END);
        else if (pos >= 0 && pos == start && end != start) kinds.push_back(A_DISTINCT_START);
        else return false;
    }
    return true;
}

// chain P0 -h0-> P1 -h1-> ... with hop i from position i to i + 1; true if the hops form that chain
bool is_chain(const Path& P) {
    for (size_t i = 0; i < P.hops.size(); ++i)
        if (P.hops[i].from != (int)i || P.hops[i].to != (int)i + 1) return false;
    return P.pos_node.size() == P.hops.size() + 1;
}

bool same_orientation(const Path& P) {
    for (const Hop& h : P.hops)
        if (h.from_role != P.hops[0].from_role) return false;
    return true;
}

// hop h read along its relationships: from the position at their source to the position at their target
Hop directed(const Hop& h) {
    Hop d;
    d.rel = h.rel;
    d.from = h.from_role == ROLE_SRC ? h.from : h.to;
    d.to = h.from_role == ROLE_SRC ? h.to : h.from;
    return d;
}

// The closed path over three positions: Expands 0 - 1 and 1 - 2 and the ExpandInto between 2 and 0 (whose Hop
// runs from the position joined on the source to the one joined on the target), each in either direction.  The
// eight spellings are two patterns up to relabelling, told apart by the positions' out-degrees among the three
// relationships: (1, 1, 1) is the directed cycle, and otherwise one position has 2 (the source of the transitive
// triangle (a)->(b)->(c)<-(a)), one 1 (the middle) and one 0 (the sink); role[p] = CAPSMI_TRI_ROLE_* of position p.
int closed_triangle(const Path& P, int role[3]) {
    if (P.hops.size() != 3 || P.pos_node.size() != 3) return TRI_NONE;
    const Hop &h0 = P.hops[0], &h1 = P.hops[1], &h2 = P.hops[2];
    if (!(h0.from == 0 && h0.to == 1 && h1.from == 1 && h1.to == 2)) return TRI_NONE;
    if (!((h2.from == 2 && h2.to == 0) || (h2.from == 0 && h2.to == 2))) return TRI_NONE;
    int out[3] = {0, 0, 0};
    for (const Hop& h : P.hops) out[directed(h).from] += 1;
    if (out[0] == 1 && out[1] == 1 && out[2] == 1) return TRI_CYCLE;
    for (int p = 0; p < 3; ++p)
        role[p] = out[p] == 2 ? CAPSMI_TRI_ROLE_SOURCE : out[p] == 1 ? CAPSMI_TRI_ROLE_MIDDLE : CAPSMI_TRI_ROLE_SINK;
    return TRI_TRANSITIVE;
}

bool all_pairs_unique(const Classified& c, int nh) {
    for (int i = 0; i < nh; ++i)
        for (int j = i + 1; j < nh; ++j)
            if (!c.uniq.count({i, j})) return false;
    return (int)c.uniq.size() == nh * (nh - 1) / 2;
}

// What the triangle routes ask of their nb branches: one relationship set for every hop, read as (start, end),
// and one node filter for every position.  Fills v0 with the set's views and returns the filter's bitmap; null
// says "not this route" (a bitmap with an id in two scanned rows comes back null too: node_bitmap).
capsmi_bitmap* one_set_one_filter(capsmi_session* s, const Path* B, const Classified* cls, size_t nb, int64_t lo,
                                  int64_t hi, BitmapSet& bs, RelViews& v0) {
    rel_views(B[0], directed(B[0].hops[0]), v0);
    for (size_t bi = 0; bi < nb; ++bi)
        for (const Hop& hp : B[bi].hops) {
            RelViews v;
            rel_views(B[bi], directed(hp), v);
            if (v.sig != v0.sig) return nullptr;
        }
    std::string k0;
    capsmi_bitmap* a = node_bitmap(s, B[0], cls[0], B[0].pos_node[0], lo, hi, bs, &k0);
    if (!a) return nullptr;
    for (size_t bi = 0; bi < nb; ++bi)
        for (int x : B[bi].pos_node) {
            std::string kx;
            if (!node_bitmap(s, B[bi], cls[bi], x, lo, hi, bs, &kx) || kx != k0) return nullptr;
        }
    return a;
}

}  // namespace planning
}  // namespace capsmi
