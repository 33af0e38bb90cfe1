// plan.hip -- lazy Table[T] plans, their operator-by-operator execution, and materialisation.
//
// CAPS's backend sees a MATCH only as the Table[T] calls RelationalPlanner emits
// (okapi-relational/.../planning/RelationalPlanner.scala:113-177): an Expand is
//   join(nodeScan, relScan, (src.id, r.source)) then join(.., nodeScan, (r.target, dst.id)),
// an ExpandInto a 2-key join, a BoundedVarLengthExpand a union of unrolled join chains with
// isomorphism filters (VarLengthExpandPlanner.scala:46-310), followed by Filter (uniqueness
// NOT(r_i = r_j), node predicates) and Aggregate (RelationalOperator.scala:293-351).  DataFrameTable
// builds a lazy Spark plan from those calls and runs it at the first action (SparkTable.scala:59).
// libcapsmi does the same: every Table operator returns a lazy table (schema known, rows not yet
// computed); materialisation first matches the plan against the shapes the fused kernels compute (the recogniser,
// plan_match.hip; the routes and their table, plan_routes.hip) over registered entity tables (capsmi_node_table /
// capsmi_rel_table, plan_entity.hip), and otherwise runs the operators one by one (api.hip eager_*), pruned as
// Catalyst would (below).
#include "plan_impl.h"

namespace capsmi {
namespace planning {

void need(const void* p, const char* what) {
    REQUIRE(p != nullptr, CAPSMI_ERR_ILLEGAL_ARGUMENT, std::string("null argument: ") + what);
}

void check(capsmi_status st) {
    if (st != CAPSMI_OK) throw Error(st, last_error_string());
}

int find_col(const capsmi_table* t, const std::string& name) {
    for (size_t i = 0; i < t->cols.size(); ++i)
        if (t->cols[i].name == name) return (int)i;
    return -1;
}

int col_of(const capsmi_table* t, const char* name) {
    need(name, "column name");
    const int i = find_col(t, name);
    REQUIRE(i >= 0, CAPSMI_ERR_ILLEGAL_ARGUMENT, std::string("no column named '") + name + "'");
    return i;
}

namespace {

Column schema_col(const std::string& name, int32_t type, bool nullable) {
    Column c;
    c.name = name;
    c.type = type;
    c.lazy_nullable = nullable;
    return c;
}

Column schema_of(const Column& c) { return schema_col(c.name, c.type, c.nullable()); }

// an input of a plan node: retained here, released by ~PlanNode (also when the builder throws)
void hold(PlanNode& p, capsmi_table* t) {
    t->refs.fetch_add(1);
    p.in.push_back(t);
}

// a lazy table over node `p` (inputs already held)
capsmi_table* lazy_table(capsmi_session* s, std::shared_ptr<PlanNode> p, std::vector<Column> schema) {
    auto* t = new capsmi_table();
    t->sess = s;
    t->nrows = -1;
    t->cols = std::move(schema);
    t->plan = std::move(p);
    return t;
}

std::vector<const char*> cstrs(const std::vector<std::string>& v) {
    std::vector<const char*> o;
    for (auto& x : v) o.push_back(x.c_str());
    return o;
}

}  // namespace

// A WITH_COLUMNS node with a CAPSMI_X_ROW_ID program (include/capsmi.h): Catalyst's nondeterministic expression.
// The recogniser never takes it into a pattern, and the pruned executor computes it whole, once, in place.
bool pinned(const capsmi_table* t) {
    if (!t->lazy() || t->plan->kind != PlanNode::WITH_COLUMNS) return false;
    for (const auto& prog : t->plan->progs)
        if (has_row_id((int32_t)prog.size(), prog.data())) return true;
    return false;
}

namespace {

// ============================ operator-by-operator execution ===============================
capsmi_table* exec_node(const PlanNode& p) {
    capsmi_table* r = nullptr;
    capsmi_table* x = p.in.empty() ? nullptr : p.in[0];
    switch (p.kind) {
        case PlanNode::SELECT: { auto c = cstrs(p.a); check(eager_select(x, (int)c.size(), c.data(), &r)); break; }
        case PlanNode::DROP: { auto c = cstrs(p.a); check(eager_drop(x, (int)c.size(), c.data(), &r)); break; }
        case PlanNode::RENAME: check(eager_with_column_renamed(x, p.a[0].c_str(), p.b[0].c_str(), &r)); break;
        case PlanNode::FILTER: check(eager_filter(x, (int)p.progs[0].size(), p.progs[0].data(), &r)); break;
        case PlanNode::WITH_COLUMNS: {
            std::vector<capsmi_expr_column> cols(p.a.size());
            for (size_t i = 0; i < p.a.size(); ++i) {
                cols[i].name = p.a[i].c_str();
                cols[i].nnodes = (int32_t)p.progs[i].size();
                cols[i].prog = p.progs[i].data();
            }
            check(eager_with_columns(x, (int)cols.size(), cols.data(), &r));
            break;
        }
        case PlanNode::JOIN: {
            auto l = cstrs(p.a), rr = cstrs(p.b);
            check(eager_join(x, p.in[1], p.jt, (int)l.size(), l.data(), rr.data(), &r));
            break;
        }
        case PlanNode::UNION: check(eager_union_all(x, p.in[1], &r)); break;
        case PlanNode::DISTINCT: check(eager_distinct(x, &r)); break;
        case PlanNode::DISTINCT_ON: { auto c = cstrs(p.a); check(eager_distinct_on(x, (int)c.size(), c.data(), &r)); break; }
        case PlanNode::GROUP: {
            auto by = cstrs(p.a);
            std::vector<capsmi_agg> ag(p.aggs.size());
            for (size_t i = 0; i < p.aggs.size(); ++i) {
                ag[i].kind = p.aggs[i].kind;
                ag[i].distinct = p.aggs[i].distinct;
                ag[i].input = p.aggs[i].input.empty() ? nullptr : p.aggs[i].input.c_str();
                ag[i].output = p.aggs[i].output.c_str();
            }
            check(eager_group(x, (int)by.size(), by.data(), (int)ag.size(), ag.data(), &r));
            break;
        }
        case PlanNode::ORDER: { auto c = cstrs(p.a); check(eager_order_by(x, (int)c.size(), c.data(), p.flags.data(), &r)); break; }
        case PlanNode::SKIP: check(eager_skip(x, p.n, &r)); break;
        case PlanNode::LIMIT: check(eager_limit(x, p.n, &r)); break;
        case PlanNode::EXPLODE:
            if (p.a.empty()) check(eager_explode_values(x, p.jt, (int32_t)p.n, p.vals.data(), p.b[0].c_str(), nullptr, &r));
            else check(eager_explode(x, p.a[0].c_str(), p.b[0].c_str(), nullptr, &r));
            break;
        case PlanNode::RANGE: check(eager_with_range_column(x, p.progs[0], p.progs[1], p.progs[2], p.a[0].c_str(), &r)); break;
        case PlanNode::MASK_LIST: check(eager_with_mask_list_column(x, p.jt, p.b, p.codes, p.a[0].c_str(), &r)); break;
    }
    return r;
}

// move a materialised result into the lazy table `t` (names from t's schema)
void adopt(capsmi_table* t, capsmi_table* r) {
    std::unique_ptr<capsmi_table> g(r);
    REQUIRE(r->cols.size() == t->cols.size(), CAPSMI_ERR_INTERNAL, "materialised schema differs from the plan's");
    for (size_t i = 0; i < r->cols.size(); ++i) r->cols[i].name = t->cols[i].name;
    t->cols = std::move(r->cols);
    t->nrows = r->nrows;
}

}  // namespace

capsmi_status build(capsmi_table* t, capsmi_table** out, const std::function<capsmi_table*()>& f) {
    P_BEGIN
    need(t, "table");
    need(out, "out");
    *out = f();
    P_END
}

// ============================ operator-by-operator execution, pruned ========================
// What Catalyst does to the DataFrame plan DataFrameTable builds before Spark runs it (the optimiser
// rules ColumnPruning and PushDownPredicate / PushPredicateThroughJoin): a plan that is not routed
// to a fused kernel executes with
//   - every Filter split into its conjuncts, each pushed below Select / Drop / WithColumnRenamed /
//     WithColumns (when it does not read a column they add) and into the side of a Join whose columns
//     it reads (inner and cross: either side; one-sided outer: the preserved side only), and applied
//     where it stops -- with the rows of only the columns still needed gathered;
//   - only the columns some operator above still reads computed and gathered (join outputs, filters,
//     WithColumns expressions nobody reads are skipped).
// Results are the same rows (conjunct order does not change a TRUE / not-TRUE filter under 3VL);
// columns are matched by name, and put back in schema order where position matters (union inputs,
// the materialised table).
// A sub-plan with two parents in the plan DAG is materialised once in place and shared.
// A WITH_COLUMNS node with a CAPSMI_X_ROW_ID program is pinned (Catalyst keeps a nondeterministic expression where
// the query put it): it too is materialised in place when first reached, whole -- every column, no conjunct pushed
// below it, its input planned as usual -- and keeps its rows, so a later reader, in this action or another, sees
// the ids the first one saw.

namespace {

using Names = std::vector<std::string>;  // ordered, unique column names

bool has(const Names& v, const std::string& x) { return std::find(v.begin(), v.end(), x) != v.end(); }
void add(Names& v, const std::string& x) {
    if (!has(v, x)) v.push_back(x);
}

struct Pred {                     // one conjunct; COL args index `names`
    std::vector<capsmi_expr> prog;
    Names names;
};

// the conjuncts of prog[lo .. hi], nested ANDs flattened, in the program's order
void conjuncts(const std::vector<capsmi_expr>& prog, int lo, int hi, std::vector<std::vector<capsmi_expr>>& out) {
    if (prog[hi].op == CAPSMI_X_AND) {
        for (const auto& kid : operand_spans(prog.data(), hi)) conjuncts(prog, kid.first, kid.second, out);
    } else {
        out.emplace_back(prog.begin() + lo, prog.begin() + hi + 1);
    }
}

Pred to_pred(const std::vector<capsmi_expr>& prog, const capsmi_table* schema) {
    Pred p;
    p.prog = prog;
    for (capsmi_expr& x : p.prog)
        if (x.op == CAPSMI_X_COL) {
            const std::string& n = schema->cols.at(x.arg).name;
            add(p.names, n);
            x.arg = (int32_t)(std::find(p.names.begin(), p.names.end(), n) - p.names.begin());
        }
    return p;
}

// a program over `from`'s columns re-indexed against `to` (by name)
std::vector<capsmi_expr> remap(std::vector<capsmi_expr> prog, const capsmi_table* from, const capsmi_table* to) {
    for (capsmi_expr& x : prog)
        if (x.op == CAPSMI_X_COL) x.arg = col_of(to, from->cols.at(x.arg).name.c_str());
    return prog;
}

struct Res {  // an operator's result: a table this executor owns, or a borrowed materialised input
    capsmi_table* t = nullptr;
    bool owned = false;
    Res() = default;
    Res(capsmi_table* x, bool o) : t(x), owned(o) {}
    Res(Res&& o) noexcept : t(o.t), owned(o.owned) { o.t = nullptr; }
    Res& operator=(Res&& o) noexcept {
        if (this != &o) {
            reset();
            t = o.t;
            owned = o.owned;
            o.t = nullptr;
        }
        return *this;
    }
    ~Res() { reset(); }
    void reset() {
        if (t && owned) capsmi_table_release(t);
        t = nullptr;
    }
};

Res owned(capsmi_table* t) { return Res(t, true); }

// apply the pending conjuncts, keep exactly `need` (in the table's order)
Res finish(Res r, const Names& need, const std::vector<Pred>& preds) {
    Names keep;
    for (const Column& c : r.t->cols)
        if (has(need, c.name)) keep.push_back(c.name);
    REQUIRE(keep.size() == need.size(), CAPSMI_ERR_INTERNAL, "pruned plan lost a column");
    capsmi_table* o = nullptr;
    if (!preds.empty()) {
        std::vector<capsmi_expr> prog;
        for (const Pred& p : preds)
            for (capsmi_expr x : p.prog) {
                if (x.op == CAPSMI_X_COL) x.arg = col_of(r.t, p.names.at(x.arg).c_str());
                prog.push_back(x);
            }
        if (preds.size() > 1) {
            capsmi_expr a{};
            a.op = CAPSMI_X_AND;
            a.arg = (int32_t)preds.size();
            prog.push_back(a);
        }
        check(eager_filter_keep(r.t, (int32_t)prog.size(), prog.data(), keep, &o));
        o->partitioned = r.t->partitioned;
        return owned(o);
    }
    if (keep.size() == r.t->cols.size()) return r;
    auto c = cstrs(keep);
    check(eager_select(r.t, (int32_t)c.size(), c.data(), &o));
    o->partitioned = r.t->partitioned;
    return owned(o);
}

// ---- Exchanges of the generic operators over a distributed result ------------------------------------
// A row-local operator keeps its input's partitioning.  An operator that needs rows of other ranks gets
// the Exchange Spark's planner would insert (SparkTable.scala:133 groupBy, :226 join; CAPSSession.scala:
// 118-119 partitions), built on the session's collective (k_dist.hip exchange_rows):
//   join: a broadcast join when one side is whole on every rank and the partitioned side is the one whose
//     rows the join type preserves (inner, cross, left outer with the left partitioned, right outer with the
//     right partitioned); else both sides hash-partitioned on the join keys (a whole side first takes its
//     slice; rows with a null key stay where they are: they match nothing).  The result is partitioned.
//   grouping with keys, distinct: hash-partitioned on the grouping / distinct columns (nulls form one
//     group), then the local operator: the result is partitioned (each group on one rank).
//   a global aggregate, order by, skip, limit: every rank's rows gathered (all-gather), then the local
//     operator: the result is whole on every rank.
//   union all of a partitioned and a whole input: the whole one takes its slice.
// String keys hash their dictionary codes: the ranks of a distributed graph share one dictionary (the same
// ingest on every rank, as the JVM shim's session-wide dictionary).
Res owned(capsmi_table* t);

std::vector<int> key_indices(const capsmi_table* t, const Names& cols) {
    std::vector<int> k;
    for (const std::string& c : cols) k.push_back(col_of(t, c.c_str()));
    return k;
}

// join inputs made co-partitioned (see above); false when neither side is partitioned
bool dist_join_inputs(capsmi_session* s, int jt, const Names& lk, const Names& rk, Res& a, Res& b) {
    const bool pa = a.t->partitioned, pb = b.t->partitioned;
    if (!pa && !pb) return false;
    if (jt == CAPSMI_JOIN_CROSS) {
        if (pa && pb) b = owned(gather_rows(s, b.t));  // broadcast the right side
        return true;
    }
    if ((jt == CAPSMI_JOIN_INNER && (!pa || !pb)) || (jt == CAPSMI_JOIN_LEFT_OUTER && pa && !pb) ||
        (jt == CAPSMI_JOIN_RIGHT_OUTER && !pa && pb))
        return true;  // broadcast join: the whole side is on every rank
    if (!pa) a = owned(slice_rows(s, a.t));
    if (!pb) b = owned(slice_rows(s, b.t));
    const std::vector<int> li = key_indices(a.t, lk), ri = key_indices(b.t, rk);
    std::vector<int> lf(li.size(), 0), rf(ri.size(), 0);
    for (size_t i = 0; i < li.size(); ++i) {  // a Long key joined with a Double key hashes as the double
        const int32_t x = a.t->cols[li[i]].type, y = b.t->cols[ri[i]].type;
        if (x == CAPSMI_F64 || y == CAPSMI_F64) {
            lf[i] = x == CAPSMI_F64 ? 2 : 1;
            rf[i] = y == CAPSMI_F64 ? 2 : 1;
        }
    }
    a = owned(exchange_by_keys(s, a.t, li, lf, true));
    b = owned(exchange_by_keys(s, b.t, ri, rf, true));
    return true;
}

// ---- unrouted-plan size guard (capsmi_session_set_unrouted_limit) ------------------------------------
// System-R estimates of a lazy plan's rows: a join emits |L| |R| / max(ndv(l), ndv(r)) rows, where the
// ndv of an entity key column is its scan's rows (node ids) or min(rows, id window) (endpoints).
double key_ndv(const capsmi_table* t, const std::string& col) {  // -1: not known (not an entity key)
    Scan sc;
    const int c = find_col(t, col);
    if (c < 0 || !as_scan(t, sc)) return -1;
    double n = 0, span = 0;
    for (const Member& m : sc.m) {
        n += (double)m.base->nrows;
        span = std::max(span, (double)(m.base->entity->hi - m.base->entity->lo));
    }
    if (sc.role[c] == ROLE_ID) return std::max(1.0, n);
    if (sc.role[c] == ROLE_SRC || sc.role[c] == ROLE_DST) return std::max(1.0, std::min(n, span));
    return -1;
}

double est_rows(const capsmi_table* t) {
    if (!t->lazy()) return (double)t->nrows;
    const PlanNode& p = *t->plan;
    switch (p.kind) {
        case PlanNode::UNION: return est_rows(p.in[0]) + est_rows(p.in[1]);
        case PlanNode::SKIP: return std::max(0.0, est_rows(p.in[0]) - (double)p.n);
        case PlanNode::LIMIT: return std::min((double)p.n, est_rows(p.in[0]));
        case PlanNode::JOIN: {
            const double l = est_rows(p.in[0]), r = est_rows(p.in[1]);
            if (p.jt == CAPSMI_JOIN_CROSS) return l * r;
            double ndv = -1;  // the larger known key cardinality (an intermediate result's keys: unknown)
            for (size_t i = 0; i < p.a.size(); ++i)
                ndv = std::max(ndv, std::max(key_ndv(p.in[0], p.a[i]), key_ndv(p.in[1], p.b[i])));
            if (ndv < 1) ndv = std::max(1.0, std::max(l, r));
            double e = l * r / ndv;
            if (p.jt == CAPSMI_JOIN_LEFT_OUTER || p.jt == CAPSMI_JOIN_FULL_OUTER) e = std::max(e, l);
            if (p.jt == CAPSMI_JOIN_RIGHT_OUTER || p.jt == CAPSMI_JOIN_FULL_OUTER) e = std::max(e, r);
            return e;
        }
        default: return est_rows(p.in[0]);
    }
}

void guard_join(const capsmi_table* t) {
    const int64_t limit = t->sess->unrouted_limit;
    if (limit <= 0) return;
    const double bytes = est_rows(t) * (double)t->cols.size() * 9.0;  // 8-B words + validity bytes
    REQUIRE(bytes <= (double)limit, CAPSMI_ERR_UNSUPPORTED,
            "unrouted join estimated at " + std::to_string((long long)(bytes / 1e9)) + " GB (" +
                std::to_string((long long)est_rows(t)) + " rows) exceeds the session limit of " +
                std::to_string((long long)(limit / 1000000000LL)) + " GB; no fused route matched this pattern");
}

using Parents = std::map<const capsmi_table*, int>;

void count_parents(const capsmi_table* t, Parents& par) {
    if (!t->lazy()) return;
    for (const capsmi_table* x : t->plan->in)
        if (++par[x] == 1) count_parents(x, par);
}

Names all_names(const capsmi_table* t) {
    Names v;
    for (const Column& c : t->cols) v.push_back(c.name);
    return v;
}

// The input `x` of a MASK_LIST node when it is a pattern and `need` holds label or property columns of its
// nodes (labels(b) above MATCH (a)-[r]->(b)).  The fused routes carry relationship columns, endpoint ids and
// constants, not node columns, so the pattern is projected on the rest of `need` plus the ids of the nodes in
// question, that projection takes whatever fused route it matches, and the node columns are joined back by id
// from the members of the node scans the pattern names (a base column or the member's constant).  *out then
// holds `need` and helper columns, in any row order.  false: no route matched and nothing was run.
bool expand_with_node_columns(capsmi_table* x, const Names& need, const Parents& par, capsmi_table** out) {
    capsmi_session* s = x->sess;
    if (!x->lazy() || !s->fused) return false;
    auto shared = par.find(x);
    if (shared != par.end() && shared->second > 1) return false;  // a shared sub-plan materialises once, in place
    std::vector<Path> B;
    if (!as_paths(x, B) || B.size() != 1 || B[0].cols.size() != x->cols.size()) return false;
    const Path& P = B[0];
    for (const Scan& sc : P.inst)
        for (const Member& m : sc.m)
            if (m.base->shard) return false;  // a distributed graph: the generic plan and its exchanges
    Names proj;
    std::map<int, std::vector<int>> fetch;  // node scan instance -> the columns of x to join back
    for (const std::string& n : need) {
        const int i = find_col(x, n);
        if (i < 0) return false;
        const Role& r = P.cols[i];
        if (r.k == RK_NODE && P.inst[r.inst].role[r.scol] != ROLE_ID) fetch[r.inst].push_back(i);
        else add(proj, n);
    }
    if (fetch.empty()) return false;
    std::map<int, std::string> id_of;
    for (const auto& f : fetch) {
        for (size_t j = 0; j < P.cols.size() && !id_of.count(f.first); ++j) {
            const Role& r = P.cols[j];
            if (r.k == RK_NODE && r.inst == f.first && P.inst[r.inst].role[r.scol] == ROLE_ID) id_of[f.first] = x->cols[j].name;
        }
        if (!id_of.count(f.first)) return false;
        add(proj, id_of[f.first]);
    }
    Res acc;
    {
        capsmi_table* sel = nullptr;
        auto pc = cstrs(proj);
        check(capsmi_select(x, (int32_t)pc.size(), pc.data(), &sel));
        Res selr = owned(sel);
        capsmi_table* fr = nullptr;
        if (!try_fused_shapes(sel, &fr)) return false;
        acc = owned(fr);
        REQUIRE(fr->cols.size() == sel->cols.size(), CAPSMI_ERR_INTERNAL, "fused result schema differs from the plan's");
        for (size_t i = 0; i < fr->cols.size(); ++i) fr->cols[i].name = sel->cols[i].name;
    }
    int q = 0;
    for (const auto& f : fetch) {
        const std::string key = "__node_id" + std::to_string(q++);
        Names names{key};
        for (int c : f.second) names.push_back(x->cols[c].name);
        Res nodes;
        for (const Member& m : P.inst[f.first].m) {
            std::vector<capsmi_expr> progs(names.size());
            progs[0].op = CAPSMI_X_COL;
            progs[0].arg = m.base->entity->id;
            for (size_t k = 0; k < f.second.size(); ++k) {
                const int sc = P.cols[f.second[k]].scol;
                if (m.src[sc] >= 0) {
                    progs[k + 1].op = CAPSMI_X_COL;
                    progs[k + 1].arg = m.src[sc];
                } else {
                    progs[k + 1] = m.cst[sc];  // the member's constant: a label flag, a property it lacks
                }
            }
            std::vector<capsmi_expr_column> cols(names.size());
            for (size_t k = 0; k < names.size(); ++k) {
                cols[k].name = names[k].c_str();
                cols[k].nnodes = 1;
                cols[k].prog = &progs[k];
            }
            capsmi_table* w = nullptr;
            check(eager_with_columns(m.base, (int32_t)cols.size(), cols.data(), &w));
            Res wr = owned(w);
            capsmi_table* part = nullptr;
            auto nc = cstrs(names);
            check(eager_select(w, (int32_t)nc.size(), nc.data(), &part));
            Res pr = owned(part);
            if (!nodes.t) {
                nodes = std::move(pr);
            } else {
                capsmi_table* u = nullptr;
                check(eager_union_all(nodes.t, part, &u));
                nodes = owned(u);
            }
        }
        REQUIRE(nodes.t != nullptr, CAPSMI_ERR_INTERNAL, "node scan without members");
        const char* lk[1] = {id_of[f.first].c_str()};
        const char* rk[1] = {key.c_str()};
        capsmi_table* j = nullptr;
        check(eager_join(acc.t, nodes.t, CAPSMI_JOIN_INNER, 1, lk, rk, &j));
        acc = owned(j);
    }
    *out = acc.t;
    acc.t = nullptr;
    return true;
}

Res exec(capsmi_table* t, const Names& need, std::vector<Pred> preds, const Parents& par, bool root = false) {
    if (t->lazy()) {
        auto it = par.find(t);
        if (it != par.end() && it->second > 1) materialize(t);  // shared sub-plan: once, in place
        // a pinned node (CAPSMI_X_ROW_ID): whole, once, in place -- every column, no conjunct below it, and the rows
        // stay with `t` for this action's other readers and for later actions.  (As the root of materialize it is
        // being computed just so: `need` is every column and there are no conjuncts.)
        else if (!root && pinned(t)) materialize(t);
    }
    if (!t->lazy()) return finish(Res(t, false), need, preds);
    capsmi_table* fr = nullptr;
    if (try_fused(t, &fr)) {
        REQUIRE(fr->cols.size() == t->cols.size(), CAPSMI_ERR_INTERNAL, "fused result schema differs from the plan's");
        for (size_t i = 0; i < fr->cols.size(); ++i) fr->cols[i].name = t->cols[i].name;
        return finish(owned(fr), need, preds);
    }
    std::shared_ptr<PlanNode> keep_alive = t->plan;
    const PlanNode& p = *keep_alive;
    capsmi_table* x = p.in.empty() ? nullptr : p.in[0];
    switch (p.kind) {
        case PlanNode::FILTER: {
            std::vector<std::vector<capsmi_expr>> cs;
            if (!p.progs[0].empty()) conjuncts(p.progs[0], 0, (int)p.progs[0].size() - 1, cs);
            for (auto& c : cs) preds.push_back(to_pred(c, x));
            return exec(x, need, std::move(preds), par);
        }
        case PlanNode::SELECT:
        case PlanNode::DROP:
            return exec(x, need, std::move(preds), par);
        case PlanNode::RENAME: {
            const std::string &a = p.a[0], &b = p.b[0];
            if (a == b) return exec(x, need, std::move(preds), par);
            Names nin;
            for (const std::string& n : need) nin.push_back(n == b ? a : n);
            for (Pred& pr : preds)
                for (std::string& n : pr.names)
                    if (n == b) n = a;
            Res r = exec(x, nin, std::move(preds), par);
            if (r.t->find(a) < 0) return r;
            capsmi_table* o = nullptr;
            check(eager_with_column_renamed(r.t, a.c_str(), b.c_str(), &o));
            o->partitioned = r.t->partitioned;
            return owned(o);
        }
        case PlanNode::WITH_COLUMNS: {
            std::vector<Pred> down, stay;
            for (Pred& pr : preds) {
                bool reads_new = false;
                for (const std::string& n : pr.names) reads_new |= has(p.a, n);
                (reads_new ? stay : down).push_back(std::move(pr));
            }
            Names out = need;
            for (const Pred& pr : stay)
                for (const std::string& n : pr.names) add(out, n);
            Names nin;
            std::vector<size_t> comp;
            for (const std::string& n : out)
                if (!has(p.a, n)) add(nin, n);
            for (size_t i = 0; i < p.a.size(); ++i) {
                if (!has(out, p.a[i])) continue;  // nobody reads it
                comp.push_back(i);
                for (const capsmi_expr& e : p.progs[i])
                    if (e.op == CAPSMI_X_COL) add(nin, x->cols.at(e.arg).name);
            }
            Res r = exec(x, nin, std::move(down), par);
            if (!comp.empty()) {
                std::vector<std::vector<capsmi_expr>> progs;
                for (size_t i : comp) progs.push_back(remap(p.progs[i], x, r.t));
                std::vector<capsmi_expr_column> cols(comp.size());
                for (size_t k = 0; k < comp.size(); ++k) {
                    cols[k].name = p.a[comp[k]].c_str();
                    cols[k].nnodes = (int32_t)progs[k].size();
                    cols[k].prog = progs[k].data();
                }
                capsmi_table* o = nullptr;
                check(eager_with_columns(r.t, (int32_t)cols.size(), cols.data(), &o));
                o->partitioned = r.t->partitioned;
                r = owned(o);
            }
            return finish(std::move(r), need, stay);
        }
        case PlanNode::JOIN: {
            capsmi_table* y = p.in[1];
            const Names L = all_names(x), R = all_names(y);
            const bool cross = p.jt == CAPSMI_JOIN_CROSS;
            const bool to_l = p.jt == CAPSMI_JOIN_INNER || cross || p.jt == CAPSMI_JOIN_LEFT_OUTER;
            const bool to_r = p.jt == CAPSMI_JOIN_INNER || cross || p.jt == CAPSMI_JOIN_RIGHT_OUTER;
            std::vector<Pred> pl, pr, stay;
            for (Pred& q : preds) {
                bool in_l = true, in_r = true;
                for (const std::string& n : q.names) {
                    in_l &= has(L, n);
                    in_r &= has(R, n);
                }
                if (to_l && in_l) pl.push_back(std::move(q));
                else if (to_r && in_r) pr.push_back(std::move(q));
                else stay.push_back(std::move(q));
            }
            Names out = need;
            for (const Pred& q : stay)
                for (const std::string& n : q.names) add(out, n);
            Names nl, nr;
            for (const std::string& n : out) add(has(L, n) ? nl : nr, n);
            for (const std::string& n : p.a) add(nl, n);
            for (const std::string& n : p.b) add(nr, n);
            guard_join(t);
            Res a = exec(x, nl, std::move(pl), par);
            Res b = exec(y, nr, std::move(pr), par);
            const bool part = dist_join_inputs(t->sess, p.jt, p.a, p.b, a, b);
            auto lk = cstrs(p.a), rk = cstrs(p.b);
            capsmi_table* o = nullptr;
            check(eager_join(a.t, b.t, p.jt, (int32_t)lk.size(), lk.data(), rk.data(), &o));
            o->partitioned = part;
            a.reset();
            b.reset();
            return finish(owned(o), need, stay);
        }
        case PlanNode::EXPLODE: {
            // row-local: a conjunct that reads the item stays above, the others run on the input rows (fewer
            // rows to expand); only the payload columns somebody above reads are gathered
            const std::string& item = p.b[0];
            std::vector<Pred> down, stay;
            for (Pred& pr : preds) (has(pr.names, item) ? stay : down).push_back(std::move(pr));
            Names out = need;
            for (const Pred& pr : stay)
                for (const std::string& n : pr.names) add(out, n);
            Names nin;
            if (!p.a.empty()) add(nin, p.a[0]);
            for (const std::string& n : out)
                if (n != item) add(nin, n);
            if (nin.empty() && !x->cols.empty()) add(nin, x->cols[0].name);  // the row count travels with a column
            Res r = exec(x, nin, std::move(down), par);
            capsmi_table* o = nullptr;
            if (p.a.empty())
                check(eager_explode_values(r.t, p.jt, (int32_t)p.n, p.vals.data(), item.c_str(), &out, &o));
            else
                check(eager_explode(r.t, p.a[0].c_str(), item.c_str(), &out, &o));
            o->partitioned = r.t->partitioned;  // no exchange: a rank's rows explode where they are
            r.reset();
            return finish(owned(o), need, stay);
        }
        case PlanNode::RANGE: {
            // row-local, like WITH_COLUMNS: a conjunct that reads the new column stays above, the others run on
            // the input rows; the input keeps the columns somebody above or an operand program reads
            const std::string& name = p.a[0];
            std::vector<Pred> down, stay;
            for (Pred& pr : preds) (has(pr.names, name) ? stay : down).push_back(std::move(pr));
            Names out = need;
            for (const Pred& pr : stay)
                for (const std::string& n : pr.names) add(out, n);
            Names nin;
            for (const std::string& n : out)
                if (n != name) add(nin, n);
            for (const auto& prog : p.progs)
                for (const capsmi_expr& e : prog)
                    if (e.op == CAPSMI_X_COL) add(nin, x->cols.at(e.arg).name);
            if (nin.empty() && !x->cols.empty()) add(nin, x->cols[0].name);  // the row count travels with a column
            Res r = exec(x, nin, std::move(down), par);
            capsmi_table* o = nullptr;
            check(eager_with_range_column(r.t, remap(p.progs[0], x, r.t), remap(p.progs[1], x, r.t),
                                          remap(p.progs[2], x, r.t), name.c_str(), &o));
            o->partitioned = r.t->partitioned;  // no exchange
            r.reset();
            return finish(owned(o), need, stay);
        }
        case PlanNode::MASK_LIST: {
            // row-local, as RANGE: a conjunct that reads the new column stays above, the others run on the input
            // rows; the input keeps the columns somebody above reads plus the mask's
            const std::string& name = p.a[0];
            std::vector<Pred> down, stay;
            for (Pred& pr : preds) (has(pr.names, name) ? stay : down).push_back(std::move(pr));
            Names out = need;
            for (const Pred& pr : stay)
                for (const std::string& n : pr.names) add(out, n);
            Names nin;
            for (const std::string& n : out)
                if (n != name) add(nin, n);
            for (const std::string& n : p.b) add(nin, n);
            if (nin.empty() && !x->cols.empty()) add(nin, x->cols[0].name);  // the row count travels with a column
            Res r;
            capsmi_table* routed = nullptr;
            if (down.empty() && expand_with_node_columns(x, nin, par, &routed)) r = owned(routed);
            else r = exec(x, nin, std::move(down), par);
            capsmi_table* o = nullptr;
            check(eager_with_mask_list_column(r.t, p.jt, p.b, p.codes, name.c_str(), &o));
            o->partitioned = r.t->partitioned;  // no exchange
            r.reset();
            return finish(owned(o), need, stay);
        }
        default: {  // union, distinct, grouping, ordering, skip / limit: conjuncts stay above
            std::vector<Names> nin(p.in.size());
            for (size_t i = 0; i < p.in.size(); ++i) nin[i] = all_names(p.in[i]);
            if (p.kind == PlanNode::GROUP) {
                Names v = p.a;
                for (const AggSpec& ag : p.aggs)
                    if (!ag.input.empty()) add(v, ag.input);
                nin[0] = v;
            } else if (p.kind == PlanNode::ORDER || p.kind == PlanNode::SKIP || p.kind == PlanNode::LIMIT) {
                Names v = need;
                for (const std::string& n : p.a) add(v, n);
                for (const Pred& q : preds)
                    for (const std::string& n : q.names) add(v, n);
                nin[0] = v;
            }
            PlanNode run;  // the same operator over the pruned inputs
            run.kind = p.kind;
            run.a = p.a;
            run.b = p.b;
            run.progs = p.progs;
            run.flags = p.flags;
            run.aggs = p.aggs;
            run.jt = p.jt;
            run.n = p.n;
            run.codes = p.codes;
            bool part = false;
            std::vector<Res> ins;
            for (size_t i = 0; i < p.in.size(); ++i) {
                Res r = exec(p.in[i], nin[i], {}, par);
                if (r.t->partitioned && p.kind != PlanNode::UNION) {  // the Exchange this operator needs
                    capsmi_session* ss = t->sess;
                    if ((p.kind == PlanNode::GROUP && !p.a.empty()) || p.kind == PlanNode::DISTINCT_ON) {
                        r = owned(exchange_by_keys(ss, r.t, key_indices(r.t, p.a), {}, false));
                    } else if (p.kind == PlanNode::DISTINCT) {
                        std::vector<int> all(r.t->cols.size());
                        for (size_t k = 0; k < all.size(); ++k) all[k] = (int)k;
                        r = owned(exchange_by_keys(ss, r.t, all, {}, false));
                    } else {  // global aggregate, order by, skip, limit: every rank's rows
                        r = owned(gather_rows(ss, r.t));
                    }
                }
                part = part || r.t->partitioned;
                if (p.kind == PlanNode::UNION) {  // positional: the input's schema order
                    capsmi_table* o = nullptr;
                    auto c = cstrs(nin[i]);
                    check(eager_select(r.t, (int32_t)c.size(), c.data(), &o));
                    o->partitioned = r.t->partitioned;
                    r = owned(o);
                }
                ins.push_back(std::move(r));
            }
            if (p.kind == PlanNode::UNION && part)  // a whole input joins a partitioned one by its slice
                for (Res& r : ins)
                    if (!r.t->partitioned) r = owned(slice_rows(t->sess, r.t));
            for (Res& r : ins) hold(run, r.t);
            ins.clear();
            capsmi_table* o = exec_node(run);
            o->partitioned = part;
            return finish(owned(o), need, preds);
        }
    }
    return Res();
}

}  // namespace
}  // namespace planning

using namespace planning;

// ================================ materialisation ===========================================
void materialize(capsmi_table* t) {
    if (!t || !t->plan) return;
    std::shared_ptr<PlanNode> p = t->plan;  // inputs stay alive while this runs
    Parents par;
    count_parents(t, par);
    const Names all = all_names(t);
    Names uniq;
    for (const std::string& n : all) add(uniq, n);
    capsmi_table* r = nullptr;
    const bool outer_missed = g_missed;  // a shared sub-plan materialises inside another materialisation
    g_missed = false;
    int64_t routed_before = 0;
    for (auto& kv : t->sess->routes) routed_before += kv.first == "miss" ? 0 : kv.second;
    {
        Res e = exec(t, uniq, {}, par, true);
        auto c = cstrs(all);
        check(eager_select(e.t, (int32_t)c.size(), c.data(), &r));  // schema order, an owned table
        r->partitioned = e.t->partitioned;
    }
    int64_t routed_after = 0;
    for (auto& kv : t->sess->routes) routed_after += kv.first == "miss" ? 0 : kv.second;
    if (g_missed && routed_after == routed_before) t->sess->routes["miss"] += 1;  // a pattern ran unrouted
    g_missed = outer_missed;
    const bool part = r->partitioned;
    adopt(t, r);
    t->partitioned = part;
    t->plan.reset();  // the inputs are released unless shared elsewhere
}

}  // namespace capsmi

using namespace capsmi;
using namespace capsmi::planning;

// ===================================== C ABI ====================================================
extern "C" {

capsmi_status capsmi_cache(capsmi_table* t, capsmi_table** out) {
    // a table keeps its rows once computed (DataFrameTable.cache, SparkTable.scala:240-246): same handle;
    // a cached relationship table also keeps the fused layouts built from it
    return build(t, out, [&] {
        t->keep_layouts = true;
        t->refs.fetch_add(1);
        return t;
    });
}

capsmi_status capsmi_select(capsmi_table* t, int32_t ncols, const char* const* cols, capsmi_table** out) {
    return build(t, out, [&] {
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::SELECT;
        hold(*p, t);
        std::vector<Column> sch;
        for (int i = 0; i < ncols; ++i) {
            sch.push_back(schema_of(t->cols[col_of(t, cols[i])]));
            p->a.push_back(cols[i]);
        }
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_drop(capsmi_table* t, int32_t ncols, const char* const* cols, capsmi_table** out) {
    return build(t, out, [&] {
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::DROP;
        hold(*p, t);
        std::set<std::string> d;
        for (int i = 0; i < ncols; ++i) {
            need(cols[i], "column name");
            d.insert(cols[i]);  // Spark drop ignores unknown names
            p->a.push_back(cols[i]);
        }
        std::vector<Column> sch;
        for (auto& c : t->cols) if (!d.count(c.name)) sch.push_back(schema_of(c));
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_with_column_renamed(capsmi_table* t, const char* old_name, const char* new_name, capsmi_table** out) {
    return build(t, out, [&] {
        need(new_name, "new name");
        const int i = col_of(t, old_name);
        const int j = find_col(t, new_name);
        REQUIRE(j < 0 || j == i, CAPSMI_ERR_ILLEGAL_ARGUMENT, std::string("column '") + new_name + "' already exists");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::RENAME;
        hold(*p, t);
        p->a = {old_name};
        p->b = {new_name};
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        sch[i].name = new_name;
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_filter(capsmi_table* t, int32_t nnodes, const capsmi_expr* prog, capsmi_table** out) {
    return build(t, out, [&] {
        REQUIRE(nnodes == 0 || prog, CAPSMI_ERR_ILLEGAL_ARGUMENT, "null program");
        std::vector<capsmi_expr> bound;
        if (has_params(nnodes, prog)) {  // parameters become literals now, as in the Spark plan
            bound = bind_params(t->sess, nnodes, prog);
            prog = bound.data();
            nnodes = (int32_t)bound.size();
        }
        refuse_row_id(nnodes, prog, "a capsmi_filter predicate");
        validate_program(t, nnodes, prog);
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::FILTER;
        hold(*p, t);
        p->progs.emplace_back(prog, prog + nnodes);
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_with_columns(capsmi_table* t, int32_t ncols, const capsmi_expr_column* cols, capsmi_table** out) {
    return build(t, out, [&] {
        REQUIRE(ncols == 0 || cols, CAPSMI_ERR_ILLEGAL_ARGUMENT, "null columns");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::WITH_COLUMNS;
        hold(*p, t);
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        for (int i = 0; i < ncols; ++i) {
            need(cols[i].name, "column name");
            REQUIRE(cols[i].nnodes == 0 || cols[i].prog, CAPSMI_ERR_ILLEGAL_ARGUMENT, "null program");
            std::vector<capsmi_expr> prog(cols[i].prog, cols[i].prog + cols[i].nnodes);
            if (has_params(cols[i].nnodes, cols[i].prog)) prog = bind_params(t->sess, cols[i].nnodes, cols[i].prog);
            REQUIRE(t->sess->world <= 1 || !has_row_id((int32_t)prog.size(), prog.data()), CAPSMI_ERR_UNSUPPORTED,
                    "CAPSMI_X_ROW_ID on a session of " + std::to_string(t->sess->world) +
                        " ranks: distributed CONSTRUCT is not implemented");
            p->a.push_back(cols[i].name);
            Column c = schema_col(cols[i].name, validate_program(t, (int32_t)prog.size(), prog.data()), true);
            p->progs.push_back(std::move(prog));
            int j = -1;
            for (size_t q = 0; q < sch.size(); ++q) if (sch[q].name == c.name) j = (int)q;
            if (j >= 0) sch[j] = c;  // replaced in place (SparkTable.scala:82-87)
            else sch.push_back(c);
        }
        return lazy_table(t->sess, p, sch);
    });
}

// the schema of an exploded table: the input's columns, the item replacing a column of its name, else appended
static std::vector<Column> explode_schema(const capsmi_table* t, const Column& item) {
    std::vector<Column> sch;
    for (auto& c : t->cols) sch.push_back(schema_of(c));
    const int j = find_col(t, item.name);
    if (j >= 0) sch[j] = item;
    else sch.push_back(item);
    return sch;
}

capsmi_status capsmi_explode(capsmi_table* t, const char* list_col, const char* item_name, capsmi_table** out) {
    return build(t, out, [&] {
        need(item_name, "item name");
        const Column& lc = t->cols[col_of(t, list_col)];
        REQUIRE(is_list_type(lc.type), CAPSMI_ERR_ILLEGAL_ARGUMENT, "column '" + lc.name + "' is not a list column");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::EXPLODE;
        hold(*p, t);
        p->a = {lc.name};
        p->b = {item_name};
        return lazy_table(t->sess, p, explode_schema(t, schema_col(item_name, lc.type - CAPSMI_LIST, false)));
    });
}

capsmi_status capsmi_explode_values(capsmi_table* t, int32_t elem_type, int32_t count, const capsmi_value* values,
                                    const char* item_name, capsmi_table** out) {
    return build(t, out, [&] {
        need(item_name, "item name");
        REQUIRE(elem_type >= CAPSMI_I64 && elem_type <= CAPSMI_STR, CAPSMI_ERR_ILLEGAL_ARGUMENT, "bad element type");
        REQUIRE(count >= 0 && (count == 0 || values), CAPSMI_ERR_ILLEGAL_ARGUMENT, "bad value list");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::EXPLODE;
        hold(*p, t);
        p->b = {item_name};
        p->jt = elem_type;
        p->n = count;
        p->vals.assign(values, values + count);
        bool any_null = false;
        for (const capsmi_value& v : p->vals) any_null |= v.is_null != 0;
        return lazy_table(t->sess, p, explode_schema(t, schema_col(item_name, elem_type, any_null)));
    });
}

capsmi_status capsmi_with_range_column(capsmi_table* t, int32_t from_nnodes, const capsmi_expr* from_prog,
                                       int32_t to_nnodes, const capsmi_expr* to_prog, int32_t step_nnodes,
                                       const capsmi_expr* step_prog, const char* name, capsmi_table** out) {
    return build(t, out, [&] {
        need(name, "column name");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::RANGE;
        hold(*p, t);
        p->a = {name};
        const int32_t nn[3] = {from_nnodes, to_nnodes, step_prog ? step_nnodes : 0};
        const capsmi_expr* pr[3] = {from_prog, to_prog, step_prog};
        for (int i = 0; i < 3; ++i) {
            REQUIRE(nn[i] > 0 ? pr[i] != nullptr : i == 2, CAPSMI_ERR_ILLEGAL_ARGUMENT, "range: null or empty operand program");
            std::vector<capsmi_expr> prog(pr[i], pr[i] + nn[i]);
            if (has_params(nn[i], pr[i])) prog = bind_params(t->sess, nn[i], pr[i]);
            refuse_row_id((int32_t)prog.size(), prog.data(), "a capsmi_with_range_column operand");
            REQUIRE(validate_program(t, (int32_t)prog.size(), prog.data()) == CAPSMI_I64,
                    CAPSMI_ERR_ILLEGAL_ARGUMENT, "range: operands must be Long");
            p->progs.push_back(std::move(prog));
        }
        return lazy_table(t->sess, p, explode_schema(t, schema_col(name, CAPSMI_LIST_I64, true)));
    });
}

capsmi_status capsmi_with_mask_list_column(capsmi_table* t, int32_t mode, int32_t ncols, const char* const* cols,
                                           const int64_t* elem_codes, const char* name, capsmi_table** out) {
    return build(t, out, [&] {
        need(name, "column name");
        REQUIRE(mode == CAPSMI_MASK_TRUE || mode == CAPSMI_MASK_NOT_NULL, CAPSMI_ERR_ILLEGAL_ARGUMENT, "mask list: mode");
        REQUIRE(ncols >= 0 && (ncols == 0 || (cols && elem_codes)), CAPSMI_ERR_ILLEGAL_ARGUMENT,
                "mask list: null columns or codes");
        REQUIRE(ncols <= kMaskListCols, CAPSMI_ERR_UNSUPPORTED,
                "mask list: " + std::to_string(ncols) + " columns, at most " + std::to_string(kMaskListCols) +
                    " (one mask word per row)");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::MASK_LIST;
        hold(*p, t);
        p->a = {name};
        p->jt = mode;
        for (int i = 0; i < ncols; ++i) {
            const Column& c = t->cols[col_of(t, cols[i])];
            REQUIRE(mode != CAPSMI_MASK_TRUE || c.type == CAPSMI_BOOL, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                    "mask list: column '" + c.name + "' is not Boolean");
            p->b.push_back(c.name);
            p->codes.push_back(elem_codes[i]);
        }
        return lazy_table(t->sess, p, explode_schema(t, schema_col(name, CAPSMI_LIST_STR, false)));
    });
}

capsmi_status capsmi_join(capsmi_table* l, capsmi_table* r, int32_t join_type, int32_t npairs, const char* const* lcols,
                          const char* const* rcols, capsmi_table** out) {
    return build(l, out, [&] {
        need(r, "right");
        REQUIRE(l->sess == r->sess, CAPSMI_ERR_ILLEGAL_ARGUMENT, "tables belong to different sessions");
        REQUIRE(join_type >= CAPSMI_JOIN_INNER && join_type <= CAPSMI_JOIN_CROSS, CAPSMI_ERR_ILLEGAL_ARGUMENT, "join type");
        REQUIRE(join_type == CAPSMI_JOIN_CROSS || npairs > 0, CAPSMI_ERR_ILLEGAL_ARGUMENT, "equi-join needs key pairs");
        for (const Column& a : l->cols)
            for (const Column& b : r->cols)
                REQUIRE(a.name != b.name, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                        "join inputs share column '" + a.name + "' (RelationalPlanner renames to disjoint columns)");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::JOIN;
        hold(*p, l);
        hold(*p, r);
        p->jt = join_type;
        if (join_type != CAPSMI_JOIN_CROSS) {
            REQUIRE(npairs <= 8, CAPSMI_ERR_NOT_IMPLEMENTED, "more than 8 key columns");
            for (int i = 0; i < npairs; ++i) {
                const int a = col_of(l, lcols[i]), b = col_of(r, rcols[i]);
                const int ta = l->cols[a].type, tb = r->cols[b].type;
                no_list_key(ta, l->cols[a].name, "a join key");
                no_list_key(tb, r->cols[b].name, "a join key");
                const bool na = ta == CAPSMI_I64 || ta == CAPSMI_F64, nb = tb == CAPSMI_I64 || tb == CAPSMI_F64;
                REQUIRE(ta == tb || (na && nb), CAPSMI_ERR_ILLEGAL_ARGUMENT,
                        "join key types differ: " + l->cols[a].name + " vs " + r->cols[b].name);
                p->a.push_back(lcols[i]);
                p->b.push_back(rcols[i]);
            }
        }
        const bool lmiss = join_type == CAPSMI_JOIN_RIGHT_OUTER || join_type == CAPSMI_JOIN_FULL_OUTER;
        const bool rmiss = join_type == CAPSMI_JOIN_LEFT_OUTER || join_type == CAPSMI_JOIN_FULL_OUTER;
        std::vector<Column> sch;
        for (auto& c : l->cols) sch.push_back(schema_col(c.name, c.type, c.nullable() || lmiss));
        for (auto& c : r->cols) sch.push_back(schema_col(c.name, c.type, c.nullable() || rmiss));
        return lazy_table(l->sess, p, sch);
    });
}

capsmi_status capsmi_union_all(capsmi_table* a, capsmi_table* b, capsmi_table** out) {
    return build(a, out, [&] {
        need(b, "right");
        REQUIRE(a->cols.size() == b->cols.size(), CAPSMI_ERR_ILLEGAL_ARGUMENT, "union all: column counts differ");
        std::vector<Column> sch;
        for (size_t i = 0; i < a->cols.size(); ++i) {
            REQUIRE(a->cols[i].type == b->cols[i].type, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                    "Equal column data types for union all (differing nullability is OK): " + a->cols[i].name + " vs " +
                        b->cols[i].name);
            sch.push_back(schema_col(a->cols[i].name, a->cols[i].type, a->cols[i].nullable() || b->cols[i].nullable()));
        }
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::UNION;
        hold(*p, a);
        hold(*p, b);
        return lazy_table(a->sess, p, sch);
    });
}

capsmi_status capsmi_order_by(capsmi_table* t, int32_t nkeys, const char* const* cols, const int32_t* descending,
                              capsmi_table** out) {
    return build(t, out, [&] {
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::ORDER;
        hold(*p, t);
        for (int i = 0; i < nkeys; ++i) {
            const int c = col_of(t, cols[i]);
            no_list_key(t->cols[c].type, t->cols[c].name, "a sort key");
            p->a.push_back(cols[i]);
            p->flags.push_back(descending ? descending[i] : 0);
        }
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_skip(capsmi_table* t, int64_t n, capsmi_table** out) {
    return build(t, out, [&] {
        REQUIRE(n >= 0, CAPSMI_ERR_ILLEGAL_ARGUMENT, "negative skip");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::SKIP;
        hold(*p, t);
        p->n = n;
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_limit(capsmi_table* t, int64_t n, capsmi_table** out) {
    return build(t, out, [&] {
        REQUIRE(n >= 0 && n <= 2147483647LL, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                "an integer: limit must fit an Int (SparkTable.scala:117)");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::LIMIT;
        hold(*p, t);
        p->n = n;
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_distinct(capsmi_table* t, capsmi_table** out) {
    return build(t, out, [&] {
        for (auto& c : t->cols) no_list_key(c.type, c.name, "a distinct key");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::DISTINCT;
        hold(*p, t);
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_distinct_on(capsmi_table* t, int32_t ncols, const char* const* cols, capsmi_table** out) {
    return build(t, out, [&] {
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::DISTINCT_ON;
        hold(*p, t);
        for (int i = 0; i < ncols; ++i) {
            const int c = col_of(t, cols[i]);
            no_list_key(t->cols[c].type, t->cols[c].name, "a distinct key");
            p->a.push_back(cols[i]);
        }
        std::vector<Column> sch;
        for (auto& c : t->cols) sch.push_back(schema_of(c));
        return lazy_table(t->sess, p, sch);
    });
}

capsmi_status capsmi_group(capsmi_table* t, int32_t nby, const char* const* by, int32_t naggs, const capsmi_agg* aggs,
                           capsmi_table** out) {
    return build(t, out, [&] {
        REQUIRE(naggs == 0 || aggs, CAPSMI_ERR_ILLEGAL_ARGUMENT, "null aggregations");
        auto p = std::make_shared<PlanNode>();
        p->kind = PlanNode::GROUP;
        hold(*p, t);
        std::vector<Column> sch;
        for (int i = 0; i < nby; ++i) {
            const int c = col_of(t, by[i]);
            no_list_key(t->cols[c].type, t->cols[c].name, "a grouping key");
            p->a.push_back(by[i]);
            sch.push_back(schema_of(t->cols[c]));
        }
        for (int i = 0; i < naggs; ++i) {
            const capsmi_agg& ag = aggs[i];
            need(ag.output, "aggregate output name");
            AggSpec sp;
            sp.kind = ag.kind;
            sp.distinct = ag.distinct;
            sp.output = ag.output;
            int32_t ty = CAPSMI_I64;
            bool nullable = false;
            switch (ag.kind) {
                case CAPSMI_AGG_COUNT_STAR: break;
                case CAPSMI_AGG_COUNT: sp.input = t->cols[col_of(t, ag.input)].name; break;
                case CAPSMI_AGG_SUM: case CAPSMI_AGG_AVG: {
                    const Column& c = t->cols[col_of(t, ag.input)];
                    REQUIRE(c.type == CAPSMI_I64 || c.type == CAPSMI_F64, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                            ag.kind == CAPSMI_AGG_SUM ? "sum of non-number" : "avg of non-number");
                    sp.input = c.name;
                    ty = c.type;
                    nullable = true;
                    break;
                }
                case CAPSMI_AGG_MIN: case CAPSMI_AGG_MAX: {
                    const Column& c = t->cols[col_of(t, ag.input)];
                    no_list_key(c.type, c.name, "an aggregate input");
                    sp.input = c.name;
                    ty = c.type;
                    nullable = true;
                    break;
                }
                case CAPSMI_AGG_COLLECT: {  // sort_array(collect_list / collect_set), SparkTable.scala:169-177
                    const Column& c = t->cols[col_of(t, ag.input)];
                    no_list_key(c.type, c.name, "an aggregate input");
                    sp.input = c.name;
                    ty = CAPSMI_LIST + c.type;
                    break;
                }
                default: throw Error(CAPSMI_ERR_NOT_IMPLEMENTED, "Aggregation function " + std::to_string(ag.kind));
            }
            p->aggs.push_back(sp);
            sch.push_back(schema_col(ag.output, ty, nullable));
        }
        return lazy_table(t->sess, p, sch);
    });
}

}  // extern "C"
