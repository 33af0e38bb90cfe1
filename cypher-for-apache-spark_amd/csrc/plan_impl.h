// plan_impl.h -- what the files of the plan family share: the lazy plan node, the recogniser's types and the
// functions that cross a file boundary.  Internal to libcapsmi; not installed.
//   plan.hip ......... PlanNode lifetime, the lazy capsmi_* builders, the operator executor, materialize
//   plan_match.hip ... the recogniser: scans, paths, conjuncts, id windows, node bitmaps, relationship views
//   plan_routes.hip .. the fused routes and their order (the route table is that file's header)
//   plan_dist.hip .... the routes' bodies over a distributed graph
//   plan_entity.hip .. entity registration, narrow and presence copies, session setters, graph_compact
#pragma once
#include <algorithm>
#include <cstring>
#include <functional>
#include <map>
#include <set>

#include "capsmi_impl.h"

namespace capsmi {

void set_last_error(const std::string& m);
std::string last_error_string();

struct AggSpec {
    int32_t kind = 0, distinct = 0;
    std::string input, output;
};

struct PlanNode {
    enum Kind { SELECT, DROP, RENAME, FILTER, WITH_COLUMNS, JOIN, UNION, DISTINCT, DISTINCT_ON, GROUP, ORDER, SKIP, LIMIT,
                EXPLODE, RANGE, MASK_LIST };
    Kind kind = SELECT;
    std::vector<capsmi_table*> in;            // retained inputs
    std::vector<std::string> a, b;            // column names (see builders)
    std::vector<std::vector<capsmi_expr>> progs;
    std::vector<int32_t> flags;               // ORDER: descending
    std::vector<AggSpec> aggs;
    int32_t jt = 0;
    int64_t n = 0;
    // EXPLODE: b[0] the item column; a[0] the list column, or a empty for the constant form with its
    // `n` values `vals` of element type `jt`
    std::vector<capsmi_value> vals;
    // RANGE: a[0] the list column; progs[0..2] the from / to / step programs (step empty: the literal 1)
    // MASK_LIST: a[0] the list column; b the mask's columns with their names' `codes`; jt the CAPSMI_MASK_* mode
    std::vector<int64_t> codes;
    ~PlanNode() {
        for (capsmi_table* t : in) capsmi_table_release(t);
    }
};

namespace planning {

#define P_BEGIN try {
#define P_END                                                   \
    }                                                           \
    catch (const capsmi::Error& e) {                            \
        set_last_error(e.what());                               \
        return e.code;                                          \
    }                                                           \
    catch (const std::bad_alloc&) {                             \
        set_last_error("host allocation failed");               \
        return CAPSMI_ERR_OUT_OF_MEMORY;                        \
    }                                                           \
    catch (const std::exception& e) {                           \
        set_last_error(e.what());                               \
        return CAPSMI_ERR_INTERNAL;                             \
    }                                                           \
    return CAPSMI_OK;

// ---- plan.hip ----------------------------------------------------------------------------------
void need(const void* p, const char* what);
void check(capsmi_status st);
int find_col(const capsmi_table* t, const std::string& name);
int col_of(const capsmi_table* t, const char* name);
bool pinned(const capsmi_table* t);
// the body of a capsmi_* builder: null checks, *out = f(), errors to status codes
capsmi_status build(capsmi_table* t, capsmi_table** out, const std::function<capsmi_table*()>& f);

// ---- plan_match.hip: the recogniser ---------------------------------------------------------------
enum { ROLE_NONE = 0, ROLE_ID = 1, ROLE_SRC = 2, ROLE_DST = 3 };

// A scan: union of registered entity tables, each column a base column or a per-table constant
// (ScanGraph.scanOperator's aligned entity tables, ScanGraph.scala:61-96).
struct Member {
    capsmi_table* base = nullptr;
    std::vector<int> src;            // per scan column: base column, or -1 (constant)
    std::vector<capsmi_expr> cst;    // the constant as a one-node program (LIT / NULL)
};
struct Scan {
    int kind = 0;  // 1 node, 2 relationship
    std::vector<Member> m;
    std::vector<int> role;  // per scan column: ROLE_* in every member, else ROLE_NONE
    // relationship scan filtered to start <> end: the incoming branch of an undirected Expand
    // (RelationalPlanner.scala:130-131)
    bool no_loops = false;
};

enum RK : int8_t { RK_EXPR, RK_CONST, RK_NODE, RK_REL };
struct Role {
    RK k = RK_EXPR;
    int inst = -1, scol = -1;
    capsmi_expr cst{};
};

struct ENode {
    capsmi_expr x{};
    Role role;  // CAPSMI_X_COL leaves
    std::vector<ENode> kids;
};

struct Hop {
    int rel = -1;          // instance of the relationship scan
    int from = -1, to = -1;  // positions
    int from_role = ROLE_SRC, to_role = ROLE_DST;
};

// A join chain over scans: positions (pattern nodes) joined by hops (relationships)
struct Path {
    std::vector<Scan> inst;
    std::vector<int> pos_node;  // per position: node-scan instance, or -1
    std::vector<Hop> hops;
    std::vector<Role> cols;     // per output column
    std::vector<ENode> conj;    // filter conjuncts
};

struct Classified {
    std::set<std::pair<int, int>> uniq;         // hop pairs (i < j) with NOT(r_i = r_j)
    std::vector<std::vector<const ENode*>> pred; // per instance: node predicate conjuncts
};

// The rank view of a route over a distributed graph (capsmi_graph_distribute, k_dist.hip): the scanned
// tables are this rank's shards; the route exchanges through the session's collective.
struct DistView {
    bool on = false;  // world > 1
    int rank = 0, world = 1;
    int64_t slice_words = 0;
    int rel_mode = -1;  // CAPSMI_RELS_* of the relationship shards
};

struct BitmapSet {
    std::vector<std::pair<std::string, capsmi_bitmap*>> made;
    ~BitmapSet() {
        for (auto& x : made) capsmi_bitmap_release(x.second);
    }
};

// the relationship tables of a hop as (source-side, target-side) column views, zero-copy
struct RelViews {
    std::vector<capsmi_table*> t;
    std::string sig;  // identity of the tables and oriented columns (hops over equal sets share kernels)
    ~RelViews() {
        for (auto* x : t) capsmi_table_release(x);
    }
};

// the (s, t) columns of relationship views, as the kernels' entry points take them
struct RelCols {
    std::vector<const int64_t*> srcs, dsts;
    std::vector<int64_t> ms;
    explicit RelCols(const std::vector<capsmi_table*>& views) {
        for (capsmi_table* t : views) {
            srcs.push_back(t->cols[0].d());
            dsts.push_back(t->cols[1].d());
            ms.push_back(t->nrows);
        }
    }
};

enum Agg1 { A_COUNT, A_DISTINCT_END, A_DISTINCT_START };
enum { TRI_NONE = 0, TRI_CYCLE = 1, TRI_TRANSITIVE = 2 };  // closed_triangle

extern thread_local const DenseIds* g_dense;  // domain of the route being planned (one at a time)
extern thread_local DistView g_dist;

bool as_scan(const capsmi_table* t, Scan& sc);
bool as_paths(const capsmi_table* t, std::vector<Path>& out);
int position_of(const Path& P, const Role& r);
bool classify(const Path& P, Classified& c);
bool id_window(const std::vector<Path>& B, int64_t* lo, int64_t* hi);
capsmi_table* dense_view(const capsmi_table* base);
capsmi_bitmap* node_bitmap(capsmi_session* s, const Path& P, const Classified& c, int inst, int64_t lo, int64_t hi,
                           BitmapSet& bs, std::string* key_out = nullptr);
void rel_views(const Path& P, const Hop& h, RelViews& v);
void reversed_views(const RelViews& v, RelViews& r);
bool id_like(const Path& P, const Role& r);
capsmi_table* result_table(capsmi_session* s, int64_t rows);
bool agg_kinds(const capsmi_table* in, const PlanNode& g, const Path& P, int start, int end, std::vector<int>& kinds);
bool is_chain(const Path& P);
bool same_orientation(const Path& P);
Hop directed(const Hop& h);
int closed_triangle(const Path& P, int role[3]);
bool all_pairs_unique(const Classified& c, int nh);
capsmi_bitmap* one_set_one_filter(capsmi_session* s, const Path* B, const Classified* cls, size_t nb, int64_t lo,
                                  int64_t hi, BitmapSet& bs, RelViews& v0);

// ---- plan_routes.hip -------------------------------------------------------------------------------
extern thread_local bool g_missed;  // a pattern shape went unrouted during the current materialisation
bool try_fused(capsmi_table* t, capsmi_table** out);
// try the fused shapes for lazy table `t`; on success *out is its materialised content
bool try_fused_shapes(capsmi_table* t, capsmi_table** out);

// ---- plan_dist.hip: the routes over a distributed graph (g_dist.on) ------------------------------------
int64_t sum_over_ranks(capsmi_session* s, int64_t v);
int64_t dist_two_hop_distinct(capsmi_session* s, const capsmi_relpart* cached, int32_t nt, capsmi_table* const* views,
                              const capsmi_bitmap* a, const capsmi_bitmap* b, const capsmi_bitmap* c);
int64_t dist_two_hop_distinct_src(capsmi_session* s, const capsmi_relpart* cached, int32_t nt, capsmi_table* const* views,
                                  const capsmi_bitmap* a, const capsmi_bitmap* b, const capsmi_bitmap* c);
int64_t dist_two_hop_count(capsmi_session* s, int32_t nt, capsmi_table* const* views, const capsmi_bitmap* a,
                           const capsmi_bitmap* b, const capsmi_bitmap* c);
int64_t dist_two_hop_count_owned(capsmi_session* s, const Path& P, const RelViews& v0, const capsmi_bitmap* a,
                               const capsmi_bitmap* b, const capsmi_bitmap* c);
int64_t dist_triangle_count(capsmi_session* s, const std::vector<capsmi_table*>& views, const capsmi_bitmap* n_ok);
void dist_undirected(capsmi_session* s, const Scan& R, const std::vector<const int64_t*>& srcs,
                     const std::vector<const int64_t*>& dsts, const std::vector<int64_t>& ms, int h,
                     const std::vector<capsmi_bitmap*>& pos, const std::vector<int>& kinds, std::vector<int64_t>& vals);
void dist_var_length(capsmi_session* s, const std::vector<capsmi_table*>& views,
                     const std::vector<const capsmi_table*>& bases, const capsmi_bitmap* a, const capsmi_bitmap* b,
                     int lower, int upper, const std::string& id_name, const std::string& count_name,
                     capsmi_table** out);

}  // namespace planning
}  // namespace capsmi
