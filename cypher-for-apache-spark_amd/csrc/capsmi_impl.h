// capsmi_impl.h -- internal runtime of libcapsmi (not part of the ABI).
//
// Device tables are column-major: one 8-byte word per row and column, plus an
// optional byte-per-row validity map.  Columns share ref-counted device buffers,
// so select/drop/rename/skip/limit are metadata-only (the Spark analogue is a
// Catalyst projection, SparkTable.scala:61-92).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <functional>
#include <vector>

#include "../../include/capsmi.h"
#include "capsmi_error.h"
#include "expr_prog.h"

namespace capsmi {

// ---- errors (Error and REQUIRE: capsmi_error.h) ------------------------------------
[[noreturn]] void throw_hip(hipError_t e, const char* what, const char* file, int line);
#define HIP_CHECK(x)                                                     \
    do {                                                                 \
        hipError_t e__ = (x);                                            \
        if (e__ != hipSuccess) ::capsmi::throw_hip(e__, #x, __FILE__, __LINE__); \
    } while (0)

// ---- device memory --------------------------------------------------------------
// Stream-ordered allocations from the device's default pool (release threshold
// raised at session create, so freed blocks are recycled instead of unmapped).
// Per-session allocation context: the device, the stream the session currently runs on, and the
// session's cache of freed device blocks (api.hip).  Blocks hold it, so a block that outlives its
// session is returned to the device instead of to a dead cache.
struct AllocCtx;
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    std::shared_ptr<AllocCtx> ctx;
    ~DevBuf();
};
using Buf = std::shared_ptr<DevBuf>;
Buf dev_alloc(size_t bytes, capsmi_session* s);

template <class T>
inline T* P(const Buf& b) { return b ? static_cast<T*>(b->ptr) : nullptr; }

// Values of a list column (CAPSMI_LIST_*): list k holds values[offsets[k] .. offsets[k+1]).  A list
// column's row word is the index k of its list, so gathers (filter, join, order, union) move list
// rows like any other column and the store rides along by reference.
struct ListStore {
    int32_t elem = CAPSMI_I64;  // element type
    int64_t nlists = 0, nvalues = 0;
    Buf offsets;                // int64, nlists + 1
    Buf values;                 // int64 words, nvalues
};

// The session's string store (capsmi_session_set_strings): string i has code codes[i] (strictly ascending) and
// bytes[offsets[i] .. offsets[i+1]).  Replaced as a whole -- by a registration, or by the merge of the strings an
// action has made (str_store_merge, k_strmake.hip) -- and a pass holds the one it started with.
struct StrStore {
    int64_t n = 0;                           // strings (> 0: an empty registration clears the store)
    Buf codes, offsets, bytes;               // int64[n], int64[n + 1], uint8[offsets[n]]
    std::vector<int64_t> hcodes, hoffsets;   // host copies: constant operands are resolved without the device
    std::string hbytes;                      // and the bytes: a sink's codes are checked against them, literal
                                             // operands of CONCAT are read from them
};
inline bool is_str_match(int32_t op) { return op >= CAPSMI_X_STARTS_WITH && op <= CAPSMI_X_CONTAINS; }

// Endpoint presence words of a registered relationship table (presence_endpoints, plan_entity.hip; the rule:
// presence_rule.h): four bitmaps over the endpoints' window [lo, hi), bit k of word 0 standing for id lo + k.
// Facts about the immutable table which no query shapes; hop 1 of a 2-hop whose first node is unfiltered reads
// them instead of the relationships (k_presence_hop1, k_part.hip).
struct PresenceWords {
    Buf in;     // ids that are the target of a relationship with source != target
    Buf out;    // ids that are the source of one
    Buf loop1;  // ids with at least one self-loop
    Buf loop2;  // ids with at least two
    int64_t lo = 0, hi = 0, nwords = 0;
    // what they were made from: the two columns' data blocks and row offsets, and the row count
    const DevBuf* src_of = nullptr;
    const DevBuf* dst_of = nullptr;
    int64_t src_off = 0, dst_off = 0, rows = 0;
};

struct Column {
    std::string name;
    int32_t type = CAPSMI_I64;
    Buf data;              // int64 words
    Buf valid;             // uint8 per row, may be null (no nulls)
    std::shared_ptr<const ListStore> list;  // list columns only
    int64_t offset = 0;    // row offset into data/valid (zero-copy skip)
    bool lazy_nullable = false;  // schema of a lazy table's column (no data yet): may hold nulls
    // host copy of the words of a column built from host values (the fused routes' count rows):
    // exports read it without a device round trip
    std::shared_ptr<const std::vector<int64_t>> host;
    // optional 32-bit copy of `data`, made when a relationship table is registered (narrow_endpoints, plan_entity.hip):
    // narrow[i] = data[i] - narrow_base over the rows the table had then, under the same row `offset`.  The
    // words are immutable and shared, so a copy of the Column carries them along; `narrow_of` names the words
    // they were made from, so a Column whose `data` was replaced since no longer offers them (n32).
    Buf narrow;
    const DevBuf* narrow_of = nullptr;
    int64_t narrow_base = 0;
    // optional presence words of the relationship table this endpoint column was registered with, shared by both
    // endpoint columns and carried along like `narrow`; presence_rel (plan_entity.hip) decides whether a pair of columns
    // may still read them
    std::shared_ptr<const PresenceWords> presence;
    const int64_t* d() const { return P<int64_t>(data) + offset; }
    const uint32_t* n32() const { return narrow && narrow_of == data.get() ? P<uint32_t>(narrow) + offset : nullptr; }
    const uint8_t* v() const { return valid ? P<uint8_t>(valid) + offset : nullptr; }
    bool nullable() const { return valid != nullptr || lazy_nullable; }
};

// Entity-table contract of a registered node / relationship table (capsmi_node_table /
// capsmi_rel_table; EntityTable.verify, okapi-relational/.../api/io/EntityTable.scala:59-65,155-164).
struct EntityInfo {
    int kind = 0;                 // 1 node, 2 relationship
    int id = -1, src = -1, dst = -1;  // column indices of the key columns
    int64_t lo = 0, hi = 0;       // [min, max + 1) of the ids (node) or of both endpoints (relationship)
    int64_t rows = 0;
    bool ids_exact = false;       // node: the ids are exactly [lo, hi), each once (checked at registration)
    bool ids_unique = false;      // node: no id occurs twice and none is null (checked at registration)
};
struct PlanNode;  // lazy Table[T] operator (plan_impl.h)

// Dense id space of one graph (capsmi_graph_compact): every node id and relationship endpoint of
// the graph's entity tables numbered 0..n-1; orig[d] is the Long id of dense id d.  The fused
// routes run on dense ids when the Long ids do not fit one window of 2^30 ids.
// The signed order of a dense domain's original ids (id_order_build, k_reach.hip): sorted_orig[p] is the p-th
// smallest original id and by_rank[p] the dense id that holds it, so orig[by_rank[p]] == sorted_orig[p].
struct IdOrder {
    int64_t n = 0;
    Buf sorted_orig, by_rank;  // int64 x n each
};

struct DenseIds {
    int64_t n = 0;
    Buf orig;
    // built at the first var-length collect(DISTINCT b) routed on this domain and kept with it: 16 B per id
    // (the orig-table form only); guarded by order_mu
    mutable std::shared_ptr<const IdOrder> order;
    mutable std::mutex order_mu;
    // a distributed graph's domain (capsmi_graph_distribute): dense = h(x) = ((x - lo) * mul) mod 2^kbits,
    // x = (dense * mul_inv mod 2^kbits) + lo; no orig table
    bool scrambled = false;
    int kbits = 0;
    uint64_t mul = 0, mul_inv = 0;
    int64_t lo = 0;
};

// A rank's shard of a distributed graph (capsmi_graph_distribute): owned dense ids are
// [rank * 32 * slice_words, (rank + 1) * 32 * slice_words) of the scrambled domain
struct Shard {
    int kind = 0;   // 1 node table, 2 relationship table
    int mode = 0;   // node: CAPSMI_NODES_*; relationship: CAPSMI_RELS_*
    int rank = 0, world = 1;
    int64_t slice_words = 0;
    // node table: its rows (over every rank's shard when OWNED) are each id of the whole scrambled
    // domain exactly once, so a predicate-free scan sets every bit without reading a row or exchanging
    bool covers = false;
};

}  // namespace capsmi

namespace capsmi {
// Session configuration: every CAPSMI_* knob of the library, read from the environment
// ONCE, when the session is created (capsmi_session_create), and changed afterwards only through
// capsmi_session_set_config -- no call site reads the environment.  The defaults are the measured
// choices; the non-defaults force the fallback forms (used above a size limit or when a layout does not
// fit) at sizes where tests can check them against the oracle.  Process-wide, outside this struct:
// CAPSMI_CACHE_BYTES (the block cache shared by all sessions, read at the first allocation) and
// CAPSMI_POOL_KEEP_BYTES (the device pool's release threshold, set at each session create).
struct Config {
    int join = 0;                 // CAPSMI_JOIN = auto | direct | hash | radix (0..3): force a join strategy
    bool count_atomic = false;    // CAPSMI_COUNT = atomic: 2-hop count(*) by per-relationship atomic degrees
                                  //   (the form above 2^26 ids) instead of the record partition
    bool rec_full = true;         // CAPSMI_REC_FULL = 0: the undirected record partition's general form also
                                  //   for full node filters
    bool grouped_keys = false;    // CAPSMI_GROUPED = keys: grouped count(DISTINCT c) by the per-binding key sort
    int pairs = 0;                // CAPSMI_PAIRS = packed | uint2 (1 | 2): force the cached layout's pair form
    int hop2 = 0;                 // CAPSMI_HOP2 = pool | cells (1 | 2): force the cold 2-hop's form for a full a_ok, both hops
                                  //   over the pass-1 pool or pass 2 + the cell hops (auto: the pool up to 2^26 ids, k_part.hip)
    bool pool_split = true;       // CAPSMI_POOL = split | pairs: the format of the pass-1 pool that the pool hops walk --
                                  //   target and source words in two arrays per chunk, so hop 1 reads 4 B per
                                  //   relationship, or 8-byte pairs (every other pool is pairs)
    bool hop2_exchange = true;    // CAPSMI_HOP2_EXCHANGE = on | off: hop 2 over the split pool lets the blocks that share a
                                  //   target slice exchange their C bits through the global C while they walk (off: each
                                  //   block finds every target of its share for itself; k_part.hip k_pool_hop2)
    bool tri_sorted_build = false;  // CAPSMI_TRI_BUILD = sorted: the sort-oriented trigraph build (above 2^24 ids)
    int tri_deg_sample = 0;       // CAPSMI_TRI_DEG_SAMPLE: 1 in k relationships for the degree order (0: auto)
    bool tri_split = true;        // CAPSMI_TRI_SPLIT = 0: the combined (not direction-split) triangle walks
    bool tri_und_hash = true;     // CAPSMI_TRI_UND_COUNT = walk: the undirected triangle's count by the search walk
    int tri_vmode_t = 256;        // CAPSMI_TRI_VMODE_T: od(v) threshold of the v-mode walks (0: all u-mode)
    bool und_stream = false;      // CAPSMI_UND = stream: undirected count(DISTINCT) by the streaming form
                                  //   (the form above 2^26 ids) instead of the cell layout
    int vl_bits = 8;              // CAPSMI_VL_BITS: bits per pair of the var-length reverse-pair filter
    int vl_sublog = -1;           // CAPSMI_VL_SUBLOG: filter regions per slice, log2 (-1: auto)
    bool vl_f2 = false;           // CAPSMI_VL_F2 = 1: the second-level filter in the T walk (the sharded form's)
    int reach_words = 0;          // CAPSMI_REACH_WORDS = auto | 1 | 2 | 4 | 8 (0 = auto): 64-bit words per node of the
                                  //   grouped var-length count(DISTINCT b), i.e. 64 sources per word and batch (k_reach.hip)
    bool reach_flat = false;      // CAPSMI_REACH = sliced | flat: flat forces the global-OR level pass (the form of
                                  //   domains beyond the target-sliced LDS pass)
    int64_t reach_list_limit = 0; // CAPSMI_REACH_LIST_LIMIT = auto | elements (0 = auto): the most list elements a
                                  //   var-length collect(DISTINCT b) may produce (auto: device memory / 16 B, the
                                  //   route's peak per element); beyond it the query is CAPSMI_ERR_UNSUPPORTED
    int64_t coll_chunk = int64_t(1) << 26;  // CAPSMI_COLL_CHUNK: elements per host collective call
    int ingest_threads = 0;       // CAPSMI_INGEST_THREADS (0: OMP_NUM_THREADS, else up to 16 hardware threads)
    bool narrow = true;           // CAPSMI_NARROW = auto | off: registering a relationship table whose endpoints span at most
                                  //   2^32 ids keeps a 32-bit copy of both endpoint columns (8 B per relationship of device
                                  //   memory), which pass 1 of the chunk partition reads instead of the int64 words; off
                                  //   builds none and reads none
    bool presence = true;         // CAPSMI_PRESENCE = auto | off: registering a relationship table whose endpoints span at
                                  //   most 2^26 ids keeps four presence bitmaps over the window (non-loop targets, non-loop
                                  //   sources, ids with one / two self-loops: 4 bits per id), from which hop 1 of a 2-hop
                                  //   with an unfiltered first node is answered without reading the relationships; off
                                  //   builds none and reads none
    int str_match = 0;            // CAPSMI_STR_MATCH = auto | rows | dict (0..2): which side a string match with a constant
                                  //   pattern runs on -- once per row, or once per entry of the string store with a
                                  //   lookup per row (auto: the store when the table has at least as many rows; k_strmatch.hip);
                                  //   size() / toInteger() / toFloat() / toBoolean() of a String column likewise (k_strconv.hip)
};
// the environment's values over the defaults
Config config_from_env();
// one knob by its environment name; value NULL = back to the environment's value (or the default).
// Returns false for an unknown name or an unparsable value.
bool config_set(Config& c, const char* name, const char* value);
}  // namespace capsmi

struct capsmi_session {
    capsmi::Config cfg;  // read once at create (capsmi::Config)
    std::shared_ptr<capsmi::AllocCtx> alloc;  // block cache of this session (api.hip)
    struct Param {
        int32_t type = 0;
        bool list = false;
        std::vector<capsmi_value> values;
    };
    std::vector<Param> params;  // query parameters (capsmi_session_set_params)
    std::shared_ptr<const capsmi::StrStore> strings;  // the string store (capsmi_session_set_strings); null: none
    // how strings made on the device get their codes (capsmi_session_set_string_sink); null: no sink
    capsmi_string_sink_fn sink = nullptr;
    void* sink_ctx = nullptr;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // current (own or external)
    int num_cus = 256;
    // small pinned staging buffer for scalar read-backs ([0]: read_scalar, [1]: read_scalar_async)
    int64_t* pinned = nullptr;
    hipEvent_t ev_read = nullptr;  // read_scalar_async's copy done
    // per-kernel event timing (capsmi_session_set_profiling)
    bool prof = false;
    std::set<std::string> prof_names;  // the timers that record (empty: all; capsmi_session_set_profiling_names)
    struct Pending {
        std::string name;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;  // resolved timer events, reused (no event creation inside a timed query)
    hipEvent_t take_event() {
        hipEvent_t e = nullptr;
        if (!ev_pool.empty()) {
            e = ev_pool.back();
            ev_pool.pop_back();
        } else if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
        }
        return e;
    }
    std::map<std::string, std::pair<int64_t, double>> totals;
    std::map<std::string, double> alg_bytes;  // algorithmic bytes of the timed launches, per name
    // fused-path routing of lazy plans (plan_routes.hip): enabled flag and per-route counters
    bool fused = true;
    std::map<std::string, int64_t> routes;
    // multi-GPU rank view (capsmi_session_set_ranks): the host's collective on this session's stream
    int rank = 0, world = 1;
    capsmi_collective_fn coll = nullptr;
    void* coll_ctx = nullptr;
    // refuse unrouted joins whose estimated output exceeds this many bytes (0 = no limit;
    // capsmi_session_set_unrouted_limit)
    int64_t unrouted_limit = 0;
    // capsmi_read_csv row ids over Spark's file-scan partitions (capsmi_session_set_csv_partitioning;
    // parallelism 0: one partition)
    int64_t csv_parallelism = 0, csv_max_partition_bytes = int64_t(128) << 20, csv_open_cost = int64_t(4) << 20;
};

namespace capsmi {
// brackets one kernel launch with events on the session stream when profiling is on
struct KernelTimer {
    capsmi_session* s;
    const char* name;
    hipEvent_t a = nullptr, b = nullptr;
    // bytes: the launch's algorithmic bytes (inputs read once, outputs written once), if known
    KernelTimer(capsmi_session* s_, const char* n, double bytes = 0) : s(s_), name(n) {
        if (!s->prof || (!s->prof_names.empty() && !s->prof_names.count(name))) return;
        a = s->take_event();
        b = s->take_event();
        if (a && b) {
            (void)hipEventRecord(a, s->stream);
            if (bytes > 0) s->alg_bytes[name] += bytes;
        } else {
            for (hipEvent_t* e : {&a, &b})
                if (*e) s->ev_pool.push_back(*e);
            a = b = nullptr;
        }
    }
    ~KernelTimer() {
        if (a && b) {
            (void)hipEventRecord(b, s->stream);
            s->pending.push_back({name, a, b});
        }
    }
};
}  // namespace capsmi

struct capsmi_table {
    std::atomic<int> refs{1};
    capsmi_session* sess = nullptr;
    int64_t nrows = 0;               // valid once materialised (plan == null)
    std::vector<capsmi::Column> cols;  // lazy: the schema only (name, type, lazy_nullable)
    std::shared_ptr<capsmi::PlanNode> plan;            // non-null until materialised (plan.hip)
    std::shared_ptr<const capsmi::EntityInfo> entity;  // registered entity table
    // Table.cache on a relationship table (SparkTable.scala:240-246): fused routes keep the layouts
    // they build from it (partitioned 2-hop layout per orientation and id window), freed with the table
    bool keep_layouts = false;
    // dense ids of a compacted graph: node tables `did`, relationship tables `dsrc` / `ddst` (int64 per row)
    std::shared_ptr<capsmi::DenseIds> dense;
    capsmi::Column did, dsrc, ddst;
    std::shared_ptr<const capsmi::Shard> shard;  // this rank's shard of a distributed graph
    // the complement of a relationship shard (dense source / target, exchanged at capsmi_graph_distribute):
    // BY_SOURCE, the relationships of other ranks' sources into this rank's owned ids; BY_TARGET, those of
    // this rank's owned sources into other ranks' ids
    capsmi::Column in_src, in_dst;
    int64_t in_rows = 0;
    bool partitioned = false;  // rows are this rank's partition of a distributed result
    std::map<std::string, std::shared_ptr<capsmi_relpart>> layouts;
    bool lazy() const { return (bool)plan; }
    int find(const std::string& n) const {
        for (size_t i = 0; i < cols.size(); ++i)
            if (cols[i].name == n) return (int)i;
        return -1;
    }
};

struct capsmi_bitmap {
    capsmi_session* sess = nullptr;
    int64_t lo = 0, hi = 0;  // id range
    int64_t nwords = 0;      // ceil((hi - lo) / 32)
    capsmi::Buf words;       // uint32 per 32 ids
    int64_t rows_added = 0;  // rows that set a bit (duplicate detection)
    bool any_dup = false;
    int64_t set_bits = -1;   // cached popcount (-1 = stale)
    bool full = false;       // every id in [lo, hi) is set
};

namespace capsmi {

// ---- kernel launchers (k_*.hip) ------------------------------------------------
// scan / compaction / gather (k_basic.hip)
void exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, capsmi_session* s);  // out has n+1 entries
void fill_i64(int64_t* p, int64_t v, int64_t n, hipStream_t st);
void fill_u8(uint8_t* p, uint8_t v, int64_t n, hipStream_t st);
void iota_i64(int64_t* p, int64_t start, int64_t n, hipStream_t st);
// indices i (ascending) with flags[i] != 0; returns count (synchronises)
int64_t flags_to_indices(capsmi_session* s, const uint8_t* flags, int64_t n, Buf& out_idx);
// the rows i < n with flags[i] set, as (id_base + i, val[i]) columns in row order, sized n; returns the row
// count (read once, after the writes are queued)
int64_t flags_to_rows(capsmi_session* s, const uint8_t* flags, int64_t n, const int64_t* val, int64_t id_base,
                      Buf& out_ids, Buf& out_vals);
// dst[i] = idx[i] < 0 ? null : src[idx[i]]; dst_valid written iff non-null
void gather_col(const int64_t* src, const uint8_t* src_valid, const int64_t* idx, int64_t n,
                int64_t* dst, uint8_t* dst_valid, hipStream_t st);
int64_t read_scalar(capsmi_session* s, const int64_t* dev);
// the same in two halves: the copy is queued now and waited for by read_scalar_wait, so the kernels queued
// in between keep the device busy while the host waits (one outstanding read per session)
void read_scalar_async(capsmi_session* s, const int64_t* dev);
int64_t read_scalar_wait(capsmi_session* s);
void invert_u8(const uint8_t* a, uint8_t* b, int64_t n, hipStream_t st);
void add_i64(int64_t* p, int64_t v, int64_t n, hipStream_t st);
void i64_to_f64(const int64_t* a, int64_t* b, int64_t n, hipStream_t st);

// hashing & grouping (k_hash.hip)
constexpr int kMaxKeys = 8;
struct KeyCols {
    const int64_t* data[kMaxKeys];
    const uint8_t* valid[kMaxKeys];
    int32_t n;
};
struct HashTable {
    Buf slot_row;    // int64, -1 = empty; representative row
    Buf slot_count;  // int64 rows per slot
    int64_t cap = 0; // power of two
};
// Insert rows (skipping rows with a null key when skip_null_keys) into a fresh table.
// slot_of_row[i] = slot id or -1.  count=true maintains slot_count.
void hash_build(capsmi_session* s, const KeyCols& k, int64_t n, bool skip_null_keys, HashTable& ht,
                Buf& slot_of_row);
// For each probe row, the slot holding an equal key of the build side, or -1 (null keys never match).
void hash_probe(capsmi_session* s, const KeyCols& probe, const KeyCols& build, int64_t n,
                const HashTable& ht, Buf& slot_of_probe);
// group ids: dense numbering of occupied slots; gid_of_row[i] (-1 for skipped rows); returns #groups
int64_t hash_group_ids(capsmi_session* s, const HashTable& ht, const Buf& slot_of_row, int64_t n,
                       Buf& gid_of_row, Buf& rep_row_of_gid);
// join: rows of the build side grouped by slot: offsets[cap+1], rows[nbuild]
void hash_group_rows(capsmi_session* s, const HashTable& ht, const Buf& slot_of_row, int64_t n,
                     Buf& offsets, Buf& rows);
// load-balanced expansion: for each probe row p with cnt(p) matches emit (p, k) pairs.
//   cnt(p) = slot>=0 ? count[slot] : (outer ? 1 : 0); pairs written to out_l/out_r (r = -1 for outer pad).
int64_t join_expand(capsmi_session* s, const Buf& slot_of_probe, int64_t nprobe, const HashTable& ht,
                    const Buf& offsets, const Buf& rows, bool left_outer, Buf& out_l, Buf& out_r,
                    Buf* matched_build, int64_t nbuild);
// aggregates (per gid)
void agg_count(const int64_t* gid, const uint8_t* valid, int64_t n, int64_t* out, hipStream_t st);
void agg_sum_i64(const int64_t* gid, const int64_t* v, const uint8_t* valid, int64_t n, int64_t* sum,
                 uint8_t* seen, hipStream_t st);
void agg_sum_f64(const int64_t* gid, const int64_t* v, const uint8_t* valid, int64_t n, double* sum,
                 uint8_t* seen, hipStream_t st);
void agg_minmax(const int64_t* gid, const int64_t* v, const uint8_t* valid, int64_t n, int type, bool is_max,
                int64_t* out, uint8_t* seen, hipStream_t st);
void avg_finish(const double* sum, const int64_t* cnt, int64_t ng, bool to_i64, int64_t* out, uint8_t* valid,
                hipStream_t st);
void minmax_finish(int64_t* v, int type, bool is_max, int64_t ng, hipStream_t st);
// Collect (k_list.hip): sort_array(collect_list / collect_set) of column (v, valid) per group id
// (ng groups) into a list store
std::shared_ptr<ListStore> collect_lists(capsmi_session* s, const int64_t* gid, int64_t ng, const int64_t* v,
                                         const uint8_t* valid, int type, int64_t n, bool distinct);
// one store holding a's lists, then b's (b's list k becomes a.nlists + k)
std::shared_ptr<ListStore> concat_lists(capsmi_session* s, const ListStore& a, const ListStore& b);
// UNWIND (k_explode.hip).  Column form: rows (word, valid) of n rows over store L -> the element words `item`
// and the input row `src` of every output row, in (input row, element position) order; returns their number
// (synchronises; item / src stay null when it is 0).  Expansion tiles hold kExplodeTile output rows.
constexpr int kExplodeTile = 2048;
int64_t explode_lists(capsmi_session* s, const int64_t* word, const uint8_t* valid, int64_t n, const ListStore& L,
                      Buf& item, Buf& src);
// constant form: output row j = input row j / count with item vals[j % count] (device words; vvalid and
// item_valid both null when no value is null); item / src hold n * count entries
void explode_values(capsmi_session* s, int64_t n, int64_t count, const int64_t* vals, const uint8_t* vvalid, int64_t* item,
                    uint8_t* item_valid, int64_t* src);
// list expressions (k_listexpr.hip), over the same tiles.  x IN list: out / out_valid[r] = the three-valued
// CAPSMI_X_IN_LIST of probe word (probe, pvalid)[r] of type ptype and the list (word, lvalid)[r] of store L
// (synchronises)
void list_contains(capsmi_session* s, const int64_t* probe, const uint8_t* pvalid, int32_t ptype, const int64_t* word,
                   const uint8_t* lvalid, const ListStore& L, int64_t n, int64_t* out, uint8_t* out_valid);
// string matching (k_strmatch.hip).  An operand is a constant (its code) or the rows' words (data, valid or null)
struct StrOperand {
    bool is_const = false;
    int64_t code = 0;
    const int64_t* data = nullptr;
    const uint8_t* valid = nullptr;
};
// out / out_valid[r] = the three-valued CAPSMI_X_STARTS_WITH / ENDS_WITH / CONTAINS `op` of haystack h and pattern p,
// not both constant, over the store registered now.  Throws ILLEGAL_ARGUMENT when none is, or when a non-null
// operand's code is not in it (synchronises)
void str_match(capsmi_session* s, int32_t op, const StrOperand& h, const StrOperand& p, int64_t n, int64_t* out,
               uint8_t* out_valid);
// the same for two constants, on the host (reads their bytes back; synchronises)
bool str_match_fold(capsmi_session* s, int32_t op, int64_t hcode, int64_t pcode);
// the pieces of it that k_strconv.hip shares.  The store index of a constant's code (throws ILLEGAL_ARGUMENT when it
// is not registered); idx[r] = the store index of row r's code, -1 for a null row and for an absent code, which
// also sets err[0] (queued, timer str_index); the check of err[0] afterwards (synchronises, throws)
int64_t str_const_index(const StrStore& S, int64_t code);
void str_index_rows(capsmi_session* s, const StrStore& S, const StrOperand& o, int64_t n, int64_t* idx, int64_t* err);
void str_index_check(capsmi_session* s, const int64_t* err);
// size(), toInteger(), toFloat() and toBoolean() of Strings (k_strconv.hip; the parsers are str_conv.h).
// out / out_valid[r] = CAPSMI_X_STR_SIZE .. CAPSMI_X_TO_BOOLEAN `op` of the rows' words o (not a constant) over the
// store registered now; throws as str_match does (synchronises)
void str_conv(capsmi_session* s, int32_t op, const StrOperand& o, int64_t n, int64_t* out, uint8_t* out_valid);
// the same for a constant, on the host (reads its bytes back; synchronises): whether the result is not NULL, and it
bool str_conv_fold(capsmi_session* s, int32_t op, int64_t code, int64_t* value);
// toString() and string concatenation (k_strmake.hip; the formatting code is str_make.h).  An operand is a column
// of String codes, Longs or Booleans (data, valid or null), or constant bytes (a literal, formatted by the caller).
struct MakeOperand {
    int32_t type = CAPSMI_STR;  // the column's type; unused for a constant
    bool is_const = false;
    std::string bytes;          // the constant
    const int64_t* data = nullptr;
    const uint8_t* valid = nullptr;
};
// out / out_valid[r] = the code of the bytes of o[0] followed by those of o[1] (nops = 1: o[0] alone), NULL when an
// operand is NULL; at least one operand is a column.  The distinct operand tuples are formatted once each, the
// session's sink gives the codes, and the new entries are merged into the registered store.  Throws
// ILLEGAL_ARGUMENT without a sink, for what the sink may not do, and as str_match does for a STR column
// (synchronises)
void str_make(capsmi_session* s, int nops, const MakeOperand* o, int64_t n, int64_t* out, uint8_t* out_valid);
// the same for constant bytes, on the host: one sink call with one string, the merge, the code
int64_t str_make_fold(capsmi_session* s, const std::string& bytes);
// the bytes of a constant String operand's code (throws ILLEGAL_ARGUMENT when no store is registered or it lacks it)
std::string str_const_bytes(capsmi_session* s, int64_t code);
// range(from, to, step) per row (step null: 1) as a store whose list r is row r's; `valid`: the rows none of
// whose operands is null.  Throws ILLEGAL_ARGUMENT for a step 0, UNSUPPORTED for more elements than the device
// holds (synchronises)
std::shared_ptr<ListStore> range_lists(capsmi_session* s, const int64_t* from, const uint8_t* fv, const int64_t* to,
                                       const uint8_t* tv, const int64_t* step, const uint8_t* sv, int64_t n, Buf& valid);
// labels() / keys() (k_masklist.hip): a String store whose list r holds codes[i], in order, for every column i
// (flag words data[i], validity valid[i] or null) that passes in row r -- non-null and TRUE under
// CAPSMI_MASK_TRUE, non-null under CAPSMI_MASK_NOT_NULL, where data is not read.  At most kMaskListCols columns
// (one mask word per row).  Throws UNSUPPORTED for more elements than the device holds (synchronises)
constexpr int kMaskListCols = 64;
std::shared_ptr<ListStore> mask_lists(capsmi_session* s, int32_t mode, const std::vector<const int64_t*>& data,
                                      const std::vector<const uint8_t*>& valid, const std::vector<int64_t>& codes,
                                      int64_t n);
// multi-GPU (k_dist.hip): the session's collective, stream-ordered (capsmi_collective_fn)
void collective(capsmi_session* s, int op, const void* send, void* recv, int64_t count, int dtype);
// calls of the host collective move at most coll_chunk() elements (CAPSMI_COLL_CHUNK); collective() and
// collective_a2av() split larger ones
int64_t coll_chunk(const capsmi_session* s);
// hipFuncAttributeMaxDynamicSharedMemorySize of `kernel`, set once per (device, kernel) and raised only when a
// launch needs more (the attribute call costs host time on every query otherwise; k_part.hip)
void lds_attr(const void* kernel, size_t bytes);
// ALL_TO_ALL_V with host count lists (world entries each); max_pair: the largest entry of the whole count
// matrix (equal on every rank), which fixes the number of rounds
void collective_a2av(capsmi_session* s, const void* send, const int64_t* send_counts, void* recv,
                     const int64_t* recv_counts, int dtype, int64_t max_pair);
int64_t matrix_max(const std::vector<int64_t>& m);
// hash Exchange of u64 words to rank dest[i] (low byte; 0xFF: not sent); dest / words are reordered
// scratch; returns the received words (rank-major), *nrecv of them; synchronises
Buf exchange_words(capsmi_session* s, uint64_t* dest, uint64_t* words, int64_t n, int64_t* nrecv);
// every rank's words concatenated in rank order; synchronises.  budget_bytes > 0: when the gathered words
// (padded staging + result) would exceed the smallest rank's budget, every rank returns an empty Buf with
// *ntotal = -1, together, right after the all-gather of the (count, budget) pairs
Buf gather_words(capsmi_session* s, const uint64_t* words, int64_t n, int64_t* ntotal, int64_t budget_bytes = 0);
// the generic operators' row exchanges over partitioned tables (k_dist.hip): rows to rank dest[r]; rows
// hash-partitioned by key columns; this rank's slice of a replicated table; every rank's rows
capsmi_table* exchange_rows(capsmi_session* s, const capsmi_table* t, uint64_t* dest);
capsmi_table* exchange_by_keys(capsmi_session* s, const capsmi_table* t, const std::vector<int>& keys,
                               const std::vector<int>& as_f64, bool null_local);
capsmi_table* slice_rows(capsmi_session* s, const capsmi_table* t);
capsmi_table* gather_rows(capsmi_session* s, const capsmi_table* t);
// the scrambled domain of [lo, hi) over `world` ranks: kbits, mul, mul_inv, slice words, domain size
struct Scramble {
    int kbits;
    uint64_t mul, mul_inv;
    int64_t lo, hi, slice_words, n;
};
Scramble make_scramble(int64_t lo, int64_t hi, int world);
// out[i] = h(in[i]); counts rows outside [lo, hi) into bad[0] and rows whose h is outside
// [own_lo, own_hi) into bad[1] (when own_lo < own_hi)
void scramble_ids(capsmi_session* s, const Scramble& sc, const int64_t* in, int64_t n, int64_t* out, int64_t own_lo,
                  int64_t own_hi, unsigned long long* bad);
// x = h^-1(d) for n dense ids, in place
void unscramble_ids(capsmi_session* s, const DenseIds& d, int64_t* v, int64_t n);
// flags[i] = h(in[i]) in [own_lo, own_hi) (ids outside [lo, hi): 0)
void owned_flags(capsmi_session* s, const Scramble& sc, const int64_t* in, int64_t n, int64_t own_lo, int64_t own_hi,
                 uint8_t* flags);
// REQUIRE(!is_list_type) for a column used as a key / expression operand
void no_list_key(int32_t type, const std::string& name, const char* what);
// radix-partitioned equi-join (k_rjoin.hip): (probe row, build row) pairs grouped by key-hash
// partition; build row -1 for an unmatched or null-key probe row when `outer`.  Returns #pairs.
int64_t radix_join(capsmi_session* s, const KeyCols& bk, int64_t nb, const KeyCols& pk, int64_t np, bool outer,
                   Buf& out_p, Buf& out_b);
// direct-address join (k_rjoin.hip): single Long key, unique build keys in a dense range; false if
// not eligible (then nothing was produced)
bool direct_join(capsmi_session* s, const KeyCols& bk, int64_t nb, const KeyCols& pk, int64_t np, bool outer,
                 Buf& out_p, Buf& out_b, int64_t* total);
// the same from two partitions of 2-byte records (k_count.hip rec::), the default
// undirected: the 2-hop of undirected Expands (both arcs of every relationship, r1 = r2 bindings subtracted)
int64_t two_hop_count_rec(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                          int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, const capsmi_bitmap* c_ok,
                          bool undirected = false);
void cross_pairs(int64_t nl, int64_t nr, int64_t* out_l, int64_t* out_r, hipStream_t st);

// expressions (k_expr.hip)
struct ExprArgs;
void eval_expr(capsmi_session* s, const capsmi_table* t, int32_t nnodes, const capsmi_expr* prog,
               int64_t* out, uint8_t* out_valid, int32_t* out_type);
// the operand prog[lo .. hi] of a validated program as a column over t's rows: a single COL is read in place,
// anything else is evaluated into a temporary of the sub-program's static type
Column operand_column(capsmi_session* s, const capsmi_table* t, const capsmi_expr* prog, int lo, int hi);
// filter flags: 1 where the predicate is TRUE
void eval_predicate(capsmi_session* s, const capsmi_table* t, int32_t nnodes, const capsmi_expr* prog,
                    uint8_t* flags);

// sort (k_sort.hip): stable ascending permutation of row indices by a 64-bit key
void radix_sort_pairs(capsmi_session* s, uint64_t* keys, int64_t* vals, int64_t n, int begin_bit,
                      int end_bit);
// the same over an explicit list of 8-bit digit positions (LSD order; digits no key uses skipped);
// vals may be null (keys only)
void radix_sort_digits(capsmi_session* s, uint64_t* keys, int64_t* vals, int64_t n, const std::vector<int>& shifts);
// the same, calling cb(keys as they stand) on the stream after the first `at` passes (an intermediate
// order, e.g. by the low digits alone; cb(keys) at once when nothing is sorted)
void radix_sort_digits(capsmi_session* s, uint64_t* keys, int64_t* vals, int64_t n, const std::vector<int>& shifts,
                       int at, const std::function<void(const uint64_t*)>& cb);
// keys only; an odd number of passes leaves the result in the sort's other buffer, which `keys` then holds
// (no copy back).  Key-only sorts run in tiles of kSortTile keys: a producer that counts its keys' first digit
// per tile (hist0[d * ntiles + tile], int64, ntiles = ceil(n / kSortTile)) hands that over and the first pass
// skips its histogram read
constexpr int kSortTile = 4096;
void radix_sort_keys(capsmi_session* s, Buf& keys, int64_t n, const std::vector<int>& shifts,
                     const int64_t* hist0 = nullptr);
void order_keys(capsmi_session* s, const int64_t* col, const uint8_t* valid, int type, bool desc, bool null_pass,
                const int64_t* perm, int64_t n, uint64_t* key);

// partitioned relationship layout (k_part.hip)
struct PartLayout {
    int64_t lo, hi;  // id domain of both endpoints
    int nt;          // target slices of 2^19 ids (<= 2048)
    int ns;          // source slices of 2^sbits ids
    int sbits;       // 19 while nt * ns <= 16384, coarser for larger domains
    int ncells;      // nt * ns, j-major (target slice major)
    int tbits;       // target slice = 2^tbits ids (19 for the 2-hop layout)
    int packed = 0;  // 2-hop layout: 5-byte cell-relative pairs (sbits + tbits <= 40), else uint2
};
// Pass 1 of the partition plus chunk ordering and the block-balanced segment split (k_part.hip):
// relationships grouped by bucket = (y >> L.tbits) of their packed (x, y) = (source - lo, target - lo)
// pair, in chunks of kCh pairs; with `swap` the pair is (target, source) and buckets follow the
// source.  Blocks of a consumer kernel launched with g2 blocks walk segments via part::seg_of.
struct ChunkPart {
    PartLayout L;
    Buf pool, meta, chist, jbuf;
    bool split = false;          // the pool's chunks are two word arrays (part_common.h: split_t / split_s), not pairs
    bool has_hist = false;       // chist holds the chunks' cell-count rows (pass 1 with want_hist, or k_chunk_hist)
    int64_t pool_chunks = 0, npool = 1, mtot = 0, g2 = 1;
    int64_t* jst = nullptr;      // nt + 1 chunk offsets per bucket in `order`
    int64_t* segbase = nullptr;  // g2 + 1
    int* ja = nullptr;           // first bucket per block
    uint32_t* order = nullptr;   // used chunks grouped by bucket
};
// The 32-bit form of one table's endpoint columns as pass 1 reads it (Column::narrow of both columns, one base):
// s[i] = source[i] - base, d[i] = target[i] - base.  s == nullptr: the table is read as int64.
struct NarrowRel {
    const uint32_t* s = nullptr;
    const uint32_t* d = nullptr;
    int64_t base = 0;
};
// the narrow form of (source column sc, target column dc) if both carry one with one base and the knob allows
NarrowRel narrow_rel(const capsmi_session* s, const Column& sc, const Column& dc);
// One table's presence words as hop 1 reads them (PresenceWords): m = the to-column's side (`in` when the walk
// follows the relationships, `out` when it runs against them), l1 / l2 = the loop words, over the window [lo, hi).
// m == nullptr: the table offers none.
struct PresenceRel {
    const uint32_t* m = nullptr;
    const uint32_t* l1 = nullptr;
    const uint32_t* l2 = nullptr;
    int64_t lo = 0, hi = 0, nwords = 0;
    std::shared_ptr<const PresenceWords> keep;  // the words' owner (a handle that stores the PresenceRel keeps them alive)
};
// the words that the walk from column `from` to column `to` over `rows` rows may read: the to-column offers them
// when both columns' data blocks, both row offsets and the row count are the ones they were made with, and the
// knob allows
PresenceRel presence_rel(const capsmi_session* s, const Column& from, const Column& to, int64_t rows);
struct RelPart {
    PartLayout L;
    // The build has two stages.  Stage 1 (pass 1) leaves the chunk partition `cp`: pairs grouped by target
    // slice.  Stage 2 (relpart_cells: pass 2) turns it into the cells below and drops the pool.  A cold 2-hop
    // with a full a_ok runs both hops over the pool and never needs stage 2 (k_pool_hop1 / k_pool_hop2);
    // every reader of `pairs` / `boff` completes the cells first (relpart_cells is a no-op once built).
    ChunkPart cp;
    bool cells = false;
    int sel = -1;   // hop-2 form: -1 none ran yet, 0 the pool (no cells built), 1 the cells
    // per kept relationship, grouped by cell: uint2 (source - lo, target - lo), or when L.packed the
    // cell-relative key k = (source low sbits) << tbits | (target low tbits) as two arrays, the low
    // word u32[cap] and the high byte u8[cap] behind it
    Buf pairs;
    int64_t cap = 0;  // entries per array (kept + slack)
    Buf boff;   // int64 cell offsets (ncells + 1); boff[ncells] = kept
    int64_t kept = 0;  // -1: on the device only (relpart_kept reads it)
    int64_t rows = 0;  // relationships offered to the build (>= kept)
    // the presence words of the tables with rows, when every one of them offers words usable over L's domain
    // (else empty): relpart_hop1 with a full a reads them instead of the cells
    std::vector<PresenceRel> pres;
};
int64_t relpart_kept(capsmi_session* s, RelPart& rp);
void relpart_digest(capsmi_session* s, RelPart& rp, int64_t* counts, uint64_t* sums, int64_t* misplaced);
// hop 1 of a 2-hop run while the layout is built: M(t) |= a_ok(s) for s != t, a_ok self-loops ->
// S1 (first) / S2 (second), target filter b_ok; outputs zeroed by the caller
struct RelPartHop1 {
    const capsmi_bitmap* a;
    const capsmi_bitmap* b;
    uint32_t *M, *S1, *S2;
};
// unpacked: keep 8-byte pairs whatever the domain (a layout walked by kernels that read uint2 pairs only)
// nar: per table its 32-bit endpoint form (NarrowRel; null: none has one)
// pres: per table its presence words (PresenceRel; null: none has any).  Where every table with rows offers words
// usable over [lo, hi), a pool hop 1 is answered from them (k_presence_hop1) and the handle keeps them.
void relpart_build(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms, int nt,
                   int64_t lo, int64_t hi, RelPart& rp, const RelPartHop1* h1 = nullptr, bool unpacked = false,
                   const NarrowRel* nar = nullptr, const PresenceRel* pres = nullptr);
// stage 2 of the build on a handle that kept its pool (no-op when the cells are there)
void relpart_cells(capsmi_session* s, RelPart& rp);
void relpart_hop1(capsmi_session* s, RelPart& rp, const capsmi_bitmap* a, const capsmi_bitmap* b, uint32_t* M,
                  uint32_t* S1, uint32_t* S2);
void relpart_hop2(capsmi_session* s, RelPart& rp, const capsmi_bitmap* c, const uint32_t* X1, const uint32_t* X2,
                  uint32_t* C);

// fused cyclic triangle count (k_tri.hip): the oriented simple graph with multiplicities
struct TriGraph {
    int64_t lo = 0, n = 0, ne = 0;
    Buf ok, ov, off;  // oriented keys (from<<32|to), payload (m(from,to)<<32|m(to,from)), CSR offsets (n + 1)
    // uint32 targets of the oriented edges (the `to` of ok, ib bits) with the edge's two multiplicities
    // in cb bits each above it (all-ones: read ov); ids are the degree order (0 = highest (degree, id))
    Buf tg;
    int ib = 0, cb = 0;
    Buf orig;         // int64 per vertex: relative id of the degree-order id (unused by the count; the per-node rows' ids)
    Buf ek, ev, sl;   // undirected keys / payload (pair terms), self-loop counts
    bool sl_relative = false;  // sl is indexed by relative id (the sorted build, as its ek) -- else by degree-order id
    Buf pair;         // the direct build: the pair terms' sum (u64), added up while the runs are written
    Buf small_u, big_u;  // vertices with out-degree in [2, 64] / above 64
    int64_t nsmall = 0, nbig = 0;
    // Direction choice per oriented edge u -> v at position p of out(u) (out-lists are sorted, and
    // every wedge u -> v -> w that can close has w < v, so from v only the prefix out(u)[0, p) needs
    // walking; from u the whole out(v)): with vmt > 0 the edges with od(v) >= vmt and p < od(v) are
    // taken from v ("v-mode"), over the in-lists (ioff, itg, ipos: sources and positions p of the
    // oriented edges grouped by target; the edge is off[u] + p); vm_c = the v-mode centers.
    int vmt = 0;
    Buf ioff, itg, ipos, vm_c;
    // direction-split lists (k_tri.hip "direction-split lists"): tgs = every out_f(x) then every out_b(x),
    // fbo = their starts (2n + 2 uint32); with split set the in-lists are ikey (to << 40 | record index, sorted)
    // and irec (16-byte records: coded source word, pf | pb << 16, the source's f / b list starts) instead of
    // itg / ipos
    bool split = false;
    Buf tgs, fbo, ikey, irec;
    Buf vrec;  // per vertex {f start, b start, f len | b len << 16, od} (k_vrec): one load per list setup
    int64_t nvm = 0;
    // ek / ev entries (= ne on one device; on a rank of a distributed build the undirected edges whose
    // lower end it owns, while ok / tg hold every oriented edge)
    int64_t nek = 0;
    bool dist = false;
    // tri_count's part p of P takes every P-th center of big_u / vm_c / small_u from p (interleaved shares);
    // a distributed build's in-lists hold only the v-mode centers v with v mod world = rank, so vm_c is
    // exactly its share
    bool vm_own = false;
};
// a distributed build (multi-GPU C4): this rank's relationships are any 1/world of them; the owner of a
// dense id x is x / span
struct TriDist {
    int rank = 0, world = 1;
    int64_t span = 0;
};
void tri_build(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms, int nt,
               const capsmi_bitmap* n_ok, TriGraph& g, const TriDist* dd = nullptr);
uint64_t tri_count(capsmi_session* s, const TriGraph& g, int part, int nparts);
// the closed triangle's shapes over a single-device trigraph (k_tri_nodes.hip): the cycle (a)->(b)->(c)->(a), the
// transitive triangle (a)->(b)->(c)<-(a) and the undirected one (a)-(b)-(c)-(a)
enum class TriShape { cycle, transitive, undirected };
// count(*) of the transitive or the undirected triangle (the latter in the form cfg.tri_und_hash selects; the
// cycle's is tri_count)
uint64_t tri_shape_count(capsmi_session* s, const TriGraph& g, TriShape shape);
// the count grouped by one node: rows (relative id, count) of the nodes with a non-zero count, unordered; returns
// their number.  cls: the transitive triangle's role (CAPSMI_TRI_ROLE_*), the undirected one's position class
// (CAPSMI_TRI_UND_*); the cycle takes none (the same rows at every position)
int64_t tri_shape_count_by_node(capsmi_session* s, const TriGraph& g, TriShape shape, int cls, Buf& ids, Buf& counts);
// the undirected count's hash walks (k_tri.hip), which add sum U U U over the simple triangles to the device word *out
void tri_und_hash_walk(capsmi_session* s, const TriGraph& g, unsigned long long* out);

// undirected Expand patterns (k_undirected.hip): hops 1 or 2; kind 0 count(*), 1 count(DISTINCT end),
// 2 count(DISTINCT start); c unused for one hop.  marks (kinds 1, 2; b's nwords words): the distinct ids'
// bitmap is written there instead of counted (returns 0) -- a rank's partial marks of a distributed route
int64_t undirected_count(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                         int nt, int hops, const capsmi_bitmap* a, const capsmi_bitmap* b, const capsmi_bitmap* c,
                         int kind, uint32_t* marks = nullptr);
// the undirected 2-hop count(DISTINCT end) over the 2-D cell layout (k_und_part.hip), domains of at most
// 2^26 ids (undirected_distinct_part_ok); marks as above
bool undirected_distinct_part_ok(int64_t n);
int64_t undirected_distinct_part(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts,
                                 const int64_t* ms, int nt, const capsmi_bitmap* a, const capsmi_bitmap* b,
                                 const capsmi_bitmap* c, uint32_t* marks);

// the 2-hop chain grouped by its start (k_grouped.hip): rows (relative start id, count(*) or count(DISTINCT
// end)); false when the distinct keys would exceed key_budget bytes
// dd (a rank of a distributed graph, BY_SOURCE shards: sources owned, dense ids [rank * span, (rank + 1) *
// span) owned): the rows of the owned starts, outC / the hop-2 lists exchanged between the ranks
struct GroupedDist {
    int rank = 0, world = 1;
    int64_t span = 0;
};
bool grouped_two_hop(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                     int nt, const capsmi_bitmap* a, const capsmi_bitmap* b, const capsmi_bitmap* c, bool distinct,
                     int64_t key_budget, Buf& out_ids, Buf& out_vals, int64_t* rows, const GroupedDist* dd = nullptr);

// fused var-length grouped count (k_varlen.hip)
int64_t var_length_count(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                         int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper,
                         Buf& out_ids, Buf& out_cnt, const NarrowRel* nar = nullptr);

// var-length count(DISTINCT b), lower in {0, 1}: k-hop reach by bit-parallel BFS (k_reach.hip).  Rows (a, |D(a)|)
// of the a_ok nodes with a non-empty D(a) (returns the row count), and |U_a D(a)|.
int64_t var_length_reach_rows(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                              int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper,
                              Buf& out_ids, Buf& out_cnt, const NarrowRel* nar = nullptr);
int64_t var_length_reach_count(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts,
                               const int64_t* ms, int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower,
                               int upper, const NarrowRel* nar = nullptr);
// var-length collect(DISTINCT b) (k_reach.hip): the rows above with D(a) itself, read off each batch's bit matrix.
// List k of `lists` is D of the k-th a_ok node in id order, strictly ascending absolute ids (empty lists included,
// which no row names); out_sel holds the rows' list indices.  CAPSMI_REACH_LIST_LIMIT bounds the elements.
// Remapped ids (orig != null: orig[d] is the original id of dense id lo + d, all distinct; ord their order): the
// lists hold original ids, ascending by signed value, and out_ids the sources' original ids; rows and lists stay
// in dense order of the sources.
int64_t var_length_reach_lists(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                               int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper,
                               Buf& out_ids, Buf& out_cnt, Buf& out_sel, std::shared_ptr<ListStore>& lists,
                               const NarrowRel* nar = nullptr, const int64_t* orig = nullptr, const IdOrder* ord = nullptr);
// the global form: U_a D(a) as ascending absolute ids (returns their number); ord: as ascending original ids
int64_t var_length_reach_list(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts, const int64_t* ms,
                              int nt, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int lower, int upper,
                              Buf& out_vals, const NarrowRel* nar = nullptr, const IdOrder* ord = nullptr);
// the order of n original ids (signed, ORDER BY's key image and radix sort); *dup (if given): two ids are equal
std::shared_ptr<const IdOrder> id_order_build(capsmi_session* s, const int64_t* orig, int64_t n, bool* dup = nullptr);
// the two collect entries behind the C interface and the route: orig / ord null for plain ids
void var_length_collect_table(capsmi_session* s, int32_t nrels, capsmi_table* const* rels, const char* src_col,
                              const char* dst_col, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int32_t lower,
                              int32_t upper, const char* id_name, const char* list_name, const char* count_name,
                              const int64_t* orig, const IdOrder* ord, capsmi_table** out);
void var_length_reach_list_table(capsmi_session* s, int32_t nrels, capsmi_table* const* rels, const char* src_col,
                                 const char* dst_col, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int32_t lower,
                                 int32_t upper, const char* list_name, const IdOrder* ord, capsmi_table** out);
// sharded var-length grouped count (multi-GPU C5; k_varlen.hip): begin -> caller sums od over ranks
// -> mid -> caller sums Y -> finish (rows of owned ids)
struct VarlenShard;
VarlenShard* varlen_shard_begin(capsmi_session* s, const int64_t* const* srcs, const int64_t* const* dsts,
                                const int64_t* ms, int nt, const int64_t* const* isrcs, const int64_t* const* idsts,
                                const int64_t* ims, int nin, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok,
                                int lower, int upper, int64_t own_lo, int64_t own_hi, int64_t* od);
void varlen_shard_mid(VarlenShard* v, int64_t* y);
int64_t varlen_shard_finish(VarlenShard* v, Buf& out_ids, Buf& out_cnt);
void varlen_shard_free(VarlenShard* v);

// [min, max] over `ncols` int64 columns of n rows into out[0], out[1] (synchronises); n > 0
void minmax_i64(capsmi_session* s, const int64_t* const* cols, int ncols, int64_t n, int64_t* out);
// oa[i] = a[i] - base and ob[i] = b[i] - base as 32-bit words for n rows, one pass on the session's stream
// (the endpoint columns' narrow copies; the caller has checked that every difference fits)
void narrow_pair_i64(capsmi_session* s, const int64_t* a, const int64_t* b, int64_t n, int64_t base, uint32_t* oa,
                     uint32_t* ob);
// widen n input values of width `code` (CAPSMI_IN_* of include/capsmi.h) to 8-byte words
void widen_words(const void* in, int code, int64_t* out, int64_t n, hipStream_t st);

// expressions (k_expr.hip; the arity table, the sub-tree walk and check_program itself: expr_prog.h).
// check_program over t's column types: throws what it refuses, returns the program's static type
int32_t validate_program(const capsmi_table* t, int32_t nn, const capsmi_expr* prog);
// a program with every CAPSMI_X_PARAM replaced by its literal(s) from the session's parameters
std::vector<capsmi_expr> bind_params(const capsmi_session* s, int32_t nn, const capsmi_expr* prog);
bool has_params(int32_t nn, const capsmi_expr* prog);

// lazy plans (plan.hip): run the plan (a fused kernel when the recogniser matches) and keep the result
void materialize(capsmi_table* t);
// mark a materialised table in canonical entity layout (ids first) as a node (1) / relationship (2)
// table whose ids (endpoints) lie in [lo, hi)
void attach_entity(capsmi_table* t, int kind, int64_t lo, int64_t hi, bool ids_exact = false, bool ids_unique = false);
inline capsmi_table* M(const capsmi_table* t) {
    materialize(const_cast<capsmi_table*>(t));
    return const_cast<capsmi_table*>(t);
}

// eager Table[T] operators over materialised inputs (api.hip)
capsmi_status eager_select(capsmi_table* t, int32_t ncols, const char* const* cols, capsmi_table** out);
capsmi_status eager_drop(capsmi_table* t, int32_t ncols, const char* const* cols, capsmi_table** out);
capsmi_status eager_with_column_renamed(capsmi_table* t, const char* old_name, const char* new_name, capsmi_table** out);
capsmi_status eager_filter(capsmi_table* t, int32_t nnodes, const capsmi_expr* prog, capsmi_table** out);
capsmi_status eager_filter_keep(capsmi_table* t, int32_t nnodes, const capsmi_expr* prog,
                                const std::vector<std::string>& keep, capsmi_table** out);
capsmi_status eager_with_columns(capsmi_table* t, int32_t ncols, const capsmi_expr_column* cols, capsmi_table** out);
capsmi_status eager_join(capsmi_table* l, capsmi_table* r, int32_t join_type, int32_t npairs, const char* const* lcols,
                         const char* const* rcols, capsmi_table** out);
capsmi_status eager_union_all(capsmi_table* a, capsmi_table* b, capsmi_table** out);
capsmi_status eager_order_by(capsmi_table* t, int32_t nkeys, const char* const* cols, const int32_t* descending,
                             capsmi_table** out);
capsmi_status eager_skip(capsmi_table* t, int64_t n, capsmi_table** out);
capsmi_status eager_limit(capsmi_table* t, int64_t n, capsmi_table** out);
capsmi_status eager_distinct(capsmi_table* t, capsmi_table** out);
capsmi_status eager_distinct_on(capsmi_table* t, int32_t ncols, const char* const* cols, capsmi_table** out);
capsmi_status eager_group(capsmi_table* t, int32_t nby, const char* const* by, int32_t naggs, const capsmi_agg* aggs,
                          capsmi_table** out);
// keep: the output columns to produce (null: all) -- payload columns outside it are not gathered
capsmi_status eager_explode(capsmi_table* t, const char* list_col, const char* item_name,
                            const std::vector<std::string>* keep, capsmi_table** out);
capsmi_status eager_explode_values(capsmi_table* t, int32_t elem_type, int32_t count, const capsmi_value* values,
                                   const char* item_name, const std::vector<std::string>* keep, capsmi_table** out);
// programs over t's columns; step empty: the literal 1
capsmi_status eager_with_range_column(capsmi_table* t, const std::vector<capsmi_expr>& from,
                                      const std::vector<capsmi_expr>& to, const std::vector<capsmi_expr>& step,
                                      const char* name, capsmi_table** out);
// the list of codes[i] for every column cols[i] of t that passes under `mode` (capsmi_with_mask_list_column)
capsmi_status eager_with_mask_list_column(capsmi_table* t, int32_t mode, const std::vector<std::string>& cols,
                                          const std::vector<int64_t>& codes, const char* name, capsmi_table** out);

// CSV ingest (ingest.hip)
capsmi_table* read_csv(capsmi_session* s, const std::vector<std::string>& paths, char delim, char comment,
                       const std::vector<std::string>& names, const std::vector<int32_t>& types, capsmi_intern_fn intern,
                       void* ctx, const char* row_id_col);

// graph (k_graph.hip)
// node predicate compiled for the bitmap scan: AND of range tests on Long columns (k_graph.hip)
constexpr int kMaxRangeTerms = 4;
struct RangePred {
    int n = 0;
    const int64_t* col[kMaxRangeTerms];
    const uint8_t* valid[kMaxRangeTerms];
    int64_t lo[kMaxRangeTerms], hi[kMaxRangeTerms];  // inclusive
};
// compile `prog` over table t (AND of comparisons Long column <op> Long literal); false if not of that form
bool compile_range_pred(const capsmi_table* t, int32_t nn, const capsmi_expr* prog, RangePred& rp);
void bitmap_add_rows(capsmi_bitmap* b, const int64_t* ids, const uint8_t* ids_valid, const uint8_t* flags, int64_t n,
                     int64_t* dev_counters, const RangePred* rp = nullptr);
void bitmap_set_range(capsmi_bitmap* b, int64_t b0, int64_t b1);  // bits [b0, b1) of the window
int64_t words_popcount(capsmi_session* s, const uint32_t* w, int64_t w_begin, int64_t w_end);
void words_popcount_async(capsmi_session* s, const uint32_t* w, int64_t w_begin, int64_t w_end, int64_t* dev_out);

}  // namespace capsmi
