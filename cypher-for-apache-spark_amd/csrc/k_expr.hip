// k_expr.hip -- row-wise evaluation of postfix expression programs.
//
// Restates the predicate subset of SparkSQLExprMapper.asSparkSQLExpr
// (spark-cypher/src/main/scala/org/opencypher/spark/impl/SparkSQLExprMapper.scala:81-312)
// with Spark SQL three-valued logic:
//   - comparisons with a NULL operand are NULL; comparisons between incomparable
//     types (Long vs String, ...) are NULL (Spark casts the string and gets null);
//   - a Long compared with a Double is cast to Double first (2^53 + 1 = 2^53.0 is TRUE);
//   - NaN follows Spark SQL's documented "NaN Semantics": NaN = NaN is TRUE and NaN is greater
//     than every other number, for = <> < <= > >= and IN alike (any sign, any payload is one NaN);
//     a comparison with NaN is therefore never NULL unless an operand is NULL;
//   - NOT NULL = NULL; AND: any FALSE -> FALSE, else any NULL -> NULL; OR dually;
//   - x IN (..): TRUE on a match, else NULL if x or any element is NULL, else FALSE;
//   - Filter keeps a row iff the value is TRUE (SparkTable.scala:65-67; pinned by
//     PredicateBehaviour.scala:131-149);
//   - bitwise and shift operators on Long (the id-tag expressions of Tags.scala:101-123), NULL in ->
//     NULL out; CASE takes the first alternative whose predicate is TRUE (a NULL predicate is not);
//   - list columns (SparkSQLExprMapper.scala:124-130 Size, :300-307 ContainerIndex, :138-145 In): a column
//     reference to a list column pushes the row's list; size() and list[i] read the store's offsets and one value
//     here; x IN list is lowered on the host (lower_in_list below) to a column that k_listexpr.hip computes over
//     all the rows' elements before this interpreter runs.  No other opcode takes a list.
//   - STARTS WITH / ENDS WITH / CONTAINS (SparkSQLExprMapper.scala:152-157) are lowered on the host the same way
//     (lower_str_match below): k_strmatch.hip matches the bytes of the session's string store.
//   - size(), toInteger(), toFloat() and toBoolean() of a String (:124-127, :231, :229, :235) are lowered likewise
//     (lower_str_conv below): k_strconv.hip reads the store's bytes, and the interpreter never sees these opcodes.
//   - toString() (:233) and Add over a String (:160-181, functions.concat) make Strings (lower_str_make below):
//     k_strmake.hip formats one string per distinct operand tuple and the session's string sink gives the codes.
//   - Divide (:186), Sqrt .. Sign (:249-260), ToFloat / ToInteger (:229-231): eval_math below, with the rules of the
//     Spark 2.2.1 Column calls the mapper makes (include/capsmi.h states them per opcode).  Double log and exp are
//     library code of some size, so these cases exist only in the kMath instantiation of the interpreter, which
//     launch_eval takes for a program that holds one of them; every other program runs the code it ran before.
//   - MonotonicallyIncreasingId (:189): CAPSMI_X_ROW_ID pushes the row's index, which the interpreter holds anyway.
//     Legal only under capsmi_with_columns, whose plan node it pins (plan.hip).
#include "capsmi_impl.h"
#include "str_make.h"

namespace capsmi {

namespace {

constexpr int8_t kNull = -1;  // kMaxStack, kMaxCols: expr_prog.h

struct ColPtrs {
    const int64_t* data[kMaxCols];
    const uint8_t* valid[kMaxCols];
    int8_t type[kMaxCols];
    const int64_t* loff[kMaxCols];  // list columns: the store's offsets and values
    const int64_t* lval[kMaxCols];
};

struct Val {
    int64_t b;
    int8_t t;  // CAPSMI_* or kNull
    int8_t c;  // a list value (t >= CAPSMI_LIST): the column whose store b indexes
};

__device__ __forceinline__ bool numeric(int8_t t) { return t == CAPSMI_I64 || t == CAPSMI_F64; }
__device__ __forceinline__ double as_f64(const Val& v) {
    return v.t == CAPSMI_F64 ? __longlong_as_double(v.b) : (double)v.b;
}

// -2: incomparable / null, else -1, 0, 1
__device__ __forceinline__ int cmp3(const Val& a, const Val& b) {
    if (a.t == kNull || b.t == kNull) return -2;
    if (numeric(a.t) && numeric(b.t)) {
        if (a.t == CAPSMI_I64 && b.t == CAPSMI_I64) return a.b < b.b ? -1 : (a.b > b.b ? 1 : 0);
        const double x = as_f64(a), y = as_f64(b);
        const bool xn = x != x, yn = y != y;  // NaN = NaN, and NaN is greater than any other number
        if (xn || yn) return xn == yn ? 0 : (xn ? 1 : -1);
        return x < y ? -1 : (x > y ? 1 : 0);
    }
    if (a.t != b.t) return -2;
    return a.b < b.b ? -1 : (a.b > b.b ? 1 : 0);
}

__device__ __forceinline__ Val mk_bool(bool x) { return Val{x ? 1 : 0, (int8_t)CAPSMI_BOOL}; }
__device__ __forceinline__ Val mk_null() { return Val{0, kNull}; }

// Java's (long) d, which Spark's casts and its Long-valued Ceil / Floor apply: 0 for NaN, saturating, else toward
// zero.  (A bare C++ cast is undefined outside the Long range.)
__device__ __forceinline__ int64_t sat_i64(double d) {
    if (d != d) return 0;
    if (d >= 9223372036854775808.0) return INT64_MAX;
    if (d <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)d;
}

__device__ __forceinline__ Val mk_f64(double d) { return Val{__double_as_longlong(d), (int8_t)CAPSMI_F64}; }
__device__ __forceinline__ Val mk_i64(int64_t v) { return Val{v, (int8_t)CAPSMI_I64}; }

// CAPSMI_X_DIV (a / b) and the one-operand numeric opcodes (a).  A NULL or non-numeric operand: NULL.
__device__ Val eval_math(int32_t op, const Val& a, const Val& b) {
    if (!numeric(a.t) || (op == CAPSMI_X_DIV && !numeric(b.t))) return mk_null();
    const bool is_long = a.t == CAPSMI_I64;
    const double x = as_f64(a);
    switch (op) {
        case CAPSMI_X_DIV: {  // Spark's Division works on doubles; a zero divisor (either sign) is NULL
            const double q = as_f64(b);
            if (q == 0.0) return mk_null();
            const double d = x / q;
            return is_long && b.t == CAPSMI_I64 ? mk_i64(sat_i64(d)) : mk_f64(d);
        }
        case CAPSMI_X_SQRT: return mk_f64(sqrt(x));
        case CAPSMI_X_LOG: return x <= 0.0 ? mk_null() : mk_f64(log(x));
        case CAPSMI_X_LOG10: return x <= 0.0 ? mk_null() : mk_f64(log(x) / 2.302585092994046);  // Logarithm(10.0, x)
        case CAPSMI_X_EXP: return mk_f64(exp(x));
        case CAPSMI_X_ABS:
            if (is_long) return mk_i64(a.b < 0 ? (int64_t)(0ULL - (uint64_t)a.b) : a.b);  // wraps at Long.MIN
            return Val{a.b & INT64_MAX, (int8_t)CAPSMI_F64};
        case CAPSMI_X_CEIL: return mk_f64(is_long ? x : (double)sat_i64(ceil(x)));
        case CAPSMI_X_FLOOR: return mk_f64(is_long ? x : (double)sat_i64(floor(x)));
        case CAPSMI_X_ROUND: {  // HALF_UP through BigDecimal: no signed zero; NaN and the infinities stay
            if (is_long || x != x || x - x != 0.0) return mk_f64(x);
            const double r2 = round(x);
            return mk_f64(r2 == 0.0 ? 0.0 : r2);
        }
        case CAPSMI_X_SIGN: return mk_i64((x > 0.0) - (x < 0.0));
        case CAPSMI_X_TO_FLOAT: return mk_f64(x);
        default: {  // CAPSMI_X_TO_INTEGER: Spark's 32-bit IntegerType, held as a Long
            if (is_long) return mk_i64((int64_t)(int32_t)(uint32_t)(uint64_t)a.b);
            if (x != x) return mk_i64(0);
            if (x >= 2147483647.0) return mk_i64(INT32_MAX);
            if (x <= -2147483648.0) return mk_i64(INT32_MIN);
            return mk_i64((int64_t)(int32_t)x);
        }
    }
}

template <bool kMath>
__device__ Val eval_row(const capsmi_expr* __restrict__ prog, int nn, const ColPtrs& cp, int64_t r) {
    Val st[kMaxStack];
    int sp = 0;
    for (int i = 0; i < nn; ++i) {
        const capsmi_expr x = prog[i];
        switch (x.op) {
            case CAPSMI_X_COL: {
                const int c = x.arg;
                const bool ok = cp.valid[c] == nullptr || cp.valid[c][r];
                st[sp++] = ok ? Val{cp.data[c][r], cp.type[c], (int8_t)c} : mk_null();
                break;
            }
            case CAPSMI_X_LIT: st[sp++] = Val{x.ival, (int8_t)x.type}; break;
            case CAPSMI_X_NULL: st[sp++] = mk_null(); break;
            case CAPSMI_X_ROW_ID: st[sp++] = mk_i64(r); break;  // the views of replace_span_and_eval keep the rows
            case CAPSMI_X_EQ: case CAPSMI_X_NEQ: case CAPSMI_X_LT: case CAPSMI_X_LE: case CAPSMI_X_GT: case CAPSMI_X_GE: {
                const Val b = st[--sp], a = st[--sp];
                const int c = cmp3(a, b);
                if (c == -2) { st[sp++] = mk_null(); break; }
                bool res = false;
                switch (x.op) {
                    case CAPSMI_X_EQ: res = c == 0; break;
                    case CAPSMI_X_NEQ: res = c != 0; break;
                    case CAPSMI_X_LT: res = c < 0; break;
                    case CAPSMI_X_LE: res = c <= 0; break;
                    case CAPSMI_X_GT: res = c > 0; break;
                    default: res = c >= 0; break;
                }
                st[sp++] = mk_bool(res);
                break;
            }
            case CAPSMI_X_NOT: {
                const Val a = st[--sp];
                st[sp++] = a.t == kNull ? mk_null() : mk_bool(a.b == 0);
                break;
            }
            case CAPSMI_X_AND: case CAPSMI_X_OR: {
                const bool is_and = x.op == CAPSMI_X_AND;
                bool any_null = false, decided = false;
                for (int k = 0; k < x.arg; ++k) {
                    const Val a = st[--sp];
                    if (a.t == kNull) any_null = true;
                    else if (is_and ? a.b == 0 : a.b != 0) decided = true;
                }
                if (decided) st[sp++] = mk_bool(!is_and);
                else if (any_null) st[sp++] = mk_null();
                else st[sp++] = mk_bool(is_and);
                break;
            }
            case CAPSMI_X_ISNULL: { const Val a = st[--sp]; st[sp++] = mk_bool(a.t == kNull); break; }
            case CAPSMI_X_ISNOTNULL: { const Val a = st[--sp]; st[sp++] = mk_bool(a.t != kNull); break; }
            case CAPSMI_X_IN: {
                bool hit = false, any_null = false;
                const Val v = st[sp - x.arg - 1];
                for (int k = 0; k < x.arg; ++k) {
                    const int c = cmp3(v, st[sp - x.arg + k]);
                    if (c == 0) hit = true;
                    else if (c == -2) any_null = true;
                }
                sp -= x.arg + 1;
                st[sp++] = hit ? mk_bool(true) : (any_null || v.t == kNull ? mk_null() : mk_bool(false));
                break;
            }
            case CAPSMI_X_ADD: case CAPSMI_X_SUB: case CAPSMI_X_MUL: {
                const Val b = st[--sp], a = st[--sp];
                if (a.t == kNull || b.t == kNull || !numeric(a.t) || !numeric(b.t)) { st[sp++] = mk_null(); break; }
                if (a.t == CAPSMI_I64 && b.t == CAPSMI_I64) {
                    const uint64_t ua = (uint64_t)a.b, ub = (uint64_t)b.b;  // Spark Long arithmetic wraps
                    const uint64_t r2 = x.op == CAPSMI_X_ADD ? ua + ub : (x.op == CAPSMI_X_SUB ? ua - ub : ua * ub);
                    st[sp++] = Val{(int64_t)r2, (int8_t)CAPSMI_I64};
                } else {
                    const double p = as_f64(a), q = as_f64(b);
                    const double r2 = x.op == CAPSMI_X_ADD ? p + q : (x.op == CAPSMI_X_SUB ? p - q : p * q);
                    st[sp++] = Val{__double_as_longlong(r2), (int8_t)CAPSMI_F64};
                }
                break;
            }
            case CAPSMI_X_NEG: {
                const Val a = st[--sp];
                if (a.t == CAPSMI_I64) st[sp++] = Val{(int64_t)(0ULL - (uint64_t)a.b), (int8_t)CAPSMI_I64};
                else if (a.t == CAPSMI_F64) st[sp++] = Val{__double_as_longlong(-__longlong_as_double(a.b)), (int8_t)CAPSMI_F64};
                else st[sp++] = mk_null();
                break;
            }
            case CAPSMI_X_COALESCE: {
                Val res = mk_null();
                for (int k = 0; k < x.arg; ++k) {
                    const Val a = st[sp - x.arg + k];
                    if (res.t == kNull && a.t != kNull) res = a;
                }
                sp -= x.arg;
                st[sp++] = res;
                break;
            }
            case CAPSMI_X_BITAND: case CAPSMI_X_BITOR: case CAPSMI_X_SHL: case CAPSMI_X_SHRU: {
                const Val b = st[--sp], a = st[--sp];
                if (a.t != CAPSMI_I64 || b.t != CAPSMI_I64) { st[sp++] = mk_null(); break; }
                const uint64_t ua = (uint64_t)a.b, ub = (uint64_t)b.b;
                uint64_t r2;
                switch (x.op) {
                    case CAPSMI_X_BITAND: r2 = ua & ub; break;
                    case CAPSMI_X_BITOR: r2 = ua | ub; break;
                    case CAPSMI_X_SHL: r2 = ua << (ub & 63); break;  // Java long shift semantics
                    default: r2 = ua >> (ub & 63); break;
                }
                st[sp++] = Val{(int64_t)r2, (int8_t)CAPSMI_I64};
                break;
            }
            case CAPSMI_X_CASE: {
                const int base = sp - (2 * x.arg + 1);
                Val res = st[sp - 1];  // default
                for (int k = x.arg - 1; k >= 0; --k) {  // the first TRUE predicate wins
                    const Val p = st[base + 2 * k];
                    if (p.t == CAPSMI_BOOL && p.b != 0) res = st[base + 2 * k + 1];
                }
                sp = base;
                st[sp++] = res;
                break;
            }
            case CAPSMI_X_SIZE: {
                const Val a = st[--sp];
                if (a.t < CAPSMI_LIST) { st[sp++] = mk_null(); break; }
                const int64_t* off = cp.loff[a.c];
                st[sp++] = Val{off[a.b + 1] - off[a.b], (int8_t)CAPSMI_I64};
                break;
            }
            case CAPSMI_X_INDEX: {
                const Val i = st[--sp], a = st[--sp];
                if (a.t < CAPSMI_LIST || i.t != CAPSMI_I64) { st[sp++] = mk_null(); break; }
                const int64_t* off = cp.loff[a.c];
                const int64_t lo = off[a.b], size = off[a.b + 1] - lo;
                if (i.b < 0 || i.b >= size) { st[sp++] = mk_null(); break; }  // GetArrayItem: no counting from the end
                st[sp++] = Val{cp.lval[a.c][lo + i.b], (int8_t)(a.t - CAPSMI_LIST)};
                break;
            }
            default:
                if constexpr (kMath) {
                    if (is_math_op(x.op)) {
                        const Val b = x.op == CAPSMI_X_DIV ? st[--sp] : mk_null(), a = st[--sp];
                        st[sp++] = eval_math(x.op, a, b);
                        break;
                    }
                }
                st[sp++] = mk_null();
                break;
        }
    }
    return sp > 0 ? st[sp - 1] : mk_null();
}

template <bool kMath>
__global__ void k_eval(const capsmi_expr* __restrict__ prog, int nn, ColPtrs cp, int64_t n, int64_t* __restrict__ out,
                       uint8_t* __restrict__ out_valid, uint8_t* __restrict__ flags) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        const Val v = eval_row<kMath>(prog, nn, cp, r);
        if (flags) flags[r] = (v.t == CAPSMI_BOOL && v.b != 0) ? 1 : 0;
        if (out) out[r] = v.t == kNull ? 0 : v.b;
        if (out_valid) out_valid[r] = v.t == kNull ? 0 : 1;
    }
}

}  // namespace

// check_program (expr_prog.h) over t's column types
int32_t validate_program(const capsmi_table* t, int32_t nn, const capsmi_expr* prog) {
    std::vector<int32_t> types;
    types.reserve(t->cols.size());
    for (const Column& c : t->cols) types.push_back(c.type);
    return check_program(types.data(), (int)types.size(), nn, prog);
}

bool has_params(int32_t nn, const capsmi_expr* prog) {
    for (int i = 0; i < nn; ++i)
        if (prog[i].op == CAPSMI_X_PARAM) return true;
    return false;
}

// Param(name) -> functions.lit(parameters(name)) (SparkSQLExprMapper.scala:86-92).  Each stack entry
// of the postfix program is tracked with the number of values it stands for: 1, or a list
// parameter's length, which only IN may consume (its element count grows by the list's values).
std::vector<capsmi_expr> bind_params(const capsmi_session* s, int32_t nn, const capsmi_expr* prog) {
    std::vector<capsmi_expr> out;
    std::vector<int> width;  // per stack entry: values it contributes (-1 - k: a list of k values)
    auto lit = [](int32_t type, const capsmi_value& v) {
        capsmi_expr x{};
        if (v.is_null) {
            x.op = CAPSMI_X_NULL;
            x.arg = type + 1;
        } else {
            x.op = CAPSMI_X_LIT;
            x.type = type;
            x.ival = v.ival;
        }
        return x;
    };
    for (int i = 0; i < nn; ++i) {
        const capsmi_expr& x = prog[i];
        if (x.op == CAPSMI_X_PARAM) {
            REQUIRE(x.arg >= 0 && x.arg < (int)s->params.size(), CAPSMI_ERR_ILLEGAL_ARGUMENT,
                    "expression parameter " + std::to_string(x.arg) + " is not set (capsmi_session_set_params)");
            const capsmi_session::Param& p = s->params[x.arg];
            if (!p.list) {
                out.push_back(lit(p.type, p.values[0]));
                width.push_back(1);
            } else {
                for (const capsmi_value& v : p.values) out.push_back(lit(p.type, v));
                width.push_back(-1 - (int)p.values.size());
            }
            continue;
        }
        const int pops = expr_pops(x);
        REQUIRE(known_expr_op(x.op), CAPSMI_ERR_NOT_IMPLEMENTED, "unknown expression op " + std::to_string(x.op));
        REQUIRE(pops >= 0 && (int)width.size() >= pops, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                "malformed expression program (stack underflow)");
        capsmi_expr y = x;
        if (x.op == CAPSMI_X_IN) {
            const size_t first = width.size() - pops;  // the tested value, then the elements
            REQUIRE(width[first] == 1, CAPSMI_ERR_ILLEGAL_ARGUMENT, "a list parameter is not a single value");
            int n = 0;
            for (size_t k = first + 1; k < width.size(); ++k) n += width[k] >= 0 ? width[k] : -1 - width[k];
            y.arg = n;
        } else {
            for (size_t k = width.size() - pops; k < width.size(); ++k)
                REQUIRE(width[k] == 1, CAPSMI_ERR_ILLEGAL_ARGUMENT, "a list parameter may only be an element of IN");
        }
        width.resize(width.size() - pops);
        width.push_back(1);
        out.push_back(y);
    }
    return out;
}

namespace {

int32_t launch_eval(capsmi_session* s, const capsmi_table* t, int32_t nn, const capsmi_expr* prog, int64_t* out,
                    uint8_t* out_valid, uint8_t* flags);

// What a node that ran as a pass of its own leaves in the program: a constant, or the BOOL column the pass wrote.
struct Lowered {
    int first;        // the node's sub-range of the program is [first .. at]
    capsmi_expr ref;  // the constant, where there is no column
    Column res;       // the column (res.data is set)
};

Lowered lowered_null(int first) {
    Lowered l{first, {}, {}};
    l.ref.op = CAPSMI_X_NULL;
    l.ref.arg = CAPSMI_BOOL + 1;
    return l;
}

Lowered lowered_column(capsmi_session* s, int first, int64_t n, const char* name, int32_t type = CAPSMI_BOOL) {
    Lowered l{first, {}, {}};
    l.res.name = name;
    l.res.type = type;
    l.res.data = dev_alloc(sizeof(int64_t) * n, s);
    l.res.valid = dev_alloc(n, s);
    return l;
}

// The sub-range [l.first .. at] of prog becomes l's constant, or a reference to l's column in a view of t that holds
// it, and the interpreter evaluates the rest over the view.  Further such nodes are lowered by the recursion.
void replace_span_and_eval(capsmi_session* s, const capsmi_table* t, int32_t nn, const capsmi_expr* prog, int at,
                           Lowered& l, int64_t* out, uint8_t* out_valid, uint8_t* flags) {
    capsmi_table view;
    view.sess = s;
    view.nrows = t->nrows;
    view.cols = t->cols;
    if (l.res.data) {
        l.ref.op = CAPSMI_X_COL;
        l.ref.arg = (int32_t)view.cols.size();
        if (l.ref.arg < kMaxCols) {
            view.cols.push_back(std::move(l.res));
        } else {  // a table at the interpreter's column limit: the view lends a column the rest does not read
            std::vector<bool> used(kMaxCols, false);
            for (int i = 0; i < nn; ++i)
                if ((i < l.first || i > at) && prog[i].op == CAPSMI_X_COL) used[prog[i].arg] = true;
            int slot = 0;
            while (slot < kMaxCols && used[slot]) ++slot;
            REQUIRE(slot < kMaxCols, CAPSMI_ERR_NOT_IMPLEMENTED,
                    std::string(prog[at].op == CAPSMI_X_IN_LIST
                                    ? "IN over a list column"
                                    : (is_str_conv(prog[at].op)
                                           ? "a function of a String's characters"
                                           : (is_str_make(prog[at].op) ? "a function that makes a String" : "a string match"))) +
                        " in a program that reads 64 columns");
            l.ref.arg = slot;
            view.cols[slot] = std::move(l.res);
        }
    }
    std::vector<capsmi_expr> low(prog, prog + l.first);
    low.push_back(l.ref);
    low.insert(low.end(), prog + at + 1, prog + nn);
    launch_eval(s, &view, (int32_t)low.size(), low.data(), out, out_valid, flags);
}

// x IN list (node `at`; its list operand is the column reference before it): the probe is an operand_column,
// k_listexpr.hip's load-balanced pass produces the BOOL column.  A NULL list: NULL without a kernel.
Lowered lower_in_list(capsmi_session* s, const capsmi_table* t, const capsmi_expr* prog, int at) {
    const auto span = operand_spans(prog, at);  // the probe, the list
    const capsmi_expr& lx = prog[at - 1];
    if (lx.op == CAPSMI_X_NULL) return lowered_null(span[0].first);
    const Column& lc = t->cols[lx.arg];
    const Column probe = operand_column(s, t, prog, span[0].first, span[0].second);
    Lowered l = lowered_column(s, span[0].first, t->nrows, "__in_list");
    list_contains(s, probe.d(), probe.v(), probe.type, lc.d(), lc.v(), *lc.list, t->nrows, P<int64_t>(l.res.data),
                  P<uint8_t>(l.res.valid));
    return l;
}

// A string match (node `at`, stack [s, p]): an operand that is a literal stays a constant, anything else is an
// operand_column; k_strmatch.hip's pass produces the BOOL column.  A NULL literal operand: NULL without a kernel;
// two constants: a literal.
Lowered lower_str_match(capsmi_session* s, const capsmi_table* t, const capsmi_expr* prog, int at) {
    const auto span = operand_spans(prog, at);  // the string, the pattern
    const int first = span[0].first;
    for (const auto& sp : span)
        if (sp.first == sp.second && prog[sp.first].op == CAPSMI_X_NULL) return lowered_null(first);
    StrOperand opd[2];
    Column col[2];
    for (int q = 0; q < 2; ++q) {
        if (span[q].first == span[q].second && prog[span[q].first].op == CAPSMI_X_LIT) {
            opd[q].is_const = true;
            opd[q].code = prog[span[q].first].ival;
            continue;
        }
        col[q] = operand_column(s, t, prog, span[q].first, span[q].second);
        opd[q].data = col[q].d();
        opd[q].valid = col[q].v();
    }
    if (opd[0].is_const && opd[1].is_const) {
        Lowered l{first, {}, {}};
        l.ref.op = CAPSMI_X_LIT;
        l.ref.type = CAPSMI_BOOL;
        l.ref.ival = str_match_fold(s, prog[at].op, opd[0].code, opd[1].code) ? 1 : 0;
        return l;
    }
    Lowered l = lowered_column(s, first, t->nrows, "__str_match");
    str_match(s, prog[at].op, opd[0], opd[1], t->nrows, P<int64_t>(l.res.data), P<uint8_t>(l.res.valid));
    return l;
}

// size(), toInteger(), toFloat() or toBoolean() of a String (node `at`, stack [s]): k_strconv.hip's passes produce
// the column.  A NULL literal operand: NULL without a kernel; a literal: folded on the host; toBoolean of a BOOL
// is its operand.
Lowered lower_str_conv(capsmi_session* s, const capsmi_table* t, const capsmi_expr* prog, int at) {
    const int32_t op = prog[at].op;
    const int32_t type = str_conv_type(op);
    const auto span = operand_spans(prog, at)[0];
    const capsmi_expr& x = prog[span.first];
    Lowered l{span.first, {}, {}};
    l.ref.op = CAPSMI_X_NULL;
    l.ref.arg = type + 1;
    if (span.first == span.second && x.op == CAPSMI_X_NULL) return l;
    if (span.first == span.second && x.op == CAPSMI_X_LIT) {
        int64_t v = x.ival;
        if (x.type == CAPSMI_BOOL || str_conv_fold(s, op, x.ival, &v)) {
            l.ref.op = CAPSMI_X_LIT;
            l.ref.arg = 0;
            l.ref.type = type;
            l.ref.ival = v;
        }
        return l;
    }
    Column col = operand_column(s, t, prog, span.first, span.second);
    if (col.type == CAPSMI_BOOL) {  // toBoolean of a Boolean (check_program lets no other opcode through)
        l.res = std::move(col);
        return l;
    }
    l = lowered_column(s, span.first, t->nrows, "__str_conv", type);
    StrOperand o;
    o.data = col.d();
    o.valid = col.v();
    str_conv(s, op, o, t->nrows, P<int64_t>(l.res.data), P<uint8_t>(l.res.valid));
    return l;
}

// toString() or a concatenation (node `at`, stack [x] or [a, b]): k_strmake.hip's passes produce the STR column and
// grow the string store.  A NULL literal operand: NULL without a kernel or a sink call; literals are formatted here
// and stay constants, and when every operand is one the string is folded on the host (one sink call); toString of a
// String is its operand.
Lowered lower_str_make(capsmi_session* s, const capsmi_table* t, const capsmi_expr* prog, int at) {
    const bool cat = prog[at].op == CAPSMI_X_CONCAT;
    const auto span = operand_spans(prog, at);
    Lowered l{span[0].first, {}, {}};
    l.ref.op = CAPSMI_X_NULL;
    l.ref.arg = CAPSMI_STR + 1;
    for (const auto& sp : span)
        if (sp.first == sp.second && prog[sp.first].op == CAPSMI_X_NULL) return l;
    MakeOperand opd[2];
    Column col[2];
    const int nops = (int)span.size();
    int ncol = 0;
    for (int q = 0; q < nops; ++q) {
        const capsmi_expr& x = prog[span[q].first];
        if (span[q].first == span[q].second && x.op == CAPSMI_X_LIT) {
            if (!cat && x.type == CAPSMI_STR) {  // toString of a String literal
                l.ref = x;
                return l;
            }
            uint8_t buf[20];
            opd[q].is_const = true;
            if (x.type == CAPSMI_STR) opd[q].bytes = str_const_bytes(s, x.ival);
            else if (x.type == CAPSMI_BOOL) opd[q].bytes.assign((const char*)buf, strmake::format_bool(x.ival != 0, buf));
            else opd[q].bytes.assign((const char*)buf, strmake::format_long(x.ival, buf));
            continue;
        }
        col[q] = operand_column(s, t, prog, span[q].first, span[q].second);
        if (!cat && col[q].type == CAPSMI_STR) {  // toString of a String
            l.res = std::move(col[q]);
            return l;
        }
        opd[q].type = col[q].type;
        opd[q].data = col[q].d();
        opd[q].valid = col[q].v();
        ++ncol;
    }
    if (ncol == 0) {
        l.ref.op = CAPSMI_X_LIT;
        l.ref.arg = 0;
        l.ref.type = CAPSMI_STR;
        l.ref.ival = str_make_fold(s, nops > 1 ? opd[0].bytes + opd[1].bytes : opd[0].bytes);
        return l;
    }
    l = lowered_column(s, span[0].first, t->nrows, "__str_make", CAPSMI_STR);
    str_make(s, nops, opd, t->nrows, P<int64_t>(l.res.data), P<uint8_t>(l.res.valid));
    return l;
}

// evaluates prog over t's rows; returns its static type
int32_t launch_eval(capsmi_session* s, const capsmi_table* t, int32_t nn, const capsmi_expr* prog, int64_t* out,
                    uint8_t* out_valid, uint8_t* flags) {
    const int32_t type = validate_program(t, nn, prog);
    const int64_t n = t->nrows;
    if (n == 0) return type;
    for (int i = 0; i < nn; ++i) {  // the first node that runs as a pass of its own; the recursion lowers the rest
        const int32_t op = prog[i].op;
        if (op != CAPSMI_X_IN_LIST && !is_str_match(op) && !is_str_conv(op) && !is_str_make(op)) continue;
        Lowered l = (op == CAPSMI_X_IN_LIST
                         ? lower_in_list
                         : (is_str_conv(op) ? lower_str_conv : (is_str_make(op) ? lower_str_make : lower_str_match)))(s, t, prog, i);
        replace_span_and_eval(s, t, nn, prog, i, l, out, out_valid, flags);
        return type;
    }
    ColPtrs cp;
    for (int c = 0; c < kMaxCols; ++c) {
        cp.data[c] = nullptr;
        cp.valid[c] = nullptr;
        cp.type[c] = 0;
        cp.loff[c] = cp.lval[c] = nullptr;
    }
    for (size_t c = 0; c < t->cols.size() && c < (size_t)kMaxCols; ++c) {
        cp.data[c] = t->cols[c].d();
        cp.valid[c] = t->cols[c].v();
        cp.type[c] = (int8_t)t->cols[c].type;
        if (t->cols[c].list) {
            cp.loff[c] = P<int64_t>(t->cols[c].list->offsets);
            cp.lval[c] = P<int64_t>(t->cols[c].list->values);
        }
    }
    Buf dprog = dev_alloc(sizeof(capsmi_expr) * (nn > 0 ? nn : 1), s);
    if (nn > 0)
        HIP_CHECK(hipMemcpyAsync(P<void>(dprog), prog, sizeof(capsmi_expr) * nn, hipMemcpyHostToDevice, s->stream));
    int64_t g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    bool math = false;  // the instantiation with the numeric block, exactly when the program holds one of its opcodes
    uint64_t cols_read = 0;  // the timer's algorithmic bytes: each distinct column the program names once (its 8-byte
                             // words and its validity bytes, whatever the words stand for), the outputs once
    for (int i = 0; i < nn; ++i) {
        math = math || is_math_op(prog[i].op);
        if (prog[i].op == CAPSMI_X_COL) cols_read |= 1ULL << prog[i].arg;  // arg < kMaxCols = 64 (check_program)
    }
    const double bytes = (double)n * (9.0 * __builtin_popcountll(cols_read) + (out ? 8 : 0) + (out_valid ? 1 : 0) + (flags ? 1 : 0));
    KernelTimer kt(s, "expr_eval", bytes);  // counts interpreter launches (a scan whose predicate ran inline has none)
    hipLaunchKernelGGL(math ? k_eval<true> : k_eval<false>, dim3((unsigned)g), dim3(256), 0, s->stream,
                       P<capsmi_expr>(dprog), nn, cp, n, out, out_valid, flags);
    HIP_CHECK(hipGetLastError());
    return type;
}

}  // namespace

Column operand_column(capsmi_session* s, const capsmi_table* t, const capsmi_expr* prog, int lo, int hi) {
    if (lo == hi && prog[lo].op == CAPSMI_X_COL) return t->cols[prog[lo].arg];
    const int64_t n = t->nrows > 0 ? t->nrows : 1;
    Column c;
    c.data = dev_alloc(sizeof(int64_t) * n, s);
    c.valid = dev_alloc(n, s);
    c.type = launch_eval(s, t, hi - lo + 1, prog + lo, P<int64_t>(c.data), P<uint8_t>(c.valid), nullptr);
    return c;
}

void eval_expr(capsmi_session* s, const capsmi_table* t, int32_t nnodes, const capsmi_expr* prog, int64_t* out,
               uint8_t* out_valid, int32_t* out_type) {
    const int32_t type = launch_eval(s, t, nnodes, prog, out, out_valid, nullptr);
    if (out_type) *out_type = type;
}

void eval_predicate(capsmi_session* s, const capsmi_table* t, int32_t nnodes, const capsmi_expr* prog, uint8_t* flags) {
    if (nnodes == 0) {
        fill_u8(flags, 1, t->nrows, s->stream);
        return;
    }
    launch_eval(s, t, nnodes, prog, nullptr, nullptr, flags);
}

}  // namespace capsmi
