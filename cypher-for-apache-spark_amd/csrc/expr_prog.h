// expr_prog.h -- what the host knows about postfix expression programs (include/capsmi.h, CAPSMI_X_*): the
// arity table, the sub-tree walk, and the one static check that also types a program.  Host-only and free of
// the HIP runtime, so tests/sanitize/expr_san.cpp runs it on the CPU; k_expr.hip, plan.hip and k_graph.hip
// use it through capsmi_impl.h.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/capsmi.h"
#include "capsmi_error.h"

namespace capsmi {

constexpr int kMaxStack = 32;  // the interpreter's value stack (k_expr.hip)
constexpr int kMaxCols = 64;   // columns a program may address

inline bool is_list_type(int32_t t) { return t >= CAPSMI_LIST_I64 && t <= CAPSMI_LIST_STR; }

// A new opcode of include/capsmi.h gets a row in expr_pops and check_program.  The numbers are not contiguous
// (32..39, 52..55, 60..63 and 66..67 are unassigned): an opcode is unknown exactly when expr_pops has no row for it (known_expr_op
// below).

// the numeric block (DIV .. TO_INTEGER): what k_expr.hip's math instantiation adds to the interpreter
constexpr bool is_math_op(int32_t op) { return op >= CAPSMI_X_DIV && op <= CAPSMI_X_TO_INTEGER; }
inline const char* math_op_name(int32_t op) {
    static const char* const names[] = {"DIV", "SQRT", "LOG", "LOG10", "EXP", "ABS", "CEIL", "FLOOR", "ROUND", "SIGN",
                                        "TO_FLOAT", "TO_INTEGER"};
    return names[op - CAPSMI_X_DIV];
}

// the functions that read a String's characters (STR_SIZE .. TO_BOOLEAN): lowered to passes of their own
// (k_strconv.hip) before the interpreter runs
constexpr bool is_str_conv(int32_t op) { return op >= CAPSMI_X_STR_SIZE && op <= CAPSMI_X_TO_BOOLEAN; }
constexpr int32_t str_conv_type(int32_t op) {  // the result's type
    return op == CAPSMI_X_STR_TO_FLOAT ? CAPSMI_F64 : (op == CAPSMI_X_TO_BOOLEAN ? CAPSMI_BOOL : CAPSMI_I64);
}

// the functions that make a String (TO_STRING, CONCAT): lowered to passes of their own (k_strmake.hip) before the
// interpreter runs; the strings get their codes from the session's string sink
constexpr bool is_str_make(int32_t op) { return op == CAPSMI_X_TO_STRING || op == CAPSMI_X_CONCAT; }

// the row's index (ROW_ID): legal only in a program of capsmi_with_columns, whose plan node it pins (plan.hip)
inline bool has_row_id(int32_t nn, const capsmi_expr* prog) {
    for (int i = 0; i < nn; ++i)
        if (prog[i].op == CAPSMI_X_ROW_ID) return true;
    return false;
}
inline void refuse_row_id(int32_t nn, const capsmi_expr* prog, const char* where) {
    REQUIRE(!has_row_id(nn, prog), CAPSMI_ERR_ILLEGAL_ARGUMENT,
            std::string("CAPSMI_X_ROW_ID in ") + where + " (the row index is legal only in a program of capsmi_with_columns)");
}

// operands an opcode pops: the one arity table (-1: unknown opcode, CAPSMI_X_PARAM included: it is bound before
// anything counts)
inline int expr_pops(const capsmi_expr& x) {
    switch (x.op) {
        case CAPSMI_X_COL: case CAPSMI_X_LIT: case CAPSMI_X_NULL: case CAPSMI_X_ROW_ID: return 0;
        case CAPSMI_X_NOT: case CAPSMI_X_ISNULL: case CAPSMI_X_ISNOTNULL: case CAPSMI_X_NEG: case CAPSMI_X_SIZE:
        case CAPSMI_X_SQRT: case CAPSMI_X_LOG: case CAPSMI_X_LOG10: case CAPSMI_X_EXP: case CAPSMI_X_ABS:
        case CAPSMI_X_CEIL: case CAPSMI_X_FLOOR: case CAPSMI_X_ROUND: case CAPSMI_X_SIGN: case CAPSMI_X_TO_FLOAT:
        case CAPSMI_X_TO_INTEGER: case CAPSMI_X_STR_SIZE: case CAPSMI_X_STR_TO_INTEGER: case CAPSMI_X_STR_TO_FLOAT:
        case CAPSMI_X_TO_BOOLEAN: case CAPSMI_X_TO_STRING: return 1;
        case CAPSMI_X_AND: case CAPSMI_X_OR: case CAPSMI_X_COALESCE: return x.arg;
        case CAPSMI_X_IN: return x.arg + 1;
        case CAPSMI_X_CASE: return 2 * x.arg + 1;
        case CAPSMI_X_EQ: case CAPSMI_X_NEQ: case CAPSMI_X_LT: case CAPSMI_X_LE: case CAPSMI_X_GT: case CAPSMI_X_GE:
        case CAPSMI_X_ADD: case CAPSMI_X_SUB: case CAPSMI_X_MUL:
        case CAPSMI_X_BITAND: case CAPSMI_X_BITOR: case CAPSMI_X_SHL: case CAPSMI_X_SHRU:
        case CAPSMI_X_INDEX: case CAPSMI_X_IN_LIST:
        case CAPSMI_X_STARTS_WITH: case CAPSMI_X_ENDS_WITH: case CAPSMI_X_CONTAINS: case CAPSMI_X_DIV:
        case CAPSMI_X_CONCAT: return 2;
        default: return -1;
    }
}

// whether expr_pops has a row for op (a negative operand count of an n-ary opcode is another matter: malformed)
inline bool known_expr_op(int32_t op) {
    capsmi_expr x{};
    x.op = op;
    x.arg = 1;
    return expr_pops(x) >= 0;
}

// first node of the complete sub-expression that ends at prog[end] (postfix)
inline int subtree_start(const capsmi_expr* prog, int end) {
    int want = 1;
    for (int i = end; i >= 0; --i) {
        const int pops = expr_pops(prog[i]);
        REQUIRE(pops >= 0, CAPSMI_ERR_NOT_IMPLEMENTED, "unknown expression op " + std::to_string(prog[i].op));
        want += pops - 1;
        if (want == 0) return i;
    }
    throw Error(CAPSMI_ERR_INTERNAL, "malformed expression program");
}

// the spans [lo, hi] of the direct operands of node `at`, first operand first
inline std::vector<std::pair<int, int>> operand_spans(const capsmi_expr* prog, int at) {
    const int pops = expr_pops(prog[at]);
    REQUIRE(pops >= 0, CAPSMI_ERR_NOT_IMPLEMENTED, "unknown expression op " + std::to_string(prog[at].op));
    std::vector<std::pair<int, int>> spans(pops);
    int end = at - 1;
    for (int k = pops - 1; k >= 0; --k) {
        spans[k] = {subtree_start(prog, end), end};
        end = spans[k].first - 1;
    }
    return spans;
}

// Static checks of a program over a schema (indices, arity, depth, the operand types of the list and string
// opcodes), and its static type: literal and column types propagate, comparisons are BOOL, an untyped result
// (a bare NULL) is reported as CAPSMI_I64.  Every stack entry carries its type (-1: unknown, an untyped NULL).
//   - A list value may only be the list operand of SIZE / INDEX / IN_LIST, or the whole program (one COL: an
//     alias).
//   - COALESCE and CASE take the type of their first typed alternative (CASE: the values, then the default).
//     An entry whose typed alternatives disagree is `mixed`, as is arithmetic over one; it is a value like any
//     other, but no operand of which one type is demanded (a string match's operands, INDEX's index, a list
//     operand): CAPSMI_ERR_ILLEGAL_ARGUMENT.
//   - The numeric block takes numbers: an operand typed BOOL or STR is CAPSMI_ERR_NOT_IMPLEMENTED; an untyped NULL
//     and a mixed entry pass (a row that holds no number yields NULL, as for ADD).
//   - STR_SIZE, STR_TO_INTEGER, STR_TO_FLOAT and TO_BOOLEAN take a String (or an untyped NULL), TO_BOOLEAN a BOOL
//     too: any other scalar type and a mixed entry are CAPSMI_ERR_ILLEGAL_ARGUMENT.
//   - ROW_ID is a Long that takes no operand and no argument.
//   - TO_STRING takes a Long, a Boolean or a String, CONCAT Strings and Longs of which at least one is a String (an
//     untyped NULL stands for either): a Double is CAPSMI_ERR_NOT_IMPLEMENTED (Java's Double.toString is not
//     restated), a Boolean in CONCAT, two Longs and a mixed entry are CAPSMI_ERR_ILLEGAL_ARGUMENT.
inline int32_t check_program(const int32_t* col_types, int ncols, int32_t nn, const capsmi_expr* prog) {
    struct Entry {
        int32_t t;
        bool mixed;
    };
    const char* const kMixed =
        "a COALESCE / CASE whose alternatives differ in type is an operand of which one type is demanded";
    std::vector<Entry> st;
    size_t maxd = 0;
    for (int i = 0; i < nn; ++i) {
        const capsmi_expr& x = prog[i];
        // the operand counts of the n-ary opcodes first: they decide what is popped
        if (x.op == CAPSMI_X_AND || x.op == CAPSMI_X_OR || x.op == CAPSMI_X_COALESCE)
            REQUIRE(x.arg >= 1, CAPSMI_ERR_ILLEGAL_ARGUMENT, "n-ary operator needs >= 1 operand");
        if (x.op == CAPSMI_X_IN) REQUIRE(x.arg >= 0, CAPSMI_ERR_ILLEGAL_ARGUMENT, "IN arity");
        if (x.op == CAPSMI_X_CASE) REQUIRE(x.arg >= 1, CAPSMI_ERR_ILLEGAL_ARGUMENT, "CASE needs >= 1 alternative");
        const int pops = expr_pops(x);
        REQUIRE(pops >= 0, CAPSMI_ERR_NOT_IMPLEMENTED, "unknown expression op " + std::to_string(x.op));
        REQUIRE((int)st.size() >= pops, CAPSMI_ERR_ILLEGAL_ARGUMENT, "malformed expression program (stack underflow)");
        const Entry* opd = st.data() + (st.size() - pops);  // the operands, first pushed first
        const bool list_op = x.op == CAPSMI_X_SIZE || x.op == CAPSMI_X_INDEX || x.op == CAPSMI_X_IN_LIST;
        const int list_at = x.op == CAPSMI_X_IN_LIST ? 1 : 0;  // which operand is the list
        for (int q = 0; q < pops; ++q)
            REQUIRE(!is_list_type(opd[q].t) || (list_op && q == list_at), CAPSMI_ERR_NOT_IMPLEMENTED,
                    "a list value as an operand of expression op " + std::to_string(x.op) +
                        " on the device path (only size(), list[i] and IN over a list column take one)");
        if (is_math_op(x.op))
            for (int q = 0; q < pops; ++q)
                REQUIRE(opd[q].mixed || (opd[q].t != CAPSMI_BOOL && opd[q].t != CAPSMI_STR), CAPSMI_ERR_NOT_IMPLEMENTED,
                        std::string(opd[q].t == CAPSMI_BOOL ? "a BOOL" : "a STR") + " operand of CAPSMI_X_" +
                            math_op_name(x.op) + " (division, the math functions, toFloat and toInteger take numbers)");
        Entry res{-1, false};
        switch (x.op) {
            case CAPSMI_X_COL:
                REQUIRE(x.arg >= 0 && x.arg < ncols, CAPSMI_ERR_ILLEGAL_ARGUMENT, "expression column index out of range");
                REQUIRE(x.arg < kMaxCols, CAPSMI_ERR_NOT_IMPLEMENTED, "expression references column >= 64");
                res.t = col_types[x.arg];
                break;
            case CAPSMI_X_LIT: res.t = x.type; break;
            case CAPSMI_X_NULL: res.t = x.arg > 0 ? x.arg - 1 : -1; break;  // arg = 1 + declared type
            case CAPSMI_X_ROW_ID:
                REQUIRE(x.arg == 0, CAPSMI_ERR_ILLEGAL_ARGUMENT, "CAPSMI_X_ROW_ID takes no argument (arg must be 0)");
                res.t = CAPSMI_I64;
                break;
            case CAPSMI_X_SIZE: case CAPSMI_X_INDEX: case CAPSMI_X_IN_LIST: {
                const int32_t l = opd[list_at].t;
                REQUIRE(!opd[list_at].mixed && (x.op != CAPSMI_X_INDEX || !opd[1].mixed), CAPSMI_ERR_ILLEGAL_ARGUMENT, kMixed);
                REQUIRE(l != CAPSMI_STR, CAPSMI_ERR_NOT_IMPLEMENTED,
                        "size() / index / IN of a string value is not implemented (string lengths live in the caller's "
                        "dictionary)");
                REQUIRE(l < 0 || is_list_type(l), CAPSMI_ERR_ILLEGAL_ARGUMENT, "the operand of a list opcode is not a list");
                // nothing but a column (or a NULL) yields a list: the node before an IN_LIST is its list operand
                REQUIRE(x.op != CAPSMI_X_IN_LIST || prog[i - 1].op == CAPSMI_X_COL || prog[i - 1].op == CAPSMI_X_NULL,
                        CAPSMI_ERR_ILLEGAL_ARGUMENT, "the list operand of IN_LIST must be a list column");
                if (x.op == CAPSMI_X_INDEX)
                    REQUIRE(opd[1].t < 0 || opd[1].t == CAPSMI_I64, CAPSMI_ERR_ILLEGAL_ARGUMENT, "a list index must be a Long");
                res.t = x.op == CAPSMI_X_SIZE ? CAPSMI_I64 : (x.op == CAPSMI_X_IN_LIST ? CAPSMI_BOOL : (l < 0 ? -1 : l - CAPSMI_LIST));
                break;
            }
            case CAPSMI_X_STARTS_WITH: case CAPSMI_X_ENDS_WITH: case CAPSMI_X_CONTAINS:
                for (int q = 0; q < 2; ++q) {
                    REQUIRE(!opd[q].mixed, CAPSMI_ERR_ILLEGAL_ARGUMENT, kMixed);
                    REQUIRE(opd[q].t < 0 || opd[q].t == CAPSMI_STR, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                            "STARTS WITH / ENDS WITH / CONTAINS take String operands (or a NULL literal that is untyped "
                            "or typed String)");
                }
                res.t = CAPSMI_BOOL;
                break;
            case CAPSMI_X_STR_SIZE: case CAPSMI_X_STR_TO_INTEGER: case CAPSMI_X_STR_TO_FLOAT: case CAPSMI_X_TO_BOOLEAN:
                REQUIRE(!opd[0].mixed, CAPSMI_ERR_ILLEGAL_ARGUMENT, kMixed);
                REQUIRE(opd[0].t < 0 || opd[0].t == CAPSMI_STR || (x.op == CAPSMI_X_TO_BOOLEAN && opd[0].t == CAPSMI_BOOL),
                        CAPSMI_ERR_ILLEGAL_ARGUMENT,
                        x.op == CAPSMI_X_TO_BOOLEAN
                            ? "toBoolean takes a String or a Boolean operand (or a NULL literal that is untyped or typed so)"
                            : "size(), toInteger() and toFloat() of a String take a String operand (or a NULL literal that "
                              "is untyped or typed String)");
                res.t = str_conv_type(x.op);
                break;
            case CAPSMI_X_TO_STRING: case CAPSMI_X_CONCAT: {
                const bool cat = x.op == CAPSMI_X_CONCAT;
                for (int q = 0; q < pops; ++q) {
                    REQUIRE(!opd[q].mixed, CAPSMI_ERR_ILLEGAL_ARGUMENT, kMixed);
                    REQUIRE(opd[q].t != CAPSMI_F64, CAPSMI_ERR_NOT_IMPLEMENTED,
                            std::string("a Double operand of ") + (cat ? "string concatenation" : "toString()") +
                                " would need Java's Double.toString, which is not restated on the device path");
                    REQUIRE(!cat || opd[q].t != CAPSMI_BOOL, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                            "string concatenation takes String and Long operands, not a Boolean");
                }
                REQUIRE(!cat || opd[0].t != CAPSMI_I64 || opd[1].t != CAPSMI_I64, CAPSMI_ERR_ILLEGAL_ARGUMENT,
                        "string concatenation needs a String operand (Long + Long is CAPSMI_X_ADD)");
                res.t = CAPSMI_STR;
                break;
            }
            case CAPSMI_X_NEG: case CAPSMI_X_ABS: res = opd[0]; break;
            case CAPSMI_X_COALESCE: case CAPSMI_X_CASE: {  // CASE: [p1, v1, .., default]; the predicates are BOOL
                const bool is_case = x.op == CAPSMI_X_CASE;
                for (int q = is_case ? 1 : 0; q < pops; q += (is_case && q < pops - 2) ? 2 : 1) {
                    res.mixed = res.mixed || opd[q].mixed || (res.t >= 0 && opd[q].t >= 0 && opd[q].t != res.t);
                    if (res.t < 0) res.t = opd[q].t;
                }
                break;
            }
            case CAPSMI_X_ADD: case CAPSMI_X_SUB: case CAPSMI_X_MUL: case CAPSMI_X_DIV:
                res.t = (opd[0].t == CAPSMI_F64 || opd[1].t == CAPSMI_F64) ? CAPSMI_F64 : CAPSMI_I64;
                res.mixed = opd[0].mixed || opd[1].mixed;
                break;
            case CAPSMI_X_BITAND: case CAPSMI_X_BITOR: case CAPSMI_X_SHL: case CAPSMI_X_SHRU:
            case CAPSMI_X_SIGN: case CAPSMI_X_TO_INTEGER: res.t = CAPSMI_I64; break;
            case CAPSMI_X_SQRT: case CAPSMI_X_LOG: case CAPSMI_X_LOG10: case CAPSMI_X_EXP: case CAPSMI_X_CEIL:
            case CAPSMI_X_FLOOR: case CAPSMI_X_ROUND: case CAPSMI_X_TO_FLOAT: res.t = CAPSMI_F64; break;
            case CAPSMI_X_EQ: case CAPSMI_X_NEQ: case CAPSMI_X_LT: case CAPSMI_X_LE: case CAPSMI_X_GT: case CAPSMI_X_GE:
            case CAPSMI_X_NOT: case CAPSMI_X_AND: case CAPSMI_X_OR: case CAPSMI_X_ISNULL: case CAPSMI_X_ISNOTNULL:
            case CAPSMI_X_IN: res.t = CAPSMI_BOOL; break;
            default: throw Error(CAPSMI_ERR_INTERNAL, "expression op " + std::to_string(x.op) + " has no type rule");
        }
        st.resize(st.size() - pops);
        st.push_back(res);
        if (st.size() > maxd) maxd = st.size();
    }
    REQUIRE(nn == 0 || st.size() == 1, CAPSMI_ERR_ILLEGAL_ARGUMENT, "expression program must leave one value");
    REQUIRE(maxd <= (size_t)kMaxStack, CAPSMI_ERR_NOT_IMPLEMENTED, "expression too deep");
    REQUIRE(nn <= 1 || !is_list_type(st[0].t), CAPSMI_ERR_NOT_IMPLEMENTED,
            "an expression that yields a list on the device path (only a column reference does)");
    return nn == 0 || st[0].t < 0 ? CAPSMI_I64 : st[0].t;
}

}  // namespace capsmi
