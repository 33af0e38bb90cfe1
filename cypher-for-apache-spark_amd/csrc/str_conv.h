// str_conv.h -- what size(), toInteger(), toFloat() and toBoolean() compute from a String's bytes
// (include/capsmi.h, CAPSMI_X_STR_SIZE .. CAPSMI_X_TO_BOOLEAN): the code-point count and the three parsers.
// Host and device code alike and free of the HIP runtime: k_strconv.hip's kernels and its host fold share it, and
// tests/sanitize/strconv_san.cpp runs it on the CPU.  Every function reads p[0 .. n) and nothing else.
//
// toFloat is Java's Double.parseDouble: the grammar below, then a correctly rounded value (ties to even).
//   - Clinger's exact path: at most 19 significant digits that make a significand <= 2^53, and a decimal exponent
//     of magnitude <= 22: one IEEE multiplication or division of two exact doubles.
//   - everything else: the "simple decimal conversion" of strconv -- up to kDecDigits decimal digits that are
//     shifted by powers of two until 53 bits stand before the point; digits beyond the capacity only set a sticky
//     flag (a decision between two doubles never needs more than 768 digits).  No tables.
//   - hex floats: 64 significand bits and a sticky bit, rounded once.
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define CAPSMI_HD __attribute__((host)) __attribute__((device))
#else
#define CAPSMI_HD
#endif

namespace capsmi {
namespace strconv {

constexpr int kDecDigits = 800;
constexpr uint64_t kNaNBits = 0x7ff8000000000000ULL;  // Double.NaN, whatever sign the text carries
constexpr uint64_t kInfBits = 0x7ff0000000000000ULL;
constexpr int64_t kExpSat = 100000000000000000LL;  // an exponent's digits saturate here (10^17)

// UTF8String.numChars over well-formed UTF-8: the bytes that are not 10xxxxxx
CAPSMI_HD inline bool is_lead_byte(uint8_t b) { return (b & 0xC0) != 0x80; }

CAPSMI_HD inline int64_t count_code_points(const uint8_t* p, int64_t n) {
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i) c += is_lead_byte(p[i]) ? 1 : 0;
    return c;
}

CAPSMI_HD inline bool is_digit(uint8_t b) { return b >= '0' && b <= '9'; }

// UTF8String.toInt: [+-]?[0-9]*(\.[0-9]*)? but not "", "+" or "-"; the fraction is checked and dropped; the signed
// integer part must fit 32 bits
CAPSMI_HD inline bool to_integer(const uint8_t* p, int64_t n, int64_t* out) {
    if (n == 0) return false;
    int64_t i = 0;
    const bool neg = p[0] == '-';
    if (neg || p[0] == '+') {
        if (n == 1) return false;
        i = 1;
    }
    int64_t acc = 0;  // saturates above 2^31
    for (; i < n && p[i] != '.'; ++i) {
        if (!is_digit(p[i])) return false;
        if (acc <= 2147483648LL) acc = acc * 10 + (p[i] - '0');
    }
    for (++i; i < n; ++i)
        if (!is_digit(p[i])) return false;
    if (acc > (neg ? 2147483648LL : 2147483647LL)) return false;
    *out = neg ? -acc : acc;
    return true;
}

// StringUtils.isTrueString / isFalseString over toLowerCase: 1 TRUE, 0 FALSE, -1 neither
CAPSMI_HD inline int to_boolean(const uint8_t* p, int64_t n) {
    if (n < 1 || n > 5) return -1;
    uint8_t s[5];
    for (int i = 0; i < (int)n; ++i) s[i] = (p[i] >= 'A' && p[i] <= 'Z') ? (uint8_t)(p[i] + 32) : p[i];
    auto is = [&](const char* w, int len) {
        if (n != len) return false;
        for (int i = 0; i < len; ++i)
            if (s[i] != (uint8_t)w[i]) return false;
        return true;
    };
    if (is("t", 1) || is("true", 4) || is("y", 1) || is("yes", 3) || is("1", 1)) return 1;
    if (is("f", 1) || is("false", 5) || is("n", 1) || is("no", 2) || is("0", 1)) return 0;
    return -1;
}

// ---- the slow decimal path: 0.d[0]d[1].. x 10^dp, digits as values 0..9 ----
struct Decimal {
    int nd = 0;
    int dp = 0;
    bool trunc = false;  // nonzero digits were dropped behind d[nd - 1]
    uint8_t d[kDecDigits];
};

CAPSMI_HD inline void dec_trim(Decimal& a) {
    while (a.nd > 0 && a.d[a.nd - 1] == 0) --a.nd;
    if (a.nd == 0) a.dp = 0;
}

// a /= 2^k, 1 <= k <= 60
CAPSMI_HD inline void dec_right_shift(Decimal& a, int k) {
    int r = 0, w = 0;
    uint64_t n = 0;
    for (; (n >> k) == 0; ++r) {  // enough leading digits to cover the shift
        if (r >= a.nd) {
            if (n == 0) {
                a.nd = 0;
                a.dp = 0;
                return;
            }
            while ((n >> k) == 0) {
                n *= 10;
                ++r;
            }
            break;
        }
        n = n * 10 + a.d[r];
    }
    a.dp -= r - 1;
    const uint64_t mask = (1ULL << k) - 1;
    for (; r < a.nd; ++r) {  // pick up a digit, put down a digit
        const uint64_t dig = n >> k;
        n &= mask;
        a.d[w++] = (uint8_t)dig;
        n = n * 10 + a.d[r];
    }
    while (n > 0) {  // the digits the remainder still holds
        const uint64_t dig = n >> k;
        n &= mask;
        if (w < kDecDigits) a.d[w++] = (uint8_t)dig;
        else if (dig > 0) a.trunc = true;
        n *= 10;
    }
    a.nd = w;
    dec_trim(a);
}

// a *= 2^k, 1 <= k <= 60.  A digit times 2^k grows by at most P = floor(k log10 2) + 1 digits, so the product is
// written P places up, from the right, and a leading zero (at most one comes about) is closed afterwards.
CAPSMI_HD inline void dec_left_shift(Decimal& a, int k) {
    if (a.nd == 0) return;
    const int P = ((k * 1233) >> 12) + 1;
    uint64_t carry = 0;
    for (int r = a.nd - 1; r >= 0; --r) {  // d[r + P] was read before it is written
        const uint64_t n = ((uint64_t)a.d[r] << k) + carry;
        const uint64_t q = n / 10;
        const uint8_t rem = (uint8_t)(n - 10 * q);
        if (r + P < kDecDigits) a.d[r + P] = rem;
        else if (rem) a.trunc = true;
        carry = q;
    }
    for (int w = P - 1; w >= 0; --w) {
        const uint64_t q = carry / 10;
        a.d[w] = (uint8_t)(carry - 10 * q);
        carry = q;
    }
    a.nd = a.nd + P < kDecDigits ? a.nd + P : kDecDigits;
    a.dp += P;
    int z = 0;
    while (z < a.nd && a.d[z] == 0) ++z;
    if (z > 0) {
        for (int i = 0; i + z < a.nd; ++i) a.d[i] = a.d[i + z];
        a.nd -= z;
        a.dp -= z;
    }
    dec_trim(a);
}

// a *= 2^k for any k (negative: a right shift)
CAPSMI_HD inline void dec_shift(Decimal& a, int k) {
    for (; k > 60; k -= 60) dec_left_shift(a, 60);
    for (; k < -60; k += 60) dec_right_shift(a, 60);
    if (k > 0) dec_left_shift(a, k);
    else if (k < 0) dec_right_shift(a, -k);
}

// the integer nearest to a, ties to even (a sticky tail breaks a tie upwards); a.dp <= 20
CAPSMI_HD inline uint64_t dec_rounded_integer(const Decimal& a) {
    uint64_t n = 0;
    int i = 0;
    for (; i < a.dp && i < a.nd; ++i) n = n * 10 + a.d[i];
    for (; i < a.dp; ++i) n *= 10;
    bool up = false;
    if (a.dp >= 0 && a.dp < a.nd) {
        if (a.d[a.dp] == 5 && a.dp + 1 == a.nd) up = a.trunc || (a.dp > 0 && (a.d[a.dp - 1] & 1));
        else up = a.d[a.dp] >= 5;
    }
    return n + (up ? 1 : 0);
}

// the double nearest to a (not zero, -330 <= a.dp <= 310), as bits without the sign
CAPSMI_HD inline uint64_t dec_to_bits(Decimal& a) {
    auto step = [](int dp) { return dp >= 9 ? 27 : (dp == 0 ? 1 : (dp * 3402) >> 10); };  // 2^step < 10^dp
    int exp = 0;
    while (a.dp > 0) {  // scale into [0.5, 1)
        const int n = step(a.dp);
        dec_shift(a, -n);
        exp += n;
    }
    while (a.dp < 0 || (a.dp == 0 && a.d[0] < 5)) {
        const int n = step(-a.dp);
        dec_shift(a, n);
        exp -= n;
    }
    --exp;  // [0.5, 1) against the format's [1, 2)
    if (exp < -1022) {  // subnormal: fewer bits stand before the point
        const int n = -1022 - exp;
        dec_shift(a, -n);
        exp += n;
    }
    if (exp > 1023) return kInfBits;
    dec_shift(a, 53);
    uint64_t mant = dec_rounded_integer(a);
    if (mant == (2ULL << 52)) {  // rounding added a bit
        mant >>= 1;
        if (++exp > 1023) return kInfBits;
    }
    if ((mant & (1ULL << 52)) == 0) return mant;  // subnormal (or zero)
    return ((uint64_t)(exp + 1023) << 52) | (mant & ((1ULL << 52) - 1));
}

// [eEpP] has been read at p[i - 1]: [+-]?D+ into *e, saturating; false when no digit follows
CAPSMI_HD inline bool scan_exponent(const uint8_t* p, int64_t n, int64_t& i, int64_t* e) {
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    if (i >= n || !is_digit(p[i])) return false;
    int64_t v = 0;
    for (; i < n && is_digit(p[i]); ++i)
        if (v < kExpSat) v = v * 10 + (p[i] - '0');
    *e = neg ? -v : v;
    return true;
}

CAPSMI_HD inline int hex_value(uint8_t b) {
    if (is_digit(b)) return b - '0';
    const uint8_t l = b | 0x20;
    return l >= 'a' && l <= 'f' ? l - 'a' + 10 : -1;
}

// the hex float behind "0x" at p[i ..): H+ [.] H* or . H+, [pP][+-]?D+, [fFdD]?
CAPSMI_HD inline bool hex_to_bits(const uint8_t* p, int64_t n, int64_t i, uint64_t* bits) {
    uint64_t mant = 0;
    bool sticky = false;
    int64_t e2 = 0, ndig = 0;
    bool point = false;
    for (; i < n; ++i) {
        if (p[i] == '.' && !point) {
            point = true;
            continue;
        }
        const int h = hex_value(p[i]);
        if (h < 0) break;
        ++ndig;
        if ((mant >> 60) == 0) {
            mant = (mant << 4) | (uint64_t)h;
            if (point) e2 -= 4;
        } else {
            sticky = sticky || h != 0;
            if (!point) e2 += 4;
        }
    }
    if (ndig == 0 || i >= n || (p[i] | 0x20) != 'p') return false;
    ++i;
    int64_t pe = 0;
    if (!scan_exponent(p, n, i, &pe)) return false;
    if (i < n && ((p[i] | 0x20) == 'f' || (p[i] | 0x20) == 'd')) ++i;
    if (i != n) return false;
    if (mant == 0) {
        *bits = 0;
        return true;
    }
    int lz = 0;
    while ((mant >> 63) == 0) {
        mant <<= 1;
        ++lz;
    }
    const int64_t E = e2 + pe - lz + 63;  // the leading bit's exponent; |e2| < 2^62 and |pe| <= 10^17
    if (E > 1023) {
        *bits = kInfBits;
        return true;
    }
    if (E < -1080) {
        *bits = 0;
        return true;
    }
    const int shift = E >= -1022 ? 11 : 11 + (int)(-1022 - E);  // 11 .. 69
    if (shift > 64) {
        *bits = 0;
        return true;
    }
    const uint64_t m = shift == 64 ? 0 : mant >> shift;
    const uint64_t half = 1ULL << (shift - 1);
    const uint64_t rem = shift == 64 ? mant : mant & ((half << 1) - 1);
    const bool up = rem > half || (rem == half && (sticky || (m & 1)));
    const uint64_t biased = E >= -1022 ? (uint64_t)(E + 1022) : 0;  // m carries the implicit bit into the exponent
    *bits = (biased << 52) + m + (up ? 1 : 0);
    return true;
}

// Double.parseDouble(s): false for what throws NumberFormatException; *bits is the double's bit pattern
CAPSMI_HD inline bool to_float(const uint8_t* p, int64_t n, uint64_t* bits) {
    int64_t i = 0;
    while (i < n && p[i] <= 0x20) ++i;  // String.trim
    while (n > i && p[n - 1] <= 0x20) --n;
    if (i >= n) return false;
    uint64_t sign = 0;
    if (p[i] == '+' || p[i] == '-') sign = p[i++] == '-' ? 1ULL << 63 : 0;
    auto word = [&](const char* w, int len) {
        if (n - i != len) return false;
        for (int q = 0; q < len; ++q)
            if (p[i + q] != (uint8_t)w[q]) return false;
        return true;
    };
    if (word("NaN", 3)) {
        *bits = kNaNBits;
        return true;
    }
    if (word("Infinity", 8)) {
        *bits = sign | kInfBits;
        return true;
    }
    if (n - i >= 2 && p[i] == '0' && (p[i + 1] | 0x20) == 'x') {
        uint64_t b = 0;
        if (!hex_to_bits(p, n, i + 2, &b)) return false;
        *bits = sign | b;
        return true;
    }
    // the decimal form: up to 19 significant digits in w, the rest counted (dexp) and remembered as `inexact`
    const int64_t ms = i;
    uint64_t w = 0;
    int nd = 0;
    int64_t dexp = 0, ndig = 0;
    bool inexact = false;
    for (; i < n && is_digit(p[i]); ++i, ++ndig) {
        const uint8_t c = p[i] - '0';
        if (nd < 19) {
            w = w * 10 + c;
            if (w != 0) ++nd;
        } else {
            ++dexp;
            inexact = inexact || c != 0;
        }
    }
    if (i < n && p[i] == '.') {
        for (++i; i < n && is_digit(p[i]); ++i, ++ndig) {
            const uint8_t c = p[i] - '0';
            if (nd < 19) {
                w = w * 10 + c;
                if (w != 0) ++nd;
                --dexp;
            } else {
                inexact = inexact || c != 0;
            }
        }
    }
    if (ndig == 0) return false;
    const int64_t me = i;
    int64_t e10 = 0;
    if (i < n && (p[i] | 0x20) == 'e') {
        ++i;
        if (!scan_exponent(p, n, i, &e10)) return false;
    }
    if (i < n && ((p[i] | 0x20) == 'f' || (p[i] | 0x20) == 'd')) ++i;
    if (i != n) return false;
    if (w == 0) {
        *bits = sign;
        return true;
    }
    const int64_t e = dexp + e10;
    if (!inexact && w <= (1ULL << 53) && e >= -22 && e <= 22) {  // Clinger: two exact doubles, one rounding
        double p10 = 1.0;
        for (int q = 0; q < (e < 0 ? -e : e); ++q) p10 *= 10.0;  // exact up to 10^22
        const double v = e < 0 ? (double)w / p10 : (double)w * p10;
        uint64_t u;
        __builtin_memcpy(&u, &v, sizeof u);
        *bits = sign | u;
        return true;
    }
    Decimal a;
    int64_t dp = 0;
    bool point = false;
    for (int64_t q = ms; q < me; ++q) {
        if (p[q] == '.') {
            point = true;
            continue;
        }
        const uint8_t c = p[q] - '0';
        if (a.nd == 0 && c == 0) {  // a leading zero
            if (point) --dp;
            continue;
        }
        if (a.nd < kDecDigits) a.d[a.nd++] = c;
        else if (c != 0) a.trunc = true;
        if (!point) ++dp;
    }
    dp += e10;
    if (dp > 310) {
        *bits = sign | kInfBits;
        return true;
    }
    if (dp < -330) {
        *bits = sign;
        return true;
    }
    a.dp = (int)dp;
    dec_trim(a);
    a.dp = (int)dp;  // the digits are not all zero (w != 0), so trimming left some
    *bits = sign | dec_to_bits(a);
    return true;
}

}  // namespace strconv
}  // namespace capsmi
