// str_make.h -- the bytes that toString() and string concatenation make (include/capsmi.h, CAPSMI_X_TO_STRING and
// CAPSMI_X_CONCAT): Java's Long.toString and the words `true` / `false`, as a length and as the byte at a position,
// so that a kernel can write one output byte per slot (k_strmake.hip) and the host can fold literals.
// Host and device code alike and free of the HIP runtime: tests/sanitize/strmake_san.cpp runs it on the CPU.
// Nothing here reads memory but the small tables below; byte_of's position q must lie in [0, length).
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define CAPSMI_HD __attribute__((host)) __attribute__((device))
#else
#define CAPSMI_HD
#endif

namespace capsmi {
namespace strmake {

// |v| without the overflow at Long.MIN_VALUE
CAPSMI_HD inline uint64_t magnitude(int64_t v) { return v < 0 ? 0ULL - (uint64_t)v : (uint64_t)v; }

// 10^k for k in [0, 19], without a table in memory
CAPSMI_HD inline uint64_t pow10(int k) {
    uint64_t p = 1;
    for (int i = 0; i < k; ++i) p *= 10ULL;
    return p;
}

// decimal digits of u: 1 .. 20
CAPSMI_HD inline int digits_of(uint64_t u) {
    int n = 1;
    uint64_t p = 10;
    while (n < 20 && u >= p) {  // p = 10^n; 10^19 < 2^64, and n stops at 20 before p would overflow
        ++n;
        if (n < 20) p *= 10ULL;
    }
    return n;
}

// Long.toString(v): its length (1 .. 20: the digits and a leading '-' for a negative value; no '+', no padding)
CAPSMI_HD inline int long_length(int64_t v) { return digits_of(magnitude(v)) + (v < 0 ? 1 : 0); }

// its byte at position q of `len` = long_length(v)
CAPSMI_HD inline uint8_t long_byte(int64_t v, int len, int q) {
    if (v < 0 && q == 0) return (uint8_t)'-';
    return (uint8_t)('0' + (magnitude(v) / pow10(len - 1 - q)) % 10ULL);
}

// `true` / `false`
CAPSMI_HD inline int bool_length(bool b) { return b ? 4 : 5; }
CAPSMI_HD inline uint8_t bool_byte(bool b, int q) {
    return (uint8_t)(b ? (q == 0 ? 't' : (q == 1 ? 'r' : (q == 2 ? 'u' : 'e')))
                       : (q == 0 ? 'f' : (q == 1 ? 'a' : (q == 2 ? 'l' : (q == 3 ? 's' : 'e')))));
}

// out[0 .. long_length(v)) = Long.toString(v); returns the length (the host fold and the CPU check)
inline int format_long(int64_t v, uint8_t* out) {
    const int len = long_length(v);
    for (int q = 0; q < len; ++q) out[q] = long_byte(v, len, q);
    return len;
}
inline int format_bool(bool b, uint8_t* out) {
    const int len = bool_length(b);
    for (int q = 0; q < len; ++q) out[q] = bool_byte(b, q);
    return len;
}

}  // namespace strmake
}  // namespace capsmi
