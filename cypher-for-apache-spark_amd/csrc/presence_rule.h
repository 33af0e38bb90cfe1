// presence_rule.h -- the endpoint presence words of a registered relationship table (PresenceWords,
// capsmi_impl.h): when a table keeps them, when a query's domain may read them, and how a word of the domain's
// bitmap is put together from them.  Host and device code alike and free of the HIP runtime:
// tests/sanitize/presence_san.cpp runs it on the CPU.
#pragma once

#include <cstdint>

#ifndef CAPSMI_HD
#if defined(__HIP__) || defined(__CUDACC__)
#define CAPSMI_HD __attribute__((host)) __attribute__((device))
#else
#define CAPSMI_HD
#endif
#endif

namespace capsmi {

// the widest window that keeps words: the widest domain on which the pool hops run (k_part.hip pool_domain)
constexpr uint64_t kPresenceMaxIds = uint64_t(1) << 26;

// [lo, hi) is the endpoints' window as EntityInfo holds it (narrow_rule.h: hi = INT64_MAX also stands for a
// maximum of INT64_MAX itself).  One bit per id of the window, so it spans at most 2^26 ids; the span is taken in
// unsigned arithmetic (lo may be negative).  No words for a table without rows or with a validity map on an
// endpoint.
CAPSMI_HD inline bool presence_eligible(bool src_has_valid, bool dst_has_valid, int64_t rows, int64_t lo, int64_t hi) {
    if (src_has_valid || dst_has_valid || rows <= 0 || hi <= lo) return false;
    const uint64_t span = (uint64_t)hi - (uint64_t)lo;
    return hi == INT64_MAX ? span < kPresenceMaxIds : span <= kPresenceMaxIds;
}

// A query over the domain [lo, hi) may read the words of a table whose window is [tlo, thi) only if the window
// lies inside the domain: pass 1 drops the rows with an endpoint outside the domain, and the words have counted
// them.
CAPSMI_HD inline bool presence_usable(int64_t tlo, int64_t thi, int64_t lo, int64_t hi) {
    return tlo >= lo && thi <= hi && tlo < thi;
}

// Word w of the domain's bitmap from a table's `nwords` words, whose bit 0 of word 0 is the domain's bit `shift`
// (shift = tlo - lo >= 0): bit j of table word k is domain bit 32 k + j + shift, so word w is a funnel of the
// table's words w - shift / 32 and the one before.  Words before the first and past the last read as zero, and
// no shift is by 32.
CAPSMI_HD inline uint32_t presence_word(const uint32_t* words, int64_t nwords, int64_t shift, int64_t w) {
    const int64_t k = w - (shift >> 5);
    const int r = (int)(shift & 31);
    const uint32_t cur = k >= 0 && k < nwords ? words[k] : 0u;
    if (r == 0) return cur;
    const uint32_t prev = k >= 1 && k - 1 < nwords ? words[k - 1] : 0u;
    return (cur << r) | (prev >> (32 - r));
}

}  // namespace capsmi
