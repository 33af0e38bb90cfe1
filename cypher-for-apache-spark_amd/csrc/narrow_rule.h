// narrow_rule.h -- when a registered relationship table keeps 32-bit copies of its endpoint columns
// (Column::narrow, capsmi_impl.h).  Plain C++ with no device code: the host tests compile it on its own.
#pragma once
#include <cstdint>

namespace capsmi {

// [lo, hi) is the endpoints' window as EntityInfo holds it: lo = their minimum, hi = their maximum + 1 -- but
// hi = INT64_MAX also stands for a maximum of INT64_MAX itself, whose + 1 has no int64.  A copy holds id - lo in
// 32 bits, so it needs maximum - lo <= 2^32 - 1: hi - lo <= 2^32, and one less where hi is INT64_MAX.  The
// difference is taken in unsigned arithmetic (lo may be negative; INT64_MIN .. INT64_MAX gives 2^64 - 1, not an
// overflow).  No copy for a table without rows or with a validity map on an endpoint.
inline bool narrow_eligible(bool src_has_valid, bool dst_has_valid, int64_t rows, int64_t lo, int64_t hi) {
    if (src_has_valid || dst_has_valid || rows <= 0 || hi <= lo) return false;
    const uint64_t span = (uint64_t)hi - (uint64_t)lo;
    const uint64_t limit = uint64_t(1) << 32;
    return hi == INT64_MAX ? span < limit : span <= limit;
}

}  // namespace capsmi
