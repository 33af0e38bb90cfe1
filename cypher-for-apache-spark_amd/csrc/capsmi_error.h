// capsmi_error.h -- the library's exception and REQUIRE, free of the HIP runtime so that host-only headers
// (expr_prog.h) compile and run on the CPU.
#pragma once

#include <stdexcept>
#include <string>

#include "../../include/capsmi.h"

namespace capsmi {

struct Error : std::runtime_error {
    capsmi_status code;
    Error(capsmi_status c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define REQUIRE(cond, code, msg)                      \
    do {                                              \
        if (!(cond)) throw ::capsmi::Error((code), (msg)); \
    } while (0)

}  // namespace capsmi
