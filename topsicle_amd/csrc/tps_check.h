// tps_check.h -- what a read-analysis call's check function hands back: the return code, and the refusal's message in *why.
// Host code without HIP: the library (topsicle_hip.hip) passes the message on to tps_last_error, the emulations (tests/emu) to theirs,
// so both sides refuse with the same code and the same words.  The check functions themselves live in the feature headers, next to
// the Args struct of their kernel.
#pragma once
#include <cstdarg>
#include <cstdio>

namespace tps {

struct Why { char msg[200] = ""; };

__attribute__((format(printf, 3, 4))) static inline int refuse(Why* why, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(why->msg, sizeof why->msg, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace tps
