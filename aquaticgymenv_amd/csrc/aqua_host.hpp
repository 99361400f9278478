// aqua_host.hpp -- the host prelude of the small libraries (policy, learner, episodes): the thread-local error text behind
// <prefix>_last_error() and the argument checks every entry point starts with.  Everything here is `static`: a library
// that includes it has an error buffer of its own.  (libaqua_hip.so keeps its own copy in aqua_hip.hip.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

static int hip_fail(hipError_t e, const char* what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return static_cast<int>(e);
}

// NaN and infinity by their bits: the libraries are built with -fno-honor-nans, which lets the compiler drop x != x
static bool is_number(double x)
{
    uint64_t bits;
    std::memcpy(&bits, &x, sizeof(bits));
    return ((bits >> 52) & 0x7FFu) != 0x7FFu;
}

static bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }
