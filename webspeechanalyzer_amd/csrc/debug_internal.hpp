// debug_internal.hpp — the host plumbing the test entries (debug*.hip, wsa_debug_*) share: a caller's table on its way to the device and back, and
// "the launches went in and ran".  No device code; everything is static, so the header exports nothing.
#pragma once
#include "host_plan.hpp"

namespace wsa_debug {
// the caller's `count` entries into a device table that exists (a table with slack behind it, or one refilled per step); nothing to copy is no failure
template <typename T>
static bool put(T* d, const T* h, size_t count) { return !count || hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice) == hipSuccess; }
// a device table holding the caller's `count` entries (one entry at least), and a zero-filled one
template <typename T>
static bool up(wsa::DevArena& A, T** d, const T* h, size_t count) { return A.alloc(d, count) && put(*d, h, count); }
template <typename T>
static bool zeros(wsa::DevArena& A, T** d, size_t count) { return A.alloc(d, count, true); }
// the table's way back; nothing to copy is no failure
template <typename T>
static bool down(T* h, const T* d, size_t count) { return !count || hipMemcpy(h, d, count * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess; }
// the launches went in and ran
static bool ran() { return hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess; }
}  // namespace wsa_debug
