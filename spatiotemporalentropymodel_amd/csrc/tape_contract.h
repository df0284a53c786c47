// The calling contract of the launch tape's trampolines (csrc/tape.hip), checked per entry point at COMPILE time by every library that
// offers recordable entry points: libstem_hip.so (tape.hip, tape_entries.inc) and libstem_tail.so (tail.hip, tape_entries_tail.inc).
#pragma once
#include <type_traits>

namespace {

constexpr int TAPE_MAXI = 40, TAPE_MAXF = 6;

// call_seq() calls f(a0, f0, a1, ...) through int(long long..., double...): that lands every argument where the callee reads it
// only if (1) each parameter is a scalar of the INTEGER class (integers, enums, pointers; <= 8 bytes) or of the SSE class (float,
// double) -- no struct / union / long double / vector by value, whose classification interleaves the two files --, (2) at most
// TAPE_MAXF <= 8 SSE arguments (all in xmm0-7: none on the stack, where they would interleave with the integer overflow), and
// (3) at most TAPE_MAXI integer ones (the trampoline table's size).
static_assert(TAPE_MAXF <= 8, "SSE arguments beyond xmm7 go to the stack and would interleave with the integer overflow area");
template <class T>
constexpr bool tape_int_class = (std::is_integral<T>::value || std::is_enum<T>::value || std::is_pointer<T>::value) && sizeof(T) <= 8;
template <class T>
constexpr bool tape_sse_class = std::is_same<T, float>::value || std::is_same<T, double>::value;
template <class... A>
constexpr bool tape_recordable(int (*)(A...))
{
    constexpr int ni = (0 + ... + (tape_int_class<A> ? 1 : 0)), nf = (0 + ... + (tape_sse_class<A> ? 1 : 0));
    return ni + nf == (int)sizeof...(A) && ni <= TAPE_MAXI && nf <= TAPE_MAXF;
}

}   // namespace
