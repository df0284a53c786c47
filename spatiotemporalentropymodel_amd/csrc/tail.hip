// libstem_tail.so (include/stem_tail.h): the optimiser pass of the fused P-frame step over a table of chunk ranges, so that its tail
// can run in the order the next forward first reads the parameters (engine.StemEngine.tail_plan).  A library of its own, like
// libstem_frameio.so: libstem_hip.so exports exactly what its headers declare.  Unlike that library's, this entry point is part of a
// recorded training step: its prototype is checked against the launch tape's calling contract here (tape_contract.h,
// tape_entries_tail.inc) and stem_tail_entry_recordable() answers for its address as stem_tape_entry_recordable() does for
// libstem_hip.so's.
#include <stdarg.h>

#include <algorithm>
#include <iterator>

#include "../../include/stem_tail.h"
#include "adam_chunk.h"
#include "tape_contract.h"

// this library's own message slot (libstem_hip.so keeps its own behind stem_last_error)
static thread_local char g_err[512] = "";
void stem_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
STEM_EXPORT const char *stem_tail_last_error(void) { return g_err; }

namespace {

// adam_bmax_kernel's pass over the chunks of a table of ranges [c0, c1) only, in the table's order.  wg0[r] = first workgroup of range r (wg0[n] = the grid)
constexpr int ADAM_MAXRANGES = STEM_ADAM_MAX_RANGES;
struct AdamRangeTable {
    unsigned c0[ADAM_MAXRANGES];
    unsigned wg0[ADAM_MAXRANGES + 1];
    int n;
};
__global__ __launch_bounds__(256) void adam_bmax_ranges_kernel(float *p, float *g, float *m, float *v, size_t n, const double *sumsq,
                                                               float max_norm, float gscale, float step_size, float b1, float b2,
                                                               float inv_sqrt_bc2, float eps, int zero_g, float *bmax,
                                                               const AdamRangeTable tab)
{
    int r = 0;
    while (r + 1 < tab.n && blockIdx.x >= tab.wg0[r + 1]) ++r;
    adam_chunk_pass(p, g, m, v, n, sumsq, max_norm, gscale, step_size, b1, b2, inv_sqrt_bc2, eps, zero_g, bmax,
                    tab.c0[r] + (blockIdx.x - tab.wg0[r]));
}

#define STEM_TAPE_ENTRY(name) \
    static_assert(tape_recordable(&name), #name ": prototype outside the launch tape's calling contract (csrc/tape.hip)");
#include "tape_entries_tail.inc"
#undef STEM_TAPE_ENTRY

#define STEM_TAPE_ENTRY(name) reinterpret_cast<const void *>(&name),
const void *const kRecordable[] = {
#include "tape_entries_tail.inc"
};
#undef STEM_TAPE_ENTRY

}   // namespace

STEM_EXPORT int stem_tail_entry_recordable(void *fn)
{
    return std::find(std::begin(kRecordable), std::end(kRecordable), (const void *)fn) != std::end(kRecordable) ? 1 : 0;
}

STEM_EXPORT int stem_adam_step_bmax_ranges(float *p, float *g, float *m, float *v, size_t n, const double *sumsq, float max_norm,
                                           float gscale, float lr, float beta1, float beta2, float eps, int step, int zero_grad,
                                           float *bmax, const int *ranges, int nranges, void *stream)
{
    STEM_CHECK_ARG(p && g && m && v && bmax && step >= 1, "stem_adam_step_bmax_ranges: bad arguments");
    STEM_CHECK_ARG(nranges >= 0 && nranges <= ADAM_MAXRANGES && (ranges || nranges == 0),
                   "stem_adam_step_bmax_ranges: %d ranges (at most %d)", nranges, ADAM_MAXRANGES);
    if (n == 0) return 0;
    const size_t nchunks = cdivz(n, STEM_ADAM_CHUNK);
    AdamRangeTable tab;
    memset(&tab, 0, sizeof(tab));
    unsigned wgs = 0;
    for (int r = 0; r < nranges; ++r) {
        const int c0 = ranges[2 * r], c1 = ranges[2 * r + 1];
        STEM_CHECK_ARG(c0 >= 0 && c0 <= c1 && (size_t)c1 <= nchunks, "stem_adam_step_bmax_ranges: range %d = [%d, %d) outside the %zu chunks",
                       r, c0, c1, nchunks);
        if (c0 == c1) continue;
        tab.c0[tab.n] = (unsigned)c0;
        tab.wg0[tab.n++] = wgs;
        wgs += (unsigned)(c1 - c0);
    }
    tab.wg0[tab.n] = wgs;
    if (wgs == 0) return 0;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    hipLaunchKernelGGL(adam_bmax_ranges_kernel, dim3(wgs), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, sumsq, max_norm, gscale,
                       (float)(lr / bc1), beta1, beta2, (float)(1.0 / sqrt(bc2)), eps, zero_grad, bmax, tab);
    STEM_LAUNCH_CHECK("adam_bmax_ranges");
    return 0;
}
