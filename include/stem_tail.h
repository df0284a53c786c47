/* C ABI of libstem_tail.so (csrc/tail.hip): the clip + Adam pass of stem_adam_step_bmax over a table of chunk ranges, so that the fused
 * P-frame step can update -- and then pack -- the parameters in the order the next forward first reads them.  The conventions of
 * stem_hip.h, with this library's own message slot (stem_tail_last_error).  A library and a header of its own, like stem_frameio.h:
 * libstem_hip.so keeps its list of entry points.  Unlike that library's entry points this one IS part of a recorded training step:
 * csrc/tape_entries_tail.inc (tools/gen_tape_table.py, from this header) lists it, csrc/tail.hip checks its prototype against the
 * launch tape's calling contract (csrc/tape_contract.h) and answers for its address in stem_tail_entry_recordable(), as
 * stem_tape_entry_recordable() does for stem_hip.h's.  _lib.py reads the ctypes prototypes from here. */
#ifndef STEM_TAIL_H
#define STEM_TAIL_H
#include <stddef.h>
#include <stdint.h>

#define STEM_ADAM_MAX_RANGES 40      /* ranges per call */

#ifdef __cplusplus
extern "C" {
#endif

/* stem_adam_step_bmax (same arguments, same meaning) over the chunks of `nranges` ranges [ranges[2r], ranges[2r + 1]) only, in units
 * of stem_adam_chunk(), in ONE launch and in the table's order: the same element update, the same four maxima per chunk in
 * bmax[4 * chunk .. + 3], the ragged last chunk included.  Calls whose tables together hold every chunk exactly once leave what one
 * stem_adam_step_bmax call leaves, bit for bit.  `ranges` is HOST memory, read during the call (2 * nranges ints); an empty range
 * is skipped; a range outside the buffer's chunks or more than STEM_ADAM_MAX_RANGES ranges is an argument error; no chunk at all:
 * 0, nothing is launched. */
int stem_adam_step_bmax_ranges(float *p, float *g, float *m, float *v, size_t n, const double *sumsq, float max_norm, float gscale,
                               float lr, float beta1, float beta2, float eps, int step, int zero_grad, float *bmax,
                               const int *ranges, int nranges, void *stream);

/* the message of the last failing call of this library on this thread */
const char *stem_tail_last_error(void);
/* 1 if `fn` is the address of an int-returning entry point of this library whose prototype passed the compile-time check of the launch
 * tape's calling contract, 0 otherwise */
int stem_tail_entry_recordable(void *fn);

#ifdef __cplusplus
}
#endif
#endif
